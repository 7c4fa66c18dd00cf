// rpf_impl_unit.inc -- what every rpf_impl_*.hip translation unit is: rpf_filter_impl.inc compiled once, inside the namespace
// of its layout and build.  The unit defines four macros and includes this file:
//     RPF_IMPL_DIMS    19: layout d19, the reference's (2 random parameters, 12 features, float planes)
//                      27: layout d27, BASELINE configs[4] (4 random parameters, 18 features, fp16 planes)
//     RPF_IMPL_PART    1 = small (K <= 8 and the packed kernels), 2 = mid (K 13 / 25), 3 = large (K 49), 4 = member (the count
//                      pass of route 10 under the membership test; plain build only)
//     RPF_IMPL_SCHED   1: the scheduled build, stage 3c from the entry's gains (RPF_FLAG_SCHEDULE_FUSED, DESIGN.md section 15e)
//     RPF_IMPL_LISTED  1: the listed build, stage 1b from the member pool (RPF_FLAG_SAMPLED_LISTED, DESIGN.md section 13g)
// The namespace is rpf::d19 | rpf::d27, then ::listed, then ::sched: kernel symbols carry it, and the entry points
// (impl_filter_small / mid / large / packed, impl_filter_mid_phase / large_phase) have the same names in each.  Compiled with
// -ffp-contract=off like every kernel TU.
#include "rpf_device_common.h"

#if RPF_IMPL_DIMS == 19
#define RPF_IMPL_LAYOUT d19
#define RPF_IMPL_NR 2
#define RPF_IMPL_NF 12
#define RPF_IMPL_PLANE_T float
#elif RPF_IMPL_DIMS == 27
#define RPF_IMPL_LAYOUT d27
#define RPF_IMPL_NR 4
#define RPF_IMPL_NF 18
#define RPF_IMPL_PLANE_T __half
#else
#error "RPF_IMPL_DIMS must be 19 or 27"
#endif

namespace rpf {
namespace RPF_IMPL_LAYOUT {
#if RPF_IMPL_LISTED
namespace listed {
#endif
#if RPF_IMPL_SCHED
// PHASE 3 / PHASE 2 of the split route have no stage 3c: parts 2 and 3 of the enclosing namespace's build hold them, and a
// scheduled unit finds them there by unqualified lookup (unscheduled_phase in rpf_filter_impl.inc)
hipError_t impl_filter_mid_phase(const PassParams &p, const LdsLayout &L, int phase, unsigned grid, hipStream_t s);
hipError_t impl_filter_large_phase(const PassParams &p, const LdsLayout &L, int phase, unsigned grid, hipStream_t s);
namespace sched {
#endif
#include "rpf_filter_impl.inc"
#if RPF_IMPL_SCHED
} // namespace sched
#endif
#if RPF_IMPL_LISTED
} // namespace listed
#endif
} // namespace RPF_IMPL_LAYOUT
} // namespace rpf
