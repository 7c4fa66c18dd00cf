// rpf_impl_d19_sched_mid.hip -- one translation unit of the fused per-pixel kernels: layout d19 (2 random parameters, 12 features, float planes),
// size-class part 2 (K 13 / 25) in its scheduled build: stage 3c from the entry's gains (RPF_FLAG_SCHEDULE_FUSED; RPF_IMPL_SCHED in
// rpf_filter_impl.inc).  Compiled with -ffp-contract=off like every kernel TU.
#include "rpf_device_common.h"

namespace rpf {
namespace d19 {
// PHASE 3 / PHASE 2 of the split route: the unscheduled parts 2 and 3 hold them (rpf_impl_d19_mid.hip, rpf_impl_d19_large.hip)
hipError_t impl_filter_mid_phase(const PassParams &p, const LdsLayout &L, int phase, unsigned grid, hipStream_t s);
hipError_t impl_filter_large_phase(const PassParams &p, const LdsLayout &L, int phase, unsigned grid, hipStream_t s);
namespace sched {
namespace {
#define RPF_IMPL_NR 2
#define RPF_IMPL_NF 12
#define RPF_IMPL_PLANE_T float
#define RPF_IMPL_PART 2
#define RPF_IMPL_SCHED 1
} // namespace
#include "rpf_filter_impl.inc"
} // namespace sched
} // namespace d19
} // namespace rpf
