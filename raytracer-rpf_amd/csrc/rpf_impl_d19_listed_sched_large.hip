// rpf_impl_d19_listed_sched_large.hip -- one translation unit of the fused per-pixel kernels: layout d19 (2 random parameters, 12 features, float planes),
// size-class part 3 (K 49) in its listed, scheduled build: stage 1b from the member pool, stage 3c from the entry's gains
// (RPF_FLAG_SAMPLED_LISTED with RPF_FLAG_SCHEDULE_FUSED; RPF_IMPL_LISTED and RPF_IMPL_SCHED in rpf_filter_impl.inc, DESIGN.md sections 13g and
// 15e).  Compiled with -ffp-contract=off like every kernel TU.
#include "rpf_device_common.h"

namespace rpf {
namespace d19 {
namespace listed {
// PHASE 3 / PHASE 2 of the split route: the listed parts 2 and 3 hold them (rpf_impl_d19_listed_mid.hip, rpf_impl_d19_listed_large.hip)
hipError_t impl_filter_mid_phase_listed(const PassParams &p, const LdsLayout &L, int phase, unsigned grid, hipStream_t s);
hipError_t impl_filter_large_phase_listed(const PassParams &p, const LdsLayout &L, int phase, unsigned grid, hipStream_t s);
namespace sched {
namespace {
#define RPF_IMPL_NR 2
#define RPF_IMPL_NF 12
#define RPF_IMPL_PLANE_T float
#define RPF_IMPL_PART 3
#define RPF_IMPL_SCHED 1
#define RPF_IMPL_LISTED 1
} // namespace
#include "rpf_filter_impl.inc"
} // namespace sched
} // namespace listed
} // namespace d19
} // namespace rpf
