// rpf_impl_d27_sched_mid.hip -- the fused per-pixel kernels: layout d27, part 2 (mid: K 13 / 25), scheduled build (rpf_impl_unit.inc)
#define RPF_IMPL_DIMS 27
#define RPF_IMPL_PART 2
#define RPF_IMPL_SCHED 1
#define RPF_IMPL_LISTED 0
#include "rpf_impl_unit.inc"
