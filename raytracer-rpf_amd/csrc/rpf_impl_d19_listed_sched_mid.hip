// rpf_impl_d19_listed_sched_mid.hip -- the fused per-pixel kernels: layout d19, part 2 (mid: K 13 / 25), listed scheduled build (rpf_impl_unit.inc)
#define RPF_IMPL_DIMS 19
#define RPF_IMPL_PART 2
#define RPF_IMPL_SCHED 1
#define RPF_IMPL_LISTED 1
#include "rpf_impl_unit.inc"
