// rpf_impl_d27_listed_sched_large.hip -- the fused per-pixel kernels: layout d27, part 3 (large: K 49), listed scheduled build (rpf_impl_unit.inc)
#define RPF_IMPL_DIMS 27
#define RPF_IMPL_PART 3
#define RPF_IMPL_SCHED 1
#define RPF_IMPL_LISTED 1
#include "rpf_impl_unit.inc"
