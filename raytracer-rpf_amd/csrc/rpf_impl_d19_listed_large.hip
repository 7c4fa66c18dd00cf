// rpf_impl_d19_listed_large.hip -- the fused per-pixel kernels: layout d19, part 3 (large: K 49), listed build (rpf_impl_unit.inc)
#define RPF_IMPL_DIMS 19
#define RPF_IMPL_PART 3
#define RPF_IMPL_SCHED 0
#define RPF_IMPL_LISTED 1
#include "rpf_impl_unit.inc"
