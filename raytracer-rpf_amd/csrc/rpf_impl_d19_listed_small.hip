// rpf_impl_d19_listed_small.hip -- the fused per-pixel kernels: layout d19, part 1 (small: K <= 8 and the packed kernels), listed build (rpf_impl_unit.inc)
#define RPF_IMPL_DIMS 19
#define RPF_IMPL_PART 1
#define RPF_IMPL_SCHED 0
#define RPF_IMPL_LISTED 1
#include "rpf_impl_unit.inc"
