// rpf_impl_d27_large.hip -- the fused per-pixel kernels: layout d27, part 3 (large: K 49), plain build (rpf_impl_unit.inc)
#define RPF_IMPL_DIMS 27
#define RPF_IMPL_PART 3
#define RPF_IMPL_SCHED 0
#define RPF_IMPL_LISTED 0
#include "rpf_impl_unit.inc"
