// rpf_impl_d27_listed_large.hip -- one translation unit of the fused per-pixel kernels: layout d27 (4 random parameters, 18 features, fp16 planes),
// size-class part 3 (K 49) in its listed build: stage 1b from the member pool (RPF_FLAG_SAMPLED_LISTED; RPF_IMPL_LISTED in
// rpf_filter_impl.inc).  Compiled with -ffp-contract=off like every kernel TU.
#include "rpf_device_common.h"

namespace rpf {
namespace d27 {
namespace listed {
namespace {
#define RPF_IMPL_NR 4
#define RPF_IMPL_NF 18
#define RPF_IMPL_PLANE_T __half
#define RPF_IMPL_PART 3
#define RPF_IMPL_LISTED 1
} // namespace
#include "rpf_filter_impl.inc"
} // namespace listed
} // namespace d27
} // namespace rpf
