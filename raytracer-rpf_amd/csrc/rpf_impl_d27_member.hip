// rpf_impl_d27_member.hip -- one translation unit of the fused per-pixel kernels: layout d27 (4 random parameters, 18 features,
// __half planes), part 4, the count pass of route 10 under the membership test (see rpf_filter_impl.inc).  Compiled with -ffp-contract=off like every kernel TU.
#include "rpf_device_common.h"

namespace rpf {
namespace d27 {
namespace {
#define RPF_IMPL_NR 4
#define RPF_IMPL_NF 18
#define RPF_IMPL_PLANE_T __half
#define RPF_IMPL_PART 4
} // namespace
#include "rpf_filter_impl.inc"
} // namespace d27
} // namespace rpf
