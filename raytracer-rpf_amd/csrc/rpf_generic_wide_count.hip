// rpf_generic_wide_count.hip -- the count pass of a wide pass dealt by size class (RPF_FLAG_WIDE_NBHD | RPF_FLAG_WIDE_CLASSES,
// rpf_query_route 7).  Compiled with -ffp-contract=off like every kernel TU.
//
// wide_count_kernel is generic::nbhd_count_kernel (rpf_generic_packed.hip) for windows of any size: one wave per pixel, the
// same 3-sigma test on 64 candidates at a time in the reference's visiting order (xn outer, yn inner, centre skipped), the
// same early break per 64 candidates.  What differs:
//   * members, not masks.  The plane offsets of the accepted candidates are staged per wave in LDS (at most 832 - S entries)
//     and, when the pixel ends with N <= 832, copied into a member pool: the wave reserves its N - S entries with one atomic
//     add on a cursor and records its base.  Bases depend on the order in which the atomics land, contents do not.  A pool
//     that turns out too small loses writes, never a reservation: the cursor ends at the sum of N - S whatever the capacity
//     was, the host compares the two at its read-back and repeats the launch with a pool of exactly that size.
//   * early exit.  Once more than 832 - S candidates are accepted the pixel belongs to the wide kernel, which runs its own
//     stage 1b and writes N: the walk stops and nbhd[pix] = 833 only steers the classifier.
//   * flat pixels.  N = S without a walk when some feature k of the pixel has pstd[k] * 3.0 == 0.0 and a finite pmean[k] --
//     the strict test then rejects every finite and every infinite candidate -- and no feature mean is NaN in the rows the
//     slab's windows reach (wide_nan_scan_kernel: a NaN sample makes its own pixel's mean NaN, and a NaN candidate is the one
//     kind that passes a zero-width test).  A mean of +-inf proves nothing: |inf - inf| is NaN, which never rejects.
// MEMBER (RPF_FLAG_MEMBER_TEST, route 9): the second instantiation runs passes_member_wave on the uploaded
// multiples and floors, and its flat proof asks of feature k: pstd[k] * mult[k] == 0.0, a finite mean AND floor[k] < 0 -- under
// a non-negative floor a zero-variance feature accepts its equals, so nothing is proven.  The first instantiation is the code it
// was.
// What it shares with sampled_count_kernel lives in rpf_generic_common.h: the pool (MemberPool, the first member of the kernel's
// second argument), the test of an instantiation (passes_stage1b_wave), the tail behind the cursor (publish_members) and the
// choice of the instantiation at the launch (dispatch_count_kernel).
#include "rpf_generic_common.h"

#include <algorithm>

namespace rpf {
namespace generic {
namespace {

constexpr int kWcCap = 832; // the largest class of the one-wave kernels

struct WideCountOut {
    MemberPool m;                // base: of a pixel with S < N <= 832
    const int32_t *nan_flag;     // [1] != 0: some feature mean in reach of the slab is NaN
    const double *member;        // MEMBER: mult[RPF_MAX_NDIM] | floor[RPF_MAX_NDIM]; the other instantiation does not read it
};

// *flag |= 1 when a feature mean of pixels [pix0, pix1) is NaN (stage 1a's planes, [nF][H*W])
__global__ __launch_bounds__(256) void wide_nan_scan_kernel(const double *pmean, uint64_t HW, uint64_t pix0, uint64_t pix1, int nF,
                                                            int32_t *flag) {
    bool any = false;
    for (uint64_t pix = pix0 + (uint64_t)blockIdx.x * 256u + threadIdx.x; pix < pix1; pix += (uint64_t)gridDim.x * 256u)
        for (int k = 0; k < nF; ++k) any = any || isnan(pmean[(uint64_t)k * HW + pix]);
    if (__any(any) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// One wave per pixel of rows [row_begin, row_end).
template <class T, bool MEMBER = false>
__global__ __launch_bounds__(256) void wide_count_kernel(PassParams p, WideCountOut o) {
    __shared__ uint32_t sOff[4][kWcCap];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t npix = (uint32_t)(p.row_end - p.row_begin) * (uint32_t)p.W;
    const uint32_t e = blockIdx.x * 4u + (uint32_t)wv;
    if (e >= npix) return; // wave-uniform; the kernel has no barrier
    const int W = p.W, H = p.H, S = p.S, b = p.b;
    const uint64_t HW = (uint64_t)H * W;
    const uint64_t pix = (uint64_t)p.row_begin * W + e;
    const int y = (int)(pix / (uint32_t)W), x = (int)(pix - (uint64_t)y * W);
    const int nF = p.lay.nF, colF = 5 + p.lay.nR;
    const int limit = kWcCap - S; // accepted candidates a class can still hold (S <= 832: the route's condition)
    uint32_t *mine = sOff[wv];

    // ---- the flat-pixel proof: lane k looks at features k, k + 64, ... ---------------------------------------------
    bool flat = false;
    if (*o.nan_flag == 0) {
        for (int k = lane; k < nF; k += 64) {
            const double m = p.pmean[(uint64_t)k * HW + pix];
            if constexpr (MEMBER) {
                if (p.pstd[(uint64_t)k * HW + pix] * o.member[k] == 0.0 && isfinite(m) && o.member[RPF_MAX_NDIM + k] < 0.0) flat = true;
            } else {
                if (p.pstd[(uint64_t)k * HW + pix] * 3.0 == 0.0 && isfinite(m)) flat = true;
            }
        }
        flat = __any(flat);
    }

    // ---- stage 1b's test, 64 candidates at a time (rpf.cpp:556-586) -------------------------------------------------
    const Window win = make_window(x, y, b, W, H, S);
    const int ncand = flat ? 0 : win.ncand;
    int acc = 0; // accepted so far
    for (int qb = 0; qb < ncand && acc <= limit; qb += 64) {
        const int qq = qb + lane;
        bool pass = qq < ncand;
        const uint32_t off = pass ? candidate_offset(win, W, S, qq) : 0u;
        pass = passes_stage1b_wave<T, MEMBER>(p, o.member, colF, nF, off, HW, pix, pass);
        const unsigned long long mask = __ballot(pass);
        if (pass) {
            const int at = acc + __popcll(mask & ((1ull << lane) - 1ull));
            if (at < limit) mine[at] = off;
        }
        acc += __popcll(mask);
    }
    if (acc > limit) { // the wide kernel's pixel: it recounts and writes N
        if (lane == 0) p.nbhd[pix] = kWcCap + 1;
        return;
    }
    if (lane == 0) p.nbhd[pix] = S + acc;
    if (acc == 0) return;
    publish_members(o.m, pix, mine, acc, lane);
}

} // namespace

hipError_t launch_wide_count(const PassParams &p, const MemberPool &m, int32_t *nan_flag, const double *member, hipStream_t s) {
    if (m.pool == nullptr || m.base == nullptr || m.cursor == nullptr || nan_flag == nullptr || p.nbhd == nullptr) return hipErrorInvalidValue;
    if (p.S < 1 || p.S > kWcCap || !p.lay.generic_ok()) return hipErrorInvalidValue;
    if (p.row_end <= p.row_begin) return hipSuccess;
    hipError_t e;
    if ((e = hipMemsetAsync(m.cursor, 0, sizeof(unsigned long long), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(nan_flag, 0, sizeof(int32_t), s)) != hipSuccess) return e;
    const uint64_t HW = (uint64_t)p.H * p.W;
    const uint64_t pix0 = (uint64_t)std::max(p.row_begin - p.b, 0) * p.W, pix1 = (uint64_t)std::min(p.row_end + p.b, p.H) * p.W;
    hipLaunchKernelGGL(wide_nan_scan_kernel, dim3((unsigned)std::min<uint64_t>((pix1 - pix0 + 255) / 256, 4096)), dim3(256), 0, s,
                       p.pmean, HW, pix0, pix1, p.lay.nF, nan_flag);
    const uint64_t npix = (uint64_t)(p.row_end - p.row_begin) * p.W;
    const dim3 grid((unsigned)((npix + 3) / 4));
    const WideCountOut o{m, nan_flag, member};
    dispatch_count_kernel(p, member, [&](auto plane, auto with_member) {
        hipLaunchKernelGGL((wide_count_kernel<typename decltype(plane)::type, decltype(with_member)::value>), grid, dim3(256), 0, s, p, o);
    });
    return hipGetLastError();
}

} // namespace generic
} // namespace rpf
