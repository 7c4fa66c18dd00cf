// rpf_generic_sampled_mask.hip -- the count pass of a sampled pass on the compiled kernels (RPF_FLAG_SAMPLED_NBHD |
// RPF_FLAG_SAMPLED_FUSED with draws > 0, rpf_query_route 11).  Compiled with -ffp-contract=off like every
// kernel TU.
//
// sampled_count_mask_kernel leaves what route 2's count pass leaves -- N into p.nbhd and one acceptance mask per 64 candidates
// of the window into p.masks -- for the neighbourhood route 8 lists: bit qq is set exactly when candidate qq of the visiting
// order (candidate_offset) is a distinct surviving draw of the pixel's key that passes stage 1b's test.  The compiled packed,
// one-wave and four-wave kernels rebuild their member lists from such masks as they do behind nbhd_count_kernel, so the list is
// route 8's: a subsequence of the full-box list in the same order.  The draws are sampled_count_kernel's statements
// (rpf_generic_sampled_draws.h), the test is passes_stage1b_wave (rpf_generic_common.h): the 3-sigma test, or under
// RPF_FLAG_MEMBER_TEST the configured one.
//
// One wave per pixel, four per workgroup.  The route stops at box*box*S <= 65535, so a window has at most 1024 mask words
// (8 KiB): a per-wave bitmap over qq in LDS -- what section 13b rejected for the 262144-candidate windows of route 8 -- is
// affordable here, and it makes the draws distinct and ascending by construction: no enumeration sort, no bitonic sort.
//   1. the wave clears the ceil(ncand / 64) words of its bitmap;
//   2. lane q forms draw q, q + 64, ... and sets bit qq with an LDS atomic or (a discarded draw sets none);
//   3. the set bits are compacted, in ascending qq, into a queue of 16-bit qq (64 words per step: a lane counts its word, an
//      in-wave scan gives its first queue slot);
//   4. stage 1b's test runs on 64 queue entries at a time; a rejected entry clears its bit with an LDS atomic and;
//   5. the words go out with coalesced stores, word w of the pixel by lane w mod 64, and N = S + the accepted entries.
// No member pool, no cursor, no flat-pixel proof (S + D bounds N by construction).
// LDS (dynamic, sized at the launch): the threshold table (512 words), then per wave mask_stride u64 and draws u16 rounded up to
// 8 bytes: 2048 + 4 * (8 * 1024 + 2 * 3136) = 59904 bytes at the widest window and the most draws.
//
// sampled_count_list_kernel (RPF_FLAG_SAMPLED_LISTED, route 12) is steps 1 to 4 with another last step: the
// accepted plane offsets go to route 8's member pool, for the listed builds of the compiled kernels.  Same LDS; no mask buffer.
#include "rpf_generic_sampled_draws.h"

#include <algorithm>

namespace rpf {
namespace generic {
namespace {

struct SampledMaskOut {
    const uint32_t *table;       // [box - 1] Gaussian thresholds of the box (rpf_sampling_table)
    uint64_t seed;
    int32_t pass_id, row_origin, draws;
    uint32_t queue_bytes;        // of one wave's queue: 2 * draws rounded up to 8
    const double *member;        // MEMBER: mult[RPF_MAX_NDIM] | floor[RPF_MAX_NDIM]; the other instantiation does not read it
};

// the second argument of sampled_count_list_kernel (route 12): the member pool in front, as in the count
// kernels of routes 7 to 9, then what SampledMaskOut holds
struct SampledListOut {
    MemberPool m;                // base: of a pixel with N > S
    const uint32_t *table;
    uint64_t seed;
    int32_t pass_id, row_origin, draws;
    uint32_t queue_bytes;
    const double *member;
};

// One wave per pixel of rows [row_begin, row_end).  p.masks / p.mask_stride: the window's words; ncand <= 64 * p.mask_stride.
template <class T, bool MEMBER = false>
__global__ __launch_bounds__(256) void sampled_count_mask_kernel(PassParams p, SampledMaskOut o) {
    extern __shared__ __align__(16) unsigned char sm_lds[];
#include "rpf_generic_sampled_bitmap.inc"
    // ---- 5: the words and N ----------------------------------------------------------------------------------------------------
    uint64_t *pm = p.masks + pix * p.mask_stride;
    for (int w = lane; w < nw; w += 64) pm[w] = bits[w];
    if (lane == 0) p.nbhd[pix] = S + acc;
}

// The listing form (route 12): steps 1 to 4 as above -- p.mask_stride says how many words a wave's bitmap
// has, p.masks is not read -- then
//   5. N = S + the accepted entries, and for acc > 0 one cursor reservation for the pixel (publish_members' statements: a pool too
//      small loses the writes, never the reservation); the bits that are left are walked once more, in ascending qq as in step 3,
//      and the plane offset of each (candidate_offset) goes to its rank behind the reservation.
// The pool content is sampled_count_kernel's: the same draws, the same test, the same order.  Nothing is staged: the bitmap is the list.
template <class T, bool MEMBER = false>
__global__ __launch_bounds__(256) void sampled_count_list_kernel(PassParams p, SampledListOut o) {
    extern __shared__ __align__(16) unsigned char sm_lds[];
#include "rpf_generic_sampled_bitmap.inc"
    if (lane == 0) p.nbhd[pix] = S + acc;
    if (acc == 0) return; // wave-uniform
    uint32_t lo = 0u, hi = 0u;
    if (lane == 0) {
        const unsigned long long at = atomicAdd(o.m.cursor, (unsigned long long)acc);
        o.m.base[pix] = at;
        lo = (uint32_t)at; hi = (uint32_t)(at >> 32);
    }
    const uint64_t at0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)hi) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
    if (at0 + (uint64_t)acc > o.m.capacity) return; // wave-uniform: the host grows the pool and repeats the launch
    uint32_t *out = o.m.pool + at0;
    int done = 0; // ranks handed out so far: ends at acc
    for (int w0 = 0; w0 < nw; w0 += 64) {
        const int w = w0 + lane;
        unsigned long long m = w < nw ? bits[w] : 0ull;
        const int cnt = __popcll(m);
        int incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        int at = done + incl - cnt;
        while (m != 0ull) {
            out[at++] = candidate_offset(win, W, S, w * 64 + (__ffsll((long long)m) - 1));
            m &= m - 1ull;
        }
        done += __shfl(incl, 63, 64);
    }
}

} // namespace

hipError_t launch_sampled_count_mask(const PassParams &p, const SampledCountArgs &a, hipStream_t s) {
    if (a.table == nullptr || p.nbhd == nullptr || p.masks == nullptr) return hipErrorInvalidValue;
    if (p.S < 1 || a.draws < 1 || (int64_t)p.S + a.draws > kMaxResident || p.box < 1 || p.box - 1 > kScTable || !p.lay.generic_ok())
        return hipErrorInvalidValue;
    // the bitmap holds the window: every candidate index below 64 * mask_stride, every qq in 16 bits
    const int64_t window = (int64_t)(p.box * p.box - 1) * p.S;
    if (window > kMaxNbhd || (int64_t)p.mask_stride * 64 < window || p.mask_stride > 1024u) return hipErrorInvalidValue;
    if (p.row_end <= p.row_begin) return hipSuccess;
    const uint64_t npix = (uint64_t)(p.row_end - p.row_begin) * p.W;
    const uint32_t queue_bytes = ((uint32_t)a.draws * 2u + 7u) & ~7u;
    const SampledMaskOut o{a.table, a.seed, a.pass_id, a.row_origin, a.draws, queue_bytes, a.member};
    const size_t lds = (size_t)kScTable * 4 + 4 * ((size_t)p.mask_stride * 8 + queue_bytes);
    if (lds > 65536) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((npix + 3) / 4));
    dispatch_count_kernel(p, a.member, [&](auto plane, auto with_member) {
        hipLaunchKernelGGL((sampled_count_mask_kernel<typename decltype(plane)::type, decltype(with_member)::value>), grid, dim3(256), lds, s, p, o);
    });
    return hipGetLastError();
}

hipError_t launch_sampled_count_list(const PassParams &p, const SampledCountArgs &a, const MemberPool &m, hipStream_t s) {
    if (m.pool == nullptr || m.base == nullptr || m.cursor == nullptr || a.table == nullptr || p.nbhd == nullptr) return hipErrorInvalidValue;
    if (p.S < 1 || a.draws < 1 || (int64_t)p.S + a.draws > kMaxResident || p.box < 1 || p.box - 1 > kScTable || !p.lay.generic_ok())
        return hipErrorInvalidValue;
    // the bitmap holds the window: every qq in 16 bits
    const int64_t window = (int64_t)(p.box * p.box - 1) * p.S;
    if (window > kMaxNbhd) return hipErrorInvalidValue;
    if (p.row_end <= p.row_begin) return hipSuccess;
    hipError_t e;
    if ((e = hipMemsetAsync(m.cursor, 0, sizeof(unsigned long long), s)) != hipSuccess) return e;
    const uint64_t npix = (uint64_t)(p.row_end - p.row_begin) * p.W;
    const uint32_t words = (uint32_t)std::max<int64_t>(1, (window + 63) / 64); // <= 1024
    const uint32_t queue_bytes = ((uint32_t)a.draws * 2u + 7u) & ~7u;
    const SampledListOut o{m, a.table, a.seed, a.pass_id, a.row_origin, a.draws, queue_bytes, a.member};
    PassParams q = p; // the bitmap's words travel where the mask kernel has them; no mask buffer
    q.masks = nullptr; q.mask_stride = words;
    const size_t lds = (size_t)kScTable * 4 + 4 * ((size_t)words * 8 + queue_bytes);
    if (lds > 65536) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((npix + 3) / 4));
    dispatch_count_kernel(p, a.member, [&](auto plane, auto with_member) {
        hipLaunchKernelGGL((sampled_count_list_kernel<typename decltype(plane)::type, decltype(with_member)::value>), grid, dim3(256), lds, s, q, o);
    });
    return hipGetLastError();
}

} // namespace generic
} // namespace rpf
