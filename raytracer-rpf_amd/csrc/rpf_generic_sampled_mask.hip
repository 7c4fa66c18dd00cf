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
#include "rpf_generic_sampled_draws.h"

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

// One wave per pixel of rows [row_begin, row_end).  p.masks / p.mask_stride: the window's words; ncand <= 64 * p.mask_stride.
template <class T, bool MEMBER = false>
__global__ __launch_bounds__(256) void sampled_count_mask_kernel(PassParams p, SampledMaskOut o) {
    extern __shared__ __align__(16) unsigned char sm_lds[];
    uint32_t *sT = reinterpret_cast<uint32_t *>(sm_lds); // [kScTable]
    const int nT = p.box - 1;
    for (int k = threadIdx.x; k < nT; k += 256) sT[k] = o.table[k];
    __syncthreads(); // the only barrier: before any wave leaves
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t npix = (uint32_t)(p.row_end - p.row_begin) * (uint32_t)p.W;
    const uint32_t e = blockIdx.x * 4u + (uint32_t)wv;
    if (e >= npix) return; // wave-uniform
    const uint32_t wave_bytes = p.mask_stride * 8u + o.queue_bytes;
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(sm_lds + kScTable * 4u + (uint32_t)wv * wave_bytes); // [mask_stride]
    uint16_t *queue = reinterpret_cast<uint16_t *>(bits + p.mask_stride);                                            // [draws]
    const int W = p.W, H = p.H, S = p.S, b = p.b;
    const uint64_t HW = (uint64_t)H * W;
    const uint64_t pix = (uint64_t)p.row_begin * W + e;
    const int y = (int)(pix / (uint32_t)W), x = (int)(pix - (uint64_t)y * W);
    const int nF = p.lay.nF, colF = 5 + p.lay.nR;
    const int D = o.draws; // 1 .. kMaxResident - S (the route's condition)

    const uint64_t h = sc_pixel_key(o, x, y);
    const Window win = make_window(x, y, b, W, H, S);
    const int nw = (win.ncand + 63) >> 6; // <= p.mask_stride (the launch checks the stride against the box)

    // ---- 1, 2: the bitmap of the pixel's D draws ------------------------------------------------------
    for (int w = lane; w < nw; w += 64) bits[w] = 0ull;
    wsync();
    for (int q = lane; q < D; q += 64) {
        const uint32_t qq = sc_draw(h, q, sT, nT, win, x, y, b, W, H, S); // < ncand, or kScNone
        if (qq != kScNone) atomicOr(&bits[qq >> 6], 1ull << (qq & 63u));
    }
    wsync();
    // ---- 3: the set bits in ascending qq, at most min(D, ncand) of them ------------------------------------------------------
    int qn = 0;
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
        int at = qn + incl - cnt;
        while (m != 0ull) {
            queue[at++] = (uint16_t)(w * 64 + (__ffsll((long long)m) - 1));
            m &= m - 1ull;
        }
        qn += __shfl(incl, 63, 64);
    }
    wsync();
    // ---- 4: stage 1b's test on the distinct draws, 64 at a time (rpf.cpp:576-586) ----------------------------------------------
    int acc = 0;
    for (int kb = 0; kb < qn; kb += 64) {
        const int k = kb + lane;
        const bool live = k < qn;
        const uint32_t qq = live ? (uint32_t)queue[k] : 0u;
        const uint32_t off = live ? candidate_offset(win, W, S, (int)qq) : 0u;
        const bool pass = passes_stage1b_wave<T, MEMBER>(p, o.member, colF, nF, off, HW, pix, live);
        if (live && !pass) atomicAnd(&bits[qq >> 6], ~(1ull << (qq & 63u)));
        acc += __popcll(__ballot(pass));
    }
    wsync();
    // ---- 5: the words and N ----------------------------------------------------------------------------------------------------
    uint64_t *pm = p.masks + pix * p.mask_stride;
    for (int w = lane; w < nw; w += 64) pm[w] = bits[w];
    if (lane == 0) p.nbhd[pix] = S + acc;
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

} // namespace generic
} // namespace rpf
