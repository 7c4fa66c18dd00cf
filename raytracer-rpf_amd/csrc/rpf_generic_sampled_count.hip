// rpf_generic_sampled_count.hip -- the count pass of a sampled pass (RPF_FLAG_SAMPLED_NBHD with draws > 0, rpf_query_route 8;
// DESIGN.md section 13).  Compiled with -ffp-contract=off like every kernel TU.
//
// sampled_count_kernel is generic::wide_count_kernel (rpf_generic_wide_count.hip) with another source of candidates: not every
// sample of the box but the D draws of the pixel's key -- SplitMix64 words mapped through the Gaussian threshold table of the box
// to a window cell and a sample, integer arithmetic only -- made distinct and put in ascending visiting-order index qq, so that
// the listed members are a subsequence of the full-box list and depend on nothing but the key.  What stays: one wave per pixel,
// the strict 3-sigma test of passes_3sigma_wave on 64 candidates at a time (passes_stage1b_wave), the accepted plane offsets staged
// per wave in LDS and copied to the member pool behind one cursor reservation per pixel (publish_members, the tail the two kernels
// share, rpf_generic_common.h), N = S + accepted into p.nbhd, no pool entry for a pixel that accepts nothing.  What goes: the early exit (S + D <= 832 bounds N by construction) and the flat-pixel proof.
//
// Distinct and ordered: an in-wave enumeration sort.  The D indices (0xffffffff for a discarded draw) are staged in LDS in draw
// order; index i goes to position #{j : key_j < key_i, or key_j == key_i and j < i} of a second array, which makes that array a
// sorted permutation with duplicates adjacent, and the test loop skips an entry equal to its predecessor.  D * ceil(D / 64) LDS
// words read per wave, at most 10816 of them, no atomics, no dependence on the order lanes land in (measured: 16 to 25 % of a
// sampled pass; beyond S + D = 832 its D * ceil(D / 64) reads are what sampled_count_block_kernel below replaces by a bitonic sort).
// A bitmap over qq would need box*box*S bits per wave (32 KiB at the widest window): one wave per workgroup at 64 KiB, against
// four here.
// LDS per workgroup: 4 waves * 2 arrays * 832 words + the threshold table (512 words) = 28672 bytes, whatever the window.
//
// sampled_count_block_kernel is the same count pass for 832 < S + D <= RPF_SAMPLED_MAX (RPF_FLAG_SAMPLED_REST):
// one workgroup of 256 threads per pixel, the keys -- sc_pixel_key and sc_draw, the statements of the kernel above -- padded with
// 0xffffffff to P, the next power of two (at least 256), and put in ascending order by a bitonic sort over the workgroup: log2 P
// (log2 P + 1) / 2 steps of P / 512 compare-exchanges per thread.  The keys are plain words, so the sorted array is the one the
// enumeration sort leaves: duplicates adjacent, discards last, the member list a function of the key alone.  Stage 1b's test runs
// on 256 entries at a time, a wave on its 64 (passes_stage1b_wave), the accepted offsets compacted over the array's own front:
// an entry is written at or below the index it was read from, behind a barrier that follows every read of the step, and the last
// key of a step is handed to the next in a register, since the slot it stood in may have been written.  One cursor reservation per
// pixel (publish_members_block).  LDS: P words + the threshold table + six words, 34840 bytes at P = 8192 (dynamic, sized at launch).
#include "rpf_generic_sampled_draws.h"

#include <algorithm>

namespace rpf {
namespace generic {
namespace {

constexpr int kScCap = 832;            // the largest class of the one-wave kernels: S + D <= kScCap
// (kScTable, kScNone, sc_mix, sc_count_le, sc_pixel_key and sc_draw: rpf_generic_sampled_draws.h, shared with route 11's count kernel)

struct SampledCountOut {
    MemberPool m;                // base: of a pixel with N > S
    const uint32_t *table;       // [box - 1] Gaussian thresholds of the box (rpf_sampling_table)
    uint64_t seed;
    int32_t pass_id, row_origin, draws;
    const double *member;        // MEMBER: mult[RPF_MAX_NDIM] | floor[RPF_MAX_NDIM]; the other instantiation does not read it
};

// One wave per pixel of rows [row_begin, row_end).  MEMBER (with RPF_FLAG_MEMBER_TEST): the draws meet
// passes_member_wave instead of the 3-sigma test, and nothing else differs; the first instantiation is the code it was.
template <class T, bool MEMBER = false>
__global__ __launch_bounds__(256) void sampled_count_kernel(PassParams p, SampledCountOut o) {
    __shared__ uint32_t sKey[4][kScCap];  // the draws' qq in draw order; later the accepted plane offsets
    __shared__ uint32_t sSort[4][kScCap]; // ... in ascending order, duplicates adjacent
    __shared__ uint32_t sT[kScTable];
    const int nT = p.box - 1;
    for (int k = threadIdx.x; k < nT; k += 256) sT[k] = o.table[k];
    __syncthreads(); // the only barrier: before any wave leaves
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t npix = (uint32_t)(p.row_end - p.row_begin) * (uint32_t)p.W;
    const uint32_t e = blockIdx.x * 4u + (uint32_t)wv;
    if (e >= npix) return; // wave-uniform
    const int W = p.W, H = p.H, S = p.S, b = p.b;
    const uint64_t HW = (uint64_t)H * W;
    const uint64_t pix = (uint64_t)p.row_begin * W + e;
    const int y = (int)(pix / (uint32_t)W), x = (int)(pix - (uint64_t)y * W);
    const int nF = p.lay.nF, colF = 5 + p.lay.nR;
    const int D = o.draws; // 1 .. kScCap - S (the route's condition)
    uint32_t *key = sKey[wv], *srt = sSort[wv];

    // ---- the pixel key and its D draws ---------------------------------------------------------
    const uint64_t h = sc_pixel_key(o, x, y);
    const Window win = make_window(x, y, b, W, H, S);
    for (int q = lane; q < D; q += 64) key[q] = sc_draw(h, q, sT, nT, win, x, y, b, W, H, S);
    wsync();
    // ---- enumeration sort: ties by draw order, so the ranks are a permutation of 0 .. D - 1 ---------------------------
    for (int i0 = 0; i0 < D; i0 += 64) {
        const int i = i0 + lane;
        const uint32_t ki = i < D ? key[i] : kScNone;
        int rank = 0;
        for (int j = 0; j < D; ++j) {
            const uint32_t kj = key[j]; // the same word in every lane
            rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
        }
        if (i < D) srt[rank] = ki;
    }
    wsync(); // key[] is dead from here: it takes the accepted offsets

    // ---- stage 1b's test on the distinct draws in ascending qq, 64 at a time (rpf.cpp:576-586) -------------------------
    int acc = 0;
    for (int kb = 0; kb < D; kb += 64) {
        const int k = kb + lane;
        const uint32_t qq = k < D ? srt[k] : kScNone;
        bool pass = qq != kScNone && (k == 0 || srt[k - 1] != qq);
        if (!__any(qq != kScNone)) break; // only discarded draws from here on
        const uint32_t off = pass ? candidate_offset(win, W, S, (int)qq) : 0u;
        pass = passes_stage1b_wave<T, MEMBER>(p, o.member, colF, nF, off, HW, pix, pass);
        const unsigned long long mask = __ballot(pass);
        if (pass) key[acc + __popcll(mask & ((1ull << lane) - 1ull))] = off;
        acc += __popcll(mask);
    }
    if (lane == 0) p.nbhd[pix] = S + acc;
    if (acc == 0) return;
    publish_members(o.m, pix, key, acc, lane);
}

// One workgroup per pixel of rows [row_begin, row_end), 832 < S + D <= RPF_SAMPLED_MAX.  P: a power of two, >= 256 and >= D; the
// dynamic LDS holds P + kScTable + 6 words.  MEMBER as above.
template <class T, bool MEMBER = false>
__global__ __launch_bounds__(256) void sampled_count_block_kernel(PassParams p, SampledCountOut o, int P) {
    extern __shared__ __align__(16) uint32_t sc_lds[];
    uint32_t *srt = sc_lds;                      // [P] the keys, then sorted; its front takes the accepted plane offsets
    uint32_t *sT = srt + P;                      // [kScTable]
    int *sCnt = reinterpret_cast<int *>(sT + kScTable);                                     // [4] accepted per wave of a step
    unsigned long long *sAt = reinterpret_cast<unsigned long long *>(sT + kScTable + 4);    // the pixel's pool reservation
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nT = p.box - 1;
    for (int k = tid; k < nT; k += 256) sT[k] = o.table[k];
    const int W = p.W, H = p.H, S = p.S, b = p.b;
    const uint64_t HW = (uint64_t)H * W;
    const uint64_t pix = (uint64_t)p.row_begin * W + blockIdx.x; // (the grid is the slab's pixels)
    const int y = (int)(pix / (uint32_t)W), x = (int)(pix - (uint64_t)y * W);
    const int nF = p.lay.nF, colF = 5 + p.lay.nR;
    const int D = o.draws; // 1 .. min(P, RPF_SAMPLED_MAX - S) (the route's condition)
    __syncthreads();

    // ---- the pixel key and its D draws, padded to P ------------------------------------------------------------------------
    const uint64_t h = sc_pixel_key(o, x, y);
    const Window win = make_window(x, y, b, W, H, S);
    for (int q = tid; q < P; q += 256) srt[q] = q < D ? sc_draw(h, q, sT, nT, win, x, y, b, W, H, S) : kScNone;
    __syncthreads();
    // ---- bitonic sort, ascending: step (k, j) orders the pairs (i, i | j), i without bit j, upwards where i has bit k clear -----
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint32_t a = srt[i], c = srt[l];
                if ((a > c) == ((i & k) == 0)) { srt[i] = c; srt[l] = a; }
            }
            __syncthreads();
        }
    }

    // ---- stage 1b's test on the distinct draws in ascending qq, 256 at a time (rpf.cpp:576-586) ------------------------------
    int acc = 0;
    uint32_t carry = kScNone; // the key in front of this step's first
    for (int kb = 0; kb < P; kb += 256) {
        if (srt[kb] == kScNone) break; // only discarded draws and padding from here on (workgroup-uniform: one word, never written)
        const int k = kb + tid;
        const uint32_t qq = srt[k], prev = tid == 0 ? carry : srt[k - 1];
        carry = srt[kb + 255];
        __syncthreads(); // every read of this step is done (and the last step's sCnt): the front of srt may be written
        bool pass = qq != kScNone && qq != prev;
        const uint32_t off = pass ? candidate_offset(win, W, S, (int)qq) : 0u;
        pass = passes_stage1b_wave<T, MEMBER>(p, o.member, colF, nF, off, HW, pix, pass);
        const unsigned long long mask = __ballot(pass);
        if (lane == 0) sCnt[wv] = __popcll(mask);
        __syncthreads();
        int at = acc;
        for (int w = 0; w < wv; ++w) at += sCnt[w];
        if (pass) srt[at + __popcll(mask & ((1ull << lane) - 1ull))] = off; // at most k: acc <= kb
        acc += sCnt[0] + sCnt[1] + sCnt[2] + sCnt[3];
    }
    if (tid == 0) p.nbhd[pix] = S + acc;
    if (acc == 0) return; // workgroup-uniform
    publish_members_block(o.m, pix, srt, acc, sAt);
}

} // namespace

hipError_t launch_sampled_count(const PassParams &p, const SampledCountArgs &a, const MemberPool &m, hipStream_t s) {
    if (m.pool == nullptr || m.base == nullptr || m.cursor == nullptr || a.table == nullptr || p.nbhd == nullptr) return hipErrorInvalidValue;
    if (p.S < 1 || a.draws < 1 || (int64_t)p.S + a.draws > RPF_SAMPLED_MAX || p.box - 1 > kScTable || !p.lay.generic_ok()) return hipErrorInvalidValue;
    if (p.row_end <= p.row_begin) return hipSuccess;
    hipError_t e;
    if ((e = hipMemsetAsync(m.cursor, 0, sizeof(unsigned long long), s)) != hipSuccess) return e;
    const uint64_t npix = (uint64_t)(p.row_end - p.row_begin) * p.W;
    const SampledCountOut o{m, a.table, a.seed, a.pass_id, a.row_origin, a.draws, a.member};
    if (p.S + a.draws > kScCap) { // the block kernel: a workgroup per pixel, the keys padded to the next power of two
        int P = 256;
        while (P < a.draws) P <<= 1;
        const size_t lds = (size_t)(P + kScTable + 6) * sizeof(uint32_t);
        dispatch_count_kernel(p, a.member, [&](auto plane, auto with_member) {
            hipLaunchKernelGGL((sampled_count_block_kernel<typename decltype(plane)::type, decltype(with_member)::value>), dim3((unsigned)npix),
                               dim3(256), lds, s, p, o, P);
        });
        return hipGetLastError();
    }
    const dim3 grid((unsigned)((npix + 3) / 4));
    dispatch_count_kernel(p, a.member, [&](auto plane, auto with_member) {
        hipLaunchKernelGGL((sampled_count_kernel<typename decltype(plane)::type, decltype(with_member)::value>), grid, dim3(256), 0, s, p, o);
    });
    return hipGetLastError();
}

} // namespace generic
} // namespace rpf
