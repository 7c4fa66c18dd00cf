// rpf_generic_sampled_draws.h -- the draws of a sampled pass: the statements the count kernels of routes 8
// and 11 share (rpf_generic_sampled_count.hip, rpf_generic_sampled_mask.hip).  Only they include it; device code has internal
// linkage, like rpf_generic_common.h: each TU carries its own copy.  Moving these here left the device assembly of
// sampled_count_kernel and sampled_count_block_kernel as it was (profiles/sampled_fused_parent_vs_new.txt).
#pragma once
#include "rpf_generic_common.h"

namespace rpf {
namespace generic {
namespace {

constexpr int kScTable = 512;          // room for the box - 1 thresholds (box <= 511: box*box*S <= 262144)
constexpr uint32_t kScNone = ~0u;      // a discarded draw
constexpr uint64_t kScG = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t sc_mix(uint64_t z) { // the SplitMix64 finaliser
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// #{k < n : t[k] <= u} of a non-decreasing table
__device__ __forceinline__ int sc_count_le(const uint32_t *t, int n, uint32_t u) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t[mid] <= u) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- the key of pixel (x, y) and draw q of it.  Out: the second argument of a count kernel, with the
// seed, the pass id and the row origin of the call
template <class Out>
__device__ __forceinline__ uint64_t sc_pixel_key(const Out &o, int x, int y) {
    uint64_t h = sc_mix(o.seed + kScG);
    h = sc_mix(h ^ (uint64_t)(uint32_t)o.pass_id);
    h = sc_mix(h ^ (uint64_t)((uint32_t)o.row_origin + (uint32_t)y)); // (mod 2^32)
    return sc_mix(h ^ (uint64_t)(uint32_t)x);
}
// the visiting-order index qq of draw q in the window of (x, y), kScNone for a draw that is discarded (off the image, the centre)
__device__ __forceinline__ uint32_t sc_draw(uint64_t h, int q, const uint32_t *sT, int nT, const Window &win, int x, int y, int b, int W, int H,
                                            int S) {
    const uint64_t r = sc_mix(h + (uint64_t)(q + 1) * kScG), r2 = sc_mix(r ^ kScG);
    const int xn = x + sc_count_le(sT, nT, (uint32_t)r) - b, yn = y + sc_count_le(sT, nT, (uint32_t)(r >> 32)) - b;
    const int s = (int)(((uint64_t)(uint32_t)r2 * (uint32_t)S) >> 32);
    uint32_t qq = kScNone;
    if (xn >= 0 && xn < W && yn >= 0 && yn < H && !(xn == x && yn == y)) {
        int cell = (xn - win.x0) * win.nyv + (yn - win.y0);
        if (cell > win.centre_rank) --cell; // candidate_offset's numbering skips the centre
        qq = (uint32_t)(cell * S + s);
    }
    return qq;
}

} // namespace
} // namespace generic
} // namespace rpf
