// rpf_spike.hip -- the spike pass (RPF_FLAG_SPIKE_CLAMP): after the last filter pass, per pixel and
// channel the mean and standard deviation of the S sample colours, a sample further than t standard deviations from the mean
// on any channel replaced by the mean of the samples that passed, the removed energy summed per pixel, per row and (on the
// host, rpf_spike_delta) per frame, and handed back to every sample of the filtered rows as one constant per channel.
// All arithmetic is IEEE fp64 in the order DESIGN.md states (this TU is compiled with -ffp-contract=off like every kernel TU):
// every sum is a serial chain whose first term is its first element, `/` and sqrt are the correctly rounded ones.
//
// Four kernels:
//   spike_clamp_tile_kernel   one wavefront per tile of consecutive pixels x 3 channels, staged through LDS (S <= kSpikeTileMaxS)
//   spike_clamp_direct_kernel one thread per pixel on global memory (S > kSpikeTileMaxS): correctness only, not tuned
//   spike_row_sum_kernel      one thread per (row, channel): the x chain over the per-pixel energy plane
//   spike_add_kernel          c += delta_k over the filtered rows of the three planes, a flat 16-byte stream
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rpf_internal.h"

namespace rpf {

namespace {

// What one pixel needs: rows r[k] of S doubles (LDS or global).  Runs the chains, replaces the spikes in place, returns the
// pixel's three e_pk and its spike count n (0 < n < S: replaced; n == S: skipped, nothing written; 0: untouched).
// A pixel with a NaN standard deviation on any channel (it holds a NaN or an infinite colour) flags nothing: the comparison
// alone would let a finite channel flag a sample whose other channel holds the NaN, and the replacement would carry it into E.
__device__ __forceinline__ int spike_pixel(double *r0, double *r1, double *r2, int S, double t, double e[3]) {
    double *r[3] = {r0, r1, r2};
    const double dS = (double)S;
    double m[3], thr[3];
    bool nan_pixel = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double sum = r[k][0];
        for (int s = 1; s < S; ++s) sum = sum + r[k][s];
        m[k] = sum / dS;
        double d = r[k][0] - m[k];
        double q = d * d;
        for (int s = 1; s < S; ++s) {
            d = r[k][s] - m[k];
            q = q + d * d;
        }
        const double sd = __dsqrt_rn(q / dS);
        thr[k] = t * sd;
        nan_pixel = nan_pixel || (sd != sd);
    }
    e[0] = 0.0; e[1] = 0.0; e[2] = 0.0;
    if (nan_pixel) return 0;
    int n = 0;
    bool have = false;
    double a[3] = {0.0, 0.0, 0.0};
    for (int s = 0; s < S; ++s) {
        const double c0 = r[0][s], c1 = r[1][s], c2 = r[2][s];
        const bool spike = (fabs(c0 - m[0]) > thr[0]) || (fabs(c1 - m[1]) > thr[1]) || (fabs(c2 - m[2]) > thr[2]);
        if (spike) {
            ++n;
        } else {
            a[0] = have ? a[0] + c0 : c0;
            a[1] = have ? a[1] + c1 : c1;
            a[2] = have ? a[2] + c2 : c2;
            have = true;
        }
    }
    if (n == 0 || n == S) return n;
    const double dK = (double)(S - n);
    const double mp[3] = {a[0] / dK, a[1] / dK, a[2] / dK};
    have = false;
    for (int s = 0; s < S; ++s) {
        const double c0 = r[0][s], c1 = r[1][s], c2 = r[2][s];
        const bool spike = (fabs(c0 - m[0]) > thr[0]) || (fabs(c1 - m[1]) > thr[1]) || (fabs(c2 - m[2]) > thr[2]);
        if (!spike) continue;
        const double d0 = c0 - mp[0], d1 = c1 - mp[1], d2 = c2 - mp[2];
        e[0] = have ? e[0] + d0 : d0;
        e[1] = have ? e[1] + d1 : d1;
        e[2] = have ? e[2] + d2 : d2;
        have = true;
        r[0][s] = mp[0]; r[1][s] = mp[1]; r[2][s] = mp[2];
    }
    return n;
}

// the three counters of rpf_spike_stats (replaced samples, clamped pixels, skipped pixels): per-lane values summed over the
// wavefront, one atomic per wavefront and non-zero counter
__device__ __forceinline__ void spike_count(const unsigned v[3], unsigned long long *counts) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        unsigned x = v[i];
        for (int off = kWave / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
        if ((threadIdx.x & (kWave - 1)) == 0 && x != 0) atomicAdd(&counts[i], (unsigned long long)x);
    }
}

struct SpikeTile {
    double *colour;         // 3 planes, plane_stride doubles apart
    uint64_t plane_stride;
    uint64_t pix0, npix;    // the filtered rows: first pixel and pixel count
    int32_t S, stride, tile; // LDS row stride in doubles (odd), pixels per tile
    uint32_t magic, ntiles; // ceil(2^32 / S) (0: S == 1): e / S for e < 2^16 as one multiply; tiles of the launch
    double t;
    double *e;              // [npix][3]
    unsigned long long *counts; // [3]
};

// Moves one tile between global memory and its LDS image, all three channels.  A channel's tile is `count` = pixels * S
// contiguous doubles in global memory, and row p of the LDS image is [k][p][stride].  Each chunk goes in 16-byte accesses from
// its first 16-byte boundary on; the one double in front of that boundary and the one behind the last whole pair (planes 1 and 2
// start 8 bytes off when W*H*S is odd, a tile's first element is odd when pix * S is) go by 8-byte accesses.  Twelve 16-byte
// loads per lane are in flight before the first of them is used.
constexpr int kMoveBatch = 4;
template <bool STORE>
__device__ __forceinline__ void spike_tile_move(double *g0, uint64_t plane_stride, double *lds, uint32_t chan, uint32_t count,
                                                uint32_t S, uint32_t magic, uint32_t stride, uint32_t lane) {
    double *g[3];
    double2 *gv[3];
    uint32_t head[3], nvec[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g[k] = g0 + (uint64_t)k * plane_stride;
        head[k] = (count != 0 && (reinterpret_cast<uintptr_t>(g[k]) & 15) != 0) ? 1u : 0u;
        nvec[k] = (count - head[k]) / 2;
        gv[k] = reinterpret_cast<double2 *>(g[k] + head[k]);
    }
    auto slot = [&](int k, uint32_t e0, double *&a, double *&b) { // LDS addresses of elements e0 and e0 + 1 of channel k
        const uint32_t p0 = magic ? __umulhi(e0, magic) : e0, s0 = e0 - p0 * S;
        a = lds + k * chan + p0 * stride + s0;
        b = (s0 + 1 == S) ? lds + k * chan + (p0 + 1) * stride : a + 1;
    };
    for (uint32_t base = lane; base < count / 2; base += kMoveBatch * kWave) {
        double2 v[3][kMoveBatch];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int i = 0; i < kMoveBatch; ++i) {
                const uint32_t j = base + i * kWave;
                if (j >= nvec[k]) continue;
                if (STORE) {
                    double *a, *b;
                    slot(k, head[k] + 2 * j, a, b);
                    v[k][i] = make_double2(*a, *b);
                } else {
                    v[k][i] = gv[k][j];
                }
            }
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int i = 0; i < kMoveBatch; ++i) {
                const uint32_t j = base + i * kWave;
                if (j >= nvec[k]) continue;
                if (STORE) {
                    gv[k][j] = v[k][i];
                } else {
                    double *a, *b;
                    slot(k, head[k] + 2 * j, a, b);
                    *a = v[k][i].x; *b = v[k][i].y;
                }
            }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { // the ragged ends of channel k: lane k
        if (lane != (uint32_t)k) continue;
        if (head[k]) {
            if (STORE) g[k][0] = lds[k * chan];
            else lds[k * chan] = g[k][0];
        }
        if (count - head[k] - 2 * nvec[k]) {
            const uint32_t e0 = count - 1, p0 = magic ? __umulhi(e0, magic) : e0, s0 = e0 - p0 * S;
            if (STORE) g[k][e0] = lds[k * chan + p0 * stride + s0];
            else lds[k * chan + p0 * stride + s0] = g[k][e0];
        }
    }
}

// One wavefront per workgroup, walking the tiles blockIdx.x, blockIdx.x + gridDim.x, ...: stage the tile, one lane per pixel
// runs the chains on its LDS rows, and the tile is written back only when the wave voted that some pixel of it changed.  The
// counters are kept in registers and reach memory once per workgroup.
__global__ __launch_bounds__(kWave) void spike_clamp_tile_kernel(SpikeTile a) {
    extern __shared__ double spike_lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t S = (uint32_t)a.S, stride = (uint32_t)a.stride;
    const uint32_t chan = (uint32_t)a.tile * stride; // doubles of one channel's LDS image
    unsigned acc[3] = {0u, 0u, 0u};
    for (uint32_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const uint64_t tp0 = (uint64_t)tile * (uint32_t)a.tile;
        const uint32_t ntp = (uint32_t)(a.npix - tp0 < (uint64_t)a.tile ? a.npix - tp0 : (uint64_t)a.tile);
        double *g0 = a.colour + (a.pix0 + tp0) * S;
        spike_tile_move<false>(g0, a.plane_stride, spike_lds, chan, ntp * S, S, a.magic, stride, lane);
        __syncthreads();
        int n = 0;
        if (lane < ntp) {
            double e[3];
            double *row = spike_lds + lane * stride;
            n = spike_pixel(row, row + chan, row + 2 * chan, a.S, a.t, e);
            double *eo = a.e + (tp0 + lane) * 3;
            eo[0] = e[0]; eo[1] = e[1]; eo[2] = e[2];
        }
        const bool clamped = n > 0 && n < a.S;
        acc[0] += clamped ? (unsigned)n : 0u;
        acc[1] += clamped ? 1u : 0u;
        acc[2] += (n == a.S && n > 0) ? 1u : 0u;
        const bool changed = __ballot(clamped) != 0; // the wave's vote: an untouched tile is not written back
        __syncthreads();
        if (changed) spike_tile_move<true>(g0, a.plane_stride, spike_lds, chan, ntp * S, S, a.magic, stride, lane);
        __syncthreads(); // the next tile's staging overwrites the image
    }
    spike_count(acc, a.counts);
}

// S > kSpikeTileMaxS: the same chains on global memory, one thread per pixel.  Correctness only.
__global__ __launch_bounds__(kWave) void spike_clamp_direct_kernel(SpikeTile a) {
    const uint64_t p = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    int n = 0;
    if (p < a.npix) {
        double e[3];
        double *row = a.colour + (a.pix0 + p) * (uint64_t)a.S;
        n = spike_pixel(row, row + a.plane_stride, row + 2 * a.plane_stride, a.S, a.t, e);
        double *eo = a.e + p * 3;
        eo[0] = e[0]; eo[1] = e[1]; eo[2] = e[2];
    }
    const bool clamped = n > 0 && n < a.S;
    const unsigned v[3] = {clamped ? (unsigned)n : 0u, clamped ? 1u : 0u, (n == a.S && n > 0) ? 1u : 0u};
    spike_count(v, a.counts);
}

// R_yk = sum over x of e_(y,x),k in order x = 0 .. W-1: one thread per (row, channel), the loads of kRowBatch pixels in flight
// ahead of the chain
constexpr int kRowBatch = 32;
__global__ __launch_bounds__(kWave) void spike_row_sum_kernel(const double *e, uint32_t rows, uint32_t W, double *out) {
    const uint32_t i = blockIdx.x * kWave + threadIdx.x;
    if (i >= rows * 3) return;
    const uint32_t y = i / 3, k = i - 3 * y;
    const double *r = e + (uint64_t)y * W * 3 + k;
    double sum = r[0];
    uint32_t x = 1;
    for (; x + kRowBatch <= W; x += kRowBatch) {
        double v[kRowBatch];
#pragma unroll
        for (int j = 0; j < kRowBatch; ++j) v[j] = r[(uint64_t)(x + j) * 3];
#pragma unroll
        for (int j = 0; j < kRowBatch; ++j) sum = sum + v[j];
    }
    for (; x < W; ++x) sum = sum + r[(uint64_t)x * 3];
    out[i] = sum;
}

// c += delta_k over `count` doubles of each plane from element e0 on: blockIdx.y = channel; the body in 16-byte accesses from
// the first 16-byte boundary, the ragged ends in 8-byte ones
constexpr int kAddThreads = 256, kAddPerThread = 4;
__global__ __launch_bounds__(kAddThreads) void spike_add_kernel(double *colour, uint64_t plane_stride, uint64_t e0, uint64_t count,
                                                                 double d0, double d1, double d2) {
    const uint32_t k = blockIdx.y;
    const double delta = k == 0 ? d0 : (k == 1 ? d1 : d2);
    double *g = colour + (uint64_t)k * plane_stride + e0;
    const uint64_t head = (count != 0 && (reinterpret_cast<uintptr_t>(g) & 15) != 0) ? 1 : 0;
    const uint64_t nvec = (count - head) / 2, tail = count - head - 2 * nvec;
    double2 *gv = reinterpret_cast<double2 *>(g + head);
    const uint64_t j0 = (uint64_t)blockIdx.x * (kAddThreads * kAddPerThread) + threadIdx.x;
    double2 v[kAddPerThread];
#pragma unroll
    for (int i = 0; i < kAddPerThread; ++i) {
        const uint64_t j = j0 + (uint64_t)i * kAddThreads;
        if (j < nvec) v[i] = gv[j];
    }
#pragma unroll
    for (int i = 0; i < kAddPerThread; ++i) {
        const uint64_t j = j0 + (uint64_t)i * kAddThreads;
        if (j < nvec) gv[j] = make_double2(v[i].x + delta, v[i].y + delta);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && head) g[0] = g[0] + delta;
    if (blockIdx.x == 0 && threadIdx.x == 1 && tail) g[count - 1] = g[count - 1] + delta;
}

} // namespace

SpikeCarve spike_carve(int S) {
    SpikeCarve c{};
    if (S <= 0 || S > kSpikeTileMaxS) return c; // the direct form
    c.stride = (uint32_t)S | 1u; // odd: lanes p and p + 1 land 2 * stride dwords apart, 32 lanes on 32 different bank pairs
    c.tile = (uint32_t)kSpikeLdsBudget / (24u * c.stride);
    if (c.tile > (uint32_t)kWave) c.tile = kWave;
    c.bytes = 24u * c.stride * c.tile;
    return c;
}

hipError_t launch_spike_clamp(double *colour, int W, int H, int S, int row_begin, int row_end, double t, double *e,
                              unsigned long long *counts, hipStream_t s) {
    if (row_end <= row_begin) return hipSuccess;
    SpikeTile a{};
    a.colour = colour;
    a.plane_stride = (uint64_t)W * H * S;
    a.pix0 = (uint64_t)row_begin * W;
    a.npix = (uint64_t)(row_end - row_begin) * W;
    a.S = S; a.t = t; a.e = e; a.counts = counts;
    const SpikeCarve c = spike_carve(S);
    if (c.tile == 0) {
        hipLaunchKernelGGL(spike_clamp_direct_kernel, dim3((unsigned)((a.npix + kWave - 1) / kWave)), dim3(kWave), 0, s, a);
        return hipGetLastError();
    }
    a.stride = (int32_t)c.stride; a.tile = (int32_t)c.tile;
    a.magic = S == 1 ? 0u : 0xFFFFFFFFu / (uint32_t)S + 1u;
    a.ntiles = (uint32_t)((a.npix + c.tile - 1) / c.tile);
    // as many one-wave workgroups as the device holds at once (LDS-bound), each walking its share of the tiles
    int dev = 0, cus = 0;
    hipError_t err = hipGetDevice(&dev);
    if (err == hipSuccess) err = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (err != hipSuccess) return err;
    const uint32_t per_cu = std::max(1u, std::min(32u, (uint32_t)max_lds_per_block() / c.bytes));
    const uint32_t grid = std::min<uint32_t>(a.ntiles, (uint32_t)std::max(cus, 1) * per_cu);
    hipLaunchKernelGGL(spike_clamp_tile_kernel, dim3(grid), dim3(kWave), c.bytes, s, a);
    return hipGetLastError();
}

hipError_t launch_spike_row_sums(const double *e, int rows, int W, double *row_sums, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(spike_row_sum_kernel, dim3((unsigned)((3u * (unsigned)rows + kWave - 1) / kWave)), dim3(kWave), 0, s, e,
                       (uint32_t)rows, (uint32_t)W, row_sums);
    return hipGetLastError();
}

hipError_t launch_spike_add(double *colour, int W, int H, int S, int row_begin, int row_end, const double delta[3], hipStream_t s) {
    if (row_end <= row_begin) return hipSuccess;
    const uint64_t row = (uint64_t)W * S, count = (uint64_t)(row_end - row_begin) * row;
    const uint64_t per_block = (uint64_t)kAddThreads * kAddPerThread;
    const uint64_t blocks = (count / 2 + per_block - 1) / per_block; // nvec <= count / 2
    hipLaunchKernelGGL(spike_add_kernel, dim3((unsigned)(blocks ? blocks : 1), 3), dim3(kAddThreads), 0, s, colour, row * H,
                       (uint64_t)row_begin * row, count, delta[0], delta[1], delta[2]);
    return hipGetLastError();
}

} // namespace rpf
