// rpf_report.hip -- the per-pass activity report (RPF_FLAG_PASS_REPORT): what one pass did to the filtered
// rows, reduced on the device from the pass's input colours a, its output colours b, N, alpha, beta and W_r_c into one
// rpf_report_row per row.  All arithmetic is IEEE fp64 in the order DESIGN.md states (this TU is compiled with -ffp-contract=off
// like every kernel TU): every sum is a serial chain whose first term is its first element.  Counts are integers, their order is free.
//
// Three kernels:
//   report_pixel_tile_kernel    one wavefront per tile of consecutive pixels, both colour buffers staged through LDS
//                               (S <= kReportTileMaxS); a lane per pixel runs the s chains: twelve doubles per pixel into the
//                               scratch plane, the three sample / pixel counts into the row records (one atomic per wave and row)
//   report_pixel_direct_kernel  one thread per pixel on global memory (S > kReportTileMaxS): correctness only, not tuned
//   report_row_kernel           one wavefront per row: lane q < 56 runs the x chain of double q of the record (the twelve pixel
//                               values, alpha, W_r_c, beta), all lanes share the row's N for the integer fields
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "rpf_internal.h"

namespace rpf {

namespace {

// the doubles of a record in the order lane q of report_row_kernel writes them, and the three counts the pixel kernels add to
static_assert(offsetof(rpf_report_row, moved2) == 0 && offsetof(rpf_report_row, in2) == 24 && offsetof(rpf_report_row, pix_moved2) == 48 &&
                  offsetof(rpf_report_row, pix_in2) == 72 && offsetof(rpf_report_row, alpha_sum) == 96 && offsetof(rpf_report_row, wrc_sum) == 120 &&
                  offsetof(rpf_report_row, beta_sum) == 128 && offsetof(rpf_report_row, sum_nbhd) == 128 + 8 * RPF_MAX_NDIM,
              "report_row_kernel: double q of the record");
constexpr int kRowAlpha = 12, kRowWrc = 15, kRowBeta = 16, kRowDoubles = kRowBeta + RPF_MAX_NDIM;
static_assert(kRowDoubles <= kWave, "one lane per double of the record");

__device__ __forceinline__ bool finite64(double v) {
    return ((unsigned long long)__double_as_longlong(v) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}

// What one pixel needs: rows a[k], b[k] of S doubles (LDS or global).  out[12] = m_k | i_k | pm_k | pi_k (+0.0 for a bad pixel);
// returns the pixel's unchanged samples and its samples that hold a non-finite value (> 0: the pixel is bad).
__device__ __forceinline__ void report_pixel(const double *const a[3], const double *const b[3], int S, double out[kReportPixelValues],
                                             unsigned &unchanged, unsigned &nonfinite) {
    double m[3], i2[3], pa[3], pb[3];
    unsigned unch = 0, bad = 0;
    {
        bool same = true, fin = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double av = a[k][0], bv = b[k][0], d = bv - av;
            m[k] = d * d; i2[k] = av * av; pa[k] = av; pb[k] = bv;
            same = same && __double_as_longlong(av) == __double_as_longlong(bv);
            fin = fin && finite64(av) && finite64(bv);
        }
        unch += same ? 1u : 0u; bad += fin ? 0u : 1u;
    }
    for (int s = 1; s < S; ++s) {
        bool same = true, fin = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double av = a[k][s], bv = b[k][s], d = bv - av;
            m[k] = m[k] + d * d; i2[k] = i2[k] + av * av; pa[k] = pa[k] + av; pb[k] = pb[k] + bv;
            same = same && __double_as_longlong(av) == __double_as_longlong(bv);
            fin = fin && finite64(av) && finite64(bv);
        }
        unch += same ? 1u : 0u; bad += fin ? 0u : 1u;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double dp = pb[k] - pa[k];
        out[k] = bad ? 0.0 : m[k];
        out[3 + k] = bad ? 0.0 : i2[k];
        out[6 + k] = bad ? 0.0 : dp * dp;
        out[9 + k] = bad ? 0.0 : pa[k] * pa[k];
    }
    unchanged = unch; nonfinite = bad;
}

// The three counts of the pixel kernels -- unchanged samples, non-finite samples, bad pixels -- per lane, for row `row` of the
// slab: summed over the lanes of the wavefront that hold the same row, one atomic per wavefront, row and non-zero count.  Every
// lane of the wavefront calls it (active: the lane holds a pixel).
__device__ __forceinline__ void report_row_counts(uint32_t row, bool active, const unsigned v[3], rpf_report_row *rows) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t r = (uint32_t)__shfl((int)row, leader, kWave);
        const bool mine = active && row == r;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            unsigned x = mine ? v[i] : 0u;
            for (int off = kWave / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
            if (lane == (uint32_t)leader && x != 0) {
                int64_t *dst = i == 0 ? &rows[r].unchanged_samples : (i == 1 ? &rows[r].nonfinite_samples : &rows[r].nonfinite_pixels);
                atomicAdd(reinterpret_cast<unsigned long long *>(dst), (unsigned long long)x);
            }
        }
        todo &= ~__ballot(mine);
    }
}

struct ReportTile {
    const double *a, *b;     // 3 planes each, plane_stride doubles apart
    uint64_t plane_stride;
    uint64_t pix0, npix;     // the filtered rows: first pixel and pixel count
    int32_t S, W, stride, tile; // LDS row stride in doubles (odd), pixels per tile
    uint32_t magic, ntiles;  // ceil(2^32 / S) (0: S == 1): e / S for e < 2^16 as one multiply; tiles of the launch
    double *pix;             // [npix][kReportPixelValues]
    rpf_report_row *rows;    // [npix / W]
};

// Stages one tile of the six planes (a0 a1 a2 b0 b1 b2) into its LDS image [6][tile][stride]: a plane's tile is `count` =
// pixels * S contiguous doubles, read lane-contiguous in 8-byte accesses, kStageBatch loads per plane in flight per lane.
constexpr int kStageBatch = 4;
__device__ __forceinline__ void report_tile_stage(const ReportTile &t, uint64_t e0, double *lds, uint32_t chan, uint32_t count, uint32_t lane) {
    const uint32_t S = (uint32_t)t.S, stride = (uint32_t)t.stride;
    const double *g[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) g[q] = (q < 3 ? t.a : t.b) + (uint64_t)(q % 3) * t.plane_stride + e0;
    for (uint32_t base = lane; base < count; base += kStageBatch * kWave) {
        double v[6][kStageBatch];
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
            for (int i = 0; i < kStageBatch; ++i) {
                const uint32_t j = base + i * kWave;
                if (j < count) v[q][i] = g[q][j];
            }
#pragma unroll
        for (int i = 0; i < kStageBatch; ++i) {
            const uint32_t j = base + i * kWave;
            if (j >= count) continue;
            const uint32_t p = t.magic ? __umulhi(j, t.magic) : j, s = j - p * S;
#pragma unroll
            for (int q = 0; q < 6; ++q) lds[q * chan + p * stride + s] = v[q][i];
        }
    }
}

// One wavefront per workgroup, walking the tiles blockIdx.x, blockIdx.x + gridDim.x, ...
__global__ __launch_bounds__(kWave) void report_pixel_tile_kernel(ReportTile t) {
    extern __shared__ double report_lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t chan = (uint32_t)t.tile * (uint32_t)t.stride; // doubles of one plane's LDS image
    for (uint32_t tile = blockIdx.x; tile < t.ntiles; tile += gridDim.x) {
        const uint64_t tp0 = (uint64_t)tile * (uint32_t)t.tile;
        const uint32_t ntp = (uint32_t)(t.npix - tp0 < (uint64_t)t.tile ? t.npix - tp0 : (uint64_t)t.tile);
        report_tile_stage(t, (t.pix0 + tp0) * (uint32_t)t.S, report_lds, chan, ntp * (uint32_t)t.S, lane);
        __syncthreads();
        unsigned v[3] = {0u, 0u, 0u};
        const bool active = lane < ntp;
        if (active) {
            const double *r = report_lds + lane * (uint32_t)t.stride;
            const double *const a[3] = {r, r + chan, r + 2 * chan};
            const double *const b[3] = {r + 3 * chan, r + 4 * chan, r + 5 * chan};
            double out[kReportPixelValues];
            report_pixel(a, b, t.S, out, v[0], v[1]);
            v[2] = v[1] ? 1u : 0u;
            double *o = t.pix + (tp0 + lane) * kReportPixelValues;
#pragma unroll
            for (int i = 0; i < kReportPixelValues; ++i) o[i] = out[i];
        }
        report_row_counts((uint32_t)((tp0 + lane) / (uint32_t)t.W), active, v, t.rows);
        __syncthreads(); // the next tile's staging overwrites the image
    }
}

// S > kReportTileMaxS: the same chains on global memory, one thread per pixel.  Correctness only.
__global__ __launch_bounds__(kWave) void report_pixel_direct_kernel(ReportTile t) {
    const uint64_t p = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    unsigned v[3] = {0u, 0u, 0u};
    const bool active = p < t.npix;
    if (active) {
        const double *ra = t.a + (t.pix0 + p) * (uint64_t)t.S, *rb = t.b + (t.pix0 + p) * (uint64_t)t.S;
        const double *const a[3] = {ra, ra + t.plane_stride, ra + 2 * t.plane_stride};
        const double *const b[3] = {rb, rb + t.plane_stride, rb + 2 * t.plane_stride};
        double out[kReportPixelValues];
        report_pixel(a, b, t.S, out, v[0], v[1]);
        v[2] = v[1] ? 1u : 0u;
        double *o = t.pix + p * kReportPixelValues;
#pragma unroll
        for (int i = 0; i < kReportPixelValues; ++i) o[i] = out[i];
    }
    report_row_counts((uint32_t)(p / (uint32_t)t.W), active, v, t.rows);
}

struct ReportRowArgs {
    const double *pix;                // [rows][W][kReportPixelValues]
    const int32_t *nbhd;              // [H*W]
    const double *alpha, *beta, *wrc; // [H*W][3], [H*W][n_feat], [H*W]; any may be null
    int32_t W, S, n_feat, row_begin;
    int32_t class_cap[RPF_REPORT_NCLASS - 1];
    rpf_report_row *rows;             // [rows]
};

template <class T>
__device__ __forceinline__ T wave_sum(T x) {
    for (int off = kWave / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
    return x;
}

// One wavefront per row of the slab.  Lane q < kRowDoubles runs the x chain of double q of the record, the loads of kChainBatch
// pixels in flight ahead of the chain; a weight (alpha, W_r_c, beta) that is not finite gives +0.0 to its chain and counts.  Then
// the lanes share the row's N for the integer fields.  Leaves the three counts of the pixel kernels alone.
constexpr int kChainBatch = 16;
__global__ __launch_bounds__(kWave) void report_row_kernel(ReportRowArgs a) {
    const uint32_t row = blockIdx.x, lane = threadIdx.x, W = (uint32_t)a.W, nF = (uint32_t)a.n_feat;
    const uint64_t ybase = (uint64_t)((uint32_t)a.row_begin + row) * W; // the row's first pixel in the [H*W] planes
    rpf_report_row *out = a.rows + row;
    const double *src = nullptr;
    uint32_t step = 0;
    const bool weight = lane >= (uint32_t)kRowAlpha;
    if (lane < (uint32_t)kRowAlpha) { src = a.pix + (uint64_t)row * W * kReportPixelValues + lane; step = kReportPixelValues; }
    else if (lane < (uint32_t)kRowWrc) { if (a.alpha) { src = a.alpha + ybase * 3 + (lane - kRowAlpha); step = 3; } }
    else if (lane == (uint32_t)kRowWrc) { if (a.wrc) { src = a.wrc + ybase; step = 1; } }
    else if (lane < (uint32_t)kRowBeta + nF) { if (a.beta) { src = a.beta + ybase * nF + (lane - kRowBeta); step = nF; } }
    double sum = 0.0;
    unsigned long long zeros = 0, nonfin = 0;
    if (src) {
        auto term = [&](double v) {
            if (!weight) return v;
            zeros += v == 0.0 ? 1u : 0u;
            if (finite64(v)) return v;
            ++nonfin;
            return 0.0;
        };
        sum = term(src[0]);
        uint32_t x = 1;
        for (; x + kChainBatch <= W; x += kChainBatch) {
            double v[kChainBatch];
#pragma unroll
            for (int j = 0; j < kChainBatch; ++j) v[j] = src[(uint64_t)(x + j) * step];
#pragma unroll
            for (int j = 0; j < kChainBatch; ++j) sum = sum + term(v[j]);
        }
        for (; x < W; ++x) sum = sum + term(src[(uint64_t)x * step]);
    }
    if (lane < (uint32_t)kRowDoubles) reinterpret_cast<double *>(out)[lane] = sum;
    if (lane >= (uint32_t)kRowAlpha && lane < (uint32_t)kRowWrc) out->alpha_zero[lane - kRowAlpha] = (int64_t)zeros;
    if (lane >= (uint32_t)kRowBeta && lane < (uint32_t)kRowDoubles) out->beta_zero[lane - kRowBeta] = (int64_t)zeros;
    const unsigned long long wn = wave_sum(nonfin);
    // N: sum, minimum, maximum, the pixels with N == S, the pixels per size class
    long long nsum = 0;
    int nmin = INT_MAX, nmax = INT_MIN;
    unsigned own = 0, cls[RPF_REPORT_NCLASS] = {};
    for (uint32_t x = lane; x < W; x += kWave) {
        const int n = a.nbhd[ybase + x];
        nsum += n;
        nmin = n < nmin ? n : nmin;
        nmax = n > nmax ? n : nmax;
        own += n == a.S ? 1u : 0u;
        int c = 0;
#pragma unroll
        for (int i = 0; i < RPF_REPORT_NCLASS - 1; ++i) c += n > a.class_cap[i] ? 1 : 0; // (the bounds ascend)
#pragma unroll
        for (int i = 0; i < RPF_REPORT_NCLASS; ++i) cls[i] += c == i ? 1u : 0u;
    }
    nsum = wave_sum(nsum);
    own = wave_sum(own);
#pragma unroll
    for (int i = 0; i < RPF_REPORT_NCLASS; ++i) cls[i] = wave_sum(cls[i]);
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const int lo = __shfl_xor(nmin, off, kWave), hi = __shfl_xor(nmax, off, kWave);
        nmin = lo < nmin ? lo : nmin;
        nmax = hi > nmax ? hi : nmax;
    }
    if (lane == 0) {
        out->weights_nonfinite = (int64_t)wn;
        out->sum_nbhd = nsum;
        out->own_only_pixels = (int64_t)own;
#pragma unroll
        for (int i = 0; i < RPF_REPORT_NCLASS; ++i) out->class_pixels[i] = (int64_t)cls[i];
        out->min_nbhd = nmin;
        out->max_nbhd = nmax;
    }
}

} // namespace

ReportCarve report_carve(int S) {
    ReportCarve c{};
    if (S <= 0 || S > kReportTileMaxS) return c; // the direct form
    c.stride = (uint32_t)S | 1u; // odd: lanes p and p + 1 land 2 * stride dwords apart, 32 lanes on 32 different bank pairs
    c.tile = (uint32_t)kReportLdsBudget / (48u * c.stride);
    if (c.tile > (uint32_t)kWave) c.tile = kWave;
    c.bytes = 48u * c.stride * c.tile;
    return c;
}

hipError_t launch_pass_report(const ReportPlanes &in, int W, int H, int S, int row_begin, int row_end, const int32_t class_cap[8],
                              double *pix, rpf_report_row *rows_out, hipStream_t s) {
    if (row_end <= row_begin) return hipSuccess;
    const uint32_t rows = (uint32_t)(row_end - row_begin);
    hipError_t err = hipMemsetAsync(rows_out, 0, (size_t)rows * sizeof(rpf_report_row), s);
    if (err != hipSuccess) return err;
    ReportTile t{};
    t.a = in.col_in; t.b = in.col_out;
    t.plane_stride = (uint64_t)W * H * S;
    t.pix0 = (uint64_t)row_begin * W;
    t.npix = (uint64_t)rows * W;
    t.S = S; t.W = W; t.pix = pix; t.rows = rows_out;
    const ReportCarve c = report_carve(S);
    if (c.tile == 0) {
        hipLaunchKernelGGL(report_pixel_direct_kernel, dim3((unsigned)((t.npix + kWave - 1) / kWave)), dim3(kWave), 0, s, t);
    } else {
        t.stride = (int32_t)c.stride; t.tile = (int32_t)c.tile;
        t.magic = S == 1 ? 0u : 0xFFFFFFFFu / (uint32_t)S + 1u;
        t.ntiles = (uint32_t)((t.npix + c.tile - 1) / c.tile);
        // as many one-wave workgroups as the device holds at once (LDS-bound), each walking its share of the tiles
        int dev = 0, cus = 0;
        err = hipGetDevice(&dev);
        if (err == hipSuccess) err = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (err != hipSuccess) return err;
        const uint32_t per_cu = std::max(1u, std::min(32u, (uint32_t)max_lds_per_block() / c.bytes));
        const uint32_t grid = std::min<uint32_t>(t.ntiles, (uint32_t)std::max(cus, 1) * per_cu);
        hipLaunchKernelGGL(report_pixel_tile_kernel, dim3(grid), dim3(kWave), c.bytes, s, t);
    }
    if ((err = hipGetLastError()) != hipSuccess) return err;
    ReportRowArgs r{};
    r.pix = pix; r.nbhd = in.nbhd; r.alpha = in.alpha; r.beta = in.beta; r.wrc = in.wrc;
    r.W = W; r.S = S; r.n_feat = in.n_feat; r.row_begin = row_begin;
    for (int i = 0; i < RPF_REPORT_NCLASS - 1; ++i) r.class_cap[i] = class_cap[i];
    r.rows = rows_out;
    hipLaunchKernelGGL(report_row_kernel, dim3(rows), dim3(kWave), 0, s, r);
    return hipGetLastError();
}

} // namespace rpf
