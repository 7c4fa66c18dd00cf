// rpf_generic_wide.hip -- the wide layout-generic kernel (RPF_FLAG_WIDE_NBHD): neighbourhoods of up to 262144 samples, the
// passes generic::filter_pixel_kernel (rpf_generic.hip) refuses above 65535.  Compiled with -ffp-contract=off like every
// kernel TU.
//
// filter_wide_kernel is a sibling of filter_pixel_kernel: 256 threads filter one pixel at a time and walk the rows of the
// slab.  Stages 1b, 2, 3a, 3c and 4 are that kernel's statements in that order -- the in-order chains, the member order and
// the halving-tree pairing of stage 4 included -- so a pixel's colours do not depend on which of the two kernels takes it
// (tests/test_wide_nbhd_gpu.py holds the two to the same bits on a frame both accept).  The device helpers are copies: a
// shared header would recompile rpf_generic.hip around them.  What differs:
//   * a bin id is 16 bits (B = floor(sqrt(N)) <= 512).  Member list (u32 [nmax]) and bin ids (u16 [ndim][nmax]) always live in
//     one HBM slot per workgroup; bin_hash hashes fnv1a_u16 of the id as before.
//   * a histogram cell is 32 bits (a near-constant column pair puts almost N counts into one cell).  The B x B joint table
//     (up to 1 MiB) is built in bands of R = floor(band_words / B) rows, ascending: every member whose first bin id lies in
//     the band adds to LDS, then T[count] is summed over the band's cells.  The sums are integers: MI does not depend on R.
//     Marginals are B <= 512 entries.
//   * T comes from the launcher: round(k ln k * 2^bits), bits = 41 (below 2^63 up to k = 2^18; PassParams::tfix saturates
//     from k = 48586 on).  TN + sum T[J] may pass 2^63, so f is formed in unsigned arithmetic (exact modulo 2^64, and
//     |f| <= N ln B * 2^41 < 2^63).  The zero band keeps its formula in units of the table.
//   * REF_ABORT: the reference's expression for an in-band table takes the cells in the reference's order, which the
//     ascending bands preserve; thread 0 carries one running sum through them.
#include "rpf_device_common.h"

#ifndef RPF_GENERIC_OWN
#define RPF_GENERIC_OWN 4 // own samples per sweep of stage 4 (their accumulators are registers; same bits at any value)
#endif

#include <algorithm>
#include <cmath>

namespace rpf {

namespace generic {
namespace {
constexpr int kThreads = 256, kChunk = 64;
constexpr int kOwn = RPF_GENERIC_OWN; // own samples per sweep of stage 4
constexpr int kMargMax = 512;         // floor(sqrt(kMaxWideNbhd)): entries of a marginal histogram
constexpr uint32_t kLdsBudget = (160u << 10) - 1024u; // dynamic LDS: the kernel also has 256 B of static LDS (barrier reductions)

// column counts of a layout (generic_dims of rpf_generic.hip)
struct WideDims {
    int nR, nF, ndim, nAnc, npairF, npairC, npair, nwt, colF;
};
__host__ __device__ inline WideDims wide_dims(const SampleLayout &l) {
    WideDims d;
    d.nR = l.nR; d.nF = l.nF; d.ndim = 5 + l.nR + l.nF;
    d.nAnc = l.nR + 2;                       // r.. and p.. anchors
    d.npairF = l.nF * d.nAnc;                // pairs (f_i, r_l | p_l)          rpf.cpp:416-427
    d.npairC = d.nAnc + l.nF;                // pairs of one colour channel     rpf.cpp:429-442
    d.npair = d.npairF + 3 * d.npairC;
    d.nwt = 5 + l.nF;                        // weighted columns of stage 4
    d.colF = 5 + l.nR;
    return d;
}
} // namespace
} // namespace generic

// The LDS carve-up of the wide kernel (rpf_internal.h): generic_carve's fp64 block and chunk (marginals of kMargMax entries),
// then the band of the joint histogram -- the whole table where it fits, else what the budget leaves -- and red4 over the
// dead chunk and band.
GenericWideCarve generic_wide_carve(const SampleLayout &lay, int nmax) {
    const generic::WideDims D = generic::wide_dims(lay);
    GenericWideCarve c{};
    auto up16 = [](uint32_t v) { return (v + 15u) & ~15u; };
    uint32_t o = (uint32_t)(8 * D.ndim + D.npair + 2 * D.nF + 20 + generic::kThreads) * 8u;
    c.off_chunk = o;
    uint32_t chunk = (uint32_t)D.ndim * (generic::kChunk + 1) * 8u;
    chunk = std::max(chunk, 2u * generic::kMargMax * 4u + (uint32_t)D.npair * 4u); // sMargX | sMargY | sNeed
    chunk = std::max(chunk, (uint32_t)generic::kOwn * (uint32_t)D.nwt * 8u);          // own rows of a sweep
    chunk = std::max(chunk, (8u + 2u * (uint32_t)D.nF) * 8u);                         // stage 1b: wave counts, feature means, 3 sigma
    o = up16(o + chunk);
    c.off_hist = o;
    const uint32_t bmax = (uint32_t)std::max(1.0, std::floor(std::sqrt((double)nmax)));
    const uint32_t table = up16(bmax * bmax * 4u), row = bmax * 4u;
    uint32_t band = o < generic::kLdsBudget ? std::min(table, (generic::kLdsBudget - o) & ~15u) : 0u;
    if (band < row) band = up16(row); // does not fit: total says so
    c.band_words = band / 4u;
    o += band;
    c.off_red4 = c.off_chunk + up16((uint32_t)generic::kOwn * (uint32_t)D.nwt * 8u);
    c.total = std::max(o, c.off_red4 + 4u * generic::kThreads * 8u);
    return c;
}

namespace generic {
namespace {

struct WideScratch {
    uint32_t *list;        // [slots][nmax]        member list (plane offsets), reference order
    uint16_t *bins;        // [slots][ndim][nmax]  bin ids
    const uint64_t *table; // round(k ln k * 2^bits), k = 0 .. nmax
    int32_t bits;
    const uint32_t *count_dev; // size of p.pix_list on the device, or null = p.list_count
};

template <class T>
__device__ __forceinline__ float ldp(const PassParams &p, int col, uint32_t off) {
    return (float)reinterpret_cast<const T *>(p.planes)[(uint64_t)col * p.plane_stride + off];
}
// value of column c of the sample at plane offset `off`: colours come from the fp64 colour planes
template <class T>
__device__ __forceinline__ double load_col(const PassParams &p, int c, uint32_t off) {
    if (c >= 2 && c < 5) return p.col_in[(uint64_t)(c - 2) * p.plane_stride + off];
    return (double)ldp<T>(p, c, off);
}
// columns of MI pair pr, in ComputeCFWeights call order (rpf.cpp:416-442 with the loop bounds generalised)
__device__ __forceinline__ void pair_cols(const WideDims &D, int pr, int &ca, int &cb) {
    if (pr < D.npairF) {
        const int i = pr / D.nAnc, l = pr - i * D.nAnc;
        ca = D.colF + i;
        cb = l < D.nR ? 5 + l : l - D.nR;
    } else {
        const int q = pr - D.npairF, c = q / D.npairC, l = q - c * D.npairC;
        ca = 2 + c;
        cb = l < D.nR ? 5 + l : (l < D.nAnc ? l - D.nR : D.colF + (l - D.nAnc));
    }
}

// order-free reductions (integer sums) over the workgroup; result in every thread.  sRed4: 4 slots
template <class V, class Op>
__device__ __forceinline__ V block_reduce(V v, V *sRed4, Op op) {
    for (int s = 32; s > 0; s >>= 1) v = op(v, __shfl_down(v, s, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sRed4[threadIdx.x >> 6] = v;
    __syncthreads();
    return op(op(sRed4[0], sRed4[1]), op(sRed4[2], sRed4[3]));
}

// One workgroup filters one pixel at a time and walks the pixels of rows [row_begin, row_end), or those of p.pix_list.
template <class T>
__global__ __launch_bounds__(256) void filter_wide_kernel(PassParams p, GenericWideCarve cv, WideScratch gs) {
    extern __shared__ __align__(16) unsigned char smem[];
    const WideDims D = wide_dims(p.lay);
    const int ndim = D.ndim, nF = D.nF, nR = D.nR, nAnc = D.nAnc, npair = D.npair, nwt = D.nwt, colF = D.colF;
    double *sStat = reinterpret_cast<double *>(smem);                 // M | SD | xmin | xmax
    double *sZ = sStat + 4 * ndim;                                    // lo | range | flags(sd0 | flat << 1) per column
    uint64_t *sHX = reinterpret_cast<uint64_t *>(sZ + 3 * ndim);      // sum_i T[hx_i] per column
    uint64_t *sPair = sHX + ndim;                                     // sum_ij T[J_ij] per pair, then the MI values
    double *sMI = reinterpret_cast<double *>(sPair);
    double *sW = sMI + npair;                                         // Drf[nF] | D9[12] | alpha[4] | beta[nF] | wrc[4]
    double *sRedD = sW + 2 * nF + 20;                                 // [256] reduction scratch (also u64 views)
    double *sChunk = reinterpret_cast<double *>(smem + cv.off_chunk); // [ndim][kChunk + 1]
    uint32_t *sHist = reinterpret_cast<uint32_t *>(smem + cv.off_hist); // [band_words] one band of a joint table, 32-bit cells
    double *sRed4 = reinterpret_cast<double *>(smem + cv.off_red4);   // [4][256] stage 4 (chunk and band are dead there)
    int *sCnt = reinterpret_cast<int *>(sChunk);                      // stage 1b: per-wave counts (the chunk is not live yet)

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int W = p.W, H = p.H, S = p.S, b = p.b;
    const uint64_t HW = (uint64_t)H * W;
    uint32_t *list = gs.list + (uint64_t)blockIdx.x * p.nmax;
    uint16_t *bins = gs.bins + (uint64_t)blockIdx.x * ndim * p.nmax;
    const uint64_t *tw = gs.table;
    const double e_eps = (p.policy == RPF_DEGEN_EPS) ? p.eps : 0.0;

    const uint32_t npix = p.pix_list ? (gs.count_dev ? *gs.count_dev : p.list_count) : (uint32_t)(p.row_end - p.row_begin) * (uint32_t)W;
    for (uint32_t e = blockIdx.x; e < npix; e += gridDim.x) {
        const uint64_t pix = p.pix_list ? (uint64_t)p.pix_list[e] : (uint64_t)p.row_begin * W + e;
        const int y = (int)(pix / (uint32_t)W), x = (int)(pix - (uint64_t)y * W);
        __syncthreads(); // the previous pixel's LDS is dead

        // ---- stage 1b: the 3-sigma test and the member list, reference order (rpf.cpp:556-586) -------------------
        const int x0 = max(x - b, 0), x1 = min(x + b, W - 1), y0 = max(y - b, 0), y1 = min(y + b, H - 1);
        const int nyv = y1 - y0 + 1;
        const int centre_rank = (x - x0) * nyv + (y - y0);
        const int ncand = ((x1 - x0 + 1) * nyv - 1) * S;
        for (int s = tid; s < S; s += kThreads) list[s] = (uint32_t)(pix * S + s); // own samples first
        int n = S;
        double *sMf = sChunk + 8, *sLf = sMf + nF;
        for (int k = tid; k < nF; k += kThreads) {
            sMf[k] = p.pmean[(uint64_t)k * HW + pix];
            sLf[k] = p.pstd[(uint64_t)k * HW + pix] * 3.0; // multiplyArray(std, 3), rpf.cpp:579
        }
        __syncthreads();
        for (int q0 = 0; q0 < ncand; q0 += kThreads) {
            const int qb = q0 + wv * 64;                       // this wave's 64-candidate block
            unsigned long long mask = 0ull;
            uint32_t off = 0u;
            if (qb < ncand) { // wave-uniform
                const int qq = qb + lane;
                bool pass = qq < ncand;
                if (pass) {
                    int cell = qq / S;
                    const int s = qq - cell * S;
                    if (cell >= centre_rank) ++cell;              // rpf.cpp:565: skip the centre pixel
                    const int ix = cell / nyv, iy = cell - ix * nyv; // xn outer, yn inner ascending (rpf.cpp:562-563)
                    off = (uint32_t)(((uint64_t)(y0 + iy) * W + (x0 + ix)) * S + s);
                    for (int k = 0; k < nF; ++k) {
                        const double a = fabs((double)ldp<T>(p, colF + k, off) - sMf[k]);
                        if (a >= sLf[k]) pass = false;     // allLessThan: fails iff a >= b (ops.h:101-104): a NaN never rejects
                    }
                }
                mask = __ballot(pass);
            }
            if (lane == 0) sCnt[wv] = __popcll(mask);
            __syncthreads();
            int base = n;
            for (int w = 0; w < wv; ++w) base += sCnt[w];
            const int tot = sCnt[0] + sCnt[1] + sCnt[2] + sCnt[3];
            if ((mask >> lane) & 1ull) {
                const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
                if (at < p.nmax) list[at] = off;
            }
            n += tot;
            __syncthreads();
        }
        if (tid == 0) p.nbhd[pix] = n;
        __threadfence_block();
        __syncthreads();
        const int B = max(1, (int)sqrt((double)n));                // mi.cpp:54
        const double dn = (double)n;

        // ---- stage 2: in-order sums over the neighbourhood (rpf.cpp:596-601), chunks of 64 staged through LDS ------
        // lane c of wave 0 adds column c's x front to back, lane c of wave 1 its x*x: one thread per chain
        {
            double acc = 0.0;
            const bool chain = wv < 2 && lane < ndim, is_sq = wv == 1;
            for (int j0 = 0; j0 < n; j0 += kChunk) {
                const int cnt = min(kChunk, n - j0);
                for (int t = tid; t < cnt * ndim; t += kThreads) {
                    const int c = t / cnt, q = t - c * cnt;
                    sChunk[c * (kChunk + 1) + q] = load_col<T>(p, c, list[j0 + q]);
                }
                __syncthreads();
                if (chain) {
                    const double *src = sChunk + lane * (kChunk + 1);
                    for (int q = 0; q < cnt; ++q) { const double v = src[q]; acc = acc + (is_sq ? v * v : v); } // ops.h:121, 138
                }
                __syncthreads();
            }
            if (chain && is_sq) sRedD[lane] = acc;
            __syncthreads();
            if (chain && !is_sq) {
                const double sq = sRedD[lane];
                const double mean = acc / dn;                                  // ops.h:123
                double sd = sqrt(sq / dn - mean * mean);                       // ops.h:141
                if (p.policy == RPF_DEGEN_EPS && isnan(sd)) sd = 0.0;
                sStat[lane] = mean; sStat[ndim + lane] = sd;
                if (p.dbg.mean) p.dbg.mean[pix * ndim + lane] = mean;
                if (p.dbg.stddev) p.dbg.stddev[pix * ndim + lane] = sd;
            }
        }
        // column minima / maxima (order-free), then the per-column constants of the binning (sd.h:229-232, mi.cpp:47-50)
        for (int c = wv; c < ndim; c += kThreads / 64) { // a column per wave
            double mn = INFINITY, mx = -INFINITY;
            for (int j = lane; j < n; j += 64) { const double v = load_col<T>(p, c, list[j]); mn = fmin(mn, v); mx = fmax(mx, v); }
            for (int s = 32; s > 0; s >>= 1) { mn = fmin(mn, __shfl_down(mn, s, 64)); mx = fmax(mx, __shfl_down(mx, s, 64)); }
            if (lane == 0) { sStat[2 * ndim + c] = mn; sStat[3 * ndim + c] = mx; }
        }
        __syncthreads();
        if (tid < ndim) {
            const double Mc = sStat[tid], SDc = sStat[ndim + tid];
            const bool sd0 = (SDc == 0.0);
            const double lo = sd0 ? 0.0 : (sStat[2 * ndim + tid] - Mc) / SDc, hi = sd0 ? 0.0 : (sStat[3 * ndim + tid] - Mc) / SDc;
            sZ[tid] = lo; sZ[ndim + tid] = hi - lo;
            sZ[2 * ndim + tid] = (double)((sd0 ? 1 : 0) | (!(hi != lo) ? 2 : 0)); // mi.cpp:7 / 28 / 34
        }
        __syncthreads();

        // ---- stage 3a: normalise, bin ids (16 bits per sample and column) -------------------------------------------
        for (int c = 0; c < ndim; ++c) {
            const double Mc = sStat[c], SDc = sStat[ndim + c], lo = sZ[c], range = sZ[ndim + c];
            const int flags = (int)sZ[2 * ndim + c];
            const bool sd0 = flags & 1, flat = flags & 2;
            uint16_t *bc = bins + (uint64_t)c * p.nmax;
            for (int j = tid; j < n; j += kThreads) {
                int bin = 0;
                if (!flat) {
                    const double a = load_col<T>(p, c, list[j]) - Mc;       // subtractArrays
                    const double z = sd0 ? 0.0 : a / SDc;                      // divideArrays, ops.h:48
                    const double t = (z - lo) / range * (double)B;             // mi.cpp:14
                    bin = max(min((int)t, B - 1), 0);
                }
                bc[j] = (uint16_t)bin;
            }
        }
        __threadfence_block();
        __syncthreads();
        if (p.dbg.member_hash != nullptr && tid == 0) {
            uint32_t h = 2166136261u;
            for (int j = 0; j < n; ++j) {
                const uint32_t o = list[j], s = o % (uint32_t)S, q = o / (uint32_t)S;
                const int yn = (int)(q / (uint32_t)W), xn = (int)(q % (uint32_t)W);
                h = fnv1a_u32(h, (uint32_t)(((xn - x + b) * p.box + (yn - y + b)) * S) + s);
            }
            p.dbg.member_hash[pix] = h;
        }
        if (p.dbg.bin_hash != nullptr && tid < ndim) {
            uint32_t h = 2166136261u;
            const uint16_t *bc = bins + (uint64_t)tid * p.nmax;
            for (int j = 0; j < n; ++j) h = fnv1a_u16(h, bc[j]);
            p.dbg.bin_hash[pix * ndim + tid] = h;
        }

        // ---- stage 3b: histograms, 32-bit cells; a joint table in bands of R rows, ascending ---------------------------
        const int R = min(B, (int)(cv.band_words / (uint32_t)B));      // rows of a band (>= 1: the carve-up holds a row of bmax)
        auto clear_band = [&](int cells) {
            for (int t = tid; t < cells; t += kThreads) sHist[t] = 0u;
        };
        // the members whose first bin id lies in rows [r0, r0 + rows) add to the band (ba == null: a marginal, one row)
        auto fill_band = [&](const uint16_t *ba, const uint16_t *bb, int r0, int rows) {
            for (int j0 = 0; j0 < n; j0 += 4 * kThreads) {
                uint32_t ra[4], cb4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + u * kThreads + tid;
                    ra[u] = 0xffffffffu; cb4[u] = 0u;
                    if (j < n) {
                        ra[u] = ba ? (uint32_t)ba[j] - (uint32_t)r0 : 0u;
                        cb4[u] = bb[j];
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (ra[u] < (uint32_t)rows) atomicAdd(&sHist[ra[u] * (uint32_t)B + cb4[u]], 1u);   // mi.cpp:39
            }
        };
        auto sum_band = [&](int cells) -> uint64_t { // sum over the band's cells of T[count] (T[0] = 0)
            uint64_t acc = 0ull;
            for (int t = tid; t < cells; t += kThreads) {
                const uint32_t c = sHist[t];
                if (c) acc += tw[c];
            }
            return acc;
        };
        auto hist_T = [&](const uint16_t *ba, const uint16_t *bb) -> uint64_t {
            uint64_t acc = 0ull;
            const int nrow = ba ? B : 1, step = ba ? R : 1;
            for (int r0 = 0; r0 < nrow; r0 += step) {
                const int rows = min(step, nrow - r0);
                __syncthreads(); // the previous band (or table) has been summed
                clear_band(rows * B);
                __syncthreads();
                fill_band(ba, bb, r0, rows);
                __syncthreads();
                acc += sum_band(rows * B);
            }
            return block_reduce(acc, reinterpret_cast<uint64_t *>(sRedD), [](uint64_t a, uint64_t b2) { return a + b2; });
        };
        for (int c = 0; c < ndim; ++c) {
            const uint64_t t = hist_T(nullptr, bins + (uint64_t)c * p.nmax);
            if (tid == 0) sHX[c] = t;
        }
        for (int pr = 0; pr < npair; ++pr) {
            int ca, cb;
            pair_cols(D, pr, ca, cb);
            const uint64_t t = hist_T(bins + (uint64_t)ca * p.nmax, bins + (uint64_t)cb * p.nmax);
            if (tid == 0) sPair[pr] = t;
        }
        __syncthreads();
        uint32_t *sMargX = reinterpret_cast<uint32_t *>(sChunk), *sMargY = sMargX + kMargMax; // (the staging chunk is not live here)
        int *sNeed = reinterpret_cast<int *>(sMargY + kMargMax);                               // [npair]
        {
            const uint64_t TN = tw[n];
            const int64_t zero_band = ((int64_t)B * B + 2 * B + 1) / 2 + 1;   // see filter_pixel_kernel (rpf_filter_impl.inc)
            for (int pr = tid; pr < npair; pr += kThreads) {
                int ca, cb;
                pair_cols(D, pr, ca, cb);
                // TN + sum T[J] may pass 2^63: unsigned sums are exact modulo 2^64, and |f| < 2^63
                int64_t f = (int64_t)(TN + sPair[pr] - sHX[ca] - sHX[cb]);
                int need = 0;
                if (f <= zero_band && f >= -zero_band) {
                    // REF_ABORT: the reference's own value for such a table is rounding residue unless its quotients are
                    // exact (N a power of two, or a one-bin column): evaluated below, term by term
                    need = p.policy == RPF_DEGEN_REF_ABORT && (n & (n - 1)) != 0 && sHX[ca] != TN && sHX[cb] != TN;
                    f = 0;
                }
                sNeed[pr] = need;
                const double mi = ldexp((double)f, -gs.bits) / dn;
                sMI[pr] = mi; // (same slot as sPair[pr]: each thread overwrites only what it has just read)
                if (p.dbg.mi) p.dbg.mi[pix * npair + pr] = mi;
            }
        }
        __syncthreads();
        // ---- the reference expression for tables inside the rounding band (REF_ABORT): mi.cpp:66-86 on the integer counts,
        // same operations in the same cell order (bands ascending, cells ascending inside a band), with log(1 +- k ulp) as the
        // host's libm returns it (rpf_reflog.h)
        if (p.policy == RPF_DEGEN_REF_ABORT) {
            for (int pr = 0; pr < npair; ++pr) {
                if (!sNeed[pr]) continue; // workgroup-uniform
                int ca, cb;
                pair_cols(D, pr, ca, cb);
                const uint16_t *ba = bins + (uint64_t)ca * p.nmax, *bb = bins + (uint64_t)cb * p.nmax;
                __syncthreads();
                for (int t = tid; t < 2 * kMargMax; t += kThreads) sMargX[t] = 0u; // both marginals
                __syncthreads();
                for (int j = tid; j < n; j += kThreads) {
                    atomicAdd(&sMargX[ba[j]], 1u);                                              // mi.cpp:17
                    atomicAdd(&sMargY[bb[j]], 1u);
                }
                double mi = 0.0; // thread 0's running sum
                for (int r0 = 0; r0 < B; r0 += R) {
                    const int rows = min(R, B - r0), cells = rows * B;
                    __syncthreads();
                    clear_band(cells);
                    __syncthreads();
                    fill_band(ba, bb, r0, rows);
                    __syncthreads();
                    for (int t0 = 0; t0 < cells; t0 += kThreads) {
                        const int t = t0 + tid;
                        double term = 0.0;
                        if (t < cells) {
                            const int i = t / B, j = t - i * B;
                            const double pX = (double)sMargX[r0 + i] / dn, pY = (double)sMargY[j] / dn; // mi.cpp:70-75
                            const double pXY = (double)sHist[t] / dn;                                   // mi.cpp:81
                            const double pp = pX * pY;                                                  // mi.cpp:82
                            if (pXY > 0 && pp != 0) {
                                const double q = pXY / pp;
                                term = pXY * (reflog_in_range(q) ? reflog_near_one(q) : log(q));        // mi.cpp:84
                            }
                        }
                        sRedD[tid] = term;
                        __syncthreads();
                        if (tid == 0) {
                            const int cnt = min(kThreads, cells - t0);
                            for (int q = 0; q < cnt; ++q) mi += sRedD[q];
                        }
                        __syncthreads();
                    }
                }
                if (tid == 0) {
                    sMI[pr] = mi;
                    if (p.dbg.mi) p.dbg.mi[pix * npair + pr] = mi;
                }
            }
            __syncthreads();
        }

        // ---- stage 3c: alpha, beta, W_r_c (rpf.cpp:444-487) ----------------------------------------------------------
        double *sDrf = sW, *sD9 = sDrf + nF, *sAlpha = sD9 + 12, *sBeta = sAlpha + 4, *sWrc = sBeta + nF;
        {
            const int k = min(tid, nF - 1), c = min(tid, 2);
            double Drf = 0.0, Dpf = 0.0, Dcf = 0.0, Drc = 0.0, Dpc = 0.0, Dfc = 0.0;
            const int base = D.npairF + c * D.npairC;
            for (int l = 0; l < nR; ++l) { Drf += sMI[k * nAnc + l]; Drc += sMI[base + l]; }                 // rpf.cpp:421, 432
            for (int l = 0; l < 2; ++l) { Dpf += sMI[k * nAnc + nR + l]; Dpc += sMI[base + nR + l]; }        // rpf.cpp:425, 436
            for (int cc = 0; cc < 3; ++cc) Dcf += sMI[D.npairF + cc * D.npairC + nAnc + k];
            for (int j = 0; j < nF; ++j) Dfc += sMI[base + nAnc + j];                                        // rpf.cpp:440
            if (tid < nF) sDrf[tid] = Drf;
            if (tid < 3) { sD9[tid] = Drc; sD9[3 + tid] = Dpc; sD9[6 + tid] = Dfc; }
            __syncthreads();
            double D_f_c = 0.0, D_r_c = 0.0, D_p_c = 0.0;                                                    // rpf.cpp:449-456
            for (int i = 0; i < 3; ++i) { D_f_c += sD9[6 + i]; D_r_c += sD9[i]; D_p_c += sD9[3 + i]; }
            const double den = D_f_c + D_r_c + D_p_c + e_eps;
            double wsum = 0.0;
            for (int i = 0; i < 3; ++i) wsum += sD9[i] / (sD9[i] + sD9[3 + i] + e_eps);                      // rpf.cpp:470, 485
            const double wrc = wsum / 3;                                                                     // rpf.cpp:487
            const double alpha_c = 1 - Drc / (Drc + Dpc + e_eps);                                            // rpf.cpp:470, 475
            // the beta presets keep the reference's stack rule for any nF: k < 3 reads D_f_ck, a gap of zeros, then D_r_fk
            double num;
            if (p.beta_map == RPF_BETA_PAPER) num = Dcf;
            else if (p.beta_map == RPF_BETA_REF_GCC11_O2) num = k < 3 ? sD9[6 + c] : (k < 8 ? 0.0 : sDrf[max(k - 8, 0)]);
            else num = k < 3 ? sD9[6 + c] : (k < 4 ? 0.0 : sDrf[max(k - 4, 0)]);
            const double beta_k = (1 - Drf / (Drf + Dpf + e_eps)) * (num / den);                             // rpf.cpp:464-465, 479
            if (tid < nF) { sBeta[tid] = beta_k; if (p.dbg.beta) p.dbg.beta[pix * nF + tid] = beta_k; }
            if (tid < 3) { sAlpha[tid] = alpha_c; if (p.dbg.alpha) p.dbg.alpha[pix * 3 + tid] = alpha_c; }
            if (tid == 0) { sWrc[0] = wrc; if (p.dbg.wrc) p.dbg.wrc[pix] = wrc; }
            __syncthreads();
        }

        // ---- stage 4: weights and blend, term by term as rpf.cpp:646-717; kOwn own samples per sweep.  The column loop is
        // outermost: a neighbour's value of column k is loaded and normalised once, then the kOwn own samples' sp / sc / sf
        // take its term -- each accumulator still receives its terms in ascending k (the reference's order).
        {
            const double wrc = sWrc[0];
            const double sigma_c2 = p.seed * p.seed / (1 - wrc) / (1 - wrc);                                  // rpf.cpp:662
            const double sigma_p2 = p.sigma_p * p.sigma_p;
            auto znorm = [&](int c, double xv) { const double sd = sStat[ndim + c]; return sd == 0.0 ? 0.0 : (xv - sStat[c]) / sd; };
            double *sOwnZ = sChunk; // [nwt][kOwn] normalised own samples of the sweep (the staging chunk is dead)
            bool bad = false;
            for (int i0 = 0; i0 < S; i0 += kOwn) {
                __syncthreads();
                for (int t = tid; t < kOwn * nwt; t += kThreads) {
                    const int k = t / kOwn, ii = t % kOwn, i = min(i0 + ii, S - 1);
                    const int col = k < 5 ? k : k + nR;
                    sOwnZ[t] = znorm(col, load_col<T>(p, col, (uint32_t)(pix * S + i)));
                }
                __syncthreads();
                double sw[kOwn], s0[kOwn], s1[kOwn], s2[kOwn];
#pragma unroll
                for (int ii = 0; ii < kOwn; ++ii) { sw[ii] = 0.0; s0[ii] = 0.0; s1[ii] = 0.0; s2[ii] = 0.0; }
                for (int j = tid; j < n; j += kThreads) {
                    const uint32_t off = list[j];
                    double sp[kOwn], sc[kOwn], sf[kOwn], cj[3];
#pragma unroll
                    for (int ii = 0; ii < kOwn; ++ii) { sp[ii] = 0.0; sc[ii] = 0.0; sf[ii] = 0.0; }
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const double zj = znorm(k, (double)ldp<T>(p, k, off));
#pragma unroll
                        for (int ii = 0; ii < kOwn; ++ii) { const double t = sOwnZ[k * kOwn + ii] - zj; sp[ii] += t * t; }
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        cj[k] = p.col_in[(uint64_t)k * p.plane_stride + off];
                        const double zj = znorm(2 + k, cj[k]), ak = sAlpha[k];
#pragma unroll
                        for (int ii = 0; ii < kOwn; ++ii) { const double t = sOwnZ[(2 + k) * kOwn + ii] - zj; sc[ii] += (t * t) * ak; }
                    }
                    for (int k = 0; k < nF; ++k) {
                        const double zj = znorm(colF + k, (double)ldp<T>(p, colF + k, off)), bk = sBeta[k];
#pragma unroll
                        for (int ii = 0; ii < kOwn; ++ii) { const double t = sOwnZ[(5 + k) * kOwn + ii] - zj; sf[ii] += (t * t) * bk; }
                    }
#pragma unroll
                    for (int ii = 0; ii < kOwn; ++ii) {
                        double w = exp(-sp[ii] / (2 * sigma_p2)) * exp(-sc[ii] / (2 * sigma_c2)) * exp(-sf[ii] / (2 * sigma_c2)); // rpf.cpp:667-670
                        w = (i0 + ii < S) ? w : 0.0;
                        sw[ii] += w; s0[ii] += w * cj[0]; s1[ii] += w * cj[1]; s2[ii] += w * cj[2];   // rpf.cpp:691-692
                    }
                }
                // the four sums of an own sample are reduced in the pairing of a halving tree over the 256 threads:
                // v[t] + v[t + 128], + 64 across the waves, then 32 ... 1 inside wave 0
#pragma unroll
                for (int ii = 0; ii < kOwn; ++ii) {
                    __syncthreads();
                    sRed4[tid] = sw[ii]; sRed4[kThreads + tid] = s0[ii];
                    sRed4[2 * kThreads + tid] = s1[ii]; sRed4[3 * kThreads + tid] = s2[ii];
                    __syncthreads();
                    if (wv == 0) {
                        double v[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const double *r = sRed4 + q * kThreads + lane;
                            double a = (r[0] + r[128]) + (r[64] + r[192]);
                            for (int s = 32; s > 0; s >>= 1) a = a + __shfl_down(a, s, 64);
                            v[q] = __shfl(a, 0, 64);
                        }
                        const int i = i0 + ii;
                        if (lane < 3 && i < S) {
                            double prime = (lane == 0 ? v[1] : (lane == 1 ? v[2] : v[3])) / v[0];                 // rpf.cpp:700
                            if (isnan(prime)) {                                                                    // rpf.cpp:702
                                bad = true;
                                if (p.policy == RPF_DEGEN_EPS) prime = p.col_in[(uint64_t)lane * p.plane_stride + pix * S + i];
                            }
                            p.col_out[(uint64_t)lane * p.plane_stride + pix * S + i] = prime;
                        }
                    }
                }
            }
            const int anybad = __syncthreads_or(bad ? 1 : 0);
            if (tid == 0 && anybad) {
                atomicAdd(&p.status[0], 1);
                atomicMin(&p.status[1], (int)pix);
            }
        }
    }
}

template <class T>
hipError_t launch_filter_wide_t(const PassParams &p, const GenericWideCarve &cv, const WideScratch &gs, unsigned grid, hipStream_t s) {
    hipError_t e = hipFuncSetAttribute((const void *)filter_wide_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cv.total);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(filter_wide_kernel<T>, dim3(grid), dim3(kThreads), cv.total, s, p, cv, gs);
    return hipGetLastError();
}

} // namespace

hipError_t launch_filter_wide(const PassParams &p, void *list, void *bins, uint32_t slots, const uint64_t *table, int table_bits,
                              const uint32_t *count_dev, hipStream_t s) {
    const GenericWideCarve cv = generic_wide_carve(p.lay, p.nmax);
    if ((int)cv.total > max_lds_per_block() || cv.total > kLdsBudget) return hipErrorInvalidValue;
    if (p.nmax < 1 || p.nmax > kMaxWideNbhd || (count_dev != nullptr && p.pix_list == nullptr)) return hipErrorInvalidValue;
    if (cv.band_words < (uint32_t)std::max(1.0, std::floor(std::sqrt((double)p.nmax)))) return hipErrorInvalidValue; // a band holds a row of the widest table
    if (p.row_end <= p.row_begin) return hipSuccess;
    if (p.pix_list != nullptr && count_dev == nullptr && p.list_count == 0) return hipSuccess;
    if (list == nullptr || bins == nullptr || table == nullptr || slots == 0) return hipErrorInvalidValue;
    const uint64_t npix = p.pix_list ? (count_dev ? (uint64_t)slots : (uint64_t)p.list_count) : (uint64_t)(p.row_end - p.row_begin) * p.W;
    const unsigned grid = (unsigned)std::min<uint64_t>(npix, slots);
    WideScratch gs;
    gs.list = (uint32_t *)list; gs.bins = (uint16_t *)bins; gs.table = table; gs.bits = table_bits; gs.count_dev = count_dev;
    return p.lay.f16 ? launch_filter_wide_t<__half>(p, cv, gs, grid, s) : launch_filter_wide_t<float>(p, cv, gs, grid, s);
}

} // namespace generic
} // namespace rpf
