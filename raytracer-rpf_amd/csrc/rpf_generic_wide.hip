// rpf_generic_wide.hip -- the wide layout-generic kernel (RPF_FLAG_WIDE_NBHD): neighbourhoods of up to 262144 samples, the
// passes generic::filter_pixel_kernel (rpf_generic.hip) refuses above 65535.  Compiled with -ffp-contract=off like every
// kernel TU.
//
// filter_wide_kernel is a sibling of filter_pixel_kernel: 256 threads filter one pixel at a time and walk the rows of the
// slab.  Stages 1b, 2, 3a, 3c and 4 are that kernel's statements in that order -- the in-order chains, the member order and
// the halving-tree pairing of stage 4 included -- and one copy of them: both kernels include rpf_generic_stream_stages.inc
// (which says why it is text and not functions), with Bin the type of a bin id.  So a pixel's colours do not depend on which
// of the two kernels takes it (tests/test_wide_nbhd_gpu.py holds the two to the same bits on a frame both accept).  Dims,
// loaders, pair_cols and block_reduce come from rpf_generic_common.h.  What this file holds is what differs (DESIGN.md
// section 11c):
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
#include "rpf_generic_common.h"

#include <algorithm>
#include <cmath>

namespace rpf {

namespace generic {
namespace {
constexpr int kMargMax = 512;         // floor(sqrt(kMaxWideNbhd)): entries of a marginal histogram
constexpr uint32_t kLdsBudget = (160u << 10) - 1024u; // dynamic LDS: the kernel also has 256 B of static LDS (barrier reductions)
} // namespace
} // namespace generic

// The LDS carve-up of the wide kernel (rpf_internal.h): generic_carve's fp64 block and chunk (marginals of kMargMax entries),
// then the band of the joint histogram -- the whole table where it fits, else what the budget leaves -- and red4 over the
// dead chunk and band.  fast: the launch of filter_wide_kernel<T, true> (own rows of kStreamFastOwn floats per weighted column).
GenericWideCarve generic_wide_carve(const SampleLayout &lay, int nmax, bool fast) {
    const GenericDims D = generic_dims(lay);
    GenericWideCarve c{};
    uint32_t o = (generic_f64_doubles(D) + generic::kThreads) * 8u;
    c.off_chunk = o;
    uint32_t chunk = (uint32_t)D.ndim * (generic::kChunk + 1) * 8u;
    chunk = std::max(chunk, 2u * generic::kMargMax * 4u + (uint32_t)D.npair * 4u); // sMargX | sMargY | sNeed
    const uint32_t own_at = fast ? up16(o) : o;                                        // where the own rows of a sweep start (as generic_carve)
    const uint32_t own = fast ? (uint32_t)generic::kStreamFastOwn * (uint32_t)D.nwt * 4u : (uint32_t)generic::kOwn * (uint32_t)D.nwt * 8u;
    chunk = std::max(chunk, own_at - o + own);
    chunk = std::max(chunk, (8u + 3u * (uint32_t)D.nF) * 8u);                         // stage 1b: wave counts, feature means, limits, floors (MEMBER)
    o = up16(o + chunk);
    c.off_hist = o;
    const uint32_t bmax = (uint32_t)std::max(1.0, std::floor(std::sqrt((double)nmax)));
    const uint32_t table = up16(bmax * bmax * 4u), row = bmax * 4u;
    uint32_t band = o < generic::kLdsBudget ? std::min(table, (generic::kLdsBudget - o) & ~15u) : 0u;
    if (band < row) band = up16(row); // does not fit: total says so
    c.band_words = band / 4u;
    o += band;
    c.off_red4 = own_at + up16(own);
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
    const double *member;  // MEMBER: mult[RPF_MAX_NDIM] | floor[RPF_MAX_NDIM]; the other instantiations do not read it
};

// One workgroup filters one pixel at a time and walks the pixels of rows [row_begin, row_end), or those of p.pix_list.
// FAST (RPF_FLAG_STREAM_FAST): stage 4 alone in the fp32 arithmetic of DESIGN.md section 11f; every other statement is shared.
// MEMBER (RPF_FLAG_MEMBER_TEST, the rest list of route 9): stage 1b alone under the two-compare test of DESIGN.md section 14.
template <class T, bool FAST = false, bool MEMBER = false>
__global__ __launch_bounds__(256) void filter_wide_kernel(PassParams p, GenericWideCarve cv, WideScratch gs) {
    constexpr bool kMemberTest = MEMBER;
    constexpr bool kListed = false; // (this kernel always walks the box: the listed stage 1b is generic::filter_pixel_kernel's alone)
    extern __shared__ __align__(16) unsigned char smem[];
    const GenericDims D = generic_dims(p.lay);
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
    using Bin = uint16_t;
    Bin *bins = gs.bins + (uint64_t)blockIdx.x * ndim * p.nmax;
    const uint64_t *tw = gs.table;
    const double *mtab = gs.member;
    const double e_eps = (p.policy == RPF_DEGEN_EPS) ? p.eps : 0.0;

    const uint32_t npix = p.pix_list ? (gs.count_dev ? *gs.count_dev : p.list_count) : (uint32_t)(p.row_end - p.row_begin) * (uint32_t)W;
    for (uint32_t e = blockIdx.x; e < npix; e += gridDim.x) {
        const uint64_t pix = p.pix_list ? (uint64_t)p.pix_list[e] : (uint64_t)p.row_begin * W + e;
        const int y = (int)(pix / (uint32_t)W), x = (int)(pix - (uint64_t)y * W);
        __syncthreads(); // the previous pixel's LDS is dead

        // ---- stages 1b, 2, 3a: member list, in-order sums and column constants, 16-bit bin ids, debug hashes ----------------
#define RPF_STREAM_PART 1
#include "rpf_generic_stream_stages.inc"

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

        // ---- stages 3c, 4: alpha, beta, W_r_c; weights and blend (fp64, or the fp32 pair arithmetic of FAST); the status report
#define RPF_STREAM_PART 2
#include "rpf_generic_stream_stages.inc"
        if constexpr (FAST) {
#define RPF_STREAM_PART 4
#include "rpf_generic_stream_stages.inc"
        } else {
#define RPF_STREAM_PART 3
#include "rpf_generic_stream_stages.inc"
        }
    }
}

template <class T, bool FAST, bool MEMBER = false>
hipError_t launch_filter_wide_t(const PassParams &p, const GenericWideCarve &cv, const WideScratch &gs, unsigned grid, hipStream_t s) {
    hipError_t e = hipFuncSetAttribute((const void *)filter_wide_kernel<T, FAST, MEMBER>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cv.total);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((filter_wide_kernel<T, FAST, MEMBER>), dim3(grid), dim3(kThreads), cv.total, s, p, cv, gs);
    return hipGetLastError();
}

} // namespace

hipError_t launch_filter_wide(const PassParams &p, void *list, void *bins, uint32_t slots, const uint64_t *table, int table_bits,
                              const uint32_t *count_dev, hipStream_t s, bool fast, const double *member) {
    const GenericWideCarve cv = generic_wide_carve(p.lay, p.nmax, fast);
    if ((int)cv.total > max_lds_per_block() || cv.total > kLdsBudget) return hipErrorInvalidValue;
    if (p.nmax < 1 || p.nmax > kMaxWideNbhd || (count_dev != nullptr && p.pix_list == nullptr)) return hipErrorInvalidValue;
    if (member != nullptr && fast) return hipErrorInvalidValue; // (the membership test is fp64 only: no such instantiation)
    if (cv.band_words < (uint32_t)std::max(1.0, std::floor(std::sqrt((double)p.nmax)))) return hipErrorInvalidValue; // a band holds a row of the widest table
    if (p.row_end <= p.row_begin) return hipSuccess;
    if (p.pix_list != nullptr && count_dev == nullptr && p.list_count == 0) return hipSuccess;
    if (list == nullptr || bins == nullptr || table == nullptr || slots == 0) return hipErrorInvalidValue;
    const uint64_t npix = p.pix_list ? (count_dev ? (uint64_t)slots : (uint64_t)p.list_count) : (uint64_t)(p.row_end - p.row_begin) * p.W;
    const unsigned grid = (unsigned)std::min<uint64_t>(npix, slots);
    WideScratch gs;
    gs.list = (uint32_t *)list; gs.bins = (uint16_t *)bins; gs.table = table; gs.bits = table_bits; gs.count_dev = count_dev;
    gs.member = member;
    if (member != nullptr) return p.lay.f16 ? launch_filter_wide_t<__half, false, true>(p, cv, gs, grid, s) : launch_filter_wide_t<float, false, true>(p, cv, gs, grid, s);
    if (fast) return p.lay.f16 ? launch_filter_wide_t<__half, true>(p, cv, gs, grid, s) : launch_filter_wide_t<float, true>(p, cv, gs, grid, s);
    return p.lay.f16 ? launch_filter_wide_t<__half, false>(p, cv, gs, grid, s) : launch_filter_wide_t<float, false>(p, cv, gs, grid, s);
}

} // namespace generic
} // namespace rpf
