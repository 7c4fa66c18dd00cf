// rpf_generic.hip -- the layout-generic kernel pair: n_random and n_feat are run-time values (PassParams::lay), the only
// template parameter is the storage type of the feature planes.  Compiled with -ffp-contract=off like every kernel TU.
//
// filter_pixel_kernel is the streaming kernel of every layout: 256 threads filter one pixel whatever its neighbourhood size
// (N <= 65535).  It has three callers (rpf_api.hip): the whole pass under RPF_FLAG_GENERIC (rpf_query_route 3: the rows of the
// slab); the last size class of the size-binned route (N > 3136: that class's pixel list); and, under REF_ABORT, the redo list
// of the compiled kernels (list size read on the device).
//
// The arithmetic follows the reference statement by statement: reference order of the member list, strict a >= b rejection,
// in-order sums, one-byte bin ids, 16-bit histogram cells, MI from the 2^-44 k ln k table, the reference's own floating-point
// expression for in-band tables under REF_ABORT (evaluated in place), three exps multiplied.  The layout (DESIGN.md section
// 11): every column count is a loop bound and the LDS carve-up comes from the host; the x and x*x chains of column c sit on
// lane c of waves 0 and 1; stage 4 runs its column loop outermost, so no per-thread array is indexed by a run-time column;
// stage 1b always runs its own 3-sigma test (PassParams::masks is not read); member list and bin ids live in LDS when
// generic_carve says they fit, else in one HBM slot per workgroup.
#include "rpf_generic_common.h"

#include <algorithm>
#include <cmath>

namespace rpf {

namespace generic {
namespace {
constexpr uint32_t kResidentBytes = 40u << 10; // member list + bin ids stay in LDS up to this many bytes
constexpr uint32_t kHistParBytes = 32u << 10;  // one histogram per wave while the four stay within this many bytes
} // namespace
} // namespace generic

// The LDS carve-up of the generic filter kernel, a function of the layout and the neighbourhood capacity only:
//   doubles: M | SD | min | max [4 ndim], lo | range | flags [3 ndim], sum T[hx] [ndim], pair sums / MI [npair],
//            Drf | D9 | alpha | beta | wrc [2 nF + 20], reduction scratch [256]
//   chunk:   the staging chunk of the in-order sums [ndim][65]; later the marginals + need flags, then the own rows of stage 4
//   hist:    joint histograms, 16-bit cells, floor(sqrt(nmax))^2 each: one per wave while four stay within kHistParBytes
//            (each wave then builds the tables of its own pairs, no workgroup barrier), else one for the workgroup
//   red4:    stage 4's reduction scratch [4][256] doubles: behind the own rows, over the dead rest of chunk and hist
//   list | bins: u32 member list [nmax] and bin ids [ndim][nmax], when resident
// fast: the launch of filter_pixel_kernel<T, true>, whose own rows are kStreamFastOwn floats per weighted column, read 16 bytes
// at a time: they start at up16(off_chunk) (off_chunk is a multiple of 8 only: npair may be odd)
GenericCarve generic_carve(const SampleLayout &lay, int nmax, bool fast) {
    const GenericDims D = generic_dims(lay);
    GenericCarve c{};
    uint32_t o = (generic_f64_doubles(D) + generic::kThreads) * 8u;
    c.off_chunk = o;
    uint32_t chunk = (uint32_t)D.ndim * (generic::kChunk + 1) * 8u;
    chunk = std::max(chunk, 2048u + (uint32_t)D.npair * 4u);      // sMargX | sMargY | sNeed
    const uint32_t own_at = fast ? up16(o) : o;                   // where the own rows of a sweep start
    const uint32_t own = fast ? (uint32_t)generic::kStreamFastOwn * (uint32_t)D.nwt * 4u : (uint32_t)generic::kOwn * (uint32_t)D.nwt * 8u;
    chunk = std::max(chunk, own_at - o + own);
    chunk = std::max(chunk, (8u + 2u * (uint32_t)D.nF) * 8u);     // stage 1b: wave counts, feature means, 3 sigma
    o = up16(o + chunk);
    c.off_hist = o;
    const uint32_t bmax = (uint32_t)std::sqrt((double)nmax);
    const uint32_t hist = up16(((bmax * bmax + 1u) / 2u) * 4u);
    c.hist_par = 4u * hist <= generic::kHistParBytes ? 4u : 1u;
    c.hist_words = hist / 4u;
    o += c.hist_par * hist;
    c.off_red4 = own_at + up16(own);
    o = std::max(o, c.off_red4 + 4u * generic::kThreads * 8u);
    const uint64_t members = (uint64_t)nmax * (4u + (uint32_t)D.ndim);
    c.resident = members <= generic::kResidentBytes ? 1u : 0u;
    if (c.resident) {
        c.off_list = o; o += up16((uint32_t)nmax * 4u);
        c.off_bins = o; o += up16((uint32_t)nmax * (uint32_t)D.ndim);
    }
    c.total = o;
    return c;
}

namespace generic {
namespace {

struct Scratch {
    uint32_t *list; // [slots][nmax]        member list (plane offsets), reference order (spilled mode)
    uint8_t *bins;  // [slots][ndim][nmax]  bin ids
    const uint32_t *count_dev; // the size of p.pix_list lives in device memory (redo list: no host read-back), else null
};

// stage 1a: per-pixel mean / std of the nF features over the pixel's own S samples, sequential sums (rpf.cpp:338-347,
// ops.h:111-144): the chains of pixel_stats_kernel with nF as a loop bound.  Output planes [nF][H*W].
template <class T>
__global__ __launch_bounds__(256) void pixel_stats_kernel(PassParams p, uint64_t pix0, uint64_t pix1) {
    const uint64_t HW = (uint64_t)p.H * p.W;
    const uint64_t pix = pix0 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= pix1) return;
    const double dn = (double)p.S;
    const int nF = p.lay.nF, colF = 5 + p.lay.nR;
    for (int k = 0; k < nF; ++k) {
        const T *src = reinterpret_cast<const T *>(p.planes) + (uint64_t)(colF + k) * p.plane_stride + pix * p.S;
        double sum = 0.0, sq = 0.0;
        for (int s = 0; s < p.S; ++s) {
            const double v = (double)(float)src[s];
            sum = sum + v;     // ops.h:121
            sq = sq + v * v;   // ops.h:138 (v*v is exact for fp32-valued v)
        }
        double mean, sd;
        column_mean_sd(sum, sq, dn, p.policy, mean, sd);
        ((double *)p.pmean)[(uint64_t)k * HW + pix] = mean;
        ((double *)p.pstd)[(uint64_t)k * HW + pix] = sd;
    }
}

// One workgroup filters one pixel at a time and walks the pixels of rows [row_begin, row_end) or, when p.pix_list is given,
// the entries of that list (*gs.count_dev of them when that is given, else p.list_count).
// FAST (RPF_FLAG_STREAM_FAST): stage 4 alone in the fp32 arithmetic of DESIGN.md section 11f; every other statement is shared.
// LISTED (the rest launch of a sampled pass, RPF_FLAG_SAMPLED_REST): stage 1b alone reads N from p.nbhd and the
// members behind the own samples from p.members / p.member_base instead of walking the box; every other statement is shared.
template <class T, bool FAST = false, bool LISTED = false>
__global__ __launch_bounds__(256) void filter_pixel_kernel(PassParams p, GenericCarve cv, Scratch gs) {
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
    uint32_t *sHist = reinterpret_cast<uint32_t *>(smem + cv.off_hist);
    double *sRed4 = reinterpret_cast<double *>(smem + cv.off_red4);   // [4][256] stage 4 (chunk and histogram are dead there)
    int *sCnt = reinterpret_cast<int *>(sChunk);                      // stage 1b: per-wave counts (the chunk is not live yet)

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int W = p.W, H = p.H, S = p.S, b = p.b;
    const uint64_t HW = (uint64_t)H * W;
    uint32_t *list = cv.resident ? reinterpret_cast<uint32_t *>(smem + cv.off_list) : gs.list + (uint64_t)blockIdx.x * p.nmax;
    using Bin = uint8_t;
    Bin *bins = cv.resident ? smem + cv.off_bins : gs.bins + (uint64_t)blockIdx.x * ndim * p.nmax;
    const double e_eps = (p.policy == RPF_DEGEN_EPS) ? p.eps : 0.0;
    constexpr bool kMemberTest = false;         // (RPF_FLAG_MEMBER_TEST never reaches this kernel: the stage text's statements
    constexpr const double *mtab = nullptr;     //  under it are discarded, and the assembly is what it was)
    constexpr bool kListed = LISTED;

    const uint32_t npix = p.pix_list == nullptr ? (uint32_t)(p.row_end - p.row_begin) * (uint32_t)W
                                                : (gs.count_dev != nullptr ? *gs.count_dev : p.list_count);
    for (uint32_t e = blockIdx.x; e < npix; e += gridDim.x) {
        const uint64_t pix = p.pix_list == nullptr ? (uint64_t)p.row_begin * W + e : (uint64_t)p.pix_list[e];
        const int y = (int)(pix / (uint32_t)W), x = (int)(pix - (uint64_t)y * W);
        __syncthreads(); // the previous pixel's LDS is dead

        // ---- stages 1b, 2, 3a: member list, in-order sums and column constants, one-byte bin ids, debug hashes --------------
#define RPF_STREAM_PART 1
#include "rpf_generic_stream_stages.inc"

        // ---- stage 3b: histograms, 16-bit cells packed two per word (counts <= N < 65536) ------------------------------
        auto hist_T = [&](const uint8_t *ba, const uint8_t *bb, int cells) -> uint64_t { // sum over cells of T[count]
            for (int t = tid; t < (cells + 1) / 2; t += kThreads) sHist[t] = 0u;
            __syncthreads();
            for (int j = tid; j < n; j += kThreads) {
                const uint32_t cell = ba ? (uint32_t)ba[j] * (uint32_t)B + bb[j] : bb[j];     // mi.cpp:39
                atomicAdd(&sHist[cell >> 1], 1u << (16u * (cell & 1u)));
            }
            __syncthreads();
            uint64_t acc = 0ull;
            for (int t = tid; t < cells; t += kThreads) acc += p.tfix[(sHist[t >> 1] >> (16u * (t & 1u))) & 0xffffu];
            return block_reduce(acc, reinterpret_cast<uint64_t *>(sRedD), [](uint64_t a, uint64_t b2) { return a + b2; });
        };
        if (cv.hist_par > 1) {
            // a histogram per wave: wave w builds tables w, w + 4, ... (the ndim marginal tables, then the pairs) on its own --
            // one wave's LDS operations execute in order, so no workgroup barrier, and the waves' table look-ups overlap
            uint32_t *h = sHist + (uint32_t)wv * cv.hist_words;
            for (int tb = wv; tb < ndim + npair; tb += kThreads / 64) {
                const uint8_t *ba = nullptr, *bb;
                int cells = B;
                if (tb < ndim) {
                    bb = bins + (uint64_t)tb * p.nmax;
                } else {
                    int ca, cb;
                    pair_cols(D, tb - ndim, ca, cb);
                    ba = bins + (uint64_t)ca * p.nmax; bb = bins + (uint64_t)cb * p.nmax;
                    cells = B * B;
                }
                for (int t = lane; t < (cells + 1) / 2; t += 64) h[t] = 0u;
                wsync();
                for (int j = lane; j < n; j += 64) {
                    const uint32_t cell = ba ? (uint32_t)ba[j] * (uint32_t)B + bb[j] : bb[j];     // mi.cpp:39
                    atomicAdd(&h[cell >> 1], 1u << (16u * (cell & 1u)));
                }
                wsync();
                uint64_t acc = 0ull;
                for (int t = lane; t < cells; t += 64) acc += p.tfix[(h[t >> 1] >> (16u * (t & 1u))) & 0xffffu];
                for (int s = 32; s > 0; s >>= 1) acc += __shfl_down(acc, s, 64);
                if (lane == 0) { if (tb < ndim) sHX[tb] = acc; else sPair[tb - ndim] = acc; }
                wsync();
            }
        } else {
            for (int c = 0; c < ndim; ++c) {
                const uint64_t t = hist_T(nullptr, bins + (uint64_t)c * p.nmax, B);
                if (tid == 0) sHX[c] = t;
            }
            for (int pr = 0; pr < npair; ++pr) {
                int ca, cb;
                pair_cols(D, pr, ca, cb);
                const uint64_t t = hist_T(bins + (uint64_t)ca * p.nmax, bins + (uint64_t)cb * p.nmax, B * B);
                if (tid == 0) sPair[pr] = t;
            }
        }
        __syncthreads();
        uint32_t *sMargX = reinterpret_cast<uint32_t *>(sChunk), *sMargY = sMargX + 256; // (the staging chunk is not live here)
        int *sNeed = reinterpret_cast<int *>(sMargY + 256);                               // [npair]
        {
            const int64_t TNf = (int64_t)p.tfix[n];
            const int64_t zero_band = ((int64_t)B * B + 2 * B + 1) / 2 + 1;   // see filter_pixel_kernel (rpf_filter_impl.inc)
            for (int pr = tid; pr < npair; pr += kThreads) {
                int ca, cb;
                pair_cols(D, pr, ca, cb);
                int64_t f = TNf + (int64_t)sPair[pr] - (int64_t)sHX[ca] - (int64_t)sHX[cb];
                int need = 0;
                if (f <= zero_band && f >= -zero_band) {
                    // REF_ABORT: the reference's own value for such a table is rounding residue unless its quotients are
                    // exact (N a power of two, or a one-bin column): evaluated below, term by term
                    need = p.policy == RPF_DEGEN_REF_ABORT && (n & (n - 1)) != 0 && (int64_t)sHX[ca] != TNf && (int64_t)sHX[cb] != TNf;
                    f = 0;
                }
                sNeed[pr] = need;
                const double mi = ldexp((double)f, -kTFixBits) / dn;
                sMI[pr] = mi; // (same slot as sPair[pr]: each thread overwrites only what it has just read)
                if (p.dbg.mi) p.dbg.mi[pix * npair + pr] = mi;
            }
        }
        __syncthreads();
        // ---- the reference expression for tables inside the rounding band (REF_ABORT): mi.cpp:66-86 on the integer counts,
        // same operations in the same cell order, with log(1 +- k ulp) as the host's libm returns it (rpf_reflog.h)
        if (p.policy == RPF_DEGEN_REF_ABORT) {
            for (int pr = 0; pr < npair; ++pr) {
                if (!sNeed[pr]) continue; // workgroup-uniform
                int ca, cb;
                pair_cols(D, pr, ca, cb);
                const uint8_t *ba = bins + (uint64_t)ca * p.nmax, *bb = bins + (uint64_t)cb * p.nmax;
                const int cells = B * B;
                __syncthreads();
                for (int t = tid; t < (cells + 1) / 2; t += kThreads) sHist[t] = 0u;
                for (int t = tid; t < 512; t += kThreads) sMargX[t] = 0u; // both marginals
                __syncthreads();
                for (int j = tid; j < n; j += kThreads) {
                    const uint32_t bx = ba[j], by = bb[j], cell = bx * (uint32_t)B + by;       // mi.cpp:39
                    atomicAdd(&sHist[cell >> 1], 1u << (16u * (cell & 1u)));
                    atomicAdd(&sMargX[bx], 1u);                                                 // mi.cpp:17
                    atomicAdd(&sMargY[by], 1u);
                }
                __syncthreads();
                double mi = 0.0; // thread 0's running sum
                for (int t0 = 0; t0 < cells; t0 += kThreads) {
                    const int t = t0 + tid;
                    double term = 0.0;
                    if (t < cells) {
                        const int i = t / B, j = t - i * B;
                        const double pX = (double)sMargX[i] / dn, pY = (double)sMargY[j] / dn;  // mi.cpp:70-75
                        const double pXY = (double)((sHist[t >> 1] >> (16u * (t & 1u))) & 0xffffu) / dn; // mi.cpp:81
                        const double pp = pX * pY;                                              // mi.cpp:82
                        if (pXY > 0 && pp != 0) {
                            const double q = pXY / pp;
                            term = pXY * (reflog_in_range(q) ? reflog_near_one(q) : log(q));    // mi.cpp:84
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

template <class T, bool FAST, bool LISTED>
hipError_t launch_filter_t(const PassParams &p, const GenericCarve &cv, const Scratch &gs, unsigned grid, hipStream_t s) {
    hipError_t e = hipFuncSetAttribute((const void *)filter_pixel_kernel<T, FAST, LISTED>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cv.total);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((filter_pixel_kernel<T, FAST, LISTED>), dim3(grid), dim3(kThreads), cv.total, s, p, cv, gs);
    return hipGetLastError();
}

} // namespace

hipError_t launch_pixel_stats(const PassParams &p, uint64_t pix0, uint64_t pix1, hipStream_t s) {
    if (pix1 <= pix0) return hipSuccess;
    const dim3 grid((unsigned)((pix1 - pix0 + 255) / 256));
    if (p.lay.f16) hipLaunchKernelGGL(pixel_stats_kernel<__half>, grid, dim3(256), 0, s, p, pix0, pix1);
    else hipLaunchKernelGGL(pixel_stats_kernel<float>, grid, dim3(256), 0, s, p, pix0, pix1);
    return hipGetLastError();
}

// list / bins: the HBM slots of the spilled mode ([slots][nmax] u32, [slots][ndim][nmax] u8), unused when the carve-up is
// resident; the grid never exceeds `slots`: min(pixels, slots), or `slots` when the list size is on the device.  listed: the
// LISTED instantiation over p.pix_list, fp64 only (p.nbhd, p.members and p.member_base as a count kernel of the member pool left them)
hipError_t launch_filter(const PassParams &p, void *list, void *bins, uint32_t slots, const uint32_t *count_dev, hipStream_t s, bool fast,
                         bool listed) {
    if (listed && (fast || p.members == nullptr || p.member_base == nullptr || p.pix_list == nullptr || count_dev != nullptr)) return hipErrorInvalidValue;
    const GenericCarve cv = generic_carve(p.lay, p.nmax, fast);
    if ((int)cv.total > max_lds_per_block()) return hipErrorInvalidValue;
    if (p.row_end <= p.row_begin) return hipSuccess;
    const uint64_t npix = p.pix_list == nullptr ? (uint64_t)(p.row_end - p.row_begin) * p.W : p.list_count;
    if (!cv.resident && (list == nullptr || bins == nullptr)) return hipErrorInvalidValue;
    const unsigned grid = p.pix_list != nullptr && count_dev != nullptr ? slots : (unsigned)std::min<uint64_t>(npix, slots);
    if (grid == 0) return hipSuccess;
    Scratch gs;
    gs.list = (uint32_t *)list; gs.bins = (uint8_t *)bins; gs.count_dev = count_dev;
    if (listed) return p.lay.f16 ? launch_filter_t<__half, false, true>(p, cv, gs, grid, s) : launch_filter_t<float, false, true>(p, cv, gs, grid, s);
    if (fast) return p.lay.f16 ? launch_filter_t<__half, true, false>(p, cv, gs, grid, s) : launch_filter_t<float, true, false>(p, cv, gs, grid, s);
    return p.lay.f16 ? launch_filter_t<__half, false, false>(p, cv, gs, grid, s) : launch_filter_t<float, false, false>(p, cv, gs, grid, s);
}

} // namespace generic
} // namespace rpf
