// rpf_generic_wave.hip -- the layout-generic one-wave kernels of mid-sized neighbourhoods (RPF_FLAG_GENERIC |
// RPF_FLAG_GENERIC_PACKED | RPF_FLAG_GENERIC_WAVE, rpf_query_route 5): n_random and n_feat are run-time values
// (PassParams::lay), the class capacity (128, 256, 448 or 832 samples) is a kernel argument, the only template parameter is
// the storage type of the feature planes.  Compiled with -ffp-contract=off like every kernel TU.
//
// filter_wave_kernel<T>: one wave64 filters one pixel of the class list (64 < N <= capacity) from start to end.  A workgroup
// holds up to four such waves (generic_wave_carve: as many as fit 160 KiB), which share T[0 .. capacity] and the column table
// of the MI pairs and are independent after that one barrier: one wave's LDS operations execute in order, so wsync() is all
// the hand-over between its lanes needs.  Against generic::filter_pixel_kernel (four waves and a workgroup barrier at every
// step, whatever N): no barrier; the member list comes from the count pass's acceptance masks, or from the members a wide
// pass's count kernel listed (p.members), with no second 3-sigma test; a
// member's columns are gathered once for both chains and the column minima / maxima, once for the bin ids and once per sweep
// of stage 4 (four own samples), where a column's value is normalised once per sweep; the four sums of an own sample are
// totalled across the 64 lanes by the all-reduce of rpf_xlane.h.
//
// The arithmetic is generic::filter_pixel_kernel's, statement by statement: reference order of the member list, in-order
// sums of x and x * x (one lane per column), sd == 0 -> z = 0, B = max(1, (int)sqrt(N)), bin ids by IEEE quotients, 16-bit
// histogram cells, MI from the 2^-44 k ln k table with the same zero band, the beta presets by the stack rule of DESIGN.md
// section 11, three exps multiplied.  Every stage output up to alpha / beta / W_r_c is the same bits as route 3's; the
// colours agree to rounding (the weight sums of stage 4 associate differently).  Under REF_ABORT a pixel with a table inside
// the zero band at a non-power-of-two N and non-degenerate marginals joins the redo list (the rule of
// rpf_generic_packed.hip) and generic::filter_pixel_kernel filters it again, whole.
//
// filter_wave_kernel<T, FAST = true> (RPF_FLAG_GENERIC_FAST): the same kernel with stage 4 in fp32 -- a
// member's z = (x - M) * (1 / SD) in fp64 with 1 / SD formed once per pixel and column, rounded once; the coefficients (log2 e
// folded in) formed in fp64 and rounded once; one accumulator per own sample, two own samples per packed fp32 instruction, one
// hardware exponential, the sums and the quotient in fp64.  Every statement outside stage 4 is shared.
#include "rpf_generic_common.h"

#include <algorithm>
#include <cmath>

namespace rpf {

namespace generic {
namespace {
constexpr int kWvChunk = 64; // members staged per step of the in-order sums
constexpr int kWvHist = 4;   // histograms a wave fills together (xl::reduce4 totals their sums)
constexpr int kWvGather = 4; // columns of a member gathered together (their latencies overlap; a register each, no run-time index)
// own samples per sweep of stage 4 (their accumulators are registers; same bits at any value).  Eight need 299 registers
// (256 VGPRs + 43 AGPRs: one wave per SIMD), four need 209: two waves per SIMD
#ifndef RPF_WAVE_OWN
#define RPF_WAVE_OWN 4
#endif
constexpr int kWvOwn = RPF_WAVE_OWN;
// ... under RPF_FLAG_GENERIC_FAST (an even number: two own samples share a packed fp32 instruction; the sweep's own rows are
// floats, so eight fit the LDS block that holds four fp64 rows; DESIGN.md section 11e has the trial of 4 against 8)
#ifndef RPF_WAVE_FAST_OWN
#define RPF_WAVE_FAST_OWN 8
#endif
constexpr int kWvFastOwn = RPF_WAVE_FAST_OWN;
static_assert(kWvFastOwn % 4 == 0 && kWvFastOwn * 4 <= kWvOwn * 8, "the fp32 own rows of a sweep fit the block of the fp64 ones; read 16 bytes at a time");
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4a __attribute__((ext_vector_type(4), may_alias));
} // namespace
} // namespace generic

GenericWaveCarve generic_wave_carve(const SampleLayout &lay, int capacity) {
    const GenericDims D = generic_dims(lay);
    const uint32_t ndim = (uint32_t)D.ndim, npair = (uint32_t)D.npair, cap = (uint32_t)capacity;
    GenericWaveCarve c{};
    c.capacity = cap;
    c.off_pairtab = up16((cap + 1u) * 8u);           // behind T[0 .. capacity]
    c.table_bytes = up16(c.off_pairtab + 2u * npair);
    uint32_t o = up16(cap * 4u);                     // member list
    // one block for the staging chunk (stage 2), the bin ids (stages 3a, 3b) and the own rows of a sweep (stage 4): never
    // live together, and held apart they cost a CU half of its resident waves at 19 dims
    c.off_bins = o; c.off_chunk = o;
    uint32_t shared = ndim * (uint32_t)(generic::kWvChunk + 1) * 8u;
    shared = std::max(shared, ndim * cap);
    shared = std::max(shared, (uint32_t)generic::kWvOwn * (uint32_t)D.nwt * 8u);
    o += up16(shared);
    c.off_hist = o;
    const uint32_t bmax = (uint32_t)std::sqrt((double)cap);
    o += up16((uint32_t)generic::kWvHist * ((bmax * bmax + 1u) / 2u) * 4u);
    c.off_stat = o;
    o += generic_f64_doubles(D) * 8u;                    // M | SD | min | max, lo | range | flags, sum T[hx], pair sums / MI, weights
    c.off_flag = o; o += 16u;
    c.wave_bytes = up16(o);
    const uint32_t lds = (uint32_t)max_lds_per_block();
    const uint32_t room = lds > c.table_bytes ? lds - c.table_bytes : 0u;
    // waves per workgroup: of the one to four that fit, the count that lets a CU hold the most waves (a workgroup of four
    // that leaves room for half a second one wastes it); the larger count on a tie (fewer copies of the tables)
    c.waves = 0u;                                    // (0: the layout does not fit; launch_filter_wave refuses it)
    uint32_t best = 0u;
    for (uint32_t w = 1u; w <= 4u && w * c.wave_bytes <= room; ++w) {
        const uint32_t per_cu = std::min(8u, lds / (c.table_bytes + w * c.wave_bytes) * w); // (8: two waves per SIMD, by registers)
        if (per_cu >= best) { best = per_cu; c.waves = w; }
    }
    c.total = c.table_bytes + c.waves * c.wave_bytes;
    return c;
}

namespace generic {
namespace {

// One wave = one pixel of the class list at a time, the entries dealt to the waves of the grid with a grid stride.
// FAST (RPF_FLAG_GENERIC_FAST): stage 4 alone in the fp32 arithmetic of DESIGN.md section 11e; every other statement is shared.
template <class T, bool FAST = false>
__global__ __launch_bounds__(256) void filter_wave_kernel(PassParams p, GenericWaveCarve cv) {
    constexpr int kOwn = FAST ? kWvFastOwn : kWvOwn;
    extern __shared__ __align__(16) unsigned char smem[];
    const GenericDims D = generic_dims(p.lay);
    const int ndim = D.ndim, nF = D.nF, nR = D.nR, nAnc = D.nAnc, npair = D.npair, nwt = D.nwt, colF = D.colF;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nthreads = (int)blockDim.x;
    const int cap = (int)cv.capacity;
    uint64_t *sT = reinterpret_cast<uint64_t *>(smem);
    for (int k = tid; k <= cap; k += nthreads) sT[k] = p.tfix[min(k, p.nmax)];
    uint16_t *sPairTab = reinterpret_cast<uint16_t *>(smem + cv.off_pairtab);
    for (int pr = tid; pr < npair; pr += nthreads) {
        int ca, cb;
        pair_cols(D, pr, ca, cb);
        sPairTab[pr] = (uint16_t)(ca | (cb << 8));
    }
    __syncthreads(); // the only barrier: from here on the waves are independent
    unsigned char *wb = smem + cv.table_bytes + (uint32_t)wv * cv.wave_bytes;
    uint32_t *list = reinterpret_cast<uint32_t *>(wb);                                  // [cap] plane offsets, reference order
    uint8_t *bins = wb + cv.off_bins;                                                   // [ndim][cap]
    uint32_t *sHist = reinterpret_cast<uint32_t *>(wb + cv.off_hist);                   // 16-bit cells, two per word
    double *sChunk = reinterpret_cast<double *>(wb + cv.off_chunk);                     // [ndim][kWvChunk + 1]
    double *sStat = reinterpret_cast<double *>(wb + cv.off_stat);                       // M | SD | xmin | xmax
    double *sZ = sStat + 4 * ndim;                                                      // lo | range | flags(sd0 | flat << 1)
    uint64_t *sHX = reinterpret_cast<uint64_t *>(sZ + 3 * ndim);                        // sum_i T[hx_i] per column
    uint64_t *sPair = sHX + ndim;                                                       // sum_ij T[J_ij] per pair, then the MI values
    double *sMI = reinterpret_cast<double *>(sPair);
    double *sW = sMI + npair;                                                           // Drf[nF] | D9[12] | alpha[4] | beta[nF] | wrc[4]
    int *sFlag = reinterpret_cast<int *>(wb + cv.off_flag);                             // redo

    const int W = p.W, H = p.H, S = p.S, b = p.b;
    const double e_eps = (p.policy == RPF_DEGEN_EPS) ? p.eps : 0.0;
    const uint32_t nwaves = (uint32_t)nthreads >> 6;
    for (uint32_t e = blockIdx.x * nwaves + (uint32_t)wv; e < p.list_count; e += gridDim.x * nwaves) {
        wsync(); // the previous pixel's LDS is dead
        const uint32_t pixu = p.pix_list[e];
        const uint64_t pix = pixu;
        const int y = (int)(pixu / (uint32_t)W), x = (int)(pixu - (uint32_t)y * (uint32_t)W);
        const int n = min(p.nbhd[pixu], cap); // <= cap by construction of the list

        // ---- stage 1b: the member list from the acceptance masks of the count pass, reference order (rpf.cpp:556-586) ----
        const int x0 = max(x - b, 0), x1 = min(x + b, W - 1), y0 = max(y - b, 0), y1 = min(y + b, H - 1);
        const int nyv = y1 - y0 + 1;
        const int centre_rank = (x - x0) * nyv + (y - y0);
        const int ncand = ((x1 - x0 + 1) * nyv - 1) * S;
        for (int s = lane; s < min(S, cap); s += 64) list[s] = (uint32_t)(pix * S + s); // own samples first
        if (lane == 0) sFlag[0] = 0;
        if (p.members != nullptr) { // (uniform) the listed members of a wide pass's count kernel, already in that order
            const uint32_t *src = p.members + p.member_base[pix];
            for (int j = S + lane; j < n; j += 64) list[j] = src[j - S];
        } else {
            const int nwords = min((ncand + 63) >> 6, (int)p.mask_stride);
            const uint64_t *pm = p.masks + pix * p.mask_stride;
            int base = S;
            for (int w = 0; w < nwords; ++w) {
                const unsigned long long mask = pm[w]; // wave-uniform
                if (mask == 0ull) continue;
                if ((mask >> lane) & 1ull) {
                    const int qq = w * 64 + lane;
                    int cell = qq / S;
                    const int s = qq - cell * S;
                    if (cell >= centre_rank) ++cell;              // rpf.cpp:565: skip the centre pixel
                    const int ix = cell / nyv, iy = cell - ix * nyv; // xn outer, yn inner ascending (rpf.cpp:562-563)
                    const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
                    if (at < cap) list[at] = (uint32_t)(((uint64_t)(y0 + iy) * W + (x0 + ix)) * S + s);
                }
                base += __popcll(mask);
            }
        }
        wsync();
        const int B = max(1, (int)sqrt((double)n));                // mi.cpp:54
        const double dn = (double)n;
        const int nk = (n + 63) >> 6;                              // members per lane: j = lane + 64 kk

        // ---- stage 2: in-order sums over the neighbourhood (rpf.cpp:596-601), chunks of 64 staged through LDS: lane q
        // gathers the columns of member j0 + q, then lane c adds both chains of column c front to back; the column's minimum
        // and maximum ride along
        {
            double acc = 0.0, acc2 = 0.0, mn = INFINITY, mx = -INFINITY;
            for (int j0 = 0; j0 < n; j0 += kWvChunk) {
                const int cnt = min(kWvChunk, n - j0);
                if (lane < cnt) {
                    const uint32_t off = list[j0 + lane];
                    for (int c0 = 0; c0 < ndim; c0 += kWvGather) { // kWvGather gathers in flight, then their stores
                        double v[kWvGather];
#pragma unroll
                        for (int u = 0; u < kWvGather; ++u) v[u] = load_col<T>(p, min(c0 + u, ndim - 1), off);
#pragma unroll
                        for (int u = 0; u < kWvGather; ++u)
                            if (c0 + u < ndim) sChunk[(c0 + u) * (kWvChunk + 1) + lane] = v[u];
                    }
                }
                wsync();
                if (lane < ndim) {
                    const double *src = sChunk + lane * (kWvChunk + 1);
                    for (int q = 0; q < cnt; ++q) {
                        const double v = src[q];
                        acc = acc + v;                               // ops.h:121
                        acc2 = acc2 + v * v;                         // ops.h:138
                        mn = fmin(mn, v); mx = fmax(mx, v);
                    }
                }
                wsync();
            }
            // the per-column constants of the binning (sd.h:229-232, mi.cpp:47-50)
            if (lane < ndim) {
                const double mean = acc / dn;                        // ops.h:123
                double sd = sqrt(acc2 / dn - mean * mean);           // ops.h:141
                if (p.policy == RPF_DEGEN_EPS && isnan(sd)) sd = 0.0;
                sStat[lane] = mean; sStat[ndim + lane] = sd;
                sStat[2 * ndim + lane] = mn; sStat[3 * ndim + lane] = mx;
                if (p.dbg.mean) p.dbg.mean[pix * ndim + lane] = mean;
                if (p.dbg.stddev) p.dbg.stddev[pix * ndim + lane] = sd;
                const bool sd0 = (sd == 0.0);
                const double lo = sd0 ? 0.0 : (mn - mean) / sd, hi = sd0 ? 0.0 : (mx - mean) / sd;
                sZ[lane] = lo; sZ[ndim + lane] = hi - lo;
                sZ[2 * ndim + lane] = (double)((sd0 ? 1 : 0) | (!(hi != lo) ? 2 : 0)); // mi.cpp:7 / 28 / 34
            }
        }
        wsync();

        // ---- stage 3a: normalise, bin ids (one byte per sample and column); lane = member lane + 64 kk ------------------
        for (int kk = 0; kk < nk; ++kk) {
            const int j = lane + 64 * kk;
            if (j < n) {
                const uint32_t off = list[j];
                for (int c0 = 0; c0 < ndim; c0 += kWvGather) {
                    double v[kWvGather];
#pragma unroll
                    for (int u = 0; u < kWvGather; ++u) v[u] = load_col<T>(p, min(c0 + u, ndim - 1), off);
#pragma unroll
                    for (int u = 0; u < kWvGather; ++u) {
                        const int c = c0 + u;
                        if (c >= ndim) break;
                        const double Mc = sStat[c], SDc = sStat[ndim + c], lo = sZ[c], range = sZ[ndim + c];
                        const int flags = (int)sZ[2 * ndim + c];
                        const bool sd0 = flags & 1, flat = flags & 2;
                        int bin = 0;
                        if (!flat) {
                            const double a = v[u] - Mc;                                // subtractArrays
                            const double z = sd0 ? 0.0 : a / SDc;                      // divideArrays, ops.h:48
                            const double t = (z - lo) / range * (double)B;             // mi.cpp:14
                            bin = max(min((int)t, B - 1), 0);
                        }
                        bins[c * cap + j] = (uint8_t)bin;
                    }
                }
            }
        }
        wsync();
        if (p.dbg.member_hash != nullptr && lane == 0) {
            uint32_t h = 2166136261u;
            for (int j = 0; j < n; ++j) {
                const uint32_t o = list[j], s = o % (uint32_t)S, q = o / (uint32_t)S;
                const int yn = (int)(q / (uint32_t)W), xn = (int)(q % (uint32_t)W);
                h = fnv1a_u32(h, (uint32_t)(((xn - x + b) * p.box + (yn - y + b)) * S) + s);
            }
            p.dbg.member_hash[pix] = h;
        }
        if (p.dbg.bin_hash != nullptr && lane < ndim) {
            uint32_t h = 2166136261u;
            const uint8_t *bc = bins + lane * cap;
            for (int j = 0; j < n; ++j) h = fnv1a_u16(h, bc[j]);
            p.dbg.bin_hash[pix * ndim + lane] = h;
        }

        // ---- stage 3b: histograms, 16-bit cells packed two per word (counts <= N < 65536): the ndim marginal tables, then
        // the pairs, kWvHist tables at a time on this wave's histograms (their LDS round trips overlap; one transposed butterfly
        // totals the four sums)
        {
            const int ntab = ndim + npair;
            const int hs = (B * B + 1) / 2;                       // words of one histogram of this pixel
            for (int tb0 = 0; tb0 < ntab; tb0 += kWvHist) {
                int oa[kWvHist], ob[kWvHist], cells[kWvHist];     // (wave-uniform; indexed by unrolled loops only)
#pragma unroll
                for (int u = 0; u < kWvHist; ++u) {
                    const int tb = tb0 + u;
                    oa[u] = -1; ob[u] = 0; cells[u] = 0;          // a table past the last: no cell, nothing added
                    if (tb < ndim) {
                        ob[u] = tb * cap; cells[u] = B;
                    } else if (tb < ntab) {
                        const uint32_t cc = sPairTab[tb - ndim];
                        oa[u] = (int)(cc & 255u) * cap; ob[u] = (int)(cc >> 8) * cap; cells[u] = B * B;
                    }
                }
                for (int t = lane; t < kWvHist * hs; t += 64) sHist[t] = 0u;
                wsync();
                for (int kk = 0; kk < nk; ++kk) {
                    const int j = lane + 64 * kk;
                    if (j < n) {
#pragma unroll
                        for (int u = 0; u < kWvHist; ++u) {
                            if (cells[u] == 0) continue;
                            const uint32_t cell = oa[u] >= 0 ? (uint32_t)bins[oa[u] + j] * (uint32_t)B + bins[ob[u] + j] : bins[ob[u] + j]; // mi.cpp:39
                            atomicAdd(&sHist[u * hs + (int)(cell >> 1)], 1u << (16u * (cell & 1u)));
                        }
                    }
                }
                wsync();
                uint64_t acc[kWvHist];
#pragma unroll
                for (int u = 0; u < kWvHist; ++u) acc[u] = 0ull;
                for (int t = lane; t < B * B; t += 64) {
#pragma unroll
                    for (int u = 0; u < kWvHist; ++u)
                        if (t < cells[u]) acc[u] += sT[(sHist[u * hs + (t >> 1)] >> (16u * (t & 1u))) & 0xffffu];
                }
                const uint64_t tot = xl::reduce4<xl::OpSum>(acc); // the lane holds the total of table tb0 + slot4(lane)
                const int tb = tb0 + xl::slot4(lane);
                if ((lane & 15) == 0 && tb < ntab) { if (tb < ndim) sHX[tb] = tot; else sPair[tb - ndim] = tot; }
                wsync();
            }
        }
        bool redo = false;
        {
            const int64_t TNf = (int64_t)sT[n];
            const int64_t zero_band = ((int64_t)B * B + 2 * B + 1) / 2 + 1;   // see filter_pixel_kernel (rpf_filter_impl.inc)
            for (int pr = lane; pr < npair; pr += 64) {
                const uint32_t cc = sPairTab[pr];
                const int ca = (int)(cc & 255u), cb = (int)(cc >> 8);
                const int64_t hxa = (int64_t)sHX[ca], hxb = (int64_t)sHX[cb];
                int64_t f = TNf + (int64_t)sPair[pr] - hxa - hxb;
                if (f <= zero_band && f >= -zero_band) {
                    // REF_ABORT: the reference's own value for such a table is rounding residue unless its quotients are
                    // exact (N a power of two, or a one-bin column): generic::filter_pixel_kernel evaluates it (redo list)
                    if (p.redo_list != nullptr && (n & (n - 1)) != 0 && hxa != TNf && hxb != TNf) redo = true;
                    f = 0;
                }
                const double mi = ldexp((double)f, -kTFixBits) / dn;
                sMI[pr] = mi; // (same slot as sPair[pr]: each lane overwrites only what it has just read)
                if (p.dbg.mi) p.dbg.mi[pix * npair + pr] = mi;
            }
        }
        if (redo) sFlag[0] = 1;
        wsync();
        const bool redo_pixel = sFlag[0] != 0; // wave-uniform

        // ---- stage 3c: alpha, beta, W_r_c (rpf.cpp:444-487), the statements of generic::filter_pixel_kernel ----------------
        double *sDrf = sW, *sD9 = sDrf + nF, *sAlpha = sD9 + 12, *sBeta = sAlpha + 4, *sWrc = sBeta + nF;
        {
            const int k = min(lane, nF - 1), c = min(lane, 2);
            double Drf = 0.0, Dpf = 0.0, Dcf = 0.0, Drc = 0.0, Dpc = 0.0, Dfc = 0.0;
            const int base = D.npairF + c * D.npairC;
            for (int l = 0; l < nR; ++l) { Drf += sMI[k * nAnc + l]; Drc += sMI[base + l]; }                 // rpf.cpp:421, 432
            for (int l = 0; l < 2; ++l) { Dpf += sMI[k * nAnc + nR + l]; Dpc += sMI[base + nR + l]; }        // rpf.cpp:425, 436
            for (int cc = 0; cc < 3; ++cc) Dcf += sMI[D.npairF + cc * D.npairC + nAnc + k];
            for (int j = 0; j < nF; ++j) Dfc += sMI[base + nAnc + j];                                        // rpf.cpp:440
            if (lane < nF) sDrf[lane] = Drf;
            if (lane < 3) { sD9[lane] = Drc; sD9[3 + lane] = Dpc; sD9[6 + lane] = Dfc; }
            wsync();
            double D_f_c = 0.0, D_r_c = 0.0, D_p_c = 0.0;                                                    // rpf.cpp:449-456
            for (int i = 0; i < 3; ++i) { D_f_c += sD9[6 + i]; D_r_c += sD9[i]; D_p_c += sD9[3 + i]; }
            const double den = D_f_c + D_r_c + D_p_c + e_eps;
            double wsum = 0.0;
            for (int i = 0; i < 3; ++i) wsum += sD9[i] / (sD9[i] + sD9[3 + i] + e_eps);                      // rpf.cpp:470, 485
            const double wrc = wsum / 3;                                                                     // rpf.cpp:487
            const bool sched = (p.generic & kGenericSchedule) != 0; // RPF_FLAG_SCHEDULE with a gain other than 1: wave-uniform
            double alpha_c;
            if (sched) alpha_c = schedule_factor(p.gain_c, Drc / (Drc + Dpc + e_eps));                       // clamp0(1 - g_c W_r^{c,k})
            else alpha_c = 1 - Drc / (Drc + Dpc + e_eps);                                                    // rpf.cpp:470, 475
            // the beta presets keep the reference's stack rule for any nF: k < 3 reads D_f_ck, a gap of zeros, then D_r_fk
            double num;
            if (p.beta_map == RPF_BETA_PAPER) num = Dcf;
            else if (p.beta_map == RPF_BETA_REF_GCC11_O2) num = k < 3 ? sD9[6 + c] : (k < 8 ? 0.0 : sDrf[max(k - 8, 0)]);
            else num = k < 3 ? sD9[6 + c] : (k < 4 ? 0.0 : sDrf[max(k - 4, 0)]);
            double beta_k;
            if (sched) beta_k = schedule_factor(p.gain_f, Drf / (Drf + Dpf + e_eps)) * (num / den);          // clamp0(1 - g_f W_r^{f,k}) W_c^{f,k}
            else beta_k = (1 - Drf / (Drf + Dpf + e_eps)) * (num / den);                                     // rpf.cpp:464-465, 479
            if (lane < nF) { sBeta[lane] = beta_k; if (p.dbg.beta) p.dbg.beta[pix * nF + lane] = beta_k; }
            if (lane < 3) { sAlpha[lane] = alpha_c; if (p.dbg.alpha) p.dbg.alpha[pix * 3 + lane] = alpha_c; }
            if (lane == 0) { sWrc[0] = wrc; if (p.dbg.wrc) p.dbg.wrc[pix] = wrc; }
            wsync();
        }

        // ---- stage 4: weights and blend, term by term as rpf.cpp:646-717; lane = member lane + 64 kk, kOwn own samples per
        // sweep.  The column loop is outermost: a member's value of column k is loaded and normalised once per sweep, then the
        // kOwn own samples' sp / sc / sf take its term -- each accumulator still receives its terms in ascending k (the
        // reference's order).  A pixel on the redo list is filtered whole by generic::filter_pixel_kernel: nothing to do here.
        bool bad = false;
        if constexpr (FAST) {
            if (!redo_pixel) {
                // per column: M and 1 / SD once per pixel (fp64; the slots of the column minima and maxima are dead), which
                // columns have SD == 0 (z = 0 there) as one wave-uniform mask, and the coefficients of the summed exponent with
                // log2 e folded in, formed in fp64 and rounded once (the sums of stage 3c they overwrite are dead)
                double *sInv = sStat + 2 * ndim;
                float *sCoef = reinterpret_cast<float *>(sDrf);
                const double wrc = sWrc[0];
                const double sigma_c2 = p.seed * p.seed / (1 - wrc) / (1 - wrc);                              // rpf.cpp:662
                const double sigma_p2 = p.sigma_p * p.sigma_p;
                const double kLog2e = 1.4426950408889634;
                const double sdl = sStat[ndim + min(lane, ndim - 1)];
                const unsigned long long sd0mask = __ballot(lane < ndim && sdl == 0.0);
                if (lane < ndim) sInv[lane] = 1.0 / sdl;
                if (lane < nwt)
                    sCoef[lane] = (float)((lane < 2 ? 1.0 / (2 * sigma_p2) : (lane < 5 ? sAlpha[lane - 2] : sBeta[lane - 5]) / (2 * sigma_c2)) * kLog2e);
                auto zfast = [&](int c, double xv) { return ((sd0mask >> c) & 1ull) ? 0.f : (float)((xv - sStat[c]) * sInv[c]); };
                float *sOwnZ = reinterpret_cast<float *>(sChunk); // [nwt][kOwn] normalised own samples of the sweep (the staging chunk is dead)
                for (int i0 = 0; i0 < S; i0 += kOwn) {
                    wsync();
                    for (int t = lane; t < kOwn * nwt; t += 64) {
                        const int k = t / kOwn, ii = t % kOwn, i = min(i0 + ii, S - 1);
                        const int col = k < 5 ? k : k + nR;
                        sOwnZ[t] = zfast(col, load_col<T>(p, col, (uint32_t)(pix * S + i)));
                    }
                    wsync();
                    double sw[kOwn], s0[kOwn], s1[kOwn], s2[kOwn];
#pragma unroll
                    for (int ii = 0; ii < kOwn; ++ii) { sw[ii] = 0.0; s0[ii] = 0.0; s1[ii] = 0.0; s2[ii] = 0.0; }
                    for (int kk = 0; kk < nk; ++kk) {
                        const int j = lane + 64 * kk;
                        const bool live = j < n;
                        const uint32_t off = list[live ? j : 0];
                        f32x2 E[kOwn / 2];
#pragma unroll
                        for (int q = 0; q < kOwn / 2; ++q) E[q] = f32x2{0.f, 0.f};
                        double cj[3];
                        // one accumulator per own sample takes the column's term: d = z_i - z_j, E += (d * d) * coef, two own
                        // samples to a packed instruction
                        auto term = [&](int k, float zj) {
                            const float ck = sCoef[k];
                            const f32x2 zj2 = f32x2{zj, zj}, ck2 = f32x2{ck, ck};
#pragma unroll
                            for (int q4 = 0; q4 < kOwn / 4; ++q4) {
                                const f32x4a zo = *reinterpret_cast<const f32x4a *>(sOwnZ + k * kOwn + 4 * q4);
                                const f32x2 da = f32x2{zo[0], zo[1]} - zj2, db = f32x2{zo[2], zo[3]} - zj2;
                                E[2 * q4] = __builtin_elementwise_fma(da * da, ck2, E[2 * q4]);
                                E[2 * q4 + 1] = __builtin_elementwise_fma(db * db, ck2, E[2 * q4 + 1]);
                            }
                        };
                        const float pf0 = ldp<T>(p, 0, off), pf1 = ldp<T>(p, 1, off);
#pragma unroll
                        for (int k = 0; k < 3; ++k) cj[k] = p.col_in[(uint64_t)k * p.plane_stride + off];
                        float fv[kWvGather];
#pragma unroll
                        for (int u = 0; u < kWvGather; ++u) fv[u] = ldp<T>(p, colF + min(u, nF - 1), off);
                        term(0, zfast(0, (double)pf0));
                        term(1, zfast(1, (double)pf1));
#pragma unroll
                        for (int k = 0; k < 3; ++k) term(2 + k, zfast(2 + k, cj[k]));
                        for (int k0 = 0; k0 < nF; k0 += kWvGather) {
                            float cur[kWvGather];
#pragma unroll
                            for (int u = 0; u < kWvGather; ++u) cur[u] = fv[u];
                            if (k0 + kWvGather < nF) {
#pragma unroll
                                for (int u = 0; u < kWvGather; ++u) fv[u] = ldp<T>(p, colF + min(k0 + kWvGather + u, nF - 1), off);
                            }
#pragma unroll
                            for (int u = 0; u < kWvGather; ++u) {
                                const int k = k0 + u;
                                if (k >= nF) break;
                                term(5 + k, zfast(colF + k, (double)cur[u]));
                            }
                        }
                        if (!live) { cj[0] = 0.0; cj[1] = 0.0; cj[2] = 0.0; } // (a padding lane adds exact zeros whatever slot 0 holds)
#pragma unroll
                        for (int ii = 0; ii < kOwn; ++ii) {
                            double w = (double)__builtin_amdgcn_exp2f(-E[ii >> 1][ii & 1]);
                            w = (live && i0 + ii < S) ? w : 0.0;
                            sw[ii] += w; s0[ii] += w * cj[0]; s1[ii] += w * cj[1]; s2[ii] += w * cj[2];   // rpf.cpp:691-692
                        }
                    }
#pragma unroll
                    for (int ii = 0; ii < kOwn; ++ii) {
                        const double vw = xl::allreduce<xl::OpSum>(sw[ii]);
                        const double v0 = xl::allreduce<xl::OpSum>(s0[ii]), v1 = xl::allreduce<xl::OpSum>(s1[ii]), v2 = xl::allreduce<xl::OpSum>(s2[ii]);
                        const int i = i0 + ii;
                        if (lane < 3 && i < S) {
                            double prime = (lane == 0 ? v0 : (lane == 1 ? v1 : v2)) / vw;                             // rpf.cpp:700
                            if (isnan(prime)) {                                                                    // rpf.cpp:702
                                bad = true;
                                if (p.policy == RPF_DEGEN_EPS) prime = p.col_in[(uint64_t)lane * p.plane_stride + pix * S + i];
                            }
                            p.col_out[(uint64_t)lane * p.plane_stride + pix * S + i] = prime;
                        }
                    }
                }
            }
        } else {
            if (!redo_pixel) {
                const double wrc = sWrc[0];
                const double sigma_c2 = p.seed * p.seed / (1 - wrc) / (1 - wrc);                                  // rpf.cpp:662
                const double sigma_p2 = p.sigma_p * p.sigma_p;
                auto znorm = [&](int c, double xv) { const double sd = sStat[ndim + c]; return sd == 0.0 ? 0.0 : (xv - sStat[c]) / sd; };
                double *sOwnZ = sChunk; // [nwt][kOwn] normalised own samples of the sweep (the staging chunk is dead)
                for (int i0 = 0; i0 < S; i0 += kOwn) {
                    wsync();
                    for (int t = lane; t < kOwn * nwt; t += 64) {
                        const int k = t / kOwn, ii = t % kOwn, i = min(i0 + ii, S - 1);
                        const int col = k < 5 ? k : k + nR;
                        sOwnZ[t] = znorm(col, load_col<T>(p, col, (uint32_t)(pix * S + i)));
                    }
                    wsync();
                    double sw[kOwn], s0[kOwn], s1[kOwn], s2[kOwn];
#pragma unroll
                    for (int ii = 0; ii < kOwn; ++ii) { sw[ii] = 0.0; s0[ii] = 0.0; s1[ii] = 0.0; s2[ii] = 0.0; }
                    for (int kk = 0; kk < nk; ++kk) {
                        const int j = lane + 64 * kk;
                        const bool live = j < n;
                        const uint32_t off = list[live ? j : 0];
                        double sp[kOwn], sc[kOwn], sf[kOwn], cj[3];
#pragma unroll
                        for (int ii = 0; ii < kOwn; ++ii) { sp[ii] = 0.0; sc[ii] = 0.0; sf[ii] = 0.0; }
                        // every gather of the member that needs no loop is issued here, the features kWvGather at a time with the
                        // next group in flight while this one is weighed
                        const float pf0 = ldp<T>(p, 0, off), pf1 = ldp<T>(p, 1, off);
#pragma unroll
                        for (int k = 0; k < 3; ++k) cj[k] = p.col_in[(uint64_t)k * p.plane_stride + off];
                        float fv[kWvGather];
#pragma unroll
                        for (int u = 0; u < kWvGather; ++u) fv[u] = ldp<T>(p, colF + min(u, nF - 1), off);
#pragma unroll
                        for (int k = 0; k < 2; ++k) {
                            const double zj = znorm(k, (double)(k == 0 ? pf0 : pf1));
#pragma unroll
                            for (int ii = 0; ii < kOwn; ++ii) { const double t = sOwnZ[k * kOwn + ii] - zj; sp[ii] += t * t; }
                        }
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const double zj = znorm(2 + k, cj[k]), ak = sAlpha[k];
#pragma unroll
                            for (int ii = 0; ii < kOwn; ++ii) { const double t = sOwnZ[(2 + k) * kOwn + ii] - zj; sc[ii] += (t * t) * ak; }
                        }
                        for (int k0 = 0; k0 < nF; k0 += kWvGather) {
                            float cur[kWvGather];
#pragma unroll
                            for (int u = 0; u < kWvGather; ++u) cur[u] = fv[u];
                            if (k0 + kWvGather < nF) {
#pragma unroll
                                for (int u = 0; u < kWvGather; ++u) fv[u] = ldp<T>(p, colF + min(k0 + kWvGather + u, nF - 1), off);
                            }
#pragma unroll
                            for (int u = 0; u < kWvGather; ++u) {
                                const int k = k0 + u;
                                if (k >= nF) break;
                                const double zj = znorm(colF + k, (double)cur[u]), bk = sBeta[k];
#pragma unroll
                                for (int ii = 0; ii < kOwn; ++ii) { const double t = sOwnZ[(5 + k) * kOwn + ii] - zj; sf[ii] += (t * t) * bk; }
                            }
                        }
                        if (!live) { cj[0] = 0.0; cj[1] = 0.0; cj[2] = 0.0; } // (a padding lane adds exact zeros whatever slot 0 holds)
#pragma unroll
                        for (int ii = 0; ii < kOwn; ++ii) {
                            double w = exp(-sp[ii] / (2 * sigma_p2)) * exp(-sc[ii] / (2 * sigma_c2)) * exp(-sf[ii] / (2 * sigma_c2)); // rpf.cpp:667-670
                            w = (live && i0 + ii < S) ? w : 0.0;
                            sw[ii] += w; s0[ii] += w * cj[0]; s1[ii] += w * cj[1]; s2[ii] += w * cj[2];   // rpf.cpp:691-692
                        }
                    }
                    // the four sums of an own sample, totalled over the 64 lanes (every lane receives the totals)
#pragma unroll
                    for (int ii = 0; ii < kOwn; ++ii) {
                        const double vw = xl::allreduce<xl::OpSum>(sw[ii]);
                        const double v0 = xl::allreduce<xl::OpSum>(s0[ii]), v1 = xl::allreduce<xl::OpSum>(s1[ii]), v2 = xl::allreduce<xl::OpSum>(s2[ii]);
                        const int i = i0 + ii;
                        if (lane < 3 && i < S) {
                            double prime = (lane == 0 ? v0 : (lane == 1 ? v1 : v2)) / vw;                             // rpf.cpp:700
                            if (isnan(prime)) {                                                                    // rpf.cpp:702
                                bad = true;
                                if (p.policy == RPF_DEGEN_EPS) prime = p.col_in[(uint64_t)lane * p.plane_stride + pix * S + i];
                            }
                            p.col_out[(uint64_t)lane * p.plane_stride + pix * S + i] = prime;
                        }
                    }
                }
            }
        }
        // status: one report per pixel; a pixel on the redo list reports nothing (generic::filter_pixel_kernel owns it)
        const unsigned long long badm = __ballot(bad);
        if (lane == 0) {
            if (redo_pixel) {
                p.redo_list[atomicAdd(p.redo_count, 1u)] = pixu;
            } else if (badm != 0ull) {
                atomicAdd(&p.status[0], 1);
                atomicMin(&p.status[1], (int)pixu);
            }
        }
    }
}

template <class T, bool FAST>
hipError_t launch_wave_t(const PassParams &p, const GenericWaveCarve &cv, hipStream_t s) {
    hipError_t e = hipFuncSetAttribute((const void *)filter_wave_kernel<T, FAST>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cv.total);
    if (e != hipSuccess) return e;
    // grid-stride walk: 2048 workgroups keep 256 CUs busy whatever the carve-up lets a CU hold
    const unsigned grid = (unsigned)std::min<uint32_t>((p.list_count + cv.waves - 1u) / cv.waves, 2048u);
    hipLaunchKernelGGL((filter_wave_kernel<T, FAST>), dim3(grid), dim3(64u * cv.waves), cv.total, s, p, cv);
    return hipGetLastError();
}

} // namespace

hipError_t launch_filter_wave(const PassParams &p, int capacity, hipStream_t s, bool fast) {
    if ((p.masks == nullptr && p.members == nullptr) || (p.members != nullptr && p.member_base == nullptr)) return hipErrorInvalidValue;
    if (p.pix_list == nullptr || p.S > capacity || capacity > 832 || (capacity & 63) != 0 || !p.lay.generic_ok())
        return hipErrorInvalidValue;
    if (p.policy == RPF_DEGEN_REF_ABORT && p.redo_list != nullptr && p.redo_count == nullptr) return hipErrorInvalidValue;
    if (p.list_count == 0) return hipSuccess;
    const GenericWaveCarve cv = generic_wave_carve(p.lay, capacity);
    if (cv.waves == 0 || (int)cv.total > max_lds_per_block()) return hipErrorInvalidValue;
    if (fast) return p.lay.f16 ? launch_wave_t<__half, true>(p, cv, s) : launch_wave_t<float, true>(p, cv, s);
    return p.lay.f16 ? launch_wave_t<__half, false>(p, cv, s) : launch_wave_t<float, false>(p, cv, s);
}

} // namespace generic
} // namespace rpf
