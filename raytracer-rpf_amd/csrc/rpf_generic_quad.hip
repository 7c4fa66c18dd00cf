// rpf_generic_quad.hip -- the layout-generic four-wave kernels of large resident neighbourhoods (RPF_FLAG_GENERIC |
// RPF_FLAG_GENERIC_PACKED | RPF_FLAG_GENERIC_WAVE | RPF_FLAG_GENERIC_QUAD, rpf_query_route 13): n_random and n_feat are run-time
// values (PassParams::lay), the class capacity (1600 or 3136 samples) is a kernel argument, the template parameters are the
// storage type of the feature planes and the own samples per sweep of stage 4.  Compiled with -ffp-contract=off like every kernel TU.  DESIGN.md section 11g.
//
// filter_quad_kernel<T, OWN>: a 256-thread workgroup (four wave64) filters one pixel of the class list (N <= capacity) at a time, with a
// grid stride over the list.  It is filter_wave_kernel with four waves on one pixel, not generic::filter_pixel_kernel with a list:
// the member list comes from the count pass's acceptance masks with no second 3-sigma test, member list, bin ids and
// T[0 .. capacity] are resident in LDS, a member's columns are gathered once for both chains and the column minima / maxima, once
// for the bin ids and once per sweep of stage 4.  What four waves change against one:
//   1b  the mask words are dealt to the waves behind an exclusive prefix sum of their popcounts (LDS): word w appends at
//       S + prefix[w] + popcount(lower bits), the reference's visiting order
//   2   all 256 threads gather chunks of 128 members into the staging block (a member's columns split between two threads); a
//       column's sums of x and x * x stay ONE lane's serial chain over the members, front to back -- the columns are dealt to
//       the waves (column c: wave c & 3, lane c >> 2), so the bits of mean / stddev do not depend on which waves gather
//   3a  thread = member t + 256 kk
//   3b  the ndim marginal and npair joint tables are dealt to the waves in groups of `hists` (GenericQuadCarve), each wave on
//       its own histograms with no barrier; the sums are integers, so any dealing gives the same f
//   3c  wave 0 alone, the shared statements
//   4   thread = member t + 256 kk, column loop outermost, four (class 1600) or eight (class 3136) own samples per sweep; a
//       wave totals its four sums per own sample with the all-reduce of rpf_xlane.h, the four waves' totals meet in LDS and are
//       added in wave order
// Every __syncthreads() is reached by all four waves: the list loop runs on blockIdx / gridDim / p.list_count, N and S are the
// same value in every thread, and the redo skip reads its flag from LDS behind a barrier.
//
// The arithmetic is generic::filter_pixel_kernel's, statement by statement, as in rpf_generic_wave.hip: every stage output up to
// alpha / beta / W_r_c is the same bits as route 3's; the colours agree to rounding (the weight sums of stage 4 associate
// differently).  Under REF_ABORT a pixel with a table inside the zero band at a non-power-of-two N and non-degenerate marginals
// joins the redo list (the rule of rpf_generic_packed.hip) and generic::filter_pixel_kernel filters it again, whole.
#include "rpf_generic_common.h"

#include <algorithm>
#include <cmath>

namespace rpf {

namespace generic {
namespace {
constexpr int kQdChunk = 128;      // members staged per step of the in-order sums (two threads gather one member)
constexpr int kQdTables = 4;       // histograms a wave can fill together (xl::reduce4 totals their sums); the carve-up says how many it has
constexpr int kQdGather = 4;       // columns of a member gathered together (their latencies overlap; a register each, no run-time index)
constexpr int kQdMaxWords = 1024;  // acceptance words of a window of at most 65535 candidates (the word prefix of stage 1b)
// own samples per sweep of stage 4 (their accumulators are registers; same bits at any value), per class.  Four need 240
// registers: two waves per SIMD, the two workgroups per CU that the LDS of the class N <= 1600 leaves room for.  Eight need 384
// (320 VGPRs + 64 AGPRs): one workgroup per CU -- all that the LDS of the class N <= 3136 allows anyway, so that class takes the
// wider sweep (a member's columns gathered and normalised half as often).  Measured both ways on both classes: DESIGN.md 11g
#ifndef RPF_QUAD_OWN
#define RPF_QUAD_OWN 4
#endif
#ifndef RPF_QUAD_OWN_BIG
#define RPF_QUAD_OWN_BIG 8
#endif
constexpr int kQdOwn = RPF_QUAD_OWN, kQdOwnBig = RPF_QUAD_OWN_BIG;
static_assert(3 * kQdOwn <= 64 && 3 * kQdOwnBig <= 64, "the threads that total a sweep's sums are lanes of wave 0");
constexpr int kQdSmallCap = 1600;  // the class of kQdOwn; above it kQdOwnBig
inline int quad_own(int capacity) { return capacity > kQdSmallCap ? kQdOwnBig : kQdOwn; }
// workgroups of a CU by registers: two waves per SIMD up to 256 registers (four own samples), one above
inline uint32_t quad_reg_workgroups(int own) { return own <= 4 ? 2u : 1u; }
} // namespace
} // namespace generic

GenericQuadCarve generic_quad_carve(const SampleLayout &lay, int capacity) {
    const GenericDims D = generic_dims(lay);
    const uint32_t ndim = (uint32_t)D.ndim, npair = (uint32_t)D.npair, cap = (uint32_t)capacity;
    const uint32_t own = (uint32_t)generic::quad_own(capacity);
    GenericQuadCarve c{};
    c.capacity = cap;
    uint32_t o = up16((cap + 1u) * 8u);              // T[0 .. capacity]
    c.off_pairtab = o; o = up16(o + 2u * npair);
    c.off_list = o; o += up16(cap * 4u);
    // one block for the word prefix (stage 1b), the staging chunk (stage 2), the bin ids (stages 3a, 3b) and the own rows of a
    // sweep (stage 4): never live together
    c.off_shared = o;
    uint32_t shared = (uint32_t)generic::kQdMaxWords * 4u;
    shared = std::max(shared, ndim * (uint32_t)(generic::kQdChunk + 1) * 8u);
    shared = std::max(shared, ndim * cap);
    shared = std::max(shared, own * (uint32_t)D.nwt * 8u);
    o += up16(shared);
    c.off_hist = o;
    const uint32_t bmax = (uint32_t)std::sqrt((double)cap);
    c.hist_words = (bmax * bmax + 1u) / 2u;
    const uint32_t stat = generic_f64_doubles(D) * 8u; // M | SD | min | max, lo | range | flags, sum T[hx], pair sums / MI, weights
    const uint32_t red = 4u * own * 4u * 8u;
    const uint32_t lds = (uint32_t)max_lds_per_block();
    // histograms per wave: of 1, 2 and 4 the count that lets a CU hold the most workgroups, the larger count on a tie (fewer
    // passes over the bin ids); 0: not even one fits, and the layout is not offered this capacity
    c.hists = 0u;
    uint32_t best = 0u;
    for (uint32_t h = 1u; h <= (uint32_t)generic::kQdTables; h *= 2u) {
        const uint32_t total = up16(o + up16(4u * h * c.hist_words * 4u) + stat + red + 16u);
        if (total > lds) continue;
        const uint32_t per_cu = std::min(generic::quad_reg_workgroups((int)own), lds / total);
        if (per_cu >= best) { best = per_cu; c.hists = h; }
    }
    const uint32_t h = std::max(c.hists, 1u);
    o += up16(4u * h * c.hist_words * 4u);
    c.off_stat = o; o += stat;
    c.off_red = o; o += red;
    c.off_flag = o; o += 16u;
    c.total = up16(o);
    c.workgroups_per_cu = c.hists ? best : 0u;
    return c;
}

namespace generic {
namespace {

// One workgroup = one pixel of the class list at a time, the entries dealt to the workgroups of the grid with a grid stride.
// OWN: own samples per sweep of stage 4 (quad_own of the class)
template <class T, int OWN>
__global__ __launch_bounds__(256) void filter_quad_kernel(PassParams p, GenericQuadCarve cv) {
    constexpr int kQdOwn = OWN; // (shadows the class-1600 constant: every use below is this instantiation's)
    extern __shared__ __align__(16) unsigned char smem[];
    const GenericDims D = generic_dims(p.lay);
    const int ndim = D.ndim, nF = D.nF, nR = D.nR, nAnc = D.nAnc, npair = D.npair, nwt = D.nwt, colF = D.colF;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cap = (int)cv.capacity;
    const int nhist = (int)cv.hists;
    uint64_t *sT = reinterpret_cast<uint64_t *>(smem);
    for (int k = tid; k <= cap; k += kThreads) sT[k] = p.tfix[min(k, p.nmax)];
    uint16_t *sPairTab = reinterpret_cast<uint16_t *>(smem + cv.off_pairtab);
    for (int pr = tid; pr < npair; pr += kThreads) {
        int ca, cb;
        pair_cols(D, pr, ca, cb);
        sPairTab[pr] = (uint16_t)(ca | (cb << 8));
    }
    uint32_t *list = reinterpret_cast<uint32_t *>(smem + cv.off_list);                   // [cap] plane offsets, reference order
    uint32_t *sPre = reinterpret_cast<uint32_t *>(smem + cv.off_shared);                 // [nwords] members ahead of a mask word
    double *sChunk = reinterpret_cast<double *>(smem + cv.off_shared);                   // [ndim][kQdChunk + 1]
    uint8_t *bins = smem + cv.off_shared;                                                // [ndim][cap]
    double *sOwnZ = reinterpret_cast<double *>(smem + cv.off_shared);                    // [nwt][kQdOwn]
    uint32_t *sHist = reinterpret_cast<uint32_t *>(smem + cv.off_hist) + (uint32_t)wv * cv.hists * cv.hist_words; // this wave's, 16-bit cells
    double *sStat = reinterpret_cast<double *>(smem + cv.off_stat);                      // M | SD | xmin | xmax
    double *sZ = sStat + 4 * ndim;                                                       // lo | range | flags(sd0 | flat << 1)
    uint64_t *sHX = reinterpret_cast<uint64_t *>(sZ + 3 * ndim);                         // sum_i T[hx_i] per column
    uint64_t *sPair = sHX + ndim;                                                        // sum_ij T[J_ij] per pair, then the MI values
    double *sMI = reinterpret_cast<double *>(sPair);
    double *sW = sMI + npair;                                                            // Drf[nF] | D9[12] | alpha[4] | beta[nF] | wrc[4]
    double *sRed = reinterpret_cast<double *>(smem + cv.off_red);                        // [4 waves][kQdOwn][4] partial sums of a sweep
    int *sFlag = reinterpret_cast<int *>(smem + cv.off_flag);                            // redo

    const int W = p.W, H = p.H, S = p.S, b = p.b;
    const double e_eps = (p.policy == RPF_DEGEN_EPS) ? p.eps : 0.0;
    const int mycol = lane * 4 + wv; // the column whose chains this thread adds (stage 2): dealt to the waves, four to a lane index
    for (uint32_t e = blockIdx.x; e < p.list_count; e += gridDim.x) {
        __syncthreads(); // the tables are written; the previous pixel's LDS is dead
        const uint32_t pixu = p.pix_list[e];
        const uint64_t pix = pixu;
        const int y = (int)(pixu / (uint32_t)W), x = (int)(pixu - (uint32_t)y * (uint32_t)W);
        const int n = min(p.nbhd[pixu], cap); // <= cap by construction of the list; the same value in every thread

        // ---- stage 1b: the member list from the acceptance masks of the count pass, reference order (rpf.cpp:556-586) ----
        const Window win = make_window(x, y, b, W, H, S);
        const int nwords = min(min((win.ncand + 63) >> 6, (int)p.mask_stride), kQdMaxWords);
        const uint64_t *pm = p.masks + pix * p.mask_stride;
        for (int s = tid; s < min(S, cap); s += kThreads) list[s] = (uint32_t)(pix * S + s); // own samples first
        if (tid == 0) sFlag[0] = 0;
        for (int w = tid; w < nwords; w += kThreads) sPre[w] = (uint32_t)__popcll(pm[w]);
        __syncthreads();
        if (wv == 0) { // exclusive prefix sum of the word popcounts, 64 words a step (wave-uniform branch: every lane shuffles)
            int carry = 0;
            for (int w0 = 0; w0 < nwords; w0 += 64) {
                const int w = w0 + lane;
                const int c = w < nwords ? (int)sPre[w] : 0;
                int incl = c;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int up = __shfl_up(incl, d, 64);
                    if (lane >= d) incl += up;
                }
                if (w < nwords) sPre[w] = (uint32_t)(carry + incl - c);
                carry += __shfl(incl, 63, 64);
            }
        }
        __syncthreads();
        for (int w = wv; w < nwords; w += 4) { // a word to a wave, a candidate to a lane
            const unsigned long long mask = pm[w]; // wave-uniform
            if (mask == 0ull) continue;
            if ((mask >> lane) & 1ull) {
                const int at = S + (int)sPre[w] + __popcll(mask & ((1ull << lane) - 1ull));
                if (at < cap) list[at] = candidate_offset(win, W, S, w * 64 + lane);
            }
        }
        __syncthreads();
        const int B = max(1, (int)sqrt((double)n));                // mi.cpp:54
        const double dn = (double)n;
        const int nk = (n + 63) >> 6;                              // members per lane of a wave that walks the whole list
        const int nk4 = (n + kThreads - 1) / kThreads;             // members per thread: j = tid + 256 kk

        // ---- stage 2: in-order sums over the neighbourhood (rpf.cpp:596-601), chunks of 128 staged through LDS: threads q and
        // q + 128 gather the columns of member j0 + q (alternate groups of kQdGather), then the thread of column c adds both
        // chains of column c front to back; the column's minimum and maximum ride along
        {
            double acc = 0.0, acc2 = 0.0, mn = INFINITY, mx = -INFINITY;
            const int q = tid & (kQdChunk - 1), half = tid >> 7;
            for (int j0 = 0; j0 < n; j0 += kQdChunk) {
                const int cnt = min(kQdChunk, n - j0);
                if (q < cnt) {
                    const uint32_t off = list[j0 + q];
                    for (int c0 = half * kQdGather; c0 < ndim; c0 += 2 * kQdGather) { // kQdGather gathers in flight, then their stores
                        double v[kQdGather];
#pragma unroll
                        for (int u = 0; u < kQdGather; ++u) v[u] = load_col<T>(p, min(c0 + u, ndim - 1), off);
#pragma unroll
                        for (int u = 0; u < kQdGather; ++u)
                            if (c0 + u < ndim) sChunk[(c0 + u) * (kQdChunk + 1) + q] = v[u];
                    }
                }
                __syncthreads();
                if (mycol < ndim) {
                    const double *src = sChunk + mycol * (kQdChunk + 1);
                    for (int k = 0; k < cnt; ++k) {
                        const double v = src[k];
                        acc = acc + v;                               // ops.h:121
                        acc2 = acc2 + v * v;                         // ops.h:138
                        mn = fmin(mn, v); mx = fmax(mx, v);
                    }
                }
                __syncthreads();
            }
            // the per-column constants of the binning (sd.h:229-232, mi.cpp:47-50)
            if (mycol < ndim) {
                const double mean = acc / dn;                        // ops.h:123
                double sd = sqrt(acc2 / dn - mean * mean);           // ops.h:141
                if (p.policy == RPF_DEGEN_EPS && isnan(sd)) sd = 0.0;
                sStat[mycol] = mean; sStat[ndim + mycol] = sd;
                sStat[2 * ndim + mycol] = mn; sStat[3 * ndim + mycol] = mx;
                if (p.dbg.mean) p.dbg.mean[pix * ndim + mycol] = mean;
                if (p.dbg.stddev) p.dbg.stddev[pix * ndim + mycol] = sd;
                const bool sd0 = (sd == 0.0);
                const double lo = sd0 ? 0.0 : (mn - mean) / sd, hi = sd0 ? 0.0 : (mx - mean) / sd;
                sZ[mycol] = lo; sZ[ndim + mycol] = hi - lo;
                sZ[2 * ndim + mycol] = (double)((sd0 ? 1 : 0) | (!(hi != lo) ? 2 : 0)); // mi.cpp:7 / 28 / 34
            }
        }
        __syncthreads(); // (the staging chunk is dead: the bin ids take its block)

        // ---- stage 3a: normalise, bin ids (one byte per sample and column); thread = member tid + 256 kk ------------------
        for (int kk = 0; kk < nk4; ++kk) {
            const int j = tid + kThreads * kk;
            if (j < n) {
                const uint32_t off = list[j];
                for (int c0 = 0; c0 < ndim; c0 += kQdGather) {
                    double v[kQdGather];
#pragma unroll
                    for (int u = 0; u < kQdGather; ++u) v[u] = load_col<T>(p, min(c0 + u, ndim - 1), off);
#pragma unroll
                    for (int u = 0; u < kQdGather; ++u) {
                        const int c = c0 + u;
                        if (c >= ndim) break;
                        bins[c * cap + j] = (uint8_t)bin_id(v[u], sStat[c], sStat[ndim + c], sZ[c], sZ[ndim + c], (int)sZ[2 * ndim + c], B);
                    }
                }
            }
        }
        __syncthreads();
        if (p.dbg.member_hash != nullptr && tid == kThreads - 1) p.dbg.member_hash[pix] = member_hash(list, n, x, y, b, p.box, S, W);
        if (p.dbg.bin_hash != nullptr && mycol < ndim) p.dbg.bin_hash[pix * ndim + mycol] = bin_hash(bins + mycol * cap, n);

        // ---- stage 3b: histograms, 16-bit cells packed two per word (counts <= N <= 3136): the ndim marginal tables, then the
        // pairs, dealt to the waves in groups of nhist tables; a wave fills its group on its own histograms (their LDS round
        // trips overlap; one transposed butterfly totals the sums) and needs no barrier until every table is done
        {
            const int ntab = ndim + npair;
            const int hs = (B * B + 1) / 2;                       // words of one histogram of this pixel (<= cv.hist_words)
            for (int tb0 = wv * nhist; tb0 < ntab; tb0 += 4 * nhist) {
                int oa[kQdTables], ob[kQdTables], cells[kQdTables]; // (wave-uniform; indexed by unrolled loops only)
#pragma unroll
                for (int u = 0; u < kQdTables; ++u) {
                    const int tb = tb0 + u;
                    oa[u] = -1; ob[u] = 0; cells[u] = 0;          // a table past the group or the last: no cell, nothing added
                    if (u < nhist && tb < ndim) {
                        ob[u] = tb * cap; cells[u] = B;
                    } else if (u < nhist && tb < ntab) {
                        const uint32_t cc = sPairTab[tb - ndim];
                        oa[u] = (int)(cc & 255u) * cap; ob[u] = (int)(cc >> 8) * cap; cells[u] = B * B;
                    }
                }
                for (int t = lane; t < nhist * hs; t += 64) sHist[t] = 0u;
                wsync();
                for (int kk = 0; kk < nk; ++kk) {
                    const int j = lane + 64 * kk;
                    if (j < n) {
#pragma unroll
                        for (int u = 0; u < kQdTables; ++u) {
                            if (cells[u] == 0) continue;
                            const uint32_t cell = oa[u] >= 0 ? (uint32_t)bins[oa[u] + j] * (uint32_t)B + bins[ob[u] + j] : bins[ob[u] + j]; // mi.cpp:39
                            atomicAdd(&sHist[u * hs + (int)(cell >> 1)], 1u << (16u * (cell & 1u)));
                        }
                    }
                }
                wsync();
                uint64_t acc[kQdTables];
#pragma unroll
                for (int u = 0; u < kQdTables; ++u) acc[u] = 0ull;
                for (int t = lane; t < B * B; t += 64) {
#pragma unroll
                    for (int u = 0; u < kQdTables; ++u)
                        if (t < cells[u]) acc[u] += sT[(sHist[u * hs + (t >> 1)] >> (16u * (t & 1u))) & 0xffffu];
                }
                const uint64_t tot = xl::reduce4<xl::OpSum>(acc); // the lane holds the total of table tb0 + slot4(lane)
                const int slot = xl::slot4(lane), tb = tb0 + slot;
                if ((lane & 15) == 0 && slot < nhist && tb < ntab) { if (tb < ndim) sHX[tb] = tot; else sPair[tb - ndim] = tot; }
                wsync();
            }
        }
        __syncthreads();
        {
            bool redo = false;
            const int64_t TNf = (int64_t)sT[n];
            const int64_t zero_band = ((int64_t)B * B + 2 * B + 1) / 2 + 1;   // see filter_pixel_kernel (rpf_filter_impl.inc)
            for (int pr = tid; pr < npair; pr += kThreads) {
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
                sMI[pr] = mi; // (same slot as sPair[pr]: each thread overwrites only what it has just read)
                if (p.dbg.mi) p.dbg.mi[pix * npair + pr] = mi;
            }
            if (redo) sFlag[0] = 1;
        }
        __syncthreads();
        const bool redo_pixel = sFlag[0] != 0; // read behind the barrier: the same value in every thread

        // ---- stage 3c: alpha, beta, W_r_c (rpf.cpp:444-487), the statements of generic::filter_pixel_kernel, on wave 0 --------
        double *sDrf = sW, *sD9 = sDrf + nF, *sAlpha = sD9 + 12, *sBeta = sAlpha + 4, *sWrc = sBeta + nF;
        if (wv == 0) {
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
            const bool sched = (p.generic & kGenericSchedule) != 0; // RPF_FLAG_SCHEDULE with a gain other than 1: uniform
            double alpha_c;
            if (sched) alpha_c = schedule_factor(p.gain_c, Drc / (Drc + Dpc + e_eps));                       // clamp0(1 - g_c W_r^{c,k})
            else alpha_c = 1 - Drc / (Drc + Dpc + e_eps);                                                    // rpf.cpp:470, 475
            const double num = beta_numerator(p.beta_map, k, c, Dcf, sD9, sDrf);
            double beta_k;
            if (sched) beta_k = schedule_factor(p.gain_f, Drf / (Drf + Dpf + e_eps)) * (num / den);          // clamp0(1 - g_f W_r^{f,k}) W_c^{f,k}
            else beta_k = (1 - Drf / (Drf + Dpf + e_eps)) * (num / den);                                     // rpf.cpp:464-465, 479
            if (lane < nF) { sBeta[lane] = beta_k; if (p.dbg.beta) p.dbg.beta[pix * nF + lane] = beta_k; }
            if (lane < 3) { sAlpha[lane] = alpha_c; if (p.dbg.alpha) p.dbg.alpha[pix * 3 + lane] = alpha_c; }
            if (lane == 0) { sWrc[0] = wrc; if (p.dbg.wrc) p.dbg.wrc[pix] = wrc; }
        }
        __syncthreads(); // (the bin ids are dead: the own rows of a sweep take their block)

        // ---- stage 4: weights and blend, term by term as rpf.cpp:646-717; thread = member tid + 256 kk, kQdOwn own samples per
        // sweep.  The column loop is outermost: a member's value of column k is loaded and normalised once per sweep, then the
        // kQdOwn own samples' sp / sc / sf take its term -- each accumulator still receives its terms in ascending k (the
        // reference's order).  A pixel on the redo list is filtered whole by generic::filter_pixel_kernel: nothing to do here.
        bool bad = false;
        if (!redo_pixel) { // (uniform: every barrier below is reached by all four waves or by none)
            const double wrc = sWrc[0];
            const double sigma_c2 = p.seed * p.seed / (1 - wrc) / (1 - wrc);                                  // rpf.cpp:662
            const double sigma_p2 = p.sigma_p * p.sigma_p;
            auto znorm = [&](int c, double xv) { const double sd = sStat[ndim + c]; return sd == 0.0 ? 0.0 : (xv - sStat[c]) / sd; };
            for (int i0 = 0; i0 < S; i0 += kQdOwn) {
                __syncthreads(); // the previous sweep's own rows and partial sums are dead
                for (int t = tid; t < kQdOwn * nwt; t += kThreads) {
                    const int k = t / kQdOwn, ii = t % kQdOwn, i = min(i0 + ii, S - 1);
                    const int col = k < 5 ? k : k + nR;
                    sOwnZ[t] = znorm(col, load_col<T>(p, col, (uint32_t)(pix * S + i)));
                }
                __syncthreads();
                double sw[kQdOwn], s0[kQdOwn], s1[kQdOwn], s2[kQdOwn];
#pragma unroll
                for (int ii = 0; ii < kQdOwn; ++ii) { sw[ii] = 0.0; s0[ii] = 0.0; s1[ii] = 0.0; s2[ii] = 0.0; }
                for (int kk = 0; kk < nk4; ++kk) {
                    const int j = tid + kThreads * kk;
                    const bool live = j < n;
                    const uint32_t off = list[live ? j : 0];
                    double sp[kQdOwn], sc[kQdOwn], sf[kQdOwn], cj[3];
#pragma unroll
                    for (int ii = 0; ii < kQdOwn; ++ii) { sp[ii] = 0.0; sc[ii] = 0.0; sf[ii] = 0.0; }
                    // every gather of the member that needs no loop is issued here, the features kQdGather at a time with the
                    // next group in flight while this one is weighed
                    const float pf0 = ldp<T>(p, 0, off), pf1 = ldp<T>(p, 1, off);
#pragma unroll
                    for (int k = 0; k < 3; ++k) cj[k] = p.col_in[(uint64_t)k * p.plane_stride + off];
                    float fv[kQdGather];
#pragma unroll
                    for (int u = 0; u < kQdGather; ++u) fv[u] = ldp<T>(p, colF + min(u, nF - 1), off);
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const double zj = znorm(k, (double)(k == 0 ? pf0 : pf1));
#pragma unroll
                        for (int ii = 0; ii < kQdOwn; ++ii) { const double t = sOwnZ[k * kQdOwn + ii] - zj; sp[ii] += t * t; }
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double zj = znorm(2 + k, cj[k]), ak = sAlpha[k];
#pragma unroll
                        for (int ii = 0; ii < kQdOwn; ++ii) { const double t = sOwnZ[(2 + k) * kQdOwn + ii] - zj; sc[ii] += (t * t) * ak; }
                    }
                    for (int k0 = 0; k0 < nF; k0 += kQdGather) {
                        float cur[kQdGather];
#pragma unroll
                        for (int u = 0; u < kQdGather; ++u) cur[u] = fv[u];
                        if (k0 + kQdGather < nF) {
#pragma unroll
                            for (int u = 0; u < kQdGather; ++u) fv[u] = ldp<T>(p, colF + min(k0 + kQdGather + u, nF - 1), off);
                        }
#pragma unroll
                        for (int u = 0; u < kQdGather; ++u) {
                            const int k = k0 + u;
                            if (k >= nF) break;
                            const double zj = znorm(colF + k, (double)cur[u]), bk = sBeta[k];
#pragma unroll
                            for (int ii = 0; ii < kQdOwn; ++ii) { const double t = sOwnZ[(5 + k) * kQdOwn + ii] - zj; sf[ii] += (t * t) * bk; }
                        }
                    }
                    if (!live) { cj[0] = 0.0; cj[1] = 0.0; cj[2] = 0.0; } // (a padding thread adds exact zeros whatever slot 0 holds)
#pragma unroll
                    for (int ii = 0; ii < kQdOwn; ++ii) {
                        double w = exp(-sp[ii] / (2 * sigma_p2)) * exp(-sc[ii] / (2 * sigma_c2)) * exp(-sf[ii] / (2 * sigma_c2)); // rpf.cpp:667-670
                        w = (live && i0 + ii < S) ? w : 0.0;
                        sw[ii] += w; s0[ii] += w * cj[0]; s1[ii] += w * cj[1]; s2[ii] += w * cj[2];   // rpf.cpp:691-692
                    }
                }
                // the four sums of an own sample: totalled over the 64 lanes of each wave, then over the four waves through LDS
#pragma unroll
                for (int ii = 0; ii < kQdOwn; ++ii) {
                    const double vw = xl::allreduce<xl::OpSum>(sw[ii]);
                    const double v0 = xl::allreduce<xl::OpSum>(s0[ii]), v1 = xl::allreduce<xl::OpSum>(s1[ii]), v2 = xl::allreduce<xl::OpSum>(s2[ii]);
                    if (lane == 0) {
                        double *r = sRed + (wv * kQdOwn + ii) * 4;
                        r[0] = vw; r[1] = v0; r[2] = v1; r[3] = v2;
                    }
                }
                __syncthreads();
                if (tid < 3 * kQdOwn) {
                    const int ii = tid / 3, ch = tid - 3 * ii, i = i0 + ii;
                    if (i < S) {
                        double den = 0.0, num = 0.0;
#pragma unroll
                        for (int w4 = 0; w4 < 4; ++w4) { den += sRed[(w4 * kQdOwn + ii) * 4]; num += sRed[(w4 * kQdOwn + ii) * 4 + 1 + ch]; }
                        bad = store_filtered(p, ch, pix, S, i, num, den) || bad;                               // rpf.cpp:700, 702
                    }
                }
            }
        }
        // status: one report per pixel; a pixel on the redo list reports nothing (generic::filter_pixel_kernel owns it)
        const unsigned long long badm = __ballot(bad); // (the threads that store are lanes of wave 0)
        if (tid == 0) {
            if (redo_pixel) {
                p.redo_list[atomicAdd(p.redo_count, 1u)] = pixu;
            } else if (badm != 0ull) {
                atomicAdd(&p.status[0], 1);
                atomicMin(&p.status[1], (int)pixu);
            }
        }
    }
}

template <class T, int OWN>
hipError_t launch_quad_t(const PassParams &p, const GenericQuadCarve &cv, hipStream_t s) {
    hipError_t e = hipFuncSetAttribute((const void *)filter_quad_kernel<T, OWN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cv.total);
    if (e != hipSuccess) return e;
    // grid-stride walk: 2048 workgroups keep 256 CUs busy whatever the carve-up lets a CU hold
    const unsigned grid = (unsigned)std::min<uint32_t>(p.list_count, 2048u);
    hipLaunchKernelGGL((filter_quad_kernel<T, OWN>), dim3(grid), dim3(kThreads), cv.total, s, p, cv);
    return hipGetLastError();
}

} // namespace

hipError_t launch_filter_quad(const PassParams &p, int capacity, hipStream_t s) {
    if (p.masks == nullptr || p.nbhd == nullptr || p.pix_list == nullptr || p.mask_stride == 0 || p.mask_stride > (uint32_t)kQdMaxWords)
        return hipErrorInvalidValue;
    if ((capacity != 1600 && capacity != 3136) || p.S > capacity || !p.lay.generic_ok()) return hipErrorInvalidValue;
    if (p.policy == RPF_DEGEN_REF_ABORT && p.redo_list != nullptr && p.redo_count == nullptr) return hipErrorInvalidValue;
    if (p.list_count == 0) return hipSuccess;
    const GenericQuadCarve cv = generic_quad_carve(p.lay, capacity);
    if (cv.hists == 0 || (int)cv.total > max_lds_per_block()) return hipErrorInvalidValue;
    if (quad_own(capacity) == kQdOwnBig) return p.lay.f16 ? launch_quad_t<__half, kQdOwnBig>(p, cv, s) : launch_quad_t<float, kQdOwnBig>(p, cv, s);
    return p.lay.f16 ? launch_quad_t<__half, kQdOwn>(p, cv, s) : launch_quad_t<float, kQdOwn>(p, cv, s);
}

} // namespace generic
} // namespace rpf
