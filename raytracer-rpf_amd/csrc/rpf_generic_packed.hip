// rpf_generic_packed.hip -- the layout-generic kernels of small neighbourhoods (RPF_FLAG_GENERIC | RPF_FLAG_GENERIC_PACKED,
// rpf_query_route 4): n_random and n_feat are run-time values (PassParams::lay), the template parameters are the storage
// type of the feature planes and the lanes a pixel gets.  Compiled with -ffp-contract=off like every kernel TU.
//
// nbhd_count_kernel: one wave per pixel applies stage 1b's 3-sigma test of generic::filter_pixel_kernel to the window's
// candidates, 64 at a time, and leaves N and one acceptance mask per 64 candidates (bit q = candidate q in the reference's
// visiting order, the numbering of the compiled count pass).
//
// filter_packed_kernel<T, G>: the algorithm of rpf_packed_impl.inc with every column count a loop bound.  A pixel of the
// class list (N <= G) gets G = 8, 16, 32 or 64 lanes, a wave filters 64 / G list entries at a time, lane g * G + t owns the
// t-th sample of group g's neighbourhood in the reference's order (slot t < S: own sample t; else the (t - S)-th set bit of
// the pixel's acceptance masks, or -- a wide pass dealt by size class, p.members -- the (t - S)-th listed member).  No
// per-thread array is indexed by a run-time column: the sample
// values stay staged in LDS as [group][column][slot] doubles for the whole unit, bin ids are LDS bytes and bit masks, and
// the LDS carve-up comes from the host (generic_packed_carve).  After the table load the waves of a workgroup are
// independent: one wave's LDS operations execute in order, so wsync() is all the hand-over between its lanes needs.
//
// The arithmetic is generic::filter_pixel_kernel's, statement by statement: in-order sums of x and x * x (one lane per
// chain), sd == 0 -> z = 0, B = max(1, (int)sqrt(N)), bin ids by IEEE quotients, joint counts as popcount(mask_a[i] &
// mask_b[j]) (the same integers as its 16-bit histogram cells), MI from the 2^-44 k ln k table with the same zero band,
// the beta presets generalised by the stack rule of DESIGN.md section 11, three exps multiplied.  Every stage output up to
// alpha / beta / W_r_c is the same bits as route 3's; the colours agree to rounding (the weight sums of stage 4 associate
// differently).  Under
// REF_ABORT a pixel with a table inside the zero band at a non-power-of-two N and non-degenerate marginals joins the redo
// list (the rule of rpf_packed_impl.inc) and generic::filter_pixel_kernel filters it again, whole.
//
// filter_packed_kernel<T, G, FAST = true> (RPF_FLAG_GENERIC_FAST): the same kernel with stage 4 in fp32 --
// z and the 5 + n_feat coefficients (log2 e folded in) formed in fp64 and rounded once, one accumulator per own sample, two own
// samples per packed fp32 instruction, one hardware exponential, the sums and the quotient in fp64.  Every statement outside
// stage 4 is shared, so the stage outputs are the FAST = false kernel's bits.
#include "rpf_generic_common.h"

#include <algorithm>

namespace rpf {

GenericPackedCarve generic_packed_carve(const SampleLayout &lay) {
    const GenericDims D = generic_dims(lay);
    const uint32_t ndim = (uint32_t)D.ndim, npair = (uint32_t)D.npair, nF = (uint32_t)D.nF;
    GenericPackedCarve c{};
    c.off_pairtab = up16(65u * 8u);                  // behind T[0 .. 64]
    c.table_bytes = up16(c.off_pairtab + 2u * npair);
    uint32_t o = 64u * ndim * 8u;                    // staged samples
    c.off_stat = o; o += 8u * ndim * 5u * 8u;
    c.off_mask = o; o += ndim * 16u * 8u;
    c.off_hx = o; o += 8u * ndim * 8u;
    c.off_bins = o; o += up16(64u * ndim);
    c.off_mi = o; o += 8u * npair * 8u;
    c.off_w = o; o += 8u * (2u * nF + 16u) * 8u;
    c.off_flag = o; o += 8u * 4u;
    c.wave_bytes = up16(o);
    const uint32_t room = (uint32_t)max_lds_per_block() - c.table_bytes;
    c.waves = std::max(1u, std::min(4u, room / c.wave_bytes));
    c.total = c.table_bytes + c.waves * c.wave_bytes;
    return c;
}

namespace generic {
namespace {

// own samples per sweep of stage 4 under RPF_FLAG_GENERIC_FAST (an even number dividing 8: two own samples share a packed
// fp32 instruction; DESIGN.md section 11e has the trial of 4 against 8)
#ifndef RPF_PACKED_FAST_OWN
#define RPF_PACKED_FAST_OWN 8
#endif
typedef float __attribute__((may_alias)) zf32;                              // fp32 z values kept in rows the fp64 staging owns
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2a __attribute__((ext_vector_type(2), may_alias));

// all-reduce over the G lanes of a group (G = 8: half a DPP row, 16: a row, 32: a row pair, 64: the wave); EXEC = all lanes
template <int G>
__device__ __forceinline__ double group_sum(double v) {
    using Sum = xl::OpSum;
    if constexpr (G == 64) return xl::allreduce<Sum>(v);
    else if constexpr (G == 32) return xl::allreduce_row<Sum>(xl::exch16<Sum>(v, v));
    else if constexpr (G == 16) return xl::allreduce_row<Sum>(v);
    else {
        v = v + xl::dpp<xl::kRowHalfMirror>(v);
        return xl::allreduce_bits10<Sum>(v);
    }
}

// One wave per pixel of rows [row_begin, row_end): the test of generic::filter_pixel_kernel stage 1b on 64 candidates at a
// time (rpf.cpp:556-586); p.masks[pix][w] bit l = candidate 64 w + l passed, p.nbhd[pix] = S + the passes.
template <class T>
__global__ __launch_bounds__(256) void nbhd_count_kernel(PassParams p) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t npix = (uint32_t)(p.row_end - p.row_begin) * (uint32_t)p.W;
    const uint32_t e = blockIdx.x * 4u + (uint32_t)wv;
    if (e >= npix) return; // wave-uniform; the kernel has no barrier
    const int W = p.W, H = p.H, S = p.S, b = p.b;
    const uint64_t HW = (uint64_t)H * W;
    const uint64_t pix = (uint64_t)p.row_begin * W + e;
    const int y = (int)(pix / (uint32_t)W), x = (int)(pix - (uint64_t)y * W);
    const int nF = p.lay.nF, colF = 5 + p.lay.nR;
    const Window win = make_window(x, y, b, W, H, S);
    const int ncand = win.ncand;
    uint64_t *pm = p.masks + pix * p.mask_stride;
    int n = S;
    for (int qb = 0; qb < ncand; qb += 64) {
        const int qq = qb + lane;
        bool pass = qq < ncand;
        const uint32_t off = pass ? candidate_offset(win, W, S, qq) : 0u;
        pass = passes_3sigma_wave<T>(p, colF, nF, off, HW, pix, pass);
        const unsigned long long mask = __ballot(pass);
        if (lane == 0) pm[qb >> 6] = mask;
        n += __popcll(mask);
    }
    if (lane == 0) p.nbhd[pix] = n;
}

// One wave = one "unit" of 64 / G list entries at a time, units dealt to the waves of the grid with a grid stride.
// FAST (RPF_FLAG_GENERIC_FAST): stage 4 alone in the fp32 arithmetic of DESIGN.md section 11e; every other statement is shared.
template <class T, int G, bool FAST = false>
__global__ __launch_bounds__(256) void filter_packed_kernel(PassParams p, GenericPackedCarve cv) {
    constexpr int P = 64 / G;                                   // pixels per wave
    constexpr int BSTR = G == 8 ? 2 : (G == 16 ? 4 : 8);        // mask slots per (pixel, column): B = floor(sqrt(N)) <= 2, 4, 5, 8
    constexpr int kOwn = FAST ? RPF_PACKED_FAST_OWN : 4;        // own samples per sweep of stage 4
    static_assert(P * BSTR <= 16, "sixteen masks per column and wave");
    extern __shared__ __align__(16) unsigned char smem[];
    const GenericDims D = generic_dims(p.lay);
    const int ndim = D.ndim, nF = D.nF, nR = D.nR, nAnc = D.nAnc, npair = D.npair, nwt = D.nwt, colF = D.colF;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nthreads = (int)blockDim.x;
    uint64_t *sT = reinterpret_cast<uint64_t *>(smem);
    for (int k = tid; k <= 64; k += nthreads) sT[k] = p.tfix[min(k, p.nmax)];
    uint16_t *sPairTab = reinterpret_cast<uint16_t *>(smem + cv.off_pairtab);
    for (int pr = tid; pr < npair; pr += nthreads) {
        int ca, cb;
        pair_cols(D, pr, ca, cb);
        sPairTab[pr] = (uint16_t)(ca | (cb << 8));
    }
    __syncthreads(); // the only barrier: from here on the waves are independent
    unsigned char *wb = smem + cv.table_bytes + (uint32_t)wv * cv.wave_bytes;
    double *sU = reinterpret_cast<double *>(wb);                                        // [P][ndim][G]
    double *sStat = reinterpret_cast<double *>(wb + cv.off_stat);                       // [P][ndim][5]
    unsigned long long *sMask = reinterpret_cast<unsigned long long *>(wb + cv.off_mask); // [P][ndim][BSTR]
    uint64_t *sHX = reinterpret_cast<uint64_t *>(wb + cv.off_hx);                       // [P][ndim]
    uint8_t *sBin = wb + cv.off_bins;                                                   // [P][ndim][G]
    double *sMI = reinterpret_cast<double *>(wb + cv.off_mi);                           // [P][npair]
    double *sW = reinterpret_cast<double *>(wb + cv.off_w);                             // [P][2 nF + 16]
    int *sFlag = reinterpret_cast<int *>(wb + cv.off_flag);                             // [P]

    const int W = p.W, H = p.H, S = p.S, b = p.b;
    const int g = lane / G, t = lane % G;
    const double e_eps = (p.policy == RPF_DEGEN_EPS) ? p.eps : 0.0;
    const uint32_t units = (p.list_count + (uint32_t)P - 1u) / (uint32_t)P;
    const uint32_t nwaves = (uint32_t)nthreads >> 6;
    for (uint32_t unit = blockIdx.x * nwaves + (uint32_t)wv; unit < units; unit += gridDim.x * nwaves) {
        wsync(); // the previous unit's LDS is dead
        const uint32_t e = unit * (uint32_t)P + (uint32_t)g;
        const bool gvalid = e < p.list_count;             // (only the last unit can be short)
        const uint32_t pixu = gvalid ? p.pix_list[e] : 0u;
        const int n = gvalid ? min(p.nbhd[pixu], G) : 0;  // <= G by construction of the list
        const uint64_t pix = pixu;
        const bool live = t < n;
        const int y = (int)(pixu / (uint32_t)W), x = (int)(pixu - (uint32_t)y * (uint32_t)W);
        const int gbase = g * ndim;                       // first (pixel, column) record of the group

        // ---- stage 1b: the lane's sample (rpf.cpp:556-586), rank select in the acceptance masks --------------------
        const Window win = make_window(x, y, b, W, H, S);
        uint32_t off = (uint32_t)(pix * S) + (uint32_t)min(t, S - 1); // own samples first
        if (p.members != nullptr) { // (uniform) the listed members of a wide pass's count kernel, already in that order
            if (live && t >= S) off = p.members[p.member_base[pix] + (uint64_t)(t - S)];
        } else {
            int rank = (live && t >= S) ? t - S : -1;        // the rank-th accepted candidate of the window
            const int nwords = (win.ncand + 63) >> 6;
            const uint64_t *pm = p.masks + pix * p.mask_stride;
            for (int w = 0; __any(rank >= 0) && w < (int)p.mask_stride; ++w) {
                unsigned long long m = (rank >= 0 && w < nwords) ? pm[w] : 0ull;
                const int c = __popcll(m);
                if (rank >= c) {
                    rank -= c;
                } else if (rank >= 0) {
                    for (int k = 0; k < rank; ++k) m &= m - 1ull;  // drop the lower set bits
                    off = candidate_offset(win, W, S, w * 64 + (__ffsll((long long)m) - 1));
                    rank = -1;
                }
            }
        }
        if (p.dbg.member_hash != nullptr) { // debug only: hash of the member list in order, by slot 0 of every group
            uint32_t *sOffD = reinterpret_cast<uint32_t *>(sU);
            sOffD[lane] = off;
            wsync();
            if (t == 0 && gvalid) p.dbg.member_hash[pix] = member_hash(sOffD + g * G, n, x, y, b, p.box, S, W);
            wsync();
        }

        // ---- the lane's sample vector, staged [group][column][slot]; masks and flags cleared ------------------------
        for (int c = 0; c < ndim; ++c) sU[(gbase + c) * G + t] = live ? load_col<T>(p, c, off) : 0.0;
        for (int k = lane; k < ndim * 16; k += 64) sMask[k] = 0ull;
        if (lane < 8) sFlag[lane] = 0;
        wsync();

        // ---- stage 2: in-order sums over the neighbourhood (rpf.cpp:596-601): lane t walks columns t, t + G, ... of its
        // group front to back, the column's minimum and maximum ride along; then the constants of the binning
        // (sd.h:229-232, mi.cpp:47-50)
        const double dn = (double)n;
        for (int c = t; c < ndim; c += G) {
            const double *src = sU + (gbase + c) * G;
            double sum = 0.0, sq = 0.0, mn = INFINITY, mx = -INFINITY;
            for (int j = 0; j < n; ++j) {
                const double v = src[j];
                sum = sum + v;                               // ops.h:121
                sq = sq + v * v;                             // ops.h:138
                mn = fmin(mn, v); mx = fmax(mx, v);
            }
            const ColumnConst cc = column_constants(sum, sq, mn, mx, dn, p.policy);
            double *st = sStat + (gbase + c) * 5;
            st[0] = cc.mean; st[1] = cc.sd; st[2] = cc.lo; st[3] = cc.range; st[4] = cc.flags;
            if (gvalid) {
                if (p.dbg.mean) p.dbg.mean[pix * ndim + c] = cc.mean;
                if (p.dbg.stddev) p.dbg.stddev[pix * ndim + c] = cc.sd;
            }
        }
        wsync();

        // ---- stage 3a: bin ids (a byte per sample and column); 3b: one bit mask per (pixel, column, bin value) -------
        const int B = max(1, (int)sqrt(dn));                 // mi.cpp:54
        for (int c = 0; c < ndim; ++c) {
            const double *st = sStat + (gbase + c) * 5;
            const int bin = bin_id(sU[(gbase + c) * G + t], st[0], st[1], st[2], st[3], (int)st[4], B);
            if (live) {
                sBin[(gbase + c) * G + t] = (uint8_t)bin;
                atomicOr(&sMask[(gbase + c) * BSTR + bin], 1ull << t);
            }
        }
        wsync();
        if (p.dbg.bin_hash != nullptr && gvalid) { // debug only: hash per column in sample order
            for (int c = t; c < ndim; c += G) p.dbg.bin_hash[pix * ndim + c] = bin_hash(sBin + (gbase + c) * G, n);
        }
        // marginals: sum_i T[hx_i] per column
        for (int c = t; c < ndim; c += G) {
            const unsigned long long *m = sMask + (gbase + c) * BSTR;
            uint64_t acc = 0ull;
            for (int v = 0; v < B; ++v) acc += sT[__popcll(m[v])];
            sHX[gbase + c] = acc;
        }
        wsync();
        // joint histograms: lane t takes the pairs t, t + G, ...; a cell's count is popcount(mask_a[i] & mask_b[j])
        bool redo = false;
        {
            const uint64_t TN = sT[n];
            for (int pr = t; pr < npair; pr += G) {
                const uint32_t cc = sPairTab[pr];
                const int ca = (int)(cc & 255u), cb = (int)(cc >> 8);
                const unsigned long long *ma = sMask + (gbase + ca) * BSTR, *mb = sMask + (gbase + cb) * BSTR;
                uint64_t acc = 0ull;
                for (int i = 0; i < B; ++i) {
                    const unsigned long long a = ma[i];
                    for (int j = 0; j < B; ++j) acc += sT[__popcll(a & mb[j])];   // T[J_ij], mi.cpp:39 / 79-86 over integer counts
                }
                const uint64_t hxa = sHX[gbase + ca], hxb = sHX[gbase + cb];
                const int64_t f = (int64_t)TN + (int64_t)acc - (int64_t)hxa - (int64_t)hxb;
                // REF_ABORT: the reference's own value for an in-band table is rounding residue unless its quotients are
                // exact (N a power of two, or a one-bin column): generic::filter_pixel_kernel evaluates it (redo list)
                bool inexact;
                const double mi = zero_band_mi(f, B, n, hxa, hxb, TN, kTFixBits, dn, inexact);
                if (p.redo_list != nullptr && inexact) redo = true;
                sMI[g * npair + pr] = mi;
                if (p.dbg.mi && gvalid) p.dbg.mi[pix * npair + pr] = mi;
            }
        }
        if (redo) sFlag[g] = 1;
        wsync();

        // ---- stage 3c: alpha, beta, W_r_c (rpf.cpp:444-487), the sums in filter_pixel_kernel's order of additions ------
        double *sDrf = sW + g * (2 * nF + 16), *sD9 = sDrf + nF, *sAlpha = sD9 + 12, *sBeta = sAlpha + 4;
        {
            const double *mi = sMI + g * npair;
            if (t < 3) { // colour channel t
                const int base = D.npairF + t * D.npairC;
                double Drc = 0.0, Dpc = 0.0, Dfc = 0.0;
                for (int l = 0; l < nR; ++l) Drc += mi[base + l];                      // rpf.cpp:432
                for (int l = 0; l < 2; ++l) Dpc += mi[base + nR + l];                  // rpf.cpp:436
                for (int j = 0; j < nF; ++j) Dfc += mi[base + nAnc + j];               // rpf.cpp:440
                sD9[t] = Drc; sD9[3 + t] = Dpc; sD9[6 + t] = Dfc;
            }
            for (int k = t; k < nF; k += G) {
                double Drf = 0.0;
                for (int l = 0; l < nR; ++l) Drf += mi[k * nAnc + l];                  // rpf.cpp:421
                sDrf[k] = Drf;
            }
            wsync();
            double D_f_c = 0.0, D_r_c = 0.0, D_p_c = 0.0;                              // rpf.cpp:449-456
            for (int i = 0; i < 3; ++i) { D_f_c += sD9[6 + i]; D_r_c += sD9[i]; D_p_c += sD9[3 + i]; }
            const double den = D_f_c + D_r_c + D_p_c + e_eps;
            double wsum = 0.0;
            for (int i = 0; i < 3; ++i) wsum += sD9[i] / (sD9[i] + sD9[3 + i] + e_eps); // rpf.cpp:470, 485
            const double wrc = wsum / 3;                                               // rpf.cpp:487
            const bool sched = (p.generic & kGenericSchedule) != 0; // RPF_FLAG_SCHEDULE with a gain other than 1: wave-uniform
            if (t < 3) {
                const double Drc = sD9[t], Dpc = sD9[3 + t];
                double alpha_c;
                if (sched) alpha_c = schedule_factor(p.gain_c, Drc / (Drc + Dpc + e_eps)); // clamp0(1 - g_c W_r^{c,t})
                else alpha_c = 1 - Drc / (Drc + Dpc + e_eps);                          // rpf.cpp:470, 475
                sAlpha[t] = alpha_c;
                if (p.dbg.alpha && gvalid) p.dbg.alpha[pix * 3 + t] = alpha_c;
            }
            if (t == 0) {
                sAlpha[3] = wrc;
                if (p.dbg.wrc && gvalid) p.dbg.wrc[pix] = wrc;
            }
            for (int k = t; k < nF; k += G) {
                const double Drf = sDrf[k];
                double Dpf = 0.0, Dcf = 0.0;
                for (int l = 0; l < 2; ++l) Dpf += mi[k * nAnc + nR + l];              // rpf.cpp:425
                for (int cc = 0; cc < 3; ++cc) Dcf += mi[D.npairF + cc * D.npairC + nAnc + k];
                const double num = beta_numerator(p.beta_map, k, k, Dcf, sD9, sDrf);
                double beta_k;
                if (sched) beta_k = schedule_factor(p.gain_f, Drf / (Drf + Dpf + e_eps)) * (num / den); // clamp0(1 - g_f W_r^{f,k}) W_c^{f,k}
                else beta_k = (1 - Drf / (Drf + Dpf + e_eps)) * (num / den);           // rpf.cpp:464-465, 479
                sBeta[k] = beta_k;
                if (p.dbg.beta && gvalid) p.dbg.beta[pix * nF + k] = beta_k;
            }
            wsync();
        }

        // ---- stage 4: weights and blend, term by term as rpf.cpp:646-717.  Lane = neighbourhood sample j; the weighted
        // columns are normalised in place (own sample i of the group is its slot i), kOwn own samples per sweep
        const double cj0 = sU[(gbase + 2) * G + t], cj1 = sU[(gbase + 3) * G + t], cj2 = sU[(gbase + 4) * G + t];
        bool bad = false;
        // own sample i of the group takes this lane's weight w: the four sums over the group, the quotient, the store
        auto blend = [&](int i, double w) {
            w = (live && i < S) ? w : 0.0;
            const double sw = group_sum<G>(w);                                 // rpf.cpp:691
            const double s0 = group_sum<G>(w * cj0), s1 = group_sum<G>(w * cj1), s2 = group_sum<G>(w * cj2); // rpf.cpp:692
            if (t < 3 && gvalid && i < S && store_filtered(p, t, pix, S, i, t == 0 ? s0 : (t == 1 ? s1 : s2), sw)) bad = true;
        };
        if constexpr (FAST) {
            // z = (x - M) / SD in fp64, rounded once and kept as the group's row of floats [column][slot] in the first half of
            // the column's fp64 row (a lane's store follows its own load; the rows of two columns are disjoint)
            for (int k = 0; k < nwt; ++k) {
                const int col = k < 5 ? k : k + nR;
                const double *st = sStat + (gbase + col) * 5;
                const double Mc = st[0], sd = st[1];
                const double xv = sU[(gbase + col) * G + t];
                wsync(); // every lane of the group has read its fp64 slot
                reinterpret_cast<zf32 *>(sU + (gbase + col) * G)[t] = (float)(sd == 0.0 ? 0.0 : (xv - Mc) / sd);
            }
            // the coefficients of the summed exponent with log2 e folded in, formed in fp64 and rounded once (the sums of
            // stage 3c they overwrite are dead)
            {
                const double wrc = sAlpha[3];
                const double sigma_c2 = p.seed * p.seed / (1 - wrc) / (1 - wrc);       // rpf.cpp:662
                const double sigma_p2 = p.sigma_p * p.sigma_p;
                const double kLog2e = 1.4426950408889634;
                zf32 *sCoefW = reinterpret_cast<zf32 *>(sDrf);
                for (int k = t; k < nwt; k += G)
                    sCoefW[k] = (float)((k < 2 ? 1.0 / (2 * sigma_p2) : (k < 5 ? sAlpha[k - 2] : sBeta[k - 5]) / (2 * sigma_c2)) * kLog2e);
            }
            wsync();
            const zf32 *sCoef = reinterpret_cast<const zf32 *>(sDrf);
            for (int i0 = 0; i0 < S; i0 += kOwn) {
                f32x2 E[kOwn / 2];
#pragma unroll
                for (int q = 0; q < kOwn / 2; ++q) E[q] = f32x2{0.f, 0.f};
                for (int k = 0; k < nwt; ++k) {
                    const int col = k < 5 ? k : k + nR;
                    const zf32 *zr = reinterpret_cast<const zf32 *>(sU + (gbase + col) * G);
                    const float zj = zr[t], ck = sCoef[k];
                    const f32x2 zj2 = f32x2{zj, zj}, ck2 = f32x2{ck, ck};
#pragma unroll
                    for (int q = 0; q < kOwn / 2; ++q) {
                        // (slots i0 .. i0 + kOwn - 1 lie inside the group's row: G is a multiple of kOwn; one past S - 1 weighs 0)
                        const f32x2 d = *reinterpret_cast<const f32x2a *>(zr + i0 + 2 * q) - zj2;
                        E[q] = __builtin_elementwise_fma(d * d, ck2, E[q]);
                    }
                }
#pragma unroll
                for (int ii = 0; ii < kOwn; ++ii) blend(i0 + ii, (double)__builtin_amdgcn_exp2f(-E[ii >> 1][ii & 1]));
            }
        } else {
            for (int k = 0; k < nwt; ++k) {
                const int col = k < 5 ? k : k + nR;
                const double *st = sStat + (gbase + col) * 5;
                const double Mc = st[0], sd = st[1];
                double *u = sU + (gbase + col) * G + t;
                const double xv = *u;
                *u = sd == 0.0 ? 0.0 : (xv - Mc) / sd;
            }
            wsync();
            const double wrc = sAlpha[3];
            const double sigma_c2 = p.seed * p.seed / (1 - wrc) / (1 - wrc);           // rpf.cpp:662
            const double sigma_p2 = p.sigma_p * p.sigma_p;
            for (int i0 = 0; i0 < S; i0 += kOwn) {
                double sp[kOwn], sc[kOwn], sf[kOwn];
#pragma unroll
                for (int ii = 0; ii < kOwn; ++ii) { sp[ii] = 0.0; sc[ii] = 0.0; sf[ii] = 0.0; }
                for (int k = 0; k < 2; ++k) {
                    const double *zr = sU + (gbase + k) * G;
                    const double zj = zr[t];
#pragma unroll
                    for (int ii = 0; ii < kOwn; ++ii) { const double d = zr[min(i0 + ii, S - 1)] - zj; sp[ii] += d * d; }
                }
                for (int k = 0; k < 3; ++k) {
                    const double *zr = sU + (gbase + 2 + k) * G;
                    const double zj = zr[t], ak = sAlpha[k];
#pragma unroll
                    for (int ii = 0; ii < kOwn; ++ii) { const double d = zr[min(i0 + ii, S - 1)] - zj; sc[ii] += (d * d) * ak; }
                }
                for (int k = 0; k < nF; ++k) {
                    const double *zr = sU + (gbase + colF + k) * G;
                    const double zj = zr[t], bk = sBeta[k];
#pragma unroll
                    for (int ii = 0; ii < kOwn; ++ii) { const double d = zr[min(i0 + ii, S - 1)] - zj; sf[ii] += (d * d) * bk; }
                }
#pragma unroll
                for (int ii = 0; ii < kOwn; ++ii)
                    blend(i0 + ii, exp(-sp[ii] / (2 * sigma_p2)) * exp(-sc[ii] / (2 * sigma_c2)) * exp(-sf[ii] / (2 * sigma_c2))); // rpf.cpp:667-670
            }
        }
        // status: one report per pixel; a pixel on the redo list reports nothing (generic::filter_pixel_kernel owns it)
        const unsigned long long badm = __ballot(bad);
        if (t == 0 && gvalid) {
            const unsigned long long gm = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << (g * G);
            if (sFlag[g] != 0) {
                p.redo_list[atomicAdd(p.redo_count, 1u)] = pixu;
            } else if (badm & gm) {
                atomicAdd(&p.status[0], 1);
                atomicMin(&p.status[1], (int)pixu);
            }
        }
    }
}

template <class T, int G, bool FAST>
hipError_t launch_packed_t(const PassParams &p, const GenericPackedCarve &cv, hipStream_t s) {
    hipError_t e = hipFuncSetAttribute((const void *)filter_packed_kernel<T, G, FAST>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cv.total);
    if (e != hipSuccess) return e;
    const uint32_t P = 64u / (uint32_t)G, units = (p.list_count + P - 1u) / P;
    // grid-stride walk: 2048 workgroups keep 256 CUs busy whatever the carve-up lets a CU hold
    const unsigned grid = (unsigned)std::min<uint32_t>((units + cv.waves - 1u) / cv.waves, 2048u);
    hipLaunchKernelGGL((filter_packed_kernel<T, G, FAST>), dim3(grid), dim3(64u * cv.waves), cv.total, s, p, cv);
    return hipGetLastError();
}

template <class T, bool FAST>
hipError_t launch_packed_g(const PassParams &p, const GenericPackedCarve &cv, int G, hipStream_t s) {
    switch (G) {
    case 8: return launch_packed_t<T, 8, FAST>(p, cv, s);
    case 16: return launch_packed_t<T, 16, FAST>(p, cv, s);
    case 32: return launch_packed_t<T, 32, FAST>(p, cv, s);
    case 64: return launch_packed_t<T, 64, FAST>(p, cv, s);
    default: return hipErrorInvalidValue;
    }
}

} // namespace

hipError_t launch_nbhd_count(const PassParams &p, hipStream_t s) {
    if (p.masks == nullptr || p.nbhd == nullptr || !p.lay.generic_ok()) return hipErrorInvalidValue;
    if (p.row_end <= p.row_begin) return hipSuccess;
    const uint64_t npix = (uint64_t)(p.row_end - p.row_begin) * p.W;
    const dim3 grid((unsigned)((npix + 3) / 4));
    if (p.lay.f16) hipLaunchKernelGGL(nbhd_count_kernel<__half>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(nbhd_count_kernel<float>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_filter_packed(const PassParams &p, int lanes_per_pixel, hipStream_t s, bool fast) {
    if (p.pix_list == nullptr || p.S > lanes_per_pixel || !p.lay.generic_ok()) return hipErrorInvalidValue;
    if (p.masks == nullptr && p.members == nullptr) return hipErrorInvalidValue; // one source of the member list
    if (p.members != nullptr && p.member_base == nullptr) return hipErrorInvalidValue;
    if (p.policy == RPF_DEGEN_REF_ABORT && p.redo_list != nullptr && p.redo_count == nullptr) return hipErrorInvalidValue;
    if (p.list_count == 0) return hipSuccess;
    const GenericPackedCarve cv = generic_packed_carve(p.lay);
    if ((int)cv.total > max_lds_per_block()) return hipErrorInvalidValue;
    if (fast) return p.lay.f16 ? launch_packed_g<__half, true>(p, cv, lanes_per_pixel, s) : launch_packed_g<float, true>(p, cv, lanes_per_pixel, s);
    return p.lay.f16 ? launch_packed_g<__half, false>(p, cv, lanes_per_pixel, s) : launch_packed_g<float, false>(p, cv, lanes_per_pixel, s);
}

} // namespace generic
} // namespace rpf
