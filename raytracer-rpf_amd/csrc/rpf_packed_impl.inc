// rpf_packed_impl.inc -- the small-neighbourhood kernels: several pixels per wavefront.  Included by rpf_filter_impl.inc
// (part 1) inside the layout's namespace; uses its constants (kNDim, kNFeat, kNPair, ...) and helpers.
//
// Why: a captured path-traced buffer keeps N = S samples for ~94 % of its pixels (SURVEY F10, H6): the 3-sigma test rejects
// nearly every neighbour.  filter_pixel_kernel gives such a pixel a whole wave64, of which 8 lanes carry samples.  Here a
// pixel gets G = 8, 16, 32 or 64 lanes (N <= G) and a wave filters P = 64 / G pixels at once; a lane owns ONE sample of ONE
// pixel (lane = g * G + t: group g, slot t = position in the reference's neighbourhood order), so the member list, the
// sample's 19 values and its bin ids live in registers.  The pixels of a launch come from the size-class lists of the
// count pass (nbhd_count_kernel: N and the acceptance masks of stage 1b), so the groups of a wave need not be neighbours.
//
// Per-pixel arithmetic is the reference's, statement for statement as in filter_pixel_kernel -- every stage output up to
// alpha / beta / W_r_c is the same bits, the colours agree to rounding (the wave sums of stage 4 associate differently):
//   1b  the lane's sample: slot t < S is own sample t; slot t >= S is the (t - S)-th set bit of the pixel's acceptance
//       masks (rank select), mapped to a plane offset in the reference's visiting order (rpf.cpp:556-586)
//   2   in-order sums (rpf.cpp:596-601): the 64 samples are staged in LDS as [group][column][slot]; lane t of a group
//       walks columns t, t + G, ... front to back (sum and sum of squares together, min / max riding along) and forms the
//       column's constants for the binning at once (column_constants_of)
//   3a  z and bin id of the lane's sample per column (bin_of_value: the three paths of bins_stage)
//   3b  histograms WITHOUT atomics-per-pair: per (pixel, column, bin value) one bit mask over the pixel's slots, built by
//       one LDS atomic-or per lane and column; a joint cell count is popcount(mask_a[i] & mask_b[j]).  Lane t evaluates the
//       pairs t, t + G, ...: B^2 popcounts + look-ups of T[k] = k ln k (2^-44 fixed point, the same exact integer sums as the
//       atomic route) against 96 x N atomics; the 19 marginals are popcounts of single masks
//   3c  alpha, beta, W_r_c: every lane forms the colour sums of its pixel, lane t features t, t + G, ...
//   4   lane = neighbourhood sample j; the own samples' rows [u_i | A_i] are broadcast from LDS; one exp per pair; the
//       four sums of an own sample are all-reduced over the G lanes of the group by DPP / permlane exchanges
// One wave's LDS operations execute in order and the workgroup's four waves never talk to each other: no s_barrier after
// the table load.
template <int G> struct PackedCfg {
    static constexpr int P = 64 / G;                                           // pixels per wave
    static constexpr int BMAX = G == 8 ? 2 : (G == 16 ? 4 : (G == 32 ? 5 : 8)); // floor(sqrt(N)), N <= G
    static constexpr int BSTR = G == 32 ? 8 : BMAX;                            // mask slots per (pixel, column)
    static constexpr int MW = G == 64 ? 2 : 1;                                 // 32-bit words per mask
    static_assert(P * BSTR * MW * 4 == 64, "64 bytes of masks per column and wave");
};
constexpr int kPkWaves = 4;                        // waves per workgroup (independent)
constexpr int kPkCK = 6;                           // doubles per column-constant record (16-byte aligned reads)
constexpr int kPkOR = (kNWt + 2) & ~1;             // doubles per own row: u_0 .. u_(kNWt-1), A (+ pad)
constexpr int kPkWS = (4 + kNFeat + 3) & ~3;       // doubles per pixel of the weight scratch: alpha[3], wrc | beta[kNFeat]
// per-wave LDS (bytes): U = staged samples [64][kNDim] doubles, then column constants, then MI values, then own rows
constexpr uint32_t kPkU = 64u * kNDim * 8u;
static_assert(8u * kNDim * kPkCK * 8u <= kPkU && 8u * kNPair * 8u <= kPkU && 64u * kPkOR * 8u <= kPkU, "the union region holds every tenant");
constexpr uint32_t kPkOffStat = kPkU;                                    // [P][kNDim][4] doubles: M, SD, 1/SD (0 if SD == 0), cz
constexpr uint32_t kPkOffMask = kPkOffStat + 8u * kNDim * 32u;           // [P][kNDim][BSTR] masks: 64 B per column
constexpr uint32_t kPkOffHX = kPkOffMask + kNDim * 64u;                  // [P][kNDim] u64: sum_i T[hx_i]
constexpr uint32_t kPkOffW = kPkOffHX + 8u * kNDim * 8u;                 // [P][kPkWS] doubles
constexpr uint32_t kPkOffFlag = kPkOffW + 8u * kPkWS * 8u;               // [P] ints: redo verdict
constexpr uint32_t kPkWaveBytes = (kPkOffFlag + 8u * 4u + 15u) & ~15u;
constexpr uint32_t kPkPairTabOff = 72u * 8u;                             // after T[0 .. 64]: the columns of every MI pair, two bytes each
constexpr uint32_t kPkTableBytes = (kPkPairTabOff + 2u * kNPair + 15u) & ~15u;
constexpr uint32_t kPkLdsBytes = kPkTableBytes + kPkWaves * kPkWaveBytes;

// all-reduce over the G lanes of a group (G = 8: half a DPP row, 16: a row, 32: a row pair, 64: the wave)
template <int G, class Op, class T>
__device__ __forceinline__ T group_allreduce(T v) {
    if constexpr (G == 64) return xl::allreduce<Op>(v);
    else if constexpr (G == 32) return xl::allreduce_row<Op>(xl::exch16<Op>(v, v));
    else if constexpr (G == 16) return xl::allreduce_row<Op>(v);
    else {
        v = Op::f(v, xl::dpp<xl::kRowHalfMirror>(v));
        return xl::allreduce_bits10<Op>(v);
    }
}

// Transposed butterfly over the G lanes of a group: v[ch * 8 + ii], ch = 0..3 (w, w c_r, w c_g, w c_b), ii = own sample of the
// sweep.  Every step halves the values a lane carries and doubles the lanes summed into each (rpf_xlane.h).  On return
//   G = 8:  r[ch] = total of v[ch * 8 + (t & 7)], all four channels
//   G = 16: r[0], r[1] = totals of channels 2 h, 2 h + 1 of own sample (t & 7), h = bit 3 of t
//   G = 32: r[0] = total of channel (bit 4, bit 3 of t) of own sample (t & 7); G = 64: the same in both halves of the wave
template <int G>
__device__ __forceinline__ void group_sums8(const double (&v)[32], int lane, double (&r)[4]) {
    using Sum = xl::OpSum;
    auto reduce8 = [&](const double (&a)[8]) -> double { // 8 values over the 8 lanes of a half row
        double x[4], y[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = xl::exch_row<Sum, xl::kRowHalfMirror, 4>(a[i], a[i + 4], lane);
#pragma unroll
        for (int i = 0; i < 2; ++i) y[i] = xl::exch_row<Sum, xl::kQuadXor2, 2>(x[i], x[i + 2], lane);
        return xl::exch_row<Sum, xl::kQuadXor1, 1>(y[0], y[1], lane);
    };
    if constexpr (G == 8) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            double a[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] = v[ch * 8 + i];
            r[ch] = reduce8(a);
        }
    } else if constexpr (G == 16) {
        double u[16]; // [ch0 * 8 + ii]: lanes with bit 3 clear keep channels 0, 1; the others 2, 3
#pragma unroll
        for (int i = 0; i < 16; ++i) u[i] = xl::exch_row<Sum, xl::kRowMirror, 8>(v[i], v[16 + i], lane);
#pragma unroll
        for (int c0 = 0; c0 < 2; ++c0) {
            double a[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] = u[c0 * 8 + i];
            r[c0] = reduce8(a);
        }
        r[2] = 0.0; r[3] = 0.0;
    } else {
        double u[16], s[8];
#pragma unroll
        for (int i = 0; i < 16; ++i) u[i] = xl::exch16<Sum>(v[i], v[16 + i]);                 // even rows: channels 0, 1; odd rows: 2, 3
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = xl::exch_row<Sum, xl::kRowMirror, 8>(u[i], u[8 + i], lane); // bit 3: the odd channel
        double tot = reduce8(s);
        if constexpr (G == 64) tot = xl::exch32<Sum>(tot, tot);
        r[0] = tot; r[1] = 0.0; r[2] = 0.0; r[3] = 0.0;
    }
}

// the per-column constants of stage 3a from the column's statistics (same statements as column_constants())
__device__ __forceinline__ void column_constants_of(double Mc, double SDc, double xlo, double xhi, double *ck) {
    const bool sd0 = (SDc == 0.0);
    const UDiv dsd = udiv_prepare(SDc);
    const double lo = sd0 ? 0.0 : udiv(xlo - Mc, dsd); // min_element over z (mi.cpp:47,49)
    const double hi = sd0 ? 0.0 : udiv(xhi - Mc, dsd); // max_element over z (mi.cpp:48,50)
    const double range = hi - lo;
    const bool flat = !(hi != lo);                       // mi.cpp:7 / 28 / 34
    const UDiv drg = udiv_prepare(range);
    const bool fast = dsd.fast && (flat || drg.fast);
    ck[0] = dsd.r; ck[1] = lo; ck[2] = range; ck[3] = drg.r;
    ck[4] = (double)((sd0 ? 1 : 0) | (flat ? 2 : 0) | (fast ? 4 : 0));
}

// bin id of one value (sd.h:229-232, mi.cpp:14-16): the three paths of bins_stage()'s do_column
__device__ __forceinline__ int bin_of_value(double xv, double Mc, double SDc, const double *ck, int B) {
    const double lo = ck[1], range = ck[2];
    const int flags = (int)ck[4];
    const bool sd0 = flags & 1, flat = flags & 2, fast = flags & 4;
    if (sd0 || flat) return 0;
    const double dB = (double)B;
    const double a = xv - Mc;                                      // subtractArrays
    double t;
    if (fast) {
        UDiv dsd, drg;
        dsd.b = SDc; dsd.r = ck[0]; dsd.fast = true;
        drg.b = range; drg.r = ck[3]; drg.fast = true;
        const double z = udiv_fast(a, dsd);                        // divideArrays, ops.h:48
        t = udiv_fast(z - lo, drg) * dB;                           // mi.cpp:14
    } else {
        const double z = a / SDc;
        t = (z - lo) / range * dB;
    }
    int bin = (int)t;
    bin = min(bin, B - 1);
    return max(bin, 0);
}

// One wave = one "unit" of P list entries at a time; the workgroups of an XCD (blockIdx % 8) walk that XCD's eighth of the
// list with a grid stride, so a launch sized for a full list costs nothing when the list is short or empty -- which is how
// the unbinned 8-spp route uses it: filter_pixel_kernel re-routes the pixels it finds small and leaves the list size in
// device memory (count_dev), and the host never learns it.
template <int G>
__global__ __launch_bounds__(64 * kPkWaves, kRef19 ? 2 : 1) void filter_packed_kernel(PassParams p, const uint32_t *count_dev) {
    using Cfg = PackedCfg<G>;
    constexpr int P = Cfg::P, BMAX = Cfg::BMAX, BSTR = Cfg::BSTR, MW = Cfg::MW;
    constexpr int R = (kNDim + G - 1) / G; // columns per lane in the column-parallel steps
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (count_dev != nullptr && *count_dev == 0u) return; // an empty class list (uniform): not even the table is loaded
    uint64_t *sT = reinterpret_cast<uint64_t *>(smem);
    for (int k = tid; k <= 64; k += 64 * kPkWaves) sT[k] = p.tfix[min(k, p.nmax)];
    uint16_t *sPairTab = reinterpret_cast<uint16_t *>(smem + kPkPairTabOff);
    for (int pr = tid; pr < kNPair; pr += 64 * kPkWaves) {
        int ca, cb;
        pair_cols(pr, ca, cb);
        sPairTab[pr] = (uint16_t)(ca | (cb << 8));
    }
    __syncthreads(); // the only barrier: from here on the waves are independent
    unsigned char *wb = smem + kPkTableBytes + (uint32_t)wv * kPkWaveBytes;
    double *sU = reinterpret_cast<double *>(wb);
    double *sStat = reinterpret_cast<double *>(wb + kPkOffStat);
    uint32_t *sMask = reinterpret_cast<uint32_t *>(wb + kPkOffMask);
    uint64_t *sHX = reinterpret_cast<uint64_t *>(wb + kPkOffHX);
    double *sW = reinterpret_cast<double *>(wb + kPkOffW);
    int *sFlag = reinterpret_cast<int *>(wb + kPkOffFlag);

    // ---- the wave's pixels: P consecutive entries of this XCD's chunk of the class list --------------------------
    const int W = p.W, H = p.H, S = p.S, b = p.b;
    const int g = lane / G, t = lane % G;
    const uint32_t list_count = count_dev ? *count_dev : p.list_count;
    const uint32_t chunk = (list_count + 7u) / 8u;
    const uint32_t units = (chunk + P - 1u) / P;                       // per XCD
    const uint32_t ustride = (gridDim.x >> 3) * kPkWaves;
    // the list entry and N of the NEXT unit are fetched while this one is filtered: two dependent global round trips off the
    // head of every unit (a wave runs a unit as one long dependent chain: at two waves per SIMD nothing else hides them)
    auto fetch_entry = [&](uint32_t unit, uint32_t &pixo, int &no, bool &valid) {
        const uint32_t q = unit * P + (uint32_t)g;
        const uint32_t e = (blockIdx.x & 7u) * chunk + q;
        valid = unit < units && q < chunk && e < list_count;
        pixo = valid ? p.pix_list[e] : 0u;
        no = valid ? min(p.nbhd[pixo], G) : 0;           // written by the count pass / the fused kernel; <= G by construction of the list
    };
    uint32_t pix_next = 0u;
    int n_next = 0;
    bool valid_next = false;
    const uint32_t unit0 = (blockIdx.x >> 3) * kPkWaves + (uint32_t)wv;
    fetch_entry(unit0, pix_next, n_next, valid_next);
    for (uint32_t unit = unit0; unit < units; unit += ustride) {
    const bool gvalid = valid_next;
    const uint32_t pixu = pix_next;
    const int n = n_next;
    fetch_entry(unit + ustride, pix_next, n_next, valid_next);
    wsync(); // the previous unit's LDS is dead
    if (!__any(gvalid)) continue; // (only the last unit of a chunk can be short)
    const uint64_t pix = pixu;
    const bool live = t < n;
    const int y = (int)(pixu / (uint32_t)W), x = (int)(pixu - (uint32_t)y * (uint32_t)W);
    // first (pixel, column) record of the group.  Opaque to the optimiser on purpose: as a loop invariant of the unit loop
    // every LDS address derived from it (19 columns x 5 regions) was hoisted in front of the loop -- 45 spilled registers;
    // re-formed per unit they are one shift-add each, or an immediate offset.
    int gbase = g * kNDim;
    asm volatile("" : "+v"(gbase));

    // ---------------- stage 1b: the lane's sample (rpf.cpp:556-586) -----------------------------------------------
    const int x0 = max(x - b, 0), x1 = min(x + b, W - 1);
    const int y0 = max(y - b, 0), y1 = min(y + b, H - 1);
    const int nyv = y1 - y0 + 1;
    const int centre_rank = (x - x0) * nyv + (y - y0);
    const int ncand = ((x1 - x0 + 1) * nyv - 1) * S;
    uint32_t off = (uint32_t)(pix * S) + (uint32_t)min(t, S - 1); // own samples first
    if constexpr (kListed) {
        // a listed build (RPF_IMPL_LISTED): the count kernel listed the members behind the own samples as plane offsets, in order
        if (live && t >= S) off = p.members[p.member_base[pix] + (uint64_t)(t - S)];
    } else {
        int rank = (live && t >= S) ? t - S : -1;            // the rank-th accepted candidate of the window
        const int nwords = (ncand + 63) >> 6;
        const uint64_t *pm = p.masks + pix * p.mask_stride;
        for (int w = 0; __any(rank >= 0) && w < (int)p.mask_stride; ++w) {
            unsigned long long m = (rank >= 0 && w < nwords) ? pm[w] : 0ull;
            const int c = __popcll(m);
            if (rank >= c) {
                rank -= c;
            } else if (rank >= 0) {
                for (int k = 0; k < rank; ++k) m &= m - 1ull;  // drop the lower set bits
                const int qq = w * 64 + (__ffsll((long long)m) - 1);
                int cell = qq / S;
                const int s = qq - cell * S;
                if (cell >= centre_rank) ++cell;              // rpf.cpp:565: skip the centre pixel
                const int ix = cell / nyv, iy = cell - ix * nyv; // xn outer, yn inner ascending (rpf.cpp:562-563)
                off = (uint32_t)(((uint64_t)(y0 + iy) * W + (x0 + ix)) * S + s);
                rank = -1;
            }
        }
    }
    if (p.dbg.member_hash != nullptr) { // debug only: hash of the member list in order, by slot 0 of every group
        uint32_t *sOffD = reinterpret_cast<uint32_t *>(sU);
        sOffD[lane] = off;
        wsync();
        if (t == 0 && gvalid) {
            uint32_t h = 2166136261u;
            for (int j = 0; j < n; ++j) {
                const uint32_t o = sOffD[g * G + j];
                const uint32_t s = o % (uint32_t)S, pp = o / (uint32_t)S;
                const int yn = (int)(pp / (uint32_t)W), xn = (int)(pp % (uint32_t)W);
                h = fnv1a_u32(h, (uint32_t)(((xn - x + b) * p.box + (yn - y + b)) * S) + s);
            }
            p.dbg.member_hash[pix] = h;
        }
        wsync();
    }

    // ---------------- the lane's sample vector ---------------------------------------------------------------------
    float xf[kNX];
    double xc[3];
#pragma unroll
    for (int i = 0; i < kNX; ++i) xf[i] = live ? ldp(p, xcol(i), off) : 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) xc[i] = live ? p.col_in[(uint64_t)i * p.plane_stride + off] : 0.0;
    auto xval = [&](int c) -> double { // column c of the sample vector (c is a compile-time constant at every call)
        return c < kColC ? (double)xf[c] : (c < kColC + 3 ? xc[c - kColC] : (double)xf[c - 3]);
    };

    // ---------------- stage 2: in-order sums over the neighbourhood (rpf.cpp:596-601) ------------------------------
    // staged [group][column][slot]; lane t walks columns t, t + G, ... of its group front to back
#pragma unroll
    for (int c = 0; c < kNDim; ++c) sU[(gbase + c) * G + t] = xval(c);
    wsync();
    const double dn = (double)n;
    double cM[R], cSD[R], cLo[R], cHi[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int c = min(r * G + t, kNDim - 1);
        const double *src = sU + (gbase + c) * G;
        double sum = 0.0, sq = 0.0, mn = INFINITY, mx = -INFINITY;
        // eight staged values per batch, read unconditionally (slots >= n hold this unit's dead lanes' zeros) and summed under
        // a select: with the reads inside `if (j < n)` every element was its own LDS round trip
#pragma unroll 1
        for (int j0 = 0; j0 < G; j0 += 8) {
            if (j0 >= n) break; // group-uniform
            double vb[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) vb[jj] = src[j0 + jj];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const bool on = j0 + jj < n;
                const double v = vb[jj];
                const double s1 = sum + v, s2 = sq + v * v;     // ops.h:121, 138
                sum = on ? s1 : sum;
                sq = on ? s2 : sq;
                mn = on ? fmin(mn, v) : mn;
                mx = on ? fmax(mx, v) : mx;
            }
        }
        const double mean = sum / dn;                       // ops.h:123
        double sd = sqrt(sq / dn - mean * mean);            // ops.h:141
        if (p.policy == RPF_DEGEN_EPS && isnan(sd)) sd = 0.0;
        cM[r] = mean; cSD[r] = sd; cLo[r] = mn; cHi[r] = mx;
        __builtin_amdgcn_sched_barrier(0);
    }
    wsync(); // every chain has read its staged column: the region now takes the column constants
    double *sCK = sU; // [P][kNDim][kPkCK]
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int c = r * G + t;
        if (c < kNDim && gvalid) {
            column_constants_of(cM[r], cSD[r], cLo[r], cHi[r], sCK + (gbase + c) * kPkCK);
            sStat[(gbase + c) * 4 + 0] = cM[r];
            sStat[(gbase + c) * 4 + 1] = cSD[r];
            if (p.dbg.mean) p.dbg.mean[pix * kNDim + c] = cM[r];
            if (p.dbg.stddev) p.dbg.stddev[pix * kNDim + c] = cSD[r];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // clear the masks (kNDim * 64 bytes per wave)
    for (int k = lane; k < kNDim * 16; k += 64) sMask[k] = 0u;
    if (lane < P) sFlag[lane] = 0;
    wsync();

    // ---------------- stage 3a: bin ids; 3b: one bit mask per (pixel, column, bin value) ----------------------------
    const int B = max(1, (int)sqrt(dn)); // mi.cpp:54
    uint64_t bp[2] = {0ull, 0ull};       // the lane's bin ids, 4 bits each (debug hash)
#pragma unroll
    for (int c = 0; c < kNDim; ++c) {
        const double *ck = sCK + (gbase + c) * kPkCK;
        const double2 ms = *reinterpret_cast<const double2 *>(sStat + (gbase + c) * 4);
        double ckr[5];
        {
            const double2 v0 = *reinterpret_cast<const double2 *>(ck), v1 = *reinterpret_cast<const double2 *>(ck + 2);
            ckr[0] = v0.x; ckr[1] = v0.y; ckr[2] = v1.x; ckr[3] = v1.y; ckr[4] = ck[4];
        }
        const int bin = live ? bin_of_value(xval(c), ms.x, ms.y, ckr, B) : 0;
        if (p.dbg.bin_hash != nullptr) bp[c >> 4] |= (uint64_t)bin << (4 * (c & 15));
        if (live) atomicOr(&sMask[((gbase + c) * BSTR + bin) * MW + (MW == 2 ? (t >> 5) : 0)], 1u << (t & 31));
        // (fully unrolled, the compiler hoists every column's LDS reads to the top: 19 x 14 live registers.  Fenced every third
        // column: three columns' reads share one LDS round trip.)
        if (c % 3 == 2) __builtin_amdgcn_sched_barrier(0);
    }
    wsync();
    if (p.dbg.bin_hash != nullptr) { // debug only: hash per column in sample order
        uint8_t *sBinD = reinterpret_cast<uint8_t *>(sHX); // [64][kNDim] bytes <= 8 * kNDim * 8
#pragma unroll
        for (int c = 0; c < kNDim; ++c) sBinD[lane * kNDim + c] = (uint8_t)((bp[c >> 4] >> (4 * (c & 15))) & 15u);
        wsync();
        for (int c = t; c < kNDim; c += G) {
            if (gvalid) {
                uint32_t h = 2166136261u;
                for (int j = 0; j < n; ++j) h = fnv1a_u16(h, sBinD[(g * G + j) * kNDim + c]);
                p.dbg.bin_hash[pix * kNDim + c] = h;
            }
        }
        wsync();
    }
    auto load_mask = [&](int col, int v) -> uint64_t {
        const uint32_t *m = sMask + ((gbase + col) * BSTR + v) * MW;
        if constexpr (MW == 2) return *reinterpret_cast<const uint64_t *>(m);
        else return (uint64_t)m[0];
    };
    auto popc = [](uint64_t m) -> int { return MW == 2 ? __popcll(m) : __popc((uint32_t)m); };
    // marginals: sum_i T[hx_i] per column
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int c = min(r * G + t, kNDim - 1);
        uint64_t acc = 0ull;
#pragma unroll
        for (int v = 0; v < BMAX; ++v) acc += sT[popc(load_mask(c, v))];
        if (r * G + t < kNDim) sHX[gbase + c] = acc;
    }
    wsync();
    // joint histograms: lane t takes the pairs t, t + G, ...
    double *sMI = sU; // [P][kNPair] (the column constants are dead: every lane has formed its bins)
    bool redo = false;
    {
        const int64_t TNf = (int64_t)sT[n];
        const int64_t zero_band = ((int64_t)B * B + 2 * B + 1) / 2 + 1;
        const UDiv ddn = udiv_prepare(dn); // dn = 1 .. 64: the exact three-instruction quotient (udiv_fast) applies
#pragma unroll 2
        for (int pr = t; pr < kNPair; pr += G) {
            const uint32_t cc = sPairTab[pr];
            const int ca = (int)(cc & 255u), cb = (int)(cc >> 8);
            uint64_t ma[BMAX], mb[BMAX];
#pragma unroll
            for (int v = 0; v < BMAX; ++v) { ma[v] = load_mask(ca, v); mb[v] = load_mask(cb, v); }
            uint64_t acc = 0ull;
#pragma unroll
            for (int i = 0; i < BMAX; ++i)
#pragma unroll
                for (int j = 0; j < BMAX; ++j) acc += sT[popc(ma[i] & mb[j])];   // T[J_ij], mi.cpp:39 / 79-86 over integer counts
            const int64_t hxa = (int64_t)sHX[gbase + ca], hxb = (int64_t)sHX[gbase + cb];
            int64_t f = TNf + (int64_t)acc - hxa - hxb;
            if (f <= zero_band && f >= -zero_band) { // see filter_pixel_kernel stage 3b: the snap, and the redo rule
                if (p.redo_list != nullptr && (n & (n - 1)) != 0 && hxa != TNf && hxb != TNf) redo = true;
                f = 0;
            }
            const double mi = gvalid ? udiv_fast(ldexp((double)f, -kTFixBits), ddn) : 0.0; // == ldexp(f, -44) / dn
            sMI[g * kNPair + pr] = mi;
            if (p.dbg.mi && gvalid) p.dbg.mi[pix * kNPair + pr] = mi;
        }
    }
    if (redo) sFlag[g] = 1;
    wsync();

    // ---------------- stage 3c: alpha, beta, W_r_c (rpf.cpp:444-487) ------------------------------------------------
    // every lane forms the three colours' sums of its pixel (same order of additions as filter_pixel_kernel)
    double *sWg = sW + g * kPkWS;
    {
        const double *mi = sMI + g * kNPair;
        double Drc[3], Dpc[3], Dfc[3];
        { // lane t < 3 sums colour channel t (same order of additions as filter_pixel_kernel); the nine sums meet in LDS
            const int c = min(t, 2);
            const int base = kNPairF + c * kNPairC;
            double a = 0.0, bq = 0.0, f = 0.0;
#pragma unroll
            for (int l = 0; l < kNR; ++l) a += mi[base + l];                 // rpf.cpp:432
#pragma unroll
            for (int l = 0; l < 2; ++l) bq += mi[base + kNR + l];            // rpf.cpp:436
#pragma unroll
            for (int j = 0; j < kNFeat; ++j) f += mi[base + kNAnc + j];      // rpf.cpp:440
            if (t < 3) { sWg[4 + t] = a; sWg[7 + t] = bq; sWg[10 + t] = f; } // (beta's slots: written below, after these are read)
            wsync();
#pragma unroll
            for (int i = 0; i < 3; ++i) { Drc[i] = sWg[4 + i]; Dpc[i] = sWg[7 + i]; Dfc[i] = sWg[10 + i]; }
            wsync();
        }
        double D_f_c = 0.0, D_r_c = 0.0, D_p_c = 0.0;                         // rpf.cpp:449-456
#pragma unroll
        for (int i = 0; i < 3; ++i) { D_f_c += Dfc[i]; D_r_c += Drc[i]; D_p_c += Dpc[i]; }
        const double eps = (p.policy == RPF_DEGEN_EPS) ? p.eps : 0.0;
        const double den = D_f_c + D_r_c + D_p_c + eps;
        double wsum = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) wsum += Drc[i] / (Drc[i] + Dpc[i] + eps); // rpf.cpp:470, 485
        const double wrc = wsum / 3;                                          // rpf.cpp:487
        // lane t: colour channel t (alpha), features t, t + G, ...
        const int c3 = min(t, 2);
#if RPF_IMPL_SCHED
        const double alpha_c = schedule_factor(p.gain_c, (c3 == 0 ? Drc[0] : (c3 == 1 ? Drc[1] : Drc[2])) / // clamp0(1 - g_c W_r^{c,k}): DESIGN.md 15a
                                       ((c3 == 0 ? Drc[0] : (c3 == 1 ? Drc[1] : Drc[2])) + (c3 == 0 ? Dpc[0] : (c3 == 1 ? Dpc[1] : Dpc[2])) + eps));
#else
        const double alpha_c = 1 - (c3 == 0 ? Drc[0] : (c3 == 1 ? Drc[1] : Drc[2])) /
                                       ((c3 == 0 ? Drc[0] : (c3 == 1 ? Drc[1] : Drc[2])) + (c3 == 0 ? Dpc[0] : (c3 == 1 ? Dpc[1] : Dpc[2])) + eps); // rpf.cpp:470, 475
#endif
        wsync(); // every lane has read its MI values
        if (t < 3 && gvalid) {
            sWg[t] = alpha_c;
            if (p.dbg.alpha) p.dbg.alpha[pix * 3 + t] = alpha_c;
        }
        if (t == 0 && gvalid) {
            sWg[3] = wrc;
            if (p.dbg.wrc) p.dbg.wrc[pix] = wrc;
        }
        for (int k = t; k < kNFeat; k += G) {
            double Drf = 0.0, Dpf = 0.0, Dcf = 0.0;
#pragma unroll
            for (int l = 0; l < kNR; ++l) Drf += mi[k * kNAnc + l];           // rpf.cpp:421
#pragma unroll
            for (int l = 0; l < 2; ++l) Dpf += mi[k * kNAnc + kNR + l];       // rpf.cpp:425
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) Dcf += mi[kNPairF + cc * kNPairC + kNAnc + k]; // PAPER numerator
            double num; // what rpf.cpp:464 reads as D_f_ck[k] (3-element array indexed to 11: SURVEY F3)
            if (p.beta_map == RPF_BETA_PAPER) {
                num = Dcf;
            } else {
                const int shift = p.beta_map == RPF_BETA_REF_GCC11_O2 ? 8 : 4;
                if (k < 3) {
                    num = k == 0 ? Dfc[0] : (k == 1 ? Dfc[1] : Dfc[2]);
                } else if (k < shift) {
                    num = 0.0;
                } else { // D_r_fk[k - shift]: that feature's own sum (rpf.cpp:421)
                    double d2 = 0.0;
#pragma unroll
                    for (int l = 0; l < kNR; ++l) d2 += mi[(k - shift) * kNAnc + l];
                    num = d2;
                }
            }
            const double Wc = num / den;                       // rpf.cpp:464
            const double Wr = Drf / (Drf + Dpf + eps);         // rpf.cpp:465
#if RPF_IMPL_SCHED
            const double beta_k = schedule_factor(p.gain_f, Wr) * Wc; // clamp0(1 - g_f W_r^{f,k}) W_c^{f,k}: DESIGN.md 15a
#else
            const double beta_k = (1 - Wr) * Wc;               // rpf.cpp:479
#endif
            if (gvalid) {
                sWg[4 + k] = beta_k;
                if (p.dbg.beta) p.dbg.beta[pix * kNFeat + k] = beta_k;
            }
        }
        wsync();
        // weighted columns: 1 / SD and cz_k = weight_k / (2 sigma^2) next to M and SD (rpf.cpp:662-668)
        const double sigma_c2 = p.seed * p.seed / (1 - wrc) / (1 - wrc);
        const double inv2sc = 1.0 / (2 * sigma_c2), inv2sp = 1.0 / (2 * (p.sigma_p * p.sigma_p));
        for (int k = t; k < kNWt; k += G) {
            const int col = k < 5 ? k : k + kNR;
            const double sd = sStat[(gbase + col) * 4 + 1];
            const double wkk = k < 2 ? 1.0 : (k < 5 ? sWg[k - 2] : sWg[4 + (k - 5)]);
            sStat[(gbase + col) * 4 + 2] = (sd == 0.0) ? 0.0 : 1.0 / sd; // SD == 0 normalises to z == 0 (ops.h:48)
            sStat[(gbase + col) * 4 + 3] = wkk * (k < 2 ? inv2sp : inv2sc);
        }
        wsync();
    }

    // ---------------- stage 4: weights and blend (rpf.cpp:627-717), z-space as in filter_pixel_kernel ---------------
    double zj[kNWt], Bj = 0.0;
#pragma unroll
    for (int k = 0; k < kNWt; ++k) {
        const int col = k < 5 ? k : k + kNR;
        const double2 ms = *reinterpret_cast<const double2 *>(sStat + (gbase + col) * 4);
        const double2 ic = *reinterpret_cast<const double2 *>(sStat + (gbase + col) * 4 + 2);
        const double z = ic.x == 0.0 ? 0.0 : (xval(col) - ms.x) * ic.x; // SD == 0: z = 0 (ops.h:48), also where x - M is not finite
        zj[k] = z;
        Bj = fma(ic.y * z, z, Bj);
        if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    double *sOwnU = sU; // [64][kPkOR]: row of own sample i of group g at lane index g * G + i (the MI values are dead)
    if (t < S) {
        double *row = sOwnU + lane * kPkOR;
#pragma unroll
        for (int k = 0; k < kNWt; ++k) {
            const int col = k < 5 ? k : k + kNR;
            row[k] = -2.0 * (sStat[(gbase + col) * 4 + 3] * zj[k]);
        }
        row[kNWt] = Bj; // A_i: the same sum of the same products
    }
    wsync();
    bool bad = false;
    constexpr int kW4 = (kNWt / 4) * 4;
    // Eight own samples per sweep: every lane weighs its sample against eight rows, and the 8 x 4 sums (w, w c_r, w c_g,
    // w c_b) are totalled over the G lanes of the group by ONE transposed butterfly (group_sums8) that leaves lane (t & 7)
    // with the sums of own sample i0 + (t & 7) -- 28 exchanges and three quotients per lane at G = 8, where an all-reduce
    // per own sample and sum was 8 x 4 x 3 exchanges and eight rounds of quotient + store.
    for (int i0 = 0; i0 < S; i0 += 8) {
        double v[32];
#pragma unroll
        for (int ii = 0; ii < 8; ++ii) {
            const int i = min(i0 + ii, S - 1);
            const double2 *ui2 = reinterpret_cast<const double2 *>(sOwnU + (g * G + i) * kPkOR);
            double ui[kPkOR];
#pragma unroll
            for (int qd = 0; qd < kPkOR / 2; ++qd) { const double2 q2 = ui2[qd]; ui[2 * qd] = q2.x; ui[2 * qd + 1] = q2.y; }
            double e0 = ui[kNWt] + Bj, e1 = 0.0, e2 = 0.0, e3 = 0.0;
#pragma unroll
            for (int k = 0; k < kW4; k += 4) {
                e0 = fma(ui[k], zj[k], e0);
                e1 = fma(ui[k + 1], zj[k + 1], e1);
                e2 = fma(ui[k + 2], zj[k + 2], e2);
                e3 = fma(ui[k + 3], zj[k + 3], e3);
            }
#pragma unroll
            for (int k = kW4; k < kNWt; ++k) e0 = fma(ui[k], zj[k], e0);
            const double E = (e0 + e1) + (e2 + e3);
            double w = exp(-E);                         // rpf.cpp:667-670
            w = (live && i0 + ii < S) ? w : 0.0;
            v[ii] = w;                                  // rpf.cpp:691
            v[8 + ii] = w * xc[0];                      // rpf.cpp:692 (raw neighbourhood colours)
            v[16 + ii] = w * xc[1];
            v[24 + ii] = w * xc[2];
            if (ii & 1) __builtin_amdgcn_sched_barrier(0); // two rows' chains interleave; unfenced, eight rows' reads are hoisted
        }
        double tw, tc; // this lane's output: sum of w and sum of w * colour[ch] of own sample i0 + (t & 7)
        int ch;        // 0 .. 2, or -1: the lane writes nothing
        double r[4];
        group_sums8<G>(v, lane, r);
        const int ii = t & 7, i = i0 + ii;
        if constexpr (G == 8) {
            // all four sums in this lane: three outputs
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (gvalid && i < S) {
                    double prime = r[1 + c] / r[0];                                   // rpf.cpp:700
                    if (isnan(prime)) {                                               // rpf.cpp:702: the reference exits here
                        bad = true;
                        if (p.policy == RPF_DEGEN_EPS) prime = p.col_in[(uint64_t)c * p.plane_stride + pix * S + i];
                    }
                    p.col_out[(uint64_t)c * p.plane_stride + pix * S + i] = prime;
                }
            }
            (void)tw; (void)tc; (void)ch;
        } else {
            if constexpr (G == 16) {
                // lanes 0..7 hold (w, c_r), lanes 8..15 (c_g, c_b): the latter fetch w from eight lanes below (DPP row_shr:8)
                const double wlo = xl::dpp<0x118>(r[0]);
                const bool hi = (t & 8) != 0;
                tw = hi ? wlo : r[0];
                // two outputs for the upper lanes: handled as two rounds below
                for (int rd = 0; rd < 2; ++rd) {
                    ch = hi ? 1 + rd : (rd == 0 ? 0 : -1);
                    tc = hi ? r[rd] : r[1];
                    if (ch >= 0 && gvalid && i < S) {
                        double prime = tc / tw;
                        if (isnan(prime)) {
                            bad = true;
                            if (p.policy == RPF_DEGEN_EPS) prime = p.col_in[(uint64_t)ch * p.plane_stride + pix * S + i];
                        }
                        p.col_out[(uint64_t)ch * p.plane_stride + pix * S + i] = prime;
                    }
                }
            } else {
                // one sum per lane: channel index = bits 4:3 of the slot (0 = w); w comes from lane (t & 7) of the group's 32
                const int sl = t & 31;
                const int chi = (sl >> 3) & 3;
                tw = __shfl(r[0], (lane & ~31) | (sl & 7), 64);
                tc = r[0];
                ch = chi - 1;
                if (ch >= 0 && (G == 32 || t < 32) && gvalid && i < S) {
                    double prime = tc / tw;
                    if (isnan(prime)) {
                        bad = true;
                        if (p.policy == RPF_DEGEN_EPS) prime = p.col_in[(uint64_t)ch * p.plane_stride + pix * S + i];
                    }
                    p.col_out[(uint64_t)ch * p.plane_stride + pix * S + i] = prime;
                }
            }
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
    } // unit loop
}

template <int G>
hipError_t launch_packed_inst(const PassParams &p, const uint32_t *count_dev, uint32_t max_count, hipStream_t s) {
    hipError_t e = hipFuncSetAttribute((const void *)filter_packed_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPkLdsBytes);
    if (e != hipSuccess) return e;
    const uint32_t chunk = (max_count + 7u) / 8u;
    const uint32_t per_block = (uint32_t)(kPkWaves * PackedCfg<G>::P);
    unsigned grid = 8u * ((chunk + per_block - 1u) / per_block);
    if (grid == 0) return hipSuccess;
    if (grid > 8u * 512u) grid = 8u * 512u; // grid-stride walk: 4096 workgroups keep 256 CUs busy, an empty list costs them nothing
    hipLaunchKernelGGL((filter_packed_kernel<G>), dim3(grid), dim3(64 * kPkWaves), kPkLdsBytes, s, p, count_dev);
    return hipGetLastError();
}

// entry point: pixels of p.pix_list with N <= lanes_per_pixel (8, 16, 32, 64); needs the acceptance masks and the N plane
// (count pass, or filter_pixel_kernel's re-route).  count_dev != null: the list size is read on the device and
// p.list_count is only its upper bound (sizes the grid).  (A listed build needs the member pool for the masks)
hipError_t impl_filter_packed(const PassParams &p, int lanes_per_pixel, const uint32_t *count_dev, hipStream_t s) {
    if (!pass_fits_build(p)) return hipErrorInvalidValue;
    if (kListed ? (p.members == nullptr || p.member_base == nullptr) : p.masks == nullptr) return hipErrorInvalidValue;
    if (p.pix_list == nullptr || p.S > lanes_per_pixel) return hipErrorInvalidValue;
    switch (lanes_per_pixel) {
    case 8: return launch_packed_inst<8>(p, count_dev, p.list_count, s);
    case 16: return launch_packed_inst<16>(p, count_dev, p.list_count, s);
    case 32: return launch_packed_inst<32>(p, count_dev, p.list_count, s);
    case 64: return launch_packed_inst<64>(p, count_dev, p.list_count, s);
    default: return hipErrorInvalidValue;
    }
}
