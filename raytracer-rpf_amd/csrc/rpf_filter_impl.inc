// rpf_filter_impl.inc -- the dimension-dependent kernels: included by the rpf_impl_*.hip translation units once per supported
// sample-vector layout and size-class part (RPF_IMPL_PART: 1 = K <= 8 kernels + stage 1a + count pass + streaming kernel,
// 2 = K 13 / 25, 3 = K 49, 4 = the count pass under the membership test alone, so that the code objects of parts 1 to 3 are
// what they were before it existed; the parts compile in parallel) through rpf_impl_unit.inc, which opens the namespace of the
// layout and build and sets
//     RPF_IMPL_NR   number of random-parameter columns  (reference: 2, sd.h:42 SD_N_RANDOM)
//     RPF_IMPL_NF   number of scene-feature columns     (reference: 12, sd.h:40 SD_N_FEATURES)
//     RPF_IMPL_PLANE_T  storage type of the feature planes (float, or __half for fp16 feature storage)
// Column layout of a sample vector (sd.h:62-94 generalised): [0,2) pFilm | [2,5) colour | [5,5+NR) random parameters |
// [5+NR, 5+NR+NF) features.  Everything else (stages, parity rules) is described in rpf_kernels.hip / DESIGN.md.

// RPF_IMPL_SCHED 1 (the rpf_impl_*_sched_* translation units, inside a nested namespace `sched`; RPF_FLAG_SCHEDULE_FUSED, DESIGN.md
// section 15e): the same part with stage 3c formed from PassParams::gain_c / gain_f (schedule_factor), and nothing a scheduled pass
// does not launch -- the non-FAST filter_pixel_kernel instantiations of PHASE 0 and PHASE 4 (and, in part 1, the packed kernels); no
// stage 1a, count or PHASE 2 / 3 kernels: those have no stage 3c, and the unscheduled parts launch them (impl_filter_*_phase)
#ifndef RPF_IMPL_SCHED
#define RPF_IMPL_SCHED 0
#endif
constexpr bool kSched = RPF_IMPL_SCHED != 0;
// RPF_IMPL_LISTED 1 (the rpf_impl_*_listed_* translation units, inside a nested namespace `listed`, and `listed::sched` together
// with RPF_IMPL_SCHED; RPF_FLAG_SAMPLED_LISTED, DESIGN.md section 13g): the same part with stage 1b reading the member list a
// count kernel left -- N from p.nbhd, the N - S plane offsets behind the own samples from p.members / p.member_base -- instead
// of testing the window or walking its acceptance masks; everything behind stage 1b is the text it was.  Such a build reads
// neither p.masks nor p.reroute_masks nor stage 1a's flat plane and does not write p.nbhd.  It holds the non-FAST
// filter_pixel_kernel instantiations (PHASES 0, 2, 3 and 4; with RPF_IMPL_SCHED PHASES 0 and 4, the listed part launches 2 and
// 3) and, in part 1, the packed kernels; no stage 1a and no count kernels
#ifndef RPF_IMPL_LISTED
#define RPF_IMPL_LISTED 0
#endif
constexpr bool kListed = RPF_IMPL_LISTED != 0;
constexpr int kNR = RPF_IMPL_NR;               // random-parameter columns
constexpr int kNFeat = RPF_IMPL_NF;            // scene-feature columns
constexpr int kColP = 0, kColC = 2, kColR = 5, kColF = 5 + kNR;
constexpr int kNDim = 5 + kNR + kNFeat;        // 19 in the reference (sd.h:21-49)
constexpr int kNX = kNDim - 3;                 // columns read from the feature planes (all but the fp64 colours)
constexpr int kNAnc = kNR + 2;                 // r.. and p.. anchors: every feature and colour is paired with each
constexpr int kNPairF = kNFeat * kNAnc;        // pairs (f_i, r_l | p_l)                       rpf.cpp:416-427
constexpr int kNPairC = kNAnc + kNFeat;        // pairs of one colour channel                  rpf.cpp:429-442
constexpr int kNPair = kNPairF + 3 * kNPairC;  // 96 in the reference
#ifndef RPF_CHAIN_BOTH
#define RPF_CHAIN_BOTH 1 // stage 2, one-wave kernels: 1 = lanes 0..18 carry the sum(x) and the sum(x*x) chain of their column; 0 = lanes 32..50 carry the second (a select per element)
#endif
#ifndef RPF_Z_HOIST
#define RPF_Z_HOIST 1 // stage 4, one-wave kernels: 1 = a sweep loop without the SD == 0 select for pixels whose weighted columns all have SD != 0
#endif
#ifndef RPF_ROWS_EARLY
#define RPF_ROWS_EARLY 1 // stage 4: own rows read in front of the own-sample loop (0: where the compiler sinks them; 1080p x 8: 65.1 vs 62.9 ms)
#endif
constexpr int kNWt = 5 + kNFeat;               // weighted columns of stage 4: pFilm, colour, features (17)
constexpr bool kRef19 = (kNR == 2 && kNFeat == 12); // the reference layout: the tuned small-K paths are written for it
using plane_t = RPF_IMPL_PLANE_T;
static_assert(kNDim <= 32 && kNFeat <= 32, "lane maps: one chain lane per column inside a 32-lane half");

// non-colour column i (0 .. kNX-1) -> column of the sample vector
__host__ __device__ constexpr int xcol(int i) { return i < 2 ? i : i + 3; }
// feature-plane value as the fp32 it stands for (fp16 storage converts exactly)
__device__ __forceinline__ float ldp(const PassParams &p, int col, uint32_t off) {
    return (float)reinterpret_cast<const plane_t *>(p.planes)[(uint64_t)col * p.plane_stride + off];
}
// columns of MI pair pr, in ComputeCFWeights call order (rpf.cpp:416-442)
__device__ __forceinline__ void pair_cols(int pr, int &ca, int &cb) {
    if (pr < kNPairF) {
        const int i = pr / kNAnc, l = pr - i * kNAnc;
        ca = kColF + i;
        cb = l < kNR ? kColR + l : kColP + (l - kNR);
    } else {
        const int q = pr - kNPairF, c = q / kNPairC, l = q - c * kNPairC;
        ca = kColC + c;
        cb = l < kNR ? kColR + l : (l < kNAnc ? kColP + (l - kNR) : kColF + (l - kNAnc));
    }
}
// index of the pair (anchor a, partner i): a = 0..kNR-1 r, kNR..kNAnc-1 p, kNAnc..kNAnc+2 colour anchors;
// i = 0..kNFeat-1 features, kNFeat..kNFeat+2 colour partners (r / p anchors only)
__device__ __forceinline__ int pair_index_of(int a, int i) {
    return a < kNAnc ? (i < kNFeat ? i * kNAnc + a : kNPairF + (i - kNFeat) * kNPairC + a)
                     : kNPairF + (a - kNAnc) * kNPairC + kNAnc + i;
}
// column of anchor a
__device__ __forceinline__ int anchor_col(int a) { return a < kNR ? kColR + a : (a < kNAnc ? kColP + (a - kNR) : kColC + (a - kNAnc)); }

// ---- the planes as the fused per-pixel kernel gathers from them ----------------------------------------------------
// The member list of a pixel (sOff) holds each sample's element offset RELATIVE to the first sample of the pixel's window,
// ((y0 * W + x0) * S: the smallest plane offset of the window, so a relative offset is >= 0 and < box * W * S), and the
// window origin is folded into the wave-uniform base of each plane.  A gather is then `global_load v, v_off32, s[base]`
// with a 32-bit per-lane byte offset (sbase / ldg_rel, rpf_device_common.h) and no per-lane address arithmetic beyond the
// shift that turns the element offset into bytes; stepping the base from one column's plane to the next is two scalar
// adds.  setup_pass refuses a call whose window span box * W * S * 8 bytes does not fit 32 bits (rpf_check_window_span).
struct Window {
    gchar *pl, *co;  // feature plane 0 / colour plane 0 at the window origin
    uint64_t pb, cb; // bytes per feature plane / per colour plane
    __device__ __forceinline__ Window(const PassParams &p, uint64_t origin)
        : pl(gptr(p.planes) + origin * sizeof(plane_t)), co(gptr(p.col_in) + origin * 8u),
          pb(p.plane_stride * sizeof(plane_t)), cb(p.plane_stride * 8u) {}
    __device__ __forceinline__ gchar *plane(int c) const { return sbase(pl + (uint64_t)c * pb); }
    __device__ __forceinline__ gchar *colour(int c) const { return sbase(co + (uint64_t)c * cb); }
    __device__ __forceinline__ gchar *next_plane(gchar *q, int n = 1) const { return sbase(q + (uint64_t)n * pb); }
    __device__ __forceinline__ gchar *next_colour(gchar *q) const { return sbase(q + cb); }
};
// feature-plane value at relative element offset `rel` of the plane based at q, as the fp32 it stands for
__device__ __forceinline__ float ldw(gchar *q, uint32_t rel) {
    if constexpr (sizeof(plane_t) == 2) return (float)__ushort_as_half(ldg_rel<unsigned short>(q, rel << 1));
    else return ldg_rel<float>(q, rel << 2);
}
// fp64 colour at relative element offset `rel` of the colour plane based at q
__device__ __forceinline__ double ldwc(gchar *q, uint32_t rel) { return ldg_rel<double>(q, rel << 3); }
// ... and both from the offset already in bytes of a feature plane (rel * sizeof(plane_t): formed once where it is reused)
constexpr int kPlaneShift = sizeof(plane_t) == 2 ? 1 : 2;
__device__ __forceinline__ float ldw_b(gchar *q, uint32_t pb) {
    if constexpr (sizeof(plane_t) == 2) return (float)__ushort_as_half(ldg_rel<unsigned short>(q, pb));
    else return ldg_rel<float>(q, pb);
}
__device__ __forceinline__ double ldwc_b(gchar *q, uint32_t pb) { return ldg_rel<double>(q, pb << (3 - kPlaneShift)); }
// the kNX plane columns (xcol order) and the three colours of one sample
__device__ __forceinline__ void gather_sample(const Window &w, uint32_t rel, float (&vf)[kNX], double (&vd)[3]) {
    gchar *q = w.plane(0);
#pragma unroll
    for (int i = 0; i < kNX; ++i) {
        vf[i] = ldw(q, rel);
        if (i + 1 < kNX) q = w.next_plane(q, xcol(i + 1) - xcol(i));
    }
    gchar *c = w.colour(0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        vd[i] = ldwc(c, rel);
        if (i < 2) c = w.next_colour(c);
    }
}
// the kNFeat feature columns of one sample (stage 1b)
__device__ __forceinline__ void gather_features(const Window &w, uint32_t rel, float (&f)[kNFeat]) {
    gchar *q = w.plane(kColF);
#pragma unroll
    for (int k = 0; k < kNFeat; ++k) {
        f[k] = ldw(q, rel);
        if (k + 1 < kNFeat) q = w.next_plane(q);
    }
}
// stage 4's columns of one sample: pFilm and the features (pf), the colours (pc)
__device__ __forceinline__ void gather_weighted(const Window &w, uint32_t rel, float (&pf)[2 + kNFeat], double (&pc)[3]) {
    gchar *q = w.plane(0);
#pragma unroll
    for (int k = 0; k < 2 + kNFeat; ++k) {
        pf[k] = ldw(q, rel);
        if (k + 1 < 2 + kNFeat) q = w.next_plane(q, k == 1 ? kColF - 1 : 1);
    }
    gchar *c = w.colour(0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        pc[i] = ldwc(c, rel);
        if (i < 2) c = w.next_colour(c);
    }
}

#if RPF_IMPL_PART == 1 && !RPF_IMPL_SCHED && !RPF_IMPL_LISTED
// ------------------------------------------------------------------------------------------------
// stage 1a: per-pixel mean / std of the 12 features over the pixel's own S samples, sequential sums
// (rpf.cpp:338-347, ops.h:111-144).  Output planes [12][H*W] so the filter kernel reads them with
// wave-uniform (scalar) loads.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pixel_stats_kernel(PassParams p, uint64_t pix0, uint64_t pix1) {
    const uint64_t HW = (uint64_t)p.H * p.W;
    const uint64_t pix = pix0 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= pix1) return;
    const double dn = (double)p.S;
    bool flat = false, any_nan = false; // by-products for stage 1b (PassParams::flat)
    for (int k = 0; k < kNFeat; ++k) {
        const plane_t *src = reinterpret_cast<const plane_t *>(p.planes) + (uint64_t)(kColF + k) * p.plane_stride + pix * p.S;
        double sum = 0.0, sq = 0.0;
        for (int s = 0; s < p.S; ++s) {
            double v = (double)(float)src[s];
            sum = sum + v;     // ops.h:121
            sq = sq + v * v;   // ops.h:138 (v*v is exact for fp32-valued v)
        }
        double mean = sum / dn;                     // ops.h:123
        double sd = sqrt(sq / dn - mean * mean);    // ops.h:141
        if (p.policy == RPF_DEGEN_EPS && isnan(sd)) sd = 0.0;
        ((double *)p.pmean)[(uint64_t)k * HW + pix] = mean;
        ((double *)p.pstd)[(uint64_t)k * HW + pix] = sd;
        any_nan = any_nan || isnan(mean);
        flat = flat || (sd * 3.0 == 0.0 && isfinite(mean)); // multiplyArray(std, 3) == 0: rejects every finite candidate
    }
    if (p.flat != nullptr) {
        p.flat[pix] = flat ? 1 : 0;
        if (any_nan) atomicOr(p.nan_flag, 1);
    }
}

// The same sums for S >= 16 through LDS.  One thread per pixel reads its S samples at a stride of S elements: at 32 spp every
// load instruction of a wave touches 64 cache lines and uses four bytes of each, 32 times over -- with a CU's worth of waves the
// lines do not survive in L1 / L2 until their next use (measured on a 3840x276x32 slab: 20.9 GB fetched for 1.6 GB of samples,
// 6.4 ms).  Here a workgroup owns PB consecutive pixels, whose PB x S values of one feature are ONE contiguous span: it is
// loaded coalesced into LDS (rows padded to S + 1 words: a thread walking its row meets no bank conflict), then thread t adds
// row t front to back -- the same additions in the same order (ops.h:121, 138), the same bits.
__global__ __launch_bounds__(256) void pixel_stats_tile_kernel(PassParams p, uint64_t pix0, uint64_t pix1, int PB) {
    extern __shared__ __align__(16) unsigned char smem_stats[];
    float *sT = reinterpret_cast<float *>(smem_stats);
    const uint64_t HW = (uint64_t)p.H * p.W;
    const int S = p.S, tid = threadIdx.x;
    const uint64_t base = pix0 + (uint64_t)blockIdx.x * (uint64_t)PB;
    if (base >= pix1) return;
    const int npx = (int)min((uint64_t)PB, pix1 - base);
    const int total = npx * S;
    const uint32_t magic_S = div_magic((uint32_t)S); // e * S < 2^32
    const double dn = (double)S;
    bool flat = false, any_nan = false;
    for (int k = 0; k < kNFeat; ++k) {
        const plane_t *src = reinterpret_cast<const plane_t *>(p.planes) + (uint64_t)(kColF + k) * p.plane_stride + base * (uint64_t)S;
        for (int e = tid; e < total; e += 256) {
            const uint32_t px = div_small((uint32_t)e, magic_S), s = (uint32_t)e - px * (uint32_t)S;
            sT[px * (uint32_t)(S + 1) + s] = (float)src[e];
        }
        __syncthreads();
        if (tid < npx) {
            const float *row = sT + tid * (S + 1);
            double sum = 0.0, sq = 0.0;
            for (int s = 0; s < S; ++s) {
                const double v = (double)row[s];
                sum = sum + v;     // ops.h:121
                sq = sq + v * v;   // ops.h:138 (v*v is exact for fp32-valued v)
            }
            const double mean = sum / dn;               // ops.h:123
            double sd = sqrt(sq / dn - mean * mean);    // ops.h:141
            if (p.policy == RPF_DEGEN_EPS && isnan(sd)) sd = 0.0;
            ((double *)p.pmean)[(uint64_t)k * HW + base + tid] = mean;
            ((double *)p.pstd)[(uint64_t)k * HW + base + tid] = sd;
            any_nan = any_nan || isnan(mean);
            flat = flat || (sd * 3.0 == 0.0 && isfinite(mean));
        }
        __syncthreads();
    }
    if (p.flat != nullptr && tid < npx) {
        p.flat[base + tid] = flat ? 1 : 0;
        if (any_nan) atomicOr(p.nan_flag, 1);
    }
}

#endif // RPF_IMPL_PART == 1 && !RPF_IMPL_SCHED && !RPF_IMPL_LISTED

template <int KD, int KW, int PACK5>
__device__ __forceinline__ void store_bins(uint32_t *sBinW, int c, int lane, const BinIds<KW, PACK5> &b) {
    if constexpr (PACK5 == 1) {
        sBinW[c * kWave + lane] = b.w[0];
        if (KD > 6) reinterpret_cast<uint8_t *>(sBinW + kNDim * kWave)[c * kWave + lane] = (uint8_t)b.b6;
    } else {
        store_words<KW>(sBinW + ((size_t)c * kWave + lane) * KW, b.w);
        if constexpr (PACK5 == 7) {
            if (KD > 12) reinterpret_cast<uint8_t *>(sBinW + kNDim * kWave * KW)[c * kWave + lane] = (uint8_t)b.b6;
        }
    }
}
template <int KD, int KW, int PACK5>
__device__ __forceinline__ void load_bins(const uint32_t *sBinW, int c, int lane, BinIds<KW, PACK5> &b) {
    if constexpr (PACK5 == 1) {
        b.w[0] = sBinW[c * kWave + lane];
        b.b6 = (KD > 6) ? (uint32_t) reinterpret_cast<const uint8_t *>(sBinW + kNDim * kWave)[c * kWave + lane] : 0u;
    } else {
        load_words<KW>(sBinW + ((size_t)c * kWave + lane) * KW, b.w);
        b.b6 = 0u;
        if constexpr (PACK5 == 7) {
            if (KD > 12) b.b6 = (uint32_t) reinterpret_cast<const uint8_t *>(sBinW + kNDim * kWave * KW)[c * kWave + lane];
        }
    }
}
// bin id of sample j = lane + 64*slot (debug hash only)
template <int KW, int PACK5>
__device__ __forceinline__ uint32_t bin_of_sample(const uint32_t *sBinW, int c, int j) {
    const int ln = j & 63, slot = j >> 6;
    if constexpr (PACK5 == 1) {
        if (slot < 6) return (sBinW[c * kWave + ln] >> (5 * slot)) & 31u;
        return reinterpret_cast<const uint8_t *>(sBinW + kNDim * kWave)[c * kWave + ln];
    } else if constexpr (PACK5 == 7) {
        if (slot < 12) return (sBinW[((size_t)c * kWave + ln) * KW + slot / 6] >> (5 * (slot % 6))) & 31u;
        return reinterpret_cast<const uint8_t *>(sBinW + kNDim * kWave * KW)[c * kWave + ln];
    } else {
        constexpr int BITS = PACK5 == 6 ? 6 : 5, SPW = 32 / BITS;
        return (sBinW[((size_t)c * kWave + ln) * KW + slot / SPW] >> (BITS * (slot % SPW))) & ((1u << BITS) - 1u);
    }
}

// ---- stage 3a: normalise, bin ids (sd.h:229-232, mi.cpp:14-16) -----------------------------------------
// bin ids are bytes packed per lane: sample kk of the lane is byte kk of KW words per column, written to LDS
// [column][lane][KW] over the (now dead) staging buffer of stage 2.  KD = sample slots handled (the occupied
// ones when the kernel is specialised on them, else K); holes compute on a dummy value and are masked.
// NW > 1 (several waves per pixel): the waves split the COLUMNS -- wave wv takes fp32 columns wv, wv+NW, ... of the
// 16 and colour column wv -- and each still covers all n samples, so no bin word is shared between waves.
// Per-column constants of stage 3a, formed ONCE per pixel by lane c for column c (they are wave-uniform: every lane
// forming all 19 sets was ~1000 redundant VALU instructions per pixel) and read back by broadcast:
//   ck[0] refined 1/SD   ck[1] lo = min z   ck[2] range = max z - min z   ck[3] refined 1/range
//   ck[4] flags: 1 SD == 0 | 2 empty z range | 4 both divisors inside the fast window
constexpr int kColConst = 5;
__device__ __forceinline__ void column_constants(const double *sStat, double *sCK, int c) {
    const double Mc = sStat[c], SDc = sStat[kNDim + c];
    const double xlo = sStat[2 * kNDim + c], xhi = sStat[3 * kNDim + c];
    const bool sd0 = (SDc == 0.0);
    const UDiv dsd = udiv_prepare(SDc);
    const double lo = sd0 ? 0.0 : udiv(xlo - Mc, dsd); // min_element over z (mi.cpp:47,49)
    const double hi = sd0 ? 0.0 : udiv(xhi - Mc, dsd); // max_element over z (mi.cpp:48,50)
    const double range = hi - lo;
    const bool flat = !(hi != lo);                       // mi.cpp:7 / 28 / 34
    const UDiv drg = udiv_prepare(range);
    const bool fast = dsd.fast && (flat || drg.fast);
    double *ck = sCK + c * kColConst;
    ck[0] = dsd.r; ck[1] = lo; ck[2] = range; ck[3] = drg.r;
    ck[4] = (double)((sd0 ? 1 : 0) | (flat ? 2 : 0) | (fast ? 4 : 0));
}

template <int KD, int KW, int PACK5, int NW = 1>
__device__ __forceinline__ void bins_stage(const PassParams &p, const Window &win, const double *sStat, const uint32_t *sOff, uint32_t *sBinW,
                                           int lane, int n, int B, const double *sCK, int wv = 0) {
    const double dB = (double)B;
    {
        uint32_t offk[KD];
#pragma unroll
        for (int kk = 0; kk < KD; ++kk) offk[kk] = (lane + kWave * kk < n) ? sOff[lane + kWave * kk] << kPlaneShift : 0u; // in bytes of a feature plane
        // one column: z, t, bin for the lane's K samples, packed into KW words
        auto do_column = [&](int c, const double (&xv)[KD]) {
            const double Mc = sStat[c], SDc = sStat[kNDim + c];
            const double *ck = sCK + c * kColConst;             // column_constants(): wave-uniform broadcast reads
            const double lo = ck[1], range = ck[2];
            const int flags = (int)ck[4];
            const bool sd0 = flags & 1, flat = flags & 2, fast = flags & 4;
            UDiv dsd, drg;
            dsd.b = SDc; dsd.r = ck[0]; dsd.fast = true;
            drg.b = range; drg.r = ck[3]; drg.fast = true;
            BinIds<KW, PACK5> w;
            w.clear();
            if (sd0 || flat) {
                // SD == 0 normalises every sample to z == 0 (ops.h:48), and a column whose z range is empty bins every
                // sample to 0 (mi.cpp:7): the cleared words are the answer -- no per-sample work (constant normals /
                // positions inside a cluster make this the common case on path-traced buffers)
            } else if (fast) {
                // the common case, straight-line for all K samples of the lane (holes compute on a dummy value
                // and are masked at the pack), so the K dependent chains interleave
#pragma unroll
                for (int kk = 0; kk < KD; ++kk) {
                    const double a = xv[kk] - Mc;                          // subtractArrays
                    const double z = udiv_fast(a, dsd);                    // divideArrays, ops.h:48
                    const double t = udiv_fast(z - lo, drg) * dB;          // mi.cpp:14
                    int bin = (int)t;
                    bin = min(bin, B - 1);
                    bin = max(bin, 0);
                    bin = (lane + kWave * kk < n) ? bin : 0;
                    w.set(kk, (uint32_t)bin);
                }
            } else {
#pragma unroll
                for (int kk = 0; kk < KD; ++kk) {
                    if (lane + kWave * kk < n) {
                        const double a = xv[kk] - Mc;
                        const double z = sd0 ? 0.0 : a / SDc;
                        int bin = 0;
                        if (!flat) {
                            const double t = (z - lo) / range * dB;
                            bin = (int)t;
                            bin = min(bin, B - 1);
                            bin = max(bin, 0);
                        }
                        w.set(kk, (uint32_t)bin);
                    }
                }
            }
            store_bins<KD, KW, PACK5>(sBinW, c, lane, w);
        };
        if constexpr (NW > 1) {
            if (p.stage_mask & 2) {
                auto colidx = [](int i) { return xcol(i); };
                float xb[KD];
                auto issue3 = [&](int i) {
                    gchar *fplane = win.plane(colidx(i));
#pragma unroll
                    for (int kk = 0; kk < KD; ++kk) {
                        asm volatile("" : "+v"(offk[kk])); // (see the one-wave form below)
                        xb[kk] = ldw_b(fplane, offk[kk]);
                    }
                };
                issue3(wv); // NW <= kNX
#pragma unroll 1
                for (int i = wv; i < kNX; i += NW) {
                    double xv[KD];
#pragma unroll
                    for (int kk = 0; kk < KD; ++kk) xv[kk] = (double)xb[kk];
                    if (i + NW < kNX) issue3(i + NW);
                    do_column(colidx(i), xv);
                }
#pragma unroll 1
                for (int c = wv; c < 3; c += NW) {
                    double xc[KD];
                    gchar *dplane = win.colour(c);
#pragma unroll
                    for (int kk = 0; kk < KD; ++kk) xc[kk] = ldwc_b(dplane, offk[kk]);
                    do_column(kColC + c, xc);
                }
            }
        } else if (p.stage_mask & 2) {
            // the kNX plane columns (all but the colours) through kPF3 rotating register buffers, gathers kPF3 columns ahead
            constexpr int kPF3 = KD <= 8 ? 4 : (KD <= 13 ? 2 : 1); // register budget: KD floats per buffer
            static_assert(kNX % 4 == 0, "the column loop below walks whole groups of kPF3");
            float xb[kPF3][KD];
            auto colidx = [](int i) { return xcol(i); };
            auto issue3 = [&](int i, float (&dst)[KD]) {
                gchar *fplane = win.plane(colidx(i));
#pragma unroll
                for (int kk = 0; kk < KD; ++kk) {
                    // the offsets are loop invariants: left visible, their 64-bit extensions are hoisted out of the column loop
                    // and every load gets a per-lane v_lshl_add_u64 again (the scalar-base form is matched per basic block)
                    asm volatile("" : "+v"(offk[kk]));
                    dst[kk] = ldw_b(fplane, offk[kk]);
                }
            };
#pragma unroll
            for (int u = 0; u < kPF3; ++u) issue3(u, xb[u]);
#pragma unroll 1
            for (int i0 = 0; i0 < kNX; i0 += kPF3) {
#pragma unroll
                for (int u = 0; u < kPF3; ++u) {
                    double xv[KD];
#pragma unroll
                    for (int kk = 0; kk < KD; ++kk) xv[kk] = (double)xb[u][kk];
                    if (i0 + u + kPF3 < kNX) issue3(i0 + u + kPF3, xb[u]);
                    do_column(colidx(i0 + u), xv);
                }
            }
            // the 3 fp64 colour columns
            double xc[3][KD];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                gchar *dplane = win.colour(c);
#pragma unroll
                for (int kk = 0; kk < KD; ++kk) xc[c][kk] = ldwc_b(dplane, offk[kk]);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) do_column(kColC + c, xc[c]);
        }
    }
}

// ---- marginal counts off a resident joint histogram ------------------------------------------------------------
// sum_i T[hx_i] of a column is needed once per column (19 of them).  Building 19 more histograms for that is the most
// expensive way to get it (a marginal has only B cells: 64 lanes pile onto a handful of addresses).  Instead the
// counts are read off a joint histogram that is resident anyway, between its atomics and its clearing store (one
// wave's LDS operations execute in order): hy_j = sum_i J[i][j] (column sums: the partner's marginal), hx_i = sum_j
// J[i][j] (row sums: the anchor's).  Counts are integers: same totals, bit for bit.  B <= 32: lane = (h, j), h = lane
// >> 5 takes every other row / column, the two halves meet in one v_permlane32_swap; NIT = compile-time trip count
// (>= ceil(B/2)).
template <int NIT, bool ROWS>
__device__ __forceinline__ uint32_t marginal_counts(const uint32_t *sHist, int lane, int B) {
    uint32_t tot = 0u;
    const int j = lane & 31, h = lane >> 5;
    uint32_t v[NIT];
    if constexpr (!ROWS) {
        // column sums: rows i = h, h + 2, ... of column j.  No masks: a row index past B lands in the cleared cells
        // behind the live histogram (the clearing stores of every ZN class cover 2 * NIT * B cells, and nothing
        // increments them), lanes j >= B read a neighbouring row and are dropped below.
        const uint32_t *col = sHist + h * B + j;
#pragma unroll
        for (int t = 0; t < NIT; ++t) v[t] = col[2 * t * B];
#pragma unroll
        for (int t = 0; t < NIT; ++t) tot += v[t];
    } else {
        const int jj = min(j, B - 1);
#pragma unroll
        for (int t = 0; t < NIT; ++t) v[t] = sHist[jj * B + min(2 * t + h, B - 1)];
#pragma unroll
        for (int t = 0; t < NIT; ++t) tot += (2 * t + h < B) ? v[t] : 0u;
    }
    tot = xl::exch32<xl::OpSum>(tot, tot);          // both halves now hold the full count of bin j
    return (j < B && h == 0) ? tot : 0u;            // one lane per bin contributes T[count] (T[0] == 0)
}

// D[c] through a 32-bit byte offset from the (wave-uniform) table base: scalar base + vector offset addressing
__device__ __forceinline__ uint64_t dlook(const uint64_t *dtab, uint32_t c) {
    return *reinterpret_cast<const uint64_t *>(reinterpret_cast<const char *>(dtab) + (c << 3));
}

// ... and with the count already scaled by 8 (mi_pgroup's cells count in units of 8: a returned count IS the byte offset)
__device__ __forceinline__ uint64_t dlook8(const uint64_t *tab, uint32_t c8) {
    return *reinterpret_cast<const uint64_t *>(reinterpret_cast<const char *>(tab) + c8);
}
// ... from the table head at LDS address 0 (the start of the workgroup's dynamic LDS: these kernels have no static LDS, and the
// kernel traps if that ever changes): the count is the address, `ds_read_b64 v, v_count`.  (Through the `smem` symbol hipcc
// resolves the base too late to fold it and emits `v_add_u32 v, 0, v_count` per look-up.)
__device__ __forceinline__ uint64_t dlook8_lds0(uint32_t c8) {
    typedef __attribute__((address_space(3))) const uint64_t lds_u64;
    return *(lds_u64 *)(uintptr_t)c8;
}

// Could a joint histogram hold a count >= kDHead?  Only if BOTH its columns have a marginal bin that large (counts x 8).  The
// pairs are (r | p anchor, feature or colour partner) and (colour anchor, feature partner): rpf.cpp:416-442.  mxF / mxC / mxRP:
// per-lane maxima over the marginal bins of the feature, colour and r / p columns.  Wave-uniform verdict.
__device__ __forceinline__ bool head_overrun(uint32_t mxF, uint32_t mxC, uint32_t mxRP) {
    const uint32_t T8 = (uint32_t)kDHead * 8u;
    const bool f = __any(mxF >= T8), c = __any(mxC >= T8), rp = __any(mxRP >= T8);
    return (rp && (f || c)) || (c && f);
}

// ---- one-wave kernels (K <= 8, 3 <= KD): PARTNER-major histogram groups ---------------------------------------
// All joint histograms of ONE partner column, one per anchor: the partner's bin ids are unpacked once for the
// whole group and every anchor's (bin * B * 4 + histogram base) sits in registers (akey4[anchor][slot], formed once per
// pixel), so the address of an increment is a single v_lshl_add.  NA = anchors of the group (7 for a feature partner:
// r0 r1 p0 p1 c0 c1 c2; 4 for a colour partner: r0 r1 p0 p1).  Slots kk < KD-1 are full by definition of KD
// (= ceil(n/64)), so only the last slot carries the hole mask: `last_ok` lanes exist, the others aim a +0 atomic at `hole`.
// Histogram u+1's atomics are queued before the D look-ups of histogram u are consumed; the clearing store sits right
// behind the atomics.  MARG bit 0: the partner's marginal from the column sums of histogram 0 -> macc; bit 1: the
// anchors' marginals from the row sums of every histogram of the group -> racc[u].
// D look-ups: the first kDHead entries of the table sit in LDS (1 KiB: costs no resident workgroup), which is where
// nearly every look-up lands (a cell that holds >= kDHead of a neighbourhood's <= 512 samples is a degenerate pixel); the
// 480 look-ups per pixel were the kernel's main load on the texture-address path.  A wave in which some count reaches
// kDHead repeats the pixel's MI stage with the full table in global memory (one wave-uniform branch per pixel, outside the
// straight-line histogram code: a branch per histogram cost 146 spilled registers).
template <int KD, int KW, int ZN, int NA, int NAMAX, int PACK5, int MARG, bool DHEAD>
__device__ __forceinline__ void mi_pgroup(const uint32_t *sBinW, uint32_t *sHist, const uint64_t *dtab, const uint64_t *sDh, const uint64_t *ttab,
                                          int lane, int B, int pcol, const uint32_t (&akey4)[NAMAX][KD], bool last_ok,
                                          uint32_t hole4, int cells, uint64_t (&acc)[8], uint64_t &macc, uint64_t (&racc)[4],
                                          uint32_t &mx, uint32_t &mxa) {
    constexpr int NIT = ZN == 1 ? 8 : (ZN == 3 ? 9 : (ZN == 4 ? 10 : 11)); // B <= 16 / 17 / 19 / 22
    static_assert(NA <= 8 && (!(MARG & 2) || NA <= 4), "slot budget of the reductions");
    uint32_t bin4[KD];
    {
        BinIds<KW, PACK5> w;
        load_bins<KD, KW, PACK5>(sBinW, pcol, lane, w);
#pragma unroll
        for (int kk = 0; kk < KD; ++kk) bin4[kk] = w.get(kk) << 2;
    }
    char *hbase = reinterpret_cast<char *>(sHist);
    uint32_t old[2][KD];
    uint32_t mcnt = 0u, rcnt[2] = {0u, 0u};
    // The cells count in units of 8: the count an atomic returns is the byte offset of its table entry (with the table head at
    // LDS address 0 -- sDh -- the look-up's address needs no instruction at all), and a marginal total read off the cells is
    // the byte offset of T[total].
    const uint32_t last_inc = last_ok ? 8u : 0u;
#pragma unroll
    for (int u = 0; u <= NA; ++u) {
        if (u < NA) {
#pragma unroll
            for (int kk = 0; kk < KD; ++kk) {
                uint32_t off = akey4[u][kk] + bin4[kk];                                  // mi.cpp:39 (x 4 bytes)
                if (kk == KD - 1) off = last_ok ? off : hole4;
                old[u & 1][kk] = atomicAdd(reinterpret_cast<uint32_t *>(hbase + off), kk == KD - 1 ? last_inc : 8u);
            }
            if constexpr (MARG != 0) {
                if ((MARG & 2) || u == 0) {
                    wsync(); // the counts other lanes' atomics left are read below (in-order LDS: program order only)
                    if constexpr (MARG & 1) if (u == 0) mcnt = marginal_counts<NIT, false>(sHist, lane, B);
                    if constexpr ((MARG & 2) != 0) {
                        rcnt[u & 1] = marginal_counts<NIT, true>(sHist, lane, B);
                        if constexpr (DHEAD) mxa = max(mxa, rcnt[u & 1]);
                    }
                    wsync();
                }
            }
            zero_cells<ZN>(sHist, cells, lane);
        }
        if (u >= 1) {
            uint64_t d[KD];
#pragma unroll
            for (int kk = 0; kk < KD; ++kk) d[kk] = DHEAD ? dlook8_lds0(old[(u - 1) & 1][kk]) : dlook8(dtab, old[(u - 1) & 1][kk]);
            uint64_t a = last_ok ? d[KD - 1] : 0ull;
#pragma unroll
            for (int kk = 0; kk < KD - 1; ++kk) a += d[kk];
            acc[u - 1] = a;
            if constexpr ((MARG & 2) != 0) racc[u - 1] = dlook8(ttab, rcnt[(u - 1) & 1]);
        }
    }
    static_assert((MARG & 1) != 0, "every group reads its partner's marginal (it also bounds the group's cell counts)");
    macc = dlook8(ttab, mcnt);
    // DHEAD: a cell of a joint histogram holds no more than its row total and no more than its column total, i.e. than the
    // largest bin of the anchor's and of the partner's marginal.  The largest bins are collected per column class (mx: this
    // group's partner; mxa: the r / p anchors, whose marginals the c0 group reads) -- one max per GROUP instead of one per
    // look-up (240 instructions per pixel) -- and head_overrun() decides from them whether some pair of columns could hold a
    // count at or past the head: the caller then repeats the stage with the full table (a superset of the pixels that need it).
    if constexpr (DHEAD) mx = max(mx, mcnt);
#pragma unroll
    for (int u = NA; u < 8; ++u) acc[u] = 0ull;
}

// The partner-major MI stage.  Anchor a: 0..1 = r0, r1; 2..3 = p0, p1; 4..6 = c0..c2.  Pair index = position in
// ComputeCFWeights' call order (rpf.cpp:416-442).  Marginal sums sHXf: every partner's from its own group (f0..f11,
// c0..c2 are all partners), r0 r1 p0 p1 from the row sums of the c0 group's four histograms.
template <int KD, int KW, int ZN, int PACK5, bool DHEAD>
__device__ __forceinline__ uint32_t mi_stage_pm(const uint32_t *sBinW, uint32_t *sHist, const uint64_t *dtab, const uint64_t *sDh, const uint64_t *ttab,
                                            uint64_t *sHXf, uint64_t *sPairF, int lane, int n, int B) {
    constexpr int NA = 7;
    const int ncell2 = B * B;
    const bool last_ok = (lane + kWave * (KD - 1)) < n;                 // does this lane's last sample slot exist?
    // (mi_group V2's always-zero hole cells -- no mask on the last slot's look-up, 192 selects per pixel -- were tried here too:
    // they need 64 spare cleared cells, which moves B = 18, 19 into the 512-cell clearing class: 1080p x 8 60.9 -> 62.0 ms.)
    const uint32_t hole4 = (uint32_t)min(lane, ncell2 - 1) << 2;        // harmless, spread-out targets of the +0 atomics
    zero_cells<ZN>(sHist, ncell2, lane);
    uint32_t mxF = 0u, mxC = 0u, mxRP = 0u; // DHEAD: largest marginal bins (x 8) per column class, see head_overrun()
    uint32_t akey4[NA][KD];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const int acol = a < 2 ? kColR + a : (a < 4 ? kColP + (a - 2) : kColC + (a - 4));
        BinIds<KW, PACK5> w;
        load_bins<KD, KW, PACK5>(sBinW, acol, lane, w);
#pragma unroll
        for (int kk = 0; kk < KD; ++kk) akey4[a][kk] = w.get(kk) * (uint32_t)(B * 4);
    }
    auto pair_index = [&](int a, int i) { // anchor a, partner i (0..11 features, 12..14 colours)
        return a < 4 ? (i < 12 ? i * 4 + a : 48 + (i - 12) * 16 + a) : 48 + (a - 4) * 16 + 4 + i;
    };
#pragma unroll 1
    for (int i = 0; i < kNFeat; ++i) { // feature partners: 7 histograms each
        uint64_t acc[8], macc = 0ull, racc[4];
        mi_pgroup<KD, KW, ZN, 7, NA, PACK5, 1, DHEAD>(sBinW, sHist, dtab, sDh, ttab, lane, B, kColF + i, akey4, last_ok, hole4, ncell2, acc, macc, racc, mxF, mxRP);
        acc[7] = macc; // the free eighth slot carries the partner's marginal
        const uint64_t tot = xl::reduce8<xl::OpSum>(acc, lane);
        if ((lane & 7) == 0) {
            const int sl = xl::slot8(lane);
            if (sl < 7) sPairF[pair_index(sl, i)] = tot;
            else sHXf[kColF + i] = tot;
        }
    }
#pragma unroll 1
    for (int c = 0; c < 3; ++c) { // colour partners: 4 histograms each (anchors r0 r1 p0 p1)
        uint64_t acc[8], macc = 0ull, racc[4] = {0ull, 0ull, 0ull, 0ull};
        if (c == 0) mi_pgroup<KD, KW, ZN, 4, NA, PACK5, 3, DHEAD>(sBinW, sHist, dtab, sDh, ttab, lane, B, kColC, akey4, last_ok, hole4, ncell2, acc, macc, racc, mxC, mxRP);
        else mi_pgroup<KD, KW, ZN, 4, NA, PACK5, 1, DHEAD>(sBinW, sHist, dtab, sDh, ttab, lane, B, kColC + c, akey4, last_ok, hole4, ncell2, acc, macc, racc, mxC, mxRP);
        acc[7] = macc;
        if (c == 0) { acc[4] = racc[0]; acc[5] = racc[1]; acc[6] = racc[2]; }
        const uint64_t tot = xl::reduce8<xl::OpSum>(acc, lane);
        const uint64_t r3 = (c == 0) ? xl::allreduce<xl::OpSum>(racc[3]) : 0ull; // wave-uniform branch
        if ((lane & 7) == 0) {
            const int sl = xl::slot8(lane);
            if (sl < 4) sPairF[pair_index(sl, 12 + c)] = tot;
            else if (sl == 7) sHXf[kColC + c] = tot;
            else if (c == 0) sHXf[sl == 4 ? kColR : (sl == 5 ? kColR + 1 : kColP)] = tot;
        }
        if (c == 0 && lane == 0) sHXf[kColP + 1] = r3;
    }
    return (DHEAD && head_overrun(mxF, mxC, mxRP)) ? 1u : 0u;
}

template <int KD, int KW, int ZN, int PACK5, bool DHEAD>
__device__ __forceinline__ void mi_pm(const uint32_t *sBinW, uint32_t *sHist, const uint64_t *dtab, const uint64_t *sDh,
                                      const uint64_t *ttab, uint64_t *sHXf, uint64_t *sPairF, int lane, int n, int B) {
    const uint32_t over = mi_stage_pm<KD, KW, ZN, PACK5, DHEAD>(sBinW, sHist, dtab, sDh, ttab, sHXf, sPairF, lane, n, B);
    if constexpr (DHEAD) {
        if (over != 0u) { // (wave-uniform) some pair of columns could hold a count past the LDS head of the table: once more, full table
            wsync();
            mi_stage_pm<KD, KW, ZN, PACK5, false>(sBinW, sHist, dtab, sDh, ttab, sHXf, sPairF, lane, n, B);
        }
    }
}

// ---- large-neighbourhood kernels (K >= 13): ANCHOR-major groups of G (3 or 4) histograms ----------------------------
// For marginals (JOINT = false) histogram u bins column cols[u]; for joints it bins (anchor, partner cols[u]).  Every
// slot carries its own mask (lane + 64*kk < n): masked lanes aim a +0 atomic at `hole`.
// sum_i T[h_i] of one column, read off a resident B x B joint histogram (cell = anchor bin * B + partner bin) between its
// atomics and its clearing store: lanes j < B total column j (the partner's marginal) or row j (the anchor's), look T up and
// the wave adds the B values.  B plain, conflict-free reads per lane against a 19-histogram marginal pass whose 64 lanes pile
// onto B cells (a fifth of the 32-spp bins + MI kernel: 122.2 -> 97.4 ms with the marginal histograms switched off).  Counts
// are integers: the same totals bit for bit.  Branch-free (lanes >= B walk a clamped index and contribute 0).
// (hipcc's loop vectoriser turns the loop below into four reads per trip with a v_mul_lo_u32 each; a hand-batched form -- eight
// clamped reads behind one wait, no multiplies -- was measured slower: 16 spp 170.0 -> 175.9 ms, 32 spp 227.6 -> 228.6.)
template <bool ROWS>
__device__ __forceinline__ uint32_t marginal_count(const uint32_t *sHist, int lane, int B) {
    const int jj = min(lane, B - 1);
    const uint32_t *pp = ROWS ? sHist + jj * B : sHist + jj;
    const int stride = ROWS ? 1 : B;
    uint32_t tot = 0u;
#pragma unroll 2
    for (int i = 0; i < B; ++i) tot += pp[i * stride];
    return lane < B ? tot : 0u; // T[0] == 0
}

// marg (wave-uniform): bit 0 -- every histogram of the group also yields its partner column's marginal sum -> sHXf[cols[u]];
// bit 1 -- histogram 0 also yields the anchor's -> sHXf[acol]
// NFULL: the first NFULL sample slots of every lane are occupied (the caller checked n > 64 * NFULL): no mask on them
// TSRC: 0 -- dtab is the table in global memory; 1 -- the table sits at LDS address 0 (T_IN_LDS; dlook8_lds0)
// Round 3, second session -- fewer instructions per increment (5-8 -> 3-4 VALU): (a) akey is the LDS ADDRESS of the anchor's
// row, so an increment's address is bit-field extract + add; (b) the cells count in units of 8, so the count an atomic returns
// IS the byte offset of its table entry -- with the table at LDS address 0 the look-up needs no address arithmetic at all;
// (c) a lane without a sample in a slot aims its +0 atomic at a cell of its own BEHIND the histogram (`hole` = the LDS address of
// cell B*B + lane: inside the cleared region, never incremented): it returns 0, D[0] == 0, and the look-ups need no mask.
// (For most of that session this form gave wrong pair sums in the one-wave K = 25 / 49 instantiations and run-to-run
// differences with a table head at K = 13, while the four-wave kernels were fine.  The cause was not here: lds_store_u64_if's
// s_and_saveexec writes SCC and its asm statement did not say so -- hipcc carried a compare across the store in those
// instantiations.  See rpf_device_common.h.)
template <int KD, int KW, int G, int PACK5, bool JOINT, int NFULL = 0, int TSRC = 0>
__device__ __forceinline__ void mi_group(const uint32_t *sBinW, uint32_t *sHist, const uint64_t *dtab, int lane, int n,
                                         const int (&cols)[4], const uint32_t (&akey)[KD], uint32_t hole, int cells,
                                         uint64_t (&acc4)[4], int marg = 0, const uint64_t *ttab = nullptr, uint64_t *sHXf = nullptr,
                                         int acol = 0, int B = 0) {
    static_assert(JOINT, "the marginal sums are read off the joints (marginal_count)");
    uint32_t old[2][KD];
    // (Deferring the table look-ups of the marginal sums to the end of the group -- T values, counts in registers, counts
    // parked in LDS -- was tried three ways: each raised the K = 25 kernel's spilled registers from 16 to 51-60 and put spill
    // code in front of an EXEC restore in a K = 49 instantiation (scripts/check_spills.py refused the builds).)
    auto slot_ok = [&](int kk) -> bool { return kk < NFULL || lane + kWave * kk < n; };
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    // program order against the previous group's clearing stores: the atomics go through integer-derived LDS pointers, the
    // clearing stores through `sHist`
    wsync();
#pragma unroll
    for (int u = 0; u <= G; ++u) {
        if (u < G) {
            BinIds<KW, PACK5> w;
            load_bins<KD, KW, PACK5>(sBinW, cols[u], lane, w);
#pragma unroll
            for (int kk = 0; kk < KD; ++kk) {
                const bool ok = slot_ok(kk);
                const uint32_t addr = (w.get(kk) << 2) + akey[kk];           // mi.cpp:39 (x 4 bytes; akey and hole are LDS addresses)
                old[u & 1][kk] = __hip_atomic_fetch_add((lds_u32 *)(uintptr_t)(ok ? addr : hole), ok ? 8u : 0u, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            if (marg != 0) { // wave-uniform (scalar branch: EXEC untouched)
                wsync(); // the counts every lane's atomics left are read below (in-order LDS: program order only)
                if (marg & 1) {
                    const uint64_t s = xl::allreduce<xl::OpSum>(dlook8(ttab, marginal_count<false>(sHist, lane, B))); // (8 x count)
                    lds_store_u64_if(lane == 0, &sHXf[cols[u]], s);
                }
                if ((marg & 2) && u == 0) {
                    const uint64_t s = xl::allreduce<xl::OpSum>(dlook8(ttab, marginal_count<true>(sHist, lane, B)));
                    lds_store_u64_if(lane == 0, &sHXf[acol], s);
                }
                wsync();
            }
            zero_cells<0>(sHist, cells, lane);
        }
        if (u >= 1) {
            uint64_t d[KD];
#pragma unroll
            for (int kk = 0; kk < KD; ++kk) d[kk] = TSRC == 1 ? dlook8_lds0(old[(u - 1) & 1][kk]) : dlook8(dtab, old[(u - 1) & 1][kk]);
            uint64_t a = d[KD - 1]; // (a lane without a sample in a slot looked up D[0] == 0)
#pragma unroll
            for (int kk = 0; kk < KD - 1; ++kk) a += d[kk];
            acc4[u - 1] = a;
        }
    }
#pragma unroll
    for (int u = G; u < 4; ++u) acc4[u] = 0ull;
}

// Small neighbourhoods (KD <= 2 sample slots, i.e. N <= 128: the regime of real path-traced buffers, where most
// pixels keep only their own S samples): a histogram costs a handful of LDS cycles, so the stage is latency bound.
// This variant queues the atomics of up to 16 histograms back to back (one wave's LDS operations execute in
// order, the clearing store sits between two histograms), then issues all D look-ups, then reduces the 16 sums
// with one 16-slot butterfly: two round trips per 16 histograms instead of per 4.
template <int KD, int KW, int ZN, int G, bool JOINT, int PACK5>
__device__ __forceinline__ void mi_group_deep(const uint32_t *sBinW, uint32_t *sHist, const uint64_t *dtab, int lane,
                                              const int (&cols)[16], const uint32_t (&akey)[KD], bool last_ok,
                                              uint32_t hole, int cells, uint64_t (&acc)[16]) {
    uint32_t old[G][KD];
    const uint32_t one = 1u, last_inc = last_ok ? 1u : 0u;
#pragma unroll
    for (int u = 0; u < G; ++u) {
        BinIds<KW, PACK5> w;
        load_bins<KD, KW, PACK5>(sBinW, cols[u], lane, w);
#pragma unroll
        for (int kk = 0; kk < KD; ++kk) {
            uint32_t key = w.get(kk);
            if (JOINT) key += akey[kk];                                      // mi.cpp:39
            if (kk == KD - 1) key = last_ok ? key : hole;
            old[u][kk] = atomicAdd(&sHist[key], kk == KD - 1 ? last_inc : one);
        }
        zero_cells<(JOINT ? ZN : (ZN > 0 ? 1 : 0))>(sHist, cells, lane);
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        uint64_t a = 0ull;
        if (u < G) {
            uint64_t d[KD];
#pragma unroll
            for (int kk = 0; kk < KD; ++kk) d[kk] = dtab[old[u][kk]];
            a = last_ok ? d[KD - 1] : 0ull;
#pragma unroll
            for (int kk = 0; kk < KD - 1; ++kk) a += d[kk];
        }
        acc[u] = a;
    }
}

template <int KD, int KW, int ZN, int PACK5>
__device__ __forceinline__ void mi_stage_deep(const uint32_t *sBinW, uint32_t *sHist, const uint64_t *dtab, uint64_t *sHXf,
                                              uint64_t *sPairF, int lane, int n, int B) {
    const int ncell2 = B * B;
    const bool last_ok = (lane + kWave * (KD - 1)) < n;
    const uint32_t hole1 = (uint32_t)min(lane, B - 1);
    const uint32_t hole2 = (uint32_t)min(lane, ncell2 - 1);
    zero_cells<ZN>(sHist, ncell2, lane);
    uint32_t akey[KD];
#pragma unroll
    for (int kk = 0; kk < KD; ++kk) akey[kk] = 0u;
    uint64_t acc[16];
    { // marginals: columns 0..15, then 16..18
        const int cols[16] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
        mi_group_deep<KD, KW, ZN, 16, false, PACK5>(sBinW, sHist, dtab, lane, cols, akey, last_ok, hole1, B, acc);
        const uint64_t tot = xl::reduce16<xl::OpSum>(acc, lane);
        if ((lane & 3) == 0) sHXf[xl::slot16(lane)] = tot;
    }
    {
        const int cols[16] = {16, 17, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18};
        mi_group_deep<KD, KW, ZN, 3, false, PACK5>(sBinW, sHist, dtab, lane, cols, akey, last_ok, hole1, B, acc);
        const uint64_t tot = xl::reduce16<xl::OpSum>(acc, lane);
        if ((lane & 3) == 0 && xl::slot16(lane) < 3) sHXf[16 + xl::slot16(lane)] = tot;
    }
#pragma unroll 1
    for (int g = 0; g < 7; ++g) {
        const int acol = g < 2 ? kColR + g : (g < 4 ? kColP + (g - 2) : kColC + (g - 4));
        const int l = g < 2 ? g : 2 + (g - 2);
        {
            BinIds<KW, PACK5> w;
            load_bins<KD, KW, PACK5>(sBinW, acol, lane, w);
#pragma unroll
            for (int kk = 0; kk < KD; ++kk) akey[kk] = w.get(kk) * (uint32_t)B;
        }
        auto pair_index = [&](int i) { return g < 4 ? (i < 12 ? i * 4 + l : 48 + (i - 12) * 16 + l) : 48 + (g - 4) * 16 + 4 + i; };
        // partners f0..f11 then (anchors r,p only) c0..c2; the c-anchors repeat a column for the unused slots
        const int cols[16] = {kColF, kColF + 1, kColF + 2, kColF + 3, kColF + 4, kColF + 5, kColF + 6, kColF + 7,
                              kColF + 8, kColF + 9, kColF + 10, kColF + 11, kColC, kColC + 1, kColC + 2, kColC + 2};
        const int np = g < 4 ? 15 : 12;
        if (g < 4) mi_group_deep<KD, KW, ZN, 15, true, PACK5>(sBinW, sHist, dtab, lane, cols, akey, last_ok, hole2, ncell2, acc);
        else mi_group_deep<KD, KW, ZN, 12, true, PACK5>(sBinW, sHist, dtab, lane, cols, akey, last_ok, hole2, ncell2, acc);
        const uint64_t tot = xl::reduce16<xl::OpSum>(acc, lane);
        const int i = xl::slot16(lane);
        if ((lane & 3) == 0 && i < np) sPairF[pair_index(i)] = tot;
    }
}

// Tiny neighbourhoods (one sample slot: N <= 64, B <= 8, at most 64 cells) -- what real path-traced buffers mostly
// are (N = S for >90 % of pixels, SURVEY F10).  Returning atomics would serialise here: a dozen lanes hit the same
// few cells.  Instead each 16-lane row increments its own replica of the histogram with a plain (non-returning)
// atomic, lane c then reads the four replica counts of cell c with one 16-byte read, looks up T[count] and clears
// the cell with one 16-byte store; two 256-word regions ping-pong so the atomics of histogram u+1 are queued before
// histogram u is read.  Sixteen histograms share one 16-slot butterfly.  Layout of a region: [cell][replica].
template <int G, bool JOINT, int KW, int PACK5>
__device__ __forceinline__ void mi_group_tiny(const uint32_t *sBinW, uint32_t *sHist, const uint64_t *ttab, int lane,
                                              const int (&cols)[16], uint32_t akey, bool ok, uint64_t (&acc)[16]) {
    const uint32_t rep = (uint32_t)lane >> 4;
#pragma unroll
    for (int u = 0; u <= G; ++u) {
        if (u < G) {
            BinIds<KW, PACK5> w;
            load_bins<1, KW, PACK5>(sBinW, cols[u], lane, w);
            uint32_t key = w.get(0);
            if (JOINT) key += akey;                                          // mi.cpp:39
            if (ok) atomicAdd(&sHist[(u & 1) * 256 + key * 4 + rep], 1u);
        }
        if (u >= 1) {
            uint32_t *cell = sHist + ((u - 1) & 1) * 256 + lane * 4;         // lane = cell id (64 cells per region)
            const uint4 c4 = *reinterpret_cast<const uint4 *>(cell);
            *reinterpret_cast<uint4 *>(cell) = make_uint4(0u, 0u, 0u, 0u);
            acc[u - 1] = ttab[c4.x + c4.y + c4.z + c4.w];                    // T[J] of this lane's cell (T[0] = 0)
        }
    }
#pragma unroll
    for (int u = G; u < 16; ++u) acc[u] = 0ull;
}

template <int KW, int PACK5>
__device__ __forceinline__ void mi_stage_tiny(const uint32_t *sBinW, uint32_t *sHist, const uint64_t *ttab, uint64_t *sHXf,
                                              uint64_t *sPairF, int lane, int n, int B) {
    const bool ok = lane < n;
    *reinterpret_cast<uint4 *>(sHist + lane * 4) = make_uint4(0u, 0u, 0u, 0u);
    *reinterpret_cast<uint4 *>(sHist + 256 + lane * 4) = make_uint4(0u, 0u, 0u, 0u);
    uint64_t acc[16];
    {
        const int cols[16] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
        mi_group_tiny<16, false, KW, PACK5>(sBinW, sHist, ttab, lane, cols, 0u, ok, acc);
        const uint64_t tot = xl::reduce16<xl::OpSum>(acc, lane);
        if ((lane & 3) == 0) sHXf[xl::slot16(lane)] = tot;
    }
    {
        const int cols[16] = {16, 17, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18, 18};
        mi_group_tiny<3, false, KW, PACK5>(sBinW, sHist, ttab, lane, cols, 0u, ok, acc);
        const uint64_t tot = xl::reduce16<xl::OpSum>(acc, lane);
        if ((lane & 3) == 0 && xl::slot16(lane) < 3) sHXf[16 + xl::slot16(lane)] = tot;
    }
#pragma unroll 1
    for (int g = 0; g < 7; ++g) {
        const int acol = g < 2 ? kColR + g : (g < 4 ? kColP + (g - 2) : kColC + (g - 4));
        const int l = g < 2 ? g : 2 + (g - 2);
        uint32_t akey;
        {
            BinIds<KW, PACK5> w;
            load_bins<1, KW, PACK5>(sBinW, acol, lane, w);
            akey = w.get(0) * (uint32_t)B;
        }
        auto pair_index = [&](int i) { return g < 4 ? (i < 12 ? i * 4 + l : 48 + (i - 12) * 16 + l) : 48 + (g - 4) * 16 + 4 + i; };
        const int cols[16] = {kColF, kColF + 1, kColF + 2, kColF + 3, kColF + 4, kColF + 5, kColF + 6, kColF + 7,
                              kColF + 8, kColF + 9, kColF + 10, kColF + 11, kColC, kColC + 1, kColC + 2, kColC + 2};
        const int np = g < 4 ? 15 : 12;
        if (g < 4) mi_group_tiny<15, true, KW, PACK5>(sBinW, sHist, ttab, lane, cols, akey, ok, acc);
        else mi_group_tiny<12, true, KW, PACK5>(sBinW, sHist, ttab, lane, cols, akey, ok, acc);
        const uint64_t tot = xl::reduce16<xl::OpSum>(acc, lane);
        const int i = xl::slot16(lane);
        if ((lane & 3) == 0 && i < np) sPairF[pair_index(i)] = tot;
    }
}

// Large neighbourhoods (K >= 13), and every K of a non-reference layout.  NW > 1: the histogram groups (marginal groups,
// then the joint groups anchor by anchor: 5 + 25 in the reference layout) are dealt round-robin to the NW waves of the
// pixel; every wave has its own histogram buffer and covers all n samples of its groups, so the stage needs no barrier.
// (These kernels sit at the register limit of 2 or 1 waves per SIMD: the partner-major key registers of the one-wave kernels
// cost them spills, measured 305 -> 466 ms on a 4K x 32 spp slab together with an unrolled marginal read-back; round 3's
// read-back -- a rolled loop, sums stored at once -- fits: mi_group.)
template <int KD, int KW, int PACK5, int NW = 1, int NFULL = 0, int TSRC = 0>
__device__ __forceinline__ void mi_stage(const uint32_t *sBinW, uint32_t *sHist, const uint64_t *dtab, const uint64_t *ttab, uint64_t *sHXf,
                                         uint64_t *sPairF, int lane, int n, int B, int wv = 0) {
    int gi = 0; // running group number (wave-uniform)
    auto mine = [&]() { const bool m = (NW == 1) || (gi % NW) == wv; ++gi; return m; };
    // the live cells and, behind them, one always-zero cell per lane: the target of the +0 atomics of lanes without a sample in
    // a slot (mi_group; lds_layout() sizes the buffer for bmax * bmax + 64 cells); hist_lds = this wave's buffer as an LDS address
    const int ncell2 = B * B + kWave;
    const uint32_t hist_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)sHist;
    const uint32_t hole2 = hist_lds + ((uint32_t)(B * B + lane) << 2);
    zero_cells<0>(sHist, ncell2, lane);
    uint32_t akey[KD];
#pragma unroll
    for (int kk = 0; kk < KD; ++kk) akey[kk] = 0u;
    constexpr int kRemF = kNFeat % 4;
    // (the 19 marginal sums come off resident joints -- marginal_count -- not from histograms of their own)
    // ---- joint histograms, grouped by an anchor column whose (bin * B) stays in registers
    //   anchors r.., p.. with partners f.., c0..c2 ; anchors c0..c2 with partners f..
#pragma unroll 1
    for (int g = 0; g < kNAnc + 3; ++g) {
        const int acol = anchor_col(g);
        {
            BinIds<KW, PACK5> w;
            load_bins<KD, KW, PACK5>(sBinW, acol, lane, w);
#pragma unroll
            for (int kk = 0; kk < KD; ++kk) akey[kk] = w.get(kk) * (uint32_t)(B * 4) + hist_lds; // the anchor's row: its LDS address
        }
#pragma unroll 1
        for (int i0 = 0; i0 + 4 <= kNFeat; i0 += 4) { // feature partners, four per group
            if (!mine()) continue;
            uint64_t acc4[4];
            const int cols[4] = {kColF + i0, kColF + i0 + 1, kColF + i0 + 2, kColF + i0 + 3};
            // the marginal sums ride on joints that are resident anyway (marginal_T_sum): every partner's on anchor 0's
            // histograms, every r / p anchor's on the first histogram of its own group (the colour anchors are partners too)
            const int marg = (g == 0 ? 1 : 0) | (g < kNAnc && i0 == 0 ? 2 : 0);
            mi_group<KD, KW, 4, PACK5, true, NFULL, TSRC>(sBinW, sHist, dtab, lane, n, cols, akey, hole2, ncell2, acc4, marg, ttab, sHXf, acol, B);
            const uint64_t tot = xl::reduce4<xl::OpSum>(acc4);
            lds_store_u64_if((lane & 15) == 0, &sPairF[pair_index_of(g, i0 + xl::slot4(lane))], tot);
        }
        if constexpr (kRemF != 0) {
            if (mine()) {
                constexpr int i0 = kNFeat - kRemF;
                uint64_t acc4[4];
                const int cols[4] = {kColF + i0, kColF + min(i0 + 1, kNFeat - 1), kColF + min(i0 + 2, kNFeat - 1), kColF + kNFeat - 1};
                mi_group<KD, KW, kRemF, PACK5, true, NFULL, TSRC>(sBinW, sHist, dtab, lane, n, cols, akey, hole2, ncell2, acc4, g == 0 ? 1 : 0, ttab, sHXf, acol, B);
                const uint64_t tot = xl::reduce4<xl::OpSum>(acc4);
                lds_store_u64_if((lane & 15) == 0 && xl::slot4(lane) < kRemF, &sPairF[pair_index_of(g, min(i0 + xl::slot4(lane), kNFeat - 1))], tot);
            }
        }
        if (g < kNAnc && mine()) { // colour partners c0..c2 (wave-uniform branch)
            uint64_t acc4[4];
            const int cols[4] = {kColC, kColC + 1, kColC + 2, kColC + 2};
            mi_group<KD, KW, 3, PACK5, true, NFULL, TSRC>(sBinW, sHist, dtab, lane, n, cols, akey, hole2, ncell2, acc4, g == 0 ? 1 : 0, ttab, sHXf, acol, B);
            const uint64_t tot = xl::reduce4<xl::OpSum>(acc4);
            lds_store_u64_if((lane & 15) == 0 && xl::slot4(lane) < 3, &sPairF[pair_index_of(g, kNFeat + min(xl::slot4(lane), 2))], tot);
        }
    }
}

// wave minimum / maximum of the kNX plane columns (per-lane running values in) -> dmin[column], dmax[column] in LDS.
// Up to 16 columns ride one 32-slot transposed butterfly ([mins | -maxs]); wider layouts take one butterfly each.
__device__ __forceinline__ void wave_minmax(const float (&fmn)[kNX], const float (&fmx)[kNX], int lane, double *dmin, double *dmax) {
    const int slot = xl::slot32(lane);
    if constexpr (kNX <= 16) {
        float a32[32];
#pragma unroll
        for (int i = 0; i < 16; ++i) { a32[i] = i < kNX ? fmn[i] : INFINITY; a32[16 + i] = i < kNX ? -fmx[i] : INFINITY; }
        const float r = xl::reduce32<xl::OpMin>(a32, lane);
        if ((lane & 1) == 0) {
            const int i = slot & 15;
            if (i < kNX) {
                if (slot < 16) dmin[xcol(i)] = (double)r;
                else dmax[xcol(i)] = (double)(-r);
            }
        }
    } else {
        float a32[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) a32[i] = i < kNX ? fmn[i] : INFINITY;
        const float r0 = xl::reduce32<xl::OpMin>(a32, lane);
#pragma unroll
        for (int i = 0; i < 32; ++i) a32[i] = i < kNX ? -fmx[i] : INFINITY;
        const float r1 = xl::reduce32<xl::OpMin>(a32, lane);
        if ((lane & 1) == 0 && slot < kNX) { dmin[xcol(slot)] = (double)r0; dmax[xcol(slot)] = (double)(-r1); }
    }
}

// Flat-quad shortcut of stage 1b.  A feature whose S values inside the pixel are all equal has sigma == 0, and
// multiplyArray(std, 3) == 0 makes the strict test of rpf.cpp:577-580 fail for EVERY finite candidate (|f - m| >= 0): such a
// pixel keeps its own samples only -- 93.9 % of the pixels of a captured pbrt buffer (SURVEY F10).  The one candidate that
// would still pass that feature is a NaN one (NaN >= 0 is false), and a NaN sample makes its own pixel's stage-1a mean NaN:
// so if no pixel of the window has a NaN mean in that feature, N = S is proven with one load per window PIXEL instead of
// twelve gathers per window SAMPLE.  Returns true when proven (wave-uniform); false = run the general test.
// (The pixel's own mean must be finite: under the EPS policy stage 1a clamps a NaN sigma to 0, and |f - NaN| >= 0 is false
// for every candidate -- that feature then rejects nobody; a mean of +-inf (a sample at +-inf: sigma = sqrt(inf - inf) = NaN,
// clamped to 0) is passed by every candidate at the same infinity, |inf - inf| = NaN, whose own pixel's mean is not NaN.)
__device__ __forceinline__ bool flat_quad_shortcut(const PassParams &p, const double (&m12)[kNFeat], const double (&lim12)[kNFeat],
                                                   int lane, uint64_t HW, int x0, int y0, int nyv, int ncells, int centre_rank) {
    int k0 = -1;
#pragma unroll
    for (int k = 0; k < kNFeat; ++k)
        if (lim12[k] == 0.0 && isfinite(m12[k])) k0 = k;
    if (k0 < 0) return false; // wave-uniform
    const double *pm = p.pmean + (uint64_t)k0 * HW;
    bool nan_seen = false;
    for (int c0 = 0; c0 < ncells - 1; c0 += kWave) {
        int cell = c0 + lane;
        if (cell < ncells - 1) {
            if (cell >= centre_rank) ++cell;
            const int ix = cell / nyv, iy = cell - ix * nyv;
            nan_seen = nan_seen || isnan(pm[(uint64_t)(y0 + iy) * p.W + (x0 + ix)]);
        }
    }
    return !__any(nan_seen);
}

// ------------------------------------------------------------------------------------------------
// the fused per-pixel kernel
//   K         compile-time bound on samples per lane: K*64 >= nmax ; lane owns samples j = lane + 64*kk
//   T_IN_LDS  keep the D table in LDS (small neighbourhoods) instead of reading it through L1
// ------------------------------------------------------------------------------------------------
//   NW        waves per pixel.  1: the workgroup is one wavefront (8 spp: twelve pixels in flight per CU).  4 (large
//             neighbourhoods, whose 40-85 KiB of LDS would otherwise leave 1-3 waves on a CU): the waves of a pixel
//             share the member list, the bin ids and the own rows, and split the work by COLUMN (stages 2, 3a), by
//             HISTOGRAM GROUP (3b, one private histogram buffer per wave) and by OWN SAMPLE (4), so that every wave
//             still walks all n samples in lane + 64*kk order and the stages need a barrier only where they meet.
// PHASE (K = 25 and 49, four waves -- 32 and 64 spp): 0 = the whole pixel in one kernel.  At K = 49 a workgroup needs 147 KiB
// of LDS, so ONE wave per SIMD runs every stage at the pace of its own dependent instruction stream, and the weight stage
// (half of the 64-spp pass) and the in-order chains need none of that LDS.  The class therefore runs as three launches
// over the same pixel list, each rebuilding the member list from the acceptance masks of the count pass:
//   PHASE 3  stages 1b, 2: the in-order chains, 52 KiB of LDS, three workgroups per CU; leaves mean, SD, min, max of every
//            column in global memory (p.carry: kCarry doubles per pixel)
//   PHASE 4  stages 1b, 3a .. 3c with those statistics (the 147-KiB kernel: bin ids, histograms, table); adds alpha,
//            beta, W_r_c to the pixel's record
//   PHASE 2  stages 1b, 4: re-gathers the own samples and runs the weights with 42 KiB of LDS at two waves per SIMD
// Same arithmetic on the same doubles, same bits.
template <int K, bool T_IN_LDS, bool FAST, int NW, int PHASE>
// (wider layouts keep 18 + 18 feature statistics and 23 weighted columns per lane: two waves per SIMD for their small-K
// kernels, where the reference layout fits three, and one workgroup per CU for the four-wave kernels: at two their
// K = 25 instantiation spilled, and hipcc 7.2 placed those spill stores in front of the EXEC restore of a join block
// -- lanes masked off lost live registers; scripts/check_spills.py scans every build for that placement)
__global__ __launch_bounds__(64 * NW, PHASE == 2 ? 2 : PHASE == 3 ? (kRef19 ? 3 : 2) : (NW > 1 ? (K <= 25 && kRef19 ? 2 : 1) : (K <= 8 ? (kRef19 ? 3 : 2) : (K <= 13 ? 2 : 1)))) void filter_pixel_kernel(PassParams p, LdsLayout L) {
    constexpr int KW = pack_words(K);        // 32-bit words of packed bin ids per lane and column
    constexpr int PACK5 = pack_scheme(K);    // packing scheme, see BinIds
    extern __shared__ __align__(16) unsigned char smem[];
    uint64_t *sD = reinterpret_cast<uint64_t *>(smem + L.off_T); // D[c] = T[c+1]-T[c], 2^-44 fixed point
    // the same table through the LDS base itself: lds_layout() puts it first (off_T == 0, checked by launch_filter_pass), and
    // with a base the compiler knows mi_pgroup's look-ups are `ds_read_b64 v, v_count` with no address arithmetic
    const uint64_t *sD0 = reinterpret_cast<const uint64_t *>(smem);
    if constexpr (PHASE != 2 && PHASE != 3) { // mi_pgroup / mi_group read the table (head) at absolute LDS address 0 (dlook8_lds0)
        if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem != 0u) __builtin_trap();
    }
    double *sStat = reinterpret_cast<double *>(smem + L.off_stat); // M[19], SD[19], xmin[19], xmax[19]
    uint64_t *sHXf = reinterpret_cast<uint64_t *>(smem + L.off_hx);     // sum_i T[hx_i] per column (fixed point)
    uint64_t *sPairF = reinterpret_cast<uint64_t *>(smem + L.off_pair); // sum_ij T[J_ij] per pair (fixed point)
    double *sMI = reinterpret_cast<double *>(smem + L.off_pair);   // 96 MI values, in place over the pair sums
    double *sOwn = reinterpret_cast<double *>(smem + L.off_own);   // raw own samples [S][19]
    uint32_t *sOff = reinterpret_cast<uint32_t *>(smem + L.off_off);
    double *sStage = reinterpret_cast<double *>(smem + L.off_union);    // [19][kStageHalf+1] (aliases bins)
    uint32_t *sBinW = reinterpret_cast<uint32_t *>(smem + L.off_union); // bin ids [19][64][KW] words (K > 8)
    uint32_t *sHist0 = reinterpret_cast<uint32_t *>(smem + L.off_hist); // wave 0's histogram buffer (also scratch)

    const int tid = threadIdx.x;
    const int lane = NW > 1 ? (tid & (kWave - 1)) : tid;
    const int wv = NW > 1 ? __builtin_amdgcn_readfirstlane(tid >> 6) : 0; // in an SGPR: branches on it are scalar, no EXEC masking
    uint32_t *sHist = reinterpret_cast<uint32_t *>(smem + L.off_hist + (NW > 1 ? (uint32_t)wv * L.hist_stride : 0u));
    // hand-off between the waves of the pixel (s_barrier) -- or between the lanes of the only wave
    auto bsync = [&]() { if constexpr (NW > 1) __syncthreads(); else wsync(); };
    constexpr int kThreads = kWave * NW;
    const int W = p.W, H = p.H, S = p.S, b = p.b;

    // pixel of this workgroup: see slab_pixel(); a size-binned launch walks its pixel list instead, dealt to the
    // XCDs in eight contiguous chunks (the list is in slab_pixel order, so a chunk is again a band of strips)
    int x, y;
    if (p.pix_list != nullptr) {
        const uint32_t chunk = (p.list_count + 7u) / 8u;
        const uint32_t ql = blockIdx.x >> 3, e = (blockIdx.x & 7u) * chunk + ql;
        if (ql >= chunk || e >= p.list_count) return;
        const uint32_t pp = p.pix_list[e];
        y = (int)(pp / (uint32_t)W);
        x = (int)(pp - (uint32_t)y * (uint32_t)W);
    } else if (!slab_pixel(p, (int)(blockIdx.x & 7), (int64_t)(blockIdx.x >> 3), x, y)) {
        return;
    }
    const uint64_t HW = (uint64_t)H * W;
    const uint64_t pix = (uint64_t)y * W + x;


    if constexpr (PHASE == 2 || PHASE == 3) {
        // no histograms in the weight kernel and the chain kernel
    } else if (T_IN_LDS) {
        for (int k = tid; k < p.nmax; k += kThreads) sD[k] = p.dfix[k];
    } else if (K <= 8) {
        for (int k = tid; k < min(p.nmax, kDHead); k += kThreads) sD[k] = p.dfix[k]; // the head of the table (mi_pgroup)
    }

    // ---------------- stage 1b: neighbourhood membership (rpf.cpp:556-586) ----------------------
    const int x0 = max(x - b, 0), x1 = min(x + b, W - 1);
    const int y0 = max(y - b, 0), y1 = min(y + b, H - 1);
    const int nyv = y1 - y0 + 1;
    const int ncells = (x1 - x0 + 1) * nyv;
    const int centre_rank = (x - x0) * nyv + (y - y0);
    const int ncand = (ncells - 1) * S;
    const uint32_t magic_S = div_magic((uint32_t)S), magic_ny = div_magic((uint32_t)nyv); // qq < 4096, S, nyv <= 64

    // the member list holds offsets relative to the window's first sample (see Window)
    const Window win(p, ((uint64_t)y0 * W + x0) * S);
    const uint32_t own_rel = (uint32_t)((y - y0) * W + (x - x0)) * (uint32_t)S;
    [[maybe_unused]] const uint32_t win_par = ((uint32_t)(y0 * W + x0) * (uint32_t)S) & 1u; // parity of the origin's element index (fp16 planes)
    for (int s = tid; s < S; s += kThreads) sOff[s] = own_rel + (uint32_t)s; // own samples first

    int n = S;
    if constexpr (kListed) {
        // a listed build (RPF_IMPL_LISTED): the count kernel listed the members behind the own samples as plane offsets, in the
        // reference's visiting order; every thread of the workgroup copies, whatever NW and PHASE are.  The window's first sample
        // comes off, so that the entries are the window-relative offsets everything behind expects.  (n <= nmax by the class
        // deal: the bound only guards LDS.  member_base is read only where a pixel lists members: the count kernel reserves none
        // for N = S)
        n = min(p.nbhd[pix], p.nmax);
        if (n > S) {
            const uint32_t *pl = p.members + p.member_base[pix];
            const uint32_t origin = (uint32_t)(y0 * W + x0) * (uint32_t)S;
            for (int i = tid; i < n - S; i += kThreads) sOff[S + i] = pl[i] - origin;
        }
    } else if constexpr (NW > 1) {
        // Several waves: the 64-candidate blocks are dealt round-robin to the waves.  Pass A tests a wave's blocks and
        // leaves one acceptance mask per block in LDS; pass B turns the masks into list positions (an exclusive scan
        // over <= 64 block counts, done by every wave for itself) and appends, so the list order is the reference's.
        uint64_t *sMask = reinterpret_cast<uint64_t *>(sHist0);
        const int nblk = (ncand + kWave - 1) / kWave; // <= 64 (host-checked: nmax <= 4096)
        const bool have_masks = p.masks != nullptr;   // size-binned launch: nbhd_count_kernel already ran the test
        if (have_masks && tid < nblk) sMask[tid] = p.masks[pix * p.mask_stride + tid];
        double m12[kNFeat], lim12[kNFeat];
#pragma unroll
        for (int k = 0; k < kNFeat; ++k) {
            m12[k] = p.pmean[(uint64_t)k * HW + pix];
            lim12[k] = p.pstd[(uint64_t)k * HW + pix] * 3.0; // multiplyArray(std, 3), rpf.cpp:579
        }
        auto cand_off = [&](int qq) -> uint32_t {
            int cell = (int)div_small((uint32_t)qq, magic_S);
            const int s = qq - cell * S;
            if (cell >= centre_rank) ++cell;          // rpf.cpp:565: skip the centre pixel
            const int ix = (int)div_small((uint32_t)cell, magic_ny); // xn outer ascending (rpf.cpp:562)
            const int iy = cell - ix * nyv;            // yn inner ascending (rpf.cpp:563)
            return (uint32_t)(iy * W + ix) * (uint32_t)S + (uint32_t)s;
        };
        constexpr int kPF1 = kNFeat <= 12 ? 3 : 2;
        float fb[kPF1][kNFeat];
        auto issue1 = [&](int blk, float (&f)[kNFeat]) {
            const int qq = blk * kWave + lane;
            if (blk < nblk && qq < ncand) {
                gather_features(win, cand_off(qq), f);
            }
        };
#pragma unroll
        for (int u = 0; u < kPF1; ++u)
            if (!have_masks) issue1(wv + NW * u, fb[u]);
#pragma unroll 1
        for (int t0 = 0; !have_masks && wv + NW * t0 < nblk; t0 += kPF1) {
#pragma unroll
            for (int u = 0; u < kPF1; ++u) {
                const int blk = wv + NW * (t0 + u);
                if (blk < nblk) { // wave-uniform
                    bool pass = (blk * kWave + lane) < ncand;
#pragma unroll
                    for (int k = 0; k < kNFeat; ++k) {
                        const double a = fabs((double)fb[u][k] - m12[k]);
                        if (a >= lim12[k]) pass = false;       // allLessThan: fails iff a >= b (ops.h:101-104)
                    }
                    const unsigned long long mask = __ballot(pass);
                    if (lane == 0) sMask[blk] = mask;
                    issue1(blk + NW * kPF1, fb[u]);
                }
            }
        }
        __syncthreads();
        const int cnt = lane < nblk ? __popcll(sMask[lane]) : 0;
        int incl = cnt;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int t = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += t;
        }
        const int excl = incl - cnt;
#pragma unroll 1
        for (int blk = wv; blk < nblk; blk += NW) {
            const int base = S + __shfl(excl, blk, kWave);
            const unsigned long long mask = sMask[blk];
            const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
            if (((mask >> lane) & 1ull) && at < p.nmax) sOff[at] = cand_off(blk * kWave + lane);
        }
        n = S + __shfl(incl, kWave - 1, kWave);
    } else if (p.masks != nullptr) {
        // size-binned launch: nbhd_count_kernel already ran the 3-sigma test and left one acceptance mask per 64
        // candidates; only the list is rebuilt here (wave-uniform mask loads, no feature gathers)
        const uint64_t *pm = p.masks + pix * p.mask_stride;
#pragma unroll 1
        for (int qb = 0; qb < ncand; qb += kWave) {
            const unsigned long long mask = pm[qb >> 6];
            const int at = n + __popcll(mask & ((1ull << lane) - 1ull));
            if (((mask >> lane) & 1ull) && at < p.nmax) {
                const int qq = qb + lane;
                int cell = (int)div_small((uint32_t)qq, magic_S);
                const int s = qq - cell * S;
                if (cell >= centre_rank) ++cell;          // rpf.cpp:565: skip the centre pixel
                const int ix = (int)div_small((uint32_t)cell, magic_ny); // xn outer ascending (rpf.cpp:562)
                const int iy = cell - ix * nyv;            // yn inner ascending (rpf.cpp:563)
                sOff[at] = (uint32_t)(iy * W + ix) * (uint32_t)S + (uint32_t)s;
            }
            n += __popcll(mask);
        }
    } else {
        double m12[kNFeat], lim12[kNFeat];
#pragma unroll
        for (int k = 0; k < kNFeat; ++k) {
            m12[k] = p.pmean[(uint64_t)k * HW + pix];
            lim12[k] = p.pstd[(uint64_t)k * HW + pix] * 3.0; // multiplyArray(std, 3), rpf.cpp:579
        }
        // candidate -> plane offset of its sample, in the reference's visiting order
        auto cand_off = [&](int qq) -> uint32_t {
            int cell = (int)div_small((uint32_t)qq, magic_S);
            const int s = qq - cell * S;
            if (cell >= centre_rank) ++cell;          // rpf.cpp:565: skip the centre pixel
            const int ix = (int)div_small((uint32_t)cell, magic_ny); // xn outer ascending (rpf.cpp:562)
            const int iy = cell - ix * nyv;            // yn inner ascending (rpf.cpp:563)
            return (uint32_t)(iy * W + ix) * (uint32_t)S + (uint32_t)s;
        };
        // rotating register buffers: the 12 feature gathers of the next kPF1 64-candidate steps are in flight while
        // a step is tested and appended (an L2/MALL round trip is ~1-2k cycles under load, a step ~0.5k)
        constexpr int kPF1 = kNFeat <= 12 ? 3 : 2;
        float fb[kPF1][kNFeat];
        uint32_t ob[kPF1];
        auto issue1 = [&](int qq, float (&f)[kNFeat], uint32_t &off) {
            if (qq < ncand) {
                off = cand_off(qq);
                gather_features(win, off, f);
            }
        };
        // (the shortcut needs the masks only where somebody reads them: a re-routed pixel with N = S reads none)
        const bool proven = flat_quad_shortcut(p, m12, lim12, lane, HW, x0, y0, nyv, ncells, centre_rank);
#pragma unroll
        for (int u = 0; u < kPF1; ++u)
            if (!proven) issue1(u * kWave + lane, fb[u], ob[u]);
#pragma unroll 1
        for (int q0 = 0; !proven && q0 < ncand; q0 += kWave * kPF1) {
#pragma unroll
            for (int u = 0; u < kPF1; ++u) {
                const int qb = q0 + u * kWave;
                if (qb < ncand) { // wave-uniform
                    bool pass = (qb + lane) < ncand;
#pragma unroll
                    for (int k = 0; k < kNFeat; ++k) {
                        const double a = fabs((double)fb[u][k] - m12[k]);
                        if (a >= lim12[k]) pass = false;       // allLessThan: fails iff a >= b (ops.h:101-104)
                    }
                    const unsigned long long mask = __ballot(pass);
                    if (p.reroute_masks != nullptr && lane == 0) p.reroute_masks[pix * p.mask_stride + (uint32_t)(qb >> 6)] = mask;
                    const int at = n + __popcll(mask & ((1ull << lane) - 1ull));
                    if (pass && at < p.nmax) sOff[at] = ob[u]; // (at < nmax always: the bound only guards LDS)
                    n += __popcll(mask);
                    issue1(qb + kWave * kPF1 + lane, fb[u], ob[u]);
                }
            }
        }
    }
    bsync();
    if constexpr (!kListed) { // (a listed build took N from there)
        if (tid == 0) p.nbhd[pix] = n;
    }
    if constexpr (NW == 1 && PHASE == 0 && !kListed) { // (every one-wave kernel: the unbinned route reaches K = 13 at 448 < box*box*S <= 512)
        // a small neighbourhood (the regime of path-traced buffers, SURVEY F10) is not this kernel's business: the packed
        // kernels filter 8 / 4 / 2 / 1 such pixels per wave from the masks left above (rpf_packed_impl.inc)
        if (p.reroute_masks != nullptr && n <= 64) return; // wave-uniform; classify_kernel lists the pixel by its N
    }

    if (p.dbg.member_hash != nullptr && tid == 0) {
        uint32_t h = 2166136261u;
        for (int j = 0; j < n; ++j) {
            const uint32_t o = sOff[j];                 // relative to the window origin (x0, y0): pp = iy * W + ix, ix < W
            const uint32_t s = o % (uint32_t)S;
            const uint32_t pp = o / (uint32_t)S;
            const int yn = y0 + (int)(pp / (uint32_t)W), xn = x0 + (int)(pp % (uint32_t)W);
            h = fnv1a_u32(h, (uint32_t)(((xn - x + b) * p.box + (yn - y + b)) * S) + s);
        }
        p.dbg.member_hash[pix] = h;
    }

    // scratch of stages 3c / 4 in the (then dead) histogram buffer: Drf[NF] | Drc,Dpc,Dfc [9 (12)] | alpha[3 (4)] | beta[NF] | wrc (4) | coef[kNWt]
    double *sT = reinterpret_cast<double *>(sHist0);
    double *sDrf = sT, *sD9 = sDrf + kNFeat, *sAlpha = sD9 + 12, *sBeta = sAlpha + 4, *sWrc = sBeta + kNFeat, *sCoef = sWrc + 4;
    int *sBadFlag = reinterpret_cast<int *>(sCoef + ((kNWt + 3) & ~3)); // NW > 1: did any wave of the pixel see a NaN colour
    static_assert((2 * kNFeat + 20 + ((kNWt + 3) & ~3) + 1) * 8 <= 1024, "stage 3c scratch must fit the smallest histogram buffer");
    constexpr int kCarry = (4 * kNDim + kNFeat + 5 + 7) & ~7; // doubles per pixel of the split route: [M | SD | min | max | alpha | beta | wrc | redo flag]
    if constexpr (PHASE != 2) {
    if constexpr (PHASE != 4) {
    // ---------------- stage 2: mean / std over the neighbourhood, reference order ---------------
    // Chunks of 64 samples: lane t gathers all 19 values of sample j0+t (the next chunk is already in
    // flight in registers), stages them (two halves of 32) as doubles [column][t] in LDS, then lanes 0..18 run the in-order
    // sum(x) chain of column `lane` and lanes 32..50 the sum(x*x) chain of column `lane-32`.
    // The per-column min / max of x ride along (order independent): z = (x-M)/SD is monotone in x, so
    // min z = z(min x) and max z = z(max x) exactly, which is all mi.cpp:47-50 needs.
    if constexpr (NW > 1) {
        // Several waves: the in-order chains cannot be split (fp64 addition is not associative), so two waves do nothing
        // but run them while the others are producers: in round r producer w gathers the 19 values of the 64 samples of
        // chunk r*NP+w (issued one round ahead), tracks the column min / max and stages the chunk as doubles
        // [column][65] in its own LDS buffer.  Barrier A: the buffers of the round are complete; the chain waves walk
        // them in order while the producers' next gathers are in flight; barrier B: the buffers may be overwritten.
        // Two chain waves: wave 0 sums x, wave 1 sums x*x (lanes 0..18 each) -- a wave's own instruction stream is what
        // bounds a chain, and one wave doing both needed a per-element select; waves 2.. are the producers.
        constexpr int NCH = 2;
        constexpr int NP = NW - NCH;
        constexpr int kCS = kStageChunk + 1; // doubles per staged column
        const int nrun = (p.stage_mask & 1) ? n : 0;
        const int nround = (nrun + NP * kStageChunk - 1) / (NP * kStageChunk);
        double *sMM = reinterpret_cast<double *>(sHist0); // [NP][38]: column min | max seen by each producer
        double *sSq = sMM + NP * 2 * kNDim;               // [19]: wave 1's sums of squares
        double chain_acc = 0.0;                           // chain waves: the running sum of column `lane`
        if (wv < NCH) {
            auto chain_loop = [&](auto sq_tag) {
                constexpr bool SQ = decltype(sq_tag)::value;
                double acc = 0.0;
                const bool chain = lane < kNDim;
                for (int r = 0; r < nround; ++r) {
                    lds_barrier(); // A
                    if (nrun - r * NP * kStageChunk >= NP * kStageChunk) {
                        // full round: NP*4 batches of 16 staged values, the reads of batch t+1 issued before batch t
                        // is summed (this wave is alone on its SIMD: nothing else hides the LDS latency)
                        constexpr int NB = NP * (kStageChunk / 16);
                        const double *col = sStage + (chain ? lane : 0) * kCS;
                        double vb[2][16];
                        auto load16 = [&](int t, double (&v)[16]) {
                            const double *src = col + (t / 4) * (kNDim * kCS) + (t % 4) * 16;
#pragma unroll
                            for (int q = 0; q < 16; ++q) v[q] = src[q];
                        };
                        load16(0, vb[0]);
#pragma unroll
                        for (int t = 0; t < NB; ++t) {
                            if (t + 1 < NB) load16(t + 1, vb[(t + 1) & 1]);
                            double (&v)[16] = vb[t & 1];
                            if constexpr (SQ) {
#pragma unroll
                                for (int q = 0; q < 16; ++q) v[q] = v[q] * v[q];       // ops.h:138 multiplyArrays
                            }
#pragma unroll
                            for (int q = 0; q < 16; ++q) acc = acc + v[q];             // ops.h:121 / 138 sumArrays
                        }
                    } else {
#pragma unroll 1
                        for (int w = 0; w < NP; ++w) {
                            const int cnt = min(kStageChunk, nrun - (r * NP + w) * kStageChunk); // wave-uniform
                            if (cnt <= 0) break;
                            if (chain) {
                                const double *src = sStage + w * (kNDim * kCS) + lane * kCS;
                                int q0 = 0;
                                for (; q0 + 16 <= cnt; q0 += 16) {
                                    double v[16];
#pragma unroll
                                    for (int q = 0; q < 16; ++q) v[q] = src[q0 + q];
                                    if constexpr (SQ) {
#pragma unroll
                                        for (int q = 0; q < 16; ++q) v[q] = v[q] * v[q];
                                    }
#pragma unroll
                                    for (int q = 0; q < 16; ++q) acc = acc + v[q];
                                }
                                for (int q = q0; q < cnt; ++q) { const double v = src[q]; acc = acc + (SQ ? v * v : v); }
                            }
                        }
                    }
                    lds_barrier(); // B
                }
                return acc;
            };
            if (wv == 0) {
                chain_acc = chain_loop(std::false_type{});
            } else {
                const double sq = chain_loop(std::true_type{});
                if (lane < kNDim) sSq[lane] = sq;
            }
        } else {
            float fmn[kNX], fmx[kNX];  // the plane columns: pFilm, then random parameters and features
            double cmn[3], cmx[3];
#pragma unroll
            for (int i = 0; i < kNX; ++i) { fmn[i] = INFINITY; fmx[i] = -INFINITY; }
#pragma unroll
            for (int i = 0; i < 3; ++i) { cmn[i] = INFINITY; cmx[i] = -INFINITY; }
            double *sStageP = sStage + (wv - NCH) * (kNDim * kCS);
            float vf[kNX];
            double vd[3];
            auto fetch = [&](int j) {
                if (j < nrun) {
                    gather_sample(win, sOff[j], vf, vd);
                }
            };
            fetch((wv - NCH) * kStageChunk + lane);
            // (a second register set -- the gathers of rounds r + 1 and r + 2 in flight -- changed nothing: 3840x270x32 chains
            // 37.5 -> 38 ms; the round is not waiting for its gathers)
            for (int r = 0; r < nround; ++r) {
                const int j0 = (r * NP + wv - NCH) * kStageChunk;
                if (j0 + lane < nrun) {
#pragma unroll
                    for (int i = 0; i < kNX; ++i) {
                        fmn[i] = fminf(fmn[i], vf[i]);
                        fmx[i] = fmaxf(fmx[i], vf[i]);
                        sStageP[xcol(i) * kCS + lane] = (double)vf[i];
                    }
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        cmn[i] = fmin(cmn[i], vd[i]);
                        cmx[i] = fmax(cmx[i], vd[i]);
                        sStageP[(kColC + i) * kCS + lane] = vd[i];
                    }
                    if (j0 + lane < S) { // own samples are entries 0..S-1 of the neighbourhood
#pragma unroll
                        for (int i = 0; i < kNX; ++i) sOwn[(j0 + lane) * kNDim + xcol(i)] = (double)vf[i];
#pragma unroll
                        for (int i = 0; i < 3; ++i) sOwn[(j0 + lane) * kNDim + kColC + i] = vd[i];
                    }
                }
                fetch(j0 + NP * kStageChunk + lane); // in flight across both barriers, while wave 0 chains
                lds_barrier(); // A
                lds_barrier(); // B
            }
            // this wave's min / max of x per column -> sMM[wv-1][c], sMM[wv-1][19 + c]
            double *mm = sMM + (wv - NCH) * (2 * kNDim);
            wave_minmax(fmn, fmx, lane, mm, mm + kNDim);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double lo = xl::allreduce<xl::OpMin>(cmn[i]), hi = xl::allreduce<xl::OpMax>(cmx[i]);
                if (lane == 0) { mm[kColC + i] = lo; mm[kNDim + kColC + i] = hi; }
            }
        }
        __syncthreads();
        if (tid < kNDim) { // wave 0 holds the sums, wave 1 left the sums of squares in LDS
            const double dn = (double)n;
            const double mean = chain_acc / dn;                       // ops.h:123
            double sd = sqrt(sSq[tid] / dn - mean * mean);            // ops.h:141
            if (p.policy == RPF_DEGEN_EPS && isnan(sd)) sd = 0.0;
            sStat[tid] = mean;
            sStat[kNDim + tid] = sd;
            if (p.dbg.mean) p.dbg.mean[pix * kNDim + tid] = mean;
            if (p.dbg.stddev) p.dbg.stddev[pix * kNDim + tid] = sd;
        }
        if (tid < 2 * kNDim) { // min over the producers (slots 0..18), max (slots 19..37)
            double v = sMM[tid];
#pragma unroll
            for (int w = 1; w < NP; ++w) v = tid < kNDim ? fmin(v, sMM[w * 2 * kNDim + tid]) : fmax(v, sMM[w * 2 * kNDim + tid]);
            sStat[2 * kNDim + tid] = v;
        }
        __syncthreads();
    } else {
        float fmn[kNX], fmx[kNX];  // the plane columns: pFilm, then random parameters and features
        double cmn[3], cmx[3];
#pragma unroll
        for (int i = 0; i < kNX; ++i) { fmn[i] = INFINITY; fmx[i] = -INFINITY; }
#pragma unroll
        for (int i = 0; i < 3; ++i) { cmn[i] = INFINITY; cmx[i] = -INFINITY; }
        {
            // RPF_CHAIN_BOTH: lane c < 19 runs both in-order chains of column c -- sum(x) and sum(x*x): a multiply and two
            // adds per sample on two independent dependency chains; the other lanes idle.  (The earlier form gave the
            // squares to lanes 32..50 and paid for it with a multiply and a 64-bit select per element in every lane:
            // four instructions per sample.  Same additions, same operands, same order: the same bits.)
            double acc = 0.0;
            [[maybe_unused]] double accq = 0.0;
            const int myc = RPF_CHAIN_BOTH ? lane : (lane & 31);
            const bool chain = myc < kNDim;
            [[maybe_unused]] const bool is_sq = lane >= 32;
            const int nrun = (p.stage_mask & 1) ? n : 0;
            float vf[kNX];
            double vd[3];
            auto fetch = [&](int j) {
                if (j < nrun) {
                    gather_sample(win, sOff[j], vf, vd);
                }
            };
            fetch(lane);
            for (int j0 = 0; j0 < nrun; j0 += kStageChunk) {
                const int cnt = min(kStageChunk, nrun - j0);
                if (lane < cnt) {
#pragma unroll
                    for (int i = 0; i < kNX; ++i) {
                        fmn[i] = fminf(fmn[i], vf[i]);
                        fmx[i] = fmaxf(fmx[i], vf[i]);
                    }
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        cmn[i] = fmin(cmn[i], vd[i]);
                        cmx[i] = fmax(cmx[i], vd[i]);
                    }
                    if (j0 + lane < S) { // own samples are entries 0..S-1 of the neighbourhood
#pragma unroll
                        for (int i = 0; i < kNX; ++i) sOwn[(j0 + lane) * kNDim + xcol(i)] = (double)vf[i];
#pragma unroll
                        for (int i = 0; i < 3; ++i) sOwn[(j0 + lane) * kNDim + kColC + i] = vd[i];
                    }
                }
                // the 64 gathered samples go through the LDS staging buffer 32 at a time ([19][33] doubles: 5 KiB)
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    const int cnth = min(kStageHalf, cnt - hf * kStageHalf); // wave-uniform, may be <= 0
                    const int t = lane - hf * kStageHalf;
                    if (t >= 0 && t < cnth) {
#pragma unroll
                        for (int i = 0; i < kNX; ++i) sStage[xcol(i) * (kStageHalf + 1) + t] = (double)vf[i];
#pragma unroll
                        for (int i = 0; i < 3; ++i) sStage[(kColC + i) * (kStageHalf + 1) + t] = vd[i];
                    }
                    wsync();
                    if (hf == 1) fetch(j0 + kStageChunk + lane); // next chunk's gathers overlap the serial chains below
                    if (chain && cnth > 0) {
                        const double *src = sStage + myc * (kStageHalf + 1);
                        if (cnth == kStageHalf) { // full half: LDS reads issue 16 at a time, only the adds are serial
#pragma unroll
                            for (int h = 0; h < kStageHalf; h += 16) {
                                double v[16];
#pragma unroll
                                for (int q = 0; q < 16; ++q) v[q] = src[h + q];
#if RPF_CHAIN_BOTH
#pragma unroll
                                for (int q = 0; q < 16; ++q) {
                                    acc = acc + v[q];                                   // ops.h:121 sumArrays
                                    accq = accq + v[q] * v[q];                          // ops.h:138 multiplyArrays, sumArrays
                                }
#else
#pragma unroll
                                for (int q = 0; q < 16; ++q) v[q] = is_sq ? v[q] * v[q] : v[q]; // ops.h:138 multiplyArrays (branch-free)
#pragma unroll
                                for (int q = 0; q < 16; ++q) acc = acc + v[q];          // ops.h:121 / 138 sumArrays
#endif
                            }
#if RPF_CHAIN_BOTH
                        } else {
                            for (int q = 0; q < cnth; ++q) { const double v = src[q]; acc = acc + v; accq = accq + v * v; }
                        }
#else
                        } else if (!is_sq) {
                            for (int q = 0; q < cnth; ++q) acc = acc + src[q];
                        } else {
                            for (int q = 0; q < cnth; ++q) { const double v = src[q]; acc = acc + v * v; }
                        }
#endif
                    }
                    wsync();
                }
            }
#if RPF_CHAIN_BOTH
            const double sq = accq;
#else
            const double sq = __shfl(acc, (lane & 31) + 32, 64);
#endif
            const double dn = (double)n;
            const double mean = acc / dn;                      // ops.h:123
            double sd = sqrt(sq / dn - mean * mean);           // ops.h:141
            if (p.policy == RPF_DEGEN_EPS && isnan(sd)) sd = 0.0;
            if (lane < kNDim) {
                sStat[lane] = mean;
                sStat[kNDim + lane] = sd;
                if (p.dbg.mean) p.dbg.mean[pix * kNDim + lane] = mean;
                if (p.dbg.stddev) p.dbg.stddev[pix * kNDim + lane] = sd;
            }
            // wave min / max of x per column -> sStat[38 + c], sStat[57 + c]
            {
                wave_minmax(fmn, fmx, lane, sStat + 2 * kNDim, sStat + 3 * kNDim);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double lo = xl::allreduce<xl::OpMin>(cmn[i]), hi = xl::allreduce<xl::OpMax>(cmx[i]);
                    if (lane == 0) { sStat[2 * kNDim + kColC + i] = lo; sStat[3 * kNDim + kColC + i] = hi; }
                }
            }
            wsync();
        }

    }
    } else {
        // PHASE 4: the statistics the chain kernel left for this pixel
        bsync();
        const double *cr = p.carry + pix * kCarry;
        for (int k = tid; k < 4 * kNDim; k += kThreads) sStat[k] = cr[k];
        bsync();
    }
    if constexpr (PHASE == 3) {
        double *cw = p.carry + pix * kCarry;
        for (int k = tid; k < 4 * kNDim; k += kThreads) cw[k] = sStat[k];
        return;
    }

    // ---------------- stage 3a: normalise, bin ids: bins_stage() above --------------------------
    const int B = max(1, (int)sqrt((double)n)); // mi.cpp:54
    const int kdyn = (n + kWave - 1) / kWave;   // wave-uniform: sample slots kk < kdyn exist
    double *sCK = reinterpret_cast<double *>(sPairF); // [19][5] column constants (the pair sums are not live before 3b)
    if (tid < kNDim) column_constants(sStat, sCK, tid);
    bsync();
    if constexpr (K <= 8) {
        switch (kdyn) {
        case 1: bins_stage<1, KW, PACK5>(p, win, sStat, sOff, sBinW, lane, n, B, sCK); break;
        case 2: if constexpr (K >= 2) bins_stage<2, KW, PACK5>(p, win, sStat, sOff, sBinW, lane, n, B, sCK); break;
        case 3: if constexpr (K >= 3) bins_stage<3, KW, PACK5>(p, win, sStat, sOff, sBinW, lane, n, B, sCK); break;
        case 4: if constexpr (K >= 4) bins_stage<4, KW, PACK5>(p, win, sStat, sOff, sBinW, lane, n, B, sCK); break;
        case 5: if constexpr (K >= 5) bins_stage<5, KW, PACK5>(p, win, sStat, sOff, sBinW, lane, n, B, sCK); break;
        case 6: if constexpr (K >= 6) bins_stage<6, KW, PACK5>(p, win, sStat, sOff, sBinW, lane, n, B, sCK); break;
        case 7: if constexpr (K >= 7) bins_stage<7, KW, PACK5>(p, win, sStat, sOff, sBinW, lane, n, B, sCK); break;
        default: if constexpr (K >= 8) bins_stage<8, KW, PACK5>(p, win, sStat, sOff, sBinW, lane, n, B, sCK); break;
        }
    } else {
        bins_stage<K, KW, PACK5, NW>(p, win, sStat, sOff, sBinW, lane, n, B, sCK, wv);
    }
    bsync();
    if (p.dbg.bin_hash != nullptr && tid < kNDim) { // debug only: hash in sample order j = lane + 64*slot
        uint32_t h = 2166136261u;
        for (int j = 0; j < n; ++j) h = fnv1a_u16(h, bin_of_sample<KW, PACK5>(sBinW, tid, j));
        p.dbg.bin_hash[pix * kNDim + tid] = h;
    }
    // ---------------- stage 3b: histograms -> mutual information: mi_stage() above ------------
    if (p.stage_mask & 4) {
        const uint64_t *dtab = T_IN_LDS ? sD : p.dfix;
        if constexpr (K <= 8 && kRef19) {
            // one straight-line instantiation per number of occupied sample slots (and per number of 1-KiB clearing
            // stores): no branch sits between the LDS operations of a histogram group, so they pipeline under
            // counted lgkmcnt waits
#define RPF_MI_CASE(KD_)                                                                                     \
    if constexpr (K >= KD_) {                                                                                \
        if constexpr (KD_ == 1) mi_stage_tiny<KW, PACK5>(sBinW, sHist, p.tfix, sHXf, sPairF, lane, n, B); /* B*B <= 64 */ \
        else if constexpr (KD_ == 2) mi_stage_deep<KD_, KW, 1, PACK5>(sBinW, sHist, dtab, sHXf, sPairF, lane, n, B); /* B*B <= 121 */ \
        else if (B * B <= 256) mi_pm<KD_, KW, 1, PACK5, !T_IN_LDS>(sBinW, sHist, dtab, sD0, p.tfix, sHXf, sPairF, lane, n, B); \
        else if (B * B <= 320) mi_pm<KD_, KW, 3, PACK5, !T_IN_LDS>(sBinW, sHist, dtab, sD0, p.tfix, sHXf, sPairF, lane, n, B); \
        else if (B * B <= 384) mi_pm<KD_, KW, 4, PACK5, !T_IN_LDS>(sBinW, sHist, dtab, sD0, p.tfix, sHXf, sPairF, lane, n, B); \
        else mi_pm<KD_, KW, 2, PACK5, !T_IN_LDS>(sBinW, sHist, dtab, sD0, p.tfix, sHXf, sPairF, lane, n, B);               \
    }
            switch (kdyn) {
            case 1: RPF_MI_CASE(1) break;
            case 2: RPF_MI_CASE(2) break;
            case 3: RPF_MI_CASE(3) break;
            case 4: RPF_MI_CASE(4) break;
            case 5: RPF_MI_CASE(5) break;
            case 6: RPF_MI_CASE(6) break;
            case 7: RPF_MI_CASE(7) break;
            default: RPF_MI_CASE(8) break;
            }
#undef RPF_MI_CASE
        } else {
            // a pixel of this kernel's own size class fills the sample slots the next smaller kernel holds (the class bounds are
            // 64 * {7, 13, 25, 49}): those slots need no mask on their atomics and look-ups
            constexpr int kFullSlots = K == 13 ? 7 : (K == 25 ? 13 : (K == 49 ? 25 : 0));
            // (Round 3's first session gave the one-wave K = 13 kernel a table head in LDS, reference layout only: its 27-dim
            // instantiation returned wrong, run-to-run varying pair sums with the head intact and no count past it -- "a
            // difference in generated code that was not tracked down".  It was the SCC hazard of lds_store_u64_if, see there.)
            // (the K = 13 kernel's table head of round 3's first session is gone: mi_group's cheaper form is faster without it, and
            // the kilobyte it took is part of what bought the kernel two more resident workgroups per CU)
            constexpr int kTSrc = T_IN_LDS ? 1 : 0; // the table at LDS address 0 (lds_layout: off_T == 0)
            if (kFullSlots > 0 && n > kWave * kFullSlots) mi_stage<K, KW, PACK5, NW, kFullSlots, kTSrc>(sBinW, sHist, dtab, p.tfix, sHXf, sPairF, lane, n, B, wv);
            else mi_stage<K, KW, PACK5, NW, 0, kTSrc>(sBinW, sHist, dtab, p.tfix, sHXf, sPairF, lane, n, B, wv);
        }
    }
    bsync();
    {
        const int64_t TNf = (int64_t)p.tfix[n];
        const double dn = (double)n;
        for (int pr = tid; pr < kNPair; pr += kThreads) {
            int ca, cb;
            pair_cols(pr, ca, cb);
            int64_t f = TNf + (int64_t)sPairF[pr] - (int64_t)sHXf[ca] - (int64_t)sHXf[cb];
            // Exactly independent histograms (J_ij N == hx_i hy_j on every occupied cell): the reference's terms are
            // p log(1.0) == 0 exactly whenever its quotients are exact (always for N a power of two, e.g. N == S), and
            // that exact zero decides 0/0 at rpf.cpp:465/470.  The table entries are rounded to 2^-44, so such a sum
            // lands within (#terms / 2) units of zero instead of on it: snap it.  (A non-zero N*MI is >= 1/(2 N^2 E),
            // orders of magnitude above the bound for all but contrived N > 1700 tables.)  This is the EPS contract
            // (DESIGN.md section 2) and, under REF_ABORT, the exact answer whenever the pixel is not redone (below).
            const int64_t zero_band = ((int64_t)B * B + 2 * B + 1) / 2 + 1;
            if (f <= zero_band && f >= -zero_band) f = 0;
            const double mi = ldexp((double)f, -kTFixBits) / dn;
            sMI[pr] = mi;
            if (p.dbg.mi) p.dbg.mi[pix * kNPair + pr] = mi;
        }
    }
    // REF_ABORT promises the reference's own value.  When N is not a power of two and both columns of a pair occupy more
    // than one bin, mi.cpp:79-86 returns rounding RESIDUE for a table inside the band (its quotients are 1 +- a few ulp),
    // not 0, and rpf.cpp:465/470 divide those residues by each other.  Such a pixel (rare: it needs an exactly independent
    // table) is appended to the redo list and filtered again, whole, by generic::filter_pixel_kernel, which evaluates the
    // reference's floating-point expression for these tables.  A one-bin column makes the integer sum an exact 0 and the
    // reference's terms exact zeros: nothing to redo.  (A second walk over the pairs, only taken at non-power-of-two N: the
    // test inside the loop above cost the K = 7 kernel a spilled register.)
    // The verdict is left in LDS (the column sums are dead) and read again where the pixel's status is reported: the pixel
    // runs on (an early exit here cost the K = 7 kernel a spilled register), its colours are overwritten by the redo.
    static_assert(kNDim % 2 == 1, "the 16-byte aligned column-sum block has one spare 8-byte slot behind an odd number of columns");
    int *sRedo = reinterpret_cast<int *>(sHXf + kNDim); // ... which nothing else writes until the kernel ends
    if (tid == 0) sRedo[0] = 0;
    bsync(); // the MI values of every pair are in LDS
    if (p.redo_list != nullptr && (n & (n - 1)) != 0) { // uniform
        const int64_t TNf = (int64_t)p.tfix[n];
        bool redo = false;
        for (int pr = tid; pr < kNPair; pr += kThreads) {
            int ca, cb;
            pair_cols(pr, ca, cb);
            if (sMI[pr] == 0.0 && (int64_t)sHXf[ca] != TNf && (int64_t)sHXf[cb] != TNf) redo = true;
        }
        bsync();
        if (redo) sRedo[0] = 1;
    }
    bsync();

    // ---------------- stage 3c: alpha, beta, W_r_c (rpf.cpp:444-487), lane-parallel -----------------
    // lane k < kNFeat owns feature k, lane c < 3 also owns colour channel c; values meet through a scratch area in the
    // (now dead) histogram buffer: Drf[NF] | Drc,Dpc,Dfc [9 (12)] | alpha[3 (4)] | beta[NF] | wrc (4) | coef[kNWt]
    if (NW == 1 || wv == 0) {
        const int k = min(lane, kNFeat - 1), c = min(lane, 2);
        double Drf = 0.0, Dpf = 0.0, Dcf = 0.0, Drc = 0.0, Dpc = 0.0, Dfc = 0.0;
        const int base = kNPairF + c * kNPairC;
#pragma unroll
        for (int l = 0; l < kNR; ++l) { Drf += sMI[k * kNAnc + l]; Drc += sMI[base + l]; }                 // rpf.cpp:421, 432
#pragma unroll
        for (int l = 0; l < 2; ++l) { Dpf += sMI[k * kNAnc + kNR + l]; Dpc += sMI[base + kNR + l]; }       // rpf.cpp:425, 436
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) Dcf += sMI[kNPairF + cc * kNPairC + kNAnc + k]; // PAPER numerator: sum_c MI(c_c, f_k)
#pragma unroll
        for (int j = 0; j < kNFeat; ++j) Dfc += sMI[base + kNAnc + j]; // rpf.cpp:440
        wsync(); // every lane has read its MI values; the scratch area may now be written
        if (lane < kNFeat) sDrf[lane] = Drf;
        if (lane < 3) { sD9[lane] = Drc; sD9[3 + lane] = Dpc; sD9[6 + lane] = Dfc; }
        wsync();
        double D_f_c = 0.0, D_r_c = 0.0, D_p_c = 0.0;             // rpf.cpp:449-456
#pragma unroll
        for (int i = 0; i < 3; ++i) { D_f_c += sD9[6 + i]; D_r_c += sD9[i]; D_p_c += sD9[3 + i]; }
        const double e = (p.policy == RPF_DEGEN_EPS) ? p.eps : 0.0;
        const double den = D_f_c + D_r_c + D_p_c + e;
        double wsum = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) wsum += sD9[i] / (sD9[i] + sD9[3 + i] + e); // rpf.cpp:470, 485
        const double wrc = wsum / 3;                                           // rpf.cpp:487
#if RPF_IMPL_SCHED
        const double alpha_c = schedule_factor(p.gain_c, Drc / (Drc + Dpc + e)); // clamp0(1 - g_c W_r^{c,k}): DESIGN.md 15a, the quotient of rpf.cpp:470
#else
        const double alpha_c = 1 - Drc / (Drc + Dpc + e);                      // rpf.cpp:470, 475
#endif
        double num; // what rpf.cpp:464 reads as D_f_ck[k] (3-element array indexed to 11: SURVEY F3)
        if (p.beta_map == RPF_BETA_PAPER) num = Dcf;
        else if (p.beta_map == RPF_BETA_REF_GCC11_O2) num = k < 3 ? sD9[6 + c] : (k < 8 ? 0.0 : sDrf[max(k - 8, 0)]);
        else num = k < 3 ? sD9[6 + c] : (k < 4 ? 0.0 : sDrf[max(k - 4, 0)]);
        const double Wc = num / den;                       // rpf.cpp:464
        const double Wr = Drf / (Drf + Dpf + e);           // rpf.cpp:465
#if RPF_IMPL_SCHED
        const double beta_k = schedule_factor(p.gain_f, Wr) * Wc; // clamp0(1 - g_f W_r^{f,k}) W_c^{f,k}: DESIGN.md 15a
#else
        const double beta_k = (1 - Wr) * Wc;               // rpf.cpp:479
#endif
        if (lane < kNFeat) {
            sBeta[lane] = beta_k;
            if (p.dbg.beta) p.dbg.beta[pix * kNFeat + lane] = beta_k;
        }
        if (lane < 3) {
            sAlpha[lane] = alpha_c;
            if (p.dbg.alpha) p.dbg.alpha[pix * 3 + lane] = alpha_c;
        }
        if (lane == 0) {
            sWrc[0] = wrc;
            if (NW > 1) sBadFlag[0] = 0;
            if (p.dbg.wrc) p.dbg.wrc[pix] = wrc;
        }
        wsync();
    }
    if constexpr (NW == 1 && PHASE == 0) {
        // own samples kept inside the histogram buffer (lds_layout: the one-wave K = 13 kernel): the histograms overwrote what
        // stage 2 left there -- gathered again (entries 0 .. S-1 of the member list)
        if (L.off_own >= L.off_hist) { // (wave-uniform)
            for (int j = lane; j < S; j += kWave) {
                float vf[kNX];
                double vd[3];
                gather_sample(win, sOff[j], vf, vd);
#pragma unroll
                for (int i = 0; i < kNX; ++i) sOwn[j * kNDim + xcol(i)] = (double)vf[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) sOwn[j * kNDim + kColC + i] = vd[i];
            }
            wsync();
        }
    }
    } else {
        // PHASE 2: what stage 4 reads -- the own samples (entries 0 .. S-1 of the member list), and the statistics and
        // weights the two earlier kernels left for this pixel
        bsync();
        for (int j = tid; j < S; j += kThreads) {
            float vf[kNX];
            double vd[3];
            gather_sample(win, sOff[j], vf, vd);
#pragma unroll
            for (int i = 0; i < kNX; ++i) sOwn[j * kNDim + xcol(i)] = (double)vf[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) sOwn[j * kNDim + kColC + i] = vd[i];
        }
        const double *cr = p.carry + pix * kCarry;
        if (cr[4 * kNDim + 3 + kNFeat + 1] != 0.0) return; // handed to the reference-expression kernel by PHASE 4 (uniform)
        for (int k = tid; k < 2 * kNDim; k += kThreads) sStat[k] = cr[k]; // M | SD
        if (tid < 3) sAlpha[tid] = cr[4 * kNDim + tid];
        if (tid < kNFeat) sBeta[tid] = cr[4 * kNDim + 3 + tid];
        if (tid == 0) { sWrc[0] = cr[4 * kNDim + 3 + kNFeat]; sBadFlag[0] = 0; }
    }
    if constexpr (NW > 1) __syncthreads();
    const double wrc = sWrc[0];
    if constexpr (PHASE == 4) {
        double *cw = p.carry + pix * kCarry;
        if (tid < 3) cw[4 * kNDim + tid] = sAlpha[tid];
        if (tid < kNFeat) cw[4 * kNDim + 3 + tid] = sBeta[tid];
        if (tid == 0) {
            cw[4 * kNDim + 3 + kNFeat] = wrc;
            const bool redo = reinterpret_cast<const int *>(sHXf + kNDim)[0] != 0; // the weight kernel skips a redo pixel
            cw[4 * kNDim + 3 + kNFeat + 1] = redo ? 1.0 : 0.0;
            if (redo) p.redo_list[atomicAdd(p.redo_count, 1u)] = (uint32_t)pix;
        }
        return;
    }

    // ---------------- stage 4: weights and blend (rpf.cpp:627-717) ------------------------------
    // z-space set-up shared by both weight modes (dead LDS regions: x-min/x-max slots -> M and 1/SD of the 17 weighted
    // columns; bin ids -> the own samples' rows).  With z = (x-M)/SD the exponent of w_ij is
    //     sum_k cz_k (z_ik - z_jk)^2 = A_i + B_j + sum_k u_ik z_jk,   cz_k = weight_k / (2 sigma^2),
    //     A_i = sum_k cz_k z_ik^2,  B_j = sum_k cz_k z_jk^2,  u_ik = -2 cz_k z_ik :
    // 17 FMAs per pair instead of 17 x (sub, mul, fma).  z is O(1) by construction, so the cancellation in
    // A + B - 2 dot costs ~1e-15 * cz in E (cz <= ~1e5): far below what exp() resolves.
    double *sFastM = sStat + 2 * kNDim;  // the x-min / x-max slots are dead after stage 3a
    double *sFastI = sFastM + kNWt;
    constexpr int kFZ = (kNWt + 3) & ~3;     // FAST: floats per own row (16-byte reads)
    constexpr int kOR = (kNWt + 2) & ~1;     // !FAST: doubles per own row = u_i0 .. u_i(kNWt-1), A_i (+ pad): 16-byte reads
    constexpr int kW4 = (kNWt / 4) * 4;
    auto wcol = [](int k) { return k < 5 ? k : k + kNR; }; // weighted column k -> column of the sample vector
    float *sFastZ = reinterpret_cast<float *>(sBinW);   // FAST: own z rows, fp32 [S][kFZ]
    double *sOwnU = reinterpret_cast<double *>(sBinW);  // !FAST: own rows, fp64 [S][kOR]
    // Far-pair screen of the large-K kernels.  With the reference's sigma^2 most cross pairs have an exponent in the
    // thousands and exp(-E) is exactly 0 (SURVEY F4); the fp64 dot product and the exp() polynomial for such a pair are
    // 47 instructions that add 0.0 to four sums.  A second copy of every own row in fp32, [u_i | A_i(1-eps)] with two
    // own samples interleaved, and of the sample's z give S32 = A(1-eps) + B(1-eps) - 747 + sum_k u_ik z_jk for two own
    // samples per packed FMA (18 in the reference layout).  Its rounding error is below 20 * 2^-24 * (|A| + |B| +
    // sum |u z|) <= 2.4e-6 (A + B) -- input rounding included, |sum u z| <= 2 sqrt(AB) <= A + B -- so with eps = 5e-6,
    // S32 > 0 proves E > 746 and exp(-E) == 0.0 (the last denormal is exp(-745.13)).  Where every lane of the wave
    // proves that for both own samples of a pair, their fp64 path is skipped; anything else -- a near pair, a NaN, an
    // fp32 overflow -- takes it unchanged, so the filtered colours are bit-for-bit those of the unscreened kernel.
#ifdef RPF_NO_SCREEN
    constexpr bool kScreen = false;
#else
    constexpr bool kScreen = !FAST && NW > 1;          // (the one-wave K = 13 kernel sweeps 16 own samples: 16 spp 251 -> 261 ms with it)
#endif
#ifndef RPF_EVOTE
#define RPF_EVOTE 1
#endif
    // the one-wave K = 13 kernel: a vote on the fp64 exponents of a sweep step skips its exp() pass (16 spp: 225.1 -> 222.6 ms).
    // Not the K <= 8 kernels: at 8 spp a sweep step spans eight pixels' samples and is hardly ever far in every lane -- the verdict
    // changes nothing there and the two-pass form costs 0.6 ms of 61 (gpurun_out/r3r).
    constexpr bool kEVote = RPF_EVOTE && !FAST && !kScreen && K == 13;
    constexpr int kQP = (kNWt + 2) & ~1;                // floats per own sample in the fp32 copy: u_0 .. u_(kNWt-1), A (+ pad)
    constexpr double kScreenShrink = 1.0 - 5e-6;
    float *sOwnQ = reinterpret_cast<float *>(sOwnU + S * kOR); // [ceil(S/2)][kQP][2]
    // (A cheaper screen on the three colour terms alone -- E >= sum_c cz_c (z_ic - z_jc)^2, six packed instructions per
    // pair of own samples -- was measured on the same frames: the z-normalised colours of a smooth neighbourhood
    // cluster, it rarely proves anything, and 32 / 64 spp went 291 -> 348 / 613 -> 771 ms.  Not kept.)
    float coefz[kNWt];
    {
        const double sigma_c2 = p.seed * p.seed / (1 - wrc) / (1 - wrc);     // rpf.cpp:662
        const double inv2sc = 1.0 / (2 * sigma_c2), inv2sp = 1.0 / (2 * (p.sigma_p * p.sigma_p)); // rpf.cpp:664,668
#pragma unroll
        for (int k = 0; k < kNWt; ++k) {
            const double wkk = k < 2 ? 1.0 : (k < 5 ? sAlpha[k >= 2 && k < 5 ? k - 2 : 0] : sBeta[k >= 5 ? k - 5 : 0]);
            coefz[k] = (float)(wkk * (k < 2 ? inv2sp : inv2sc));
        }
        bsync(); // every wave has read alpha / beta: the coefficient slots may be overwritten
        if (tid < kNWt) {
            const int col = wcol(lane);
            const double sd = sStat[kNDim + col];
            const double wkk = lane < 2 ? 1.0 : (lane < 5 ? sAlpha[max(lane - 2, 0)] : sBeta[max(lane - 5, 0)]);
            sFastM[lane] = sStat[col];
            sFastI[lane] = (sd == 0.0) ? 0.0 : 1.0 / sd; // SD == 0 normalises to z == 0 (ops.h:48)
            sCoef[lane] = wkk * (lane < 2 ? inv2sp : inv2sc); // cz_k (overwrites the raw-space coefficient slot)
        }
        bsync();
        // (SD == 0 gives z = 0 by a select, not by (x - M) * 0: a column whose samples hold +-inf has M = +-inf or NaN and SD =
        // NaN, which EPS clamps to 0 -- there x - M is inf or NaN, and the reference's z is still 0, ops.h:48)
        if constexpr (FAST) {
            for (int t = tid; t < S * kFZ; t += kThreads) {
                const int i = t / kFZ, k = t - i * kFZ;
                float z = 0.f;
                if (k < kNWt && sFastI[k] != 0.0) z = (float)((sOwn[i * kNDim + wcol(k)] - sFastM[k]) * sFastI[k]);
                sFastZ[t] = z;
            }
        } else {
            for (int i = tid; i < S; i += kThreads) {
                double A = 0.0;
#pragma unroll
                for (int k = 0; k < kNWt; ++k) {
                    const double z = sFastI[k] == 0.0 ? 0.0 : (sOwn[i * kNDim + wcol(k)] - sFastM[k]) * sFastI[k];
                    const double t = sCoef[k] * z;
                    A = fma(t, z, A);
                    sOwnU[i * kOR + k] = -2.0 * t;
                    if constexpr (kScreen) sOwnQ[((i >> 1) * kQP + k) * 2 + (i & 1)] = (float)(-2.0 * t);
                }
                sOwnU[i * kOR + kNWt] = A;
                if constexpr (kScreen) {
                    float *q = sOwnQ + (i >> 1) * kQP * 2 + (i & 1);
                    q[kNWt * 2] = (A < 1e30) ? (float)(A * kScreenShrink) : __builtin_nanf(""); // NaN: never "far"
#pragma unroll
                    for (int k = kNWt + 1; k < kQP; ++k) q[k * 2] = 0.f;
                    if (i == S - 1 && (S & 1)) { // odd S: the missing partner of the last own sample is never "far"... nor live
#pragma unroll
                        for (int k = 0; k < kQP; ++k) q[k * 2 + 1] = 0.f;
                    }
                }
            }
        }
        bsync();
    }
    // (one-wave kernels) no weighted column of this pixel has SD == 0: the sweeps form z without the select.  Wave-uniform.
    [[maybe_unused]] bool z_plain = false;
    if constexpr (NW == 1 && RPF_Z_HOIST && !FAST) z_plain = !__any(lane < kNWt && sFastI[min(lane, kNWt - 1)] == 0.0);
    bool bad = false;
    // own samples weighted per sweep over the neighbourhood (register budget: 4 at 3 waves/SIMD; the multi-wave kernels
    // run 1-2 waves/SIMD and take 8, halving the per-sample set-up, and gather one sample slot ahead)
    // (the weight kernel of the split 64-spp route has the registers for 16 as well: 64 spp 465 -> 435 ms; the 27-dim one spills)
    constexpr int kOwnBlock = ((NW == 1 && K == 13) || (PHASE == 2 && kRef19)) ? 16 : 8;
    double *sRed = sMI + 16 * wv; // 16 sums of a sweep meet here (the MI values are dead; one slot set per wave)
    // NW > 1: the sweeps are dealt round-robin to the waves of the pixel
    for (int i0 = kOwnBlock * wv; i0 < ((p.stage_mask & 8) ? S : 0); i0 += kOwnBlock * NW) {
        double sw[kOwnBlock], s0[kOwnBlock], s1[kOwnBlock], s2[kOwnBlock];
#pragma unroll
        for (int ii = 0; ii < kOwnBlock; ++ii) { sw[ii] = 0.0; s0[ii] = 0.0; s1[ii] = 0.0; s2[ii] = 0.0; }
        // raw values of the lane's next neighbourhood sample are gathered while the current one is weighted
        float pf[2 + kNFeat];  // pFilm and the features
        double pc[3];  // colours
        auto fetch17 = [&](int j) { // lanes past the end re-load the last sample (no branch, never an invalid address)
            gather_weighted(win, sOff[min(j, n - 1)], pf, pc);
        };
        // gathers one sample slot ahead (a second register set) in the four-wave kernels.  Not in the weight kernel of the
        // split route: with 16 own samples per sweep the second set spilled 6-7 registers per sweep step INSIDE the loop --
        // 86 GB of scratch writes per 32-spp launch for no gain in time (64 spp: 437 ms with the spills, 459 without).
        // (The 27-dim weight kernel, 8 own samples per sweep: 85 GB of scratch writes and 18 % slower with the second set.)
        constexpr bool kAhead = NW > 1 && PHASE != 2;
        if constexpr (kAhead) fetch17(lane);
        // The weight kernel of the split route prefetches WITHOUT registers: the next slot's 17 values go global -> LDS
        // directly (global_load_lds: per-lane source address, destination = wave-uniform base + 4 * lane) while the current
        // slot is weighted, one [value][lane] image per wave (L.off_T: this kernel keeps no table).  At two waves per SIMD every
        // slot otherwise begins with an exposed gather round trip.
        // Always dword loads (a 64-bit size operand crashes hipcc 7.2's instruction selection, and the LDS placement of a
        // sub-dword global_load_lds is not lane * size: with 2-byte loads the 27-dim layout's results came out wrong): an fp16
        // plane value arrives as the aligned dword that holds it, and the half is picked by the parity of its element index.
        // (The one-wave kernels do not take it: at three waves per SIMD their gather latency is covered already, and the staging
        // instructions cost more than they hide -- 1080p x 8: 65.3 -> 66.9 ms, 16 spp 246 -> 247 ms with it.)
        constexpr bool kGlds = !FAST && PHASE == 2;
        constexpr bool kHalfPlanes = sizeof(plane_t) == 2;
        constexpr int kPreRowF = kWave * 4;                              // bytes per staged plane value row
        constexpr int kPreBytes = (2 + kNFeat) * kPreRowF + 6 * kWave * 4; // + three fp64 colours as two dwords each
        // (one-wave kernels: behind the own rows, in the dead bin-id region -- lds_layout() sizes the union for it -- except the
        // last two rows, which sit in the dead MI values behind the 16 reduction slots: with them in the union the 8-spp
        // workgroup was 128 bytes too large for twelve per CU)
        constexpr int kPreRows = 2 + kNFeat + 6;
        constexpr int kPreMain = PHASE == 2 ? kPreRows : kPreRows - 2;
        unsigned char *sPre = PHASE == 2 ? smem + L.off_T + (uint32_t)wv * (uint32_t)kPreBytes
                                         : reinterpret_cast<unsigned char *>(sOwnU) + (((uint32_t)S * kOR * 8u + 15u) & ~15u);
        unsigned char *sPre2 = reinterpret_cast<unsigned char *>(sMI + 16); // rows kPreMain .. (one-wave kernels only)
        auto pre_row = [&](int r) -> unsigned char * { return r < kPreMain ? sPre + r * kPreRowF : sPre2 + (r - kPreMain) * kPreRowF; };
        uint32_t off_cur = 0u, off_nxt = 0u; // fp16 planes: the staged slot's plane offset (parity of the element index)
        auto prefetch17 = [&](int j) { // lanes past the end re-load their last sample: never an invalid address
            const uint32_t off = sOff[min(j, n - 1)]; // relative to the window origin
            off_nxt = off;
#pragma unroll
            for (int k = 0; k < 2 + kNFeat; ++k) {
                // byte address of the value; fp16 planes: of the aligned dword that holds it
                const uint64_t a = (uint64_t)(uintptr_t)(win.pl + (uint64_t)(k < 2 ? k : kColF + (k - 2)) * win.pb) + ((uint64_t)off << (kHalfPlanes ? 1 : 2));
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(uintptr_t)(kHalfPlanes ? (a & ~3ull) : a),
                                                 (__attribute__((address_space(3))) void *)pre_row(k), 4, 0, 0);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint64_t a = (uint64_t)(uintptr_t)(win.co + (uint64_t)k * win.cb) + ((uint64_t)off << 3);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(uintptr_t)a,
                                                 (__attribute__((address_space(3))) void *)pre_row(2 + kNFeat + 2 * k), 4, 0, 0);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(uintptr_t)(a + 4),
                                                 (__attribute__((address_space(3))) void *)pre_row(2 + kNFeat + 2 * k + 1), 4, 0, 0);
            }
        };
        auto take17 = [&]() { // the staged slot -> registers; the image may be overwritten once these reads have returned
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            off_cur = off_nxt;
#pragma unroll
            for (int k = 0; k < 2 + kNFeat; ++k) {
                const uint32_t wd = reinterpret_cast<const uint32_t *>(pre_row(k))[lane];
                if constexpr (kHalfPlanes) {
                    // which half of the dword: the parity of the value's element index in the plane buffer (4-byte aligned)
                    const uint32_t par = (((uint32_t)(k < 2 ? k : kColF + (k - 2)) & (uint32_t)p.plane_stride) + win_par + off_cur) & 1u;
                    pf[k] = (float)__ushort_as_half((unsigned short)(wd >> (16u * par)));
                } else {
                    pf[k] = __uint_as_float(wd);
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint32_t lo = reinterpret_cast<const uint32_t *>(pre_row(2 + kNFeat + 2 * k))[lane];
                const uint32_t hi = reinterpret_cast<const uint32_t *>(pre_row(2 + kNFeat + 2 * k + 1))[lane];
                const uint64_t u = ((uint64_t)hi << 32) | (uint64_t)lo;
                pc[k] = __longlong_as_double((long long)u);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        };
        if constexpr (kGlds) {
            if (i0 < ((p.stage_mask & 8) ? S : 0)) prefetch17(lane);
        }
        if constexpr (!FAST) {
            // The own rows [u_i0 .. u_i(kNWt-1), A_i] are wave-uniform operands of every pair's dot product.  They live ACROSS
            // the lanes of register pairs -- value k < 16 of own sample ii in lane k of every 16-lane row of rowlo[ii], the
            // values past 16 of kOwnsPerQ own samples side by side in rowhi[] -- and each FMA takes its operand by DPP
            // row_newbcast (xl::fmac_rowbc): nine 8-byte LDS reads per sweep step instead of nine 16-byte broadcast reads per
            // (own sample, sweep step) -- those were a quarter of the one-wave kernels' LDS time and an exposed round trip per
            // pair at two waves per SIMD -- and 18 registers for eight rows instead of 36 for one.  Same FMAs in the same order: the same bits.  DPP reads the
            // register of ANOTHER lane, so every lane stays enabled through a sweep step: the loop bound is wave-uniform and a
            // lane past the end of the neighbourhood weighs 0 (its colours are zeroed: 0 x inf would be NaN).
            static_assert(kNWt >= 16 && kOR - 16 <= 8, "own rows: 16 values in rowlo, the rest (at most 8) in rowhi");
            constexpr int kRowHi = kOR - 16;                                   // u_16 .. u_(kNWt-1), A_i (+ pad)
            constexpr int kHiPad = kRowHi <= 2 ? 2 : (kRowHi <= 4 ? 4 : 8);
            constexpr int kOwnsPerQ = 16 / kHiPad;
            constexpr int kNQ = (kOwnBlock + kOwnsPerQ - 1) / kOwnsPerQ;
            int l16 = lane & 15;
            const int nu = __builtin_amdgcn_readfirstlane(n);
            // The sweep loop exists twice in the one-wave kernels (RPF_Z_HOIST): whether a weighted column has SD == 0 is a
            // property of the pixel, so the select that forces its z to 0 (a compare and two v_cndmask per column and sweep
            // step, on a wave-uniform condition) is left out of the copy that runs when no such column exists.  Both copies
            // compute (x - M) * (1 / SD) there: the same bits.  One scalar branch per sweep, no EXEC region.
            auto sweep = [&](auto plain_tag) {
            constexpr bool kPlainZ = decltype(plain_tag)::value;
#pragma unroll 1
            for (int kk = 0; kk < K; ++kk) {
                const int j = lane + kWave * kk;
                if (kWave * kk >= nu) break;                 // wave-uniform: no lane leaves a sweep step early
                const bool lane_ok = j < n;
                if constexpr (kGlds) {
                    take17();
                    prefetch17(j + kWave);
                } else if constexpr (!kAhead) {
                    fetch17(j); // no register double-buffering: three waves per SIMD cover the gather latency
                }
                double zj[kNWt], cj[3];
                double Bj = 0.0;
                if constexpr (NW == 1) {
                // the per-column constants (M, 1 / SD, c_z: wave-uniform, read from LDS by broadcast) in batches of four columns:
                // one wait per batch instead of one per column (the compiler reads each pair just in time and waits at once).
                // One-wave kernels: 1080p x 8 61.2 -> 60.9 ms, 16 spp 179.2 -> 175.1; the four-wave kernels lose 0.6 % with it.
#pragma unroll
                for (int k0 = 0; k0 < kNWt; k0 += 4) {
                    double cm[4], ci[4], cc[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int k = min(k0 + g, kNWt - 1);
                        cm[g] = sFastM[k]; ci[g] = sFastI[k]; cc[g] = sCoef[k];
                    }
                    asm volatile("" : "+v"(cm[0]), "+v"(cm[1]), "+v"(cm[2]), "+v"(cm[3]), "+v"(ci[0]), "+v"(ci[1]), "+v"(ci[2]), "+v"(ci[3]),
                                      "+v"(cc[0]), "+v"(cc[1]), "+v"(cc[2]), "+v"(cc[3]));
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int k = k0 + g;
                        if (k < kNWt) {
                            const double xv = k < 2 ? (double)pf[k] : (k < 5 ? pc[k < 5 && k >= 2 ? k - 2 : 0] : (double)pf[k >= 5 ? k - 3 : 0]);
                            double z = (xv - cm[g]) * ci[g];
                            if constexpr (!kPlainZ) z = ci[g] == 0.0 ? 0.0 : z;
                            zj[k] = z;
                            Bj = fma(cc[g] * z, z, Bj);
                        }
                    }
                }
                } else {
#pragma unroll
                for (int k = 0; k < kNWt; ++k) {
                    const double xv = k < 2 ? (double)pf[k] : (k < 5 ? pc[k < 5 && k >= 2 ? k - 2 : 0] : (double)pf[k >= 5 ? k - 3 : 0]);
                    const double z = sFastI[k] == 0.0 ? 0.0 : (xv - sFastM[k]) * sFastI[k];
                    zj[k] = z;
                    Bj = fma(sCoef[k] * z, z, Bj);
                }
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) cj[k] = lane_ok ? pc[k] : 0.0;
                if constexpr (kAhead) fetch17(j + kWave); // the next slot's gathers fly while this one is weighted
                typedef float v2f __attribute__((ext_vector_type(2)));
                bool skip[kOwnBlock / 2];
#pragma unroll
                for (int pp = 0; pp < kOwnBlock / 2; ++pp) skip[pp] = false;
                if constexpr (kScreen) {
                    float zq[kQP];
#pragma unroll
                    for (int k = 0; k < kQP; ++k) zq[k] = k < kNWt ? (float)zj[k] : (k == kNWt ? 1.f : 0.f);
                    // (a neighbour whose COLOUR is not finite is never "far": 0.0 x inf is NaN in the reference's sums, and
                    // rpf.cpp:702 exits on it -- the screened path must not turn that pixel finite)
                    // (0 x (c_r + c_g + c_b) is NaN exactly when a colour is inf / NaN or their sum overflows: one compare, no
                    // extra live registers -- three separate tests cost this kernel 46 spilled registers)
                    const double Bc = Bj + 0.0 * ((cj[0] + cj[1]) + cj[2]);
                    const float Bq = (Bc < 1e30) ? (float)(Bj * kScreenShrink - 747.0) : __builtin_nanf("");
                    // (The fp32 rows as DPP row broadcasts, like the fp64 ones below -- one v_fmac_f32_dpp per (own sample, column)
                    // instead of one v_pk_fma_f32 per (pair of own samples, column) fed by nine 16-byte LDS reads per pair -- was
                    // measured: twice the screen's VALU instructions for 72 fewer LDS reads per sweep step, 32 spp 232.5 -> 237.5 ms,
                    // 64 spp 357.9 -> 366.6 ms (gpurun_out/r3t).  Not kept: this kernel does not wait for those reads.)
#pragma unroll
                    for (int pp = 0; pp < kOwnBlock / 2; ++pp) { // own samples i0 + 2 pp, + 1 in the two halves of a packed FMA
                        const float4 *rq = reinterpret_cast<const float4 *>(sOwnQ + min((i0 >> 1) + pp, (S - 1) >> 1) * (kQP * 2));
                        v2f acc = {Bq, Bq};
#pragma unroll
                        for (int q = 0; q < kQP / 2; ++q) {
                            const float4 v = rq[q];
                            const v2f r0 = {v.x, v.y}, r1 = {v.z, v.w};
                            acc = __builtin_elementwise_fma(r0, (v2f)(zq[2 * q]), acc);
                            acc = __builtin_elementwise_fma(r1, (v2f)(zq[2 * q + 1]), acc);
                        }
                        skip[pp] = __all((acc.x > 0.f && acc.y > 0.f) || !lane_ok) && p.screen != 0; // false for NaN (option "screen" 0: the test runs, its verdict is dropped)
                    }
                }
                // straight-line over the kOwnBlock own samples (a missing one re-reads the last row and its weight is
                // forced to 0) so their dependent chains interleave; the 17-term dot product runs as four partial sums.
                // (Skipping only exp() behind a vote on the fp64 exponent was tried in four forms -- a wave-uniform branch
                // per own sample, one per sweep step over stored exponents, the stored form and a two-pass vote with a
                // predictor in the large-K kernels -- and every one spills: 24 .. 140 registers at three waves per SIMD
                // (75.9 vs 69.8 ms), 44 .. 101 in the K = 13 / 25 kernels (32 spp: 313 -> 400 ms).  The accumulators of 8
                // own samples + the sample's 17 z values + one own row fill the register file.  The layout with fewer
                // live accumulators was built too -- lanes are own samples, a 64-sample block normalised lane-parallel
                // and staged row-wise in LDS, each group of lanes reading its row by broadcast: 8 accumulator registers,
                // every parity test green -- and it moves the stage from the VALU to the LDS pipe (ten 16-byte
                // broadcast reads per 64 pairs plus the row stores): 8 spp 63.7 -> 93.6 ms, 32 spp 313 -> 307, 64 spp
                // 661 -> 632.  Not kept.  What is kept is the fp32 screen above: on the benchmark frames 77 % (32 spp) and
                // 85 % (64 spp) of the 64 x 8 sweep steps are far in every lane.)
                // (loaded per sweep step, behind the z values: held across the gathers and the z formation of a step they cost
                // the K <= 8 kernels 61 spilled registers; the opaque lane index keeps the loads inside the loop)
                double rowlo[kOwnBlock], rowhi[kNQ];
                asm volatile("" : "+v"(l16));
#pragma unroll
                for (int ii = 0; ii < kOwnBlock; ++ii) rowlo[ii] = sOwnU[min(i0 + ii, S - 1) * kOR + l16];
#pragma unroll
                for (int q = 0; q < kNQ; ++q) {
                    const int ii = min(q * kOwnsPerQ + l16 / kHiPad, kOwnBlock - 1);
                    rowhi[q] = sOwnU[min(i0 + ii, S - 1) * kOR + 16 + min(l16 % kHiPad, kRowHi - 1)];
                }
#if RPF_ROWS_EARLY
                // all row reads issued (and waited for) here, in front of the own-sample loop: without this the compiler sinks
                // each read next to its first use and every own sample starts with an exposed LDS round trip
#pragma unroll
                for (int ii = 0; ii < kOwnBlock; ++ii) asm volatile("" : "+v"(rowlo[ii]));
#pragma unroll
                for (int q = 0; q < kNQ; ++q) asm volatile("" : "+v"(rowhi[q]));
#endif
                // Two passes over the own samples of the sweep: the exponents first, then exp() and the sums -- and the second
                // pass only if some lane needs it.  With the reference's sigma^2 most sweep steps hold nothing but far pairs
                // (SURVEY F4): E > 746 in every lane for every own sample, every weight exactly 0.0 (the last denormal is
                // exp(-745.13)), and adding w = 0.0 and fma(0.0, c_j, s) leaves the four sums as they are -- unless a c_j is not
                // finite (0 x inf = NaN, which rpf.cpp:702 turns into an abort: such a lane never votes "far"; NaN exponents do
                // not either).  One wave-uniform branch per sweep step around straight-line code; same bits either way.
                // (Round 2 tried this vote four ways and every one spilled: the own rows now live across lanes -- 18 registers
                // instead of 36 -- and the kernels have the room.  kEVote kernels only; the screen of the four-wave kernels
                // works per pair of own samples in fp32, in front of the exponents.)
                auto exponent = [&](auto iic) -> double { // E_ij of own sample ii of the sweep and this lane's neighbour j
                    constexpr int ii = decltype(iic)::value;
                    // (an own-sample slot past S re-reads row S - 1; its sums are never stored)
                    constexpr int qi = ii / kOwnsPerQ, qb = (ii % kOwnsPerQ) * kHiPad;
                    double e0 = xl::rowbc<qb + (kNWt - 16), true>(rowhi[qi]) + Bj, e1 = 0.0, e2 = 0.0, e3 = 0.0; // A_i + B_j
                    xl::static_for<0, kNWt>([&](auto kc) {
                        constexpr int k = decltype(kc)::value;
                        double &e = (k >= kW4 || (k & 3) == 0) ? e0 : ((k & 3) == 1 ? e1 : ((k & 3) == 2 ? e2 : e3));
                        if constexpr (k < 16) xl::fmac_rowbc<k>(e, rowlo[ii], zj[k]);
                        else xl::fmac_rowbc<qb + (k - 16)>(e, rowhi[qi], zj[k]);
                    });
                    return (e0 + e1) + (e2 + e3);
                };
                auto weigh = [&](auto iic, double E) {
                    constexpr int ii = decltype(iic)::value;
                    double w = exp(-E);                         // rpf.cpp:667-670
                    w = lane_ok ? w : 0.0;
                    sw[ii] += w;                                // rpf.cpp:691
                    s0[ii] = fma(w, cj[0], s0[ii]);             // rpf.cpp:692 (raw neighbourhood colours)
                    s1[ii] = fma(w, cj[1], s1[ii]);
                    s2[ii] = fma(w, cj[2], s2[ii]);
                };
                if constexpr (kEVote) {
                    double Ev[kOwnBlock];
                    xl::static_for<0, kOwnBlock>([&](auto iic) { Ev[decltype(iic)::value] = exponent(iic); });
                    bool far = (0.0 * ((cj[0] + cj[1]) + cj[2])) == 0.0; // finite colours (one compare: see the screen above)
#pragma unroll
                    for (int ii = 0; ii < kOwnBlock; ++ii) far = far && (Ev[ii] > 746.0);
                    if (p.screen != 0 && __all(far || !lane_ok)) continue; // every weight of this sweep step is exactly 0.0
                    xl::static_for<0, kOwnBlock>([&](auto iic) { weigh(iic, Ev[decltype(iic)::value]); });
                } else {
                    xl::static_for<0, kOwnBlock>([&](auto iic) {
                        if (skip[decltype(iic)::value >> 1]) return; // (screen) both own samples of the pair weigh exactly 0.0 in every lane
                        weigh(iic, exponent(iic));
                    });
                }
            }
            };
            if constexpr (NW == 1 && RPF_Z_HOIST) {
                if (z_plain) sweep(std::true_type{});
                else sweep(std::false_type{});
            } else {
                sweep(std::false_type{});
            }
        } else {
            // opt-in RPF_FLAG_FAST_WEIGHTS: per-pair arithmetic in fp32 on z-space values (x-M)/SD that are formed in
            // fp64 (so large world coordinates do not cancel in fp32), v_exp_f32, fp64 accumulation of the sums.
            // Filtered colours differ from the fp64 path by ~1e-6 relative (bar: 1e-4).
#pragma unroll 1
            for (int kk = 0; kk < K; ++kk) {
                const int j = lane + kWave * kk;
                if (j >= n) break;
                if constexpr (!kAhead) fetch17(j);
                float zj[kNWt];
                double cj[3];
                zj[0] = (float)(((double)pf[0] - sFastM[0]) * sFastI[0]);
                zj[1] = (float)(((double)pf[1] - sFastM[1]) * sFastI[1]);
#pragma unroll
                for (int k = 0; k < 3; ++k) { cj[k] = pc[k]; zj[2 + k] = (float)((pc[k] - sFastM[2 + k]) * sFastI[2 + k]); }
#pragma unroll
                for (int k = 0; k < kNFeat; ++k) zj[5 + k] = (float)(((double)pf[2 + k] - sFastM[5 + k]) * sFastI[5 + k]);
#pragma unroll
                for (int k = 0; k < kNWt; ++k)
                    if (sFastI[k] == 0.0) zj[k] = 0.f;
                if constexpr (kAhead) fetch17(j + kWave);
#pragma unroll
                for (int ii = 0; ii < kOwnBlock; ++ii) {
                    const int i = i0 + ii;
                    if (i < S) {
                        const float *zi = sFastZ + i * kFZ; // rows padded to whole 16-byte reads (20 floats in the reference layout)
                        float zo[kFZ];
#pragma unroll
                        for (int q4 = 0; q4 < kFZ / 4; ++q4) {
                            const float4 v = reinterpret_cast<const float4 *>(zi)[q4];
                            zo[4 * q4] = v.x; zo[4 * q4 + 1] = v.y; zo[4 * q4 + 2] = v.z; zo[4 * q4 + 3] = v.w;
                        }
                        float E = 0.f;
#pragma unroll
                        for (int k = 0; k < kNWt; ++k) {
                            const float d = zo[k] - zj[k];
                            E = fmaf(d * d, coefz[k], E);
                        }
                        const double w = (double)__expf(-E);
                        sw[ii] += w;
                        s0[ii] = fma(w, cj[0], s0[ii]);
                        s1[ii] = fma(w, cj[1], s1[ii]);
                        s2[ii] = fma(w, cj[2], s2[ii]);
                    }
                }
            }
        }
        // 16 wave sums by one transposed butterfly, gathered through LDS: [0..3] sum w, [4..7] r, [8..11] g, [12..15] b
#pragma unroll
        for (int hb = 0; hb < kOwnBlock; hb += 4) {
            double ga[16];
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) { ga[ii] = sw[hb + ii]; ga[4 + ii] = s0[hb + ii]; ga[8 + ii] = s1[hb + ii]; ga[12 + ii] = s2[hb + ii]; }
            const double ta = xl::reduce16<xl::OpSum>(ga, lane);
            wsync();
            if ((lane & 3) == 0) sRed[xl::slot16(lane)] = ta;
            wsync();
            if (lane < 12) {
                const int ii = lane / 3, k = lane % 3;
                const int i = i0 + hb + ii;
                if (i < S) {
                    double prime = sRed[4 * (k + 1) + ii] / sRed[ii];     // rpf.cpp:700
                    if (isnan(prime)) {                                    // rpf.cpp:702: the reference exits here
                        bad = true;
                        if (p.policy == RPF_DEGEN_EPS) prime = sOwn[i * kNDim + kColC + k];
                    }
                    p.col_out[(uint64_t)k * p.plane_stride + pix * S + i] = prime;
                }
            }
        }
    }
    // a pixel on the redo list (stage 3b) reports nothing here: generic::filter_pixel_kernel filters it again and owns its status
    if constexpr (NW > 1) {
        if (__any(bad) && lane == 0) sBadFlag[0] = 1;
        __syncthreads();
        if (tid == 0) {
            bool redo = false;
            if constexpr (PHASE != 2) redo = reinterpret_cast<const int *>(sHXf + kNDim)[0] != 0;
            if (redo) {
                p.redo_list[atomicAdd(p.redo_count, 1u)] = (uint32_t)pix;
            } else if (sBadFlag[0]) {
                atomicAdd(&p.status[0], 1);
                atomicMin(&p.status[1], (int)pix);
            }
        }
    } else {
        const bool anybad = __any(bad);
        if (lane == 0) {
            if (reinterpret_cast<const int *>(sHXf + kNDim)[0] != 0) {
                p.redo_list[atomicAdd(p.redo_count, 1u)] = (uint32_t)pix;
            } else if (anybad) {
                atomicAdd(&p.status[0], 1);
                atomicMin(&p.status[1], (int)pix);
            }
        }
    }
}

#if (RPF_IMPL_PART == 1 || RPF_IMPL_PART == 4) && !RPF_IMPL_SCHED && !RPF_IMPL_LISTED
// ---- neighbourhood-size binning -----------------------------------------------------------------------------------
// The cost and the LDS footprint of a pixel are set by its neighbourhood size N, and N is data dependent: box*box*S is
// only its ceiling (path-traced buffers keep little more than the S own samples, SURVEY F10).  When the ceiling is above
// what the one-wave kernels hold, N is counted first (stage 1b's test without the list), the pixels are dealt into one
// list per kernel family, and every family filters its own list with LDS sized for ITS capacity.
// Stage 1b's test for ONE pixel by one wave that has 2 KiB of LDS to itself (sQ: 1024 u16, sMW: 16 u64): N and the acceptance
// masks, in two phases.  A: every candidate of a 1024-candidate chunk of the window against the first kA features only; the
// survivors' candidate numbers are queued in order (ballot + prefix popcount).  B: the queue, 64 at a time, against the other
// features; a candidate that passes sets its bit of the acceptance mask (LDS atomic or).  Twelve gathers per candidate are
// what the one-pass test costs (39 GB through the L1s per 1080p x 8 spp frame, 6.2 ms); on a path-traced buffer few
// candidates outlive phase A, so most of those gathers are never issued (2.7 ms).  Every (candidate, feature) comparison is
// the one of the one-pass test in filter_pixel_kernel on the same operands (ops.h:101-104), and a candidate passes iff all
// of them do: same masks, same N.  Returns N.
// MEMBER (RPF_FLAG_MEMBER_TEST | RPF_FLAG_MEMBER_FUSED, route 10; DESIGN.md section 14e): the configured test of section 14a on
// mt = mult[RPF_MAX_NDIM] | floor[RPF_MAX_NDIM] (rpf_ctx::d_member).  lim_k = sd_k * mult_k (one rounding) and fl_k = sd_k > floor_k
// ? -inf : floor_k are pixel-uniform: formed once per pixel from the scalar-loaded statistics and the table at wave-uniform
// addresses, never per candidate; a candidate is rejected on k iff a >= lim_k && a > fl_k, and a comparison with a NaN is false.
// The test is a conjunction of per-feature tests, so phase A, which applies the first kA of them, rejects only what the whole
// conjunction rejects.  The flat proof is the 3-sigma one (sd_k == 0 gives lim_k == 0 for any finite positive multiple) and holds
// exactly where floor_k < 0: p.flat is one bit over all features, so the host hands it over only when every floor below n_feat is
// negative, and null otherwise.  The other instantiation is the code it was.
template <bool MEMBER = false>
__device__ __forceinline__ int membership_pixel_two_phase(const PassParams &p, int x, int y, int lane, uint16_t *sQ, unsigned long long *sMW,
                                                          [[maybe_unused]] const double *mt = nullptr) {
    constexpr int kA = 2, kChunk = 1024, kPF = 7;
    const int W = p.W, H = p.H, S = p.S, b = p.b;
    const uint64_t HW = (uint64_t)H * W, pix = (uint64_t)y * W + x;
    const int x0 = max(x - b, 0), x1 = min(x + b, W - 1);
    const int y0 = max(y - b, 0), y1 = min(y + b, H - 1);
    const int nyv = y1 - y0 + 1;
    const int centre_rank = (x - x0) * nyv + (y - y0);
    const int ncand = ((x1 - x0 + 1) * nyv - 1) * S;
    const uint32_t magic_S = div_magic((uint32_t)S), magic_ny = div_magic((uint32_t)nyv);
    if (p.flat != nullptr && p.flat[pix] != 0 && *p.nan_flag == 0) { // proven by stage 1a: the own samples only (wave-uniform)
        if (p.masks != nullptr)
            for (int w = lane; w < (ncand + kWave - 1) / kWave; w += kWave) p.masks[pix * p.mask_stride + (uint32_t)w] = 0ull;
        if (lane == 0) p.nbhd[pix] = S;
        return S;
    }
    double m12[kNFeat], lim12[kNFeat];
    [[maybe_unused]] double fl12[kNFeat];
#pragma unroll
    for (int k = 0; k < kNFeat; ++k) {
        m12[k] = p.pmean[(uint64_t)k * HW + pix];
        if constexpr (MEMBER) {
            const double sd = p.pstd[(uint64_t)k * HW + pix], fl = mt[RPF_MAX_NDIM + k];
            lim12[k] = sd * mt[k];
            fl12[k] = sd > fl ? -__builtin_inf() : fl;
        } else {
            lim12[k] = p.pstd[(uint64_t)k * HW + pix] * 3.0; // multiplyArray(std, 3), rpf.cpp:579
        }
    }
    auto cand_off = [&](int qq) -> uint32_t {
        int cell = (int)div_small((uint32_t)qq, magic_S); // (qq < 65536 * 64 / S ... the chunks keep n * d < 2^32: ncand * S < 2^32)
        const int s = qq - cell * S;
        if (cell >= centre_rank) ++cell;          // rpf.cpp:565
        const int ix = (int)div_small((uint32_t)cell, magic_ny), iy = cell - ix * nyv;
        return (uint32_t)(((uint64_t)(y0 + iy) * W + (x0 + ix)) * S + s);
    };
    int n = S;
#pragma unroll 1
    for (int c0 = 0; c0 < ncand; c0 += kChunk) {
        const int cend = min(c0 + kChunk, ncand);
        if (lane < kChunk / 64) sMW[lane] = 0ull;
        int qn = 0;
        float fa[kPF][kA];
        auto issueA = [&](int qb, float (&f)[kA]) {
            const int qq = qb + lane;
            if (qq < cend) {
                const uint32_t off = cand_off(qq);
#pragma unroll
                for (int k = 0; k < kA; ++k) f[k] = ldp(p, kColF + k, off);
            }
        };
#pragma unroll
        for (int u = 0; u < kPF; ++u) issueA(c0 + u * kWave, fa[u]);
#pragma unroll 1
        for (int q0 = c0; q0 < cend; q0 += kWave * kPF) {
#pragma unroll
            for (int u = 0; u < kPF; ++u) {
                const int qb = q0 + u * kWave;
                if (qb < cend) { // wave-uniform
                    bool surv = (qb + lane) < cend;
#pragma unroll
                    for (int k = 0; k < kA; ++k) {
                        const double a = fabs((double)fa[u][k] - m12[k]);
                        if constexpr (MEMBER) {
                            if (a >= lim12[k] && a > fl12[k]) surv = false;
                        } else {
                            if (a >= lim12[k]) surv = false;       // allLessThan (ops.h:101-104)
                        }
                    }
                    const unsigned long long m = __ballot(surv);
                    if (surv) sQ[qn + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)(qb + lane - c0);
                    qn += __popcll(m);
                    issueA(qb + kWave * kPF, fa[u]);
                }
            }
        }
        wsync();
#pragma unroll 1
        for (int q0 = 0; q0 < qn; q0 += kWave) {
            bool pass = q0 + lane < qn;
            const int ql = pass ? (int)sQ[q0 + lane] : 0;
            float fbv[kNFeat - kA];
            if (pass) {
                const uint32_t off = cand_off(c0 + ql);
#pragma unroll
                for (int k = kA; k < kNFeat; ++k) fbv[k - kA] = ldp(p, kColF + k, off);
            }
#pragma unroll
            for (int k = kA; k < kNFeat; ++k) {
                const double a = fabs((double)fbv[k - kA] - m12[k]);
                if constexpr (MEMBER) {
                    if (pass && a >= lim12[k] && a > fl12[k]) pass = false;
                } else {
                    if (pass && a >= lim12[k]) pass = false;
                }
            }
            if (pass) atomicOr(&sMW[ql >> 6], 1ull << (ql & 63));
            n += __popcll(__ballot(pass));
        }
        wsync();
        const int cw = (cend - c0 + 63) >> 6;
        if (p.masks != nullptr && lane < cw) p.masks[pix * p.mask_stride + (uint32_t)(c0 >> 6) + (uint32_t)lane] = sMW[lane];
        wsync();
    }
    if (lane == 0) p.nbhd[pix] = n;
    return n;
}

#endif // (RPF_IMPL_PART == 1 || RPF_IMPL_PART == 4) && !RPF_IMPL_SCHED && !RPF_IMPL_LISTED

#if RPF_IMPL_PART == 1 && !RPF_IMPL_SCHED && !RPF_IMPL_LISTED
// The pixels: every pixel of the slab (step 1, list null); the entries of `list` (its size read from *list_count: the
// pixels stage 1a could not prove flat, rpf_kernels.hip prelist_kernel); or (step > 1: the route probe of the unbinned pass,
// rpf_api.hip) the points of a lattice with that pitch, probe[0] += how many of them have N <= 64 without being proven flat,
// probe[1] += how many are proven flat.
__global__ __launch_bounds__(256) void nbhd_count_kernel(PassParams p, int step, uint32_t *probe, const uint32_t *list, const uint32_t *list_count) {
    __shared__ uint16_t sQ[4][1024];
    __shared__ unsigned long long sMW[4][16];
    const int lane = threadIdx.x & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // scalar: the pixel's
    const int64_t q = (int64_t)blockIdx.x * 4 + wv;                                                     // statistics load into SGPRs
    int xi, yi;
    if (list != nullptr) {
        if (q >= (int64_t)*list_count) return; // wave-uniform
        const uint32_t pp = list[q];
        yi = (int)(pp / (uint32_t)p.W);
        xi = (int)(pp - (uint32_t)yi * (uint32_t)p.W);
    } else if (step == 1) {
        // the fused kernels' pixel walk (slab_pixel: one band of rows per XCD, strips inside): a row-major walk of a 3840-wide
        // 32-spp slab re-fetched every window row from beyond the L2 (41 GB per launch)
        if (!slab_pixel(p, (int)(blockIdx.x & 7u), (int64_t)(blockIdx.x >> 3) * 4 + wv, xi, yi)) return; // wave-uniform
    } else {
        const int cols = (p.W + step - 1) / step, rows = (p.row_end - p.row_begin + step - 1) / step;
        if (q >= (int64_t)rows * cols) return; // wave-uniform
        // (lattice points sit in the middle of their cells: border pixels have clipped windows and say little about the frame)
        xi = min((int)(q % cols) * step + (step >> 1), p.W - 1);
        yi = p.row_begin + min((int)(q / cols) * step + (step >> 1), p.row_end - p.row_begin - 1);
    }
    const int n = membership_pixel_two_phase(p, xi, yi, lane, sQ[wv], sMW[wv]);
    if (probe != nullptr && lane == 0) {
        const bool flat = p.flat != nullptr && p.flat[(uint64_t)yi * p.W + xi] != 0 && *p.nan_flag == 0;
        if (flat) atomicAdd(probe + 1, 1u);
        else if (n <= 64) atomicAdd(probe, 1u);
    }
}

#endif // RPF_IMPL_PART == 1 && !RPF_IMPL_SCHED && !RPF_IMPL_LISTED

#if RPF_IMPL_PART == 4
// The count kernel of route 10: every pixel of the slab (the same walk, the same LDS) under the configured test on mt
__global__ __launch_bounds__(256) void nbhd_count_member_kernel(PassParams p, const double *mt) {
    __shared__ uint16_t sQ[4][1024];
    __shared__ unsigned long long sMW[4][16];
    const int lane = threadIdx.x & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int xi, yi;
    if (!slab_pixel(p, (int)(blockIdx.x & 7u), (int64_t)(blockIdx.x >> 3) * 4 + wv, xi, yi)) return; // wave-uniform
    (void)membership_pixel_two_phase<true>(p, xi, yi, lane, sQ[wv], sMW[wv], mt);
}

#endif // RPF_IMPL_PART == 4

// what every entry point asks first: is p a pass of this unit's layout and list source (pass_fits_unit), and of its schedule too (pass_fits_build)?  The
// table in rpf_kernels.hip picks a build by the same three facts, so a wrong cell is refused here, on the host, before a listed
// kernel is handed a mask pass or the reverse (either would follow a null pointer on the device)
inline bool pass_fits_unit(const PassParams &p) { return p.lay.is_ref19() == kRef19 && ((p.generic & kGenericSampledListed) != 0) == kListed; }
inline bool pass_fits_build(const PassParams &p) { return pass_fits_unit(p) && ((p.generic & kGenericScheduleFused) != 0) == kSched; }

#if RPF_IMPL_PART == 1
#include "rpf_packed_impl.inc"
#endif

template <int K, bool TL, bool FAST, int NW, int PHASE = 0>
hipError_t launch_filter_inst(const PassParams &p, const LdsLayout &L, unsigned grid, hipStream_t s) {
    hipError_t e = hipFuncSetAttribute((const void *)filter_pixel_kernel<K, TL, FAST, NW, PHASE>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.total);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((filter_pixel_kernel<K, TL, FAST, NW, PHASE>), dim3(grid), dim3(64 * NW), L.total, s, p, L);
    return hipGetLastError();
}
// the fp32 pair-weight variant (RPF_FLAG_FAST_WEIGHTS) is built for the reference layout only
template <int K, bool TL, int NW>
hipError_t launch_filter_w(const PassParams &p, const LdsLayout &L, unsigned grid, hipStream_t s) {
    if constexpr (kSched || kListed) { // the scheduled builds are fp64 only: check_schedule refuses gains with RPF_FLAG_FAST_WEIGHTS
        // (... and the listed ones: RPF_FLAG_FAST_WEIGHTS is refused on a sampled pass)
        return p.fast_weights ? hipErrorNotSupported : launch_filter_inst<K, TL, false, NW>(p, L, grid, s);
    } else if constexpr (kRef19) {
        if (p.fast_weights) return launch_filter_inst<K, TL, true, NW>(p, L, grid, s);
    } else {
        if (p.fast_weights) return hipErrorNotSupported;
    }
    return launch_filter_inst<K, TL, false, NW>(p, L, grid, s);
}
#if RPF_IMPL_SCHED
// PHASE 3 (chains) or PHASE 2 (weights) of the split route on the unscheduled part that holds class K's kernels: the entry points
// of parts 2 and 3 below in the enclosing namespace (the layout's, or its `listed`), where rpf_impl_unit.inc declares them
template <int K>
hipError_t unscheduled_phase(const PassParams &p, const LdsLayout &L, int phase, unsigned grid, hipStream_t s) {
    if constexpr (K == 25) return impl_filter_mid_phase(p, L, phase, grid, s);
    else return impl_filter_large_phase(p, L, phase, grid, s);
}
#endif
template <int K>
hipError_t launch_filter_k(const PassParams &p, const LdsLayout &L, const LdsLayout &L2, const LdsLayout &L3, bool t_in_lds,
                           unsigned grid, hipStream_t s) {
    if constexpr (K == 49 || K == 25) {
        // the split route of the 32- and 64-spp classes (see PHASE above): chains, then bins + MI + weights' coefficients,
        // then the weights (on two waves per pixel where two sweeps cover the own samples)
        if (L.nw == 4 && L2.total != 0 && L3.total != 0 && p.carry != nullptr && (kListed || p.masks != nullptr) && !p.fast_weights) {
            // (eight waves per pixel -- six producers, in case the chain waves were waiting for gathers -- measured SLOWER: 3840x270x32
            // chains 37.9 -> 50.6 ms; the kernel is bound by its dependent fp64 additions, not by the gathers)
#if RPF_IMPL_SCHED
            // PHASE 3 and PHASE 2 hold no stage 3c: the unscheduled part's kernels run around the scheduled PHASE 4
            hipError_t e = unscheduled_phase<K>(p, L3, 3, grid, s);
            if (e != hipSuccess) return e;
            e = t_in_lds ? launch_filter_inst<K, true, false, 4, 4>(p, L, grid, s) : launch_filter_inst<K, false, false, 4, 4>(p, L, grid, s);
            if (e != hipSuccess) return e;
            return unscheduled_phase<K>(p, L2, 2, grid, s);
#else
            hipError_t e = launch_filter_inst<K, false, false, 4, 3>(p, L3, grid, s);
            if (e != hipSuccess) return e;
            e = t_in_lds ? launch_filter_inst<K, true, false, 4, 4>(p, L, grid, s) : launch_filter_inst<K, false, false, 4, 4>(p, L, grid, s);
            if (e != hipSuccess) return e;
            return L2.nw == 2 ? launch_filter_inst<K, false, false, 2, 2>(p, L2, grid, s) : launch_filter_inst<K, false, false, 4, 2>(p, L2, grid, s);
#endif
        }
    }
    if constexpr (K >= 13) {
        if (L.nw == 4)
            return t_in_lds ? launch_filter_w<K, true, 4>(p, L, grid, s) : launch_filter_w<K, false, 4>(p, L, grid, s);
    }
    return t_in_lds ? launch_filter_w<K, true, 1>(p, L, grid, s) : launch_filter_w<K, false, 1>(p, L, grid, s);
}

// entry points of this layout, build and part (rpf_kernels.hip calls them through its table of builds); they carry the same
// names in every build's namespace.  A scheduled or listed build of part 1 emits the filter entries alone
#if RPF_IMPL_PART == 1
hipError_t impl_filter_small(const PassParams &p, const LdsLayout &L, bool t_in_lds, unsigned grid, hipStream_t s) {
    if (!pass_fits_build(p)) return hipErrorInvalidValue;
    const LdsLayout none{};
    switch (samples_per_lane(p.nmax)) {
    case 1: return launch_filter_k<1>(p, L, none, none, t_in_lds, grid, s);
    case 2: return launch_filter_k<2>(p, L, none, none, t_in_lds, grid, s);
    case 4: return launch_filter_k<4>(p, L, none, none, t_in_lds, grid, s);
    case 7: return launch_filter_k<7>(p, L, none, none, t_in_lds, grid, s);
    default: return hipErrorInvalidValue;
    }
}
#if !RPF_IMPL_SCHED && !RPF_IMPL_LISTED
hipError_t impl_pixel_stats(const PassParams &p, uint64_t pix0, uint64_t pix1, hipStream_t s) {
    if (p.S >= 16 && p.S <= 128 && pix1 > pix0) { // (below 16 spp neighbouring threads share their cache lines: the plain kernel reads at full rate)
        const int PB = p.S <= 32 ? 256 : (p.S <= 64 ? 128 : 64);
        const size_t lds = (size_t)PB * (p.S + 1) * sizeof(float);
        hipError_t e = hipFuncSetAttribute((const void *)pixel_stats_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(pixel_stats_tile_kernel, dim3((unsigned)((pix1 - pix0 + PB - 1) / PB)), dim3(256), lds, s, p, pix0, pix1, PB);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(pixel_stats_kernel, dim3((unsigned)((pix1 - pix0 + 255) / 256)), dim3(256), 0, s, p, pix0, pix1);
    return hipGetLastError();
}
hipError_t impl_nbhd_count(const PassParams &p, int step, uint32_t *probe, const uint32_t *list, const uint32_t *list_count, uint32_t list_max, hipStream_t s) {
    const int64_t cols = (p.W + step - 1) / step, rows = (p.row_end - p.row_begin + step - 1) / step;
    const int64_t npx = list ? (int64_t)list_max : cols * rows;
    if (npx <= 0) return hipSuccess;
    unsigned grid = (unsigned)((npx + 3) / 4);
    if (!list && step == 1) grid = (unsigned)(8 * (((int64_t)((p.row_end - p.row_begin + 7) / 8) * p.W + 3) / 4)); // 8 XCD bands
    hipLaunchKernelGGL(nbhd_count_kernel, dim3(grid), dim3(256), 0, s, p, step, probe, list, list_count);
    return hipGetLastError();
}
#endif // !RPF_IMPL_SCHED && !RPF_IMPL_LISTED
#elif RPF_IMPL_PART == 2
hipError_t impl_filter_mid(const PassParams &p, const LdsLayout &L, const LdsLayout &L2, const LdsLayout &L3, bool t_in_lds, unsigned grid, hipStream_t s) {
    if (!pass_fits_build(p)) return hipErrorInvalidValue;
    switch (samples_per_lane(p.nmax)) {
    case 13: return launch_filter_k<13>(p, L, L2, L3, t_in_lds, grid, s);
    case 25: return launch_filter_k<25>(p, L, L2, L3, t_in_lds, grid, s);
    default: return hipErrorInvalidValue;
    }
}
#if !RPF_IMPL_SCHED
// one kernel of the split route alone, for the scheduled build of this part (RPF_IMPL_SCHED, which compiles PHASE 4 only): PHASE 3,
// the chains, on L = lds_layout_chains, or PHASE 2, the weights, on L = lds_layout_weights (two or four waves: L.nw)
hipError_t impl_filter_mid_phase(const PassParams &p, const LdsLayout &L, int phase, unsigned grid, hipStream_t s) {
    if (!pass_fits_unit(p)) return hipErrorInvalidValue; // (called from the scheduled units too)
    if (samples_per_lane(p.nmax) != 25 || (phase != 2 && phase != 3)) return hipErrorInvalidValue;
    if (phase == 3) return launch_filter_inst<25, false, false, 4, 3>(p, L, grid, s);
    return L.nw == 2 ? launch_filter_inst<25, false, false, 2, 2>(p, L, grid, s) : launch_filter_inst<25, false, false, 4, 2>(p, L, grid, s);
}
#endif
#elif RPF_IMPL_PART == 3
hipError_t impl_filter_large(const PassParams &p, const LdsLayout &L, const LdsLayout &L2, const LdsLayout &L3, bool t_in_lds, unsigned grid, hipStream_t s) {
    if (!pass_fits_build(p)) return hipErrorInvalidValue;
    if (samples_per_lane(p.nmax) != 49) return hipErrorInvalidValue;
    return launch_filter_k<49>(p, L, L2, L3, t_in_lds, grid, s);
}
#if !RPF_IMPL_SCHED
// (as impl_filter_mid_phase, for the K = 49 class)
hipError_t impl_filter_large_phase(const PassParams &p, const LdsLayout &L, int phase, unsigned grid, hipStream_t s) {
    if (!pass_fits_unit(p)) return hipErrorInvalidValue; // (called from the scheduled units too)
    if (samples_per_lane(p.nmax) != 49 || (phase != 2 && phase != 3)) return hipErrorInvalidValue;
    if (phase == 3) return launch_filter_inst<49, false, false, 4, 3>(p, L, grid, s);
    return L.nw == 2 ? launch_filter_inst<49, false, false, 2, 2>(p, L, grid, s) : launch_filter_inst<49, false, false, 4, 2>(p, L, grid, s);
}
#endif
#elif RPF_IMPL_PART == 4
hipError_t impl_nbhd_count_member(const PassParams &p, const double *mt, hipStream_t s) {
    if (p.row_end <= p.row_begin || mt == nullptr) return mt == nullptr ? hipErrorInvalidValue : hipSuccess;
    const unsigned grid = (unsigned)(8 * (((int64_t)((p.row_end - p.row_begin + 7) / 8) * p.W + 3) / 4)); // 8 XCD bands
    hipLaunchKernelGGL(nbhd_count_member_kernel, dim3(grid), dim3(256), 0, s, p, mt);
    return hipGetLastError();
}
#else
#error "RPF_IMPL_PART must be 1, 2, 3 or 4"
#endif
#if (RPF_IMPL_SCHED || RPF_IMPL_LISTED) && RPF_IMPL_PART == 4
#error "part 4 has no scheduled and no listed build: the count pass has no stage 3c and lists nothing"
#endif
