// rpf_generic_common.h -- what the layout-generic translation units share (rpf_generic.hip, rpf_generic_packed.hip,
// rpf_generic_wave.hip, rpf_generic_wide.hip, rpf_generic_wide_count.hip, rpf_generic_sampled_count.hip, rpf_generic_sampled_mask.hip;
// routes 3 to 9 and the count pass of route 11).  Only they include it.  Device
// code has internal linkage, like rpf_device_common.h: each TU carries its own copy.
//
// For every TU: the column counts of a layout (GenericDims), up16 and the size of the fp64 block of the LDS carve-ups (host side), the
// plane loaders, pair_cols and block_reduce.  Moving these here left the device assembly of every kernel as it was.
//
// For the packed kernels and the count kernels, whose stage bodies call them: the window of stage 1b and the decode of a
// candidate, the 3-sigma test of a wave, the column constants and the bin id, the zero band of stage 3b, the beta numerator, the
// debug hashes and the store of a filtered colour -- the statements the routes promise the same bits for.  For the two count
// kernels of the member pool (routes 7 to 9) alone: passes_stage1b_wave, the test their instantiation runs, publish_members, their
// common tail behind one cursor reservation (publish_members_block: its workgroup form), and dispatch_count_kernel, which picks the instantiation at the launch.
//
// filter_pixel_kernel, filter_wide_kernel and filter_wave_kernel spell the same statements inside their stage bodies and do not
// call these functions.  Two forms that do were built and held to the bars (profiles/generic_refactor_parent_vs_new.txt): (a)
// stage 3c and the streaming kernels' stages as __forceinline__ functions, (b) the stage bodies inline, calling the small functions
// and an offsets struct of the fp64 block.  Both: same bits, waves per SIMD kept, no scratch; both outside the parent's spread
// on scripts/generic_timing.py.  filter_pixel_kernel<float>, route-3 legs of the 1920x270x8 slabs: (a) +0.43 to +0.65 %, (b) +0.7 to
// +1.8 % (142.62 -> 143.60 ms, 189.84 -> 192.33 ms).  filter_wave_kernel, route-5 legs: (a) +0.2 to +0.8 %, (b) +0.2 to +1.7 %
// (fp16 planes 155.66 -> 157.56 ms, FAST 135.88 -> 138.22 ms).  filter_wide_kernel passed in form (b) (wide57 583.15 -> 580.22 ms,
// flat57 126.19 -> 126.19 ms) but shares its stage text with filter_pixel_kernel (rpf_generic_stream_stages.inc), which did not.
// So the three keep their bodies, with the parent's assembly byte for byte.
#pragma once
#include "rpf_device_common.h"

#ifndef RPF_GENERIC_OWN
#define RPF_GENERIC_OWN 4 // own samples per sweep of stage 4 (their accumulators are registers; same bits at any value)
#endif
// ... under RPF_FLAG_STREAM_FAST (a multiple of 4: two own samples share a packed fp32 instruction and the sweep's own rows, floats,
// are read 16 bytes at a time).  A member's columns are gathered and normalised once per sweep, so the wider sweep wins where N is
// large, which is what the flag is for; DESIGN.md section 11f has 8 against 16 and their registers
#ifndef RPF_STREAM_FAST_OWN
#define RPF_STREAM_FAST_OWN 16
#endif

namespace rpf {

// column counts of a layout, as the kernels and the host carve-ups use them
struct GenericDims {
    int nR, nF, ndim, nAnc, npairF, npairC, npair, nwt, colF;
};
__host__ __device__ inline GenericDims generic_dims(const SampleLayout &l) {
    GenericDims d;
    d.nR = l.nR; d.nF = l.nF; d.ndim = 5 + l.nR + l.nF;
    d.nAnc = l.nR + 2;                       // r.. and p.. anchors
    d.npairF = l.nF * d.nAnc;                // pairs (f_i, r_l | p_l)          rpf.cpp:416-427
    d.npairC = d.nAnc + l.nF;                // pairs of one colour channel     rpf.cpp:429-442
    d.npair = d.npairF + 3 * d.npairC;
    d.nwt = 5 + l.nF;                        // weighted columns of stage 4
    d.colF = 5 + l.nR;
    return d;
}

__host__ __device__ constexpr uint32_t up16(uint32_t v) { return (v + 15u) & ~15u; }

// Doubles in the fp64 block of the stream, wide and one-wave kernels, which their carve-ups size and the kernels walk in this order:
//   sStat M | SD | min | max [4 ndim], sZ lo | range | flags(sd0 | flat << 1) [3 ndim], sHX sum_i T[hx_i] [ndim],
//   sPair sum_ij T[J_ij] per pair, then the MI values [npair], sW Drf[nF] | D9[12] | alpha[4] | beta[nF] | wrc[4]
// (the streaming kernels keep 256 doubles of reduction scratch, sRedD, behind it)
inline uint32_t generic_f64_doubles(const GenericDims &D) { return (uint32_t)(8 * D.ndim + D.npair + 2 * D.nF + 20); }

namespace generic {
namespace {

constexpr int kThreads = 256, kChunk = 64; // the streaming kernels: threads of a workgroup, members staged per step of stage 2
constexpr int kOwn = RPF_GENERIC_OWN;      // ... and own samples per sweep of stage 4
constexpr int kStreamFastOwn = RPF_STREAM_FAST_OWN; // ... of the fp32 stage 4 (rpf_generic_stream_stages.inc part 4)
constexpr int kStreamGather = 4;           // ... whose feature columns are gathered this many at a time
static_assert(kStreamFastOwn % 4 == 0 && kStreamFastOwn >= 4, "the fp32 own rows of a sweep are read 16 bytes at a time");
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4a __attribute__((ext_vector_type(4), may_alias));

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
__device__ __forceinline__ void pair_cols(const GenericDims &D, int pr, int &ca, int &cb) {
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

// order-free reductions (min, max, integer sums) over a workgroup of 256; result in every thread.  sRed4: 4 slots
template <class V, class Op>
__device__ __forceinline__ V block_reduce(V v, V *sRed4, Op op) {
    for (int s = 32; s > 0; s >>= 1) v = op(v, __shfl_down(v, s, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sRed4[threadIdx.x >> 6] = v;
    __syncthreads();
    return op(op(sRed4[0], sRed4[1]), op(sRed4[2], sRed4[3]));
}

// ---- stage 1b: the window of pixel (x, y) and its candidates in the reference's visiting order (rpf.cpp:556-586) ---------
struct Window {
    int x0, y0, nyv, centre_rank, ncand;
};
__device__ __forceinline__ Window make_window(int x, int y, int b, int W, int H, int S) {
    const int x0 = max(x - b, 0), x1 = min(x + b, W - 1), y0 = max(y - b, 0), y1 = min(y + b, H - 1);
    const int nyv = y1 - y0 + 1;
    const int centre_rank = (x - x0) * nyv + (y - y0);
    const int ncand = ((x1 - x0 + 1) * nyv - 1) * S;
    return Window{x0, y0, nyv, centre_rank, ncand};
}
// plane offset of candidate qq < ncand
__device__ __forceinline__ uint32_t candidate_offset(const Window &w, int W, int S, int qq) {
    int cell = qq / S;
    const int s = qq - cell * S;
    if (cell >= w.centre_rank) ++cell;              // rpf.cpp:565: skip the centre pixel
    const int ix = cell / w.nyv, iy = cell - ix * w.nyv; // xn outer, yn inner ascending (rpf.cpp:562-563)
    return (uint32_t)(((uint64_t)(w.y0 + iy) * W + (w.x0 + ix)) * S + s);
}
// the strict 3-sigma test as the count kernels run it, a wave on 64 candidates of pixel `pix`: a rejected candidate stays
// rejected, so the later features are read only while some lane still passes
template <class T>
__device__ __forceinline__ bool passes_3sigma_wave(const PassParams &p, int colF, int nF, uint32_t off, uint64_t HW, uint64_t pix, bool pass) {
    for (int k = 0; k < nF; ++k) {
        if (!__any(pass)) break;
        const double m = p.pmean[(uint64_t)k * HW + pix];
        const double lim = p.pstd[(uint64_t)k * HW + pix] * 3.0;  // multiplyArray(std, 3), rpf.cpp:579
        if (pass) {
            const double a = fabs((double)ldp<T>(p, colF + k, off) - m);
            if (a >= lim) pass = false;           // allLessThan: fails iff a >= b (ops.h:101-104): a NaN never rejects
        }
    }
    return pass;
}

// The membership test of RPF_FLAG_MEMBER_TEST on the same terms: mt = mult[RPF_MAX_NDIM] |
// floor[RPF_MAX_NDIM].  lim and fl are wave-uniform, formed once per feature; a candidate is rejected on k iff a >= lim && a > fl,
// fl = -inf where the pixel's sigma is above the floor.  Every comparison with a NaN is false: a NaN never rejects.  With mult 3.0
// and a negative floor: lim has the bits of pstd * 3.0 above and a > fl holds wherever a >= lim does -- passes_3sigma_wave
template <class T>
__device__ __forceinline__ bool passes_member_wave(const PassParams &p, const double *mt, int colF, int nF, uint32_t off, uint64_t HW,
                                                   uint64_t pix, bool pass) {
    for (int k = 0; k < nF; ++k) {
        if (!__any(pass)) break;
        const double m = p.pmean[(uint64_t)k * HW + pix];
        const double sd = p.pstd[(uint64_t)k * HW + pix];
        const double lim = sd * mt[k];
        const double fl = sd > mt[RPF_MAX_NDIM + k] ? -__builtin_inf() : mt[RPF_MAX_NDIM + k];
        if (pass) {
            const double a = fabs((double)ldp<T>(p, colF + k, off) - m);
            if (a >= lim && a > fl) pass = false;
        }
    }
    return pass;
}
// stage 1b's test as an instantiation of a count kernel runs it: the configured test on mt (MEMBER), else the 3-sigma test
template <class T, bool MEMBER>
__device__ __forceinline__ bool passes_stage1b_wave(const PassParams &p, const double *mt, int colF, int nF, uint32_t off, uint64_t HW,
                                                    uint64_t pix, bool pass) {
    if constexpr (MEMBER) return passes_member_wave<T>(p, mt, colF, nF, off, HW, pix, pass);
    else return passes_3sigma_wave<T>(p, colF, nF, off, HW, pix, pass);
}

// The tail of a count kernel, a wave with acc > 0 accepted plane offsets staged in LDS: the wave reserves its entries with one
// atomic add on the cursor, records its base and copies the offsets where the pool holds them.  A pool too small loses the
// writes, never the reservation: the cursor ends at the sum of acc whatever the capacity was
__device__ __forceinline__ void publish_members(const MemberPool &m, uint64_t pix, const uint32_t *staged, int acc, int lane) {
    wsync(); // the staged offsets are read by other lanes than wrote them
    uint32_t lo = 0u, hi = 0u;
    if (lane == 0) {
        const unsigned long long at = atomicAdd(m.cursor, (unsigned long long)acc);
        m.base[pix] = at;
        lo = (uint32_t)at; hi = (uint32_t)(at >> 32);
    }
    const uint64_t at = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)hi) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
    if (at + (uint64_t)acc <= m.capacity)
        for (int j = lane; j < acc; j += 64) m.pool[at + j] = staged[j];
}

// The same tail for a workgroup of 256 threads that counted one pixel (sampled_count_block_kernel): acc > 0 offsets staged in LDS,
// acc workgroup-uniform; thread 0 reserves and hands the base to the others through sAt (LDS)
__device__ __forceinline__ void publish_members_block(const MemberPool &m, uint64_t pix, const uint32_t *staged, int acc, unsigned long long *sAt) {
    __syncthreads(); // the staged offsets are read by other threads than wrote them
    if (threadIdx.x == 0) {
        const unsigned long long at = atomicAdd(m.cursor, (unsigned long long)acc);
        m.base[pix] = at;
        *sAt = at;
    }
    __syncthreads();
    const uint64_t at = *sAt;
    if (at + (uint64_t)acc <= m.capacity)
        for (int j = threadIdx.x; j < acc; j += 256) m.pool[at + j] = staged[j];
}

// The launch of a count kernel: f(PlaneType<T>, std::bool_constant<MEMBER>) is called for the instantiation that p's planes
// (fp32 or fp16) and the presence of a membership table pick
template <class T>
struct PlaneType { using type = T; };
template <class F>
inline void dispatch_count_kernel(const PassParams &p, const double *member, F &&f) {
    if (member != nullptr) p.lay.f16 ? f(PlaneType<__half>{}, std::true_type{}) : f(PlaneType<float>{}, std::true_type{});
    else p.lay.f16 ? f(PlaneType<__half>{}, std::false_type{}) : f(PlaneType<float>{}, std::false_type{});
}

// ---- stage 2: the constants of a column from its in-order sums and its extrema (sd.h:229-232, mi.cpp:47-50) -----------
__device__ __forceinline__ void column_mean_sd(double sum, double sq, double dn, int policy, double &mean, double &sd) {
    mean = sum / dn;                                    // ops.h:123
    sd = sqrt(sq / dn - mean * mean);                   // ops.h:141
    if (policy == RPF_DEGEN_EPS && isnan(sd)) sd = 0.0;
}
// lo, range and the flags sd0 | flat << 1 of the binning
__device__ __forceinline__ void column_bin_range(double Mc, double SDc, double mn, double mx, double &lo, double &range, double &flags) {
    const bool sd0 = (SDc == 0.0);
    lo = sd0 ? 0.0 : (mn - Mc) / SDc;
    const double hi = sd0 ? 0.0 : (mx - Mc) / SDc;
    range = hi - lo;
    flags = (double)((sd0 ? 1 : 0) | (!(hi != lo) ? 2 : 0)); // mi.cpp:7 / 28 / 34
}
struct ColumnConst {
    double mean, sd, lo, range, flags;
};
__device__ __forceinline__ ColumnConst column_constants(double sum, double sq, double mn, double mx, double dn, int policy) {
    ColumnConst c;
    column_mean_sd(sum, sq, dn, policy, c.mean, c.sd);
    column_bin_range(c.mean, c.sd, mn, mx, c.lo, c.range, c.flags);
    return c;
}

// ---- stage 3a: the bin id of value v in a column with those constants, B bins ----------------------------------------------
__device__ __forceinline__ int bin_id(double v, double Mc, double SDc, double lo, double range, int flags, int B) {
    const bool sd0 = flags & 1, flat = flags & 2;
    int bin = 0;
    if (!flat) {
        const double a = v - Mc;                                   // subtractArrays
        const double z = sd0 ? 0.0 : a / SDc;                      // divideArrays, ops.h:48
        const double t = (z - lo) / range * (double)B;             // mi.cpp:14
        bin = max(min((int)t, B - 1), 0);
    }
    return bin;
}

// ---- stage 3b: MI of a pair from f = T[N] + sum T[J] - sum T[hx] - sum T[hy] in units of 2^-bits, with the zero band of the
// fixed-point sums (rpf_filter_impl.inc, filter_pixel_kernel).  inexact: the table is inside the band at a non-power-of-two N
// with non-degenerate marginals -- the reference's own value for it is rounding residue, not zero (REF_ABORT: the packed
// kernel puts the pixel on the redo list, and generic::filter_pixel_kernel evaluates the reference's expression)
__device__ __forceinline__ double zero_band_mi(int64_t f, int B, int n, uint64_t hxa, uint64_t hxb, uint64_t TN, int bits, double dn,
                                               bool &inexact) {
    const int64_t zero_band = ((int64_t)B * B + 2 * B + 1) / 2 + 1;
    inexact = false;
    if (f <= zero_band && f >= -zero_band) {
        inexact = (n & (n - 1)) != 0 && hxa != TN && hxb != TN;
        f = 0;
    }
    return ldexp((double)f, -bits) / dn;
}

// ---- stage 3c: the numerator of beta_k.  The presets keep the reference's stack rule for any nF: k < 3 reads D_f_ck (c = k on
// every lane whose beta is kept), a gap of zeros, then D_r_fk
__device__ __forceinline__ double beta_numerator(int beta_map, int k, int c, double Dcf, const double *sD9, const double *sDrf) {
    if (beta_map == RPF_BETA_PAPER) return Dcf;
    if (beta_map == RPF_BETA_REF_GCC11_O2) return k < 3 ? sD9[6 + c] : (k < 8 ? 0.0 : sDrf[max(k - 8, 0)]);
    return k < 3 ? sD9[6 + c] : (k < 4 ? 0.0 : sDrf[max(k - 4, 0)]);
}

// ---- stage 3c under RPF_FLAG_SCHEDULE (kGenericSchedule): schedule_factor, clamp0(1 - g * w), is in
// rpf_device_common.h -- the scheduled builds of the compiled kernels form alpha and beta with the same statement

// ---- debug outputs: FNV-1a of the member list in order (window coordinates of each member), and of a column's bin ids ------
__device__ __forceinline__ uint32_t member_hash(const uint32_t *list, int n, int x, int y, int b, int box, int S, int W) {
    uint32_t h = 2166136261u;
    for (int j = 0; j < n; ++j) {
        const uint32_t o = list[j], s = o % (uint32_t)S, q = o / (uint32_t)S;
        const int yn = (int)(q / (uint32_t)W), xn = (int)(q % (uint32_t)W);
        h = fnv1a_u32(h, (uint32_t)(((xn - x + b) * box + (yn - y + b)) * S) + s);
    }
    return h;
}
template <class Bin>
__device__ __forceinline__ uint32_t bin_hash(const Bin *bc, int n) {
    uint32_t h = 2166136261u;
    for (int j = 0; j < n; ++j) h = fnv1a_u16(h, bc[j]);
    return h;
}

// ---- stage 4: channel ch of own sample i of pixel pix = num / den (rpf.cpp:700); a NaN (rpf.cpp:702: the reference exits
// there) is reported by the return value and, under EPS, replaced by the input colour
__device__ __forceinline__ bool store_filtered(const PassParams &p, int ch, uint64_t pix, int S, int i, double num, double den) {
    double prime = num / den;
    const bool bad = isnan(prime);
    if (bad && p.policy == RPF_DEGEN_EPS) prime = p.col_in[(uint64_t)ch * p.plane_stride + pix * S + i];
    p.col_out[(uint64_t)ch * p.plane_stride + pix * S + i] = prime;
    return bad;
}

} // namespace
} // namespace generic
} // namespace rpf
