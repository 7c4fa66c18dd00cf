// rpf_internal.h -- shared between the kernel TUs (rpf_kernels.hip, rpf_film.hip, rpf_impl_*.hip) and the C-ABI TUs (rpf_api*.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rpf_hip.h"

namespace rpf {

constexpr int kWave = 64;

// Which sample-vector layout a call uses (rpf_desc n_random / n_feat / plane_dtype).  Columns: [0,2) pFilm | [2,5) colour
// | [5,5+nR) random parameters | [5+nR, 5+nR+nF) features (sd.h:62-94 is nR = 2, nF = 12).  Compiled (fused) kernels exist
// for the reference layout with fp32 planes and for BASELINE configs[4]'s 27 dims (nR = 4, nF = 18) with fp16 planes; the
// layout-generic kernels (rpf_generic.hip, RPF_FLAG_GENERIC) take any layout within generic_ok().
struct SampleLayout {
    int32_t nR = 2, nF = 12, f16 = 0;
    int ndim() const { return 5 + nR + nF; }
    int npair() const { return nF * (nR + 2) + 3 * (nR + 2 + nF); } // rpf.cpp:416-442 generalised
    int nwt() const { return 5 + nF; }                              // weighted columns of stage 4
    size_t plane_bytes() const { return f16 ? 2 : 4; }
    bool is_ref19() const { return nR == 2 && nF == 12 && !f16; }
    bool supported() const { return is_ref19() || (nR == 4 && nF == 18 && f16 == 1); }
    bool generic_ok() const { return nR >= 1 && nF >= 1 && ndim() <= RPF_MAX_NDIM && (f16 == 0 || f16 == 1); }
};
constexpr int kStageChunk = 64; // samples gathered per step of the in-order (reference-order) sums
constexpr int kStageHalf = 32;  // ... and staged through LDS this many at a time

// The bits of PassParams::generic (setup_pass writes them, route_pass and the routes read them; 0 = a pass on the compiled, fused
// kernels).  Two bits reach device-side decisions: kGenericOn (stage 1a's kernel) and kGenericSchedule (stage 3c of the layout-generic
// filter kernels, a wave-uniform branch); the two fast bits are host-side only: no kernel reads them, and PassParams::fast_weights
// stays 0.
enum GenericBits : int32_t {
    kGenericOn = 1,           // RPF_FLAG_GENERIC: stage 1a and the filter pass run on the layout-generic kernels (rpf_generic.hip)
    kGenericPacked = 2,       // RPF_FLAG_GENERIC_PACKED: small neighbourhoods on the packed generic kernels (rpf_generic_packed.hip)
    kGenericWave = 4,         // RPF_FLAG_GENERIC_WAVE: 64 < N <= 832 on the one-wave generic kernels (rpf_generic_wave.hip)
    kGenericWide = 8,         // a wide pass (RPF_FLAG_WIDE_NBHD and box*box*S > 65535, or option "wide" = 1): every pixel on
                              //   generic::filter_wide_kernel (rpf_generic_wide.hip), whatever the bits above say; stage 1a is not affected
    kGenericWideClasses = 16, // with kGenericWide, RPF_FLAG_WIDE_CLASSES and S <= 832: the wide pass is counted first and dealt by size
                              //   class (route_wide_classes); only N > 832 stays on the wide kernel
    kGenericClassFast = 32,   // RPF_FLAG_GENERIC_FAST: routes 4 and 5 launch the fp32-weight instantiations of their packed and
                              //   one-wave class kernels (class_fast below); their rest lists and route 7 do not read it
    kGenericStreamFast = 64,  // RPF_FLAG_STREAM_FAST on a pass that runs layout-generic kernels (kGenericOn or kGenericWide; never set on
                              //   a fused pass): route 3, the rest lists of routes 4 / 5, route 6 and every class and the rest list
                              //   of route 7 launch the fp32-weight instantiations (stream_fast below); redo launches never do
    kGenericSampled = 128,    // RPF_FLAG_SAMPLED_NBHD on a pass with draws > 0: route 8 whatever the bits above say (route_sampled; the
                              //   draws and the pass id are rpf_ctx::samp_now, which setup_pass fills); stage 1a is not affected
    kGenericMemberTest = 256, // RPF_FLAG_MEMBER_TEST: stage 1b under the configured multiples and floors (rpf_ctx::d_member, which
                              //   setup_pass uploads).  A full-box pass: route 9 whatever the bits above say (route_member_test); a
                              //   sampled pass stays route 8 and its count kernel runs the test; stage 1a is not affected
    kGenericSchedule = 512,   // RPF_FLAG_SCHEDULE on a pass whose entry has a gain other than 1 (setup_pass; never on a fused pass, which
                              //   check_schedule refuses or, under RPF_FLAG_SCHEDULE_FUSED, marks kGenericScheduleFused instead): stage 3c of the packed, one-wave, streaming and wide layout-generic kernels
                              //   forms alpha and beta from PassParams::gain_c / gain_f; selects no route
    kGenericMemberFused = 1024, // RPF_FLAG_MEMBER_FUSED on a full-box pass of a call under RPF_FLAG_MEMBER_TEST that the compiled kernels can
                              //   take (setup_pass: a compiled layout without RPF_FLAG_GENERIC, not wide, no kGenericSchedule): route 10
                              //   (route_member_fused), the size-binned route behind the count kernel's MEMBER form.
                              //   Host-side only: no kernel reads it, and the compiled kernels read no bit of `generic`
    kGenericScheduleFused = 2048, // RPF_FLAG_SCHEDULE_FUSED on a pass of the compiled kernels whose entry has a gain other than 1 (setup_pass:
                              //   no layout-generic bit, or route 10): the pass runs the scheduled builds of those kernels
                              //   (rpf_impl_*_sched_*.hip: launch_filter_pass and launch_filter_packed pick their table row by it), which form alpha
                              //   and beta from PassParams::gain_c / gain_f; its streaming class gets a copy of the params with
                              //   kGenericSchedule in its place (scheduled_stream).  Host-side only, selects no route
    kGenericSampledFused = 4096, // RPF_FLAG_SAMPLED_FUSED on a pass that carries kGenericSampled and that the compiled kernels can take
                              //   (setup_pass: a compiled layout without RPF_FLAG_GENERIC, not wide, S + draws <= kMaxResident, no
                              //   kGenericSchedule, option "sampled_fused_stride"): route 11 (route_sampled_fused),
                              //   the size-binned route's class kernels behind generic::sampled_count_mask_kernel.  generic_route looks at
                              //   it before kGenericSampled.  Host-side only: no kernel reads it
    kGenericSampledListed = 8192, // RPF_FLAG_SAMPLED_LISTED on a pass that carries kGenericSampled and that the listed builds of the compiled
                              //   kernels can take (setup_pass: a compiled layout without RPF_FLAG_GENERIC, S + draws <= kMaxResident, not
                              //   forced wide, no kGenericSchedule; with kGenericSampledFused possible too, option "sampled_listed_stride"
                              //   picks one): route 12 (route_sampled_listed), the size-binned route's class kernels
                              //   in their listed builds (rpf_impl_*_listed_*.hip: launch_filter_pass and launch_filter_packed pick their table row by
                              //   it) behind a count kernel that lists into the member pool.  Never together with kGenericSampledFused or
                              //   kGenericWide; generic_route looks at it before kGenericSampled.  Host-side only: no kernel reads it
    kGenericQuad = 16384,     // RPF_FLAG_GENERIC_QUAD (validate: only with kGenericOn | kGenericPacked | kGenericWave): 832 < N <= 3136 on
                              //   the four-wave generic kernels (rpf_generic_quad.hip): route 13 for a pass with S <= 3136 that is
                              //   neither sampled, member-test nor wide (generic_route looks at those first).  Host-side only
};
// what routes a pass: its bits without the one that only picks the build of the compiled kernels
inline int32_t route_bits(int32_t generic) { return generic & ~kGenericScheduleFused; }

// everything one pass needs, passed by value to the kernels
struct PassParams {
    int32_t W, H, S;
    int32_t row_begin, row_end;
    int32_t box, b;        // b = (box-1)/2, rpf.cpp:561
    int32_t beta_map, policy;
    int32_t fast_weights;  // RPF_FLAG_FAST_WEIGHTS: fp32 pair arithmetic in stage 4
    int32_t generic;       // GenericBits below: which layout-generic kernels the pass runs (0: the compiled, fused ones)
    int32_t stage_mask;    // diagnostics only (rpf_set_option "stage_mask"): bit0 stats chain, bit1 bins, bit2 MI, bit3 weights; -1 = all
    int32_t screen;        // far-pair screen of the four-wave kernels: 0 off, 1 on
    int32_t strip_w;       // pixels per XCD strip of the pixel walk (slab_pixel)
    int32_t nmax;          // box*box*S: capacity of a neighbourhood
    int32_t bmax;          // floor(sqrt(nmax)): max histogram bins per axis
    double eps, seed, sigma_p;
    uint64_t plane_stride; // H*W*S
    SampleLayout lay;
    const void *planes;    // ndim planes of fp32 (or fp16: lay.f16); the colour planes are only read to seed d_colour
    const double *col_in;  // 3 fp64 planes
    double *col_out;       // 3 fp64 planes
    const double *pmean;   // [12][H*W] stage 1a
    const double *pstd;    // [12][H*W]
    const uint64_t *tfix;  // round(k ln k * 2^44), k = 0..nmax
    const uint64_t *dfix;  // tfix[k+1] - tfix[k], k = 0..nmax-1
    int32_t *nbhd;         // [H*W] N per pixel (always written)
    double *carry;            // split route of the 32- / 64-spp classes: per-pixel statistics and weights between its three kernels (kCarryStride doubles per pixel), or null
    const uint32_t *pix_list; // size-binned launch: the pixels (y*W+x) this launch filters, or null = every pixel of the slab
    uint32_t list_count;
    uint64_t *masks;       // size-binned launch: acceptance masks of stage 1b, [H*W][mask_stride] (one per 64 candidates,
    uint32_t mask_stride;  //   written by nbhd_count_kernel, re-used by the filter kernels), or null
    // unbinned route (box*box*S <= 512): filter_pixel_kernel leaves the pixels whose neighbourhood turns out small (N <= 64) to
    // the packed kernels -- it writes its acceptance masks and N and exits; classify_kernel then deals those pixels into the
    // lane-class lists (one atomic per wave and class: a per-pixel append on one counter cost 11 ns per pixel, 22 ms a frame)
    uint64_t *reroute_masks;   // [H*W][mask_stride], or null = no re-routing
    // stage 1a's by-product: flat[pix] = 1 when some feature of the pixel has sigma == 0 and a FINITE mean -- the strict 3-sigma
    // test then rejects every finite candidate (|f - m| >= 0) and every infinite one (|+-inf - m| = inf >= 0), see
    // flat_quad_shortcut -- and *nan_flag != 0 when any feature mean of the buffer is NaN (a NaN sample makes its pixel's mean
    // NaN, and a NaN candidate is the one kind that would still pass).  flat && !*nan_flag proves N = S without touching a
    // sample.  (A mean of +-inf is not enough: EPS clamps its NaN sigma to 0, and a candidate at the same infinity gives
    // |inf - inf| = NaN, which never rejects, while its own pixel's mean is +-inf, not NaN.)
    uint8_t *flat;         // [H*W], or null
    int32_t *nan_flag;     // [1]
    uint32_t *redo_list;   // REF_ABORT: pixels whose MI stage met a table inside the rounding band at a non-power-of-two N are
    uint32_t *redo_count;  //   appended here and filtered again by generic::filter_pixel_kernel (reference expression); or null
    int32_t *status;       // [0] count of NaN pixels, [1] lowest bad pixel index (atomicMin)
    rpf_debug dbg;         // device pointers, any may be null
    // a wide pass dealt by size class (route 7): the packed and one-wave layout-generic kernels take a pixel's members behind
    // its own samples from members[member_base[pix] ..], N - S plane offsets in the reference's order (generic::wide_count_kernel
    // wrote them), instead of rebuilding them from `masks`; or null
    const uint32_t *members;
    const uint64_t *member_base; // [H*W]
    // RPF_FLAG_SCHEDULE (kGenericSchedule; read by no kernel without that bit): the gains of this pass's entry, g_c and g_f of
    // alpha_k = clamp0(1 - g_c * W_r^{c,k}), beta_k = clamp0(1 - g_f * W_r^{f,k}) * W_c^{f,k}.  Last: no other field moves
    double gain_c, gain_f;
};
// the kernel argument block: a field that moves or grows moves it under every kernel at once
static_assert(sizeof(PassParams) == 368 && offsetof(PassParams, generic) == 40 && offsetof(PassParams, gain_c) == 352, "PassParams is the kernel argument block");
// the two fp32 pair-weight selections: the class kernels of routes 4 / 5 | the streaming and wide kernels, and every kernel of a wide pass
inline bool class_fast(const PassParams &p) { return (p.generic & kGenericClassFast) != 0; }
inline bool stream_fast(const PassParams &p) { return (p.generic & kGenericStreamFast) != 0; }
// the params of the streaming class of a pass on the compiled kernels (generic::filter_pixel_kernel on routes 0 to 2, the wide
// kernel on route 10): a scheduled pass hands them kGenericSchedule, the one bit of `generic` those kernels read (stage 3c), for
// its host-side kGenericScheduleFused; the gains are in p already
inline PassParams scheduled_stream(const PassParams &p) {
    PassParams q = p;
    if (q.generic & kGenericScheduleFused) q.generic = (q.generic & ~kGenericScheduleFused) | kGenericSchedule;
    return q;
}

// Per-context tuning / diagnostic overrides (rpf_set_option).  Defaults = the library's own choices; nothing here is
// read from the environment.  stage_mask != -1 skips stages (timing ablation: results are wrong) and is reported in
// rpf_counters.options_active.
struct Tuning {
    int32_t waves_per_pixel = 0; // 0 auto, 1 or 4
    int32_t table_in_lds = -1;   // -1 auto, 0 / 1
    int32_t lds_pad = 0;         // extra LDS bytes per workgroup (occupancy experiments)
    int32_t binning = -1;        // -1 auto (box*box*S > 512), 0 / 1
    int32_t stage_mask = -1;     // bit0 stats chain, bit1 bins, bit2 MI, bit3 weights; -1 = all
    int32_t screen = 1;          // far-pair screen (stage 4, four-wave kernels): 0 off, 1 on; same results
    int32_t split_weights = -1;  // 32- / 64-spp classes as three kernels (chains; bins + MI; weights): -1 auto (on), 0 off, 1 on; same results
    int32_t split_chunk = 0;     // split route: run its three launches chunk by chunk over this many list entries (0 = the whole list at once); same results
    int32_t strip_w = 0;         // pixels per XCD strip of the pixel walk: 0 auto (by box and spp), else a multiple of 8; same results
    int32_t count_first = -1;    // box*box*S <= 512: stage 1b as its own launch ahead of the filter kernels (the small-N route): -1 auto (probe), 0 off, 1 on; same results
    int32_t wide = -1;           // RPF_FLAG_WIDE_NBHD: -1 auto (passes with box*box*S > 65535 on the wide kernel), 1 every pass of such a call (test hook)
    int32_t packed = -1;         // small neighbourhoods (N <= 64) on the packed kernels, several pixels per wave: -1 auto (on), 0 off, 1 on
    int32_t sampled_fused_stride = -1; // RPF_FLAG_SAMPLED_FUSED: the largest mask stride (u64 words per pixel, ceil((box*box - 1) * S / 64)) at which a sampled pass takes route 11: -1 no bound, else that many; a pass above it stays on route 8 (test hook)
    int32_t sampled_listed_stride = -1; // RPF_FLAG_SAMPLED_LISTED together with RPF_FLAG_SAMPLED_FUSED: the smallest mask stride from which a sampled pass that both routes can take runs on route 12: -1 auto (kSampledListedStride), else 0 .. 1025 (0: always route 12, 1025: never where route 11 applies); a pass route 11 cannot take is route 12's whatever it says
    int64_t wide_pool = -1;      // RPF_FLAG_WIDE_CLASSES: entries of the member pool at the first count launch: -1 auto (8 per pixel of the slab), else that many (test hook: a pool too small is grown to the exact size and the count launch repeated; same results)
    bool is_default() const { return waves_per_pixel == 0 && table_in_lds == -1 && lds_pad == 0 && binning == -1 && stage_mask == -1 && screen == 1 && strip_w == 0 && split_chunk == 0 && count_first == -1 && split_weights == -1 && packed == -1 && wide == -1 && wide_pool == -1 && sampled_fused_stride == -1 && sampled_listed_stride == -1; }
};
// what option "sampled_listed_stride" = -1 stands for: the smallest mask stride of the measured schedules from which route 12 beat
// route 11 on both frames by more than either side's spread (DESIGN.md section 13g has the table): box 17 x 32 spp; 1025 would say: at no stride
constexpr int32_t kSampledListedStride = 144;

struct LdsLayout {
    uint32_t off_T, off_stat, off_hx, off_pair, off_mi, off_own, off_off, off_union, off_hist, total;
    uint32_t hist_stride; // bytes of one wave's histogram buffer
    uint32_t nw;          // waves per pixel (1 or 4)
};
LdsLayout lds_layout(int S, int nmax, int bmax, bool t_in_lds, const Tuning &tun, const SampleLayout &lay);
LdsLayout lds_layout_weights(int S, int nmax, const SampleLayout &lay, int nw); // the weight kernel of the split route (32- / 64-spp classes)
LdsLayout lds_layout_chains(int S, int nmax, const SampleLayout &lay, int nw);  // ... and its chain kernel (4 or 8 waves per pixel)
constexpr int kCarryStride = 136; // doubles per pixel of PassParams::carry (>= kCarry of either layout)
int samples_per_lane(int nmax); // the K the filter kernel is instantiated with (0 = unsupported)
bool table_in_lds(int S, int nmax, int bmax, const Tuning &tun, const SampleLayout &lay);
int waves_per_pixel(int nmax, const Tuning &tun);

hipError_t launch_pixel_stats(const PassParams &p, hipStream_t s);
hipError_t launch_pixel_stats_rows(const PassParams &p, int r0, int r1, hipStream_t s);
hipError_t launch_filter_pass(const PassParams &p, const Tuning &tun, hipStream_t s, uint32_t *lds_bytes_out);
// neighbourhood-size binning (large box*box*S): count N per pixel, then deal the pixels into one list per kernel family
constexpr int kNumPacked = 4;       // lane classes of the packed kernels: N <= 8, 16, 32, 64 (8, 4, 2, 1 pixels per wave)
constexpr int kNumClasses = 11;     // four packed lane classes (one-wave K = 1 kernel when the packed route is off), six more
                                    // LDS-resident kernel families, the streaming kernel for larger neighbourhoods
constexpr int kMaxResident = 3136;  // largest neighbourhood the LDS-resident kernels hold (64 lanes x 49 samples)
constexpr int kMaxNbhd = 65535;     // the streaming kernel: 16-bit histogram cells, one-byte bin ids
int class_capacity(int c);          // 8, 16, 32, 64, 128, 256, 448, 832, 1600, 3136, 65535
// the packed kernels (rpf_packed_impl.inc): pixels of p.pix_list with N <= lanes_per_pixel; count_dev != null: the list size
// is read on the device and p.list_count is only its upper bound
hipError_t launch_filter_packed(const PassParams &p, int lanes_per_pixel, const uint32_t *count_dev, hipStream_t s);
// stage 1b's test (N and the acceptance masks): for every pixel of the slab (step 1, list null); for the entries of `list`
// (size on the device in *list_count, at most list_max: sizes the grid); or for the points of a lattice of pitch `step`, with
// probe[0] += how many of them have N <= 64 without being proven flat and probe[1] += how many are proven flat
hipError_t launch_nbhd_count(const PassParams &p, int step, uint32_t *probe, const uint32_t *list, const uint32_t *list_count,
                             uint32_t list_max, hipStream_t s);
// the same for route 10: every pixel of the slab under the configured test of RPF_FLAG_MEMBER_TEST (member: device,
// mult[RPF_MAX_NDIM] | floor[RPF_MAX_NDIM]); N into p.nbhd and the masks into p.masks, which must be given.  p.flat: null unless
// every floor below n_feat is negative (the flat proof is the 3-sigma test's)
hipError_t launch_nbhd_count_member(const PassParams &p, const double *member, hipStream_t s);
// max_class < kNumClasses: pixels of that class and above join the list of rest_class (-1: they are left out)
hipError_t launch_classify(const PassParams &p, uint32_t *lists /*[kNumClasses][H*W]*/, uint32_t *counts /*[kNumClasses], zeroed*/,
                           int max_class, int rest_class, hipStream_t s);
hipError_t launch_colour_from_planes(const void *planes, bool f16, double *colour, uint64_t plane_stride, hipStream_t s);
hipError_t launch_colour_from_planes_span(const void *planes, bool f16, double *colour, uint64_t plane_stride, uint64_t e0,
                                          uint64_t cnt, hipStream_t s);
hipError_t launch_copy_f64(const double *src, double *dst, uint64_t n, hipStream_t s);
hipError_t launch_copy_colour_span(const double *src, double *dst, uint64_t plane_stride, uint64_t e0, uint64_t cnt,
                                   hipStream_t s);
hipError_t launch_reduce_rows(const double *colour, const float *ray_weight, float *sample_rgb, float *pixel_rgb, int W,
                              int H, int S, int r0, int r1, hipStream_t s);
hipError_t launch_reduce(const double *colour, const float *ray_weight, float *sample_rgb, float *pixel_rgb, int W,
                         int H, int S, hipStream_t s);
// unbinned route: deals the pixels of the slab (slab_pixel order) into the list of those that need the fused kernel's own
// stage 1b; a proven flat pixel gets nbhd = S instead (the packed kernels take it from there)
hipError_t launch_prelist(const PassParams &p, uint32_t *list, uint32_t *count /* zeroed */, hipStream_t s);
hipError_t launch_nbhd_reduce(const int32_t *nbhd, int W, int row_begin, int row_end, unsigned long long *out2,
                              hipStream_t s);
hipError_t launch_feature_images(const float *planes, int W, int H, int S, double *out, unsigned long long *maxbits, hipStream_t s);
// the film step (rpf_film.hip): pbrt's FilmTile::AddSample for every sample, gathered per output pixel
struct FilmParams {
    int32_t W, H, S;
    int32_t sx0, sy0;          // raster coords of buffer pixel (0,0)
    int32_t px0, py0, px1, py1;
    int32_t hx, hy;            // window half-widths in pixels (rpf_api_film.hip film_window)
    float rx, ry, inv_rx, inv_ry; // Filter::radius, FilmTile::invFilterRadius (1 / r, formed on the host)
    float max_lum, scale;
    uint64_t plane_stride;     // H*W*S
};
// pFilm outside [q, q+1] (or NaN): *first_bad = min over such samples of ((x*H + y)*S + s), the reference's order
hipError_t launch_film_check(const FilmParams &f, const float *planes, unsigned long long *first_bad, hipStream_t s);
// per sample: d = pFilm - 0.5 (float2, [y][s][x]) and the clamped L * sampleWeight (3 planes [y][s][x])
hipError_t launch_film_stage(const FilmParams &f, const float *planes, const double *colour, const float *ray_weight,
                             float2 *d_stage, float *lw_stage, hipStream_t s);
// every output pixel: contribSum, filterWeightSum and WriteImage's value; any output may be null
hipError_t launch_film_splat(const FilmParams &f, const float *table, const float2 *d_stage, const float *lw_stage,
                             float *tile_rgb, float *tile_w, float *image_rgb, hipStream_t s);

// ---- the layout-generic kernels (rpf_generic.hip): nR / nF are run-time values of p.lay ------------------------------
// LDS carve-up of its filter kernel, a host-side function of the layout and the neighbourhood capacity only (byte offsets
// into the dynamic LDS block); resident: member list and bin ids live in LDS (off_list / off_bins), else in HBM slots
struct GenericCarve {
    uint32_t off_chunk, off_hist, off_red4, off_list, off_bins, total, resident;
    uint32_t hist_par, hist_words; // histograms in the hist region (4: one per wave, 1) and the 32-bit words of one
};
GenericCarve generic_carve(const SampleLayout &lay, int nmax, bool fast = false); // fast: the carve-up of a launch_filter(..., fast = true)
namespace generic {
hipError_t launch_pixel_stats(const PassParams &p, uint64_t pix0, uint64_t pix1, hipStream_t s);
// the streaming kernel: one launch filters rows [p.row_begin, p.row_end), or the pixels of p.pix_list when that is given
// (the last size class of the binned route; the redo list).  list / bins: global scratch of `slots` workgroups, [slots][nmax]
// u32 and [slots][ndim][nmax] u8 (needed when the carve-up is not resident); the grid is min(pixels, slots).
// count_dev != null: the size of p.pix_list is read from device memory (redo list: no host read-back), grid = slots.
// fast: stage 4 in the fp32 arithmetic of RPF_FLAG_STREAM_FAST (route 3 and the rest lists of routes 4 / 5 pass it; the redo
// list and the streaming class of the fused routes never do)
// listed: the rest launch of a sampled pass (route 8 under RPF_FLAG_SAMPLED_REST): stage 1b reads N from p.nbhd and the members
// behind the own samples from p.members / p.member_base, as the count kernel left them, instead of walking the box; p.pix_list is
// the rest list, p.nmax the listed capacity S + draws (it sizes the carve-up and the slots); fp64 only, never with count_dev
hipError_t launch_filter(const PassParams &p, void *list, void *bins, uint32_t slots, const uint32_t *count_dev, hipStream_t s,
                         bool fast = false, bool listed = false);
} // namespace generic

// ---- the packed layout-generic kernels (rpf_generic_packed.hip, RPF_FLAG_GENERIC_PACKED): N <= 64, several pixels per wave --
// LDS carve-up of generic::filter_packed_kernel, a host-side function of the layout only.  The workgroup holds T[0 .. 64] and
// the columns of every MI pair (off_pairtab), then `waves` independent per-wave blocks of wave_bytes each; the off_* below
// are byte offsets from a wave's block, sized for the eight pixels a wave holds at G = 8:
//   staged samples [8 G-lane groups][ndim][G] fp64 at 0 (64 ndim doubles whatever G is), stat [8][ndim][5] fp64 (M, SD, lo,
//   range, flags), mask [ndim][16] u64 (one bit mask per pixel, column and bin value), hx [8][ndim] u64, bins [64][ndim] bytes,
//   mi [8][npair] fp64, w [8][2 nF + 16] fp64 (D_r_fk | the nine colour sums | alpha, W_r_c | beta), flag [8] ints (redo)
// waves: as many of the four as fit 160 KiB.
struct GenericPackedCarve {
    uint32_t off_pairtab, table_bytes;
    uint32_t off_stat, off_mask, off_hx, off_bins, off_mi, off_w, off_flag, wave_bytes;
    uint32_t waves, total;
};
GenericPackedCarve generic_packed_carve(const SampleLayout &lay);
namespace generic {
// stage 1b's test for every pixel of rows [p.row_begin, p.row_end): N into p.nbhd, the acceptance masks into p.masks
// ([H*W][p.mask_stride] u64, bit q = candidate q in the reference's visiting order -- the numbering of the compiled
// nbhd_count_kernel)
hipError_t launch_nbhd_count(const PassParams &p, hipStream_t s);
// the pixels of p.pix_list (p.list_count of them, N <= lanes_per_pixel = 8, 16, 32 or 64) from p.nbhd and p.masks; under
// REF_ABORT p.redo_list / p.redo_count take the pixels that generic::filter_pixel_kernel must filter again.  fast: stage 4 in
// the fp32 arithmetic of RPF_FLAG_GENERIC_FAST (routes 4 and 5 pass it; nothing else of PassParams says so)
hipError_t launch_filter_packed(const PassParams &p, int lanes_per_pixel, hipStream_t s, bool fast = false);
} // namespace generic

// ---- the one-wave layout-generic kernels (rpf_generic_wave.hip, RPF_FLAG_GENERIC_WAVE): 64 < N <= 832, one wave per pixel --
// LDS carve-up of generic::filter_wave_kernel, a host-side function of the layout and the class capacity (128, 256, 448 or
// 832).  The workgroup holds T[0 .. capacity] and the columns of every MI pair (off_pairtab), then `waves` independent
// per-wave blocks of wave_bytes each; the off_* below are byte offsets from a wave's block:
//   member list [capacity] u32 at 0; one block shared by the staging chunk [ndim][65] fp64 of the in-order sums (stage 2),
//   the bin ids [ndim][capacity] bytes (stages 3a, 3b) and the own rows of a sweep of stage 4 (never live together:
//   off_chunk == off_bins); hist: four joint histograms of floor(sqrt(capacity))^2 16-bit cells (four tables are filled
//   together); stat (M | SD | min | max [4 ndim], lo | range | flags [3 ndim], sum T[hx] [ndim], pair sums / MI [npair],
//   D_r_fk | the nine colour sums | alpha | beta | W_r_c [2 nF + 20], all fp64), flag (redo)
// waves: of the one to four per workgroup that fit 160 KiB, the count that lets a CU hold the most waves (at most the eight
// its registers allow), the larger count on a tie; 0: none fits, which no layout within RPF_MAX_NDIM reaches.
struct GenericWaveCarve {
    uint32_t off_pairtab, table_bytes;
    uint32_t off_bins, off_hist, off_chunk, off_stat, off_flag, wave_bytes;
    uint32_t waves, total, capacity;
};
GenericWaveCarve generic_wave_carve(const SampleLayout &lay, int capacity);
namespace generic {
// the pixels of p.pix_list (p.list_count of them, 64 < N <= capacity = 128, 256, 448 or 832) from p.nbhd and p.masks; under
// REF_ABORT p.redo_list / p.redo_count take the pixels that generic::filter_pixel_kernel must filter again.  fast: as for
// launch_filter_packed
hipError_t launch_filter_wave(const PassParams &p, int capacity, hipStream_t s, bool fast = false);
} // namespace generic

// ---- the four-wave layout-generic kernels (rpf_generic_quad.hip, RPF_FLAG_GENERIC_QUAD): 832 < N <= 3136, four waves per pixel --
// LDS carve-up of generic::filter_quad_kernel, a host-side function of the layout and the class capacity (1600 or 3136); byte
// offsets into the workgroup's one block:
//   T[0 .. capacity] u64 at 0, the columns of every MI pair (off_pairtab), the member list [capacity] u32 (off_list); one block
//   (off_shared) shared by the word prefix of stage 1b, the staging chunk [ndim][129] fp64 of the in-order sums (stage 2), the bin
//   ids [ndim][capacity] bytes (stages 3a, 3b) and the own rows of a sweep of stage 4 (never live together); hist: per wave
//   `hists` histograms of hist_words 32-bit words each (floor(sqrt(capacity))^2 16-bit cells); stat (the fp64 block of
//   generic_f64_doubles); red: [4 waves][own samples of a sweep][4] fp64 partial sums of stage 4; flag (redo)
// hists: of 4, 2 and 1 the count that lets a CU hold the most workgroups within 160 KiB (at most what its registers allow: two
// at the four own samples per sweep of the class 1600, one at the eight of the class 3136), the larger on a tie; 0: the layout does not fit the capacity and route 13 does not offer it that class.
struct GenericQuadCarve {
    uint32_t off_pairtab, off_list, off_shared, off_hist, off_stat, off_red, off_flag;
    uint32_t hist_words, hists, total, capacity, workgroups_per_cu;
};
GenericQuadCarve generic_quad_carve(const SampleLayout &lay, int capacity);
namespace generic {
// the pixels of p.pix_list (p.list_count of them, N <= capacity = 1600 or 3136) from p.nbhd and p.masks; under REF_ABORT
// p.redo_list / p.redo_count take the pixels that generic::filter_pixel_kernel must filter again.  fp64 only
hipError_t launch_filter_quad(const PassParams &p, int capacity, hipStream_t s);
} // namespace generic

// ---- the wide layout-generic kernel (rpf_generic_wide.hip, RPF_FLAG_WIDE_NBHD): 65535 < box*box*S <= 262144 ----------------
constexpr int kMaxWideNbhd = 1 << 18; // B = floor(sqrt(N)) <= 512: a bin id fits 16 bits with room to spare
constexpr int kTFixExact = 48585;     // the last k at which round(k ln k * 2^44) is below 2^63 (PassParams::tfix is exact up to here)
constexpr int kTWideBits = 41;        // the wide table: round(k ln k * 2^41), below 2^63 up to k = 2^18
// LDS carve-up of generic::filter_wide_kernel, a host-side function of the layout and the neighbourhood capacity only.  The
// fp64 block and the chunk are generic_carve's, with marginals of 512 entries; member list and bin ids always live in HBM
// slots; `band_words` 32-bit cells of the joint histogram follow (a band of floor(band_words / B) rows of the B x B table of a
// pixel: the whole table where it fits, else whatever 160 KiB leave); red4 as in generic_carve.  total > 160 KiB: not even
// one row of the widest table fits (no layout within RPF_MAX_NDIM reaches that).
struct GenericWideCarve {
    uint32_t off_chunk, off_hist, off_red4, band_words, total;
};
GenericWideCarve generic_wide_carve(const SampleLayout &lay, int nmax, bool fast = false);
namespace generic {
// one launch filters rows [p.row_begin, p.row_end), or the pixels of p.pix_list when that is given (the rest class and the
// redo list of route 7).  list / bins: global scratch of `slots` workgroups, [slots][nmax] u32 and [slots][ndim][nmax] u16; the
// grid is min(pixels, slots).  table: round(k ln k * 2^table_bits), k = 0 .. p.nmax (p.tfix is not read).  count_dev != null:
// the size of p.pix_list is read from device memory (redo list: no host read-back), grid = slots.  fast: as for launch_filter
// (route 6 and the rest list of route 7 pass it, route 7's redo launch never does)
// member != null (RPF_FLAG_MEMBER_TEST, never with fast): device, mult[RPF_MAX_NDIM] | floor[RPF_MAX_NDIM]; stage 1b runs the
// two-compare test of DESIGN.md section 14 on them (the MEMBER instantiations; the others are the code they were)
hipError_t launch_filter_wide(const PassParams &p, void *list, void *bins, uint32_t slots, const uint64_t *table, int table_bits,
                              const uint32_t *count_dev, hipStream_t s, bool fast = false, const double *member = nullptr);
// The member pool of routes 7, 8 and 9, all in device memory: what a count kernel fills and the class kernels read back as
// PassParams::members / member_base.  The two count kernels take it as the first 32 bytes of their second argument
struct MemberPool {
    uint32_t *pool;              // [capacity] plane offsets of the listed members behind the own samples
    uint64_t capacity;
    uint64_t *base;              // [H*W] first pool entry of a pixel that lists members
    unsigned long long *cursor;  // [1] entries reserved so far
};
static_assert(sizeof(MemberPool) == 32 && offsetof(MemberPool, capacity) == 8 && offsetof(MemberPool, base) == 16 &&
                  offsetof(MemberPool, cursor) == 24, "the count kernels' argument offsets");
// the count pass of routes 7 and 9 (rpf_generic_wide_count.hip, S <= 832): for every pixel of rows [p.row_begin, p.row_end) N
// into p.nbhd -- 833 for any N > 832 -- and, for S < N <= 832, the N - S members behind the own samples into
// m.pool[m.base[pix] ..]; *m.cursor ends at the sum of those N - S, whether or not m.capacity entries held them (a pool too small
// loses writes only: the caller compares and repeats).  nan_flag: [1], scratch of the flat-pixel proof.  Reads stage 1a's planes
// of the rows the slab's windows reach.  member != null (route 9): as for launch_filter_wide; the flat-pixel proof then asks for
// a negative floor as well
hipError_t launch_wide_count(const PassParams &p, const MemberPool &m, int32_t *nan_flag, const double *member, hipStream_t s);
// the count pass of route 8 (rpf_generic_sampled_count.hip): sampled_count_kernel for S + draws <= 832, else
// sampled_count_block_kernel (S + draws <= RPF_SAMPLED_MAX; section 13e), with the same result.  For every pixel of rows
// [p.row_begin, p.row_end) the distinct draws of its key that pass the 3-sigma test, in ascending visiting order, into
// m.pool[m.base[pix] ..] and N = S + their number into p.nbhd; *m.cursor as launch_wide_count leaves it.  table: device, the
// box - 1 Gaussian thresholds of p.box; member != null (with RPF_FLAG_MEMBER_TEST): as for launch_filter_wide, the test of the draws
struct SampledCountArgs {
    const uint32_t *table;
    uint64_t seed;
    int32_t pass_id, row_origin, draws;
    const double *member = nullptr;
};
hipError_t launch_sampled_count(const PassParams &p, const SampledCountArgs &a, const MemberPool &m, hipStream_t s);
// the count pass of route 11 (rpf_generic_sampled_mask.hip), S + draws <= kMaxResident and box*box*S <=
// kMaxNbhd: the same draws under the same test, left as route 2's count pass leaves its result -- N = S + the accepted draws into
// p.nbhd and, for every pixel of rows [p.row_begin, p.row_end), the ceil(ncand / 64) acceptance words of its window into p.masks
// ([H*W][p.mask_stride] u64, which must be given: bit qq = candidate qq of the visiting order).  No pool, no cursor
hipError_t launch_sampled_count_mask(const PassParams &p, const SampledCountArgs &a, hipStream_t s);
// the count pass of route 12 for windows of box*box*S <= kMaxNbhd (rpf_generic_sampled_mask.hip), S + draws <=
// kMaxResident: the mask kernel's bitmap, draws, compaction and test, and launch_sampled_count's result -- the accepted plane offsets
// in ascending visiting order into m.pool[m.base[pix] ..] behind one cursor reservation per pixel with N > S, N into p.nbhd,
// *m.cursor (zeroed here) as launch_wide_count leaves it.  Reads neither p.masks nor p.mask_stride
hipError_t launch_sampled_count_list(const PassParams &p, const SampledCountArgs &a, const MemberPool &m, hipStream_t s);
} // namespace generic

// ---- the spike pass (rpf_spike.hip, RPF_FLAG_SPIKE_CLAMP) -----------------------------------------------
constexpr int kSpikeTileMaxS = 1024;       // above it 24 * S bytes per pixel leave no useful tile: one thread per pixel on global memory
constexpr int kSpikeLdsBudget = 64 * 1024; // LDS of one tile (one wavefront): two pixels at S = 1024, 64 pixels up to S = 41
// LDS image of the clamp kernel's tile, [3][tile][stride] doubles; tile == 0: the direct form (S > kSpikeTileMaxS)
struct SpikeCarve {
    uint32_t stride, tile, bytes;
};
SpikeCarve spike_carve(int S);
// rows [row_begin, row_end) of the three fp64 planes [3][H][W][S]: spikes replaced in place, e [(row_end-row_begin)*W][3] the
// per-pixel removed energy (every entry written), counts [3] += replaced samples, clamped pixels, skipped pixels
hipError_t launch_spike_clamp(double *colour, int W, int H, int S, int row_begin, int row_end, double t, double *e,
                              unsigned long long *counts, hipStream_t s);
// row_sums [rows][3] = the x chain over e [rows][W][3]
hipError_t launch_spike_row_sums(const double *e, int rows, int W, double *row_sums, hipStream_t s);
// c += delta[k] for every sample of rows [row_begin, row_end) of plane k
hipError_t launch_spike_add(double *colour, int W, int H, int S, int row_begin, int row_end, const double delta[3], hipStream_t s);

// ---- the per-pass activity report (rpf_report.hip, RPF_FLAG_PASS_REPORT) --------------------------------
constexpr int kReportTileMaxS = 512;        // above it 48 * S bytes per pixel leave no useful tile: one thread per pixel on global memory
constexpr int kReportLdsBudget = 64 * 1024; // LDS of one tile (one wavefront): 64 pixels up to S = 21, two at S = 512
constexpr int kReportPixelValues = 12;      // doubles of scratch per filtered pixel: m_k | i_k | pm_k | pi_k
// LDS image of the pixel kernel's tile, [6][tile][stride] doubles (a then b, three channels each); tile == 0: the direct form
struct ReportCarve {
    uint32_t stride, tile, bytes;
};
ReportCarve report_carve(int S);
struct ReportPlanes {
    const double *col_in, *col_out; // 3 fp64 planes [3][H][W][S] each
    const int32_t *nbhd;            // [H*W]
    const double *alpha, *beta, *wrc; // [H*W][3], [H*W][n_feat], [H*W]; any may be null
    int32_t n_feat;
};
// rows [row_begin, row_end): pix [(row_end-row_begin)*W][kReportPixelValues] scratch (every entry written), rows_out
// [row_end-row_begin] records (device; every field written).  class_cap: the eight class bounds (class_capacity(0 .. 7))
hipError_t launch_pass_report(const ReportPlanes &in, int W, int H, int S, int row_begin, int row_end, const int32_t class_cap[8],
                              double *pix, rpf_report_row *rows_out, hipStream_t s);

int max_lds_per_block();
hipError_t launch_udiv_selftest(uint64_t n, uint64_t seed, int mode, unsigned long long *d_mismatch, hipStream_t s);

} // namespace rpf
