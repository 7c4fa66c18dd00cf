// rpf_api.h -- host only: what the TUs of the C ABI share.  rpf_api.hip holds the context, validation, pass set-up and the
// two pass loops; rpf_api_routes.hip the pass router (route_pass); rpf_api_film.hip the film step's host half;
// rpf_api_multi.hip the one-process multi-GPU driver; rpf_api_spike.hip the spike pass; rpf_api_report.hip the per-pass report.
#pragma once
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "rpf_internal.h"

struct rpf_ctx;

namespace rpf {

int32_t fail(rpf_ctx *c, int32_t st, const std::string &msg); // records the message in the context, returns st

// A grow-only device allocation, pointer + capacity: the one place that allocates and frees HBM.  It frees itself with the
// context that holds it.
template <class T>
struct DevBuf {
    T *ptr = nullptr;
    size_t cap = 0; // the bytes last asked for
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    operator T *() const { return ptr; }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
    void swap(DevBuf &o) { std::swap(ptr, o.ptr); std::swap(cap, o.cap); }
    // keeps an allocation that is large enough; otherwise frees it and allocates anew (the contents are not carried over)
    int32_t ensure(rpf_ctx *ctx, size_t bytes) {
        if (bytes <= cap && ptr) return RPF_OK;
        release();
        hipError_t e = hipMalloc((void **)&ptr, bytes ? bytes : 16);
        if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? RPF_E_NOMEM : RPF_E_HIP,
                                         std::string("hipMalloc: ") + hipGetErrorString(e));
        cap = bytes;
        return RPF_OK;
    }
};

// Which kernel route a pass took: what rpf_query_route returns (include/rpf_hip.h documents the values)
enum Route : int {
    kRouteNone = -1,         // no pass yet
    kRouteFused = 0,         // filter_pixel_kernel runs stage 1b itself
    kRouteCountFirst = 1,    // stage 1b as its own launch ahead of the fused and packed kernels
    kRouteBinned = 2,        // size-binned (box*box*S > 512)
    kRouteGeneric = 3,       // the layout-generic filter kernel, one launch
    kRouteGenericPacked = 4, // ... with small neighbourhoods (N <= 64) on the packed layout-generic kernels
    kRouteGenericWave = 5,   // ... and 64 < N <= 832 on the one-wave layout-generic kernels
    kRouteWide = 6,          // the wide kernel, one launch
    kRouteWideClasses = 7,   // a wide pass counted first and dealt by size class
    kRouteSampled = 8,       // a sampled pass: the draws' count kernel, then the class kernels on its member lists
    kRouteMemberTest = 9,    // a full-box pass under RPF_FLAG_MEMBER_TEST: route 7's structure with the configured test
    kRouteMemberFused = 10,  // ... with RPF_FLAG_MEMBER_FUSED, on a compiled layout: route 2's structure behind the configured test
    kRouteSampledFused = 11, // a sampled pass under RPF_FLAG_SAMPLED_FUSED on a compiled layout: route 2's class kernels behind the draws' mask kernel
    kRouteSampledListed = 12, // ... under RPF_FLAG_SAMPLED_LISTED: the listed builds of route 2's class kernels behind a count kernel that lists into the member pool
    kRouteGenericQuad = 13,  // route 5 with 832 < N <= 3136 on the four-wave layout-generic kernels (RPF_FLAG_GENERIC_QUAD)
};

static_assert(sizeof(rpf_sampling) == 48 && offsetof(rpf_sampling, draws) == 16, "rpf_sampling is ABI");
static_assert(sizeof(rpf_membership) == 2 * RPF_MAX_NDIM * sizeof(double) && offsetof(rpf_membership, floor) == RPF_MAX_NDIM * sizeof(double),
              "rpf_membership is ABI, and the image of the device table: mult[RPF_MAX_NDIM] | floor[RPF_MAX_NDIM]");
static_assert(sizeof(rpf_schedule) == 8 + 3 * RPF_MAX_BOXES * sizeof(double) && offsetof(rpf_schedule, seed) == 8 &&
                  offsetof(rpf_schedule, gain_c) == 8 + RPF_MAX_BOXES * sizeof(double), "rpf_schedule is ABI");

// The redo counts of a pass under REF_ABORT: one per route_pass call, and rpf_filter's row-band pipeline cuts a pass into at most
// eight bands (run_host_pipeline)
constexpr int kRedoCounts = 8;

// The sampled pass in progress (RPF_FLAG_SAMPLED_NBHD; setup_pass fills it, route_sampled reads it): draws == 0, not sampled
struct SampledPass {
    int32_t draws = 0, pass_id = 0;
    int32_t max_draws = 0; // rpf_max_draws of the call's descriptor: 832 - S, or RPF_SAMPLED_MAX - S under RPF_FLAG_SAMPLED_REST
};

} // namespace rpf

struct rpf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // grow-only HBM workspace
    rpf::DevBuf<char> d_planes;                 // ndim planes of fp32 (or fp16)
    rpf::DevBuf<float> d_rayw;
    rpf::DevBuf<double> d_colA, d_colB;         // 3 planes fp64
    rpf::DevBuf<double> d_pmean, d_pstd;        // [12][H*W]
    rpf::DevBuf<int32_t> d_nbhd;
    rpf::DevBuf<uint64_t> d_tfix; int tfix_n = 0; // round(k ln k * 2^44), k = 0..n
    rpf::DevBuf<uint64_t> d_dfix;               // first differences
    rpf::DevBuf<uint64_t> d_twide; int twide_n = 0; // the wide kernel's table: round(k ln k * 2^41), k = 0..n (RPF_FLAG_WIDE_NBHD)
    rpf::DevBuf<float> d_srgb, d_prgb;
    rpf::DevBuf<double> d_carry;                // split route of the 32- / 64-spp classes: statistics / weights between its three kernels
    rpf::DevBuf<int32_t> d_status;              // [0] bad count [1] first bad
    rpf::DevBuf<unsigned long long> d_nred;     // [0] sum N [1] max N
    rpf::DevBuf<uint32_t> d_lists;              // size binning: [kNumClasses][H*W] pixel lists
    int last_route = rpf::kRouteNone;           // the rpf::Route of the last pass (rpf_query_route)
    rpf::DevBuf<uint32_t> d_class_counts;       // [kNumClasses] list sizes + [2] the route probe's counts
    rpf::DevBuf<uint64_t> d_masks;              // size binning: stage-1b acceptance masks [H*W][stride]
    rpf::DevBuf<char> d_big_list;               // streaming kernel: member lists [slots][nmax] u32
    rpf::DevBuf<char> d_big_bins;               //                   bin ids [slots][ndim][nmax] u8 (the wide kernel: u16)
    rpf::DevBuf<uint8_t> d_flat;                // stage 1a by-product: pixels with a zero-variance feature [H*W]
    rpf::DevBuf<int32_t> d_nan_flag;            // ... and whether any feature mean of the buffer is NaN
    rpf::DevBuf<uint32_t> d_redo_list;          // REF_ABORT: pixels handed to the reference-expression kernel [H*W]
    rpf::DevBuf<uint32_t> d_redo_count;         // [kRedoCounts] ... and how many: one count per route_pass call of a pass (per row band)
    // the rows the route probe of an unbinned pass reads (option "count_first" at -1), when they are not those of the route_pass call:
    // rpf_filter's row-band pipeline names the rows of the slab that are resident, so that a band is not judged by its own few rows
    // and the last band of a pass decides on the whole slab, as the serial call does.  Empty: the call's own rows (setup_pass)
    int probe_r0 = 0, probe_r1 = 0;
    int redo_used = 0;                          // the counts the pass in progress has taken (setup_pass: 0; begin_redo: the next)
    // a wide pass dealt by size class (RPF_FLAG_WIDE_CLASSES, route 7): what its count kernel leaves for the class kernels
    rpf::DevBuf<uint32_t> d_wc_pool;            // member pool: the N - S members behind the own samples of every pixel with N <= 832
    rpf::DevBuf<uint64_t> d_wc_base;            // [H*W] a pixel's first pool entry
    rpf::DevBuf<unsigned long long> d_wc_cursor; // [0] pool entries reserved, [1] (an int32) the NaN flag of the flat-pixel proof
    // membership depends on the features only, so within one call a pass with the same box and rows re-uses the
    // previous pass's masks and lists (reset at every API entry: the planes may change between calls)
    bool flat_fresh = false;                    // d_flat / d_nan_flag describe the planes of the call in progress (stage 1a ran in it)
    bool bin_valid = false;
    bool bin_member = false;                    // whose masks the cache holds: route 10's (the configured test) or route 2's (3 sigma)
    int bin_box = 0, bin_r0 = 0, bin_r1 = 0;
    uint32_t bin_counts[rpf::kNumClasses] = {};
    rpf::DevBuf<void> d_dbg[9];                 // debug planes
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // host-buffer entry (rpf_filter): row-band pipeline, uploads / downloads on their own streams
    hipStream_t s_up = nullptr, s_down = nullptr;
    std::vector<hipEvent_t> band_ev; // no-timing events, two per band
    rpf_counters counters{};
    rpf::Tuning tun;                      // rpf_set_option
    // the film step (rpf_filter_film / rpf_film_splat_device)
    rpf::DevBuf<float2> d_film_d;               // [H][S][W] pFilm - 0.5
    rpf::DevBuf<float> d_film_lw;               // 3 planes [H][S][W] clamped L * sampleWeight
    rpf::DevBuf<float> d_film_out;              // host entry: tile rgb | tile weight | image rgb
    rpf::DevBuf<float> d_film_table;            // [16*16]
    rpf::DevBuf<unsigned long long> d_film_bad; // first sample whose pFilm lies outside its pixel
    // the spike pass (RPF_FLAG_SPIKE_CLAMP; rpf_api_spike.hip)
    double spike_threshold = 1.0;               // rpf_set_spike
    int32_t spike_energy = 1;
    rpf_spike_stats spike{};                    // of the most recent call (begin_call zeroes it)
    rpf::DevBuf<double> d_spike_e;              // [rows][W][3] removed energy per pixel
    rpf::DevBuf<double> d_spike_rows;           // [rows][3] its row sums
    rpf::DevBuf<unsigned long long> d_spike_cnt; // [3] replaced samples, clamped pixels, skipped pixels
    // the per-pass activity report (RPF_FLAG_PASS_REPORT; rpf_api_report.hip): nothing here is allocated without the flag
    rpf_pass_report report[RPF_MAX_BOXES] = {}; // of the most recent call (begin_call clears them)
    std::vector<rpf_report_row> report_rows[RPF_MAX_BOXES]; // ... and the row records each entry was folded from
    rpf::DevBuf<double> d_rep_alpha, d_rep_beta, d_rep_wrc; // [H*W][3], [H*W][n_feat], [H*W]: where a reporting pass writes its weights
    rpf::DevBuf<double> d_rep_pix;              // [rows][W][12] the per-pixel values between the two report kernels
    rpf::DevBuf<rpf_report_row> d_rep_rows;     // [rows] the row records
    // sampled neighbourhoods (RPF_FLAG_SAMPLED_NBHD)
    rpf_sampling sampling{};                    // rpf_set_sampling
    bool sampling_set = false;
    rpf::SampledPass samp_now;                  // of the pass setup_pass prepared last
    rpf::DevBuf<uint32_t> d_samp_table; int samp_table_box = 0; // the Gaussian thresholds of that box (rpf_sampling_table)
    // the membership test (RPF_FLAG_MEMBER_TEST)
    rpf_membership membership{};                // rpf_set_membership
    bool membership_set = false;
    rpf::DevBuf<double> d_member; bool member_fresh = false; // its device image, which setup_pass uploads when it is stale
    // the per-pass schedule of the weight stage (RPF_FLAG_SCHEDULE): host only, setup_pass copies a pass's entry
    rpf_schedule schedule{};                    // rpf_set_schedule
    bool schedule_set = false;
};

namespace rpf {

// Per-stage tracing hooks (the reference brackets its phases with ProfilePhase, core/stats.h:254): roctx ranges around the
// host-side enqueue of upload / stage 1a / count + classify / each size-class launch / redo / reduce / download, visible in
// `rocprofv3 --marker-trace --kernel-trace`.  The marker library is looked up at run time (the profiler preloads it; without
// it, or without the library on the machine, the hooks are two null checks): librpf_hip.so has no link-time dependency on it.
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        for (const char *lib : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
            void *h = dlopen(lib, RTLD_LAZY | RTLD_GLOBAL);
            if (!h) continue;
            push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
            pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
            if (push && pop) return;
            push = nullptr; pop = nullptr;
        }
    }
};
inline const Roctx &roctx() { static const Roctx r; return r; }
struct Range {
    bool on;
    explicit Range(const char *name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
    ~Range() { if (on) roctx().pop(); }
    Range(const Range &) = delete;
    Range &operator=(const Range &) = delete;
};

// needs `ctx` in scope
#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return rpf::fail(ctx, RPF_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// floor(sqrt(nmax)), at least 1: the most histogram bins per axis a neighbourhood of that capacity can ask for
inline int bmax_of(int nmax) { return std::max(1, (int)std::sqrt((double)nmax)); }

// defined in rpf_api.hip, where each is described (route_pass: in rpf_api_routes.hip)
SampleLayout layout_of(const rpf_desc *d);
int32_t layout_kernels(const rpf_desc *d, int32_t *generic_out, std::string *why);
void wide_table(int nmax, uint64_t *out); // out[k] = round(k ln k * 2^kTWideBits), k = 0 .. nmax
void sampling_table(int box, uint32_t *out); // the box - 1 Gaussian thresholds of an odd box (rpf_sampling_table)
int32_t check_sampling(const rpf_sampling *cfg, std::string &why); // what rpf_set_sampling refuses
int32_t check_sampled(rpf_ctx *ctx, const rpf_desc *d, int n_pass); // RPF_FLAG_SAMPLED_NBHD of a call that runs n_pass passes
int32_t check_membership(const rpf_membership *cfg, std::string &why); // what rpf_set_membership refuses
int32_t check_member_test(rpf_ctx *ctx, const rpf_desc *d, int n_pass); // RPF_FLAG_MEMBER_TEST of a call that runs n_pass passes
int32_t check_schedule_table(const rpf_schedule *cfg, std::string &why); // what rpf_set_schedule refuses
// RPF_FLAG_SCHEDULE of a call that runs n_pass passes at boxes[0 .. n_pass)
int32_t check_schedule(rpf_ctx *ctx, const rpf_desc *d, const int32_t *boxes, int n_pass);
// the GenericBits of pass `pass` at `box` without kGenericSchedule (0: the fused kernels): what setup_pass and check_schedule share
int32_t pass_generic_bits(const rpf_ctx *ctx, const rpf_desc *d, int box, int pass);
int32_t validate(rpf_ctx *ctx, const rpf_desc *d, bool need_boxes);
int32_t enter(rpf_ctx *ctx, const rpf_desc *d, bool need_boxes); // validate, then make the context's device current

struct PassSetup {
    PassParams p;
    uint32_t lds = 0;
};
// pass: the index of the pass in its call (what RPF_FLAG_SAMPLED_NBHD reads draws[] and forms the pass id with)
int32_t setup_pass(rpf_ctx *ctx, const rpf_desc *d, int box, int pass, const void *d_planes, const double *col_in,
                   double *col_out, const rpf_debug *dbg_dev, PassSetup &out);
int32_t route_pass(rpf_ctx *ctx, const PassParams &p_in, hipStream_t s, int *launches);

int32_t begin_call(rpf_ctx *ctx, hipStream_t s);
std::string nonfinite_message(int x, int y, long long count);
int32_t finish_counters(rpf_ctx *ctx, const rpf_desc *d, int n_pass, hipStream_t s);
int32_t pass_through(rpf_ctx *ctx, const rpf_desc *d, const double *cin, double *cout, int r0, int r1, hipStream_t s);
int32_t ensure_frame(rpf_ctx *ctx, const rpf_desc *d, bool ray_weight, bool colour);
int32_t ensure_outputs(rpf_ctx *ctx, const rpf_desc *d, bool sample_rgb, bool pixel_rgb);
int32_t upload_frame(rpf_ctx *ctx, const rpf_desc *d, const void *planes, const float *ray_weight, bool colour,
                     const double *colour64, hipStream_t s);
int32_t download_rows(rpf_ctx *ctx, const rpf_desc *d, const double *colour, const float *d_ray_weight, int r0, int r1,
                      float *sample_rgb_out, float *pixel_rgb_out, size_t out_plane, int out_row, hipStream_t s,
                      hipStream_t to, hipEvent_t ready);
int32_t run_passes(rpf_ctx *ctx, const rpf_desc *d, const void *d_planes, double *d_colour, hipStream_t s);

// defined in rpf_api_film.hip, where each is described; the multi-GPU driver runs the same film step on every slab
int32_t film_geometry(const rpf_desc *d, const rpf_film *film, FilmParams &f, std::string &why);
int32_t film_ensure(rpf_ctx *ctx, const FilmParams &f);
constexpr unsigned long long kFilmNoOffender = ~0ull;
int32_t film_first_offender(rpf_ctx *ctx, const FilmParams &f, const float *d_planes, hipStream_t s, unsigned long long *key);
std::string film_offender_message(const FilmParams &f, int x, int y, int smp, float pfilm_x, float pfilm_y);
int32_t film_splat(rpf_ctx *ctx, const FilmParams &f, const rpf_film *film, const float *d_planes, const double *d_colour,
                   const float *d_ray_weight, float *d_tile_rgb, float *d_tile_w, float *d_image, hipStream_t s);

// defined in rpf_api_spike.hip, where each is described; the multi-GPU driver runs the two halves on every slab
int32_t spike_check_params(double threshold, int32_t preserve_energy, std::string &why);
int32_t spike_clamp(rpf_ctx *ctx, const rpf_desc *d, double *d_colour, double threshold, double *row_sums, rpf_spike_stats *stats,
                    hipStream_t s);
int32_t spike_add(rpf_ctx *ctx, const rpf_desc *d, double *d_colour, const double delta[3], hipStream_t s);
int32_t spike_pass(rpf_ctx *ctx, const rpf_desc *d, double *d_colour, hipStream_t s);

// defined in rpf_api_report.hip, where each is described; every pass loop runs report_planes before setup_pass and report_pass
// after route_pass, the multi-GPU driver folds the rows of every slab with rpf_pass_report_fold
void report_clear(rpf_ctx *ctx);
int32_t report_planes(rpf_ctx *ctx, const rpf_desc *d, rpf_debug &dev, hipStream_t s);
int32_t report_rows(rpf_ctx *ctx, const rpf_desc *d, const double *col_in, const double *col_out, const int32_t *nbhd,
                    const double *alpha, const double *beta, const double *wrc, rpf_report_row *rows_out, hipStream_t s);
int32_t report_pass(rpf_ctx *ctx, const rpf_desc *d, int pass, int box, const double *col_in, const double *col_out,
                    const rpf_debug &dev, hipStream_t s);

} // namespace rpf
