// rpf_api.hip -- the C ABI of include/rpf_hip.h: context, HBM workspace, pass sequencing, status and
// counters.  The pass loop mirrors RPFIntegrator::Render (rpf.cpp:767-775): for each box size run
// FillMeanAndStddev (stage 1a) then the fused filter; filtered colours replace the film's colours
// (rpf.cpp:732) and feed the next pass.  The pass router (route_pass) is rpf_api_routes.hip, the film step's host half
// rpf_api_film.hip, the one-process multi-GPU driver rpf_api_multi.hip; rpf_api.h is what they share.
#include <hip/hip_runtime.h>

#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "rpf_api.h"

using namespace rpf;

namespace rpf {

int32_t fail(rpf_ctx *c, int32_t st, const std::string &msg) {
    if (c) c->err = msg;
    return st;
}

// the sample-vector layout a descriptor names (0 in all three fields = the reference's 19 dims, fp32 planes)
SampleLayout layout_of(const rpf_desc *d) {
    SampleLayout l;
    if (d->n_random != 0 || d->n_feat != 0 || d->plane_dtype != 0) {
        l.nR = d->n_random ? d->n_random : 2;
        l.nF = d->n_feat ? d->n_feat : 12;
        l.f16 = d->plane_dtype == RPF_PLANES_F16 ? 1 : (d->plane_dtype == RPF_PLANES_F32 ? 0 : -1);
    }
    return l;
}

namespace {

// One refusal of layout_kernels: a descriptor with every flag of `when` is refused with `msg` unless it has all of `all_of`, one of
// `one_of` (0: nothing asked) and none of `none_of`.  The first failing row in this order answers.
struct FlagRule {
    uint32_t when, all_of, one_of, none_of;
    const char *msg;
};
constexpr uint32_t kPackedRoute = RPF_FLAG_GENERIC | RPF_FLAG_GENERIC_PACKED;
constexpr uint32_t kWaveRoute = kPackedRoute | RPF_FLAG_GENERIC_WAVE;
constexpr FlagRule kFlagRules[] = {
    {RPF_FLAG_GENERIC_QUAD, kWaveRoute, 0, 0, "RPF_FLAG_GENERIC_QUAD without RPF_FLAG_GENERIC | RPF_FLAG_GENERIC_PACKED | RPF_FLAG_GENERIC_WAVE: the flag modifies the one-wave layout-generic route"},
    {RPF_FLAG_GENERIC_QUAD, 0, 0, RPF_FLAG_FAST_WEIGHTS, "RPF_FLAG_FAST_WEIGHTS with RPF_FLAG_GENERIC_QUAD: the layout-generic kernels are fp64 throughout"},
    {RPF_FLAG_GENERIC_QUAD, 0, 0, RPF_FLAG_GENERIC_FAST, "RPF_FLAG_GENERIC_QUAD with RPF_FLAG_GENERIC_FAST: the four-wave layout-generic kernels are fp64 only, and a pixel would move from an fp32 launch to an fp64 class kernel"},
    {RPF_FLAG_GENERIC_QUAD, 0, 0, RPF_FLAG_STREAM_FAST, "RPF_FLAG_GENERIC_QUAD with RPF_FLAG_STREAM_FAST: the four-wave layout-generic kernels are fp64 only, and a pixel would move from an fp32 streaming launch to an fp64 class kernel"},
    {RPF_FLAG_SAMPLED_LISTED, RPF_FLAG_SAMPLED_NBHD, 0, 0, "RPF_FLAG_SAMPLED_LISTED without RPF_FLAG_SAMPLED_NBHD: the flag modifies the sampled route"},
    {RPF_FLAG_SAMPLED_FUSED, RPF_FLAG_SAMPLED_NBHD, 0, 0, "RPF_FLAG_SAMPLED_FUSED without RPF_FLAG_SAMPLED_NBHD: the flag modifies the sampled route"},
    {RPF_FLAG_SCHEDULE_FUSED, RPF_FLAG_SCHEDULE, 0, 0, "RPF_FLAG_SCHEDULE_FUSED without RPF_FLAG_SCHEDULE: the flag modifies the per-pass schedule"},
    {RPF_FLAG_MEMBER_FUSED, RPF_FLAG_MEMBER_TEST, 0, 0, "RPF_FLAG_MEMBER_FUSED without RPF_FLAG_MEMBER_TEST: the flag modifies the membership-test route"},
    {RPF_FLAG_MEMBER_TEST, 0, 0, RPF_FLAG_FAST_WEIGHTS, "RPF_FLAG_MEMBER_TEST with RPF_FLAG_FAST_WEIGHTS: passes under the membership test are fp64 throughout"},
    {RPF_FLAG_MEMBER_TEST, 0, 0, RPF_FLAG_GENERIC_FAST, "RPF_FLAG_MEMBER_TEST with RPF_FLAG_GENERIC_FAST: passes under the membership test are fp64 throughout"},
    {RPF_FLAG_MEMBER_TEST, 0, 0, RPF_FLAG_STREAM_FAST, "RPF_FLAG_MEMBER_TEST with RPF_FLAG_STREAM_FAST: passes under the membership test are fp64 throughout"},
    {RPF_FLAG_SAMPLED_NBHD, 0, 0, RPF_FLAG_FAST_WEIGHTS, "RPF_FLAG_SAMPLED_NBHD with RPF_FLAG_FAST_WEIGHTS: sampled passes are fp64 throughout"},
    {RPF_FLAG_SAMPLED_NBHD, 0, 0, RPF_FLAG_GENERIC_FAST, "RPF_FLAG_SAMPLED_NBHD with RPF_FLAG_GENERIC_FAST: sampled passes are fp64 throughout"},
    {RPF_FLAG_SAMPLED_NBHD, 0, 0, RPF_FLAG_STREAM_FAST, "RPF_FLAG_SAMPLED_NBHD with RPF_FLAG_STREAM_FAST: sampled passes are fp64 throughout"},
    {RPF_FLAG_SAMPLED_REST, RPF_FLAG_SAMPLED_NBHD, 0, 0, "RPF_FLAG_SAMPLED_REST without RPF_FLAG_SAMPLED_NBHD: the flag modifies the sampled route"},
    {RPF_FLAG_WIDE_CLASSES, RPF_FLAG_WIDE_NBHD, 0, 0, "RPF_FLAG_WIDE_CLASSES without RPF_FLAG_WIDE_NBHD: the flag modifies the wide route"},
    {RPF_FLAG_GENERIC_FAST, kPackedRoute, 0, 0, "RPF_FLAG_GENERIC_FAST without RPF_FLAG_GENERIC | RPF_FLAG_GENERIC_PACKED: the flag modifies the packed layout-generic route"},
    {RPF_FLAG_GENERIC_FAST, 0, 0, RPF_FLAG_FAST_WEIGHTS, "RPF_FLAG_GENERIC_FAST with RPF_FLAG_FAST_WEIGHTS: that flag selects the fused fp32 kernels of the 19-dim layout, this one the layout-generic ones"},
    {RPF_FLAG_GENERIC_FAST, 0, 0, RPF_FLAG_WIDE_NBHD, "RPF_FLAG_GENERIC_FAST with RPF_FLAG_WIDE_NBHD: wide passes are fp64 throughout"},
    {RPF_FLAG_STREAM_FAST, 0, RPF_FLAG_GENERIC | RPF_FLAG_WIDE_NBHD, 0, "RPF_FLAG_STREAM_FAST without RPF_FLAG_GENERIC or RPF_FLAG_WIDE_NBHD: the flag modifies the streaming and wide layout-generic kernels"},
    {RPF_FLAG_WIDE_NBHD, 0, 0, RPF_FLAG_FAST_WEIGHTS, "RPF_FLAG_FAST_WEIGHTS with RPF_FLAG_WIDE_NBHD: the wide layout-generic kernel is fp64 throughout"},
    {RPF_FLAG_GENERIC_WAVE, kPackedRoute, 0, 0, "RPF_FLAG_GENERIC_WAVE without RPF_FLAG_GENERIC | RPF_FLAG_GENERIC_PACKED: the flag modifies the packed layout-generic route"},
    {RPF_FLAG_GENERIC_WAVE, 0, 0, RPF_FLAG_FAST_WEIGHTS, "RPF_FLAG_FAST_WEIGHTS with RPF_FLAG_GENERIC_WAVE: the layout-generic kernels are fp64 throughout"},
    {RPF_FLAG_GENERIC_PACKED, RPF_FLAG_GENERIC, 0, 0, "RPF_FLAG_GENERIC_PACKED without RPF_FLAG_GENERIC: the flag modifies the layout-generic route"},
    {RPF_FLAG_GENERIC_PACKED, 0, 0, RPF_FLAG_FAST_WEIGHTS, "RPF_FLAG_FAST_WEIGHTS with RPF_FLAG_GENERIC_PACKED: the layout-generic kernels are fp64 throughout"},
    {RPF_FLAG_GENERIC, 0, 0, RPF_FLAG_FAST_WEIGHTS, "RPF_FLAG_FAST_WEIGHTS with RPF_FLAG_GENERIC: the layout-generic kernels are fp64 throughout"},
};

// ... and, for flags no row refuses, the layout against the kernels they select: the refusal's text, or null
const char *layout_refusal(const SampleLayout &lay, uint32_t flags) {
    if (flags & RPF_FLAG_GENERIC)
        return lay.generic_ok() ? nullptr
                                : "sample layout: the layout-generic kernels take n_random >= 1, n_feat >= 1, 5 + n_random + n_feat <= "
                                  "RPF_MAX_NDIM (40), fp32 or fp16 planes";
    if (!lay.supported())
        return "sample layout: kernels exist for n_random=2, n_feat=12, fp32 planes (the reference's 19 dims) and n_random=4, "
               "n_feat=18, fp16 planes (27 dims); any other layout needs RPF_FLAG_GENERIC (the layout-generic kernels)";
    // (launch_filter_w, rpf_filter_impl.inc: the FAST instantiations are built for the reference layout alone)
    if ((flags & RPF_FLAG_FAST_WEIGHTS) && !lay.is_ref19())
        return "RPF_FLAG_FAST_WEIGHTS: the fp32 pair-weight kernels exist for n_random=2, n_feat=12, fp32 planes (the reference's "
               "19 dims) only";
    return nullptr;
}

} // namespace

// Which kernels the filter entry points run for the layout and flags of d (rpf_layout_kernels; needs no device): RPF_OK with
// *generic_out = 0 (the compiled, fused kernels) or 1 (the layout-generic kernels: RPF_FLAG_GENERIC, and no other flag changes
// that answer), else the refusal and its text in *why -- the first failing row of kFlagRules, then the layout against the
// kernels the flags select.  RPF_FLAG_STREAM_FAST is refused only without either of RPF_FLAG_GENERIC and RPF_FLAG_WIDE_NBHD; with
// RPF_FLAG_FAST_WEIGHTS one of the older rows fires.  Both compiled layouts take RPF_FLAG_WIDE_NBHD as they are (the wide kernel is
// layout-generic).
int32_t layout_kernels(const rpf_desc *d, int32_t *generic_out, std::string *why) {
    if (!d) return RPF_E_BADARG;
    const SampleLayout lay = layout_of(d);
    const uint32_t flags = (uint32_t)d->flags;
    const int32_t generic = (flags & RPF_FLAG_GENERIC) ? 1 : 0;
    const char *msg = nullptr;
    for (const FlagRule &r : kFlagRules) {
        const bool refused = (flags & r.all_of) != r.all_of || (r.one_of && !(flags & r.one_of)) || (flags & r.none_of);
        if ((flags & r.when) == r.when && refused) { msg = r.msg; break; }
    }
    if (!msg) msg = layout_refusal(lay, flags);
    if (msg) {
        if (why) *why = msg;
        return RPF_E_UNSUPPORTED;
    }
    if (generic_out) *generic_out = generic;
    return RPF_OK;
}

// RPF_FLAG_SAMPLED_NBHD against the context's configuration, for a call that runs passes 0 .. n_pass - 1 of it (the entry points
// that filter: validate with the box list, rpf_filter_pass_debug with its one pass).  An entry point that runs no pass -- stage 1a,
// the colour / reduce / spike / film-window helpers -- accepts a descriptor with the flag as it accepts one without
int32_t check_sampled(rpf_ctx *ctx, const rpf_desc *d, int n_pass) {
    if (!(d->flags & RPF_FLAG_SAMPLED_NBHD)) return RPF_OK;
    if (!ctx->sampling_set) return fail(ctx, RPF_E_BADARG, "RPF_FLAG_SAMPLED_NBHD without a prior rpf_set_sampling");
    for (int i = 0; i < std::max(0, std::min(n_pass, RPF_MAX_BOXES)); ++i) {
        const int32_t D = ctx->sampling.draws[i];
        if (D < 0) return fail(ctx, RPF_E_BADARG, "rpf_sampling: a negative draw count");
        int32_t dmax = 0;
        (void)rpf_max_draws(d, &dmax); // (validate refused S <= 0)
        if (D > dmax)
            return fail(ctx, RPF_E_BADARG, (d->flags & RPF_FLAG_SAMPLED_REST)
                ? "RPF_FLAG_SAMPLED_NBHD | RPF_FLAG_SAMPLED_REST: S + draws > 8192 (RPF_SAMPLED_MAX: the count kernel sorts a pixel's draws in 32 KiB of LDS)"
                : "RPF_FLAG_SAMPLED_NBHD: S + draws > 832 (the largest size class of the one-wave kernels; RPF_FLAG_SAMPLED_REST "
                  "lifts the bound to 8192)");
        if (D > 0 && d->degenerate_policy == RPF_DEGEN_REF_ABORT)
            return fail(ctx, RPF_E_UNSUPPORTED, "a sampled pass under RPF_DEGEN_REF_ABORT: the reference has no sampled gather to reproduce, "
                                                "and the redo kernels run their own full-box stage 1b (use RPF_DEGEN_EPS)");
    }
    return RPF_OK;
}

// RPF_FLAG_MEMBER_TEST on the same terms, after check_sampled: the configuration, the policy, and S of every full-box pass -- one
// without draws of its own -- against the largest size class (a pixel's own samples are members of a class kernel's list)
int32_t check_member_test(rpf_ctx *ctx, const rpf_desc *d, int n_pass) {
    if (!(d->flags & RPF_FLAG_MEMBER_TEST)) return RPF_OK;
    if (!ctx->membership_set) return fail(ctx, RPF_E_BADARG, "RPF_FLAG_MEMBER_TEST without a prior rpf_set_membership");
    if (d->degenerate_policy == RPF_DEGEN_REF_ABORT)
        return fail(ctx, RPF_E_UNSUPPORTED, "RPF_FLAG_MEMBER_TEST under RPF_DEGEN_REF_ABORT: the reference has no such test to reproduce, and "
                                            "the redo kernels run their own stage 1b (use RPF_DEGEN_EPS)");
    const bool draws = (d->flags & RPF_FLAG_SAMPLED_NBHD) && ctx->sampling_set;
    for (int i = 0; i < std::max(0, std::min(n_pass, RPF_MAX_BOXES)); ++i)
        if (!(draws && ctx->sampling.draws[i] > 0) && d->S > 832)
            return fail(ctx, RPF_E_UNSUPPORTED, "RPF_FLAG_MEMBER_TEST: a full-box pass with S > 832 (the largest size class of the one-wave "
                                                "kernels; the count kernel deals every pixel by N >= S)");
    return RPF_OK;
}

// Which layout-generic kernels pass `pass` of a call under d runs at `box`: the GenericBits of PassParams::generic, all but
// kGenericSchedule (setup_pass adds that one from the table's entry); 0 = the compiled, fused kernels.  Reads the flags, S, option
// "wide" and the two configurations; setup_pass and check_schedule both ask here.
int32_t pass_generic_bits(const rpf_ctx *ctx, const rpf_desc *d, int box, int pass) {
    int32_t g = 0;
    if (d->flags & RPF_FLAG_GENERIC) {
        g = kGenericOn;
        if (d->flags & RPF_FLAG_GENERIC_PACKED) g |= kGenericPacked;
        if (d->flags & RPF_FLAG_GENERIC_WAVE) g |= kGenericWave;
        if (d->flags & RPF_FLAG_GENERIC_QUAD) g |= kGenericQuad; // (validate: only with all three above, never with an fp32 flag)
    }
    if (d->flags & RPF_FLAG_GENERIC_FAST) g |= kGenericClassFast; // (validate: only with G | P; read by routes 4 and 5, never by the fused code)
    // a wide pass: every pixel on generic::filter_wide_kernel (option "wide" = 1: every pass of a call with the flag)
    const bool wide = (d->flags & RPF_FLAG_WIDE_NBHD) && ((int64_t)box * box * d->S > kMaxNbhd || ctx->tun.wide == 1);
    if (wide) g |= kGenericWide;
    // ... counted first and dealt by size class under RPF_FLAG_WIDE_CLASSES (above 832 spp no class can hold a pixel)
    if (wide && (d->flags & RPF_FLAG_WIDE_CLASSES) && d->S <= 832) g |= kGenericWideClasses;
    // fp32 pair weights on the streaming / wide kernels: only a pass that runs layout-generic kernels carries the bit (a fused pass
    // of a WIDE_NBHD | STREAM_FAST call keeps generic == 0 and runs exactly as without the flag)
    if ((d->flags & RPF_FLAG_STREAM_FAST) && (g & (kGenericOn | kGenericWide))) g |= kGenericStreamFast;
    // a sampled pass: draws[pass] > 0; with 0 draws the pass carries no bit and runs as without the flag
    if ((d->flags & RPF_FLAG_SAMPLED_NBHD) && ctx->sampling_set && pass >= 0 && pass < RPF_MAX_BOXES && ctx->sampling.draws[pass] > 0)
        g |= kGenericSampled;
    // the membership test: every pass of the call carries the bit
    if ((d->flags & RPF_FLAG_MEMBER_TEST) && ctx->membership_set) g |= kGenericMemberTest;
    return g;
}

// RPF_FLAG_SCHEDULE on the terms of check_sampled, after it and check_member_test: the table, the entries passes 0 .. n_pass - 1
// read, and -- for a pass whose entry has a gain other than 1 -- the policy and that the pass runs layout-generic kernels or, under
// RPF_FLAG_SCHEDULE_FUSED, the scheduled fp64 builds of the compiled ones.  A pass with both gains 1 is any pass with another seed
// and is never refused here
int32_t check_schedule(rpf_ctx *ctx, const rpf_desc *d, const int32_t *boxes, int n_pass) {
    if (!(d->flags & RPF_FLAG_SCHEDULE)) return RPF_OK;
    if (!ctx->schedule_set) return fail(ctx, RPF_E_BADARG, "RPF_FLAG_SCHEDULE without a prior rpf_set_schedule");
    const rpf_schedule &sc = ctx->schedule;
    if (n_pass < 0 || (int64_t)sc.pass0 + n_pass > RPF_MAX_BOXES)
        return fail(ctx, RPF_E_BADARG, "RPF_FLAG_SCHEDULE: pass0 + the number of passes > RPF_MAX_BOXES (the call would read beyond entry 7 of rpf_schedule)");
    for (int i = 0; i < n_pass; ++i) {
        const int e = sc.pass0 + i;
        if (sc.gain_c[e] == 1.0 && sc.gain_f[e] == 1.0) continue;
        if (d->degenerate_policy == RPF_DEGEN_REF_ABORT)
            return fail(ctx, RPF_E_UNSUPPORTED, "RPF_FLAG_SCHEDULE: a pass with a gain other than 1 under RPF_DEGEN_REF_ABORT: the reference has no "
                                                "such rule to reproduce, and the redo launch would have to carry it (use RPF_DEGEN_EPS)");
        if (pass_generic_bits(ctx, d, boxes[i], i) == 0 && (d->flags & RPF_FLAG_SCHEDULE_FUSED)) {
            // RPF_FLAG_SCHEDULE_FUSED: the scheduled builds of the compiled kernels take the pass; they are fp64 only
            if (d->flags & RPF_FLAG_FAST_WEIGHTS)
                return fail(ctx, RPF_E_UNSUPPORTED, "RPF_FLAG_SCHEDULE_FUSED with RPF_FLAG_FAST_WEIGHTS: a pass with a gain other than 1 on the fused "
                                                    "kernels runs their scheduled builds, which are fp64 throughout");
            continue;
        }
        if (pass_generic_bits(ctx, d, boxes[i], i) == 0)
            return fail(ctx, RPF_E_UNSUPPORTED, "RPF_FLAG_SCHEDULE: a pass with a gain other than 1 would run on the fused kernels, which do not know "
                                                "the rule; a layout-generic route does: RPF_FLAG_GENERIC (| RPF_FLAG_GENERIC_PACKED | "
                                                "RPF_FLAG_GENERIC_WAVE), RPF_FLAG_WIDE_NBHD on a wide pass, RPF_FLAG_SAMPLED_NBHD with draws > 0 for "
                                                "the pass, or RPF_FLAG_MEMBER_TEST");
    }
    return RPF_OK;
}

int32_t validate(rpf_ctx *ctx, const rpf_desc *d, bool need_boxes) {
    if (!ctx) return RPF_E_BADARG;
    if (!d) return fail(ctx, RPF_E_BADARG, "desc is NULL");
    if (d->W <= 0 || d->H <= 0 || d->S <= 0) return fail(ctx, RPF_E_BADARG, "W, H, S must be positive");
    if (d->row_begin < 0 || d->row_end > d->H || d->row_begin > d->row_end)
        return fail(ctx, RPF_E_BADARG, "row range must satisfy 0 <= row_begin <= row_end <= H");
    if ((uint64_t)d->W * d->H * d->S >= (1ull << 32))
        return fail(ctx, RPF_E_BADARG, "W*H*S must be < 2^32 per slab (split the image into row slabs)");
    if (d->beta_map < 0 || d->beta_map > RPF_BETA_PAPER) return fail(ctx, RPF_E_BADARG, "unknown beta_map");
    {
        std::string why;
        const int32_t st = layout_kernels(d, nullptr, &why);
        if (st) return fail(ctx, st, why);
    }
    if (d->degenerate_policy < 0 || d->degenerate_policy > RPF_DEGEN_EPS)
        return fail(ctx, RPF_E_BADARG, "unknown degenerate_policy");
    // RPF_DEGEN_EPS adds eps to the three denominators of stage 3c: a zero (-0 adds what +0 adds), +inf and every positive value are IEEE arithmetic there, a
    // NaN or a negative one is a mistake.  RPF_DEGEN_REF_ABORT never reads the field
    if (d->degenerate_policy == RPF_DEGEN_EPS && (std::isnan(d->eps) || d->eps < 0.0))
        return fail(ctx, RPF_E_BADARG, "eps must be zero, positive or +inf under RPF_DEGEN_EPS (NaN or negative)");
    if (need_boxes) {
        int32_t st = check_sampled(ctx, d, d->n_box);
        if (st) return st;
        if ((st = check_member_test(ctx, d, d->n_box))) return st;
    }
    if (need_boxes) {
        if (d->n_box < 1 || d->n_box > RPF_MAX_BOXES) return fail(ctx, RPF_E_BADARG, "n_box must be 1..8");
        // The reference filters the WHOLE film in every pass (rpf.cpp:732 swaps the full film), so pass i+1 reads
        // filtered colours in every window row.  A strict sub-slab only filters its own rows: its halo rows would stay
        // unfiltered and the owned rows next to them would silently differ from the full-frame result.  Sub-slabs are
        // therefore driven one pass per call, with a colour-halo exchange in between (rpf_filter_multi does exactly
        // that inside one process; slabs.py across processes).
        if (d->n_box > 1 && (d->row_begin != 0 || d->row_end != d->H))
            return fail(ctx, RPF_E_BADARG, "n_box > 1 needs row_begin == 0 and row_end == H: a sub-slab must be filtered "
                                           "one pass per call with a colour-halo exchange in between (or rpf_filter_multi)");
        for (int i = 0; i < d->n_box; ++i)
            if (d->box_sizes[i] < 1 || (d->box_sizes[i] & 1) == 0)
                return fail(ctx, RPF_E_BADARG, "box sizes must be odd and positive (rpf.cpp:561)");
        const int32_t st = check_schedule(ctx, d, d->box_sizes, d->n_box);
        if (st) return st;
    }
    return RPF_OK;
}

// an entry point begins: the descriptor is refused before any device work, then the context's device is made current
int32_t enter(rpf_ctx *ctx, const rpf_desc *d, bool need_boxes) {
    const int32_t st = validate(ctx, d, need_boxes);
    if (st) return st;
    HIP_TRY(hipSetDevice(ctx->device));
    return RPF_OK;
}

// T_w[k] = k ln k in 2^-41 fixed point (computed in long double, rounded once): 2^18 ln 2^18 * 2^41 = 7.19e18 < 2^63, where
// the 2^-44 table of ensure_tables is 2^63 and more from k = 48586 on
void wide_table(int nmax, uint64_t *out) {
    out[0] = 0;
    for (int k = 1; k <= nmax; ++k) out[k] = (uint64_t)std::llroundl(std::ldexp((long double)k * std::log((long double)k), kTWideBits));
}

// The Gaussian threshold table of an odd box: out[k] = floor(2^32 * C_k / C_(box-1)), k = 0 .. box - 2,
// C_k = sum_{j <= k} exp(-(j - b)^2 / (2 sigma^2)), sigma = box / 4.0, in long double.  C_k < C_(box-1): every entry is below 2^32.
void sampling_table(int box, uint32_t *out) {
    const int b = (box - 1) / 2;
    const long double sigma = (long double)box / 4.0L;
    std::vector<long double> c((size_t)box);
    long double acc = 0.0L;
    for (int j = 0; j < box; ++j) {
        const long double dj = (long double)(j - b);
        acc += std::exp(-(dj * dj) / (2.0L * sigma * sigma));
        c[j] = acc;
    }
    for (int k = 0; k + 1 < box; ++k) out[k] = (uint32_t)std::floor(std::ldexp(c[k] / c[box - 1], 32));
}

int32_t check_sampling(const rpf_sampling *cfg, std::string &why) {
    if (!cfg) { why = "rpf_sampling is NULL"; return RPF_E_BADARG; }
    for (int i = 0; i < RPF_MAX_BOXES; ++i)
        if (cfg->draws[i] < 0) { why = "rpf_sampling: a negative draw count"; return RPF_E_BADARG; }
    return RPF_OK;
}

int32_t check_membership(const rpf_membership *cfg, std::string &why) {
    if (!cfg) { why = "rpf_membership is NULL"; return RPF_E_BADARG; }
    for (int k = 0; k < RPF_MAX_NDIM; ++k) {
        if (!(std::isfinite(cfg->mult[k]) && cfg->mult[k] > 0.0)) { why = "rpf_membership: a multiple that is not finite and > 0"; return RPF_E_BADARG; }
        if (std::isnan(cfg->floor[k]) || (std::isinf(cfg->floor[k]) && cfg->floor[k] > 0.0)) { why = "rpf_membership: a floor that is NaN or +inf"; return RPF_E_BADARG; }
    }
    return RPF_OK;
}

int32_t check_schedule_table(const rpf_schedule *cfg, std::string &why) {
    if (!cfg) { why = "rpf_schedule is NULL"; return RPF_E_BADARG; }
    if (cfg->pass0 < 0 || cfg->pass0 >= RPF_MAX_BOXES) { why = "rpf_schedule: pass0 outside [0, RPF_MAX_BOXES)"; return RPF_E_BADARG; }
    for (int e = 0; e < RPF_MAX_BOXES; ++e) {
        if (!(std::isfinite(cfg->seed[e]) && cfg->seed[e] > 0.0)) { why = "rpf_schedule: a seed that is not finite and > 0"; return RPF_E_BADARG; }
        if (!(std::isfinite(cfg->gain_c[e]) && cfg->gain_c[e] >= 0.0) || !(std::isfinite(cfg->gain_f[e]) && cfg->gain_f[e] >= 0.0)) {
            why = "rpf_schedule: a gain that is not finite and >= 0";
            return RPF_E_BADARG;
        }
    }
    return RPF_OK;
}

namespace {

// the multiples and floors of RPF_FLAG_MEMBER_TEST on the device: mult[RPF_MAX_NDIM] | floor[RPF_MAX_NDIM]
int32_t ensure_member_table(rpf_ctx *ctx) {
    if (ctx->d_member && ctx->member_fresh) return RPF_OK;
    int32_t st;
    ctx->member_fresh = false;
    if ((st = ctx->d_member.ensure(ctx, sizeof(rpf_membership)))) return st;
    HIP_TRY(hipMemcpy(ctx->d_member, &ctx->membership, sizeof(rpf_membership), hipMemcpyHostToDevice));
    ctx->member_fresh = true;
    return RPF_OK;
}

// the sampled count kernel's table of `box`, on the device
int32_t ensure_sampling_table(rpf_ctx *ctx, int box) {
    if (ctx->d_samp_table && ctx->samp_table_box == box) return RPF_OK;
    std::vector<uint32_t> t((size_t)std::max(box - 1, 1), 0u);
    sampling_table(box, t.data());
    int32_t st;
    ctx->samp_table_box = 0;
    if ((st = ctx->d_samp_table.ensure(ctx, t.size() * sizeof(uint32_t)))) return st;
    HIP_TRY(hipMemcpy(ctx->d_samp_table, t.data(), t.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    ctx->samp_table_box = box;
    return RPF_OK;
}

// T[k] = k ln k in 2^-44 fixed point (computed in long double, rounded once) and its first differences
int32_t ensure_tables(rpf_ctx *ctx, int nmax) {
    if (ctx->d_tfix && ctx->tfix_n >= nmax + 1) return RPF_OK;
    std::vector<uint64_t> t((size_t)nmax + 1), d((size_t)nmax + 1, 0);
    t[0] = 0;
    for (int k = 1; k <= nmax; ++k) t[k] = (uint64_t)std::llroundl(std::ldexp((long double)k * std::log((long double)k), 44));
    for (int k = 0; k < nmax; ++k) d[k] = t[k + 1] - t[k];
    int32_t st;
    if ((st = ctx->d_tfix.ensure(ctx, t.size() * sizeof(uint64_t)))) return st;
    if ((st = ctx->d_dfix.ensure(ctx, d.size() * sizeof(uint64_t)))) return st;
    HIP_TRY(hipMemcpy(ctx->d_tfix, t.data(), t.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx->d_dfix, d.data(), d.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    ctx->tfix_n = nmax + 1;
    return RPF_OK;
}

// the wide kernel's table (RPF_FLAG_WIDE_NBHD)
int32_t ensure_wide_table(rpf_ctx *ctx, int nmax) {
    if (ctx->d_twide && ctx->twide_n >= nmax + 1) return RPF_OK;
    std::vector<uint64_t> t((size_t)nmax + 1);
    wide_table(nmax, t.data());
    int32_t st;
    if ((st = ctx->d_twide.ensure(ctx, t.size() * sizeof(uint64_t)))) return st;
    HIP_TRY(hipMemcpy(ctx->d_twide, t.data(), t.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    ctx->twide_n = nmax + 1;
    return RPF_OK;
}

} // namespace

int32_t setup_pass(rpf_ctx *ctx, const rpf_desc *d, int box, int pass, const void *d_planes, const double *col_in,
                   double *col_out, const rpf_debug *dbg_dev, PassSetup &out) {
    if (box < 1 || (box & 1) == 0) return fail(ctx, RPF_E_BADARG, "box must be odd and positive");
    PassParams &p = out.p;
    std::memset(&p, 0, sizeof(p));
    p.W = d->W; p.H = d->H; p.S = d->S;
    p.lay = layout_of(d);
    const int kNFeat = p.lay.nF;
    p.row_begin = d->row_begin; p.row_end = d->row_end;
    p.box = box; p.b = (box - 1) / 2;
    p.beta_map = d->beta_map; p.policy = d->degenerate_policy;
    p.fast_weights = (d->flags & RPF_FLAG_FAST_WEIGHTS) ? 1 : 0;
    p.generic = pass_generic_bits(ctx, d, box, pass);
    p.stage_mask = ctx->tun.stage_mask; // timing ablation knob (rpf_set_option); results are wrong unless -1
    p.screen = ctx->tun.screen;
    const int64_t nmax64 = (int64_t)box * box * d->S;
    int32_t nbhd_cap = 0;
    (void)rpf_max_nbhd(d, &nbhd_cap);
    if (nmax64 > nbhd_cap)
        return fail(ctx, RPF_E_UNSUPPORTED, nbhd_cap == kMaxNbhd
            ? "box*box*S > 65535: neighbourhood too large (16-bit histogram cells, one-byte bin ids) without RPF_FLAG_WIDE_NBHD"
            : "box*box*S > 262144: neighbourhood too large for the wide kernel of RPF_FLAG_WIDE_NBHD (16-bit bin ids, B <= 512)");
    p.nmax = (int)nmax64;
    bool wide = (p.generic & kGenericWide) != 0; // (a route-12 pass drops the bit below)
    // a sampled pass (validate checked the configuration): draws[pass] > 0; with 0 draws the pass carries no bit and runs as without the flag
    ctx->samp_now = SampledPass{};
    ctx->probe_r0 = ctx->probe_r1 = 0; // ... and its route probe reads the rows of its route_pass calls unless the caller names others
    ctx->redo_used = 0; // a pass begins: its route_pass calls take the redo counts from the first on (begin_redo)
    if (p.generic & kGenericSampled) {
        ctx->samp_now.draws = ctx->sampling.draws[pass];
        ctx->samp_now.pass_id = (int32_t)((uint32_t)ctx->sampling.pass_id0 + (uint32_t)pass); // (mod 2^32: the key reads it as uint32)
        (void)rpf_max_draws(d, &ctx->samp_now.max_draws);
    }
    // the membership test (validate checked the configuration and refused every fp32 flag): every pass of the call carries the bit
    const bool member = (p.generic & kGenericMemberTest) != 0;
    // the fused kernels address a window's samples by 32-bit byte offsets from its first sample (Window, rpf_filter_impl.inc)
    if (rpf_check_window_span(d->W, d->S, box) != RPF_OK)
        return fail(ctx, RPF_E_UNSUPPORTED, "box*W*S*8 >= 2^32: a window's span in bytes of an fp64 plane must fit 32 bits (narrower slabs or a smaller box)");
    {   // XCD strip width: box rows x (strip + halo) px x S samples x ~88 B against a budget of L2 bytes.  Measured
        // (scripts/strip_sweep.sh, profiles/r02_strip_width.txt): the kernel time does not depend on it, the fetched bytes
        // do -- at 8 spp wide strips win (a quarter of the 4 MiB L2: 128 px), from 16 spp up narrow ones (the size-binned
        // route reads every window twice, count pass and filter pass, several hundred microseconds apart): 256 KiB.
        const int64_t per_px = (int64_t)box * d->S * 88;
        const int64_t budget = d->S > 8 ? (256 << 10) : (1 << 20);
        int w = (int)(budget / std::max<int64_t>(per_px, 1)) - 2 * ((box - 1) / 2);
        w = std::max(8, std::min(128, w));
        p.strip_w = w & ~7;
        if (ctx->tun.strip_w > 0) p.strip_w = ctx->tun.strip_w;
    }
    p.bmax = bmax_of(p.nmax);
    p.eps = d->eps; p.seed = d->sigma_seed;
    // the schedule (check_schedule checked the table, the entry's range, and that a pass with a gain other than 1 is layout-generic):
    // the entry's seed stands for the descriptor's; with both gains 1 the pass carries no bit and runs as without the flag
    if ((d->flags & RPF_FLAG_SCHEDULE) && ctx->schedule_set) {
        const int e = ctx->schedule.pass0 + pass;
        if (pass < 0 || e < 0 || e >= RPF_MAX_BOXES) return fail(ctx, RPF_E_BADARG, "RPF_FLAG_SCHEDULE: the pass reads beyond the table's last entry");
        p.seed = ctx->schedule.seed[e];
        if (ctx->schedule.gain_c[e] != 1.0 || ctx->schedule.gain_f[e] != 1.0) {
            // on the compiled kernels: only under RPF_FLAG_SCHEDULE_FUSED, on their scheduled, fp64 builds (the host-side bit; no
            // kernel of that family reads `generic`)
            if (!p.generic && (!(d->flags & RPF_FLAG_SCHEDULE_FUSED) || p.fast_weights))
                return fail(ctx, RPF_E_UNSUPPORTED, "RPF_FLAG_SCHEDULE: a pass with a gain other than 1 on the fused kernels");
            p.generic |= p.generic ? kGenericSchedule : kGenericScheduleFused;
            p.gain_c = ctx->schedule.gain_c[e]; p.gain_f = ctx->schedule.gain_f[e];
        }
    }
    // RPF_FLAG_MEMBER_FUSED (route 10): a full-box pass of a call under the membership test that the compiled
    // kernels can take -- a compiled layout without RPF_FLAG_GENERIC, not wide, no gain other than 1 (the bits above already say so:
    // check_schedule and the branch above keep treating a gain-other-than-1 pass of such a call as layout-generic, route 9)
    // RPF_FLAG_SCHEDULE_FUSED lifts the last condition: the pass takes route 10 on the scheduled builds, kGenericSchedule gives way to
    // the host-side kGenericScheduleFused
    const int32_t no_fused = kGenericOn | kGenericWide | kGenericSampled | ((d->flags & RPF_FLAG_SCHEDULE_FUSED) ? 0 : kGenericSchedule);
    const bool member_fused = (d->flags & RPF_FLAG_MEMBER_FUSED) && member && p.lay.supported() &&
                              !(p.generic & no_fused) && p.nmax <= kMaxNbhd;
    if (member_fused) p.generic |= kGenericMemberFused;
    if (member_fused && (p.generic & kGenericSchedule)) p.generic = (p.generic & ~kGenericSchedule) | kGenericScheduleFused;
    // RPF_FLAG_SAMPLED_FUSED (route 11): a sampled pass that the compiled kernels can take behind the draws'
    // mask kernel -- a compiled layout without RPF_FLAG_GENERIC, not wide, S + draws within the largest resident class (the
    // streaming class repeats a full-box stage 1b and cannot read a sampled list: it is empty by construction), no gain other than
    // 1 unless RPF_FLAG_SCHEDULE_FUSED hands the pass to the scheduled builds, and a mask stride within option
    // "sampled_fused_stride".  Every other sampled pass stays on route 8 with the bits it had
    const int64_t window_words = std::max<int64_t>(1, ((int64_t)(box * box - 1) * d->S + 63) / 64);
    const int32_t no_sampled_fused = kGenericOn | kGenericWide | ((d->flags & RPF_FLAG_SCHEDULE_FUSED) ? 0 : kGenericSchedule);
    const bool sampled_fused = (d->flags & RPF_FLAG_SAMPLED_FUSED) && (p.generic & kGenericSampled) && p.lay.supported() &&
                               !(p.generic & no_sampled_fused) && p.nmax <= kMaxNbhd &&
                               (int64_t)d->S + ctx->samp_now.draws <= kMaxResident &&
                               (ctx->tun.sampled_fused_stride < 0 || window_words <= ctx->tun.sampled_fused_stride);
    // RPF_FLAG_SAMPLED_LISTED (route 12): a sampled pass that the listed builds of the compiled kernels can
    // take behind a count kernel that lists into the member pool -- route 11's conditions without the two its masks impose: the
    // window may be wide by its size (the pass is accepted at all: nbhd_cap above; a pass that option "wide" forces is not taken),
    // and no mask stride bounds it.  Where route 11 applies as well, option "sampled_listed_stride" decides: route 12 from that
    // stride on.  A wide pass loses its wide bits: it is sized and set up from min(box*box*S, S + draws), not as a wide-kernel pass
    const int32_t no_sampled_listed = kGenericOn | ((d->flags & RPF_FLAG_SCHEDULE_FUSED) ? 0 : kGenericSchedule);
    const int32_t listed_from = ctx->tun.sampled_listed_stride < 0 ? kSampledListedStride : ctx->tun.sampled_listed_stride;
    const bool sampled_listed = (d->flags & RPF_FLAG_SAMPLED_LISTED) && (p.generic & kGenericSampled) && p.lay.supported() &&
                                !(p.generic & no_sampled_listed) && ctx->tun.wide != 1 &&
                                (int64_t)d->S + ctx->samp_now.draws <= kMaxResident &&
                                (!sampled_fused || window_words >= listed_from);
    if (sampled_listed) {
        p.generic = (p.generic & ~(kGenericWide | kGenericWideClasses | kGenericStreamFast)) | kGenericSampledListed;
        if (p.generic & kGenericSchedule) p.generic = (p.generic & ~kGenericSchedule) | kGenericScheduleFused;
        wide = false;
    } else if (sampled_fused) {
        p.generic |= kGenericSampledFused;
        if (p.generic & kGenericSchedule) p.generic = (p.generic & ~kGenericSchedule) | kGenericScheduleFused;
    }
    p.sigma_p = (double)(box / 4); // rpf.cpp:531: integer division
    p.plane_stride = (uint64_t)d->W * d->H * d->S;
    p.planes = d_planes; p.col_in = col_in; p.col_out = col_out;
    const size_t HW = (size_t)d->W * d->H;
    int32_t st;
    if ((st = ctx->d_pmean.ensure(ctx, HW * kNFeat * sizeof(double)))) return st;
    if ((st = ctx->d_pstd.ensure(ctx, HW * kNFeat * sizeof(double)))) return st;
    if ((st = ctx->d_nbhd.ensure(ctx, HW * sizeof(int32_t)))) return st;
    // (the 2^-44 tables stop at the old cap: a wide pass reads them only where they are exact, launch_wide)
    if ((st = ensure_tables(ctx, std::min(p.nmax, kMaxNbhd)))) return st;
    if (wide && (st = ensure_wide_table(ctx, p.nmax))) return st;
    // (route 9's rest launch reads the 2^-44 table where that is exact, as a forced wide pass does, and route 6's table above)
    if (member && !wide && !sampled_listed && p.nmax > kTFixExact && (st = ensure_wide_table(ctx, p.nmax))) return st;
    if (member && (st = ensure_member_table(ctx))) return st;
    if ((p.generic & kGenericSampled) && (st = ensure_sampling_table(ctx, box))) return st;
    p.pmean = ctx->d_pmean; p.pstd = ctx->d_pstd; p.tfix = ctx->d_tfix; p.dfix = ctx->d_dfix;
    p.nbhd = ctx->d_nbhd; p.status = ctx->d_status;
    if ((st = ctx->d_flat.ensure(ctx, HW))) return st;
    p.flat = ctx->d_flat; p.nan_flag = ctx->d_nan_flag;
    if (dbg_dev) p.dbg = *dbg_dev;
    if (sampled_fused || sampled_listed) { // the largest resident kernel of the pass: no list is longer than S + draws, whatever the window holds
        const int nres = (int)std::min<int64_t>(p.nmax, (int64_t)d->S + ctx->samp_now.draws), bres = bmax_of(nres);
        out.lds = lds_layout(p.S, nres, bres, table_in_lds(p.S, nres, bres, ctx->tun, p.lay), ctx->tun, p.lay).total;
    } else if (member_fused) { // the largest resident kernel of the pass, as on route 2, and -- its streaming class -- the wide kernel's carve-up
        const int nres = std::min(p.nmax, kMaxResident), bres = bmax_of(nres);
        out.lds = lds_layout(p.S, nres, bres, table_in_lds(p.S, nres, bres, ctx->tun, p.lay), ctx->tun, p.lay).total;
        if (p.nmax > kMaxResident) out.lds = std::max(out.lds, generic_wide_carve(p.lay, p.nmax, false).total);
    } else if (wide || (member && !(p.generic & kGenericSampled))) { // the wide kernel's carve-up: what 160 KiB leave of the joint table is one band of it
        out.lds = generic_wide_carve(p.lay, p.nmax, stream_fast(p)).total;
    } else if (route_bits(p.generic)) { // the generic kernel's own carve-up (one kernel for every neighbourhood size of the pass)
        out.lds = generic_carve(p.lay, p.nmax, stream_fast(p)).total;
    } else { // LDS of the largest resident kernel this pass can launch (larger neighbourhoods stream: generic::filter_pixel_kernel)
        const int nres = std::min(p.nmax, kMaxResident), bres = bmax_of(nres);
        out.lds = lds_layout(p.S, nres, bres, table_in_lds(p.S, nres, bres, ctx->tun, p.lay), ctx->tun, p.lay).total;
    }
    if ((int)out.lds > max_lds_per_block())
        return fail(ctx, RPF_E_UNSUPPORTED, "neighbourhood working set exceeds 160 KiB of LDS");
    return RPF_OK;
}

// A call begins: no bad pixel yet, N reduction and NaN flag zero (stage 1a of pass 0 refills the flag and the flat plane),
// nothing kept from the planes of an earlier call, counters at their start.
int32_t begin_call(rpf_ctx *ctx, hipStream_t s) {
    static const int32_t init_status[2] = {0, INT_MAX};
    HIP_TRY(hipMemcpyAsync(ctx->d_status, init_status, sizeof(init_status), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(ctx->d_nred, 0, 2 * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(ctx->d_nan_flag, 0, sizeof(int32_t), s));
    ctx->flat_fresh = true;
    ctx->bin_valid = false;
    ctx->counters = rpf_counters{};
    ctx->counters.first_bad_pixel = -1;
    ctx->spike = rpf_spike_stats{}; // applied = 0 until this call's spike pass has run
    report_clear(ctx);              // ... and every pass report's until that pass has reported (RPF_FLAG_PASS_REPORT)
    return RPF_OK;
}

std::string nonfinite_message(int x, int y, long long count) {
    char buf[160];
    std::snprintf(buf, sizeof(buf), "non-finite filtered colour at pixel (x=%d, y=%d); %lld pixel(s) affected "
                  "(the reference exits here, rpf.cpp:702-705)", x, y, count);
    return buf;
}

// A call ends, after n_pass passes over the slab of d: reduces N, reads status, N reduction and the last pass's redo counts back (one
// synchronisation of s) and fills the counters that do not depend on the entry point.
int32_t finish_counters(rpf_ctx *ctx, const rpf_desc *d, int n_pass, hipStream_t s) {
    rpf_counters &c = ctx->counters;
    HIP_TRY(launch_nbhd_reduce(ctx->d_nbhd, d->W, d->row_begin, d->row_end, ctx->d_nred, s));
    int32_t hst[2];
    unsigned long long nred[2];
    uint32_t redo[kRedoCounts] = {};
    HIP_TRY(hipMemcpyAsync(hst, ctx->d_status, sizeof(hst), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(nred, ctx->d_nred, sizeof(nred), hipMemcpyDeviceToHost, s));
    if (d->degenerate_policy == RPF_DEGEN_REF_ABORT)
        HIP_TRY(hipMemcpyAsync(redo, ctx->d_redo_count, sizeof(redo), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // the last pass's: one count per route_pass call of it -- one, or one per row band of rpf_filter's pipeline
    c.redo_pixels = (int32_t)std::accumulate(redo, redo + std::min(ctx->redo_used, kRedoCounts), (uint32_t)0);
    c.samples_filtered = (int64_t)(d->row_end - d->row_begin) * d->W * d->S * n_pass;
    c.options_active = ctx->tun.is_default() ? 0 : 1;
    c.sum_nbhd = (int64_t)nred[0];
    c.max_nbhd = (int32_t)nred[1];
    c.nonfinite_pixels = hst[0];
    c.first_bad_pixel = hst[0] ? hst[1] : -1;
    if (hst[0] && d->degenerate_policy == RPF_DEGEN_REF_ABORT)
        return fail(ctx, RPF_E_NONFINITE, nonfinite_message(hst[1] % d->W, hst[1] / d->W, hst[0]));
    return RPF_OK;
}

// Rows [r0, r1) of a pass over the slab [row_begin, row_end) of d: those outside the slab (halo) pass through unchanged
// (rpf.cpp filters whole films; slabs are this build's multi-GPU cut)
int32_t pass_through(rpf_ctx *ctx, const rpf_desc *d, const double *cin, double *cout, int r0, int r1, hipStream_t s) {
    const size_t row = (size_t)d->W * d->S, ps = row * d->H;
    const int a0 = r0, a1 = std::min(r1, d->row_begin), b0 = std::max(r0, d->row_end), b1 = r1;
    if (a1 > a0) HIP_TRY(launch_copy_colour_span(cin, cout, ps, (uint64_t)a0 * row, (uint64_t)(a1 - a0) * row, s));
    if (b1 > b0) HIP_TRY(launch_copy_colour_span(cin, cout, ps, (uint64_t)b0 * row, (uint64_t)(b1 - b0) * row, s));
    return RPF_OK;
}

// Device copies of a whole frame of d: the planes, the ray weights when the caller has them, the colours (d_colA) when asked
int32_t ensure_frame(rpf_ctx *ctx, const rpf_desc *d, bool ray_weight, bool colour) {
    const size_t ps = (size_t)d->W * d->H * d->S;
    const SampleLayout lay = layout_of(d);
    int32_t st;
    if ((st = ctx->d_planes.ensure(ctx, (size_t)lay.ndim() * ps * lay.plane_bytes()))) return st;
    if (colour && (st = ctx->d_colA.ensure(ctx, 3 * ps * sizeof(double)))) return st;
    if (ray_weight && (st = ctx->d_rayw.ensure(ctx, ps * sizeof(float)))) return st;
    return RPF_OK;
}

// ... and of the reduced outputs a caller wants: sample colours (3 planes fp32), pixel colours ([H][W][3])
int32_t ensure_outputs(rpf_ctx *ctx, const rpf_desc *d, bool sample_rgb, bool pixel_rgb) {
    const size_t HW = (size_t)d->W * d->H;
    int32_t st;
    if (sample_rgb && (st = ctx->d_srgb.ensure(ctx, 3 * HW * d->S * sizeof(float)))) return st;
    if (pixel_rgb && (st = ctx->d_prgb.ensure(ctx, 3 * HW * sizeof(float)))) return st;
    return RPF_OK;
}

// Uploads a whole frame from host memory on s.  colour: d_colA is uploaded from colour64, or seeded from the colour planes
// when that is null.
int32_t upload_frame(rpf_ctx *ctx, const rpf_desc *d, const void *planes, const float *ray_weight, bool colour,
                     const double *colour64, hipStream_t s) {
    int32_t st;
    if ((st = ensure_frame(ctx, d, ray_weight != nullptr, colour))) return st;
    const size_t ps = (size_t)d->W * d->H * d->S;
    const SampleLayout lay = layout_of(d);
    HIP_TRY(hipMemcpyAsync(ctx->d_planes, planes, (size_t)lay.ndim() * ps * lay.plane_bytes(), hipMemcpyHostToDevice, s));
    if (ray_weight) HIP_TRY(hipMemcpyAsync(ctx->d_rayw, ray_weight, ps * sizeof(float), hipMemcpyHostToDevice, s));
    if (colour && colour64) HIP_TRY(hipMemcpyAsync(ctx->d_colA, colour64, 3 * ps * sizeof(double), hipMemcpyHostToDevice, s));
    else if (colour) HIP_TRY(launch_colour_from_planes(ctx->d_planes, lay.f16 != 0, ctx->d_colA, ps, s));
    return RPF_OK;
}

// Reduces rows [r0, r1) of `colour` (a frame of d) on s and queues their download on `to` -- ordered behind the reduction
// by `ready` when that is another stream -- to the caller's sample colours (planes `out_plane` floats apart) and pixel
// colours, from row out_row on.  Either output may be null.
int32_t download_rows(rpf_ctx *ctx, const rpf_desc *d, const double *colour, const float *d_ray_weight, int r0, int r1,
                      float *sample_rgb_out, float *pixel_rgb_out, size_t out_plane, int out_row, hipStream_t s,
                      hipStream_t to, hipEvent_t ready) {
    if (!sample_rgb_out && !pixel_rgb_out) return RPF_OK;
    const size_t row = (size_t)d->W * d->S, ps = row * d->H, n = (size_t)(r1 - r0) * row;
    HIP_TRY(launch_reduce_rows(colour, d_ray_weight, sample_rgb_out ? ctx->d_srgb.ptr : nullptr,
                               pixel_rgb_out ? ctx->d_prgb.ptr : nullptr, d->W, d->H, d->S, r0, r1, s));
    if (to != s) {
        HIP_TRY(hipEventRecord(ready, s));
        HIP_TRY(hipStreamWaitEvent(to, ready, 0));
    }
    if (sample_rgb_out && n == ps && out_plane == ps) // whole planes, back to back on both sides
        HIP_TRY(hipMemcpyAsync(sample_rgb_out, ctx->d_srgb, 3 * ps * sizeof(float), hipMemcpyDeviceToHost, to));
    else if (sample_rgb_out)
        for (int k = 0; k < 3; ++k)
            HIP_TRY(hipMemcpyAsync(sample_rgb_out + k * out_plane + (size_t)out_row * row, ctx->d_srgb + k * ps + (size_t)r0 * row,
                                   n * sizeof(float), hipMemcpyDeviceToHost, to));
    if (pixel_rgb_out)
        HIP_TRY(hipMemcpyAsync(pixel_rgb_out + (size_t)out_row * d->W * 3, ctx->d_prgb + (size_t)r0 * d->W * 3,
                               (size_t)(r1 - r0) * d->W * 3 * sizeof(float), hipMemcpyDeviceToHost, to));
    return RPF_OK;
}

// runs all passes of desc on device-resident buffers; colour ends up in d_colour
int32_t run_passes(rpf_ctx *ctx, const rpf_desc *d, const void *d_planes, double *d_colour, hipStream_t s) {
    const bool timing = (d->flags & RPF_FLAG_TIMING) != 0;
    const size_t ps = (size_t)d->W * d->H * d->S;
    int32_t st;
    if ((st = ctx->d_colB.ensure(ctx, 3 * ps * sizeof(double)))) return st;
    if ((st = begin_call(ctx, s))) return st;
    rpf_counters &c = ctx->counters;
    float ms_filter = 0.f, ms_stats = 0.f;
    if (timing) HIP_TRY(hipEventRecord(ctx->ev[0], s));
    double *cin = d_colour, *cout = ctx->d_colB; // ping-pong: the filtered colours replace the film's (rpf.cpp:732)
    const bool report = (d->flags & RPF_FLAG_PASS_REPORT) != 0;
    for (int i = 0; i < d->n_box; ++i) {
        PassSetup ps_;
        rpf_debug rep{}; // RPF_FLAG_PASS_REPORT: the pass writes alpha, beta and W_r_c into the context's scratch planes
        if (report && (st = report_planes(ctx, d, rep, s))) return st;
        if ((st = setup_pass(ctx, d, d->box_sizes[i], i, d_planes, cin, cout, report ? &rep : nullptr, ps_))) return st;
        if ((st = pass_through(ctx, d, cin, cout, 0, d->H, s))) return st;
        if (timing) HIP_TRY(hipEventRecord(ctx->ev[1], s));
        // stage 1a depends on the features only: formed once (the reference recomputes identical values per pass)
        if (i == 0) {
            Range rg("rpf:stage 1a pixel_stats");
            HIP_TRY(launch_pixel_stats(ps_.p, s));
        }
        if (timing) HIP_TRY(hipEventRecord(ctx->ev[2], s));
        if ((st = route_pass(ctx, ps_.p, s, &c.filter_kernel_launches))) return st;
        if (timing) {
            HIP_TRY(hipEventRecord(ctx->ev[3], s));
            HIP_TRY(hipEventSynchronize(ctx->ev[3]));
            float a = 0.f, b = 0.f;
            HIP_TRY(hipEventElapsedTime(&a, ctx->ev[1], ctx->ev[2]));
            HIP_TRY(hipEventElapsedTime(&b, ctx->ev[2], ctx->ev[3]));
            ms_stats += a;
            ms_filter += b;
        }
        // the pass's report: behind route_pass (its redo launch included), outside the filter's timing bracket
        if (report && (st = report_pass(ctx, d, i, d->box_sizes[i], cin, cout, rep, s))) return st;
        std::swap(cin, cout);
    }
    if (cin != d_colour) HIP_TRY(hipMemcpyAsync(d_colour, cin, 3 * ps * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (timing) {
        HIP_TRY(hipEventRecord(ctx->ev[3], s));
        HIP_TRY(hipEventSynchronize(ctx->ev[3]));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[3]));
        c.device_total_ms = t;
    }
    c.filter_kernel_ms = ms_filter;
    c.stats_kernel_ms = ms_stats;
    // the spike pass: after the last pass, before every reduce / download / film step of the callers; it runs whatever
    // finish_counters is about to say (RPF_E_NONFINITE included)
    if ((d->flags & RPF_FLAG_SPIKE_CLAMP) && (st = spike_pass(ctx, d, d_colour, s))) return st;
    return finish_counters(ctx, d, d->n_box, s);
}

namespace {

double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// ---- host-buffer entry: row-band pipeline ----------------------------------------------------------------
// rpf_filter() receives the film in host memory.  The planes are [dim][y][x][s], so a band of rows is one
// contiguous span per plane: the image is cut into ~8 row bands, band j+1 is uploaded (s_up) while band j is
// filtered (compute stream), and in the last pass band j is reduced and downloaded (s_down) while band j+1 is
// filtered.  A band can be filtered once the b halo rows below it are resident, i.e. once the next band is up.
// The per-pixel feature statistics (stage 1a) depend on the features only, so they are formed once, in pass 0
// (the reference recomputes identical values every pass, rpf.cpp:529).
struct Band { int r0, r1; };

int32_t ensure_band_events(rpf_ctx *ctx, size_t n) {
    while (ctx->band_ev.size() < n) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->band_ev.push_back(e);
    }
    return RPF_OK;
}

int32_t run_host_pipeline(rpf_ctx *ctx, const rpf_desc *d, const void *planes_v, const float *ray_weight,
                          float *sample_rgb_out, float *pixel_rgb_out) {
    const int W = d->W, H = d->H, S = d->S;
    const size_t row = (size_t)W * S, ps = row * H;
    const SampleLayout lay = layout_of(d);
    const int kNDim = lay.ndim();
    const size_t pb = lay.plane_bytes();
    const char *planes = static_cast<const char *>(planes_v);
    hipStream_t s = ctx->stream, up = ctx->s_up, down = ctx->s_down;
    int32_t st;
    if ((st = ctx->d_colB.ensure(ctx, 3 * ps * sizeof(double)))) return st; // the frame and the outputs: rpf_filter_ex

    // bands: about eight, never thinner than the widest halo of the first / last pass (or 16 rows)
    const int b_first = (d->box_sizes[0] - 1) / 2, b_last = (d->box_sizes[d->n_box - 1] - 1) / 2;
    const int min_rows = std::max(16, std::max(b_first, b_last));
    int nb = std::min(8, std::max(1, H / min_rows));
    const int bh = (H + nb - 1) / nb;
    nb = (H + bh - 1) / bh;
    std::vector<Band> bands(nb);
    for (int j = 0; j < nb; ++j) bands[j] = Band{j * bh, std::min(H, (j + 1) * bh)};
    if ((st = ensure_band_events(ctx, 2 * (size_t)nb))) return st;
    hipEvent_t *ev_up = ctx->band_ev.data(), *ev_done = ctx->band_ev.data() + nb;

    if ((st = begin_call(ctx, s))) return st;
    rpf_counters &c = ctx->counters;

    double *cin = ctx->d_colA, *cout = ctx->d_colB;
    const bool want_out = sample_rgb_out || pixel_rgb_out;
    const double t0 = now_ms();
    for (int i = 0; i < d->n_box; ++i) {
        const bool first = i == 0, last = i == d->n_box - 1;
        PassSetup ps_;
        if ((st = setup_pass(ctx, d, d->box_sizes[i], i, ctx->d_planes, cin, cout, nullptr, ps_))) return st;
        auto filter_rows = [&](int r0, int r1) -> int32_t {
            PassParams q = ps_.p;
            q.row_begin = std::max(r0, d->row_begin);
            q.row_end = std::min(r1, d->row_end);
            if ((st = pass_through(ctx, d, cin, cout, r0, r1, s))) return st;
            if (q.row_end <= q.row_begin) return RPF_OK;
            // the route probe of an unbinned pass: every row of the slab that is resident and has its stage 1a -- in the first pass
            // those down to the band's last row (the band below it, its halo, is up), afterwards the whole slab.  The last band of
            // a pass so decides on the serial call's lattice, and rpf_query_route answers as after the serial call
            ctx->probe_r0 = d->row_begin;
            ctx->probe_r1 = first ? std::min(r1, d->row_end) : d->row_end;
            st = route_pass(ctx, q, s, &c.filter_kernel_launches);
            ctx->probe_r0 = ctx->probe_r1 = 0;
            return st;
        };
        auto emit_rows = [&](int j) -> int32_t { // last pass: reduce + download band j
            if (!want_out) return RPF_OK;
            Range rg("rpf:reduce + download band");
            const Band &bd = bands[j];
            return download_rows(ctx, d, cout, ray_weight ? ctx->d_rayw.ptr : nullptr, bd.r0, bd.r1, sample_rgb_out,
                                 pixel_rgb_out, ps, bd.r0, s, down, ev_done[j]);
        };
        if (!first && !last) { // middle passes: one launch over the slab
            if ((st = filter_rows(0, H))) return st;
        } else {
            for (int j = 0; j < nb; ++j) {
                const Band &bd = bands[j];
                if (first) {
                    Range rg("rpf:upload band + stage 1a");
                    const size_t o = (size_t)bd.r0 * row, n = (size_t)(bd.r1 - bd.r0) * row;
                    for (int k = 0; k < kNDim; ++k)
                        HIP_TRY(hipMemcpyAsync(ctx->d_planes + (k * ps + o) * pb, planes + (k * ps + o) * pb, n * pb,
                                               hipMemcpyHostToDevice, up));
                    if (ray_weight)
                        HIP_TRY(hipMemcpyAsync(ctx->d_rayw + o, ray_weight + o, n * sizeof(float), hipMemcpyHostToDevice, up));
                    HIP_TRY(hipEventRecord(ev_up[j], up));
                    HIP_TRY(hipStreamWaitEvent(s, ev_up[j], 0));
                    HIP_TRY(launch_colour_from_planes_span(ctx->d_planes, lay.f16 != 0, cin, ps, o, n, s));
                    HIP_TRY(launch_pixel_stats_rows(ps_.p, bd.r0, bd.r1, s));
                    if (j >= 1) { // band j-1 has its lower halo now
                        if ((st = filter_rows(bands[j - 1].r0, bands[j - 1].r1))) return st;
                        if (last && (st = emit_rows(j - 1))) return st;
                    }
                } else {
                    if ((st = filter_rows(bd.r0, bd.r1))) return st;
                    if ((st = emit_rows(j))) return st;
                }
            }
            if (first) {
                if ((st = filter_rows(bands[nb - 1].r0, bands[nb - 1].r1))) return st;
                if (last && (st = emit_rows(nb - 1))) return st;
            }
        }
        std::swap(cin, cout);
    }
    // cin now names the buffer holding the final colours; keep the convention "result in d_colA"
    if (cin != ctx->d_colA) ctx->d_colA.swap(ctx->d_colB);
    const int32_t fst = finish_counters(ctx, d, d->n_box, s);
    HIP_TRY(hipStreamSynchronize(down));
    HIP_TRY(hipStreamSynchronize(up));
    c.device_total_ms = (float)(now_ms() - t0); // wall clock of the overlapped upload + passes + download
    return fst;
}

} // namespace

} // namespace rpf

extern "C" {

const char *rpf_version(void) { return "rpf_hip 0.1 (gfx950)"; }

const char *rpf_status_string(int32_t s) {
    switch (s) {
    case RPF_OK: return "RPF_OK";
    case RPF_E_BADARG: return "RPF_E_BADARG";
    case RPF_E_HIP: return "RPF_E_HIP";
    case RPF_E_NONFINITE: return "RPF_E_NONFINITE";
    case RPF_E_NOMEM: return "RPF_E_NOMEM";
    case RPF_E_UNSUPPORTED: return "RPF_E_UNSUPPORTED";
    case RPF_E_NODEVICE: return "RPF_E_NODEVICE";
    default: return "RPF_E_?";
    }
}

int32_t rpf_create(rpf_ctx **out, int32_t device) {
    if (!out) return RPF_E_BADARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RPF_E_NODEVICE;
    if (device < 0 || device >= n) return RPF_E_BADARG;
    rpf_ctx *ctx = new rpf_ctx();
    ctx->device = device;
    *out = ctx; // returned even on failure so that rpf_last_error() can be read; caller destroys it
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&ctx->s_up, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&ctx->s_down, hipStreamNonBlocking));
    int32_t st;
    if ((st = ctx->d_status.ensure(ctx, 2 * sizeof(int32_t)))) return st;
    if ((st = ctx->d_nred.ensure(ctx, 2 * sizeof(unsigned long long)))) return st;
    if ((st = ctx->d_class_counts.ensure(ctx, (kNumClasses + 2) * sizeof(uint32_t)))) return st;
    if ((st = ctx->d_nan_flag.ensure(ctx, sizeof(int32_t)))) return st;
    HIP_TRY(hipMemset(ctx->d_nan_flag, 0, sizeof(int32_t)));
    if ((st = ctx->d_redo_count.ensure(ctx, kRedoCounts * sizeof(uint32_t)))) return st;
    HIP_TRY(hipMemset(ctx->d_redo_count, 0, kRedoCounts * sizeof(uint32_t)));
    for (auto &e : ctx->ev) HIP_TRY(hipEventCreate(&e));
    return RPF_OK;
}

void rpf_destroy(rpf_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    const std::vector<hipEvent_t> band_ev = ctx->band_ev;
    const hipEvent_t ev[4] = {ctx->ev[0], ctx->ev[1], ctx->ev[2], ctx->ev[3]};
    const hipStream_t streams[3] = {ctx->s_up, ctx->s_down, ctx->stream};
    delete ctx; // frees every buffer: before the events and streams go
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : band_ev)
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t q : streams)
        if (q) (void)hipStreamDestroy(q);
}

const char *rpf_last_error(const rpf_ctx *ctx) { return ctx ? ctx->err.c_str() : "ctx is NULL"; }

int32_t rpf_check_window_span(int32_t W, int32_t S, int32_t box) {
    if (W <= 0 || S <= 0 || box <= 0) return RPF_E_BADARG;
    // box rows of W pixels of S samples, 8 bytes each in the widest plane type (the fp64 colours)
    return (uint64_t)box * (uint64_t)W * (uint64_t)S * 8ull < (1ull << 32) ? RPF_OK : RPF_E_UNSUPPORTED;
}

int32_t rpf_layout_kernels(const rpf_desc *d, int32_t *generic_out) { return layout_kernels(d, generic_out, nullptr); }

int32_t rpf_max_nbhd(const rpf_desc *d, int32_t *nmax_out) {
    if (!d || !nmax_out) return RPF_E_BADARG;
    *nmax_out = (d->flags & RPF_FLAG_WIDE_NBHD) ? kMaxWideNbhd : kMaxNbhd;
    return RPF_OK;
}

int32_t rpf_max_draws(const rpf_desc *d, int32_t *dmax_out) {
    if (!d || !dmax_out || d->S <= 0) return RPF_E_BADARG;
    const int32_t cap = (d->flags & RPF_FLAG_SAMPLED_REST) ? RPF_SAMPLED_MAX : 832;
    *dmax_out = std::max(0, cap - d->S);
    return RPF_OK;
}

int32_t rpf_generic_quad_carve(const rpf_desc *d, int32_t capacity, int32_t *workgroups_per_cu_out, int64_t *lds_bytes_out) {
    if (!d || (capacity != class_capacity(kNumClasses - 3) && capacity != class_capacity(kNumClasses - 2))) return RPF_E_BADARG;
    const SampleLayout lay = layout_of(d);
    if (!lay.generic_ok()) return RPF_E_UNSUPPORTED;
    const GenericQuadCarve cv = generic_quad_carve(lay, capacity);
    if (cv.hists == 0) return RPF_E_UNSUPPORTED;
    if (workgroups_per_cu_out) *workgroups_per_cu_out = (int32_t)cv.workgroups_per_cu;
    if (lds_bytes_out) *lds_bytes_out = (int64_t)cv.total;
    return RPF_OK;
}

int32_t rpf_set_sampling(rpf_ctx *ctx, const rpf_sampling *cfg) {
    if (!ctx) return RPF_E_BADARG;
    std::string why;
    const int32_t st = check_sampling(cfg, why);
    if (st) return fail(ctx, st, why);
    ctx->sampling = *cfg;
    ctx->sampling_set = true;
    ctx->bin_valid = false;
    return RPF_OK;
}

int32_t rpf_set_membership(rpf_ctx *ctx, const rpf_membership *cfg) {
    if (!ctx) return RPF_E_BADARG;
    std::string why;
    const int32_t st = check_membership(cfg, why);
    if (st) return fail(ctx, st, why);
    ctx->membership = *cfg;
    ctx->membership_set = true;
    ctx->member_fresh = false; // setup_pass uploads it
    ctx->bin_valid = false;
    return RPF_OK;
}

int32_t rpf_membership_preset(int32_t kind, int32_t n_feat, rpf_membership *out) {
    if (!out || kind < 0 || kind > 1 || n_feat < 1 || n_feat > RPF_MAX_NDIM) return RPF_E_BADARG;
    if (kind == 1 && n_feat != 12) return RPF_E_BADARG; // the 19-dim layout: n0 | p0 | n1 | p1, three features each
    for (int k = 0; k < RPF_MAX_NDIM; ++k) { out->mult[k] = 3.0; out->floor[k] = -1.0; }
    if (kind == 1)
        for (int k = 0; k < 12; ++k) {
            out->mult[k] = ((k >= 3 && k < 6) || k >= 9) ? 30.0 : 3.0;
            out->floor[k] = 0.1;
        }
    return RPF_OK;
}

int32_t rpf_set_schedule(rpf_ctx *ctx, const rpf_schedule *cfg) {
    if (!ctx) return RPF_E_BADARG;
    std::string why;
    const int32_t st = check_schedule_table(cfg, why);
    if (st) return fail(ctx, st, why);
    ctx->schedule = *cfg;
    ctx->schedule_set = true; // (host only: setup_pass copies a pass's entry into its PassParams)
    return RPF_OK;
}

int32_t rpf_schedule_preset(int32_t kind, int32_t S, rpf_schedule *out) {
    if (!out || kind < 0 || kind > 1 || S <= 0) return RPF_E_BADARG;
    out->pass0 = 0; out->reserved = 0;
    for (int t = 0; t < RPF_MAX_BOXES; ++t) {
        if (kind == 0) { // the reference: one seed (rpf.cpp:662's 0.002), alpha = 1 - W_r^c, beta = (1 - W_r^f) W_c^f
            out->seed[t] = 0.002; out->gain_c[t] = 1.0; out->gain_f[t] = 1.0;
        } else { // "published", from memory of the paper (include/rpf_hip.h says so): nothing in the library depends on these
            const double v_t = t == 0 ? 0.02 : 0.002;
            out->seed[t] = sqrt(8.0 * v_t / (double)S);
            out->gain_c[t] = 2.0 * (1.0 + 0.1 * t);
            out->gain_f[t] = 1.0 + 0.1 * t;
        }
    }
    return RPF_OK;
}

int32_t rpf_sampling_table(int32_t box, uint32_t *table_out) {
    if (!table_out || box < 1 || box > 511 || (box & 1) == 0) return RPF_E_BADARG;
    sampling_table(box, table_out);
    return RPF_OK;
}

int32_t rpf_sampling_draws(const rpf_sampling *cfg, int32_t pass, int32_t box, int32_t W, int32_t H, int32_t S, int32_t x, int32_t y,
                           int32_t *qq_out, int32_t *n_out) {
    if (!cfg || !qq_out || !n_out || pass < 0 || pass >= RPF_MAX_BOXES || box < 1 || box > 511 || (box & 1) == 0) return RPF_E_BADARG;
    if (W <= 0 || H <= 0 || S <= 0 || x < 0 || x >= W || y < 0 || y >= H || cfg->draws[pass] < 0) return RPF_E_BADARG;
    auto mix = [](uint64_t z) {
        z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
        z ^= z >> 27; z *= 0x94D049BB133111EBull;
        z ^= z >> 31;
        return z;
    };
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    const int b = (box - 1) / 2, D = cfg->draws[pass];
    std::vector<uint32_t> T((size_t)std::max(box - 1, 1), 0u);
    sampling_table(box, T.data());
    const int nT = box - 1;
    auto count_le = [&](uint32_t u) { return (int)(std::upper_bound(T.begin(), T.begin() + nT, u) - T.begin()); };
    uint64_t h = mix(cfg->seed + G);
    h = mix(h ^ (uint64_t)((uint32_t)cfg->pass_id0 + (uint32_t)pass)); // (sums mod 2^32: no signed overflow at any configuration)
    h = mix(h ^ (uint64_t)((uint32_t)cfg->row_origin + (uint32_t)y));
    h = mix(h ^ (uint64_t)(uint32_t)x);
    // the window's numbering: candidate_offset of rpf_generic_common.h, inverted
    const int x0 = std::max(x - b, 0), y0 = std::max(y - b, 0), y1 = std::min(y + b, H - 1);
    const int nyv = y1 - y0 + 1, centre_rank = (x - x0) * nyv + (y - y0);
    std::vector<int32_t> qq;
    qq.reserve((size_t)D);
    for (int q = 0; q < D; ++q) {
        const uint64_t r = mix(h + (uint64_t)(q + 1) * G), r2 = mix(r ^ G);
        const int xn = x + count_le((uint32_t)r) - b, yn = y + count_le((uint32_t)(r >> 32)) - b;
        const int smp = (int)(((uint64_t)(uint32_t)r2 * (uint32_t)S) >> 32);
        if (xn < 0 || xn >= W || yn < 0 || yn >= H || (xn == x && yn == y)) continue;
        int cell = (xn - x0) * nyv + (yn - y0);
        if (cell > centre_rank) --cell;
        qq.push_back(cell * S + smp);
    }
    std::sort(qq.begin(), qq.end());
    qq.erase(std::unique(qq.begin(), qq.end()), qq.end());
    std::copy(qq.begin(), qq.end(), qq_out);
    *n_out = (int32_t)qq.size();
    return RPF_OK;
}

int32_t rpf_wide_table(int32_t nmax, uint64_t *table_out) {
    if (!table_out || nmax < 0 || nmax > kMaxWideNbhd) return RPF_E_BADARG;
    wide_table(nmax, table_out);
    return RPF_OK;
}

int64_t rpf_lds_bytes_required(int32_t S, int32_t box) {
    if (S <= 0 || box <= 0) return -1;
    const int64_t nmax = (int64_t)box * box * S;
    if (nmax > 49 * 64) return -1;
    const int nm = (int)nmax;
    const int bmax = bmax_of(nm);
    const Tuning tun;
    const SampleLayout lay;
    return lds_layout(S, nm, bmax, table_in_lds(S, nm, bmax, tun, lay), tun, lay).total;
}

int32_t rpf_colour_from_planes_device(rpf_ctx *ctx, const rpf_desc *d, const void *d_planes, double *d_colour,
                                      void *stream) {
    int32_t st = enter(ctx, d, false);
    if (st) return st;
    if (!d_planes || !d_colour) return fail(ctx, RPF_E_BADARG, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream; // NULL = the legacy default stream: ordered after the caller's own work
    HIP_TRY(launch_colour_from_planes(d_planes, layout_of(d).f16 != 0, d_colour, (uint64_t)d->W * d->H * d->S, s));
    return RPF_OK;
}

int32_t rpf_reduce_device(rpf_ctx *ctx, const rpf_desc *d, const double *d_colour, const float *d_ray_weight,
                          float *d_sample_rgb_out, float *d_pixel_rgb_out, void *stream) {
    int32_t st = enter(ctx, d, false);
    if (st) return st;
    if (!d_colour) return fail(ctx, RPF_E_BADARG, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream; // NULL = the legacy default stream: ordered after the caller's own work
    HIP_TRY(launch_reduce(d_colour, d_ray_weight, d_sample_rgb_out, d_pixel_rgb_out, d->W, d->H, d->S, s));
    return RPF_OK;
}

int32_t rpf_filter_device(rpf_ctx *ctx, const rpf_desc *d, const void *d_planes, double *d_colour, void *stream) {
    int32_t st = enter(ctx, d, true);
    if (st) return st;
    if (!d_planes || !d_colour) return fail(ctx, RPF_E_BADARG, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream; // NULL = the legacy default stream: ordered after the caller's own work
    return run_passes(ctx, d, d_planes, d_colour, s);
}

int32_t rpf_host_alloc(rpf_ctx *ctx, uint64_t bytes, void **out) {
    if (!ctx) return RPF_E_BADARG;
    if (!out) return fail(ctx, RPF_E_BADARG, "out is NULL");
    *out = nullptr;
    HIP_TRY(hipSetDevice(ctx->device));
    hipError_t e = hipHostMalloc(out, bytes ? (size_t)bytes : 16, hipHostMallocDefault);
    if (e != hipSuccess)
        return fail(ctx, e == hipErrorOutOfMemory ? RPF_E_NOMEM : RPF_E_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    return RPF_OK;
}

int32_t rpf_host_free(rpf_ctx *ctx, void *ptr) { // ctx may be NULL (a buffer can outlive its context)
    if (!ptr) return RPF_OK;
    const hipError_t e = hipHostFree(ptr);
    if (e != hipSuccess) return fail(ctx, RPF_E_HIP, std::string("hipHostFree: ") + hipGetErrorString(e));
    return RPF_OK;
}

namespace {
// one (name, value) of rpf_set_option applied to t: false for an unknown name or a value outside its range (t is then unchanged)
bool apply_option(Tuning &t, const std::string &n, int64_t value) {
    if (n == "stage_mask") t.stage_mask = (int32_t)value;
    else if (n == "binning" && value >= -1 && value <= 1) t.binning = (int32_t)value;
    else if (n == "waves_per_pixel" && (value == 0 || value == 1 || value == 4)) t.waves_per_pixel = (int32_t)value;
    else if (n == "table_in_lds" && value >= -1 && value <= 1) t.table_in_lds = (int32_t)value;
    else if (n == "screen" && value >= 0 && value <= 1) t.screen = (int32_t)value;
    else if (n == "split_weights" && value >= -1 && value <= 1) t.split_weights = (int32_t)value;
    else if (n == "strip_w" && value >= 0 && value <= 4096 && value % 8 == 0) t.strip_w = (int32_t)value;
    else if (n == "packed" && value >= -1 && value <= 1) t.packed = (int32_t)value;
    else if (n == "wide" && (value == -1 || value == 1)) t.wide = (int32_t)value;
    else if (n == "wide_pool" && value >= -1 && value <= ((int64_t)1 << 40)) t.wide_pool = value;
    else if (n == "sampled_fused_stride" && value >= -1 && value <= 1024) t.sampled_fused_stride = (int32_t)value;
    else if (n == "sampled_listed_stride" && value >= -1 && value <= 1025) t.sampled_listed_stride = (int32_t)value;
    else if (n == "split_chunk" && value >= 0 && value <= (1 << 30)) t.split_chunk = (int32_t)value;
    else if (n == "count_first" && value >= -1 && value <= 1) t.count_first = (int32_t)value;
    else if (n == "lds_pad" && value >= 0 && value <= 160 * 1024) t.lds_pad = (int32_t)value;
    else return false;
    return true;
}
} // namespace

int32_t rpf_set_option(rpf_ctx *ctx, const char *name, int64_t value) {
    if (!ctx) return RPF_E_BADARG;
    if (!name) return fail(ctx, RPF_E_BADARG, "option name is NULL");
    const std::string n(name);
    if (!apply_option(ctx->tun, n, value)) return fail(ctx, RPF_E_BADARG, "unknown option or value out of range: " + n);
    ctx->bin_valid = false;
    return RPF_OK;
}

// whether rpf_set_option would take the pair; needs no context and no device (like rpf_layout_kernels)
int32_t rpf_check_option(const char *name, int64_t value) {
    if (!name) return RPF_E_BADARG;
    Tuning t;
    return apply_option(t, name, value) ? RPF_OK : RPF_E_BADARG;
}

int32_t rpf_filter(rpf_ctx *ctx, const rpf_desc *d, const void *planes, const float *ray_weight,
                   float *sample_rgb_out, float *pixel_rgb_out) {
    return rpf_filter_ex(ctx, d, planes, nullptr, ray_weight, sample_rgb_out, pixel_rgb_out, nullptr);
}

int32_t rpf_filter_ex(rpf_ctx *ctx, const rpf_desc *d, const void *planes, const double *colour64_in,
                      const float *ray_weight, float *sample_rgb_out, float *pixel_rgb_out, double *colour64_out) {
    int32_t st = enter(ctx, d, true);
    if (st) return st;
    if (!planes) return fail(ctx, RPF_E_BADARG, "planes is NULL");
    hipStream_t s = ctx->stream;
    const size_t ps = (size_t)d->W * d->H * d->S;
    if ((st = ensure_frame(ctx, d, ray_weight != nullptr, true))) return st;
    if ((st = ensure_outputs(ctx, d, sample_rgb_out != nullptr, pixel_rgb_out != nullptr))) return st;
    // the band pipeline needs asynchronous copies, i.e. page-locked buffers on the host side (rpf_host_alloc or the
    // caller's own hipHostMalloc / hipHostRegister); with pageable memory every copy blocks the submitting thread
    // and the serial order is faster (scripts/host_path.py)
    auto pinned = [](const void *p) {
        if (!p) return true;
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
        return a.type == hipMemoryTypeHost;
    };
    // (RPF_FLAG_SPIKE_CLAMP: no band may leave before delta is known; RPF_FLAG_PASS_REPORT: a pass reports on whole rows of both buffers)
    if (!(d->flags & (RPF_FLAG_TIMING | RPF_FLAG_NO_OVERLAP | RPF_FLAG_SPIKE_CLAMP | RPF_FLAG_PASS_REPORT)) && !colour64_in && !colour64_out &&
        pinned(planes) &&
        pinned(ray_weight) && pinned(sample_rgb_out) && pinned(pixel_rgb_out))
        return run_host_pipeline(ctx, d, planes, ray_weight, sample_rgb_out, pixel_rgb_out);
    // serial variant (per-kernel event timing needs it): upload, passes, download
    const double t0 = now_ms();
    {
        Range rg("rpf:upload");
        if ((st = upload_frame(ctx, d, planes, ray_weight, true, colour64_in, s))) return st;
        HIP_TRY(hipStreamSynchronize(s));
    }
    const double t1 = now_ms();
    const int32_t fst = run_passes(ctx, d, ctx->d_planes, ctx->d_colA, s);
    if (fst != RPF_OK && fst != RPF_E_NONFINITE) return fst;
    const double t2 = now_ms();
    if (colour64_out) {
        HIP_TRY(hipMemcpyAsync(colour64_out, ctx->d_colA, 3 * ps * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (sample_rgb_out || pixel_rgb_out) {
        Range rg("rpf:reduce + download");
        if ((st = download_rows(ctx, d, ctx->d_colA, ray_weight ? ctx->d_rayw.ptr : nullptr, 0, d->H, sample_rgb_out,
                                pixel_rgb_out, ps, 0, s, s, nullptr)))
            return st;
        HIP_TRY(hipStreamSynchronize(s));
    }
    ctx->counters.h2d_ms = (float)(t1 - t0);
    ctx->counters.d2h_ms = (float)(now_ms() - t2);
    return fst;
}

int32_t rpf_stage_pixel_stats(rpf_ctx *ctx, const rpf_desc *d, const void *planes, double *mean, double *stddev) {
    int32_t st = enter(ctx, d, false);
    if (st) return st;
    if (!planes || !mean || !stddev) return fail(ctx, RPF_E_BADARG, "NULL pointer");
    hipStream_t s = ctx->stream;
    const size_t ps = (size_t)d->W * d->H * d->S, HW = (size_t)d->W * d->H;
    const SampleLayout lay = layout_of(d);
    const int kNFeat = lay.nF;
    if ((st = ctx->d_pmean.ensure(ctx, HW * kNFeat * sizeof(double)))) return st;
    if ((st = ctx->d_pstd.ensure(ctx, HW * kNFeat * sizeof(double)))) return st;
    if ((st = upload_frame(ctx, d, planes, nullptr, false, nullptr, s))) return st;
    PassParams p{};
    p.lay = lay;
    p.generic = (d->flags & RPF_FLAG_GENERIC) ? kGenericOn : 0; // (stage 1a is the same kernel with and without RPF_FLAG_GENERIC_PACKED / _WAVE)
    p.W = d->W; p.H = d->H; p.S = d->S; p.policy = d->degenerate_policy;
    p.plane_stride = ps; p.planes = ctx->d_planes; p.pmean = ctx->d_pmean; p.pstd = ctx->d_pstd;
    HIP_TRY(launch_pixel_stats(p, s));
    std::vector<double> m(HW * kNFeat), sd(HW * kNFeat);
    HIP_TRY(hipMemcpyAsync(m.data(), ctx->d_pmean, m.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(sd.data(), ctx->d_pstd, sd.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t pix = 0; pix < HW; ++pix) // device planes are [12][H*W]; the ABI is pixel-major
        for (int k = 0; k < kNFeat; ++k) {
            mean[pix * kNFeat + k] = m[(size_t)k * HW + pix];
            stddev[pix * kNFeat + k] = sd[(size_t)k * HW + pix];
        }
    return RPF_OK;
}

int32_t rpf_filter_pass_debug(rpf_ctx *ctx, const rpf_desc *d, int32_t box, const void *planes,
                              const double *colour_in, double *colour_out, const rpf_debug *dbg) {
    int32_t st = enter(ctx, d, false);
    if (st) return st;
    if (!planes || !colour_out) return fail(ctx, RPF_E_BADARG, "NULL pointer");
    if ((st = check_sampled(ctx, d, 1))) return st; // pass id pass_id0, draws[0]
    if ((st = check_member_test(ctx, d, 1))) return st;
    if ((st = check_schedule(ctx, d, &box, 1))) return st; // entry pass0
    if (d->flags & RPF_FLAG_SPIKE_CLAMP)
        return fail(ctx, RPF_E_UNSUPPORTED, "RPF_FLAG_SPIKE_CLAMP with rpf_filter_pass_debug: the spike pass follows the last pass of "
                                            "a whole call (rpf_filter / _ex / _device / _film); this entry point returns one pass's raw colours");
    hipStream_t s = ctx->stream;
    const size_t ps = (size_t)d->W * d->H * d->S, HW = (size_t)d->W * d->H;
    const SampleLayout lay = layout_of(d);
    const size_t kNDim = (size_t)lay.ndim(), kNFeat = (size_t)lay.nF, kNPair = (size_t)lay.npair();
    if ((st = ctx->d_colB.ensure(ctx, 3 * ps * sizeof(double)))) return st;
    if ((st = upload_frame(ctx, d, planes, nullptr, true, colour_in, s))) return st;
    // debug planes
    const size_t dbg_bytes[9] = {HW * 4, HW * kNDim * 8, HW * kNDim * 8, HW * kNPair * 8, HW * 3 * 8,
                                 HW * kNFeat * 8, HW * 8, HW * kNDim * 4, HW * 4};
    void *host_dbg[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (dbg) {
        void *tmp[9] = {dbg->nbhd_size, dbg->mean, dbg->stddev, dbg->mi, dbg->alpha, dbg->beta, dbg->wrc,
                        dbg->bin_hash, dbg->member_hash};
        std::memcpy(host_dbg, tmp, sizeof(tmp));
    }
    rpf_debug dev{};
    void **dev_slots[9] = {(void **)&dev.nbhd_size, (void **)&dev.mean, (void **)&dev.stddev, (void **)&dev.mi,
                           (void **)&dev.alpha, (void **)&dev.beta, (void **)&dev.wrc, (void **)&dev.bin_hash,
                           (void **)&dev.member_hash};
    for (int i = 0; i < 9; ++i) {
        if (!host_dbg[i]) continue;
        if ((st = ctx->d_dbg[i].ensure(ctx, dbg_bytes[i]))) return st;
        HIP_TRY(hipMemsetAsync(ctx->d_dbg[i], 0, dbg_bytes[i], s));
        *dev_slots[i] = ctx->d_dbg[i];
    }
    if ((st = begin_call(ctx, s))) return st;
    // RPF_FLAG_PASS_REPORT: entry 0, from the caller's alpha / beta / W_r_c planes where they were asked for, scratch planes where not
    const bool report = (d->flags & RPF_FLAG_PASS_REPORT) != 0;
    if (report && (st = report_planes(ctx, d, dev, s))) return st;
    PassSetup ps_;
    if ((st = setup_pass(ctx, d, box, 0, ctx->d_planes, ctx->d_colA, ctx->d_colB, &dev, ps_))) return st;
    HIP_TRY(launch_copy_f64(ctx->d_colA, ctx->d_colB, 3 * ps, s));
    const bool timing = (d->flags & RPF_FLAG_TIMING) != 0;
    HIP_TRY(launch_pixel_stats(ps_.p, s));
    if (timing) HIP_TRY(hipEventRecord(ctx->ev[0], s));
    rpf_counters &c = ctx->counters;
    if ((st = route_pass(ctx, ps_.p, s, &c.filter_kernel_launches))) return st;
    if (timing) HIP_TRY(hipEventRecord(ctx->ev[1], s));
    if (report && (st = report_pass(ctx, d, 0, box, ctx->d_colA, ctx->d_colB, dev, s))) return st;
    HIP_TRY(hipMemcpyAsync(colour_out, ctx->d_colB, 3 * ps * sizeof(double), hipMemcpyDeviceToHost, s));
    if (dbg && dbg->nbhd_size) // N is always produced in the context's own plane
        HIP_TRY(hipMemcpyAsync(ctx->d_dbg[0], ctx->d_nbhd, HW * 4, hipMemcpyDeviceToDevice, s));
    for (int i = 0; i < 9; ++i)
        if (host_dbg[i]) HIP_TRY(hipMemcpyAsync(host_dbg[i], ctx->d_dbg[i], dbg_bytes[i], hipMemcpyDeviceToHost, s));
    const int32_t fst = finish_counters(ctx, d, 1, s); // one pass; synchronises
    if (fst != RPF_OK && fst != RPF_E_NONFINITE) return fst;
    if (timing) HIP_TRY(hipEventElapsedTime(&c.filter_kernel_ms, ctx->ev[0], ctx->ev[1]));
    return fst;
}

int32_t rpf_feature_images(rpf_ctx *ctx, const rpf_desc *d, const void *planes, double *images_out) {
    int32_t st = enter(ctx, d, false);
    if (st) return st;
    if (!planes || !images_out) return fail(ctx, RPF_E_BADARG, "NULL pointer");
    if (!layout_of(d).is_ref19()) return fail(ctx, RPF_E_UNSUPPORTED, "visualizeSF's six images are defined for the reference's 19-dim layout");
    hipStream_t s = ctx->stream;
    const size_t HW = (size_t)d->W * d->H;
    if ((st = ctx->d_dbg[1].ensure(ctx, (18 * HW + 18) * sizeof(double)))) return st;
    double *d_img = static_cast<double *>(ctx->d_dbg[1].ptr);
    unsigned long long *d_max = (unsigned long long *)(d_img + 18 * HW);
    if ((st = upload_frame(ctx, d, planes, nullptr, false, nullptr, s))) return st;
    HIP_TRY(launch_feature_images(reinterpret_cast<const float *>(ctx->d_planes.ptr), d->W, d->H, d->S, d_img, d_max, s));
    HIP_TRY(hipMemcpyAsync(images_out, d_img, 18 * HW * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return RPF_OK;
}

int32_t rpf_selftest_udiv(rpf_ctx *ctx, uint64_t n, uint64_t seed, int32_t mode, uint64_t *mismatches) {
    if (!ctx || !mismatches) return RPF_E_BADARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemsetAsync(ctx->d_nred, 0, 2 * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(launch_udiv_selftest(n, seed, mode, ctx->d_nred, ctx->stream));
    unsigned long long r = 0;
    HIP_TRY(hipMemcpyAsync(&r, ctx->d_nred, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *mismatches = r;
    return RPF_OK;
}

int32_t rpf_query_counters(rpf_ctx *ctx, rpf_counters *out) {
    if (!ctx || !out) return RPF_E_BADARG;
    *out = ctx->counters;
    return RPF_OK;
}

int32_t rpf_query_nbhd(rpf_ctx *ctx, int32_t *nbhd_out, int64_t count) {
    if (!ctx) return RPF_E_BADARG;
    if (!nbhd_out || count <= 0) return fail(ctx, RPF_E_BADARG, "nbhd_out is NULL or count <= 0");
    if (!ctx->d_nbhd || (size_t)count * sizeof(int32_t) > ctx->d_nbhd.cap)
        return fail(ctx, RPF_E_BADARG, "no neighbourhood plane of that size: run a filter call first (count = W*H)");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpy(nbhd_out, ctx->d_nbhd, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RPF_OK;
}

int32_t rpf_query_route(rpf_ctx *ctx, int32_t *route_out) {
    if (!ctx) return RPF_E_BADARG;
    if (!route_out) return fail(ctx, RPF_E_BADARG, "route_out is NULL");
    *route_out = ctx->last_route;
    return RPF_OK;
}

} // extern "C"
