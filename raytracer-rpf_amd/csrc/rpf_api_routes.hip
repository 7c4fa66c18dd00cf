// rpf_api_routes.hip -- the pass router of the C ABI: route_pass, which runs one filter pass on the route its flags, its sizes
// and the options pick, and what only the routes use -- the slot rules of the streaming and wide kernels, the redo list, the
// class launches, count_and_deal, the one count-and-deal step of the listed-member routes 7, 8, 9 and 12, and binned_params /
// deal_classes / filter_classes, the steps the routes behind a mask-leaving count pass share (2, 10 and 11).  Host code only;
// rpf_api.hip prepares a pass (setup_pass) and calls route_pass from its pass loops.
#include <hip/hip_runtime.h>

#include <cstring>

#include "rpf_api.h"

namespace rpf {

namespace {

// How many workgroups (= scratch slots) a launch of the streaming or the wide kernel gets, for a slot of nmax members at
// 4 + bin_bytes * ndim bytes each (a u32 list entry and one bin id per column: one byte on the streaming kernel, two on the wide
// one): min(pixels, max(lo, min(hi, budget / bytes of a slot))) -- or min(pixels, resident) where the streaming kernel's carve-up
// keeps member list and bin ids in LDS and the rule names a count for that (kSameWhenResident: it does not)
struct SlotRule {
    uint32_t resident, lo, hi, bin_bytes;
    size_t budget;
};
constexpr uint32_t kSameWhenResident = 0;        // SlotRule::resident: the carve-up does not change the rule
constexpr uint64_t kCountOnDevice = UINT64_MAX;  // `pixels` of a launch: the list size is on the device, nothing to clamp to
constexpr SlotRule kPassSlots = {2048, 64, 1024, 1, (size_t)1 << 30};           // resident: eight workgroups on each of 256 CUs
constexpr SlotRule kRedoSlots = {kSameWhenResident, 8, 128, 1, (size_t)64 << 20}; // a fixed small grid: ordinary frames leave the list empty
constexpr SlotRule kBinnedSlots = {kSameWhenResident, 1024, 1024, 1, 0};        // the streaming class of the size-binned route: 1024, no budget
constexpr SlotRule kWideSlots = {kSameWhenResident, 1, 1024, 2, (size_t)1 << 30};    // kPassSlots without its floor
constexpr SlotRule kWideRedoSlots = {kSameWhenResident, 8, 64, 2, (size_t)256 << 20}; // as kRedoSlots, for slots of up to 21 MiB

uint32_t slot_count(const SlotRule &rule, const PassParams &p, uint64_t pixels) {
    uint64_t slots = rule.resident;
    if (rule.resident == kSameWhenResident || !generic_carve(p.lay, p.nmax).resident) {
        const size_t per_slot = (size_t)p.nmax * (4 + (size_t)rule.bin_bytes * p.lay.ndim());
        slots = std::max<size_t>(rule.lo, std::min<size_t>(rule.hi, rule.budget / per_slot));
    }
    return (uint32_t)std::min<uint64_t>(pixels, slots);
}

// the slots' scratch in HBM: member lists [slots][nmax] u32 and bin ids [slots][ndim][nmax] of bin_bytes each; none when the
// streaming kernel's carve-up holds them in LDS (the wide kernel's never does)
int32_t ensure_slot_scratch(rpf_ctx *ctx, const PassParams &p, uint32_t slots, uint32_t bin_bytes) {
    if (bin_bytes == 1 && generic_carve(p.lay, p.nmax).resident) return RPF_OK;
    int32_t st;
    if ((st = ctx->d_big_list.ensure(ctx, (size_t)slots * p.nmax * 4))) return st;
    return ctx->d_big_bins.ensure(ctx, (size_t)slots * p.nmax * p.lay.ndim() * bin_bytes);
}

// One launch of the streaming kernel over p's rows or pixel list (`pixels` of them; kCountOnDevice with count_dev: the list size
// is read on the device and the grid is the rule's slots): the slots by `rule`, the scratch, the launch, counted in *launches.
// fast: the fp32 stage 4 of RPF_FLAG_STREAM_FAST; listed: the LISTED instantiation (the rest launch of a sampled pass)
int32_t launch_streaming(rpf_ctx *ctx, const PassParams &p, uint64_t pixels, const SlotRule &rule, const uint32_t *count_dev,
                         hipStream_t s, int *launches, bool fast, bool listed = false) {
    const uint32_t slots = slot_count(rule, p, pixels);
    int32_t st;
    if ((st = ensure_slot_scratch(ctx, p, slots, rule.bin_bytes))) return st;
    HIP_TRY(generic::launch_filter(p, ctx->d_big_list, ctx->d_big_bins, slots, count_dev, s, fast, listed));
    if (launches) ++*launches;
    return RPF_OK;
}

// The same for the wide kernel.  The table: T_w (2^-41), or -- a forced pass below 48586 samples, where that one is exact and
// three bits finer -- the 2^-44 table of the other kernels, so that such a pass gives route 3's bits.  member: the table of
// RPF_FLAG_MEMBER_TEST for the kernel's own stage 1b (route 9's rest launch), or null
int32_t launch_wide(rpf_ctx *ctx, const PassParams &p, uint64_t pixels, const SlotRule &rule, const uint32_t *count_dev,
                    hipStream_t s, int *launches, bool fast, const double *member) {
    const uint32_t slots = slot_count(rule, p, pixels);
    int32_t st;
    if ((st = ensure_slot_scratch(ctx, p, slots, rule.bin_bytes))) return st;
    const bool fine = p.nmax <= kTFixExact;
    if (!fine && (!ctx->d_twide || ctx->twide_n < p.nmax + 1)) return fail(ctx, RPF_E_BADARG, "wide pass without its table (setup_pass builds it)");
    HIP_TRY(generic::launch_filter_wide(p, ctx->d_big_list, ctx->d_big_bins, slots, fine ? ctx->d_tfix.ptr : ctx->d_twide.ptr,
                                        fine ? 44 : kTWideBits, count_dev, s, fast, member));
    if (launches) ++*launches;
    return RPF_OK;
}

// REF_ABORT: the pixels the resident kernels appended to the redo list (an MI table inside the fixed-point rounding band at
// a non-power-of-two N: the reference returns rounding residue there, rpf_filter_impl.inc stage 3b) are filtered again,
// whole, by the streaming kernel, which evaluates the reference's floating-point expression for such tables.  The list
// size stays on the device (no read-back): a fixed small grid whose workgroups find the list empty on ordinary frames.
int32_t launch_redo(rpf_ctx *ctx, const PassParams &p, hipStream_t s, int *launches) {
    if (p.redo_list == nullptr) return RPF_OK;
    Range rg("rpf:redo (reference-expression kernel)");
    PassParams q = p;
    q.pix_list = p.redo_list;
    q.list_count = 0;
    return launch_streaming(ctx, q, kCountOnDevice, kRedoSlots, p.redo_count, s, launches, false); // a redone pixel is fp64 under every flag
}

// A route_pass call begins under p's policy.  REF_ABORT: the call takes the next of the pass's redo counts (setup_pass starts a pass
// at the first) and zeroes it, whether or not the route keeps a list: a pass filtered band by band (rpf_filter's row-band pipeline)
// gives every band a count of its own -- the list size its redo launch reads on the device -- and finish_counters adds up those of
// the last pass.  A route that keeps a list gets d_redo_list and p pointed at it and at that count.  Otherwise p names none.
int32_t begin_redo(rpf_ctx *ctx, PassParams &p, bool keeps_list, hipStream_t s) {
    p.redo_list = nullptr; p.redo_count = nullptr;
    if (p.policy != RPF_DEGEN_REF_ABORT) return RPF_OK;
    if (ctx->redo_used >= kRedoCounts) return fail(ctx, RPF_E_BADARG, "a pass cut into more row bands than it has redo counts");
    uint32_t *count = ctx->d_redo_count + ctx->redo_used++;
    HIP_TRY(hipMemsetAsync(count, 0, sizeof(uint32_t), s));
    if (!keeps_list) return RPF_OK;
    int32_t st;
    if ((st = ctx->d_redo_list.ensure(ctx, (size_t)p.W * p.H * sizeof(uint32_t)))) return st;
    p.redo_list = ctx->d_redo_list; p.redo_count = count;
    return RPF_OK;
}

// u64 acceptance masks per pixel: one bit per candidate of the window (the pixel's own samples are members without a test)
uint32_t mask_stride(const PassParams &p) {
    return (uint32_t)std::max<int64_t>(1, ((int64_t)(p.box * p.box - 1) * p.S + 63) / 64);
}

// the launch of size class c: the kernel family of that capacity walks the class's pixel list
PassParams class_params(const rpf_ctx *ctx, const PassParams &p, int c, uint32_t list_count) {
    PassParams q = p;
    q.nmax = std::min(p.nmax, class_capacity(c));
    q.bmax = bmax_of(q.nmax);
    q.pix_list = ctx->d_lists + (size_t)c * p.W * p.H;
    q.list_count = list_count;
    return q;
}

// The unbinned route (box*box*S <= 512): the fused kernel, or stage 1b first, and the packed kernels behind either.
int32_t route_unbinned(rpf_ctx *ctx, const PassParams &p, bool packed, hipStream_t s, int *launches) {
    const size_t HW = (size_t)p.W * p.H;
    int32_t st;
    PassParams q = p;
    if (packed) {
        // the fused kernel finds N itself (stage 1b); a pixel with N <= 64 leaves its acceptance masks, joins the list of
        // its lane class and exits; the four packed launches read their list sizes on the device (no host read-back)
        q.mask_stride = mask_stride(p);
        if ((st = ctx->d_lists.ensure(ctx, (size_t)kNumClasses * HW * sizeof(uint32_t)))) return st;
        if ((st = ctx->d_masks.ensure(ctx, HW * q.mask_stride * sizeof(uint64_t)))) return st;
        HIP_TRY(hipMemsetAsync(ctx->d_class_counts, 0, kNumClasses * sizeof(uint32_t), s));
        q.reroute_masks = ctx->d_masks;
    }
    // Two routes, same results (tests: option "count_first" 0 / 1).  FUSED: filter_pixel_kernel runs stage 1b itself (its
    // twelve gathers per candidate hide behind the other stages of the pixels in flight) and re-routes the pixels it finds
    // small; the route of buffers whose neighbourhoods are large (the headline generator: N = 296 of 392).  COUNT FIRST:
    // stage 1b for the whole slab as its own launch (nbhd_count_kernel, two phases: a path-traced buffer rejects most
    // candidates on the first features), then the pixels are dealt by N -- the four packed lists, and the rest (N > 64) into
    // the list the fused kernel walks, rebuilding its member list from the masks; the route of buffers whose neighbourhoods
    // are small, where a one-wave workgroup per pixel that only finds out it has nothing to do is the whole cost (6.2 vs
    // 2.7 ms per 1080p frame).  Which one: a probe -- the test on a lattice of every 32nd pixel of every 32nd row (~2000
    // pixels of a 1080p frame, ~20 us + a 4-byte read-back): count first when half of them have N <= 64.
    uint32_t *glist = ctx->d_lists + (size_t)(kNumClasses - 1) * HW, *gcount = ctx->d_class_counts + (kNumClasses - 1);
    uint32_t *pcount = ctx->d_class_counts + kNumClasses;
    const uint32_t npix = (uint32_t)((size_t)(p.row_end - p.row_begin) * p.W);
    bool run_main = true;
    int count_first = packed ? ctx->tun.count_first : 0;
    uint32_t n_general = npix;
    // (the packed kernels are what filters the pixels the prelist leaves out: above 64 spp their N = S fits no packed class,
    // so every pixel goes to the fused kernel, which proves a flat pixel's N = S itself -- flat_quad_shortcut)
    const bool prelisted = packed && ctx->flat_fresh && p.S <= class_capacity(kNumPacked - 1);
    if (packed && (count_first < 0 || prelisted)) {
        // pixels that stage 1a proved flat (a zero-variance feature, no NaN mean in the buffer: N = S) never reach the fused
        // kernel or the count pass: the others are listed in slab order (the list of the streaming class is free on this
        // route): a one-wave workgroup per flat pixel that only finds out it has nothing to do cost 5.8 ms per 1080p frame
        // of a captured-like buffer.
        Range rg("rpf:route probe + prelist (flat quads)");
        uint32_t probe[2] = {0, 0};
        const int step = 32;
        PassParams pr = q; // the probe's rows: the call's, or those the band pipeline names (rpf_ctx::probe_r0)
        if (ctx->probe_r1 > ctx->probe_r0) { pr.row_begin = ctx->probe_r0; pr.row_end = ctx->probe_r1; }
        if (count_first < 0) {
            pr.masks = nullptr; pr.reroute_masks = nullptr;
            if (!ctx->flat_fresh) pr.flat = nullptr;
            HIP_TRY(hipMemsetAsync(pcount, 0, 2 * sizeof(uint32_t), s));
            HIP_TRY(launch_nbhd_count(pr, step, pcount, nullptr, nullptr, 0, s));
            HIP_TRY(hipMemcpyAsync(probe, pcount, sizeof(probe), hipMemcpyDeviceToHost, s));
        }
        if (prelisted) {
            HIP_TRY(launch_prelist(q, glist, gcount, s));
            HIP_TRY(hipMemcpyAsync(&n_general, gcount, sizeof(n_general), hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipStreamSynchronize(s)); // one read-back for both
        if (count_first < 0) {
            const uint32_t n_probe = (uint32_t)((p.W + step - 1) / step) * (uint32_t)((pr.row_end - pr.row_begin + step - 1) / step);
            const uint32_t n_probe_general = n_probe - std::min(n_probe, probe[1]);
            count_first = (n_probe_general != 0 && 2u * probe[0] >= n_probe_general) ? 1 : 0; // (only flat pixels: nothing to count)
        }
    }
    ctx->last_route = count_first == 1 ? kRouteCountFirst : kRouteFused;
    if (count_first == 1 && n_general != 0) {
        Range rg("rpf:stage 1b + classify");
        uint32_t *rlist = ctx->d_lists + (size_t)(kNumClasses - 2) * HW, *rcount = ctx->d_class_counts + (kNumClasses - 2);
        uint32_t n_rest = 0;
        q.reroute_masks = nullptr;
        q.masks = ctx->d_masks;
        if (!ctx->flat_fresh) q.flat = nullptr;
        if (prelisted && n_general < npix) { HIP_TRY(launch_nbhd_count(q, 1, nullptr, glist, gcount, n_general, s)); }
        else { HIP_TRY(launch_nbhd_count(q, 1, nullptr, nullptr, nullptr, 0, s)); }
        HIP_TRY(launch_classify(q, ctx->d_lists, ctx->d_class_counts, kNumPacked, kNumClasses - 2, s));
        HIP_TRY(hipMemcpyAsync(&n_rest, rcount, sizeof(n_rest), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s)); // the fused kernel's grid
        if (n_rest != 0) { q.pix_list = rlist; q.list_count = n_rest; }
        else run_main = false;
    } else if (prelisted) {
        if (n_general == 0) run_main = false;
        else if (n_general < npix) { q.pix_list = glist; q.list_count = n_general; }
    }
    if (run_main) {
        Range rg("rpf:filter_pixel_kernel");
        HIP_TRY(launch_filter_pass(q, ctx->tun, s, nullptr));
        if (launches) ++*launches;
    }
    q.pix_list = nullptr; q.list_count = 0;
    if (packed) {
        Range rg("rpf:packed kernels (N <= 8, 16, 32, 64)");
        if (!(count_first == 1 && n_general != 0)) { HIP_TRY(launch_classify(q, ctx->d_lists, ctx->d_class_counts, kNumPacked, -1, s)); }
        for (int c = 0; c < kNumPacked; ++c) {
            if (p.S > class_capacity(c)) continue; // N >= S: the list is empty by construction
            PassParams r = class_params(ctx, q, c, npix); // npix: an upper bound, it sizes the grid
            r.reroute_masks = nullptr;
            r.masks = ctx->d_masks;
            HIP_TRY(launch_filter_packed(r, class_capacity(c), ctx->d_class_counts + c, s));
            if (launches) ++*launches;
        }
    }
    return launch_redo(ctx, p, s, launches);
}

// What the passes that run the compiled class kernels behind a count pass share (routes 2, 10 and 11): the buffers, the deal and
// the class loop.  binned_params: p's copy with the class lists, the acceptance masks (one u64 per 64 candidates of the window,
// which the count pass keeps so that the filter kernels only rebuild the list) and, where the 32- / 64-spp classes run as three
// kernels, the hand-over buffer.
int32_t binned_params(rpf_ctx *ctx, const PassParams &p, PassParams &pc) {
    const size_t HW = (size_t)p.W * p.H;
    int32_t st;
    if ((st = ctx->d_lists.ensure(ctx, (size_t)kNumClasses * HW * sizeof(uint32_t)))) return st;
    pc = p;
    pc.mask_stride = mask_stride(p);
    if ((st = ctx->d_masks.ensure(ctx, HW * pc.mask_stride * sizeof(uint64_t)))) return st;
    pc.masks = ctx->d_masks;
    pc.carry = nullptr;
    if (p.nmax > class_capacity(kNumClasses - 4) && p.nmax <= kMaxResident && ctx->tun.split_weights != 0) {
        // the 32- and 64-spp classes run as three kernels (chains; bins + MI; weights): per-pixel hand-over buffer
        if ((st = ctx->d_carry.ensure(ctx, HW * (size_t)kCarryStride * sizeof(double)))) return st;
        pc.carry = ctx->d_carry;
    }
    return RPF_OK;
}

// ... the deal behind the count launch (d_class_counts zeroed ahead of it): the pixels into the eleven class lists by the N the
// count pass left, and the list sizes read back (one synchronisation of s)
int32_t deal_classes(rpf_ctx *ctx, const PassParams &pc, uint32_t counts[kNumClasses], hipStream_t s) {
    HIP_TRY(launch_classify(pc, ctx->d_lists, ctx->d_class_counts, kNumClasses, -1, s));
    HIP_TRY(hipMemcpyAsync(counts, ctx->d_class_counts, kNumClasses * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return RPF_OK;
}

// ... and one launch per non-empty class, then the redo launch.  member: route 10's table (its streaming class is the wide
// kernel's), else null
int32_t filter_classes(rpf_ctx *ctx, const PassParams &pc, bool packed, const double *member, const uint32_t counts[kNumClasses],
                       hipStream_t s, int *launches) {
    int32_t st;
    // the four-wave kernels keep one acceptance mask per 64 candidates of the WINDOW in a 64-entry LDS array: windows
    // beyond 4096 candidates (boxes 17 and up) run their resident classes on the one-wave instantiations
    // (a listed pass, route 12, has no such array: its "auto" is the classes' own choice at every window)
    Tuning tun = ctx->tun;
    if (!(pc.generic & kGenericSampledListed) && (int64_t)(pc.box * pc.box - 1) * pc.S > 4096) tun.waves_per_pixel = 1;
    for (int c = 0; c < kNumClasses; ++c) {
        if (counts[c] == 0) continue;
        static const char *const kClassName[kNumClasses] = {
            "rpf:filter class N<=8", "rpf:filter class N<=16", "rpf:filter class N<=32", "rpf:filter class N<=64",
            "rpf:filter class N<=128", "rpf:filter class N<=256", "rpf:filter class N<=448",
            "rpf:filter class N<=832", "rpf:filter class N<=1600", "rpf:filter class N<=3136", "rpf:filter class streaming"};
        Range rg(kClassName[c]);
        const PassParams q = class_params(ctx, pc, c, counts[c]);
        if (c == kNumClasses - 1 && member) { // ... under the configured test: the wide kernel runs its own stage 1b on the table
            PassParams w = scheduled_stream(q); // (a scheduled pass: the wide kernel forms its stage 3c on kGenericSchedule)
            w.masks = nullptr; w.mask_stride = 0; w.carry = nullptr;
            w.redo_list = nullptr; w.redo_count = nullptr;
            if ((st = launch_wide(ctx, w, counts[c], kWideSlots, nullptr, s, launches, false, member))) return st;
            continue;
        }
        if (c == kNumClasses - 1) { // neighbourhoods beyond the LDS-resident kernels: stream through global scratch (fp64 under every flag)
            // (a scheduled pass: generic::filter_pixel_kernel forms its stage 3c on kGenericSchedule, the one bit of `generic` it reads)
            if ((st = launch_streaming(ctx, scheduled_stream(q), counts[c], kBinnedSlots, nullptr, s, launches, false))) return st;
            continue;
        }
        if (c < kNumPacked && packed) { HIP_TRY(launch_filter_packed(q, class_capacity(c), nullptr, s)); }
        else { HIP_TRY(launch_filter_pass(q, tun, s, nullptr)); }
        if (launches) ++*launches;
    }
    return launch_redo(ctx, pc, s, launches);
}

// The size-binned route: the neighbourhood sizes are counted first, then every kernel family filters the list of its class.
// member: null on route 2; the uploaded table on route 10 (route_member_fused below), the same structure
// with three differences.  The count launch is the MEMBER form of nbhd_count_kernel, which gets stage 1a's flat plane only when
// the flat proof is sound under the table (every floor below n_feat negative).  The streaming class N > 3136 repeats stage 1b,
// so it runs on the kernel that does so under the same test: the wide kernel's MEMBER instantiation over the class's list, route
// 9's rest launch (launch_wide: the 2^-44 table where that is exact, kWideSlots).  The membership cache is keyed by whose masks
// it holds (bin_member): a route-10 pass is served by a route-10 pass only, a route-2 pass by a route-2 pass only.
int32_t route_binned(rpf_ctx *ctx, const PassParams &p, bool packed, const double *member, hipStream_t s, int *launches) {
    int32_t st;
    ctx->last_route = member ? kRouteMemberFused : kRouteBinned;
    PassParams pc;
    if ((st = binned_params(ctx, p, pc))) return st;
    uint32_t counts[kNumClasses];
    if (ctx->bin_valid && ctx->bin_member == (member != nullptr) && ctx->bin_box == p.box && ctx->bin_r0 == p.row_begin && ctx->bin_r1 == p.row_end) {
        std::memcpy(counts, ctx->bin_counts, sizeof(counts));
    } else {
        Range rg(member ? "rpf:count + classify (configured membership test, size classes)" : "rpf:count + classify (stage 1b test, size classes)");
        ctx->bin_valid = false;
        ctx->bin_member = member != nullptr;
        HIP_TRY(hipMemsetAsync(ctx->d_class_counts, 0, kNumClasses * sizeof(uint32_t), s));
        if (member) {
            // p.flat says "some feature has sigma * 3 == 0 and a finite mean": N = S under the configured test exactly where that
            // feature's floor is negative, and the plane does not say which feature it was
            PassParams pm = pc;
            bool sound = ctx->flat_fresh;
            for (int k = 0; k < p.lay.nF; ++k) sound = sound && ctx->membership.floor[k] < 0.0;
            if (!sound) pm.flat = nullptr;
            HIP_TRY(launch_nbhd_count_member(pm, member, s));
        } else {
            HIP_TRY(launch_nbhd_count(pc, 1, nullptr, nullptr, nullptr, 0, s));
        }
        if ((st = deal_classes(ctx, pc, counts, s))) return st;
        std::memcpy(ctx->bin_counts, counts, sizeof(counts));
        ctx->bin_box = p.box; ctx->bin_r0 = p.row_begin; ctx->bin_r1 = p.row_end;
        ctx->bin_valid = true;
    }
    return filter_classes(ctx, pc, packed, member, counts, s, launches);
}

// The layout-generic route (RPF_FLAG_GENERIC): one launch per pass, every neighbourhood size on the same kernel; member
// lists and bin ids in LDS, or -- when generic_carve says they do not fit -- in the streaming kernel's HBM slots.  No redo
// list: the kernel evaluates the reference's MI expression in place.  None of the rpf_set_option names applies here.
int32_t route_generic(rpf_ctx *ctx, const PassParams &p, hipStream_t s, int *launches) {
    Range rg("rpf:generic filter kernel");
    ctx->last_route = kRouteGeneric;
    if (p.row_end <= p.row_begin) return RPF_OK;
    return launch_streaming(ctx, p, (uint64_t)(p.row_end - p.row_begin) * p.W, kPassSlots, nullptr, s, launches, stream_fast(p));
}

// The wide route (RPF_FLAG_WIDE_NBHD on a pass with box*box*S > 65535, or option "wide" = 1): one launch per pass, every pixel
// on generic::filter_wide_kernel; no count pass, no classes, no redo list (the kernel evaluates the reference's MI expression
// in place).  Member lists (u32) and bin ids (u16) in HBM slots by kWideSlots: at most 1024, within 1 GiB, never more than pixels.
int32_t route_wide(rpf_ctx *ctx, const PassParams &p, hipStream_t s, int *launches) {
    Range rg("rpf:wide filter kernel");
    ctx->last_route = kRouteWide;
    if (p.row_end <= p.row_begin) return RPF_OK;
    return launch_wide(ctx, p, (uint64_t)(p.row_end - p.row_begin) * p.W, kWideSlots, nullptr, s, launches, stream_fast(p), nullptr);
}

constexpr int kNumWave = 8;                   // classes 0 .. 3 packed, 4 .. 7 one wave per pixel (capacities 128, 256, 448, 832)
constexpr int kNumQuad = 10;                  // ... 8 and 9 four waves per pixel (capacities 1600, 3136; route 13 only)
constexpr int kRestClass = kNumClasses - 1;   // the list of the pixels no class kernel of a generic route takes

// One launch per non-empty list of the classes 0 .. n_classes - 1 of p's pass: generic::filter_packed_kernel below kNumPacked,
// generic::filter_wave_kernel below kNumWave, else (route 13) generic::filter_quad_kernel, which is fp64 only.  fast: the fp32
// stage 4 of the first two -- class_fast on routes 4 / 5, stream_fast on route 7
int32_t launch_classes(rpf_ctx *ctx, const PassParams &p, const uint32_t *counts, int n_classes, bool fast, const char *packed_label,
                       const char *wave_label, hipStream_t s, int *launches) {
    for (int c = 0; c < n_classes; ++c) {
        if (counts[c] == 0) continue;
        Range rg(c < kNumPacked ? packed_label : (c < kNumWave ? wave_label : "rpf:generic quad class"));
        PassParams q = p;
        q.pix_list = ctx->d_lists + (size_t)c * p.W * p.H;
        q.list_count = counts[c];
        if (c < kNumPacked) { HIP_TRY(generic::launch_filter_packed(q, class_capacity(c), s, fast)); }
        else if (c >= kNumWave) { HIP_TRY(generic::launch_filter_quad(q, class_capacity(c), s)); }
        else { HIP_TRY(generic::launch_filter_wave(q, class_capacity(c), s, fast)); }
        if (launches) ++*launches;
    }
    return RPF_OK;
}

// What the listed-member routes 7, 8 and 9 differ in at their count-and-deal step
struct ListedPass {
    // the first count launch is offered what the grow-only pool already holds, not 8 entries per pixel only: routes 8 and 9 list
    // hundreds of members per pixel where route 7 lists a handful, and so the repeat is paid by the first pass of that size only,
    // not by every pass of every call
    bool held_pool;
    const char *count_label;   // the roctx range of the step
    const char *overflow_msg;  // the refusal when the pool overflows at its exact size
    // the deal (launch_classify's max_class and rest_class): the eight classes of route 5 and a rest class on routes 7, 8 and 9, the
    // eleven classes of route 2 on route 12
    int max_class = kNumWave, rest_class = kRestClass;
};

// The count-and-deal step of a listed-member pass over p's rows (not empty): `count` -- hipError_t(const PassParams &, const
// generic::MemberPool &, hipStream_t), the route's count kernel -- lists each pixel's members behind its own samples into the
// member pool behind one cursor and writes N; the pixels are dealt into the eight classes of route 5 and a rest class (route 12:
// lp's deal, the eleven classes of route 2); one
// read-back brings the list sizes (counts) and the cursor.  The pool holds `wide_pool` entries (option), else 8 per pixel of the
// slab or, where lp says so, what it already holds if that is more; when the cursor says the data needed more, the pool is grown
// to exactly that and the count and the deal are repeated, once: the cursor ends at the sum of N - S over the listed pixels
// whatever the capacity was.  Leaves p without acceptance masks and with members / member_base pointing at the pool.
template <class Count>
int32_t count_and_deal(rpf_ctx *ctx, PassParams &p, const ListedPass &lp, Count &&count, uint32_t counts[kNumClasses], hipStream_t s) {
    const size_t HW = (size_t)p.W * p.H;
    int32_t st;
    p.masks = nullptr; p.mask_stride = 0;
    if ((st = ctx->d_lists.ensure(ctx, (size_t)kNumClasses * HW * sizeof(uint32_t)))) return st;
    if ((st = ctx->d_wc_base.ensure(ctx, HW * sizeof(uint64_t)))) return st;
    if ((st = ctx->d_wc_cursor.ensure(ctx, 2 * sizeof(unsigned long long)))) return st;
    uint64_t capacity = 8 * (uint64_t)(p.row_end - p.row_begin) * p.W;
    if (lp.held_pool && ctx->d_wc_pool.ptr) capacity = std::max<uint64_t>(capacity, ctx->d_wc_pool.cap / sizeof(uint32_t));
    if (ctx->tun.wide_pool >= 0) capacity = (uint64_t)ctx->tun.wide_pool;
    for (int attempt = 0;; ++attempt) {
        Range rg(lp.count_label);
        if ((st = ctx->d_wc_pool.ensure(ctx, (size_t)std::max<uint64_t>(capacity, 1) * sizeof(uint32_t)))) return st;
        unsigned long long used = 0;
        HIP_TRY(hipMemsetAsync(ctx->d_class_counts, 0, kNumClasses * sizeof(uint32_t), s));
        HIP_TRY(count(p, generic::MemberPool{ctx->d_wc_pool, capacity, ctx->d_wc_base, ctx->d_wc_cursor}, s));
        HIP_TRY(launch_classify(p, ctx->d_lists, ctx->d_class_counts, lp.max_class, lp.rest_class, s));
        HIP_TRY(hipMemcpyAsync(counts, ctx->d_class_counts, kNumClasses * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&used, ctx->d_wc_cursor, sizeof(used), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (used <= capacity) break;
        if (attempt != 0) return fail(ctx, RPF_E_HIP, lp.overflow_msg);
        capacity = used;
    }
    p.members = ctx->d_wc_pool; p.member_base = ctx->d_wc_base;
    return RPF_OK;
}

// A wide pass dealt by size class (RPF_FLAG_WIDE_NBHD | RPF_FLAG_WIDE_CLASSES, S <= 832): stage 1b as
// its own launch (generic::wide_count_kernel: N, and the members of every pixel with N <= 832 in a member pool), the pixels
// dealt into the eight classes of route 5 and a rest class, one read-back (the list sizes and the pool cursor),
// then one launch per non-empty class -- generic::filter_packed_kernel / filter_wave_kernel reading the listed members, with
// the 2^-44 table, exact for N <= 832 -- and the wide kernel over the rest list (N > 832; its own stage 1b, route 6's table).
// REF_ABORT: the class kernels' redo list goes to the wide kernel as well (generic::filter_pixel_kernel cannot hold the
// window), its size read on the device.  Pool capacity and growth: count_and_deal above (option "wide_pool"); which kernel
// filters a pixel never depends on the capacity.
// member: null on route 7; the uploaded table on route 9 (route_member_test below), the same structure with the count kernel's
// and the wide kernel's MEMBER instantiations.  The lists of this pass are no other pass's: the membership cache of the
// size-binned route neither serves it nor survives it (d_lists is overwritten).
int32_t route_wide_classes(rpf_ctx *ctx, const PassParams &p_in, const double *member, hipStream_t s, int *launches) {
    const size_t HW = (size_t)p_in.W * p_in.H;
    int32_t st;
    const ListedPass lp = {member != nullptr, "rpf:wide count + classify (stage 1b test, listed members, lane and wave classes)",
                           "wide count pass: the member pool overflowed at its exact size"};
    ctx->last_route = member ? kRouteMemberTest : kRouteWideClasses;
    PassParams p = p_in;
    if (p.row_end <= p.row_begin) return RPF_OK;
    uint32_t counts[kNumClasses];
    // (launch_wide_count zeroes the cursor and, in the cursor's second slot, the NaN flag of the flat-pixel proof itself)
    const auto count = [&](const PassParams &q, const generic::MemberPool &m, hipStream_t cs) {
        return generic::launch_wide_count(q, m, reinterpret_cast<int32_t *>(ctx->d_wc_cursor.ptr + 1), member, cs);
    };
    if ((st = count_and_deal(ctx, p, lp, count, counts, s))) return st;
    if ((st = launch_classes(ctx, p, counts, kNumWave, stream_fast(p), "rpf:wide pass, packed class", "rpf:wide pass, wave class", s, launches))) return st;
    PassParams w = p_in; // the wide kernel: as on route 6, over a list; it keeps no redo list of its own
    w.redo_list = nullptr; w.redo_count = nullptr;
    if (counts[kRestClass] != 0) {
        Range rg("rpf:wide filter kernel (N > 832)");
        w.pix_list = ctx->d_lists + (size_t)kRestClass * HW;
        w.list_count = counts[kRestClass];
        if ((st = launch_wide(ctx, w, w.list_count, kWideSlots, nullptr, s, launches, stream_fast(p), member))) return st;
    }
    if (p.redo_list != nullptr) {
        Range rg("rpf:redo (wide kernel)");
        w.pix_list = p.redo_list;
        w.list_count = 0;
        // (a fixed small grid whose workgroups find the list empty on ordinary frames, as launch_redo's; a redone pixel is fp64 under every flag)
        if ((st = launch_wide(ctx, w, kCountOnDevice, kWideRedoSlots, p.redo_count, s, launches, false, nullptr))) return st;
    }
    return RPF_OK;
}

// A full-box pass under RPF_FLAG_MEMBER_TEST (route 9): route 7's structure, whatever the window's size, with
// the configured test in the count kernel and in the wide kernel's own stage 1b.  The class kernels read the listed members as
// they are.  REF_ABORT is refused, so there is no redo list; the lists of this pass are no other pass's (the membership cache of
// the size-binned route neither serves it nor survives it).
int32_t route_member_test(rpf_ctx *ctx, const PassParams &p, hipStream_t s, int *launches) {
    if (!ctx->d_member || !ctx->member_fresh || p.S > class_capacity(kNumWave - 1) || p.redo_list != nullptr)
        return fail(ctx, RPF_E_BADARG, "pass under the membership test without its configuration (setup_pass prepares it)");
    return route_wide_classes(ctx, p, ctx->d_member, s, launches);
}

// A full-box pass under RPF_FLAG_MEMBER_TEST | RPF_FLAG_MEMBER_FUSED on a compiled layout (route 10): route
// 2's structure behind the count kernel's MEMBER form, whatever box*box*S <= 65535 is and whatever option "binning" says.
// REF_ABORT is refused, so there is no redo list.
int32_t route_member_fused(rpf_ctx *ctx, const PassParams &p, bool packed, hipStream_t s, int *launches) {
    if (!ctx->d_member || !ctx->member_fresh || !p.lay.supported() || p.nmax > kMaxNbhd || p.redo_list != nullptr)
        return fail(ctx, RPF_E_BADARG, "pass under the membership test without its configuration (setup_pass prepares it)");
    return route_binned(ctx, p, packed, ctx->d_member, s, launches);
}

// A sampled pass (RPF_FLAG_SAMPLED_NBHD with draws > 0): route 7 with another count kernel.
// generic::launch_sampled_count lists, per pixel, the distinct draws of its key that pass the 3-sigma test; S + draws <= 832 puts
// every pixel into one of the eight classes, so there is no rest launch, and REF_ABORT is refused, so there is no redo launch.
// Under RPF_FLAG_SAMPLED_REST S + draws may reach RPF_SAMPLED_MAX (section 13e): the count is then the block kernel's, and the
// pixels with N > 832 -- the rest list -- go to one launch of generic::filter_pixel_kernel's LISTED instantiation, which reads their
// listed members, with nmax = S + draws (never more than the window holds) for its carve-up and its HBM slots, kPassSlots' rule,
// and the 2^-44 table.  Pool capacity and growth are route 7's (option "wide_pool"): up to pixels * draws entries.  The lists of this
// pass are no other pass's: the membership cache of the size-binned route neither serves it nor survives it (d_lists is overwritten).
int32_t route_sampled(rpf_ctx *ctx, const PassParams &p_in, hipStream_t s, int *launches) {
    int32_t st;
    ctx->last_route = kRouteSampled;
    PassParams p = p_in;
    p.redo_list = nullptr; p.redo_count = nullptr;
    if (p.row_end <= p.row_begin) return RPF_OK;
    const SampledPass sp = ctx->samp_now;
    if (sp.draws < 1 || sp.draws > sp.max_draws || !ctx->d_samp_table || ctx->samp_table_box != p.box)
        return fail(ctx, RPF_E_BADARG, "sampled pass without its configuration (setup_pass prepares it)");
    generic::SampledCountArgs a = {ctx->d_samp_table, ctx->sampling.seed, sp.pass_id, ctx->sampling.row_origin, sp.draws};
    if (p.generic & kGenericMemberTest) { // with RPF_FLAG_MEMBER_TEST the draws meet the configured test
        if (!ctx->d_member || !ctx->member_fresh) return fail(ctx, RPF_E_BADARG, "pass under the membership test without its configuration (setup_pass prepares it)");
        a.member = ctx->d_member;
    }
    uint32_t counts[kNumClasses];
    const ListedPass lp = {true, "rpf:sampled count + classify (draws, stage 1b test, listed members, lane and wave classes)",
                           "sampled count pass: the member pool overflowed at its exact size"};
    // (launch_sampled_count zeroes the cursor itself)
    const auto count = [&](const PassParams &q, const generic::MemberPool &m, hipStream_t cs) { return generic::launch_sampled_count(q, a, m, cs); };
    if ((st = count_and_deal(ctx, p, lp, count, counts, s))) return st;
    if (counts[kRestClass] != 0 && p.S + sp.draws <= class_capacity(kNumWave - 1)) return fail(ctx, RPF_E_HIP, "sampled count pass: a pixel with N > 832");
    if ((st = launch_classes(ctx, p, counts, kNumWave, false, "rpf:sampled pass, packed class", "rpf:sampled pass, wave class", s, launches))) return st;
    if (counts[kRestClass] != 0) {
        Range rg("rpf:sampled pass, listed rest kernel (N > 832)");
        PassParams q = p;
        q.nmax = (int32_t)std::min<int64_t>(p.nmax, (int64_t)p.S + sp.draws);
        q.bmax = bmax_of(q.nmax);
        q.pix_list = ctx->d_lists + (size_t)kRestClass * p.W * p.H;
        q.list_count = counts[kRestClass];
        if ((st = launch_streaming(ctx, q, q.list_count, kPassSlots, nullptr, s, launches, false, true))) return st;
    }
    return RPF_OK;
}

// A sampled pass under RPF_FLAG_SAMPLED_FUSED on a compiled layout (route 11): the size-binned route's deal
// and class loop behind generic::sampled_count_mask_kernel, which leaves N and the acceptance masks of the draws route 8 lists.  A
// sampled neighbourhood is an acceptance mask over the window with few bits set, so the compiled packed, one-wave and four-wave
// kernels rebuild route 8's member lists from the masks as they do on route 2.  No list is longer than S + draws: the kernels are
// sized from min(box*box*S, S + draws), setup_pass admits S + draws <= 3136 only, and a non-empty streaming class -- it would
// repeat a full-box stage 1b -- is an internal error.  Under RPF_FLAG_MEMBER_TEST the draws meet the configured test, as on route
// 8.  REF_ABORT is refused on a sampled pass, so there is no redo list.  The masks and lists of this pass are no other pass's
// (its draws change with the pass id): route_pass dropped the membership cache before it ran, and it sets none.
int32_t route_sampled_fused(rpf_ctx *ctx, const PassParams &p_in, bool packed, hipStream_t s, int *launches) {
    int32_t st;
    ctx->last_route = kRouteSampledFused;
    PassParams p = p_in;
    p.redo_list = nullptr; p.redo_count = nullptr;
    if (p.row_end <= p.row_begin) return RPF_OK;
    const SampledPass sp = ctx->samp_now;
    if (sp.draws < 1 || sp.draws > sp.max_draws || !ctx->d_samp_table || ctx->samp_table_box != p.box || !p.lay.supported() ||
        p.nmax > kMaxNbhd || (int64_t)p.S + sp.draws > kMaxResident)
        return fail(ctx, RPF_E_BADARG, "sampled pass without its configuration (setup_pass prepares it)");
    generic::SampledCountArgs a = {ctx->d_samp_table, ctx->sampling.seed, sp.pass_id, ctx->sampling.row_origin, sp.draws};
    if (p.generic & kGenericMemberTest) { // with RPF_FLAG_MEMBER_TEST the draws meet the configured test
        if (!ctx->d_member || !ctx->member_fresh) return fail(ctx, RPF_E_BADARG, "pass under the membership test without its configuration (setup_pass prepares it)");
        a.member = ctx->d_member;
    }
    p.nmax = (int32_t)std::min<int64_t>(p.nmax, (int64_t)p.S + sp.draws); // the longest list of the pass sizes its kernels
    p.bmax = bmax_of(p.nmax);
    PassParams pc;
    if ((st = binned_params(ctx, p, pc))) return st;
    uint32_t counts[kNumClasses];
    {
        Range rg("rpf:sampled count + classify (draws, stage 1b test, acceptance masks, size classes)");
        HIP_TRY(hipMemsetAsync(ctx->d_class_counts, 0, kNumClasses * sizeof(uint32_t), s));
        HIP_TRY(generic::launch_sampled_count_mask(pc, a, s));
        if ((st = deal_classes(ctx, pc, counts, s))) return st;
    }
    if (counts[kNumClasses - 1] != 0) return fail(ctx, RPF_E_HIP, "sampled count pass: a pixel with N > 3136");
    return filter_classes(ctx, pc, packed, nullptr, counts, s, launches);
}

// A sampled pass under RPF_FLAG_SAMPLED_LISTED on a compiled layout (route 12): route 8's count-and-deal step
// with the deal of route 2 -- the eleven classes -- and then the size-binned route's class loop on the listed builds of the compiled
// kernels (kGenericSampledListed in p.generic: launch_filter_pass and launch_filter_packed dispatch on it), which copy their member
// lists from the pool.  The count kernel: for a window of at most 65535 candidates generic::sampled_count_list_kernel, route 11's
// bitmap kernel with a listing tail; above that route 8's own launch (the enumeration sort, or the block kernel above S + draws =
// 832), whose candidate indices are 32 bits wide.  Either way the pool content is route 8's.  No list is longer than S + draws: the
// kernels are sized from min(box*box*S, S + draws) on a wide window too, setup_pass admits S + draws <= 3136 only, and a non-empty
// streaming class is an internal error.  No mask buffer; pool capacity and growth are route 7's (option "wide_pool").  REF_ABORT is
// refused on a sampled pass, so there is no redo list.  The lists of this pass are no other pass's: route_pass dropped the
// membership cache before it ran, and it sets none.
int32_t route_sampled_listed(rpf_ctx *ctx, const PassParams &p_in, bool packed, hipStream_t s, int *launches) {
    int32_t st;
    ctx->last_route = kRouteSampledListed;
    PassParams p = p_in;
    p.redo_list = nullptr; p.redo_count = nullptr;
    if (p.row_end <= p.row_begin) return RPF_OK;
    const SampledPass sp = ctx->samp_now;
    if (sp.draws < 1 || sp.draws > sp.max_draws || !ctx->d_samp_table || ctx->samp_table_box != p.box || !p.lay.supported() ||
        (int64_t)p.S + sp.draws > kMaxResident || (p.generic & (kGenericWide | kGenericSampledFused)))
        return fail(ctx, RPF_E_BADARG, "sampled pass without its configuration (setup_pass prepares it)");
    generic::SampledCountArgs a = {ctx->d_samp_table, ctx->sampling.seed, sp.pass_id, ctx->sampling.row_origin, sp.draws};
    if (p.generic & kGenericMemberTest) { // with RPF_FLAG_MEMBER_TEST the draws meet the configured test
        if (!ctx->d_member || !ctx->member_fresh) return fail(ctx, RPF_E_BADARG, "pass under the membership test without its configuration (setup_pass prepares it)");
        a.member = ctx->d_member;
    }
    const bool bitmap = p.nmax <= kMaxNbhd; // the window's candidate indices fit the bitmap kernel's 16-bit queue
    p.nmax = (int32_t)std::min<int64_t>(p.nmax, (int64_t)p.S + sp.draws); // the longest list of the pass sizes its kernels
    p.bmax = bmax_of(p.nmax);
    p.reroute_masks = nullptr;
    p.carry = nullptr;
    if (p.nmax > class_capacity(kNumClasses - 4) && ctx->tun.split_weights != 0) {
        // the 32- and 64-spp classes run as three kernels (chains; bins + MI; weights): per-pixel hand-over buffer (binned_params)
        if ((st = ctx->d_carry.ensure(ctx, (size_t)p.W * p.H * (size_t)kCarryStride * sizeof(double)))) return st;
        p.carry = ctx->d_carry;
    }
    uint32_t counts[kNumClasses];
    const ListedPass lp = {true, "rpf:sampled count + classify (draws, stage 1b test, listed members, size classes)",
                           "sampled count pass: the member pool overflowed at its exact size", kNumClasses, -1};
    // (both launches zero the cursor themselves)
    const auto count = [&](const PassParams &q, const generic::MemberPool &m, hipStream_t cs) {
        return bitmap ? generic::launch_sampled_count_list(q, a, m, cs) : generic::launch_sampled_count(q, a, m, cs);
    };
    if ((st = count_and_deal(ctx, p, lp, count, counts, s))) return st;
    if (counts[kNumClasses - 1] != 0) return fail(ctx, RPF_E_HIP, "sampled count pass: a pixel with N > 3136");
    return filter_classes(ctx, p, packed, nullptr, counts, s, launches);
}

// Routes 4 and 5, the layout-generic route with its small neighbourhoods on class kernels (RPF_FLAG_GENERIC |
// RPF_FLAG_GENERIC_PACKED on a pass with S <= 64; ... | RPF_FLAG_GENERIC_WAVE on one with S <= 832): stage 1b as its own launch
// (generic::nbhd_count_kernel: N and the acceptance masks), the pixels dealt by N into n_classes classes -- four lane classes
// N <= 8, 16, 32, 64 of generic::filter_packed_kernel and, on route 5, N <= 128, 256, 448, 832 for generic::filter_wave_kernel
// (one wave per pixel, member list from the acceptance masks, LDS sized for the class) -- and the rest into the list
// generic::filter_pixel_kernel walks (it runs its own 3-sigma test); then one launch per non-empty list.  One read-back per pass
// (the list sizes).  REF_ABORT: the class kernels put the pixels with an in-band table on the redo list, which launch_redo
// filters again.  None of the rpf_set_option names applies here.
// Route 13 (... | RPF_FLAG_GENERIC_QUAD on a pass with S <= 3136) is route 5 with up to two classes more,
// N <= 1600 and N <= 3136 on generic::filter_quad_kernel: n_classes is kNumQuad cut back to the last capacity whose carve-up the
// layout fits (generic_quad_carve), and the rest list is what lies above it.
int32_t route_generic_classes(rpf_ctx *ctx, const PassParams &p_in, int n_classes, Route route, hipStream_t s, int *launches) {
    const size_t HW = (size_t)p_in.W * p_in.H;
    const bool wave = route == kRouteGenericWave || route == kRouteGenericQuad;
    int32_t st;
    ctx->last_route = route;
    PassParams p = p_in;
    if (p.row_end <= p.row_begin) return RPF_OK;
    while (n_classes > kNumWave && generic_quad_carve(p.lay, class_capacity(n_classes - 1)).hists == 0) --n_classes; // (route 13)
    if ((st = ctx->d_lists.ensure(ctx, (size_t)kNumClasses * HW * sizeof(uint32_t)))) return st;
    p.mask_stride = mask_stride(p);
    if ((st = ctx->d_masks.ensure(ctx, HW * p.mask_stride * sizeof(uint64_t)))) return st;
    p.masks = ctx->d_masks;
    uint32_t counts[kNumClasses];
    {
        Range rg(wave ? "rpf:generic count + classify (stage 1b test, lane and wave classes)"
                      : "rpf:generic count + classify (stage 1b test, lane classes)");
        HIP_TRY(hipMemsetAsync(ctx->d_class_counts, 0, kNumClasses * sizeof(uint32_t), s));
        HIP_TRY(generic::launch_nbhd_count(p, s));
        HIP_TRY(launch_classify(p, ctx->d_lists, ctx->d_class_counts, n_classes, kRestClass, s));
        HIP_TRY(hipMemcpyAsync(counts, ctx->d_class_counts, sizeof(counts), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if ((st = launch_classes(ctx, p, counts, n_classes, class_fast(p), "rpf:generic packed class", "rpf:generic wave class", s, launches))) return st;
    if (counts[kRestClass] != 0) {
        Range rg(n_classes > kNumWave ? "rpf:generic filter kernel (N above the four-wave classes)"
                                      : (wave ? "rpf:generic filter kernel (N > 832)" : "rpf:generic filter kernel (N > 64)"));
        PassParams q = p;
        q.pix_list = ctx->d_lists + (size_t)kRestClass * HW;
        q.list_count = counts[kRestClass];
        if ((st = launch_streaming(ctx, q, q.list_count, kPassSlots, nullptr, s, launches, stream_fast(p)))) return st;
    }
    return launch_redo(ctx, p, s, launches);
}

// Which layout-generic route a pass takes (kRouteNone: none, a pass on the compiled kernels).  Above 64 spp N >= S fits no
// packed class, above 832 spp no one-wave class, above 3136 spp no four-wave class: such a pass runs as route 3 does.
Route generic_route(const PassParams &p) {
    if (p.generic & kGenericSampledListed) return kRouteSampledListed; // (... a sampled pass the listed builds take under RPF_FLAG_SAMPLED_LISTED)
    if (p.generic & kGenericSampledFused) return kRouteSampledFused; // (... a sampled pass the compiled kernels take under RPF_FLAG_SAMPLED_FUSED)
    if (p.generic & kGenericSampled) return kRouteSampled; // (setup_pass marked it: draws > 0)
    if (p.generic & kGenericMemberFused) return kRouteMemberFused; // (... a full-box pass the compiled kernels take under RPF_FLAG_MEMBER_FUSED)
    if (p.generic & kGenericMemberTest) return kRouteMemberTest; // (... a full-box pass of a call under RPF_FLAG_MEMBER_TEST)
    if (p.generic & kGenericWide) return (p.generic & kGenericWideClasses) ? kRouteWideClasses : kRouteWide; // (setup_pass marked it)
    if (!route_bits(p.generic)) return kRouteNone; // (kGenericScheduleFused picks the build of the compiled kernels, not a route)
    if ((p.generic & kGenericQuad) && p.S <= class_capacity(kNumQuad - 1)) return kRouteGenericQuad; // (validate: the three bits below are set)
    if ((p.generic & kGenericWave) && p.S <= class_capacity(kNumWave - 1)) return kRouteGenericWave;
    if ((p.generic & kGenericPacked) && p.S <= class_capacity(kNumPacked - 1)) return kRouteGenericPacked;
    return kRouteGeneric;
}

} // namespace

// One filter pass over rows [p.row_begin, p.row_end), on the route its flags, its sizes and the options pick.  A layout-generic
// or wide pass: generic_route.  A pass on the compiled kernels: when box*box*S is above what the one-wave kernels hold (512
// samples), the neighbourhood sizes are counted first and every kernel family filters its own pixel list with LDS sized for its
// capacity (rpf_kernels.hip, "neighbourhood-size binning"); option "binning" = 0/1 overrides.
// Needs stage 1a's planes (pmean / pstd) for those rows.  Synchronises the stream when it bins (list sizes).
int32_t route_pass(rpf_ctx *ctx, const PassParams &p_in, hipStream_t s, int *launches) {
    const Route route = generic_route(p_in);
    PassParams p = p_in;
    int32_t st;
    // Who keeps a redo list: routes 4, 5, 7 and 13; routes 3 and 6 never (their kernels evaluate the reference's expression in
    // place); a fused pass unless stages are skipped.  RPF_FLAG_FAST_WEIGHTS keeps the list too: MI, alpha, beta and W_r_c are the
    // reference's under the flag as well, and a redone pixel is filtered whole, in fp64, by the reference-expression kernel (the
    // FAST instantiations test p.redo_list at run time like the others, stage 3b)
    const bool keeps_list = route == kRouteNone ? ctx->tun.stage_mask == -1 : route != kRouteGeneric && route != kRouteWide;
    if ((st = begin_redo(ctx, p, keeps_list, s))) return st;
    // a pass on the compiled kernels: size-binned or not
    bool bin = route == kRouteNone && p.nmax > 512;
    if (route == kRouteNone && ctx->tun.binning >= 0) bin = ctx->tun.binning != 0;
    if (route == kRouteNone && p.nmax > kMaxResident) bin = true; // the streaming kernel takes the pixels no resident kernel can hold
    // The membership cache of the size-binned route (bin_valid: the class counts on the host, d_lists and d_masks on the device)
    // outlives a pass only from one size-binned pass to the next: route_binned alone sets it, and every other route drops it
    // here, before it runs -- the unbinned route with its packed lists, routes 4 and 5, the listed-member routes 7, 8 and 9 and
    // routes 11 and 12 write their own lists, masks and class counts into the same buffers.  Route 10 is route_binned under another test: it keeps
    // the cache, keyed by bin_member, so that neither of routes 2 and 10 is served the other's masks
    if (!bin && route != kRouteMemberFused) ctx->bin_valid = false;
    // small neighbourhoods (N <= 64) run on the packed kernels, several pixels per wave (rpf_packed_impl.inc); option "packed"
    const bool packed = ctx->tun.packed != 0 && !p.fast_weights && ctx->tun.stage_mask == -1 && ctx->tun.lds_pad == 0;
    switch (route) {
    case kRouteMemberFused: return route_member_fused(ctx, p, packed, s, launches);
    case kRouteSampledFused: return route_sampled_fused(ctx, p, packed, s, launches);
    case kRouteSampledListed: return route_sampled_listed(ctx, p, packed, s, launches);
    case kRouteSampled: return route_sampled(ctx, p, s, launches);
    case kRouteMemberTest: return route_member_test(ctx, p, s, launches);
    case kRouteWideClasses: return route_wide_classes(ctx, p, nullptr, s, launches);
    case kRouteWide: return route_wide(ctx, p, s, launches);
    case kRouteGenericQuad: return route_generic_classes(ctx, p, kNumQuad, route, s, launches);
    case kRouteGenericWave: return route_generic_classes(ctx, p, kNumWave, route, s, launches);
    case kRouteGenericPacked: return route_generic_classes(ctx, p, kNumPacked, route, s, launches);
    case kRouteGeneric: return route_generic(ctx, p, s, launches);
    default: break;
    }
    return bin ? route_binned(ctx, p, packed, nullptr, s, launches) : route_unbinned(ctx, p, packed, s, launches);
}

} // namespace rpf
