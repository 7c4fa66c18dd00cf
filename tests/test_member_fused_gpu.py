"""GPU tests of RPF_FLAG_MEMBER_FUSED (rpf_query_route 10): a full-box pass under the membership test on the
compiled kernels, behind the count kernel's MEMBER form.  Held to the numpy restatement tests/member_test_ref.py on every pixel, to
the unflagged size-binned route 2 under the reference's multiples and floors (the anchor), to route 9 for the bin ids, and to the
chain of one-pass calls for pass sequences.  EPS policy throughout (REF_ABORT is refused), sigma_seed 0.5 (the filter is active).

Before the feature the bit is not refused without RPF_FLAG_MEMBER_TEST and changes nothing with it: the cases of groups 1 to 5 and
7 to 12 fail on `route == 10` or on the refusal.  Group 6 (the fallbacks: same bits and counters as without the bit) and the
assertions on the restatement alone (the class census of a frame) pass before and after, and are no evidence for the feature."""
import functools

import numpy as np
import pytest

import member_test_ref as MR
import sampled_ref as SR
import spike_ref
import stage4_bars as B
from raytracer_rpf_amd import feature_buffer as fb

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
SIGMA = 0.5
SEED = 0x5EED5EED
BITS = ("nbhd_size", "member_hash", "mean", "stddev", "bin_hash")
STAGES = BITS + ("mi", "alpha", "beta", "wrc")
CAPS = (8, 16, 32, 64, 128, 256, 448, 832, 1600, 3136)   # the resident classes of route 2 / route 10
STREAM = 65535                                           # the name of the streaming class

# name: W, H, S, box, generator arguments, floors as a multiple of preset 1's, the classes the frame is here for
CASES = {
    "k7": (12, 10, 8, 7, dict(flat_frac=0.94), 1.0, (128, 256, 448)),
    "b11": (16, 13, 8, 11, dict(flat_frac=0.94), 1.0, (448, 832, 1600)),          # nmax 968: the split-weights classes
    "b13": (14, 13, 8, 13, dict(flat_frac=0.94), 1.0, (448, 832, 1600)),          # 1344 candidates: two chunks of the count kernel
    "b15s16": (16, 15, 16, 15, dict(flat_frac=0.94), 1.0, (1600, 3136, STREAM)),  # four-wave kernels with masks
    "b17s16": (18, 17, 16, 17, dict(flat_frac=0.94), 1.0, (1600, 3136, STREAM)),  # > 4096 candidates: one-wave resident instantiations
    "packed": (6, 5, 2, 5, dict(), 0.1, (8, 16, 32)),
}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def class_of(n):
    return next((c for c in CAPS if n <= c), STREAM)


def classes_of(nbhd):
    return {class_of(int(n)) for n in np.asarray(nbhd).ravel()}


@functools.lru_cache(maxsize=None)
def frame(W, H, S, seed=11, **kw):
    p = fb.synth_planes(W, H, S, seed=seed, **kw)
    p.setflags(write=False)
    return p


def planes_of(name):
    W, H, S, _, kw, _, _ = CASES[name]
    return frame(W, H, S, **kw)


def member_cfg(hipmod, mt):
    return hipmod.make_membership(mt[0].tolist(), mt[1].tolist())


_refs = {}


def ref_of(oracle, name):
    """the restatement of the case's pass: computed once, shared, never modified"""
    if name not in _refs:
        _, _, _, box, _, scale, _ = CASES[name]
        _refs[name] = MR.member_pass(oracle, planes_of(name), MR.published19(scale), box, SIGMA, EPS)
    return _refs[name]


def flags_of(hipmod, fused=True, member=True):
    return (hipmod.MEMBER_TEST_FLAG if member else 0) | (hipmod.MEMBER_FUSED_FLAG if fused and member else 0)


def desc_of(hipmod, planes, extra=0, fused=True, member=True, **kw):
    _, H, W, S = planes.shape
    kw.setdefault("sigma_seed", SIGMA)
    return hipmod.make_desc(W, H, S, policy=EPS, flags=flags_of(hipmod, fused, member) | extra, **kw)


def run(c, hipmod, planes, mt, box, extra=0, fused=True, member=True, allow_nonfinite=False, colour_in=None, **kw):
    if mt is not None:
        c.set_membership(member_cfg(hipmod, mt))
    got = c.filter_pass_debug(planes, desc_of(hipmod, planes, extra, fused, member, **kw), box=box, allow_nonfinite=allow_nonfinite,
                              colour_in=colour_in)
    cn = c.counters()
    got.update(route=c.route(), launches=cn.filter_kernel_launches, redo_pixels=cn.redo_pixels)
    return got


def assert_same_pass(a, b, keys=STAGES + ("colour",)):
    for k in keys:
        assert same_bits(a[k], b[k]), k
    assert (a["sum_nbhd"], a["max_nbhd"], a["launches"], a["redo_pixels"]) == (b["sum_nbhd"], b["max_nbhd"], b["launches"], b["redo_pixels"])


class options:
    """options set on a shared context, put back on exit"""
    DEFAULTS = dict(binning=-1, split_weights=-1, waves_per_pixel=0, packed=-1, wide=-1)

    def __init__(self, c, **kw):
        self.c, self.kw = c, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.c.set_option(k, v)

    def __exit__(self, *a):
        for k in self.kw:
            self.c.set_option(k, self.DEFAULTS[k])


def full_window(W, H, S, box):
    b = (box - 1) // 2
    nx = np.minimum(np.arange(W) + b, W - 1) - np.maximum(np.arange(W) - b, 0) + 1
    ny = np.minimum(np.arange(H) + b, H - 1) - np.maximum(np.arange(H) - b, 0) + 1
    return (ny[:, None] * nx[None, :] * S).astype(np.int32)


# ---- 1. the anchor: multiples 3 and floors -1 on route 10 are the unflagged size-binned route 2 ----------------------------------
@pytest.mark.parametrize("W,H,S,box,flat", [(12, 10, 8, 7, False), (12, 10, 8, 7, True), (16, 13, 8, 11, True)],
                         ids=["box7-smooth", "box7-flat94", "box11-flat94"])
def test_anchor_route_10_against_route_2(ctx, hipmod, W, H, S, box, flat):
    planes = frame(W, H, S, **(dict(flat_frac=0.94) if flat else {}))
    with options(ctx, binning=1):
        want = run(ctx, hipmod, planes, None, box, member=False)
    assert want["route"] == 2
    got = run(ctx, hipmod, planes, MR.reference(), box)
    assert got["route"] == 10 and got["status"] == hipmod.OK and got["redo_pixels"] == 0
    assert_same_pass(got, want)                                   # the same kernels on the same lists: every plane, colours included
    assert got["launches"] == len(classes_of(got["nbhd_size"]))
    if flat:  # the flat proof under a negative floor: the flat pixels keep N = S, as without the flags
        assert (got["nbhd_size"] == S).mean() >= 0.90
    else:
        assert got["nbhd_size"].min() > S


# ---- 2. stage parity on every pixel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_stage_parity_on_every_pixel(ctx, hipmod, oracle, name):
    W, H, S, box, _, scale, reach = CASES[name]
    planes, mt = planes_of(name), MR.published19(scale)
    want = ref_of(oracle, name)
    classes = classes_of(want["nbhd_size"])
    print("FUSED %s: N %d .. %d, classes %s" % (name, want["nbhd_size"].min(), want["nbhd_size"].max(), sorted(classes)))
    assert set(reach) <= classes, (reach, sorted(classes))              # the frame reaches the kernels it is here for
    got = run(ctx, hipmod, planes, mt, box)
    assert got["status"] == hipmod.OK and got["route"] == 10 and got["redo_pixels"] == 0
    assert got["launches"] == len(classes)                              # one launch per non-empty class of the eleven
    assert np.array_equal(got["nbhd_size"], want["nbhd_size"])
    assert np.array_equal(got["member_hash"], want["member_hash"])
    assert np.array_equal(got["mean"], want["mean"]) and np.array_equal(got["stddev"], want["stddev"])
    np.testing.assert_allclose(got["mi"], want["mi"], rtol=0, atol=1e-11)
    for k in ("alpha", "beta", "wrc"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12)
    assert got["max_nbhd"] == want["nbhd_size"].max() and got["sum_nbhd"] == int(want["nbhd_size"].sum())
    assert np.array_equal(ctx.nbhd(W, H), want["nbhd_size"])
    if name == "packed":   # the smaller floors reject some candidates, only packed classes are reached, some pixels keep N = S
        assert (want["nbhd_size"] < full_window(W, H, S, box)).any() and classes <= {8, 16, 32, 64}
        assert (want["nbhd_size"] == S).sum() >= 1
    # the bin ids: route 9's, on the same context, without the new bit
    r9 = run(ctx, hipmod, planes, None, box, fused=False)
    assert r9["route"] == 9 and same_bits(got["bin_hash"], r9["bin_hash"])
    # stage 4: the restatement on the device's own stage outputs, every sample, the bar of the form the pixel's kernel uses
    ref = MR.stage4_on(oracle, planes, got, mt, box, SIGMA, EPS)
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(ref))
    cmax = B.cmax_of(planes[2:5])
    n = want["nbhd_size"]
    both = np.isfinite(got["colour"]) & np.isfinite(ref)
    dist = np.where(both, np.abs(got["colour"] - ref), 0.0).max(axis=(0, 3)) / cmax      # per pixel
    bars = np.empty((H, W))
    for form, sel in (("expanded", n <= B.RESIDENT), ("direct", n > B.RESIDENT)):
        if sel.any():
            bars[sel] = B.sample_bar(form, 12, int(n[sel].max()), SIGMA, box)
    worst = np.unravel_index(np.argmax(dist / bars), dist.shape)
    print("FUSED %s stage 4: worst %.3e (bar %.3e) at pixel %s N %d" % (name, dist[worst], bars[worst], worst, n[worst]))
    assert both.any() and (dist <= bars).all(), (float(dist[worst]), float(bars[worst]))
    assert np.abs(got["colour"] - want["colour"]).max() <= 1e-4 * cmax                   # and the whole restatement, loosely


# ---- 3. the flat proof ---------------------------------------------------------------------------------------------------------
def test_flat_proof_fires_only_under_a_negative_floor(ctx, hipmod, oracle):
    """tests/test_member_test_gpu.py's three frames on route 10"""
    W, H, S, box = 12, 10, 8, 7
    planes = np.array(frame(W, H, S))
    for k in range(12):
        planes[7 + k] = np.float32(0.125 * (k + 1))
    pub = run(ctx, hipmod, planes, MR.published19(), box, allow_nonfinite=True)
    assert pub["route"] == 10 and np.array_equal(pub["nbhd_size"], full_window(W, H, S, box))
    ref = run(ctx, hipmod, planes, MR.reference(), box, allow_nonfinite=True)
    assert ref["route"] == 10 and (ref["nbhd_size"] == S).all()
    # one zero-variance feature among live ones, its floor alone non-negative: the restatement's lists
    planes = np.array(frame(W, H, S))
    planes[7] = np.float32(0.25)
    mult, floor = MR.published19()
    floor[1:] = -1.0
    want_n, want_codes = MR.counts(oracle, planes, (mult, floor), box)
    got = run(ctx, hipmod, planes, (mult, floor), box, allow_nonfinite=True)
    assert got["route"] == 10 and want_n.min() > S and np.array_equal(got["nbhd_size"], want_n)
    assert all(SR.fnv1a_u32(want_codes[(y, x)]) == got["member_hash"][y, x] for y in range(H) for x in range(W))
    floor[0] = -1.0
    got = run(ctx, hipmod, planes, (mult, floor), box, allow_nonfinite=True)
    assert got["route"] == 10 and (got["nbhd_size"] == S).all()


# ---- 4. NaN and +inf ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_special_values(ctx, hipmod, oracle, value):
    W, H, S, box = 12, 10, 8, 7
    planes = np.array(planes_of("k7"))
    planes[7 + 4, 5, 6, 3] = value                                                   # one sample of feature 4 (a world position)
    for mt in (MR.published19(), MR.reference()):
        want_n, want_codes = MR.counts(oracle, planes, mt, box)
        got = run(ctx, hipmod, planes, mt, box, allow_nonfinite=True)
        assert got["route"] == 10
        assert np.array_equal(got["nbhd_size"], want_n)
        assert all(SR.fnv1a_u32(want_codes[(y, x)]) == got["member_hash"][y, x] for y in range(H) for x in range(W))


# ---- 5. layouts ------------------------------------------------------------------------------------------------------------------
def test_compiled_27_dim_layout_takes_route_10(ctx, hipmod, oracle):
    W, H, S, box, nr, nf = 12, 10, 8, 7, 4, 18
    stored = fb.synth_planes(W, H, S, seed=5, n_random=nr, n_feat=nf, dtype="f16", flat_frac=0.5)
    mt = (np.where(np.arange(nf) % 6 >= 3, 30.0, 3.0), np.full(nf, 0.05))
    want = MR.member_pass(oracle, stored.astype(np.float32), mt, box, SIGMA, EPS, n_random=nr, n_feat=nf, weights=False)
    desc = hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=SIGMA, flags=flags_of(hipmod), n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16)
    assert hipmod.layout_kernels(desc) == (hipmod.OK, 0)
    ctx.set_membership(member_cfg(hipmod, mt))
    got = ctx.filter_pass_debug(stored, desc, box=box)
    assert ctx.route() == 10 and got["status"] == hipmod.OK
    assert want["nbhd_size"].max() > 64
    assert np.array_equal(got["nbhd_size"], want["nbhd_size"]) and np.array_equal(got["member_hash"], want["member_hash"])
    assert np.array_equal(got["mean"], want["mean"]) and np.array_equal(got["stddev"], want["stddev"])


def test_generic_layout_stays_on_route_9(ctx, hipmod):
    W, H, S, box, nr, nf = 12, 10, 8, 7, 3, 7
    stored = fb.synth_planes(W, H, S, seed=5, n_random=nr, n_feat=nf, dtype="f16", flat_frac=0.5)
    mt = (np.where(np.arange(nf) % 6 >= 3, 30.0, 3.0), np.full(nf, 0.05))
    ctx.set_membership(member_cfg(hipmod, mt))
    out = []
    for fused in (False, True):
        desc = hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=SIGMA, flags=flags_of(hipmod, fused) | hipmod.FLAG_GENERIC, n_random=nr,
                                n_feat=nf, plane_dtype=hipmod.PLANES_F16)
        assert hipmod.layout_kernels(desc) == (hipmod.OK, 1)
        got = ctx.filter_pass_debug(stored, desc, box=box)
        cn = ctx.counters()
        got.update(route=ctx.route(), launches=cn.filter_kernel_launches, redo_pixels=cn.redo_pixels)
        out.append(got)
    assert out[0]["route"] == out[1]["route"] == 9
    assert_same_pass(out[1], out[0])


# ---- 6. fallbacks: the same bits and counters as the same call without the new bit ------------------------------------------------
def test_fallback_sampled_pass(ctx, hipmod):
    planes, mt = planes_of("k7"), MR.published19()
    ctx.set_sampling(hipmod.make_sampling(SEED, [40]))
    a = run(ctx, hipmod, planes, mt, 7, extra=hipmod.SAMPLED_NBHD_FLAG, fused=False)
    b = run(ctx, hipmod, planes, None, 7, extra=hipmod.SAMPLED_NBHD_FLAG)
    assert a["route"] == b["route"] == 8
    assert_same_pass(b, a)


def test_fallback_scheduled_gains(ctx, hipmod):
    planes, mt = planes_of("k7"), MR.published19()
    ctx.set_schedule(hipmod.make_schedule(SIGMA, 2.0, 1.1))
    a = run(ctx, hipmod, planes, mt, 7, extra=hipmod.SCHEDULE_FLAG, fused=False)
    b = run(ctx, hipmod, planes, None, 7, extra=hipmod.SCHEDULE_FLAG)
    assert a["route"] == b["route"] == 9
    assert_same_pass(b, a)


def test_fallback_wide_pass(ctx, hipmod):
    W, H, S, box = 2, 2, 810, 9
    assert box * box * S > 65535
    planes, mt = frame(W, H, S), MR.published19()
    a = run(ctx, hipmod, planes, mt, box, extra=hipmod.FLAG_WIDE_NBHD, fused=False)
    b = run(ctx, hipmod, planes, None, box, extra=hipmod.FLAG_WIDE_NBHD)
    assert a["route"] == b["route"] == 9
    assert_same_pass(b, a)
    with options(ctx, wide=1):           # option "wide" forcing a pass that route 10 could take
        c = run(ctx, hipmod, planes_of("k7"), None, 7, extra=hipmod.FLAG_WIDE_NBHD)
    assert c["route"] == 9


def test_gain_1_schedule_entry_runs_route_10_with_its_seed(ctx, hipmod):
    planes, mt = planes_of("k7"), MR.published19()
    want = run(ctx, hipmod, planes, mt, 7)
    ctx.set_schedule(hipmod.make_schedule(SIGMA, 1.0, 1.0))
    got = run(ctx, hipmod, planes, None, 7, extra=hipmod.SCHEDULE_FLAG, sigma_seed=0.002)
    assert want["route"] == got["route"] == 10
    assert_same_pass(got, want)
    cold = run(ctx, hipmod, planes, None, 7, sigma_seed=0.002)       # the descriptor's own seed is another filter
    assert not same_bits(cold["colour"], want["colour"])


# ---- 7. pass sequences -----------------------------------------------------------------------------------------------------------
def call(c, hipmod, planes, boxes, flags, colour64_in=None):
    _, H, W, S = planes.shape
    desc = hipmod.make_desc(W, H, S, boxes=boxes, policy=EPS, sigma_seed=SIGMA, flags=flags)
    out = c.filter(planes, desc, colour64_in=colour64_in, want_colour64=True)
    assert out[2] == hipmod.OK
    return out[3], c.route(), c.counters()


@pytest.mark.parametrize("boxes", [(7, 7), (7, 11, 7)], ids=["7-7", "7-11-7"])
def test_pass_sequence_equals_its_chain(ctx, hipmod, boxes):
    planes, F = planes_of("b11"), flags_of(hipmod)
    ctx.set_membership(member_cfg(hipmod, MR.published19()))
    whole, route, cn = call(ctx, hipmod, planes, boxes, F)
    assert route == 10
    colour = None
    for box in boxes:
        colour, r, cn1 = call(ctx, hipmod, planes, (box,), F, colour64_in=colour)
        assert r == 10
    assert same_bits(whole, colour)
    assert (cn.sum_nbhd, cn.max_nbhd, cn.redo_pixels) == (cn1.sum_nbhd, cn1.max_nbhd, 0)          # of the last pass


def test_sampled_pass_between_two_full_box_passes(ctx, hipmod):
    """routes 10, 8, 10 at one box: the sampled pass overwrites the class lists, so the third pass must count again"""
    planes, boxes, draws = planes_of("b11"), (7, 7, 7), (0, 40, 0)
    F = flags_of(hipmod) | hipmod.SAMPLED_NBHD_FLAG
    ctx.set_membership(member_cfg(hipmod, MR.published19()))
    ctx.set_sampling(hipmod.make_sampling(SEED, draws))
    whole, route, _ = call(ctx, hipmod, planes, boxes, F)
    assert route == 10
    reported, _, _ = call(ctx, hipmod, planes, boxes, F | hipmod.PASS_REPORT_FLAG)
    assert [ctx.pass_report(p).route for p in range(3)] == [10, 8, 10] and same_bits(reported, whole)
    colour = None
    for p, box in enumerate(boxes):
        ctx.set_sampling(hipmod.make_sampling(SEED, [draws[p]], pass_id0=p))
        colour, r, _ = call(ctx, hipmod, planes, (box,), F, colour64_in=colour)
        assert r == (8 if draws[p] else 10)
    assert same_bits(whole, colour)


# ---- 8. table changes ------------------------------------------------------------------------------------------------------------
def test_set_membership_between_calls_and_an_unflagged_call_after(ctx, hipmod, oracle):
    planes, box = planes_of("k7"), 7
    with hipmod.Context(0) as fresh:
        plain = run(fresh, hipmod, planes, None, box, member=False)
    pub = run(ctx, hipmod, planes, MR.published19(), box)
    assert pub["route"] == 10 and np.array_equal(pub["nbhd_size"], ref_of(oracle, "k7")["nbhd_size"])
    ref = run(ctx, hipmod, planes, MR.reference(), box)
    want_n, _ = MR.counts(oracle, planes, MR.reference(), box)
    assert ref["route"] == 10 and np.array_equal(ref["nbhd_size"], want_n) and (pub["nbhd_size"] > ref["nbhd_size"]).any()
    got = run(ctx, hipmod, planes, None, box, member=False)
    assert got["route"] == plain["route"] and got["route"] not in (9, 10)
    assert_same_pass(got, plain)
    # the same inside one context with the size-binned route on both sides: neither is served the other's masks
    with options(ctx, binning=1):
        two = run(ctx, hipmod, planes, None, box, member=False)
        pub2 = run(ctx, hipmod, planes, MR.published19(), box)
        two2 = run(ctx, hipmod, planes, None, box, member=False)
    assert two["route"] == two2["route"] == 2 and pub2["route"] == 10
    assert_same_pass(pub2, pub)
    assert_same_pass(two2, two)


# ---- 9. entry points ---------------------------------------------------------------------------------------------------------------
def test_entry_points_agree_with_the_debug_pass(ctx, hipmod):
    import torch
    planes, F = planes_of("k7"), flags_of(hipmod)
    _, H, W, S = planes.shape
    dbg = run(ctx, hipmod, planes, MR.published19(), 7)
    assert dbg["route"] == 10
    desc = hipmod.make_desc(W, H, S, boxes=(7,), policy=EPS, sigma_seed=SIGMA, flags=F)
    want32 = dbg["colour"].astype(np.float32)
    # rpf_filter from page-locked buffers: the row-band pipeline's path
    pin = ctx.host_empty(planes.shape, planes.dtype)
    pin[...] = planes
    out_s, out_p = ctx.host_empty(want32.shape), ctx.host_empty((H, W, 3))
    ctx.filter(pin, desc, out_samples=out_s, out_pixels=out_p)
    assert ctx.route() == 10 and np.array_equal(out_s, want32)
    # rpf_filter_ex
    srgb, _, st, c64 = ctx.filter(planes, desc, want_colour64=True)
    assert st == hipmod.OK and ctx.route() == 10 and same_bits(c64, dbg["colour"]) and np.array_equal(srgb, want32)
    # rpf_filter_device
    dev = torch.device("cuda", 0)
    dp = torch.from_numpy(np.array(planes)).to(dev)
    col = dp[2:5].to(torch.float64).contiguous()
    ctx.filter_device(desc, dp.data_ptr(), col.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ctx.route() == 10 and same_bits(col.cpu().numpy(), dbg["colour"])
    # rpf_filter_film
    film = hipmod.make_film(((0, 0), (W, H)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX), sample_origin=(0, 0))
    fp = np.array(planes)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fp[0] = (xx[..., None] + (np.arange(S) + 0.5) / S).astype(np.float32)            # pFilm inside its pixel (no feature: the pass is the same)
    fp[1] = (yy[..., None] + 0.5).astype(np.float32)
    dbg_f = run(ctx, hipmod, fp, None, 7)
    s_film = ctx.filter_film(fp, desc, film)[0]
    assert ctx.route() == 10 and np.array_equal(s_film, dbg_f["colour"].astype(np.float32))


def test_banded_call_gives_the_serial_call_s_bits(ctx, hipmod):
    """48 rows are three bands of rpf_filter's row-band pipeline: first and last pass band by band, each band its own count pass"""
    W, H, S = 6, 48, 8
    planes, F = frame(W, H, S, flat_frac=0.5), flags_of(hipmod)
    ctx.set_membership(member_cfg(hipmod, MR.published19()))
    for boxes in ((7,), (7, 5, 7)):
        desc = hipmod.make_desc(W, H, S, boxes=boxes, policy=EPS, sigma_seed=SIGMA, flags=F)
        s_serial, p_serial, st = ctx.filter(planes, desc)
        assert st == hipmod.OK and ctx.route() == 10
        pin = ctx.host_empty(planes.shape, planes.dtype)
        pin[...] = planes
        out_s, out_p = ctx.host_empty(s_serial.shape), ctx.host_empty(p_serial.shape)
        ctx.filter(pin, desc, out_samples=out_s, out_pixels=out_p)
        assert ctx.route() == 10
        assert np.array_equal(out_s, s_serial) and np.array_equal(out_p, p_serial)


def need_devices(devices):
    import torch
    if max(devices) >= torch.cuda.device_count():
        pytest.skip("needs %d visible GPUs" % (max(devices) + 1))


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0), (0, 1)])
def test_multi_filter_equals_one_context(ctx, hipmod, devices):
    need_devices(devices)
    planes, cfg = frame(12, 12, 8, seed=3, flat_frac=0.94), member_cfg(hipmod, MR.published19())
    desc = hipmod.make_desc(12, 12, 8, boxes=(7, 7), policy=EPS, sigma_seed=SIGMA, flags=flags_of(hipmod))
    ctx.set_membership(cfg)
    s1, p1, st1 = ctx.filter(planes, desc)
    c1 = ctx.counters()
    assert ctx.route() == 10 and c1.max_nbhd > 64
    with hipmod.MultiContext(list(devices)) as mc:
        mc.set_membership(cfg)
        s2, p2, st2 = mc.filter(planes, desc)
        c2 = mc.counters()
    assert st1 == st2 == hipmod.OK
    assert np.array_equal(s1.view(np.uint32), s2.view(np.uint32)) and np.array_equal(p1.view(np.uint32), p2.view(np.uint32))
    assert (c2.samples_filtered, c2.sum_nbhd, c2.max_nbhd, c2.redo_pixels) == (c1.samples_filtered, c1.sum_nbhd, c1.max_nbhd, 0)


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0), (0, 1)])
def test_multi_filter_film_equals_one_context(ctx, hipmod, devices):
    need_devices(devices)
    planes, cfg = np.array(frame(12, 12, 8, seed=3, flat_frac=0.94)), member_cfg(hipmod, MR.published19())
    _, H, W, S = planes.shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    planes[0] = (xx[..., None] + (np.arange(S) + 0.5) / S).astype(np.float32)        # pFilm inside its pixel
    planes[1] = (yy[..., None] + 0.5).astype(np.float32)
    film = hipmod.make_film(((0, 0), (W, H)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX), sample_origin=(0, 0))
    desc = hipmod.make_desc(W, H, S, boxes=(7,), policy=EPS, sigma_seed=SIGMA, flags=flags_of(hipmod))
    ctx.set_membership(cfg)
    one = ctx.filter_film(planes, desc, film)
    assert ctx.route() == 10
    with hipmod.MultiContext(list(devices)) as mc:
        mc.set_membership(cfg)
        two = mc.filter_film(planes, desc, film)
    for a, b in zip(one, two):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 10. options -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,option,value", [("b11", "split_weights", 0), ("b11", "split_weights", 1), ("b11", "waves_per_pixel", 1),
                                               ("b11", "waves_per_pixel", 4), ("b11", "packed", 0), ("b11", "packed", 1),
                                               ("packed", "packed", 0), ("packed", "packed", 1), ("b11", "binning", 0)])
def test_options_act_as_on_route_2(ctx, hipmod, name, option, value):
    _, _, _, box, _, scale, _ = CASES[name]
    planes, mt = planes_of(name), MR.published19(scale)
    base = run(ctx, hipmod, planes, mt, box)
    with options(ctx, **{option: value}):
        got = run(ctx, hipmod, planes, None, box)
    assert base["route"] == got["route"] == 10
    for k in STAGES:
        assert same_bits(got[k], base[k]), k
    if option == "packed":      # colours agree to rounding (include/rpf_hip.h, option "packed"; the bar of tests/test_gpu_parity.py)
        np.testing.assert_allclose(got["colour"], base["colour"], rtol=1e-12, atol=1e-300)
    else:
        assert same_bits(got["colour"], base["colour"])
    if option == "binning":
        assert got["launches"] == base["launches"]


# ---- 11. on top --------------------------------------------------------------------------------------------------------------------
def test_spike_pass_on_top(ctx, hipmod):
    planes = np.array(planes_of("k7"))
    hit = np.random.default_rng(7).random(planes.shape[1:]) < 0.04
    planes[2:5, hit] *= np.float32(1e3)                                              # fireflies
    F = flags_of(hipmod)
    ctx.set_membership(member_cfg(hipmod, MR.published19()))
    plain, route, _ = call(ctx, hipmod, planes, (7,), F)
    ctx.set_spike(1.0, True)
    spiked, route2, _ = call(ctx, hipmod, planes, (7,), F | hipmod.FLAG_SPIKE_CLAMP)
    st = ctx.spike_stats()
    want = spike_ref.apply(plain, 1.0, True)
    assert route == route2 == 10 and st.applied == 1 and st.spike_samples == want["spike_samples"] > 0
    assert same_bits(spiked, want["colour"])


def test_pass_report_n_fields_equal_route_9(ctx, hipmod):
    planes = planes_of("b11")
    ctx.set_membership(member_cfg(hipmod, MR.published19()))
    reps = {}
    for fused in (False, True):
        call(ctx, hipmod, planes, (11,), flags_of(hipmod, fused) | hipmod.PASS_REPORT_FLAG)
        reps[fused] = ctx.pass_report(0)
    a, b = reps[False], reps[True]
    assert (a.applied, b.applied, a.route, b.route) == (1, 1, 9, 10)
    assert (b.box, b.rows, b.pixels, b.samples) == (a.box, a.rows, a.pixels, a.samples)
    for k in ("sum_nbhd", "min_nbhd", "max_nbhd", "own_only_pixels"):
        assert getattr(b.total, k) == getattr(a.total, k), k
    assert list(b.total.class_pixels) == list(a.total.class_pixels) and sum(b.total.class_pixels) == b.pixels


# ---- 12. refusals, from every device entry point, before any device work ----------------------------------------------------------
def entry_points(c, mc, hipmod, planes, boxes):
    _, H, W, S = planes.shape
    film = hipmod.make_film(((0, 0), (W, H)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX), sample_origin=(0, 0))
    return {
        "rpf_filter": lambda d: c.filter(planes, d),
        "rpf_filter_ex": lambda d: c.filter(planes, d, want_colour64=True),
        "rpf_filter_device": lambda d: c.filter_device(d, None, None),
        "rpf_filter_pass_debug": lambda d: c.filter_pass_debug(planes, d, box=boxes[0]),
        "rpf_filter_film": lambda d: c.filter_film(planes, d, film),
        "rpf_multi_filter": lambda d: mc.filter(planes, d),
        "rpf_multi_filter_film": lambda d: mc.filter_film(planes, d, film),
    }


def test_refusals_on_the_device_entry_points(hipmod):
    planes = frame(12, 10, 8)
    _, H, W, S = planes.shape
    M, X = hipmod.MEMBER_TEST_FLAG, hipmod.MEMBER_FUSED_FLAG
    G = hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED

    def desc(flags, policy=EPS, S=S):
        return hipmod.make_desc(W, H, S, boxes=(7,), policy=policy, flags=flags)
    with hipmod.Context(0) as c, hipmod.MultiContext([0, 0]) as mc:
        calls = entry_points(c, mc, hipmod, planes, (7,))

        def refused(d, status, word, only=None):
            for name, fn in calls.items():
                if only and name not in only:
                    continue
                with pytest.raises(hipmod.RpfError) as e:
                    fn(d)
                assert e.value.status == status and word in str(e.value), (name, str(e.value))
        refused(desc(M | X), hipmod.E_BADARG, "rpf_set_membership")                  # no configuration set
        good = hipmod.membership_preset(hipmod.MEMBERSHIP_PUBLISHED_19)
        for m in (c, mc):
            m.set_membership(good)
        refused(desc(X), hipmod.E_UNSUPPORTED, "MEMBER_FUSED")                       # the bit without RPF_FLAG_MEMBER_TEST
        refused(desc(X | hipmod.FLAG_WIDE_NBHD), hipmod.E_UNSUPPORTED, "MEMBER_FUSED")
        assert hipmod.layout_kernels(desc(X)) == (hipmod.E_UNSUPPORTED, None)
        # with it, the parent's refusals stand
        refused(desc(M | X, REF_ABORT), hipmod.E_UNSUPPORTED, "REF_ABORT")
        refused(desc(M | X | hipmod.FLAG_FAST_WEIGHTS), hipmod.E_UNSUPPORTED, "FAST_WEIGHTS")
        refused(desc(M | X | G | hipmod.FLAG_GENERIC_FAST), hipmod.E_UNSUPPORTED, "GENERIC_FAST")
        refused(desc(M | X | hipmod.FLAG_GENERIC | hipmod.FLAG_STREAM_FAST), hipmod.E_UNSUPPORTED, "STREAM_FAST")
        refused(desc(M | X, S=833), hipmod.E_UNSUPPORTED, "832", only=("rpf_filter_device",))
        # an entry point that runs no pass does not ask
        m0, s0 = c.pixel_stats(planes, desc(M | X))
        m1, s1 = c.pixel_stats(planes, desc(0))
        assert np.array_equal(m0, m1) and np.array_equal(s0, s1, equal_nan=True)
        # ... and accepted again
        assert c.filter_pass_debug(planes, desc(M | X), box=7)["status"] == hipmod.OK and c.route() == 10


def test_s_above_832_is_refused_by_every_entry_point(hipmod):
    W, H, S = 2, 2, 833
    planes = fb.synth_planes(W, H, S, seed=11)
    with hipmod.Context(0) as c, hipmod.MultiContext([0, 0]) as mc:
        for m in (c, mc):
            m.set_membership(hipmod.membership_preset(0))
        for name, fn in entry_points(c, mc, hipmod, planes, (3,)).items():
            with pytest.raises(hipmod.RpfError) as e:
                fn(hipmod.make_desc(W, H, S, boxes=(3,), policy=EPS, flags=hipmod.MEMBER_TEST_FLAG | hipmod.MEMBER_FUSED_FLAG))
            assert e.value.status == hipmod.E_UNSUPPORTED and "832" in str(e.value), (name, str(e.value))
