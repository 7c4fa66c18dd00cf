"""GPU tests of RPF_FLAG_SCHEDULE_FUSED: a pass whose schedule entry has a gain other than 1 on the scheduled
builds of the compiled kernels -- routes 0 to 2, and route 10 under RPF_FLAG_MEMBER_TEST | RPF_FLAG_MEMBER_FUSED.  Held, on every
pixel of every frame, to the same call with gains (1, 1) for everything in front of stage 3c, to tests/schedule_ref.py on the
device's own MI for stage 3c (bit for bit) and on the device's own stage outputs for stage 4 (the per-sample bar of the form the
pixel's kernel uses), to route 9 and route 3 for whole passes, and to chains of one-pass calls for pass sequences.  EPS policy and
seed 0.5 throughout (REF_ABORT is refused with gains).  The frames, gains and their branch coverage are
tests/test_schedule_fused_cpu.py's.

Before the feature a flagged call is not refused without RPF_FLAG_SCHEDULE, a gain other than 1 on the compiled kernels is refused
with it, and MEMBER_FUSED with gains is route 9: groups 1 to 7 fail.  The gains-(1, 1) control of group 1 and group 8 pass before
and after, and are no evidence for the feature."""
import hashlib

import numpy as np
import pytest

import schedule_ref as SRf
import spike_ref
import stage4_bars as B
from raytracer_rpf_amd import feature_buffer as fb
from test_schedule_fused_cpu import CASES, MEMBER_ROWS, REFERENCE_ROWS, SHARE, STREAM, classes_of, frame, mt_of, planes_of
from test_schedule_gpu import TWO

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
SIGMA = 0.5
BITS = ("nbhd_size", "member_hash", "mean", "stddev", "bin_hash", "mi", "wrc")
FRONT = ("nbhd_size", "member_hash", "mean", "stddev", "bin_hash")
PLANES = BITS + ("alpha", "beta", "colour")
DEFAULTS = dict(binning=-1, split_weights=-1, waves_per_pixel=0, packed=-1, table_in_lds=-1)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_or_nan(a, b):
    """bit for bit where neither is a NaN, and the same NaN pattern (a NaN's payload is not part of the contract)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


class options:
    """options set on a shared context, put back on exit"""

    def __init__(self, c, **kw):
        self.c, self.kw = c, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.c.set_option(k, v)

    def __exit__(self, *a):
        for k in self.kw:
            self.c.set_option(k, DEFAULTS[k])


def flags_of(hipmod, member=False, fused=True, sched_fused=True):
    f = hipmod.SCHEDULE_FLAG | (hipmod.SCHEDULE_FUSED_FLAG if sched_fused else 0)
    if member:
        f |= hipmod.MEMBER_TEST_FLAG | (hipmod.MEMBER_FUSED_FLAG if fused else 0)
    return f


def run(c, hipmod, planes, box, gains, mt=None, extra=0, fused=True, sched_fused=True, seed=SIGMA, colour_in=None, lay=None, pass0=0):
    """one pass through rpf_filter_pass_debug under RPF_FLAG_SCHEDULE | RPF_FLAG_SCHEDULE_FUSED (the descriptor's own seed is 0.002:
    the entry's is what counts), with the configured membership test on route 10 when mt is given"""
    _, H, W, S = planes.shape
    if mt is not None:
        c.set_membership(hipmod.make_membership(mt[0].tolist(), mt[1].tolist()))
    c.set_schedule(hipmod.make_schedule([seed] * (pass0 + 1), [1.0] * pass0 + [gains[0]], [1.0] * pass0 + [gains[1]], pass0=pass0))
    desc = hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=0.002, flags=flags_of(hipmod, mt is not None, fused, sched_fused) | extra, **(lay or {}))
    got = c.filter_pass_debug(planes, desc, box=box, colour_in=colour_in)
    cn = c.counters()
    got.update(route=c.route(), launches=cn.filter_kernel_launches, redo_pixels=cn.redo_pixels)
    return got


_stage4 = {}


def stage4_ref(oracle, planes, got, box, mt):
    """schedule_ref.stage4_on on the device's own stage outputs; cached on those outputs (the routes and options of one frame give
    the same bits, so the restatement runs once for them), never modified"""
    h = hashlib.sha1()
    for k in ("nbhd_size", "mean", "stddev", "alpha", "beta", "wrc"):
        h.update(np.ascontiguousarray(got[k]).tobytes())
    key = (planes.shape, box, mt is not None, h.hexdigest())
    if key not in _stage4:
        _stage4[key] = SRf.stage4_on(oracle, planes, got, SIGMA, box, EPS, mt=mt)
        _stage4[key].setflags(write=False)
    return _stage4[key]


def check_stage4(oracle, planes, got, box, mt, label):
    """every sample within the per-sample bar of the form of the kernel that filtered its pixel: "expanded" on the resident classes
    N <= 3136, "direct" on the streaming class; the NaN patterns equal"""
    ref = stage4_ref(oracle, planes, got, box, mt)
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(ref))
    cmax = B.cmax_of(planes[2:5])
    n = got["nbhd_size"]
    both = np.isfinite(got["colour"]) & np.isfinite(ref)
    dist = np.where(both, np.abs(got["colour"] - ref), 0.0).max(axis=(0, 3)) / cmax      # per pixel
    bars = np.empty(n.shape)
    for form, sel in (("expanded", n <= B.RESIDENT), ("direct", n > B.RESIDENT)):
        if sel.any():
            bars[sel] = B.sample_bar(form, 12, int(n[sel].max()), SIGMA, box)
    worst = np.unravel_index(np.argmax(dist / bars), dist.shape)
    print("SCHEDULE_FUSED %s stage 4: worst %.3e (bar %.3e) at pixel %s N %d" % (label, dist[worst], bars[worst], worst, n[worst]))
    assert (dist <= bars).all(), (float(dist[worst]), float(bars[worst]))


def check_scheduled(oracle, hipmod, name, planes, box, gains, base, got, routes, label, mt=None, share=True):
    """the assertions of group 1: the scheduled pass `got` against the gains-(1, 1) pass `base` of the same call and the restatement"""
    gc, gf = gains
    assert got["status"] == hipmod.OK and got["route"] == base["route"] and got["route"] in routes, (got["route"], base["route"], routes)
    for k in ("launches", "redo_pixels", "sum_nbhd", "max_nbhd"):
        assert got[k] == base[k], k
    for k in BITS:                                                       # stages 1 to 3b and W_r_c: the gains-(1, 1) run's bits
        assert same(got[k], base[k]), k
    classes = classes_of(got["nbhd_size"])
    assert set(CASES[name][7]) <= classes, (CASES[name][7], sorted(classes))
    ac, ao = SRf.shares(got["mi"], gc, "c", 1e-10)
    bc, bo = SRf.shares(got["mi"], gf, "f", 1e-10)
    print("SCHEDULE_FUSED %s: route %d, %d launches, N %d .. %d, alpha clamped / open %.3f / %.3f, beta factor %.3f / %.3f" % (
        label, got["route"], got["launches"], got["nbhd_size"].min(), got["nbhd_size"].max(), ac, ao, bc, bo))
    # the control: the gains-(1, 1) run is the unscheduled statement on its own MI (passes before the feature: no evidence for it)
    a1, b1, w1 = SRf.alpha_beta(base["mi"], 1.0, 1.0, 0, 1e-10)
    assert same_or_nan(base["alpha"], a1) and same_or_nan(base["beta"], b1) and same_or_nan(base["wrc"], w1)
    # stage 3c: the restatement on the device's own MI, bit for bit
    a, b, w = SRf.alpha_beta(got["mi"], gc, gf, 0, 1e-10)
    assert same_or_nan(got["alpha"], a) and same_or_nan(got["beta"], b) and same_or_nan(got["wrc"], w)
    with np.errstate(invalid="ignore"):
        assert not (got["alpha"] < 0).any() and not (got["beta"] < 0).any()
    if share:  # (the class-8 frame without the membership test is exempt: tests/test_schedule_fused_cpu.py)
        assert min(ac, ao) >= SHARE and min(bc, bo) >= SHARE, (ac, ao, bc, bo)
        assert not same(got["alpha"], base["alpha"]) and not same(got["beta"], base["beta"])
        assert (got["alpha"] == 0).any()
    check_stage4(oracle, planes, got, box, mt, label)
    if box // 4 > 0 and share:   # (sigma_p = box // 4 = 0 at box 3: every colour falls back to the input, gains or no gains)
        assert not same(got["colour"], base["colour"])


# ---- 1. stage parity on every pixel ------------------------------------------------------------------------------------------------
def route_cases():
    out = []
    for name in REFERENCE_ROWS:
        W, H, S, box = CASES[name][:4]
        out.append((name, "default"))
        # the other setting of option "binning": the size-binned route for a pass the unbinned one takes by default, and -- where one
        # resident kernel can hold the whole window -- the unbinned route for a pass that is size-binned by default
        if box * box * S > 512:
            out.append((name, "binning1"))
            if box * box * S <= B.RESIDENT:
                out.append((name, "binning0"))
        else:
            out.append((name, "binning1"))
    return out


@pytest.mark.parametrize("name,how", route_cases(), ids=["%s-%s" % c for c in route_cases()])
def test_stage_parity_on_routes_0_to_2(ctx, hipmod, oracle, name, how):
    W, H, S, box, _, _, gains, _, share = CASES[name]
    planes = planes_of(name)
    with options(ctx, **({} if how == "default" else dict(binning=int(how[-1])))):
        base = run(ctx, hipmod, planes, box, (1.0, 1.0))
        got = run(ctx, hipmod, planes, box, gains)
    binned = how == "binning1" or (how == "default" and box * box * S > 512)
    check_scheduled(oracle, hipmod, name, planes, box, gains, base, got, (2,) if binned else (0, 1), "%s, %s" % (name, how), share=share)
    if STREAM in CASES[name][7]:
        assert got["max_nbhd"] > B.RESIDENT                              # the streaming kernel took its class


@pytest.mark.parametrize("name", MEMBER_ROWS)
def test_stage_parity_on_route_10(ctx, hipmod, oracle, name):
    W, H, S, box, _, _, gains, _, share = CASES[name]
    planes, mt = planes_of(name), mt_of(name)
    base = run(ctx, hipmod, planes, box, (1.0, 1.0), mt=mt)
    got = run(ctx, hipmod, planes, box, gains, mt=mt)
    check_scheduled(oracle, hipmod, name, planes, box, gains, base, got, (10,), name, mt=mt, share=share)
    assert got["launches"] == len(classes_of(got["nbhd_size"]))          # one launch per non-empty class of the eleven
    if STREAM in CASES[name][7]:
        assert got["max_nbhd"] > B.RESIDENT                              # the wide kernel took its class


# ---- 2. route 10 against route 9 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m-k7", "m-b11"])
def test_route_10_against_route_9(ctx, hipmod, name):
    W, H, S, box, _, _, gains, _, _ = CASES[name]
    planes, mt = planes_of(name), mt_of(name)
    r9 = run(ctx, hipmod, planes, box, gains, mt=mt, sched_fused=False)              # without the new bit: route 9, as before it
    r10 = run(ctx, hipmod, planes, box, gains, mt=mt)
    assert r9["route"] == 9 and r10["route"] == 10 and r9["status"] == r10["status"] == hipmod.OK
    for k in FRONT:
        assert same(r9[k], r10[k]), k
    d = np.abs(r9["colour"] - r10["colour"]).max() / B.cmax_of(planes[2:5])
    print("SCHEDULE_FUSED %s: route 10 against route 9, max |d| / cmax %.3e" % (name, d))
    assert d <= 1e-4


# ---- 3. the compiled 27-dim layout, fp16 planes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("member", [False, True], ids=["default-route", "route10"])
def test_compiled_27_dim_layout(ctx, hipmod, member):
    W, H, S, box, nr, nf = 12, 10, 8, 7, 4, 18
    gains = (1.15, 1.6)
    stored = fb.synth_planes(W, H, S, seed=5, n_random=nr, n_feat=nf, dtype="f16", **(dict(flat_frac=0.5) if member else {}))
    mt = (np.where(np.arange(nf) % 6 >= 3, 30.0, 3.0), np.full(nf, 0.05)) if member else None
    lay = dict(n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16)
    base = run(ctx, hipmod, stored, box, (1.0, 1.0), mt=mt, lay=lay)
    got = run(ctx, hipmod, stored, box, gains, mt=mt, lay=lay)
    assert got["status"] == hipmod.OK and got["route"] == base["route"] and (got["route"] == 10 if member else got["route"] in (0, 1, 2))
    assert (got["launches"], got["redo_pixels"], got["sum_nbhd"], got["max_nbhd"]) == (base["launches"], base["redo_pixels"], base["sum_nbhd"], base["max_nbhd"])
    assert got["nbhd_size"].max() > 64
    for k in BITS:
        assert same(got[k], base[k]), k
    a, b, w = SRf.alpha_beta(got["mi"], gains[0], gains[1], 0, 1e-10, n_random=nr, n_feat=nf)
    assert same_or_nan(got["alpha"], a) and same_or_nan(got["beta"], b) and same_or_nan(got["wrc"], w)
    assert not same(got["alpha"], base["alpha"]) and not same(got["beta"], base["beta"])
    # the same pass on the layout-generic kernels, which know the rule without the new bit: route 3, or route 9 under the test
    c = ctx
    c.set_schedule(hipmod.make_schedule(SIGMA, *gains))
    desc = hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=0.002, flags=hipmod.FLAG_GENERIC | hipmod.SCHEDULE_FLAG |
                            (hipmod.MEMBER_TEST_FLAG if member else 0), **lay)
    ref = c.filter_pass_debug(stored, desc, box=box)
    assert c.route() == (9 if member else 3)
    assert same(ref["nbhd_size"], got["nbhd_size"]) and same(ref["member_hash"], got["member_hash"])
    d = np.abs(ref["colour"] - got["colour"]).max() / B.cmax_of(stored[2:5].astype(np.float32))
    print("SCHEDULE_FUSED d27 %s: against route %d, max |d| / cmax %.3e" % ("route 10" if member else "default", c.route(), d))
    assert d <= 1e-4


# ---- 4. options ---------------------------------------------------------------------------------------------------------------------
def test_options_on_b11(ctx, hipmod, oracle):
    name = "b11"
    W, H, S, box, _, _, gains, _, _ = CASES[name]
    planes = planes_of(name)
    want = run(ctx, hipmod, planes, box, gains)
    assert want["route"] == 2
    bar = B.sample_bar("expanded", 12, int(want["nbhd_size"].max()), SIGMA, box) * B.cmax_of(planes[2:5])
    for opt, values, exact in (("split_weights", (0, 1), True), ("waves_per_pixel", (1, 4), False), ("packed", (0, 1), False),
                               ("table_in_lds", (0, 1), False)):
        for v in values:
            with options(ctx, **{opt: v}):
                got = run(ctx, hipmod, planes, box, gains)
            assert got["route"] == 2 and got["status"] == hipmod.OK, (opt, v)
            for k in BITS + ("alpha", "beta"):                           # the same stage-3c bits throughout
                assert same(got[k], want[k]), (opt, v, k)
            if exact:
                assert same(got["colour"], want["colour"]), (opt, v)
            else:  # two results within the per-sample bar of the restatement each: within twice the bar of each other
                check_stage4(oracle, planes, got, box, None, "b11, %s=%d" % (opt, v))
                assert np.abs(got["colour"] - want["colour"]).max() <= 2 * bar, (opt, v)


# ---- 5. pass sequences ----------------------------------------------------------------------------------------------------------------
def c64_of(c, hipmod, planes, boxes, flags, colour64_in=None):
    _, H, W, S = planes.shape
    desc = hipmod.make_desc(W, H, S, boxes=boxes, policy=EPS, sigma_seed=0.002, flags=flags)
    out = c.filter(planes, desc, colour64_in=colour64_in, want_colour64=True)
    cn = c.counters()
    return out[3], out[2], c.route(), cn.filter_kernel_launches


def test_two_pass_call_on_routes_0_to_2(ctx, hipmod):
    planes, F = planes_of("wave"), flags_of(hipmod)
    ctx.set_schedule(hipmod.make_schedule(**TWO))
    both, st, route, _ = c64_of(ctx, hipmod, planes, (7, 5), F)
    assert st == hipmod.OK and route in (0, 1, 2)
    first, _, _, _ = c64_of(ctx, hipmod, planes, (7,), F)                            # pass0 = 0: entry 0
    ctx.set_schedule(hipmod.make_schedule(pass0=1, **TWO))
    second, _, _, _ = c64_of(ctx, hipmod, planes, (5,), F, colour64_in=first)        # pass0 = 1: entry 1
    assert same(both, second) and not same(both, first)
    ctx.set_schedule(hipmod.make_schedule(**{k: v[::-1] for k, v in TWO.items()}))
    swapped, _, _, _ = c64_of(ctx, hipmod, planes, (7, 5), F)
    assert not same(both, swapped)


def test_two_pass_call_on_route_10_reuses_the_masks(ctx, hipmod):
    planes, mt, F = planes_of("m-k7"), mt_of("m-k7"), flags_of(hipmod, member=True)
    ctx.set_membership(hipmod.make_membership(mt[0].tolist(), mt[1].tolist()))
    entries = dict(seed=[0.5, 0.25], gain_c=[1.1, 1.3], gain_f=[2.0, 1.15])
    ctx.set_schedule(hipmod.make_schedule(**entries))
    both, st, route, launches = c64_of(ctx, hipmod, planes, (7, 7), F)
    assert st == hipmod.OK and route == 10
    first, _, r1, l1 = c64_of(ctx, hipmod, planes, (7,), F)
    ctx.set_schedule(hipmod.make_schedule(pass0=1, **entries))
    second, _, r2, l2 = c64_of(ctx, hipmod, planes, (7,), F, colour64_in=first)
    assert r1 == r2 == 10
    # the masks are keyed by box, rows and table, not by gains: the second pass of the one call deals the same lists to the same
    # classes -- filter_kernel_launches counts filter kernels alone, one per non-empty class and pass -- and gives the chain's bits
    assert launches == l1 + l2 and l1 == l2
    assert same(both, second) and not same(both, first)


def test_mixed_call_runs_the_gains_one_entry_unscheduled(ctx, hipmod):
    planes, F = planes_of("wave"), flags_of(hipmod)
    ctx.set_schedule(hipmod.make_schedule([0.5, 0.25], [1.0, 1.3], [1.0, 1.15]))
    both, st, route, _ = c64_of(ctx, hipmod, planes, (7, 5), F)
    first, _, _, _ = c64_of(ctx, hipmod, planes, (7,), F)                            # entry 0 alone: gains 1
    _, H, W, S = planes.shape
    plain = ctx.filter(planes, hipmod.make_desc(W, H, S, boxes=(7,), policy=EPS, sigma_seed=0.5, flags=0), want_colour64=True)[3]
    assert same(first, plain)                                                        # ... is the unflagged pass with that seed
    ctx.set_schedule(hipmod.make_schedule([0.5, 0.25], [1.0, 1.3], [1.0, 1.15], pass0=1))
    second, _, _, _ = c64_of(ctx, hipmod, planes, (5,), F, colour64_in=plain)
    assert st == hipmod.OK and same(both, second)


# ---- 6. the other entry points --------------------------------------------------------------------------------------------------------
def test_row_band_pipeline_equals_the_serial_call(hipmod):
    planes = planes_of("b11")
    _, H, W, S = planes.shape
    with hipmod.Context(0) as c:
        c.set_schedule(hipmod.make_schedule(**TWO))
        F = flags_of(hipmod)
        serial = c.filter(planes, hipmod.make_desc(W, H, S, boxes=(11, 7), policy=EPS, sigma_seed=0.002, flags=F | hipmod.FLAG_NO_OVERLAP))
        route = c.route()
        pin = c.host_empty(planes.shape, planes.dtype)
        pin[...] = planes
        out_s, out_p = c.host_empty((3, H, W, S)), c.host_empty((H, W, 3))
        out_s[...], out_p[...] = -1.0, -1.0
        _, _, st = c.filter(pin, hipmod.make_desc(W, H, S, boxes=(11, 7), policy=EPS, sigma_seed=0.002, flags=F), out_samples=out_s, out_pixels=out_p)
        assert st == serial[2] == hipmod.OK and c.route() == route and route in (0, 1, 2)
        assert same(np.array(out_s), serial[0]) and same(np.array(out_p), serial[1])
        unscheduled = c.filter(planes, hipmod.make_desc(W, H, S, boxes=(11, 7), policy=EPS, sigma_seed=0.5, flags=hipmod.FLAG_NO_OVERLAP))
        assert not same(unscheduled[0], serial[0])


@pytest.mark.parametrize("devices", [(0,), (0, 0)])
def test_multi_equals_one_context(ctx, hipmod, devices):
    planes, sched = frame(12, 12, 8, seed=3), hipmod.make_schedule(**TWO)
    desc = hipmod.make_desc(12, 12, 8, boxes=(7, 5), policy=EPS, sigma_seed=0.002, flags=flags_of(hipmod))
    ctx.set_schedule(sched)
    s1, p1, st1 = ctx.filter(planes, desc)
    c1 = ctx.counters()
    assert ctx.route() in (0, 1, 2)
    with hipmod.MultiContext(list(devices)) as mc:
        mc.set_schedule(sched)
        s2, p2, st2 = mc.filter(planes, desc)
        c2 = mc.counters()
    assert st1 == st2 == hipmod.OK and same(s1, s2) and same(p1, p2)
    assert (c2.samples_filtered, c2.sum_nbhd, c2.max_nbhd) == (c1.samples_filtered, c1.sum_nbhd, c1.max_nbhd)
    unscheduled = ctx.filter(planes, hipmod.make_desc(12, 12, 8, boxes=(7, 5), policy=EPS, sigma_seed=0.5))[0]
    assert not same(s1, unscheduled)


def test_spike_pass_on_top(ctx, hipmod):
    planes = np.array(planes_of("wave"))
    hit = np.random.default_rng(7).random(planes.shape[1:]) < 0.04
    planes[2:5, hit] *= np.float32(1e3)                                              # fireflies
    F = flags_of(hipmod)
    ctx.set_schedule(hipmod.make_schedule(SIGMA, *CASES["wave"][6]))
    plain, st, route, _ = c64_of(ctx, hipmod, planes, (7,), F)
    ctx.set_spike(1.0, True)
    spiked, st2, route2, _ = c64_of(ctx, hipmod, planes, (7,), F | hipmod.FLAG_SPIKE_CLAMP)
    stats = ctx.spike_stats()
    want = spike_ref.apply(plain, 1.0, True)
    assert st == st2 == hipmod.OK and route == route2 and route in (0, 1, 2)
    assert stats.applied == 1 and stats.spike_samples == want["spike_samples"] > 0
    assert same(spiked, want["colour"])


def test_pass_report_on_top(ctx, hipmod):
    name = "wave"
    W, H, S, box, _, _, gains, _, _ = CASES[name]
    planes = planes_of(name)
    plain = run(ctx, hipmod, planes, box, gains)
    got = run(ctx, hipmod, planes, box, gains, extra=hipmod.PASS_REPORT_FLAG)
    rep = ctx.pass_report(0)
    assert rep.applied == 1 and rep.route == got["route"] == plain["route"]
    for k in PLANES:
        assert same(got[k], plain[k]), k
    zeros = [int((got["alpha"][..., c] == 0).sum()) for c in range(3)]
    assert list(rep.total.alpha_zero) == zeros and sum(zeros) > 0


# ---- 7. refusals, each before any device work ------------------------------------------------------------------------------------------
def test_refusals(hipmod):
    planes = frame(12, 10, 8)
    _, H, W, S = planes.shape
    F, X = hipmod.SCHEDULE_FLAG, hipmod.SCHEDULE_FUSED_FLAG

    def desc(flags, boxes=(7,), policy=EPS):
        return hipmod.make_desc(W, H, S, boxes=boxes, policy=policy, sigma_seed=SIGMA, flags=flags)
    with hipmod.Context(0) as c, hipmod.MultiContext([0, 0]) as mc:
        assert c.filter(planes, desc(0))[2] == hipmod.OK                             # the previous call, whose counters must stay
        before = bytes(c.counters())

        def refused(d, status, word, box=7):
            for name, call in (("rpf_filter", lambda: c.filter(planes, d)), ("rpf_filter_ex", lambda: c.filter(planes, d, want_colour64=True)),
                               ("rpf_filter_device", lambda: c.filter_device(d, None, None)),
                               ("rpf_filter_pass_debug", lambda: c.filter_pass_debug(planes, d, box=box)),
                               ("rpf_multi_filter", lambda: mc.filter(planes, d))):
                with pytest.raises(hipmod.RpfError) as e:
                    call()
                assert e.value.status == status and word in str(e.value), (name, str(e.value))
            assert bytes(c.counters()) == before
        refused(desc(X), hipmod.E_UNSUPPORTED, "RPF_FLAG_SCHEDULE_FUSED")            # the bit without RPF_FLAG_SCHEDULE
        refused(desc(X | hipmod.FLAG_GENERIC), hipmod.E_UNSUPPORTED, "RPF_FLAG_SCHEDULE_FUSED")
        refused(desc(F | X), hipmod.E_BADARG, "rpf_set_schedule")                    # the bit without a table
        for m in (c, mc):
            m.set_schedule(hipmod.make_schedule(SIGMA, 1.15, 1.6))
        refused(desc(F | X, policy=REF_ABORT), hipmod.E_UNSUPPORTED, "REF_ABORT")    # gains under REF_ABORT: the older refusal
        d = desc(F | X | hipmod.FLAG_FAST_WEIGHTS)                                   # gains with the fp32 pair weights: both flags named
        refused(d, hipmod.E_UNSUPPORTED, "RPF_FLAG_SCHEDULE_FUSED")
        refused(d, hipmod.E_UNSUPPORTED, "RPF_FLAG_FAST_WEIGHTS")
        refused(desc(F), hipmod.E_UNSUPPORTED, "RPF_FLAG_GENERIC")                   # and without the bit nothing changed
        # accepted: the fp32 pair weights with a gains-(1, 1) table under the bit, and the gains without them
        for m in (c, mc):
            m.set_schedule(hipmod.make_schedule(SIGMA, 1.0, 1.0))
        fast = c.filter(planes, desc(F | X | hipmod.FLAG_FAST_WEIGHTS))
        assert fast[2] == hipmod.OK and c.route() in (0, 1, 2)
        assert same(fast[0], c.filter(planes, desc(hipmod.FLAG_FAST_WEIGHTS))[0])
        assert mc.filter(planes, desc(F | X | hipmod.FLAG_FAST_WEIGHTS))[2] == hipmod.OK
        c.set_schedule(hipmod.make_schedule(SIGMA, 1.15, 1.6))
        assert c.filter_pass_debug(planes, desc(F | X), box=7)["status"] == hipmod.OK and c.route() in (0, 1, 2)


# ---- 8. afterwards ------------------------------------------------------------------------------------------------------------------
def test_unflagged_call_after_a_flagged_one(ctx, hipmod):
    W, H, S, box = CASES["wave"][:4]
    planes = planes_of("wave")
    desc = hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=SIGMA)

    def plain():
        got = ctx.filter_pass_debug(planes, desc, box=box)
        cn = ctx.counters()
        got.update(route=ctx.route(), launches=cn.filter_kernel_launches, redo_pixels=cn.redo_pixels)
        return got
    want = plain()
    try:
        flagged = run(ctx, hipmod, planes, box, CASES["wave"][6])
    except hipmod.RpfError:   # (before the feature the flagged call is refused: what is claimed here is the unflagged call's bits)
        flagged = None
    got = plain()
    assert got["route"] == want["route"] and (got["launches"], got["redo_pixels"]) == (want["launches"], want["redo_pixels"])
    for k in PLANES:
        assert same(got[k], want[k]), k
    if flagged is not None:
        assert flagged["status"] == hipmod.OK and not same(flagged["colour"], got["colour"])
