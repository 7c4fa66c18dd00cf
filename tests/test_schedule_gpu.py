"""GPU tests of the per-pass schedule (RPF_FLAG_SCHEDULE) against the numpy restatement
tests/schedule_ref.py, on every pixel of every frame: stage parity on the packed, one-wave, streaming and wide kernels (alpha and
beta bit for bit from the device's own MI, colours within the direct form's per-sample bar), the flag composed with the membership
test, a sampled pass, the spike pass and the two fp32 flags, per-pass indexing and pass0, seeds alone on the fused routes under
both policies, the anchor (preset 0 is the unflagged call), MultiContext, the refusals, and an unflagged call after a flagged
one.  EPS policy and seed 0.5 unless stated.  The frames, gains and their branch coverage are tests/test_schedule_cpu.py's."""
import numpy as np
import pytest

import member_test_ref as MR
import schedule_ref as SRf
import spike_ref
import stage4_bars as B
from test_generic_fast_gpu import REL_L2_BAR as CLASS_FAST_BAR          # the contract bar of RPF_FLAG_GENERIC_FAST
from test_schedule_cpu import CASES, MEMBER_GAINS, SAMPLED, SHARE, class_of, frame, gains_of, planes_of
from test_stream_fast_gpu import REL_L2_BAR as STREAM_FAST_BAR          # ... and of RPF_FLAG_STREAM_FAST

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
SIGMA = 0.5
BITS = ("nbhd_size", "member_hash", "mean", "stddev", "bin_hash", "mi", "wrc")
PLANES = BITS + ("alpha", "beta", "colour")
TWO = dict(seed=[0.5, 0.25], gain_c=[1.15, 1.3], gain_f=[1.6, 1.15])     # the entries of the two-pass cases


def gpw(hipmod):
    return hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED | hipmod.FLAG_GENERIC_WAVE


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def run(c, hipmod, planes, box, sched=None, extra=0, policy=EPS, seed=SIGMA, allow_nonfinite=False):
    """one pass through rpf_filter_pass_debug: sched a Schedule -> under the flag (the descriptor keeps `seed`, which the flag
    overrides), None -> without it"""
    _, H, W, S = planes.shape
    if sched is not None:
        c.set_schedule(sched)
    desc = hipmod.make_desc(W, H, S, policy=policy, sigma_seed=seed, flags=(hipmod.SCHEDULE_FLAG if sched is not None else 0) | extra)
    got = c.filter_pass_debug(planes, desc, box=box, allow_nonfinite=allow_nonfinite)
    cn = c.counters()
    got.update(route=c.route(), launches=cn.filter_kernel_launches, redo_pixels=cn.redo_pixels)
    return got


def check_scheduled(oracle, hipmod, planes, box, gains, base, got, route, label, mt=None, cfg=None):
    """the assertions of a scheduled pass `got` against the unflagged pass `base` of the same flags and the restatement"""
    gc, gf = gains
    assert got["status"] == hipmod.OK and got["route"] == base["route"] == route, (got["route"], base["route"])
    for k in ("launches", "redo_pixels", "sum_nbhd", "max_nbhd"):
        assert got[k] == base[k], k
    for k in BITS:                                                       # stages 1 to 3b and W_r_c: the unflagged run's bits
        assert same(got[k], base[k]), k
    # branch coverage, from the restatement on the device's own MI
    ac, ao = SRf.shares(got["mi"], gc, "c", 1e-10)
    bc, bo = SRf.shares(got["mi"], gf, "f", 1e-10)
    print("SCHEDULE %s: route %d, N %d .. %d, alpha clamped / open %.3f / %.3f, beta factor %.3f / %.3f" % (
        label, route, got["nbhd_size"].min(), got["nbhd_size"].max(), ac, ao, bc, bo))
    assert min(ac, ao) >= SHARE and min(bc, bo) >= SHARE, (ac, ao, bc, bo)
    # stage 3c: the restatement on the device's own MI, bit for bit
    a, b, w = SRf.alpha_beta(got["mi"], gc, gf, 0, 1e-10)
    assert same(got["alpha"], a) and same(got["beta"], b) and same(got["wrc"], w)
    assert not same(got["alpha"], base["alpha"]) and not same(got["beta"], base["beta"])
    assert (got["alpha"] == 0).any() and not (got["alpha"] < 0).any() and not (got["beta"] < 0).any()
    # stage 4: the restatement on the device's own stage outputs, every sample, the direct form's bar
    ref = SRf.stage4_on(oracle, planes, got, SIGMA, box, EPS, mt=mt, cfg=cfg)
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(ref))
    cmax = B.cmax_of(planes[2:5])
    bar = B.sample_bar("direct", 12, int(got["nbhd_size"].max()), SIGMA, box)
    worst = B.worst_sample(got["colour"], ref) / cmax
    print("SCHEDULE %s stage 4: worst %.3e (bar %.3e)" % (label, worst, bar))
    assert worst <= bar, (worst, bar)
    if box // 4 > 0:   # (sigma_p = box // 4 = 0 at box 3: every weight is NaN and every colour falls back to the input, flag or no flag)
        assert not same(got["colour"], base["colour"])


# ---- 1. stage parity on every pixel: routes 4 / 5 -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_stage_parity_on_every_pixel(ctx, hipmod, oracle, name):
    W, H, S, box, _, _, reach = CASES[name]
    planes, gains = planes_of(name), gains_of(name)
    base = run(ctx, hipmod, planes, box, None, gpw(hipmod))
    got = run(ctx, hipmod, planes, box, hipmod.make_schedule(SIGMA, *gains), gpw(hipmod), seed=0.002)
    classes = {class_of(int(n)) for n in got["nbhd_size"].ravel()}
    assert set(reach) <= classes, (reach, sorted(classes))
    check_scheduled(oracle, hipmod, planes, box, gains, base, got, 5, name)
    if name == "rest":
        assert got["max_nbhd"] > 832                                                 # the streaming kernel took the rest list


# ---- 2. the wide kernel: routes 6 and 7 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [False, True], ids=["route6", "route7"])
def test_wide_kernel(hipmod, oracle, classes):
    W, H, S, box, _, _, _ = CASES["wave"]
    planes, gains = planes_of("wave"), gains_of("wave")
    extra = hipmod.FLAG_WIDE_NBHD | (hipmod.FLAG_WIDE_CLASSES if classes else 0)
    with hipmod.Context(0) as c:
        c.set_option("wide", 1)
        base = run(c, hipmod, planes, box, None, extra)
        got = run(c, hipmod, planes, box, hipmod.make_schedule(SIGMA, *gains), extra)
    check_scheduled(oracle, hipmod, planes, box, gains, base, got, 7 if classes else 6, "wave, wide")


# ---- 3. composition: the membership test, a sampled pass, the spike pass ------------------------------------------------------
def test_with_the_membership_test(ctx, hipmod, oracle):
    W, H, S, box, _, _, _ = CASES["preset"]
    planes, gains, mt = planes_of("preset"), MEMBER_GAINS, MR.published19()   # (why not the preset's gains: test_schedule_cpu.py)
    ctx.set_membership(hipmod.make_membership(mt[0].tolist(), mt[1].tolist()))
    base = run(ctx, hipmod, planes, box, None, hipmod.MEMBER_TEST_FLAG)
    got = run(ctx, hipmod, planes, box, hipmod.make_schedule(SIGMA, *gains), hipmod.MEMBER_TEST_FLAG)
    check_scheduled(oracle, hipmod, planes, box, gains, base, got, 9, "preset, member test", mt=mt)
    want = SRf.scheduled_pass(oracle, planes, (SIGMA,) + gains, box, mt=mt)
    assert np.array_equal(got["nbhd_size"], want["nbhd_size"]) and same(got["mean"], want["mean"]) and same(got["stddev"], want["stddev"])
    np.testing.assert_allclose(got["mi"], want["mi"], rtol=0, atol=1e-11)            # check_pass's bars
    np.testing.assert_allclose(got["wrc"], want["wrc"], rtol=1e-9, atol=1e-12)       # (alpha / beta: bit for bit from the device's MI above)
    assert np.abs(got["colour"] - want["colour"]).max() <= 1e-4 * B.cmax_of(planes[2:5])


def test_with_a_sampled_pass(ctx, hipmod, oracle):
    W, H, S, box, D, SEED, gains = (SAMPLED[k] for k in ("W", "H", "S", "box", "draws", "seed", "gains"))
    planes = frame(W, H, S)
    ctx.set_sampling(hipmod.make_sampling(SEED, [D]))
    base = run(ctx, hipmod, planes, box, None, hipmod.SAMPLED_NBHD_FLAG)
    got = run(ctx, hipmod, planes, box, hipmod.make_schedule(SIGMA, *gains), hipmod.SAMPLED_NBHD_FLAG)
    check_scheduled(oracle, hipmod, planes, box, gains, base, got, 8, "sampled", cfg=(SEED, 0, D))
    want = SRf.scheduled_pass(oracle, planes, (SIGMA,) + gains, box, cfg=(SEED, 0, D))
    assert np.array_equal(got["nbhd_size"], want["nbhd_size"]) and same(got["mean"], want["mean"]) and same(got["stddev"], want["stddev"])
    np.testing.assert_allclose(got["mi"], want["mi"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got["wrc"], want["wrc"], rtol=1e-9, atol=1e-12)       # (alpha / beta: bit for bit from the device's MI above)


def c64_of(c, hipmod, planes, boxes, flags, colour64_in=None, policy=EPS, seed=0.002, allow_nonfinite=False):
    _, H, W, S = planes.shape
    desc = hipmod.make_desc(W, H, S, boxes=boxes, policy=policy, sigma_seed=seed, flags=flags)
    out = c.filter(planes, desc, colour64_in=colour64_in, want_colour64=True, allow_nonfinite=allow_nonfinite)
    return out[3], out[2], c.route()


def test_spike_pass_on_top(ctx, hipmod):
    planes = np.array(planes_of("wave-c"))
    hit = np.random.default_rng(7).random(planes.shape[1:]) < 0.04
    planes[2:5, hit] *= np.float32(1e3)                                              # fireflies
    F = gpw(hipmod) | hipmod.SCHEDULE_FLAG
    ctx.set_schedule(hipmod.make_schedule(SIGMA, *gains_of("wave-c")))
    plain, st, route = c64_of(ctx, hipmod, planes, (7,), F)
    ctx.set_spike(1.0, True)
    spiked, st2, route2 = c64_of(ctx, hipmod, planes, (7,), F | hipmod.FLAG_SPIKE_CLAMP)
    stats = ctx.spike_stats()
    want = spike_ref.apply(plain, 1.0, True)
    assert st == st2 == hipmod.OK and route == route2 == 5 and stats.applied == 1 and stats.spike_samples == want["spike_samples"] > 0
    assert same(spiked, want["colour"])
    unscheduled, _, _ = c64_of(ctx, hipmod, planes, (7,), gpw(hipmod), seed=SIGMA)
    assert not same(plain, unscheduled)


# ---- 4. fp32 pair weights: the coefficients come from the scheduled alpha / beta ------------------------------------------------
def test_generic_fast_on_route_5(ctx, hipmod):
    W, H, S, box, _, _, _ = CASES["wave"]
    planes, sched = planes_of("wave"), hipmod.make_schedule(SIGMA, *gains_of("wave"))
    f64 = run(ctx, hipmod, planes, box, sched, gpw(hipmod))
    f32 = run(ctx, hipmod, planes, box, sched, gpw(hipmod) | hipmod.FLAG_GENERIC_FAST)
    assert f32["route"] == f64["route"] == 5 and f32["launches"] == f64["launches"]
    for k in BITS + ("alpha", "beta"):
        assert same(f32[k], f64[k]), k
    d = rel_l2(f32["colour"], f64["colour"])
    print("SCHEDULE GENERIC_FAST: rel-L2 against the fp64 run %.3e (bar %.1e)" % (d, CLASS_FAST_BAR))
    assert 0 < d <= CLASS_FAST_BAR


def test_stream_fast_on_route_6(hipmod):
    W, H, S, box, _, _, _ = CASES["wave"]
    planes, sched = planes_of("wave"), hipmod.make_schedule(SIGMA, *gains_of("wave"))
    with hipmod.Context(0) as c:
        c.set_option("wide", 1)
        f64 = run(c, hipmod, planes, box, sched, hipmod.FLAG_WIDE_NBHD)
        f32 = run(c, hipmod, planes, box, sched, hipmod.FLAG_WIDE_NBHD | hipmod.FLAG_STREAM_FAST)
    assert f32["route"] == f64["route"] == 6 and f32["launches"] == f64["launches"]
    for k in BITS + ("alpha", "beta"):
        assert same(f32[k], f64[k]), k
    d = rel_l2(f32["colour"], f64["colour"])
    print("SCHEDULE STREAM_FAST: rel-L2 against the fp64 run %.3e (bar %.1e)" % (d, STREAM_FAST_BAR))
    assert 0 < d <= STREAM_FAST_BAR


# ---- 5. per-pass indexing ------------------------------------------------------------------------------------------------------
def test_two_pass_call_indexes_the_table_by_pass(ctx, hipmod):
    planes, F = planes_of("wave"), gpw(hipmod) | hipmod.SCHEDULE_FLAG
    ctx.set_schedule(hipmod.make_schedule(**TWO))
    both, st, route = c64_of(ctx, hipmod, planes, (7, 5), F)
    assert st == hipmod.OK and route == 5
    first, _, _ = c64_of(ctx, hipmod, planes, (7,), F)                               # pass0 = 0: entry 0
    ctx.set_schedule(hipmod.make_schedule(pass0=1, **TWO))
    second, _, _ = c64_of(ctx, hipmod, planes, (5,), F, colour64_in=first)           # pass0 = 1: entry 1
    assert same(both, second) and not same(both, first)
    ctx.set_schedule(hipmod.make_schedule(**{k: v[::-1] for k, v in TWO.items()}))
    swapped, _, _ = c64_of(ctx, hipmod, planes, (7, 5), F)
    assert not same(both, swapped)


def test_pass_debug_reads_entry_pass0(ctx, hipmod):
    W, H, S, box, _, _, _ = CASES["wave"]
    planes = planes_of("wave")
    want = run(ctx, hipmod, planes, box, hipmod.make_schedule(0.25, 1.3, 1.15), gpw(hipmod))
    got = run(ctx, hipmod, planes, box, hipmod.make_schedule([9.0, 9.0, 9.0, 0.25], [0.0, 0.0, 0.0, 1.3], [0.0, 0.0, 0.0, 1.15], pass0=3), gpw(hipmod))
    for k in PLANES:
        assert same(got[k], want[k]), k


# ---- 6. seeds only, on the fused routes, under both policies ------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
def test_seeds_alone_run_the_fused_routes(ctx, hipmod, policy):
    planes = frame(12, 10, 8)
    ctx.set_schedule(hipmod.make_schedule([0.5, 0.25], 1.0, 1.0))
    got, st, route = c64_of(ctx, hipmod, planes, (7, 5), hipmod.SCHEDULE_FLAG, policy=policy, seed=0.002, allow_nonfinite=True)
    assert route in (0, 1, 2)
    first, st1, _ = c64_of(ctx, hipmod, planes, (7,), 0, policy=policy, seed=0.5, allow_nonfinite=True)
    second, st2, route2 = c64_of(ctx, hipmod, planes, (5,), 0, colour64_in=first, policy=policy, seed=0.25, allow_nonfinite=True)
    assert route2 == route and st == st2
    assert same(got, second) and not same(got, first)
    ignored, _, _ = c64_of(ctx, hipmod, planes, (7, 5), 0, policy=policy, seed=0.002, allow_nonfinite=True)
    assert not same(got, ignored)                                                    # the descriptor's own seed was not used


# ---- 7. the anchor: preset 0 is the unflagged call ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["fused", "route5", "route9"])
def test_anchor_preset_zero_is_the_unflagged_call(ctx, hipmod, which):
    W, H, S, box, _, _, _ = CASES["preset"]
    planes = planes_of("preset")
    extra = {"fused": 0, "route5": gpw(hipmod), "route9": hipmod.MEMBER_TEST_FLAG}[which]
    if which == "route9":
        ctx.set_membership(hipmod.membership_preset(hipmod.MEMBERSHIP_PUBLISHED_19))
    for policy in ((EPS, REF_ABORT) if which != "route9" else (EPS,)):
        want = run(ctx, hipmod, planes, box, None, extra, policy=policy, seed=0.002, allow_nonfinite=True)
        got = run(ctx, hipmod, planes, box, hipmod.schedule_preset(hipmod.SCHEDULE_REFERENCE, S), extra, policy=policy, seed=0.75,
                  allow_nonfinite=True)
        assert got["route"] == want["route"] and (got["route"] in (0, 1) if which == "fused" else got["route"] == int(which[-1]))
        for k in ("status", "launches", "redo_pixels", "sum_nbhd", "max_nbhd"):
            assert got[k] == want[k], k
        for k in PLANES:
            assert same(got[k], want[k]), (k, policy)


# ---- 8. MultiContext ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [(0,), (0, 0)])
def test_multi_equals_one_context(ctx, hipmod, devices):
    planes, sched = frame(12, 12, 8, seed=3), hipmod.make_schedule(**TWO)
    desc = hipmod.make_desc(12, 12, 8, boxes=(7, 5), policy=EPS, sigma_seed=0.002, flags=gpw(hipmod) | hipmod.SCHEDULE_FLAG)
    ctx.set_schedule(sched)
    s1, p1, st1 = ctx.filter(planes, desc)
    c1 = ctx.counters()
    assert ctx.route() == 5
    with hipmod.MultiContext(list(devices)) as mc:
        mc.set_schedule(sched)
        s2, p2, st2 = mc.filter(planes, desc)
        c2 = mc.counters()
    assert st1 == st2 == hipmod.OK and same(s1, s2) and same(p1, p2)
    assert (c2.samples_filtered, c2.sum_nbhd, c2.max_nbhd) == (c1.samples_filtered, c1.sum_nbhd, c1.max_nbhd)
    unscheduled = ctx.filter(planes, hipmod.make_desc(12, 12, 8, boxes=(7, 5), policy=EPS, sigma_seed=0.5, flags=gpw(hipmod)))[0]
    assert not same(s1, unscheduled)


# ---- 9. refusals, each before any device work ---------------------------------------------------------------------------------------
def test_refusals(hipmod):
    planes = frame(12, 10, 8)
    _, H, W, S = planes.shape
    F, G = hipmod.SCHEDULE_FLAG, gpw(hipmod)

    def desc(flags, boxes=(7,), policy=EPS):
        return hipmod.make_desc(W, H, S, boxes=boxes, policy=policy, sigma_seed=SIGMA, flags=flags)
    with hipmod.Context(0) as c, hipmod.MultiContext([0, 0]) as mc:
        assert c.filter(planes, desc(G))[2] == hipmod.OK                             # the previous call, whose counters must stay
        before = bytes(c.counters())

        def refused(d, status, word, box=7):
            for name, call in (("rpf_filter", lambda: c.filter(planes, d)), ("rpf_filter_ex", lambda: c.filter(planes, d, want_colour64=True)),
                               ("rpf_filter_device", lambda: c.filter_device(d, None, None)),
                               ("rpf_filter_pass_debug", lambda: c.filter_pass_debug(planes, d, box=box)),
                               ("rpf_multi_filter", lambda: mc.filter(planes, d))):
                if name == "rpf_filter_pass_debug" and d.n_box > 1:
                    continue                                                         # one pass: it reads entry pass0 alone
                with pytest.raises(hipmod.RpfError) as e:
                    call()
                assert e.value.status == status and word in str(e.value), (name, str(e.value))
            assert bytes(c.counters()) == before
        refused(desc(F | G), hipmod.E_BADARG, "rpf_set_schedule")                    # the flag without a table
        m0, s0 = c.pixel_stats(planes, desc(F | G))                                  # ... which an entry point that runs no pass ignores
        m1, s1 = c.pixel_stats(planes, desc(G))
        assert same(m0, m1) and same(s0, s1)
        good = hipmod.make_schedule(SIGMA, 1.15, 1.6)
        for field, e, bad in [("gain_c", 0, -0.5), ("gain_f", 7, -1e-300), ("gain_c", 3, np.inf), ("gain_f", 2, np.nan), ("seed", 0, np.nan),
                              ("seed", 7, 0.0), ("seed", 4, -0.5), ("seed", 1, np.inf), ("pass0", None, 8), ("pass0", None, -1)]:
            cfg = hipmod.make_schedule(SIGMA, 1.15, 1.6)
            if e is None:
                cfg.pass0 = bad
            else:
                getattr(cfg, field)[e] = bad
            for m in (c, mc):
                with pytest.raises(hipmod.RpfError) as err:
                    m.set_schedule(cfg)
                assert err.value.status == hipmod.E_BADARG, (field, e, bad)
        for m in (c, mc):
            with pytest.raises(hipmod.RpfError):
                m.set_schedule(None)
        refused(desc(F | G), hipmod.E_BADARG, "rpf_set_schedule")                    # a refused table is no table
        zero = hipmod.make_schedule(SIGMA, 0.0, 0.0)                                 # a gain of 0 is a gain: alpha = 1, beta = W_c
        for m in (c, mc):
            m.set_schedule(zero)
            m.set_schedule(hipmod.make_schedule(SIGMA, 1.15, 1.6, pass0=7))
        refused(desc(F | G, boxes=(7, 5)), hipmod.E_BADARG, "RPF_MAX_BOXES")         # pass0 = 7 with two boxes
        for m in (c, mc):
            m.set_schedule(good)
        refused(desc(F), hipmod.E_UNSUPPORTED, "RPF_FLAG_GENERIC")                   # a gain of 1.15 on the fused kernels
        refused(desc(F | hipmod.FLAG_WIDE_NBHD), hipmod.E_UNSUPPORTED, "RPF_FLAG_GENERIC")   # ... which a box-7 pass of a wide call runs
        refused(desc(F | hipmod.FLAG_GENERIC, policy=REF_ABORT), hipmod.E_UNSUPPORTED, "REF_ABORT")
        for m in (c, mc):                                                            # the second pass alone is scheduled: still refused
            m.set_schedule(hipmod.make_schedule(SIGMA, [1.0, 1.15], [1.0, 1.0]))
        refused(desc(F, boxes=(7, 5)), hipmod.E_UNSUPPORTED, "RPF_FLAG_GENERIC")
        assert c.filter(planes, desc(F))[2] == hipmod.OK and c.route() in (0, 1, 2)  # ... and one box reads entry 0 alone: gains 1
        # accepted again
        c.set_schedule(good)
        assert c.filter_pass_debug(planes, desc(F | G), box=7)["status"] == hipmod.OK and c.route() == 5


# ---- 10. an unflagged call after a flagged one ----------------------------------------------------------------------------------
def test_unflagged_call_after_a_flagged_one(ctx, hipmod):
    W, H, S, box, _, _, _ = CASES["wave"]
    planes = planes_of("wave")
    for extra in (gpw(hipmod), 0):
        want = run(ctx, hipmod, planes, box, None, extra)
        flagged = run(ctx, hipmod, planes, box, hipmod.make_schedule(0.25, 1.3 if extra else 1.0, 1.15 if extra else 1.0), extra)
        got = run(ctx, hipmod, planes, box, None, extra)
        assert got["route"] == want["route"] == flagged["route"]
        assert (got["launches"], got["redo_pixels"]) == (want["launches"], want["redo_pixels"])
        for k in PLANES:
            assert same(got[k], want[k]), k
        assert not same(flagged["colour"], got["colour"])
