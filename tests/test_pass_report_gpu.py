"""GPU tests of the per-pass activity report (RPF_FLAG_PASS_REPORT).  Every comparison is bit for bit
against the numpy restatement tests/pass_report_ref.py: the device half on synthetic planes at every shape at which the kernels
change path, the flag end to end on every route (the restatement's inputs come from a call per pass to rpf_filter_pass_debug
WITHOUT the flag), composition and edge cases, MultiContext against one context, and the refusals.  The frames and what they
cover are tests/test_pass_report_cpu.py's."""
import ctypes as C

import numpy as np
import pytest

import pass_report_ref as PR
from raytracer_rpf_amd import feature_buffer as fb
from test_pass_report_cpu import ACTIVE, BOX, CLUSTERED, FLAT, IDENTITY, SCHED_GAINS, colours_of, frame

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
TILE_MAX_S = 512   # kReportTileMaxS: above it the pixel kernel is the one-thread-per-pixel form


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_rows(got_rows, want_recs, label=""):
    assert len(got_rows) == len(want_recs), (label, len(got_rows), len(want_recs))
    for y, (g, w) in enumerate(zip(got_rows, want_recs)):
        assert PR.differing(PR.of_ctypes(g), w) == [], (label, "row", y, PR.differing(PR.of_ctypes(g), w))


def assert_report(rep, want_recs, label=""):
    """a PassReport against the fold of the restatement's rows"""
    assert rep.applied == 1 and rep.rows == len(want_recs), (label, rep.applied, rep.rows)
    d = PR.differing(PR.of_ctypes(rep.total), PR.fold(want_recs))
    assert d == [], (label, d)


# ---- 1. the device half on synthetic planes -----------------------------------------------------------------------------------------
def synthetic(Wd, Hd, Sd, nF, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((3, Hd, Wd, Sd)) * 10.0 ** rng.integers(-3, 4, (3, Hd, Wd, 1))
    b = a + np.where(rng.random((1, Hd, Wd, Sd)) < 0.5, 0.0, rng.standard_normal((3, Hd, Wd, Sd)) * 1e-3)   # half the samples stay
    nbhd = rng.choice(np.array([Sd, 1, 8, 9, 64, 65, 448, 832, 833, 3000, 70000], np.int32), (Hd, Wd)).astype(np.int32)
    return a, b, nbhd, rng.random((Hd, Wd, 3)), rng.random((Hd, Wd, nF)), rng.random((Hd, Wd))


def device_rows(ctx, hipmod, a, b, nbhd, alpha, beta, wrc, nF, r0=0, r1=None):
    import torch
    dev = torch.device("cuda", 0)
    _, Hd, Wd, Sd = a.shape
    up = [None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (a, b, nbhd, alpha, beta, wrc)]
    ptr = [None if t is None else t.data_ptr() for t in up]
    desc = hipmod.make_desc(Wd, Hd, Sd, row_begin=r0, row_end=r1, n_feat=nF, n_random=2 if nF != 12 else 0,
                            flags=hipmod.FLAG_GENERIC if nF != 12 else 0)
    rows = ctx.pass_report_rows_device(desc, *ptr, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rows


def check_device(ctx, hipmod, a, b, nbhd, alpha, beta, wrc, nF, r0=0, r1=None, label=""):
    rows = device_rows(ctx, hipmod, a, b, nbhd, alpha, beta, wrc, nF, r0, r1)
    want = PR.rows(a, b, nbhd, alpha, beta, wrc, r0, r1)
    assert_rows(rows, want, label)
    assert PR.differing(PR.of_ctypes(hipmod.pass_report_fold(rows)), PR.fold(want)) == [], label
    return want


@pytest.mark.parametrize("Sd", [1, 8, 65, TILE_MAX_S + 1])
@pytest.mark.parametrize("Wd", [1, 63, 64, 65, 257])
def test_device_half_at_every_path(ctx, hipmod, Wd, Sd):
    a, b, nbhd, alpha, beta, wrc = synthetic(Wd, 3, Sd, 12, 1000 * Wd + Sd)
    want = check_device(ctx, hipmod, a, b, nbhd, alpha, beta, wrc, 12, label="W %d S %d" % (Wd, Sd))
    t = PR.fold(want)
    assert 0 < t["unchanged_samples"] < 3 * Wd * Sd or Wd * Sd < 4
    assert t["class_pixels"].sum() == 3 * Wd


def test_device_half_on_a_row_slab_and_other_feature_counts(ctx, hipmod):
    for nF, Hd in ((12, 6), (7, 5), (33, 4)):
        a, b, nbhd, alpha, beta, wrc = synthetic(37, Hd, 5, nF, nF)
        check_device(ctx, hipmod, a, b, nbhd, alpha, beta, wrc, nF, 1, Hd - 1, label="slab nF %d" % nF)


def test_device_half_with_non_finite_colours(ctx, hipmod):
    a, b, nbhd, alpha, beta, wrc = synthetic(70, 3, 8, 12, 77)
    a[0, 0, 3, 2] = np.nan                       # in a only
    a[2, 1, 69, 7] = -np.inf
    b[1, 0, 5, 0] = np.inf                       # in b only
    b[0, 2, 0, 1] = np.nan
    a[1, 1, 10, 4] = b[1, 1, 10, 4] = np.nan     # in both: same sample
    a[0, 2, 40, 0] = np.inf                      # in both: two samples of one pixel
    b[2, 2, 40, 5] = np.nan
    b[:, 1, 11, :] = a[:, 1, 11, :]              # an unchanged pixel beside a bad one
    want = check_device(ctx, hipmod, a, b, nbhd, alpha, beta, wrc, 12, label="non-finite colours")
    t = PR.fold(want)
    assert (t["nonfinite_pixels"], t["nonfinite_samples"]) == (6, 7)


def test_device_half_with_non_finite_and_negative_zero_weights(ctx, hipmod):
    a, b, nbhd, alpha, beta, wrc = synthetic(65, 3, 4, 12, 78)
    alpha[0, :, 0] = -0.0                        # a row whose alpha sum is -0.0
    alpha[1, 0, 1] = np.nan
    alpha[1, 64, 2] = 0.0
    alpha[2, 0, 0] = -0.0                        # the chain's first term
    beta[0, 7, 3] = np.inf
    beta[2, 64, 11] = -np.inf
    beta[1, :, 5] = 0.0
    beta[1, 9, 5] = -0.0
    wrc[2, 33] = np.nan
    wrc[0, 0] = -0.0
    want = check_device(ctx, hipmod, a, b, nbhd, alpha, beta, wrc, 12, label="weights")
    assert np.signbit(want[0]["alpha_sum"][0]) and want[0]["alpha_zero"][0] == 65 and want[1]["beta_zero"][5] == 65
    assert PR.fold(want)["weights_nonfinite"] == 4


@pytest.mark.parametrize("missing", ["alpha", "beta", "wrc", "all"])
def test_device_half_with_null_weight_planes(ctx, hipmod, missing):
    a, b, nbhd, alpha, beta, wrc = synthetic(20, 3, 8, 12, 79)
    alpha = None if missing in ("alpha", "all") else alpha
    beta = None if missing in ("beta", "all") else beta
    wrc = None if missing in ("wrc", "all") else wrc
    want = check_device(ctx, hipmod, a, b, nbhd, alpha, beta, wrc, 12, label="null " + missing)
    t = PR.fold(want)
    if alpha is None:
        assert not t["alpha_sum"].any() and not t["alpha_zero"].any()
    if wrc is None:
        assert t["wrc_sum"] == 0


# ---- 2. the flag end to end, one pass on each route ---------------------------------------------------------------------------------
def gp(hipmod, n):
    return hipmod.FLAG_GENERIC | (hipmod.FLAG_GENERIC_PACKED if n >= 4 else 0) | (hipmod.FLAG_GENERIC_WAVE if n >= 5 else 0)


def route_cases(hipmod):
    """name: route, (W, H, S), box, flags, options, layout, configuration"""
    wide = hipmod.FLAG_WIDE_NBHD
    cases = {
        "route0": (0, (12, 10, 8), 7, 0, dict(count_first=0), None, None),
        "route1": (1, (12, 10, 8), 7, 0, dict(count_first=1), None, None),
        "route2": (2, (10, 8, 16), 7, 0, {}, None, None),
        "route6": (6, (12, 10, 8), 7, wide, dict(wide=1), None, None),
        "route7": (7, (12, 10, 8), 7, wide | hipmod.FLAG_WIDE_CLASSES, dict(wide=1), None, None),
        "route8": (8, (12, 10, 8), 17, hipmod.SAMPLED_NBHD_FLAG, {}, None, "sampling"),
        "route9": (9, (12, 10, 8), 7, hipmod.MEMBER_TEST_FLAG, {}, None, "membership"),
    }
    for n in (3, 4, 5):
        cases["route%d" % n] = (n, (12, 10, 8), 7, gp(hipmod, n), {}, None, None)
        cases["route%d-3x7-f32" % n] = (n, (12, 10, 8), 7, gp(hipmod, n), {}, (3, 7, "f32"), None)
        cases["route%d-4x18-f16" % n] = (n, (12, 10, 8), 7, gp(hipmod, n), {}, (4, 18, "f16"), None)
    return cases


ROUTE_NAMES = ["route0", "route1", "route2", "route3", "route3-3x7-f32", "route3-4x18-f16", "route4", "route4-3x7-f32", "route4-4x18-f16",
               "route5", "route5-3x7-f32", "route5-4x18-f16", "route6", "route7", "route8", "route9"]


def debug_recs(c, hipmod, planes, desc_kw, box, colour_in=None, r0=0, r1=None, allow_nonfinite=False):
    """the restatement's row records from one rpf_filter_pass_debug call without the flag, and that call's colours"""
    _, Hd, Wd, Sd = planes.shape
    d = hipmod.make_desc(Wd, Hd, Sd, row_begin=r0, row_end=r1, **desc_kw)
    dbg = c.filter_pass_debug(planes, d, box=box, colour_in=colour_in, allow_nonfinite=allow_nonfinite)
    a = colours_of(planes) if colour_in is None else colour_in
    return PR.rows(a, dbg["colour"], dbg["nbhd_size"], dbg["alpha"], dbg["beta"], dbg["wrc"], r0, r1), dbg


@pytest.mark.parametrize("name", ROUTE_NAMES)
def test_flag_end_to_end_on_every_route(hipmod, name):
    route, (Wd, Hd, Sd), box, flags, options, lay, cfg = route_cases(hipmod)[name]
    kw, sigma = ACTIVE
    lay_kw = dict(n_random=lay[0], n_feat=lay[1], dtype=lay[2]) if lay else {}
    planes = frame(Wd, Hd, Sd, **kw, **lay_kw)
    desc_kw = dict(policy=EPS, sigma_seed=sigma, flags=flags)
    if lay:
        desc_kw.update(n_random=lay[0], n_feat=lay[1], plane_dtype=hipmod.PLANES_F16 if lay[2] == "f16" else hipmod.PLANES_F32)
    with hipmod.Context(0) as c:
        for k, v in options.items():
            c.set_option(k, v)
        if cfg == "sampling":
            c.set_sampling(hipmod.make_sampling(0x5EED5EED, [200]))
        if cfg == "membership":
            c.set_membership(hipmod.membership_preset(hipmod.MEMBERSHIP_PUBLISHED_19))
        on = hipmod.make_desc(Wd, Hd, Sd, boxes=(box,), **dict(desc_kw, flags=flags | hipmod.PASS_REPORT_FLAG))
        out = c.filter(planes, on, want_colour64=True)
        rep, rows, cn, r = c.pass_report(0), c.pass_report_rows(0), c.counters(), c.route()
        want, dbg = debug_recs(c, hipmod, planes, desc_kw, box)
    assert r == route == rep.route, (r, rep.route)
    assert same(out[3], dbg["colour"])
    assert (rep.box, rep.draws, rep.rows, rep.pixels, rep.samples) == (box, 200 if cfg == "sampling" else 0, Hd, Wd * Hd, Wd * Hd * Sd)
    assert_rows(rows, want, name)
    assert_report(rep, want, name)
    assert (rep.total.sum_nbhd, rep.total.max_nbhd) == (cn.sum_nbhd, cn.max_nbhd)
    t = PR.fold(want)
    print("PASS REPORT %s: unchanged %d of %d, rel-L2 moved %.3e, mean alpha %s, own-only %d, classes %s" % (
        name, t["unchanged_samples"], rep.samples, PR.moved_rel_l2(t), t["alpha_sum"] / rep.pixels, t["own_only_pixels"], t["class_pixels"].tolist()))
    assert t["moved2"].sum() > 0 and t["alpha_sum"].sum() > 0 and t["beta_sum"].sum() > 0 and t["wrc_sum"] > 0   # every plane was written


# ---- 3. composition and edge cases ----------------------------------------------------------------------------------------------------
def test_two_passes_then_a_call_without_the_flag(ctx, hipmod):
    kw, sigma = ACTIVE
    planes = frame(**kw)
    desc_kw = dict(policy=EPS, sigma_seed=sigma, flags=gp(hipmod, 5))
    on = hipmod.make_desc(12, 10, 8, boxes=(7, 5), **dict(desc_kw, flags=gp(hipmod, 5) | hipmod.PASS_REPORT_FLAG))
    off = hipmod.make_desc(12, 10, 8, boxes=(7, 5), **desc_kw)
    got = ctx.filter(planes, on, want_colour64=True)
    reps = [ctx.pass_report(i) for i in range(hipmod.MAX_BOXES)]
    cn_on = bytes(ctx.counters())[:32], ctx.counters().filter_kernel_launches, ctx.counters().redo_pixels, ctx.route()
    want0, dbg0 = debug_recs(ctx, hipmod, planes, desc_kw, 7)
    want1, dbg1 = debug_recs(ctx, hipmod, planes, desc_kw, 5, colour_in=dbg0["colour"])
    assert_report(reps[0], want0, "pass 0")
    assert_report(reps[1], want1, "pass 1")
    assert (reps[0].box, reps[1].box) == (7, 5) and same(got[3], dbg1["colour"])
    assert all(r.applied == 0 and bytes(r) == bytes(hipmod.PassReport()) for r in reps[2:])
    # the same call without the flag: the same colour bits, counters and launch counts, and every entry cleared
    plain = ctx.filter(planes, off, want_colour64=True)
    cn_off = bytes(ctx.counters())[:32], ctx.counters().filter_kernel_launches, ctx.counters().redo_pixels, ctx.route()
    assert same(plain[3], got[3]) and same(plain[0], got[0]) and same(plain[1], got[1]) and cn_on == cn_off
    assert all(bytes(ctx.pass_report(i)) == bytes(hipmod.PassReport()) for i in range(hipmod.MAX_BOXES))
    assert ctx.pass_report_rows(0) == []


def test_identity_and_scheduled_frames(ctx, hipmod):
    kw, sigma = IDENTITY
    planes = frame(**kw)
    on = hipmod.make_desc(12, 10, 8, boxes=(BOX,), policy=EPS, sigma_seed=sigma, flags=hipmod.PASS_REPORT_FLAG)
    ctx.filter(planes, on)
    rep = ctx.pass_report(0)
    want, dbg = debug_recs(ctx, hipmod, planes, dict(policy=EPS, sigma_seed=sigma), BOX)
    assert_report(rep, want, "identity")
    # The oracle is the identity on this frame bit for bit (test_pass_report_cpu.py); the device's weights differ from the oracle's
    # in their last bits (the suite's colour bar between the two is 1e-4 relative), so a few samples may move by that little.  The
    # report counts exactly the samples whose bits the device kept, and says that the pass did next to nothing
    kept = int((colours_of(planes).view(np.uint64) == dbg["colour"].view(np.uint64)).all(axis=0).sum())
    print("PASS REPORT identity: unchanged %d of %d, rel-L2 moved %.3e" % (rep.total.unchanged_samples, rep.samples, PR.moved_rel_l2(PR.of_ctypes(rep.total))))
    assert rep.samples == 960 and rep.total.unchanged_samples == kept >= 0.95 * rep.samples
    assert PR.moved_rel_l2(PR.of_ctypes(rep.total)) <= 1e-4
    # the scheduled frame: the report counts the clamped alphas
    planes = frame(**FLAT)
    ctx.set_schedule(hipmod.make_schedule(0.5, *SCHED_GAINS))
    desc_kw = dict(policy=EPS, sigma_seed=0.002, flags=gp(hipmod, 5) | hipmod.SCHEDULE_FLAG)
    ctx.filter(planes, hipmod.make_desc(12, 10, 8, boxes=(BOX,), **dict(desc_kw, flags=desc_kw["flags"] | hipmod.PASS_REPORT_FLAG)))
    rep = ctx.pass_report(0)
    want, _ = debug_recs(ctx, hipmod, planes, desc_kw, BOX)
    assert_report(rep, want, "scheduled")
    assert all(0 < z < rep.pixels for z in rep.total.alpha_zero) and 0 < rep.total.own_only_pixels < rep.pixels


def test_spike_clamp_leaves_the_report_alone(ctx, hipmod):
    planes = np.array(frame(**CLUSTERED))
    hit = np.random.default_rng(7).random(planes.shape[1:]) < 0.04
    planes[2:5, hit] *= np.float32(1e3)                                                # fireflies
    F = hipmod.PASS_REPORT_FLAG
    ctx.set_spike(1.0, True)
    a = ctx.filter(planes, hipmod.make_desc(12, 10, 8, policy=EPS, sigma_seed=0.5, flags=F), want_colour64=True)
    ra = ctx.pass_report(0)
    b = ctx.filter(planes, hipmod.make_desc(12, 10, 8, policy=EPS, sigma_seed=0.5, flags=F | hipmod.FLAG_SPIKE_CLAMP), want_colour64=True)
    rb, stats = ctx.pass_report(0), ctx.spike_stats()
    assert stats.applied == 1 and stats.spike_samples > 0 and not same(a[3], b[3])
    assert ra.applied == 1 and bytes(ra) == bytes(rb)                                  # the outputs are taken before the spike pass


def test_pass_debug_with_the_flag(ctx, hipmod):
    kw, sigma = ACTIVE
    planes = frame(**kw)
    for debug in (True, False):                                                        # the caller's planes | the context's scratch planes
        d = hipmod.make_desc(12, 10, 8, policy=EPS, sigma_seed=sigma, flags=gp(hipmod, 5) | hipmod.PASS_REPORT_FLAG)
        got = ctx.filter_pass_debug(planes, d, box=BOX, debug=debug)
        rep, rows = ctx.pass_report(0), ctx.pass_report_rows(0)
        if debug:
            want = PR.rows(colours_of(planes), got["colour"], got["nbhd_size"], got["alpha"], got["beta"], got["wrc"])
            colour = got["colour"]
        assert same(got["colour"], colour)
        assert_rows(rows, want, "pass_debug")
        assert_report(rep, want, "pass_debug")
        assert rep.route == 5 and ctx.pass_report(1).applied == 0


def test_film_and_device_entry_points(ctx, hipmod):
    import torch
    kw, sigma = ACTIVE
    planes = frame(**kw)
    desc_kw = dict(policy=EPS, sigma_seed=sigma, flags=0)
    on = hipmod.make_desc(12, 10, 8, boxes=(BOX,), **dict(desc_kw, flags=hipmod.PASS_REPORT_FLAG))
    film = hipmod.make_film(((0, 0), (12, 10)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX), sample_origin=(0, 0))
    ctx.filter_film(planes, on, film)
    r_film = ctx.pass_report(0)
    dev = torch.device("cuda", 0)
    dp = torch.from_numpy(np.ascontiguousarray(planes)).to(dev)
    dc = torch.empty((3, 10, 12, 8), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    ctx.colour_from_planes_device(on, dp.data_ptr(), dc.data_ptr(), stream)
    ctx.filter_device(on, dp.data_ptr(), dc.data_ptr(), stream)
    torch.cuda.synchronize()
    r_dev = ctx.pass_report(0)
    want, dbg = debug_recs(ctx, hipmod, planes, desc_kw, BOX)
    assert_report(r_film, want, "rpf_filter_film")
    assert_report(r_dev, want, "rpf_filter_device")
    assert same(dc.cpu().numpy(), dbg["colour"])


def test_sub_slab(ctx, hipmod):
    kw, sigma = ACTIVE
    planes = frame(**kw)
    desc_kw = dict(policy=EPS, sigma_seed=sigma, flags=gp(hipmod, 4))
    on = hipmod.make_desc(12, 10, 8, boxes=(BOX,), row_begin=3, row_end=7, **dict(desc_kw, flags=gp(hipmod, 4) | hipmod.PASS_REPORT_FLAG))
    ctx.filter(planes, on)
    rep, rows = ctx.pass_report(0), ctx.pass_report_rows(0)
    want, _ = debug_recs(ctx, hipmod, planes, desc_kw, BOX, r0=3, r1=7)
    assert (rep.rows, rep.pixels, rep.samples) == (4, 48, 384) and len(want) == 4
    assert_rows(rows, want, "sub-slab")
    assert_report(rep, want, "sub-slab")
    whole, _ = debug_recs(ctx, hipmod, planes, desc_kw, BOX)
    assert PR.differing(PR.fold(whole[3:7]), PR.fold(want)) == []                      # the rows of the whole frame's report


def test_report_is_filled_under_ref_abort(ctx, hipmod):
    Wd, Hd, Sd = 12, 8, 8
    planes = fb.synth_planes(Wd, Hd, Sd, seed=5)
    planes[7:10] = np.float32([0.0, 0.0, 1.0])[:, None, None, None]                     # flat surface: constant normal
    on = hipmod.make_desc(Wd, Hd, Sd, boxes=(BOX,), policy=REF_ABORT, flags=hipmod.PASS_REPORT_FLAG)
    out = ctx.filter(planes, on, allow_nonfinite=True, want_colour64=True)
    rep, cn = ctx.pass_report(0), ctx.counters()
    assert out[2] == hipmod.E_NONFINITE and rep.applied == 1
    assert rep.total.nonfinite_samples > 0 and rep.total.nonfinite_pixels == cn.nonfinite_pixels > 0
    want, dbg = debug_recs(ctx, hipmod, planes, dict(policy=REF_ABORT), BOX, allow_nonfinite=True)
    assert dbg["status"] == hipmod.E_NONFINITE
    assert_report(rep, want, "ref_abort")


# ---- 4. MultiContext --------------------------------------------------------------------------------------------------------------------
def _second_gpu():
    import torch
    return torch.cuda.device_count() > 1


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0), (0, 1)])
def test_multi_equals_one_context(ctx, hipmod, devices):
    if 1 in devices and not _second_gpu():
        pytest.skip("needs a second GPU")
    kw, sigma = ACTIVE
    planes = frame(12, 24, 8, **kw)
    desc = hipmod.make_desc(12, 24, 8, boxes=(7, 5), policy=EPS, sigma_seed=sigma, flags=gp(hipmod, 5) | hipmod.PASS_REPORT_FLAG)
    s1, p1, st1 = ctx.filter(planes, desc)
    one = [ctx.pass_report(i) for i in range(hipmod.MAX_BOXES)]
    with hipmod.MultiContext(list(devices)) as mc:
        s2, p2, st2 = mc.filter(planes, desc)
        multi = [mc.pass_report(i) for i in range(hipmod.MAX_BOXES)]
        plain = mc.filter(planes, hipmod.make_desc(12, 24, 8, boxes=(7, 5), policy=EPS, sigma_seed=sigma, flags=gp(hipmod, 5)))
        cleared = [mc.pass_report(i) for i in range(hipmod.MAX_BOXES)]
    assert st1 == st2 == hipmod.OK and same(s1, s2) and same(p1, p2) and same(plain[0], s1)
    assert one[0].applied == one[1].applied == 1 and one[0].total.moved2[0] > 0
    for i in range(hipmod.MAX_BOXES):
        assert bytes(multi[i]) == bytes(one[i]), i                                     # every field of every entry
        assert bytes(cleared[i]) == bytes(hipmod.PassReport()), i


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(hipmod):
    L = hipmod.load()
    with hipmod.Context(0) as c, hipmod.MultiContext([0, 0]) as mc:
        for i in range(hipmod.MAX_BOXES):                                              # before any call
            assert c.pass_report(i).applied == 0 and bytes(c.pass_report(i)) == bytes(hipmod.PassReport())
            assert mc.pass_report(i).applied == 0 and c.pass_report_rows(i) == []
        for bad in (-1, hipmod.MAX_BOXES):
            for call in (lambda: c.pass_report(bad), lambda: c.pass_report_rows(bad, 0), lambda: mc.pass_report(bad)):
                with pytest.raises(hipmod.RpfError) as e:
                    call()
                assert e.value.status == hipmod.E_BADARG
        assert L.rpf_query_pass_report(c._h, 0, None) == hipmod.E_BADARG
        assert L.rpf_query_pass_report_rows(c._h, 0, None, 0) == hipmod.E_BADARG
        assert L.rpf_multi_query_pass_report(mc._h, 0, None) == hipmod.E_BADARG
        planes = frame(**ACTIVE[0])
        c.filter(planes, hipmod.make_desc(12, 10, 8, policy=EPS, flags=hipmod.PASS_REPORT_FLAG))
        assert len(c.pass_report_rows(0)) == 10
        for n in (0, 9, 11):
            with pytest.raises(hipmod.RpfError) as e:
                c.pass_report_rows(0, n)
            assert e.value.status == hipmod.E_BADARG and "n_rows" in str(e.value)
        d = hipmod.make_desc(12, 10, 8)
        rows = (hipmod.ReportRow * 10)()
        assert L.rpf_pass_report_rows_device(c._h, C.byref(d), None, None, None, None, None, None, rows, None) == hipmod.E_BADARG
        assert L.rpf_pass_report_rows_device(None, C.byref(d), None, None, None, None, None, None, rows, None) == hipmod.E_BADARG
        m0, s0 = c.pixel_stats(planes, hipmod.make_desc(12, 10, 8, flags=hipmod.PASS_REPORT_FLAG))   # an entry point that runs no pass ignores it
        m1, s1 = c.pixel_stats(planes, d)
        assert same(m0, m1) and same(s0, s1)
