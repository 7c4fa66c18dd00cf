"""GPU tests of RPF_FLAG_SAMPLED_FUSED (rpf_query_route 11): a sampled pass on the compiled kernels, behind a
count kernel that leaves the draws of route 8 as acceptance masks.  Held, on every pixel of every frame, to the numpy restatement
tests/sampled_ref.py (member lists and statistics bit for bit, the weight planes at tests/test_sampled_gpu.py's bars, the colours at
the per-sample stage-4 bar of the expanded form, which is the form of the resident compiled kernels), to route 8 -- the same call
without the bit -- for member lists, statistics and bin ids, to tests/member_test_ref.py and tests/schedule_ref.py under the other
two steps of the published pipeline, and to chains of one-pass calls, slabs and the band pipeline.  EPS policy throughout (a
sampled pass under REF_ABORT is refused), sigma_seed 0.5 (the filter is active).

Before the feature the constant SAMPLED_FUSED_FLAG does not exist: every test here fails on the parent."""
import functools

import numpy as np
import pytest

import member_test_ref as MR
import sampled_ref as SR
import schedule_ref as SRf
import spike_ref
import stage4_bars as B
from raytracer_rpf_amd import feature_buffer as fb

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
SIGMA = 0.5
SEED = 0x5EED5EED
FRONT = ("nbhd_size", "member_hash", "mean", "stddev")
BITS = FRONT + ("bin_hash",)
STAGES = BITS + ("mi", "alpha", "beta", "wrc")
CAPS = (8, 16, 32, 64, 128, 256, 448, 832, 1600, 3136)   # the resident classes of route 2 / route 11
GAINS = (2.2, 1.1)

# name: W, H, S, box, D, generator, the classes the frame is here for, needs SAMPLED_REST, restatement with weights
CASES = {
    "class8": (6, 5, 4, 7, 3, "smooth", (8,), False, True),              # N <= S + D = 7: class 8 on every pixel by construction
    "packed32": (12, 10, 8, 7, 24, "smooth", (16, 32), False, True),     # interior windows unclipped
    "edge64": (12, 10, 8, 7, 56, "smooth", (64,), False, True),
    "wave128": (10, 8, 8, 17, 120, "smooth", (128,), False, True),       # 36-word stride
    "box55": (10, 8, 8, 55, 484, "smooth", (64,), False, True),          # 378-word stride, every window clipped: the published box-55 configuration
    "box35": (12, 10, 8, 35, 392, "iid", (128,), False, True),           # 153 words
    "big832": (14, 12, 32, 17, 800, "iid", (256, 448, 832), False, True),
    "rest1600": (14, 12, 32, 17, 2016, "iid", (832, 1600), True, True),
    "rest3136": (14, 12, 32, 17, 3001, "iid", (3136,), True, True),
    "cap": (14, 12, 32, 17, 3104, "iid", (3136,), True, True),          # S + D = 3136, the cap
    "dups": (6, 5, 4, 7, 200, "smooth", (64,), False, True),             # heavy duplicates
}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_or_nan(a, b):
    """bit for bit where neither is a NaN, and the same NaN pattern (a NaN's payload is not part of the contract)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def class_of(n):
    return next(c for c in CAPS if n <= c)


def classes_of(nbhd):
    return {class_of(int(n)) for n in np.asarray(nbhd).ravel()}


def stride_of(box, S):
    return max(1, ((box * box - 1) * S + 63) // 64)


@functools.lru_cache(maxsize=None)
def frame(W, H, S, mode="smooth", **kw):
    if mode == "iid":  # tests/test_sampled_gpu.py::planes_of: the features replaced by unit normals, the same law in every pixel
        p = fb.synth_planes(W, H, S, seed=11)
        p[7:] = np.random.default_rng(11).standard_normal(p[7:].shape).astype(np.float32)
    else:
        p = fb.synth_planes(W, H, S, seed=11, **kw)
    p.setflags(write=False)
    return p


def planes_of(name):
    W, H, S, _, _, mode, _, _, _ = CASES[name]
    return frame(W, H, S, mode)


_refs = {}


def ref_of(oracle, name):
    """the restatement of the case's pass: computed once, shared, never modified"""
    if name not in _refs:
        _, _, _, box, D, _, _, _, weights = CASES[name]
        _refs[name] = SR.sampled_pass(oracle, planes_of(name), (SEED, 0, D), 0, box, SIGMA, EPS, weights=weights)
    return _refs[name]


def flags_of(hipmod, fused=True, rest=False):
    return hipmod.SAMPLED_NBHD_FLAG | (hipmod.SAMPLED_FUSED_FLAG if fused else 0) | (hipmod.SAMPLED_REST_FLAG if rest else 0)


def run(c, hipmod, planes, box, D, fused=True, rest=False, extra=0, seed=SEED, pass_id0=0, mt=None, sched=None, lay=None, sigma_seed=SIGMA):
    """one pass through rpf_filter_pass_debug with D draws; mt / sched: under the membership test / the schedule as well"""
    _, H, W, S = planes.shape
    c.set_sampling(hipmod.make_sampling(seed, [D], pass_id0=pass_id0))
    if mt is not None:
        c.set_membership(hipmod.make_membership(mt[0].tolist(), mt[1].tolist()))
        extra |= hipmod.MEMBER_TEST_FLAG
    if sched is not None:
        c.set_schedule(sched)
        extra |= hipmod.SCHEDULE_FLAG
    desc = hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=sigma_seed, flags=flags_of(hipmod, fused, rest) | extra, **(lay or {}))
    got = c.filter_pass_debug(planes, desc, box=box)
    cn = c.counters()
    got.update(route=c.route(), launches=cn.filter_kernel_launches, redo_pixels=cn.redo_pixels, options_active=cn.options_active)
    return got


def assert_same_pass(a, b, keys=STAGES + ("colour",)):
    for k in keys:
        assert same_bits(a[k], b[k]), k
    assert (a["route"], a["sum_nbhd"], a["max_nbhd"], a["launches"], a["redo_pixels"]) == (b["route"], b["sum_nbhd"], b["max_nbhd"], b["launches"], b["redo_pixels"])


def check_stage4(planes, got, ref, box, label):
    """every sample within the per-sample bar of the expanded form (every pixel of route 11 runs a resident compiled kernel)"""
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(ref))
    cmax = B.cmax_of(planes[2:5])
    n = got["nbhd_size"]
    assert n.max() <= B.RESIDENT
    bar = B.sample_bar("expanded", 12, int(n.max()), SIGMA, box)
    worst = B.worst_sample(got["colour"], ref) / cmax
    print("SAMPLED_FUSED %s stage 4: worst %.3e (bar %.3e)" % (label, worst, bar))
    assert worst <= bar, (worst, bar)


class options:
    """options set on a shared context, put back on exit"""
    DEFAULTS = dict(wide=-1, sampled_fused_stride=-1, binning=-1)

    def __init__(self, c, **kw):
        self.c, self.kw = c, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.c.set_option(k, v)

    def __exit__(self, *a):
        for k in self.kw:
            self.c.set_option(k, self.DEFAULTS[k])


# ---- 1. stage parity on every pixel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_stage_parity_on_every_pixel(ctx, hipmod, oracle, name):
    W, H, S, box, D, _, reach, rest, weights = CASES[name]
    planes = planes_of(name)
    want = ref_of(oracle, name)
    classes = classes_of(want["nbhd_size"])
    print("SAMPLED_FUSED %s: N %d .. %d, classes %s, stride %d" % (name, want["nbhd_size"].min(), want["nbhd_size"].max(), sorted(classes), stride_of(box, S)))
    assert set(reach) <= classes, (reach, sorted(classes))              # the frame reaches the kernels it is here for
    if name == "class8":
        assert classes == {8}
    if name == "box55":
        assert stride_of(box, S) == 378 and W < box and H < box         # every window clipped by the frame
    if name == "cap":
        assert S + D == 3136
    if name == "dups":   # more draws than the frame has candidates: most repeat an earlier one, on every pixel
        assert all(len(SR.draws(SEED, 0, 0, D, box, W, H, S, x, y)) <= (W * H - 1) * S < D for y in range(H) for x in range(W))
    got = run(ctx, hipmod, planes, box, D, rest=rest)
    assert got["status"] == hipmod.OK and got["route"] == 11 and got["redo_pixels"] == 0
    assert got["launches"] == len(classes)                              # one launch per non-empty class; the count kernel is not counted
    for k in ("nbhd_size", "member_hash", "mean", "stddev"):
        assert np.array_equal(got[k], want[k]), k
    assert got["max_nbhd"] == want["nbhd_size"].max() and got["sum_nbhd"] == int(want["nbhd_size"].sum())
    assert np.array_equal(ctx.nbhd(W, H), want["nbhd_size"])
    # route 8: the same call without the bit
    r8 = run(ctx, hipmod, planes, box, D, fused=False, rest=rest)
    assert r8["route"] == 8
    for k in BITS:
        assert same_bits(got[k], r8[k]), k
    assert (got["sum_nbhd"], got["max_nbhd"]) == (r8["sum_nbhd"], r8["max_nbhd"])
    # the weight planes at tests/test_sampled_gpu.py's bars: against the restatement, or -- where that runs without weights -- route 8
    base = want if weights else r8
    np.testing.assert_allclose(got["mi"], base["mi"], rtol=0, atol=1e-11)
    for k in ("alpha", "beta", "wrc"):
        np.testing.assert_allclose(got[k], base[k], rtol=1e-9, atol=1e-12)
    # stage 4: the restatement on the device's own stage outputs, every sample, the expanded form's bar
    ref = SR.stage4_on(oracle, planes, got, (SEED, 0, D), 0, box, SIGMA, EPS)
    check_stage4(planes, got, ref, box, name)
    cmax = B.cmax_of(planes[2:5])
    assert np.abs(got["colour"] - (want["colour"] if weights else r8["colour"])).max() <= 1e-4 * cmax   # and the whole pass, loosely


# ---- 2. staying put: the bits, route and counters of the same call without the bit -----------------------------------------------
def stays(c, hipmod, planes, box, D, route, **kw):
    a = run(c, hipmod, planes, box, D, fused=False, **kw)
    b = run(c, hipmod, planes, box, D, fused=True, **kw)
    assert a["route"] == route, a["route"]
    assert_same_pass(b, a)
    return b


def test_stays_put_with_zero_draws(ctx, hipmod):
    planes = planes_of("packed32")
    with options(ctx, binning=1):
        got = stays(ctx, hipmod, planes, 7, 0, 2)
    assert got["nbhd_size"].max() > 8 + 24


def test_stays_put_above_the_resident_cap(ctx, hipmod):
    W, H, S, box, D = 6, 5, 32, 17, 3105
    assert S + D == 3137
    stays(ctx, hipmod, frame(W, H, S, "iid"), box, D, 8, rest=True)
    got = run(ctx, hipmod, frame(W, H, S, "iid"), box, D - 1, rest=True)      # ... and one draw fewer is taken
    assert got["route"] == 11


def test_stays_put_under_flag_generic(ctx, hipmod):
    gpw = hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED | hipmod.FLAG_GENERIC_WAVE
    for extra in (hipmod.FLAG_GENERIC, gpw):
        stays(ctx, hipmod, planes_of("packed32"), 7, 24, 8, extra=extra)


def test_stays_put_on_a_generic_layout(ctx, hipmod):
    W, H, S, box, D, nr, nf = 12, 10, 8, 7, 24, 3, 7
    stored = fb.synth_planes(W, H, S, seed=5, n_random=nr, n_feat=nf, dtype="f16")
    lay = dict(n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16)
    stays(ctx, hipmod, stored, box, D, 8, extra=hipmod.FLAG_GENERIC, lay=lay)


def test_stays_put_under_option_wide(hipmod):
    with hipmod.Context(0) as c:
        c.set_option("wide", 1)
        stays(c, hipmod, planes_of("packed32"), 7, 24, 8, extra=hipmod.FLAG_WIDE_NBHD)
        c.set_option("wide", -1)
        assert run(c, hipmod, planes_of("packed32"), 7, 24, extra=hipmod.FLAG_WIDE_NBHD)["route"] == 11


def test_stays_put_above_option_sampled_fused_stride(hipmod):
    planes, box, D = planes_of("wave128"), 17, 120
    assert stride_of(box, 8) == 36
    with hipmod.Context(0) as c:
        c.set_option("sampled_fused_stride", 35)
        got = stays(c, hipmod, planes, box, D, 8)
        assert got["options_active"] == 1
        c.set_option("sampled_fused_stride", 36)                            # the bound is inclusive
        assert run(c, hipmod, planes, box, D)["route"] == 11
        c.set_option("sampled_fused_stride", -1)
        got = run(c, hipmod, planes, box, D)
        assert got["route"] == 11 and got["options_active"] == 0
        with pytest.raises(hipmod.RpfError):
            c.set_option("sampled_fused_stride", 1025)


# ---- 3. the d27 compiled layout ----------------------------------------------------------------------------------------------------
def test_compiled_27_dim_layout_takes_route_11(ctx, hipmod, oracle):
    W, H, S, box, D, nr, nf = 12, 10, 8, 7, 24, 4, 18
    stored = fb.synth_planes(W, H, S, seed=5, n_random=nr, n_feat=nf, dtype="f16")
    lay = dict(n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16)
    r8 = run(ctx, hipmod, stored, box, D, fused=False, lay=lay)
    got = run(ctx, hipmod, stored, box, D, lay=lay)
    assert (r8["route"], got["route"]) == (8, 11) and got["status"] == hipmod.OK
    assert got["nbhd_size"].max() > S
    for k in FRONT:
        assert same_bits(got[k], r8[k]), k
    want = SR.sampled_pass(oracle, stored.astype(np.float32), (SEED, 0, D), 0, box, SIGMA, EPS, n_random=nr, n_feat=nf, weights=False)
    for k in FRONT:
        assert np.array_equal(got[k], want[k]), k
    assert got["launches"] == len(classes_of(want["nbhd_size"]))


# ---- 4. under the membership test ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,S,box,D", [(12, 10, 8, 7, 56), (10, 8, 8, 17, 120)], ids=["box7-D56", "box17-D120"])
def test_draws_meet_the_configured_test(ctx, hipmod, oracle, W, H, S, box, D):
    """tests/test_member_test_gpu.py's two sampled frames on route 11"""
    planes, mt = frame(W, H, S, flat_frac=0.94), MR.published19()
    want = MR.member_pass(oracle, planes, mt, box, SIGMA, EPS, cfg=(SEED, 0, D))
    got = run(ctx, hipmod, planes, box, D, mt=mt)
    assert got["route"] == 11 and got["status"] == hipmod.OK and got["redo_pixels"] == 0
    assert got["launches"] == len(classes_of(want["nbhd_size"]))
    assert want["nbhd_size"].max() > S
    for k in FRONT:
        assert np.array_equal(got[k], want[k]), k
    np.testing.assert_allclose(got["mi"], want["mi"], rtol=0, atol=1e-11)
    for k in ("alpha", "beta", "wrc"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12)
    check_stage4(planes, got, MR.stage4_on(oracle, planes, got, mt, box, SIGMA, EPS, cfg=(SEED, 0, D)), box, "member box %d" % box)
    r8 = run(ctx, hipmod, planes, box, D, fused=False, mt=mt)
    assert r8["route"] == 8
    for k in BITS:
        assert same_bits(got[k], r8[k]), k
    # ... and it is another list than the 3-sigma test's (the flat pixels accept nothing there)
    plain = run(ctx, hipmod, planes, box, D)
    assert plain["route"] == 11 and (plain["nbhd_size"] < got["nbhd_size"]).any()


def test_reference_multiples_and_floors_equal_the_run_without_the_test(ctx, hipmod):
    planes = planes_of("edge64")
    plain = run(ctx, hipmod, planes, 7, 56)
    got = run(ctx, hipmod, planes, 7, 56, mt=MR.reference())
    assert plain["route"] == got["route"] == 11
    assert_same_pass(got, plain)


# ---- 5. under the schedule ------------------------------------------------------------------------------------------------------------
def test_scheduled_gains_need_the_permission(ctx, hipmod, oracle):
    planes, box, D = planes_of("edge64"), 7, 56
    sched = hipmod.make_schedule(SIGMA, *GAINS)
    # without RPF_FLAG_SCHEDULE_FUSED the pass stays on route 8, as without the bit
    stays(ctx, hipmod, planes, box, D, 8, sched=sched, sigma_seed=0.002)
    # with it: route 11 on the scheduled builds
    base = run(ctx, hipmod, planes, box, D, sched=hipmod.make_schedule(SIGMA, 1.0, 1.0), extra=hipmod.SCHEDULE_FUSED_FLAG, sigma_seed=0.002)
    got = run(ctx, hipmod, planes, box, D, sched=sched, extra=hipmod.SCHEDULE_FUSED_FLAG, sigma_seed=0.002)
    assert base["route"] == got["route"] == 11 and got["status"] == hipmod.OK
    for k in BITS + ("mi", "wrc"):                                       # everything in front of stage 3c: the gains-(1, 1) run's bits
        assert same_bits(got[k], base[k]), k
    assert (got["launches"], got["sum_nbhd"], got["max_nbhd"]) == (base["launches"], base["sum_nbhd"], base["max_nbhd"])
    assert_same_pass(base, run(ctx, hipmod, planes, box, D))            # gains (1, 1) with the entry's seed: the unscheduled pass
    want = SRf.scheduled_pass(oracle, planes, (SIGMA,) + GAINS, box, cfg=(SEED, 0, D))
    for k in ("nbhd_size", "mean", "stddev"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("alpha", "beta"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12)
    a, b, w = SRf.alpha_beta(got["mi"], GAINS[0], GAINS[1], 0, 1e-10)    # stage 3c on the device's own MI: bit for bit
    assert same_or_nan(got["alpha"], a) and same_or_nan(got["beta"], b) and same_or_nan(got["wrc"], w)
    assert not same_bits(got["alpha"], base["alpha"]) and not same_bits(got["beta"], base["beta"])
    check_stage4(planes, got, SRf.stage4_on(oracle, planes, got, SIGMA, box, EPS, cfg=(SEED, 0, D)), box, "scheduled")


# ---- 6. the published call -----------------------------------------------------------------------------------------------------------
def call(c, hipmod, planes, boxes, flags, draws, pass0=0, colour64_in=None, seed=SEED):
    """one call through rpf_filter_ex, its passes with ids pass0 .. (a schedule's entries stand for the descriptor's seed)"""
    _, H, W, S = planes.shape
    c.set_sampling(hipmod.make_sampling(seed, draws, pass_id0=pass0))
    desc = hipmod.make_desc(W, H, S, boxes=boxes, policy=EPS, sigma_seed=SIGMA, flags=flags)
    out = c.filter(planes, desc, colour64_in=colour64_in, want_colour64=True)
    assert out[2] == hipmod.OK
    return out[3], c.route(), c.counters()


def test_the_published_call(ctx, hipmod):
    planes = frame(14, 12, 8, flat_frac=0.5)
    boxes, draws = (17, 7), (120, 24)
    seeds, gc, gf = [SIGMA, SIGMA / 2], [2.2, 1.3], [1.1, 1.15]
    mt = MR.published19()
    six = (hipmod.SAMPLED_NBHD_FLAG | hipmod.SAMPLED_FUSED_FLAG | hipmod.MEMBER_TEST_FLAG | hipmod.MEMBER_FUSED_FLAG |
           hipmod.SCHEDULE_FLAG | hipmod.SCHEDULE_FUSED_FLAG)
    old = hipmod.SAMPLED_NBHD_FLAG | hipmod.MEMBER_TEST_FLAG | hipmod.SCHEDULE_FLAG
    ctx.set_membership(hipmod.make_membership(mt[0].tolist(), mt[1].tolist()))
    ctx.set_spike(1.0, True)
    ctx.set_schedule(hipmod.make_schedule(seeds, gc, gf))
    whole, route, cn = call(ctx, hipmod, planes, boxes, six | hipmod.FLAG_SPIKE_CLAMP, draws)
    assert route == 11 and ctx.spike_stats().applied == 1
    reported, _, _ = call(ctx, hipmod, planes, boxes, six | hipmod.FLAG_SPIKE_CLAMP | hipmod.PASS_REPORT_FLAG, draws)
    assert [ctx.pass_report(p).route for p in range(2)] == [11, 11] and same_bits(reported, whole)
    assert cn.filter_kernel_launches >= 1 and cn.redo_pixels == 0
    # the chain of one-pass calls, the spike pass behind the last
    colour = None
    for p, box in enumerate(boxes):
        ctx.set_schedule(hipmod.make_schedule(seeds, gc, gf, pass0=p))
        colour, r, cn1 = call(ctx, hipmod, planes, (box,), six | (hipmod.FLAG_SPIKE_CLAMP if p == 1 else 0), [draws[p]], pass0=p, colour64_in=colour)
        assert r == 11
    assert same_bits(whole, colour)
    assert (cn.sum_nbhd, cn.max_nbhd, cn.redo_pixels) == (cn1.sum_nbhd, cn1.max_nbhd, 0)           # of the last pass
    # the same call on routes 8 / 9: the colour bar
    ctx.set_schedule(hipmod.make_schedule(seeds, gc, gf))
    slow, route, cn8 = call(ctx, hipmod, planes, boxes, old | hipmod.FLAG_SPIKE_CLAMP | hipmod.PASS_REPORT_FLAG, draws)
    assert [ctx.pass_report(p).route for p in range(2)] == [8, 8]
    assert (cn8.sum_nbhd, cn8.max_nbhd) == (cn.sum_nbhd, cn.max_nbhd)
    assert np.abs(whole - slow).max() <= 1e-4 * B.cmax_of(planes[2:5])
    # draws (120, 0): the second pass is a full-box pass under the membership test on the compiled kernels
    call(ctx, hipmod, planes, boxes, six | hipmod.FLAG_SPIKE_CLAMP | hipmod.PASS_REPORT_FLAG, (120, 0))
    assert [ctx.pass_report(p).route for p in range(2)] == [11, 10]


# ---- 7. slabs and determinism ---------------------------------------------------------------------------------------------------------
def need_devices(devices):
    import torch
    if max(devices) >= torch.cuda.device_count():
        pytest.skip("needs %d visible GPUs" % (max(devices) + 1))


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0), (0, 1), (0, 1, 0)])
def test_multi_filter_equals_one_context(ctx, hipmod, devices):
    need_devices(devices)
    planes, cfg = frame(12, 12, 8), hipmod.make_sampling(SEED, [24, 40], pass_id0=3)
    desc = hipmod.make_desc(12, 12, 8, boxes=(7, 7), policy=EPS, sigma_seed=SIGMA, flags=flags_of(hipmod))
    ctx.set_sampling(cfg)
    s1, p1, st1 = ctx.filter(planes, desc)
    c1 = ctx.counters()
    assert ctx.route() == 11 and c1.max_nbhd > 8
    with hipmod.MultiContext(list(devices)) as mc:
        mc.set_sampling(cfg)
        s2, p2, st2 = mc.filter(planes, desc)
        c2 = mc.counters()
        s3, _, _ = mc.filter(planes, desc)                                           # row_origin does not drift between calls
    assert st1 == st2 == hipmod.OK
    assert np.array_equal(s1.view(np.uint32), s2.view(np.uint32)) and np.array_equal(p1.view(np.uint32), p2.view(np.uint32))
    assert np.array_equal(s2.view(np.uint32), s3.view(np.uint32))
    assert (c2.samples_filtered, c2.sum_nbhd, c2.max_nbhd, c2.redo_pixels) == (c1.samples_filtered, c1.sum_nbhd, c1.max_nbhd, 0)


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0), (0, 1), (0, 1, 0)])
def test_multi_filter_film_equals_one_context(ctx, hipmod, devices):
    need_devices(devices)
    planes, cfg = np.array(frame(12, 12, 8)), hipmod.make_sampling(SEED, [24])
    _, H, W, S = planes.shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    planes[0] = (xx[..., None] + (np.arange(S) + 0.5) / S).astype(np.float32)        # pFilm inside its pixel
    planes[1] = (yy[..., None] + 0.5).astype(np.float32)
    film = hipmod.make_film(((0, 0), (W, H)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX), sample_origin=(0, 0))
    desc = hipmod.make_desc(W, H, S, boxes=(7,), policy=EPS, sigma_seed=SIGMA, flags=flags_of(hipmod))
    ctx.set_sampling(cfg)
    one = ctx.filter_film(planes, desc, film)
    assert ctx.route() == 11
    with hipmod.MultiContext(list(devices)) as mc:
        mc.set_sampling(cfg)
        two = mc.filter_film(planes, desc, film)
    for a, b in zip(one, two):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_banded_call_gives_the_serial_call_s_bits(ctx, hipmod):
    """48 rows are three bands of rpf_filter's row-band pipeline: each band its own count pass, the keys by image row"""
    W, H, S = 6, 48, 8
    planes = frame(W, H, S)
    ctx.set_sampling(hipmod.make_sampling(SEED, [24, 40, 24]))
    for boxes in ((7,), (7, 5, 7)):
        desc = hipmod.make_desc(W, H, S, boxes=boxes, policy=EPS, sigma_seed=SIGMA, flags=flags_of(hipmod))
        s_serial, p_serial, st, c64 = ctx.filter(planes, desc, want_colour64=True)     # rpf_filter_ex
        assert st == hipmod.OK and ctx.route() == 11
        pin = ctx.host_empty(planes.shape, planes.dtype)
        pin[...] = planes
        out_s, out_p = ctx.host_empty(s_serial.shape), ctx.host_empty(p_serial.shape)
        ctx.filter(pin, desc, out_samples=out_s, out_pixels=out_p)                  # rpf_filter from page-locked buffers
        assert ctx.route() == 11
        assert np.array_equal(out_s, s_serial) and np.array_equal(out_p, p_serial)
        assert np.array_equal(s_serial, c64.astype(np.float32))


def test_determinism_seed_and_pass_id(ctx, hipmod, oracle):
    planes, box, D = planes_of("edge64"), 7, 56
    a, b = run(ctx, hipmod, planes, box, D), run(ctx, hipmod, planes, box, D)
    for k in STAGES + ("colour",):
        assert same_bits(a[k], b[k]), k
    other_seed, other_pass = run(ctx, hipmod, planes, box, D, seed=SEED + 1), run(ctx, hipmod, planes, box, D, pass_id0=1)
    assert other_seed["route"] == other_pass["route"] == 11
    assert (other_seed["member_hash"] != a["member_hash"]).any() and (other_pass["member_hash"] != a["member_hash"]).any()
    for got, kw in ((other_seed, dict(seed=SEED + 1)), (other_pass, dict(pass_id0=1))):
        r8 = run(ctx, hipmod, planes, box, D, fused=False, **kw)
        assert same_bits(got["member_hash"], r8["member_hash"]) and same_bits(got["nbhd_size"], r8["nbhd_size"])


def test_entry_points_agree_with_the_debug_pass(ctx, hipmod):
    import torch
    planes, box, D = planes_of("edge64"), 7, 56
    _, H, W, S = planes.shape
    dbg = run(ctx, hipmod, planes, box, D)
    assert dbg["route"] == 11
    desc = hipmod.make_desc(W, H, S, boxes=(box,), policy=EPS, sigma_seed=SIGMA, flags=flags_of(hipmod))
    want32 = dbg["colour"].astype(np.float32)
    srgb, _, st, c64 = ctx.filter(planes, desc, want_colour64=True)                  # rpf_filter_ex
    assert st == hipmod.OK and ctx.route() == 11 and same_bits(c64, dbg["colour"]) and np.array_equal(srgb, want32)
    dev = torch.device("cuda", 0)                                                    # rpf_filter_device
    dp = torch.from_numpy(np.array(planes)).to(dev)
    col = dp[2:5].to(torch.float64).contiguous()
    ctx.filter_device(desc, dp.data_ptr(), col.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ctx.route() == 11 and same_bits(col.cpu().numpy(), dbg["colour"])


def test_refusals_on_the_device_entry_points(hipmod):
    planes = planes_of("packed32")
    _, H, W, S = planes.shape
    N, X = hipmod.SAMPLED_NBHD_FLAG, hipmod.SAMPLED_FUSED_FLAG
    film = hipmod.make_film(((0, 0), (W, H)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX), sample_origin=(0, 0))

    def desc(flags, policy=EPS):
        return hipmod.make_desc(W, H, S, boxes=(7,), policy=policy, flags=flags)
    with hipmod.Context(0) as c, hipmod.MultiContext([0, 0]) as mc:
        calls = {
            "rpf_filter": lambda d: c.filter(planes, d),
            "rpf_filter_ex": lambda d: c.filter(planes, d, want_colour64=True),
            "rpf_filter_device": lambda d: c.filter_device(d, None, None),
            "rpf_filter_pass_debug": lambda d: c.filter_pass_debug(planes, d, box=7),
            "rpf_filter_film": lambda d: c.filter_film(planes, d, film),
            "rpf_multi_filter": lambda d: mc.filter(planes, d),
            "rpf_multi_filter_film": lambda d: mc.filter_film(planes, d, film),
        }

        def refused(d, status, word):
            for name, fn in calls.items():
                with pytest.raises(hipmod.RpfError) as e:
                    fn(d)
                assert e.value.status == status and word in str(e.value), (name, str(e.value))
        refused(desc(N | X), hipmod.E_BADARG, "rpf_set_sampling")                    # no configuration set
        for m in (c, mc):
            m.set_sampling(hipmod.make_sampling(1, [24]))
        refused(desc(X), hipmod.E_UNSUPPORTED, "SAMPLED_FUSED")                      # the bit without RPF_FLAG_SAMPLED_NBHD
        refused(desc(X | hipmod.FLAG_WIDE_NBHD), hipmod.E_UNSUPPORTED, "SAMPLED_FUSED")
        assert hipmod.layout_kernels(desc(X)) == (hipmod.E_UNSUPPORTED, None)
        # with it, the parent's refusals stand
        refused(desc(N | X, REF_ABORT), hipmod.E_UNSUPPORTED, "REF_ABORT")
        refused(desc(N | X | hipmod.FLAG_FAST_WEIGHTS), hipmod.E_UNSUPPORTED, "FAST_WEIGHTS")
        refused(desc(N | X | hipmod.FLAG_GENERIC | hipmod.FLAG_STREAM_FAST), hipmod.E_UNSUPPORTED, "STREAM_FAST")
        for m in (c, mc):
            m.set_sampling(hipmod.make_sampling(1, [832 - S + 1]))
        refused(desc(N | X), hipmod.E_BADARG, "832")                                 # S + D = 833 still needs RPF_FLAG_SAMPLED_REST
        # ... and accepted again
        c.set_sampling(hipmod.make_sampling(1, [832 - S]))
        assert c.filter_pass_debug(planes, desc(N | X), box=7)["status"] == hipmod.OK and c.route() == 11


# ---- 8. the membership cache of the size-binned route --------------------------------------------------------------------------------
def test_cache_is_neither_served_nor_poisoned(hipmod):
    """a route-2 pass, a route-11 pass and the route-2 pass again at the same box, in one call: the third pass must count again"""
    planes = frame(12, 10, 8)
    with hipmod.Context(0) as c:
        c.set_option("binning", 1)
        three, route, _ = call(c, hipmod, planes, (7, 7, 7), flags_of(hipmod) | hipmod.PASS_REPORT_FLAG, (0, 24, 0))
        assert [c.pass_report(p).route for p in range(3)] == [2, 11, 2]
        colour = None
        for p, d in enumerate((0, 24, 0)):
            colour, r, _ = call(c, hipmod, planes, (7,), flags_of(hipmod), [d], pass0=p, colour64_in=colour)
            assert r == (11 if d else 2)
        assert same_bits(three, colour)
        # and against a call that never ran route 11: two route-2 passes around a route-8 pass
        old, _, _ = call(c, hipmod, planes, (7, 7, 7), flags_of(hipmod, fused=False) | hipmod.PASS_REPORT_FLAG, (0, 24, 0))
        assert [c.pass_report(p).route for p in range(3)] == [2, 8, 2]
        assert np.abs(three - old).max() <= 1e-4 * B.cmax_of(planes[2:5])


# ---- on top -----------------------------------------------------------------------------------------------------------------------
def test_spike_pass_on_top(ctx, hipmod):
    planes = np.array(planes_of("packed32"))
    hit = np.random.default_rng(7).random(planes.shape[1:]) < 0.04
    planes[2:5, hit] *= np.float32(1e3)                                              # fireflies
    _, H, W, S = planes.shape
    ctx.set_sampling(hipmod.make_sampling(SEED, [24]))

    def c64(flags):
        out = ctx.filter(planes, hipmod.make_desc(W, H, S, boxes=(7,), policy=EPS, sigma_seed=SIGMA, flags=flags), want_colour64=True)
        assert out[2] == hipmod.OK
        return out[3], ctx.route()
    plain, route = c64(flags_of(hipmod))
    ctx.set_spike(1.0, True)
    spiked, route2 = c64(flags_of(hipmod) | hipmod.FLAG_SPIKE_CLAMP)
    st = ctx.spike_stats()
    want = spike_ref.apply(plain, 1.0, True)
    assert route == route2 == 11 and st.applied == 1 and st.spike_samples == want["spike_samples"] > 0
    assert same_bits(spiked, want["colour"])


def test_pass_report_n_fields_equal_route_8(ctx, hipmod):
    planes = planes_of("wave128")
    reps = {}
    for fused in (False, True):
        call(ctx, hipmod, planes, (17,), flags_of(hipmod, fused) | hipmod.PASS_REPORT_FLAG, [120])
        reps[fused] = ctx.pass_report(0)
    a, b = reps[False], reps[True]
    assert (a.applied, b.applied, a.route, b.route) == (1, 1, 8, 11)
    assert (b.box, b.rows, b.pixels, b.samples, b.draws) == (a.box, a.rows, a.pixels, a.samples, a.draws)
    for k in ("sum_nbhd", "min_nbhd", "max_nbhd", "own_only_pixels"):
        assert getattr(b.total, k) == getattr(a.total, k), k
    assert list(b.total.class_pixels) == list(a.total.class_pixels) and sum(b.total.class_pixels) == b.pixels
