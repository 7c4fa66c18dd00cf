"""GPU tests of RPF_FLAG_SAMPLED_LISTED (rpf_query_route 12): a sampled pass on the listed builds of the
compiled kernels, which copy their member lists from route 8's member pool.  Held, on every pixel of every frame, to the numpy
restatement tests/sampled_ref.py (member lists and statistics bit for bit, the weight planes at tests/test_sampled_gpu.py's bars,
the colours at the per-sample stage-4 bar of the expanded form), to route 8 -- the same call without the bit -- for member lists,
statistics and bin ids, to route 11 -- RPF_FLAG_SAMPLED_FUSED instead -- bit for bit in every stage output and the colours (the
same code behind the same list), to tests/member_test_ref.py and tests/schedule_ref.py under the other two steps of the published
pipeline, and to chains of one-pass calls, slabs and the band pipeline.  Wide windows (box*box*S > 65535), which route 11 cannot
take, are among the frames.  EPS policy throughout, sigma_seed 0.5 (the filter is active).

Before the feature the constant SAMPLED_LISTED_FLAG does not exist: every test here fails on the parent."""
import functools

import numpy as np
import pytest

import member_test_ref as MR
import pass_report_ref as PR
import sampled_ref as SR
import schedule_ref as SRf
import stage4_bars as B
from raytracer_rpf_amd import feature_buffer as fb

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
SIGMA = 0.5
SEED = 0x5EED5EED
FRONT = ("nbhd_size", "member_hash", "mean", "stddev")
BITS = FRONT + ("bin_hash",)
STAGES = BITS + ("mi", "alpha", "beta", "wrc")
CAPS = (8, 16, 32, 64, 128, 256, 448, 832, 1600, 3136)   # the resident classes of routes 2, 11 and 12
GAINS = (2.2, 1.1)

# name: W, H, S, box, D, generator, the classes the frame is here for, needs SAMPLED_REST, wide by formula (needs WIDE_NBHD)
CASES = {
    "class8": (6, 5, 4, 7, 3, "smooth", (8,), False, False),             # N <= S + D = 7: class 8 on every pixel by construction
    "packed32": (12, 10, 8, 7, 24, "smooth", (16, 32), False, False),    # the listed packed kernels
    "edge64": (12, 10, 8, 7, 56, "smooth", (64,), False, False),
    "dups": (6, 5, 4, 7, 200, "smooth", (64,), False, False),            # heavy duplicates
    "wave128": (10, 8, 8, 17, 120, "smooth", (128,), False, False),      # one-wave listed
    "box55": (10, 8, 8, 55, 484, "smooth", (64,), False, False),         # every window clipped, the bitmap count kernel at 378 words
    "big832": (14, 12, 32, 17, 800, "iid", (256, 448, 832), False, False),
    "rest1600": (14, 12, 32, 17, 2016, "iid", (832, 1600), True, False),  # split-route PHASES 2 / 3 / 4, four-wave at a window above 4096 candidates
    "cap": (14, 12, 32, 17, 3104, "iid", (1600, 3136), True, False),     # S + D = 3136, the cap
    "wide22": (10, 8, 22, 55, 484, "smooth", (64,), False, True),        # wide by formula (66550): route 8's enumeration count kernel in front
    "wide32": (10, 8, 32, 55, 1904, "iid", (128, 256), True, True),      # wide (96800), the block count kernel; the paper's box-55 draws at 32 spp
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
        _, _, _, box, D, _, _, _, _ = CASES[name]
        _refs[name] = SR.sampled_pass(oracle, planes_of(name), (SEED, 0, D), 0, box, SIGMA, EPS, weights=True)
    return _refs[name]


def flags_of(hipmod, mode="listed", rest=False, wide=False):
    """mode: "plain" route 8, "fused" SAMPLED_FUSED_FLAG, "listed" SAMPLED_LISTED_FLAG, "both" """
    return (hipmod.SAMPLED_NBHD_FLAG | (hipmod.SAMPLED_FUSED_FLAG if mode in ("fused", "both") else 0) |
            (hipmod.SAMPLED_LISTED_FLAG if mode in ("listed", "both") else 0) | (hipmod.SAMPLED_REST_FLAG if rest else 0) |
            (hipmod.FLAG_WIDE_NBHD if wide else 0))


def run(c, hipmod, planes, box, D, mode="listed", rest=False, wide=False, extra=0, seed=SEED, pass_id0=0, mt=None, sched=None, lay=None,
        sigma_seed=SIGMA):
    """one pass through rpf_filter_pass_debug with D draws; mt / sched: under the membership test / the schedule as well"""
    _, H, W, S = planes.shape
    c.set_sampling(hipmod.make_sampling(seed, [D], pass_id0=pass_id0))
    if mt is not None:
        c.set_membership(hipmod.make_membership(mt[0].tolist(), mt[1].tolist()))
        extra |= hipmod.MEMBER_TEST_FLAG
    if sched is not None:
        c.set_schedule(sched)
        extra |= hipmod.SCHEDULE_FLAG
    desc = hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=sigma_seed, flags=flags_of(hipmod, mode, rest, wide) | extra, **(lay or {}))
    got = c.filter_pass_debug(planes, desc, box=box)
    cn = c.counters()
    got.update(route=c.route(), launches=cn.filter_kernel_launches, redo_pixels=cn.redo_pixels, options_active=cn.options_active)
    return got


def run_case(c, hipmod, name, mode="listed", **kw):
    _, _, _, box, D, _, _, rest, wide = CASES[name]
    return run(c, hipmod, planes_of(name), box, D, mode=mode, rest=rest, wide=wide, **kw)


def assert_same_pass(a, b, keys=STAGES + ("colour",), route=True):
    for k in keys:
        assert same_bits(a[k], b[k]), k
    assert (a["sum_nbhd"], a["max_nbhd"], a["launches"], a["redo_pixels"]) == (b["sum_nbhd"], b["max_nbhd"], b["launches"], b["redo_pixels"])
    if route:
        assert a["route"] == b["route"]


def check_stage4(planes, got, ref, box, label):
    """every sample within the per-sample bar of the expanded form (every pixel of route 12 runs a resident compiled kernel)"""
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(ref))
    cmax = B.cmax_of(planes[2:5])
    n = got["nbhd_size"]
    assert n.max() <= B.RESIDENT
    bar = B.sample_bar("expanded", 12, int(n.max()), SIGMA, box)
    worst = B.worst_sample(got["colour"], ref) / cmax
    print("SAMPLED_LISTED %s stage 4: worst %.3e (bar %.3e)" % (label, worst, bar))
    assert worst <= bar, (worst, bar)


class options:
    """options set on a shared context, put back on exit"""
    DEFAULTS = dict(wide=-1, sampled_fused_stride=-1, sampled_listed_stride=-1, binning=-1, wide_pool=-1, waves_per_pixel=0)

    def __init__(self, c, **kw):
        self.c, self.kw = c, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.c.set_option(k, v)

    def __exit__(self, *a):
        for k in self.kw:
            self.c.set_option(k, self.DEFAULTS[k])


# ---- 1 to 3. the restatement on every pixel, route 8, route 11 ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_stage_parity_on_every_pixel(ctx, hipmod, oracle, name):
    W, H, S, box, D, _, reach, rest, wide = CASES[name]
    planes = planes_of(name)
    want = ref_of(oracle, name)
    classes = classes_of(want["nbhd_size"])
    print("SAMPLED_LISTED %s: N %d .. %d, classes %s, window %d, stride %d" % (name, want["nbhd_size"].min(), want["nbhd_size"].max(), sorted(classes),
                                                                                box * box * S, stride_of(box, S)))
    assert set(reach) <= classes, (reach, sorted(classes))              # the frame reaches the kernels it is here for
    assert wide == (box * box * S > 65535)
    if name == "class8":
        assert classes == {8}
    if name == "box55":
        assert stride_of(box, S) == 378 and W < box and H < box         # every window clipped by the frame
    if name in ("big832", "rest1600", "cap"):
        assert (box * box - 1) * S > 4096                               # where route 11 shuts the four-wave kernels out
    if name == "cap":
        assert S + D == 3136
    if name == "wide22":
        assert box * box * S == 66550 and S + D <= 832                  # route 8's enumeration count kernel
    if name == "wide32":
        assert box * box * S == 96800 and S + D > 832                   # ... and its block kernel
    if name == "dups":   # more draws than the frame has candidates: most repeat an earlier one, on every pixel
        assert all(len(SR.draws(SEED, 0, 0, D, box, W, H, S, x, y)) <= (W * H - 1) * S < D for y in range(H) for x in range(W))
    got = run_case(ctx, hipmod, name)
    assert got["status"] == hipmod.OK and got["route"] == 12 and got["redo_pixels"] == 0
    assert got["launches"] == len(classes)                              # one launch per non-empty class; the count kernel is not counted
    # 1. the restatement
    for k in FRONT:
        assert np.array_equal(got[k], want[k]), k
    assert got["max_nbhd"] == want["nbhd_size"].max() and got["sum_nbhd"] == int(want["nbhd_size"].sum())
    assert np.array_equal(ctx.nbhd(W, H), want["nbhd_size"])
    np.testing.assert_allclose(got["mi"], want["mi"], rtol=0, atol=1e-11)
    for k in ("alpha", "beta", "wrc"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12)
    ref = SR.stage4_on(oracle, planes, got, (SEED, 0, D), 0, box, SIGMA, EPS)   # stage 4 on the device's own stage outputs, every sample
    check_stage4(planes, got, ref, box, name)
    # 2. route 8: the same call without the bit
    r8 = run_case(ctx, hipmod, name, mode="plain")
    assert r8["route"] == 8
    for k in BITS:
        assert same_bits(got[k], r8[k]), k
    assert (got["sum_nbhd"], got["max_nbhd"]) == (r8["sum_nbhd"], r8["max_nbhd"])
    # 3. route 11, where it applies: the same code behind the same list
    if not wide:
        r11 = run_case(ctx, hipmod, name, mode="fused")
        assert r11["route"] == 11
        assert_same_pass(got, r11, route=False)


# ---- 3b. the d27 compiled layout -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,S,box,D,reach", [(12, 10, 8, 7, 24, (16, 32)), (10, 8, 8, 17, 300, (128,))], ids=["packed", "one-wave"])   # (120 draws leave this generator below N = 65)
def test_compiled_27_dim_layout_takes_route_12(ctx, hipmod, oracle, W, H, S, box, D, reach):
    nr, nf = 4, 18
    stored = fb.synth_planes(W, H, S, seed=5, n_random=nr, n_feat=nf, dtype="f16")
    lay = dict(n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16)
    want = SR.sampled_pass(oracle, stored.astype(np.float32), (SEED, 0, D), 0, box, SIGMA, EPS, n_random=nr, n_feat=nf, weights=False)
    classes = classes_of(want["nbhd_size"])
    assert set(reach) <= classes, (reach, sorted(classes))
    got = run(ctx, hipmod, stored, box, D, lay=lay)
    assert got["route"] == 12 and got["status"] == hipmod.OK and got["launches"] == len(classes)
    for k in FRONT:
        assert np.array_equal(got[k], want[k]), k
    r8 = run(ctx, hipmod, stored, box, D, mode="plain", lay=lay)
    assert r8["route"] == 8
    for k in BITS:
        assert same_bits(got[k], r8[k]), k
    r11 = run(ctx, hipmod, stored, box, D, mode="fused", lay=lay)
    assert r11["route"] == 11
    assert_same_pass(got, r11, route=False)


# ---- 4. routing: staying put ---------------------------------------------------------------------------------------------------------
def stays(c, hipmod, planes, box, D, route, **kw):
    a = run(c, hipmod, planes, box, D, mode="plain", **kw)
    b = run(c, hipmod, planes, box, D, mode="listed", **kw)
    assert a["route"] == route, a["route"]
    assert_same_pass(b, a)
    return b


def test_stays_put_with_zero_draws(ctx, hipmod):
    with options(ctx, binning=1):
        got = stays(ctx, hipmod, planes_of("packed32"), 7, 0, 2)
    assert got["nbhd_size"].max() > 8 + 24


def test_stays_put_above_the_resident_cap(ctx, hipmod):
    W, H, S, box, D = 6, 5, 32, 17, 3105
    assert S + D == 3137
    stays(ctx, hipmod, frame(W, H, S, "iid"), box, D, 8, rest=True)
    assert run(ctx, hipmod, frame(W, H, S, "iid"), box, D - 1, rest=True)["route"] == 12      # ... and one draw fewer is taken


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
        stays(c, hipmod, planes_of("packed32"), 7, 24, 8, wide=True)
        c.set_option("wide", -1)
        assert run(c, hipmod, planes_of("packed32"), 7, 24, wide=True)["route"] == 12


def test_stays_put_with_a_gain_without_the_permission(ctx, hipmod):
    planes, box, D = planes_of("edge64"), 7, 56
    stays(ctx, hipmod, planes, box, D, 8, sched=hipmod.make_schedule(SIGMA, *GAINS), sigma_seed=0.002)
    # gains (1, 1): any pass with another seed, taken as without the schedule
    got = run(ctx, hipmod, planes, box, D, sched=hipmod.make_schedule(SIGMA, 1.0, 1.0), sigma_seed=0.002)
    assert got["route"] == 12
    assert_same_pass(got, run(ctx, hipmod, planes, box, D))


def test_both_bits_the_option_picks_the_route(hipmod):
    planes, box, D = planes_of("wave128"), 17, 120
    assert stride_of(box, 8) == 36
    with hipmod.Context(0) as c:
        auto = run(c, hipmod, planes, box, D, mode="both")
        assert auto["options_active"] == 0
        c.set_option("sampled_listed_stride", 37)
        r11 = run(c, hipmod, planes, box, D, mode="both")
        assert r11["route"] == 11 and r11["options_active"] == 1
        c.set_option("sampled_listed_stride", 36)                           # the bound is inclusive: route 12 from that stride on
        r12 = run(c, hipmod, planes, box, D, mode="both")
        assert r12["route"] == 12
        assert_same_pass(r12, r11, route=False)
        assert_same_pass(auto, r11, route=False)
        c.set_option("sampled_listed_stride", 0)
        assert run(c, hipmod, planes, 7, 24, mode="both")["route"] == 12
        c.set_option("sampled_listed_stride", 1025)                         # never where route 11 applies ...
        assert run(c, hipmod, planes, box, D, mode="both")["route"] == 11
        c.set_option("sampled_fused_stride", 35)                            # ... and always where it does not: above its stride bound,
        assert run(c, hipmod, planes, box, D, mode="both")["route"] == 12
        c.set_option("sampled_fused_stride", -1)
        got = run_case(c, hipmod, "wide22", mode="both")                    # or wide
        assert got["route"] == 12
        with pytest.raises(hipmod.RpfError):
            c.set_option("sampled_listed_stride", 1026)


# ---- 5. composition -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,S,box,D", [(12, 10, 8, 7, 56), (10, 8, 8, 17, 120)], ids=["box7-D56", "box17-D120"])
def test_draws_meet_the_configured_test(ctx, hipmod, oracle, W, H, S, box, D):
    """tests/test_member_test_gpu.py's two sampled frames on route 12, preset 1"""
    planes, mt = frame(W, H, S, flat_frac=0.94), MR.published19()
    want = MR.member_pass(oracle, planes, mt, box, SIGMA, EPS, cfg=(SEED, 0, D))
    got = run(ctx, hipmod, planes, box, D, mt=mt)
    assert got["route"] == 12 and got["status"] == hipmod.OK and got["redo_pixels"] == 0
    assert got["launches"] == len(classes_of(want["nbhd_size"]))
    assert want["nbhd_size"].max() > S
    for k in FRONT:
        assert np.array_equal(got[k], want[k]), k
    np.testing.assert_allclose(got["mi"], want["mi"], rtol=0, atol=1e-11)
    for k in ("alpha", "beta", "wrc"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12)
    check_stage4(planes, got, MR.stage4_on(oracle, planes, got, mt, box, SIGMA, EPS, cfg=(SEED, 0, D)), box, "member box %d" % box)
    r11 = run(ctx, hipmod, planes, box, D, mode="fused", mt=mt)
    assert r11["route"] == 11
    assert_same_pass(got, r11, route=False)
    plain = run(ctx, hipmod, planes, box, D)                              # another list than the 3-sigma test's
    assert plain["route"] == 12 and (plain["nbhd_size"] < got["nbhd_size"]).any()


@pytest.mark.parametrize("name", ["edge64", "wave128", "rest1600"])       # packed, one-wave, split route
def test_scheduled_gains_on_the_listed_scheduled_builds(ctx, hipmod, oracle, name):
    W, H, S, box, D, _, _, rest, wide = CASES[name]
    planes = planes_of(name)
    sched = hipmod.make_schedule(SIGMA, *GAINS)
    kw = dict(rest=rest, wide=wide, extra=hipmod.SCHEDULE_FUSED_FLAG, sigma_seed=0.002)
    base = run(ctx, hipmod, planes, box, D, sched=hipmod.make_schedule(SIGMA, 1.0, 1.0), **kw)
    got = run(ctx, hipmod, planes, box, D, sched=sched, **kw)
    assert base["route"] == got["route"] == 12 and got["status"] == hipmod.OK
    for k in BITS + ("mi", "wrc"):                                       # everything in front of stage 3c: the gains-(1, 1) run's bits
        assert same_bits(got[k], base[k]), k
    assert (got["launches"], got["sum_nbhd"], got["max_nbhd"]) == (base["launches"], base["sum_nbhd"], base["max_nbhd"])
    assert_same_pass(base, run_case(ctx, hipmod, name))                 # gains (1, 1) with the entry's seed: the unscheduled pass
    want = SRf.scheduled_pass(oracle, planes, (SIGMA,) + GAINS, box, cfg=(SEED, 0, D))
    for k in ("nbhd_size", "mean", "stddev"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("alpha", "beta"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12)
    a, b, w = SRf.alpha_beta(got["mi"], GAINS[0], GAINS[1], 0, 1e-10)    # stage 3c on the device's own MI: bit for bit
    assert same_or_nan(got["alpha"], a) and same_or_nan(got["beta"], b) and same_or_nan(got["wrc"], w)
    assert not same_bits(got["alpha"], base["alpha"]) and not same_bits(got["beta"], base["beta"])
    check_stage4(planes, got, SRf.stage4_on(oracle, planes, got, SIGMA, box, EPS, cfg=(SEED, 0, D)), box, "scheduled " + name)
    r11 = run(ctx, hipmod, planes, box, D, mode="fused", sched=sched, **kw)     # the scheduled builds behind the masks
    assert r11["route"] == 11
    assert_same_pass(got, r11, route=False)


def call(c, hipmod, planes, boxes, flags, draws, pass0=0, colour64_in=None, seed=SEED):
    """one call through rpf_filter_ex, its passes with ids pass0 .. (a schedule's entries stand for the descriptor's seed)"""
    _, H, W, S = planes.shape
    c.set_sampling(hipmod.make_sampling(seed, draws, pass_id0=pass0))
    desc = hipmod.make_desc(W, H, S, boxes=boxes, policy=EPS, sigma_seed=SIGMA, flags=flags)
    out = c.filter(planes, desc, colour64_in=colour64_in, want_colour64=True)
    assert out[2] == hipmod.OK
    return out[3], c.route(), c.counters()


def test_the_published_call(ctx, hipmod):
    """all bits plus spike clamp and pass report, the published boxes and draws at 8 spp on a 12 x 10 frame"""
    planes = frame(12, 10, 8, flat_frac=0.5)
    boxes, draws = (55, 35, 17, 7), (484, 392, 120, 24)
    seeds, gc, gf = [SIGMA, SIGMA / 2, SIGMA / 4, SIGMA / 8], [2.2, 1.3, 1.2, 1.0], [1.1, 1.15, 1.0, 1.0]
    mt = MR.published19()
    H_ = hipmod
    common = H_.SAMPLED_NBHD_FLAG | H_.MEMBER_TEST_FLAG | H_.MEMBER_FUSED_FLAG | H_.SCHEDULE_FLAG | H_.SCHEDULE_FUSED_FLAG
    listed, fused = common | H_.SAMPLED_LISTED_FLAG, common | H_.SAMPLED_FUSED_FLAG
    old = H_.SAMPLED_NBHD_FLAG | H_.MEMBER_TEST_FLAG | H_.SCHEDULE_FLAG
    ctx.set_membership(hipmod.make_membership(mt[0].tolist(), mt[1].tolist()))
    ctx.set_spike(1.0, True)
    ctx.set_schedule(hipmod.make_schedule(seeds, gc, gf))
    whole, route, cn = call(ctx, hipmod, planes, boxes, listed | H_.FLAG_SPIKE_CLAMP | H_.PASS_REPORT_FLAG, draws)
    reps = [ctx.pass_report(p) for p in range(4)]
    assert route == 12 and [r.route for r in reps] == [12] * 4 and ctx.spike_stats().applied == 1
    assert cn.filter_kernel_launches >= 1 and cn.redo_pixels == 0
    unchanged = [r.total.unchanged_samples for r in reps]
    plain, _, _ = call(ctx, hipmod, planes, boxes, listed | H_.FLAG_SPIKE_CLAMP, draws)                # the report changes no result
    assert same_bits(plain, whole)
    # the chain of one-pass calls, the spike pass behind the last; the report's unchanged samples from each pass's two colour buffers
    colour = None
    for p, box in enumerate(boxes):
        ctx.set_schedule(hipmod.make_schedule(seeds, gc, gf, pass0=p))
        before = planes[2:5].astype(np.float64) if colour is None else colour
        colour, r, cn1 = call(ctx, hipmod, planes, (box,), listed, [draws[p]], pass0=p, colour64_in=colour)
        assert r == 12
        assert unchanged[p] == int(PR.pixel_values(before, colour)[1].sum()), p
    ctx.set_schedule(hipmod.make_schedule(seeds, gc, gf, pass0=3))
    last, _, cn1 = call(ctx, hipmod, planes, (boxes[3],), listed | H_.FLAG_SPIKE_CLAMP, [draws[3]], pass0=3, colour64_in=before)
    assert same_bits(whole, last)
    assert (cn.sum_nbhd, cn.max_nbhd, cn.redo_pixels) == (cn1.sum_nbhd, cn1.max_nbhd, 0)           # of the last pass
    # the same call on route 11 and on route 8: the colour bar, the same neighbourhoods
    ctx.set_schedule(hipmod.make_schedule(seeds, gc, gf))
    cmax = B.cmax_of(planes[2:5])
    for flags, want_route in ((fused, 11), (old, 8)):
        other, _, cn8 = call(ctx, hipmod, planes, boxes, flags | H_.FLAG_SPIKE_CLAMP | H_.PASS_REPORT_FLAG, draws)
        assert [ctx.pass_report(p).route for p in range(4)] == [want_route] * 4
        assert (cn8.sum_nbhd, cn8.max_nbhd) == (cn.sum_nbhd, cn.max_nbhd)
        assert [ctx.pass_report(p).total.sum_nbhd for p in range(4)] == [r.total.sum_nbhd for r in reps]
        assert np.abs(whole - other).max() <= 1e-4 * cmax
        if want_route == 11:
            assert same_bits(whole, other)


# ---- 6. the same bits any way it is cut ----------------------------------------------------------------------------------------------
def need_devices(devices):
    import torch
    if max(devices) >= torch.cuda.device_count():
        pytest.skip("needs %d visible GPUs" % (max(devices) + 1))


def test_chain_of_one_pass_calls_equals_one_call(ctx, hipmod):
    planes = frame(12, 10, 8)
    boxes, draws = (17, 7, 17), (120, 24, 200)
    whole, route, _ = call(ctx, hipmod, planes, boxes, flags_of(hipmod) | hipmod.PASS_REPORT_FLAG, draws)
    assert [ctx.pass_report(p).route for p in range(3)] == [12, 12, 12]
    colour = None
    for p, box in enumerate(boxes):
        colour, r, _ = call(ctx, hipmod, planes, (box,), flags_of(hipmod), [draws[p]], pass0=p, colour64_in=colour)
        assert r == 12
    assert same_bits(whole, colour)


@pytest.mark.parametrize("devices", [(0, 0), (0, 1)])
def test_multi_filter_equals_one_context(ctx, hipmod, devices):
    need_devices(devices)
    W, H, S = 10, 24, 8
    planes, cfg = frame(W, H, S), hipmod.make_sampling(SEED, [120, 24], pass_id0=3)
    desc = hipmod.make_desc(W, H, S, boxes=(17, 7), policy=EPS, sigma_seed=SIGMA, flags=flags_of(hipmod))
    ctx.set_sampling(cfg)
    s1, p1, st1 = ctx.filter(planes, desc)
    c1 = ctx.counters()
    assert ctx.route() == 12 and c1.max_nbhd > S
    with hipmod.MultiContext(list(devices)) as mc:
        mc.set_sampling(cfg)
        s2, p2, st2 = mc.filter(planes, desc)
        c2 = mc.counters()
        s3, _, _ = mc.filter(planes, desc)                                           # row_origin does not drift between calls
    assert st1 == st2 == hipmod.OK
    assert np.array_equal(s1.view(np.uint32), s2.view(np.uint32)) and np.array_equal(p1.view(np.uint32), p2.view(np.uint32))
    assert np.array_equal(s2.view(np.uint32), s3.view(np.uint32))
    assert (c2.samples_filtered, c2.sum_nbhd, c2.max_nbhd, c2.redo_pixels) == (c1.samples_filtered, c1.sum_nbhd, c1.max_nbhd, 0)


def test_banded_call_gives_the_serial_call_s_bits(ctx, hipmod):
    """48 rows are three bands of rpf_filter's row-band pipeline: each band its own count pass and pool, the keys by image row"""
    W, H, S = 6, 48, 8
    planes = frame(W, H, S)
    ctx.set_sampling(hipmod.make_sampling(SEED, [24, 40, 24]))
    for boxes in ((7,), (7, 5, 7)):
        desc = hipmod.make_desc(W, H, S, boxes=boxes, policy=EPS, sigma_seed=SIGMA, flags=flags_of(hipmod))
        s_serial, p_serial, st, c64 = ctx.filter(planes, desc, want_colour64=True)     # rpf_filter_ex
        assert st == hipmod.OK and ctx.route() == 12
        pin = ctx.host_empty(planes.shape, planes.dtype)
        pin[...] = planes
        out_s, out_p = ctx.host_empty(s_serial.shape), ctx.host_empty(p_serial.shape)
        ctx.filter(pin, desc, out_samples=out_s, out_pixels=out_p)                  # rpf_filter from page-locked buffers
        assert ctx.route() == 12
        assert np.array_equal(out_s, s_serial) and np.array_equal(out_p, p_serial)
        assert np.array_equal(s_serial, c64.astype(np.float32))


def test_two_runs_and_a_pool_that_has_to_grow(hipmod):
    """option wide_pool = 1: one entry at the first count launch, grown once to the cursor's figure, the count repeated"""
    for name in ("wave128", "wide22"):                                    # the bitmap kernel's listing tail, route 8's own
        with hipmod.Context(0) as c:
            a = run_case(c, hipmod, name)
            b = run_case(c, hipmod, name)
            assert_same_pass(a, b)
            c.set_option("wide_pool", 1)
            small = run_case(c, hipmod, name)
            assert small["route"] == 12 and small["options_active"] == 1
            assert_same_pass(small, a)
            assert a["sum_nbhd"] > a["nbhd_size"].size * CASES[name][2] + 1      # the pool needed more than the one entry


def test_refusals_on_the_device_entry_points(hipmod):
    planes = planes_of("packed32")
    _, H, W, S = planes.shape
    N, L = hipmod.SAMPLED_NBHD_FLAG, hipmod.SAMPLED_LISTED_FLAG
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
        for m in (c, mc):
            m.set_sampling(hipmod.make_sampling(1, [24]))
        refused(desc(L), hipmod.E_UNSUPPORTED, "SAMPLED_LISTED")                     # the bit without RPF_FLAG_SAMPLED_NBHD
        refused(desc(L | hipmod.SAMPLED_FUSED_FLAG), hipmod.E_UNSUPPORTED, "SAMPLED_LISTED")
        assert hipmod.layout_kernels(desc(L)) == (hipmod.E_UNSUPPORTED, None)
        # with it, the parent's refusals stand
        refused(desc(N | L, REF_ABORT), hipmod.E_UNSUPPORTED, "REF_ABORT")
        refused(desc(N | L | hipmod.FLAG_FAST_WEIGHTS), hipmod.E_UNSUPPORTED, "FAST_WEIGHTS")
        for m in (c, mc):
            m.set_sampling(hipmod.make_sampling(1, [832 - S + 1]))
        refused(desc(N | L), hipmod.E_BADARG, "832")                                 # S + D = 833 still needs RPF_FLAG_SAMPLED_REST
        c.set_sampling(hipmod.make_sampling(1, [832 - S]))
        assert c.filter_pass_debug(planes, desc(N | L), box=7)["status"] == hipmod.OK and c.route() == 12


def test_a_wide_pass_still_needs_wide_nbhd(hipmod):
    W, H, S, box, D = CASES["wide22"][:5]
    with hipmod.Context(0) as c:
        c.set_sampling(hipmod.make_sampling(SEED, [D]))
        d = hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=SIGMA, flags=flags_of(hipmod))
        with pytest.raises(hipmod.RpfError) as e:
            c.filter_pass_debug(planes_of("wide22"), d, box=box)
        assert e.value.status == hipmod.E_UNSUPPORTED and "65535" in str(e.value)


# ---- 7. the membership cache of the size-binned route --------------------------------------------------------------------------------
def test_cache_is_neither_served_nor_poisoned(hipmod):
    """a route-2 pass, a route-12 pass and the route-2 pass again at the same box, in one call: the third pass must count again"""
    planes = frame(12, 10, 8)
    with hipmod.Context(0) as c:
        c.set_option("binning", 1)
        three, route, _ = call(c, hipmod, planes, (7, 7, 7), flags_of(hipmod) | hipmod.PASS_REPORT_FLAG, (0, 24, 0))
        assert [c.pass_report(p).route for p in range(3)] == [2, 12, 2]
        colour = None
        for p, d in enumerate((0, 24, 0)):
            colour, r, _ = call(c, hipmod, planes, (7,), flags_of(hipmod), [d], pass0=p, colour64_in=colour)
            assert r == (12 if d else 2)
        assert same_bits(three, colour)


# ---- on top ------------------------------------------------------------------------------------------------------------------------
def test_pass_report_n_fields_equal_route_8(ctx, hipmod):
    planes = planes_of("wave128")
    reps = {}
    for mode in ("plain", "listed"):
        call(ctx, hipmod, planes, (17,), flags_of(hipmod, mode) | hipmod.PASS_REPORT_FLAG, [120])
        reps[mode] = ctx.pass_report(0)
    a, b = reps["plain"], reps["listed"]
    assert (a.applied, b.applied, a.route, b.route) == (1, 1, 8, 12)
    assert (b.box, b.rows, b.pixels, b.samples, b.draws) == (a.box, a.rows, a.pixels, a.samples, a.draws)
    for k in ("sum_nbhd", "min_nbhd", "max_nbhd", "own_only_pixels"):
        assert getattr(b.total, k) == getattr(a.total, k), k
    assert list(b.total.class_pixels) == list(a.total.class_pixels) and sum(b.total.class_pixels) == b.pixels
