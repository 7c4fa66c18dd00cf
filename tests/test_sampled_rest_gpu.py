"""GPU tests of RPF_FLAG_SAMPLED_REST (sampled passes with 832 < S + draws <= 8192): the block count kernel
and the rest launch that reads listed members, against the numpy restatement tests/sampled_ref.py on every pixel of every frame;
that a small pass and a call without the flag are what they were; the membership test, the schedule and the spike pass on top;
the other layouts, slabs and entry points, the pool's grow path, determinism, and the refusals of every device entry point.  The
design, the bars and the frames are those of tests/test_sampled_gpu.py; EPS policy throughout."""
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
SEED = 0x5EED5EED
SIGMA = 0.5
CAPS = (8, 16, 32, 64, 128, 256, 448, 832)
REST = 833                       # class_of() of a pixel on the rest list

# name: W, H, S, box, D, generator mode, what the frame must reach (class capacities; REST: a non-empty rest list)
CASES = {
    "over833": (14, 12, 32, 17, 801, "iid", (832,)),             # S + D = 833: the block count kernel, every pixel still in a class
    "odd1025": (14, 12, 32, 17, 1025, "iid", (832,)),            # the keys padded from 1025 to 2048
    "mix2048": (14, 12, 32, 17, 2016, "iid", (832, REST)),       # S + D a power of two; classes and rest list in one pass
    "odd3001": (14, 12, 32, 17, 3001, "iid", (REST,)),
    "cap8192": (14, 12, 32, 17, 8160, "iid", (REST,)),           # the cap: heavy duplicates, every pixel on the rest list
    "box7": (12, 10, 32, 7, 2016, "smooth", (832, REST)),        # a small window
    "s8": (20, 16, 8, 17, 4088, "iid", (832, REST)),
    "s840": (5, 4, 840, 3, 160, "smooth", (REST,)),              # S > 832: every pixel on the rest list by construction
    # box * box * S > 65535: with RPF_FLAG_WIDE_NBHD, as route 8 takes such a pass today (most draws of sigma = 55 / 4 leave a 10 x 8 buffer)
    "wide55": (10, 8, 32, 55, 8160, "iid", (832,)),
}
BITS = ("nbhd_size", "member_hash", "bin_hash", "mean", "stddev", "mi", "alpha", "beta", "wrc", "colour")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def class_of(n):
    return next((c for c in CAPS if n <= c), REST)


def launches_of(nbhd):
    """one launch per non-empty class plus one for a non-empty rest list"""
    return len({class_of(int(n)) for n in np.asarray(nbhd).ravel()})


@functools.lru_cache(maxsize=None)
def frame(W, H, S, mode):
    p = fb.synth_planes(W, H, S, seed=11) if mode == "iid" else fb.synth_planes(W, H, S, seed=11, mode=mode)
    if mode == "iid":  # the smooth frame with its features replaced by unit normals, the same law in every pixel: most draws pass
        p[7:] = np.random.default_rng(11).standard_normal(p[7:].shape).astype(np.float32)
    p.setflags(write=False)
    return p


def planes_of(name):
    W, H, S, _, _, mode, _ = CASES[name]
    return frame(W, H, S, mode)


_refs = {}


def ref_of(oracle, name):
    """the restatement of the case's pass: computed once, shared, never modified.  A box below 4 has sigma_p = box // 4 = 0, where
    sampled_ref's stage 4 divides Python floats by zero; schedule_ref restates the same pass (gains of exactly 1 are the
    unscheduled expressions, its members are member_test_ref's under the reference's test on the same draws) with that quotient
    in IEEE arithmetic, and the member codes come from member_test_ref.counts"""
    if name not in _refs:
        _, _, _, box, D, _, _ = CASES[name]
        if box // 4 > 0:
            _refs[name] = SR.sampled_pass(oracle, planes_of(name), (SEED, 0, D), 0, box, SIGMA, EPS)
        else:
            want = SRf.scheduled_pass(oracle, planes_of(name), (SIGMA, 1.0, 1.0), box, cfg=(SEED, 0, D))
            n, codes = MR.counts(oracle, planes_of(name), MR.reference(), box, cfg=(SEED, 0, D))
            assert np.array_equal(n, want["nbhd_size"])
            want["member_hash"] = np.zeros(n.shape, np.uint32)
            for (y, x), c in codes.items():
                want["member_hash"][y, x] = SR.fnv1a_u32(c)
            _refs[name] = want
    return _refs[name]


def stage4_of(oracle, name, got):
    """stage 4 restated on the device's own stage outputs (ref_of says why a box below 4 goes through schedule_ref)"""
    _, _, _, box, D, _, _ = CASES[name]
    if box // 4 > 0:
        return SR.stage4_on(oracle, planes_of(name), got, (SEED, 0, D), 0, box, SIGMA, EPS)
    return SRf.stage4_on(oracle, planes_of(name), got, SIGMA, box, EPS, cfg=(SEED, 0, D))


def flags_of(hipmod, rest=True, extra=0):
    return hipmod.SAMPLED_NBHD_FLAG | (hipmod.SAMPLED_REST_FLAG if rest else 0) | extra


def run(c, hipmod, planes, box, D, extra=0, rest=True, colour_in=None):
    _, H, W, S = planes.shape
    c.set_sampling(hipmod.make_sampling(SEED, [D]))
    wide = hipmod.FLAG_WIDE_NBHD if box * box * S > 65535 else 0
    desc = hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=SIGMA, flags=flags_of(hipmod, rest, extra | wide))
    got = c.filter_pass_debug(planes, desc, box=box, colour_in=colour_in)
    cn = c.counters()
    got.update(route=c.route(), launches=cn.filter_kernel_launches, redo_pixels=cn.redo_pixels)
    return got


def run_case(c, hipmod, name, extra=0):
    _, _, _, box, D, _, _ = CASES[name]
    return run(c, hipmod, planes_of(name), box, D, extra)


_base = {}


def base_of(ctx, hipmod, name):
    """the plain flagged run of a case, shared by the tests that compare against it"""
    if name not in _base:
        _base[name] = run_case(ctx, hipmod, name)
    return _base[name]


# ---- stage parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_stage_parity_on_every_pixel(ctx, hipmod, oracle, name):
    """Fails on the parent commit, which refuses S + draws > 832."""
    W, H, S, box, D, _, reach = CASES[name]
    want = ref_of(oracle, name)
    classes = {class_of(int(n)) for n in want["nbhd_size"].ravel()}
    assert set(reach) <= classes, (reach, sorted(classes))              # the frame reaches the kernels it is here for
    got = run_case(ctx, hipmod, name)
    print("SAMPLED_REST %s: N %d .. %d, classes %s, %d rest pixels" % (
        name, want["nbhd_size"].min(), want["nbhd_size"].max(), sorted(classes), int((want["nbhd_size"] > 832).sum())))
    assert got["status"] == hipmod.OK and got["route"] == 8 and got["redo_pixels"] == 0
    assert got["launches"] == len(classes)                              # one launch per non-empty class, one for the rest list
    assert np.array_equal(got["nbhd_size"], want["nbhd_size"])
    assert np.array_equal(got["member_hash"], want["member_hash"])
    assert np.array_equal(got["mean"], want["mean"]) and np.array_equal(got["stddev"], want["stddev"])
    np.testing.assert_allclose(got["mi"], want["mi"], rtol=0, atol=1e-11)           # check_pass's bars
    for k in ("alpha", "beta", "wrc"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12)
    assert got["max_nbhd"] == want["nbhd_size"].max() and got["sum_nbhd"] == int(want["nbhd_size"].sum())
    assert np.array_equal(ctx.nbhd(W, H), want["nbhd_size"])
    # stage 4: the restatement on the device's own stage outputs, every sample, the direct form's bar
    ref = stage4_of(oracle, name, got)
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(ref))
    cmax = B.cmax_of(planes_of(name)[2:5])
    bar = B.sample_bar("direct", 12, int(want["nbhd_size"].max()), SIGMA, box)
    worst = B.worst_sample(got["colour"], ref) / cmax
    print("SAMPLED_REST %s stage 4: worst %.3e (bar %.3e)" % (name, worst, bar))
    assert worst <= bar, (worst, bar)
    assert np.abs(got["colour"] - want["colour"]).max() <= 1e-4 * cmax              # and the whole restatement, loosely


# ---- unchanged without need ---------------------------------------------------------------------------------------------------
def test_small_pass_is_the_pass_without_the_flag(ctx, hipmod):
    planes = frame(12, 10, 8, "smooth")
    a, b = run(ctx, hipmod, planes, 7, 56, rest=False), run(ctx, hipmod, planes, 7, 56, rest=True)
    assert a["route"] == b["route"] == 8 and a["launches"] == b["launches"] and a["max_nbhd"] == b["max_nbhd"] > 8
    for k in BITS:
        assert same_bits(a[k], b[k]), k


def test_without_the_flag_833_is_still_refused(ctx, hipmod):
    planes = frame(12, 10, 8, "smooth")
    with pytest.raises(hipmod.RpfError) as e:
        run(ctx, hipmod, planes, 7, 832 - 8 + 1, rest=False)
    assert e.value.status == hipmod.E_BADARG and "832" in str(e.value)


# ---- composition, on mix2048 --------------------------------------------------------------------------------------------------
def test_with_the_membership_test(ctx, hipmod, oracle):
    _, _, _, box, D, _, _ = CASES["mix2048"]
    planes, base = planes_of("mix2048"), base_of(ctx, hipmod, "mix2048")
    ref3 = MR.reference()
    ctx.set_membership(hipmod.make_membership(ref3[0].tolist(), ref3[1].tolist()))     # preset kind 0: the reference's test
    got = run_case(ctx, hipmod, "mix2048", hipmod.MEMBER_TEST_FLAG)
    assert got["route"] == 8 and got["launches"] == base["launches"]
    for k in BITS:
        assert same_bits(got[k], base[k]), k
    mt = (np.full(12, 2.0), np.full(12, 0.5))                                         # a second table
    want = MR.member_pass(oracle, planes, mt, box, SIGMA, EPS, weights=False, cfg=(SEED, 0, D))
    ctx.set_membership(hipmod.make_membership(mt[0].tolist(), mt[1].tolist()))
    got = run_case(ctx, hipmod, "mix2048", hipmod.MEMBER_TEST_FLAG)
    assert got["route"] == 8 and got["status"] == hipmod.OK and got["launches"] == launches_of(want["nbhd_size"])
    assert (want["nbhd_size"] != base["nbhd_size"]).any()
    assert np.array_equal(got["nbhd_size"], want["nbhd_size"]) and np.array_equal(got["member_hash"], want["member_hash"])
    assert np.array_equal(got["mean"], want["mean"]) and np.array_equal(got["stddev"], want["stddev"])


def test_with_the_schedule(ctx, hipmod, oracle):
    _, _, _, box, D, _, _ = CASES["mix2048"]
    planes, base, gains = planes_of("mix2048"), base_of(ctx, hipmod, "mix2048"), (2.0, 1.1)
    ctx.set_schedule(hipmod.make_schedule(SIGMA, *gains))
    got = run_case(ctx, hipmod, "mix2048", hipmod.SCHEDULE_FLAG)
    assert got["route"] == 8 and got["status"] == hipmod.OK and got["launches"] == base["launches"]
    for k in ("nbhd_size", "member_hash", "bin_hash", "mean", "stddev", "mi", "wrc"):  # stages 1 to 3b and W_r_c: the unscheduled bits
        assert same_bits(got[k], base[k]), k
    a, b, w = SRf.alpha_beta(got["mi"], gains[0], gains[1], 0, 1e-10)                  # stage 3c on the device's own MI, bit for bit
    assert same_bits(got["alpha"], a) and same_bits(got["beta"], b) and same_bits(got["wrc"], w)
    assert not same_bits(got["alpha"], base["alpha"]) and not same_bits(got["beta"], base["beta"])
    rest = got["nbhd_size"] > 832                                                     # ... on the rest pixels and on the class pixels
    assert rest.any() and (~rest).any()
    assert (got["alpha"][rest] != base["alpha"][rest]).any() and (got["alpha"][~rest] != base["alpha"][~rest]).any()
    ref = SRf.stage4_on(oracle, planes, got, SIGMA, box, EPS, cfg=(SEED, 0, D))
    cmax = B.cmax_of(planes[2:5])
    assert B.worst_sample(got["colour"], ref) / cmax <= B.sample_bar("direct", 12, int(got["nbhd_size"].max()), SIGMA, box)


def c64_of(c, hipmod, planes, boxes, draws, extra=0, rest=True, colour64_in=None):
    _, H, W, S = planes.shape
    c.set_sampling(hipmod.make_sampling(SEED, draws))
    desc = hipmod.make_desc(W, H, S, boxes=boxes, policy=EPS, sigma_seed=SIGMA, flags=flags_of(hipmod, rest, extra))
    out = c.filter(planes, desc, colour64_in=colour64_in, want_colour64=True)
    assert out[2] == hipmod.OK
    return out


def test_spike_pass_on_top(ctx, hipmod):
    _, _, _, box, D, _, _ = CASES["mix2048"]
    planes = planes_of("mix2048")
    plain = c64_of(ctx, hipmod, planes, (box,), [D])[3]
    assert ctx.route() == 8 and same_bits(plain, base_of(ctx, hipmod, "mix2048")["colour"])
    ctx.set_spike(1.0, True)
    spiked = c64_of(ctx, hipmod, planes, (box,), [D], hipmod.FLAG_SPIKE_CLAMP)[3]
    want = spike_ref.apply(plain, 1.0, True)
    assert ctx.route() == 8 and ctx.spike_stats().applied == 1
    assert same_bits(spiked, want["colour"])


# ---- other layouts: N, member hash, mean / std --------------------------------------------------------------------------------
@pytest.mark.parametrize("nr,nf,needs_generic", [(3, 7, True), (4, 18, False)], ids=["generic-3-7-f16", "compiled-4-18-f16"])
def test_other_layouts(ctx, hipmod, oracle, nr, nf, needs_generic):
    W, H, S, box, D = 14, 12, 32, 17, 2016
    stored = fb.synth_planes(W, H, S, seed=5, n_random=nr, n_feat=nf, dtype="f16")
    stored[5 + nr:] = np.random.default_rng(11).standard_normal(stored[5 + nr:].shape).astype(stored.dtype)
    want = SR.sampled_pass(oracle, stored.astype(np.float32), (SEED, 0, D), 0, box, SIGMA, EPS, n_random=nr, n_feat=nf, weights=False)
    flags = flags_of(hipmod, True, hipmod.FLAG_GENERIC if needs_generic else 0)
    desc = hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=SIGMA, flags=flags, n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16)
    ctx.set_sampling(hipmod.make_sampling(SEED, [D]))
    got = ctx.filter_pass_debug(stored, desc, box=box)
    assert ctx.route() == 8 and got["status"] == hipmod.OK
    assert (want["nbhd_size"] > 832).any() and (want["nbhd_size"] <= 832).any()       # rest list and classes
    assert ctx.counters().filter_kernel_launches == launches_of(want["nbhd_size"])
    assert np.array_equal(got["nbhd_size"], want["nbhd_size"]) and np.array_equal(got["member_hash"], want["member_hash"])
    assert np.array_equal(got["mean"], want["mean"]) and np.array_equal(got["stddev"], want["stddev"])


# ---- slabs and entry points ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_multi_filter_equals_one_context(ctx, hipmod, devices):
    """mix2048's frame at twice its height: rpf_multi_filter wants every slab at least as tall as the halo, (box - 1) / 2 = 8 rows,
    and the twelve rows of mix2048 give two slabs six each (refused: "a row slab is thinner than the halo").  Same width, S, box,
    draws and construction at H = 24: slabs of 12 and of 8 rows, classes and rest list on every slab"""
    W, _, S, box, D, mode, _ = CASES["mix2048"]
    H = 24
    planes = frame(W, H, S, mode)
    s1, p1, st1 = c64_of(ctx, hipmod, planes, (box,), [D])[:3]
    c1, n1 = ctx.counters(), ctx.nbhd(W, H)
    assert ctx.route() == 8
    for rows in np.array_split(n1, len(devices), axis=0):
        assert (rows > 832).any() and (rows <= 832).any()
    desc = hipmod.make_desc(W, H, S, boxes=(box,), policy=EPS, sigma_seed=SIGMA, flags=flags_of(hipmod))
    with hipmod.MultiContext(list(devices)) as mc:
        mc.set_sampling(hipmod.make_sampling(SEED, [D]))
        s2, p2, st2 = mc.filter(planes, desc)
        c2 = mc.counters()
    assert st1 == st2 == hipmod.OK
    assert same_bits(s1, s2) and same_bits(p1, p2)
    assert (c2.samples_filtered, c2.sum_nbhd, c2.max_nbhd, c2.redo_pixels) == (c1.samples_filtered, c1.sum_nbhd, c1.max_nbhd, 0)


def test_two_pass_call_equals_the_passes_chained(ctx, hipmod):
    """boxes (17, 7), draws (2016, 0): the second pass is no sampled pass and takes its usual route"""
    _, _, _, box, D, _, _ = CASES["mix2048"]
    planes = planes_of("mix2048")
    both = c64_of(ctx, hipmod, planes, (box, 7), [D, 0])[3]
    route_both = ctx.route()
    first = base_of(ctx, hipmod, "mix2048")["colour"]
    _, H, W, S = planes.shape
    second = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=SIGMA), box=7, colour_in=first)
    assert ctx.route() == route_both != 8
    assert same_bits(both, second["colour"]) and not same_bits(both, first)


def test_filter_device_equals_filter(ctx, hipmod):
    import torch
    _, _, _, box, D, _, _ = CASES["mix2048"]
    planes = planes_of("mix2048")
    want = c64_of(ctx, hipmod, planes, (box,), [D])[3]
    _, H, W, S = planes.shape
    dev = torch.device("cuda", 0)
    dp = torch.from_numpy(np.array(planes)).to(dev)
    col = dp[2:5].to(torch.float64).contiguous()
    desc = hipmod.make_desc(W, H, S, boxes=(box,), policy=EPS, sigma_seed=SIGMA, flags=flags_of(hipmod))
    ctx.filter_device(desc, dp.data_ptr(), col.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ctx.route() == 8 and ctx.counters().max_nbhd > 832
    assert same_bits(col.cpu().numpy(), want)


# ---- the pool's grow path, determinism ----------------------------------------------------------------------------------------
def test_wide_pool_option_forces_the_grow_path_same_bits(ctx, hipmod):
    base = base_of(ctx, hipmod, "cap8192")
    with hipmod.Context(0) as c:
        c.set_option("wide_pool", 16)
        got = run_case(c, hipmod, "cap8192")
        assert c.counters().options_active == 1
    assert got["route"] == 8 and got["launches"] == base["launches"]
    for k in BITS:
        assert same_bits(got[k], base[k]), k


def test_determinism(ctx, hipmod):
    a, b = base_of(ctx, hipmod, "cap8192"), run_case(ctx, hipmod, "cap8192")
    with hipmod.Context(0) as c:
        fresh = run_case(c, hipmod, "cap8192")
    for k in BITS:
        assert same_bits(a[k], b[k]) and same_bits(a[k], fresh[k]), k


# ---- refusals, from every device entry point, before any device work ----------------------------------------------------------
def test_refusals_on_the_device_entry_points(hipmod):
    planes = frame(12, 10, 8, "smooth")
    _, H, W, S = planes.shape
    F, G = flags_of(hipmod), hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED
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
            for name, call in calls.items():
                with pytest.raises(hipmod.RpfError) as e:
                    call(d)
                assert e.value.status == status and word in str(e.value), (name, str(e.value))
        for m in (c, mc):
            m.set_sampling(hipmod.make_sampling(1, [8192 - S + 1]))
        refused(desc(F), hipmod.E_BADARG, "8192")                                    # S + D = 8193
        refused(desc(hipmod.SAMPLED_REST_FLAG), hipmod.E_UNSUPPORTED, "SAMPLED_NBHD")  # the modifier without its flag
        for m in (c, mc):
            m.set_sampling(hipmod.make_sampling(1, [2016]))
        refused(desc(F, REF_ABORT), hipmod.E_UNSUPPORTED, "REF_ABORT")
        refused(desc(F | hipmod.FLAG_FAST_WEIGHTS), hipmod.E_UNSUPPORTED, "FAST_WEIGHTS")
        refused(desc(F | G | hipmod.FLAG_GENERIC_FAST), hipmod.E_UNSUPPORTED, "GENERIC_FAST")
        refused(desc(F | hipmod.FLAG_GENERIC | hipmod.FLAG_STREAM_FAST), hipmod.E_UNSUPPORTED, "STREAM_FAST")
        # ... and S + D = 8192 is accepted
        c.set_sampling(hipmod.make_sampling(1, [8192 - S]))
        assert c.filter_pass_debug(planes, desc(F), box=7)["status"] == hipmod.OK and c.route() == 8
