"""GPU tests of the membership test (RPF_FLAG_MEMBER_TEST, rpf_query_route 9) against the numpy restatement
tests/member_test_ref.py, on every pixel of every frame: the anchor (the reference's multiples and floors give the unflagged
pass), stage parity per size class and on the rest list, the flat proof, NaN and infinity, the other layouts, sampled passes
under the test (route 8), a two-pass call, slabs, the pool's grow path, the spike pass on top, the refusals of every device entry
point, and an unflagged call after a flagged one.  EPS policy throughout (REF_ABORT is refused), sigma_seed 0.5 (the filter is
active)."""
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
CLUSTERED = dict(mode="clustered", sigma_f=1e-3, sigma_c=0.01)
BITS = ("nbhd_size", "member_hash", "mean", "stddev", "bin_hash")

# name: W, H, S, box, generator arguments, floors as a multiple of preset 1's, the classes the frame must reach (833: the rest list)
CASES = {
    "wave": (12, 10, 8, 7, dict(flat_frac=0.94), 1.0, (128, 256, 448)),
    "wave-c": (12, 10, 8, 7, dict(flat_frac=0.94, **CLUSTERED), 1.0, (128, 256, 448)),
    "rest": (16, 13, 8, 11, dict(flat_frac=0.94), 1.0, (448, 832, 833)),
    "rest-c": (16, 13, 8, 11, dict(flat_frac=0.94, **CLUSTERED), 1.0, (448, 832, 833)),
    "packed": (6, 5, 2, 5, dict(), 0.1, (8, 16)),
    "packed-c": (6, 5, 2, 5, dict(**CLUSTERED), 0.1, (16, 32)),
}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


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


def desc_of(hipmod, planes, extra=0, flag=True, **kw):
    _, H, W, S = planes.shape
    return hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=SIGMA, flags=(hipmod.MEMBER_TEST_FLAG if flag else 0) | extra, **kw)


def run(c, hipmod, planes, mt, box, extra=0, flag=True, allow_nonfinite=False):
    if mt is not None:
        c.set_membership(member_cfg(hipmod, mt))
    got = c.filter_pass_debug(planes, desc_of(hipmod, planes, extra, flag), box=box, allow_nonfinite=allow_nonfinite)
    cn = c.counters()
    got.update(route=c.route(), launches=cn.filter_kernel_launches, redo_pixels=cn.redo_pixels)
    return got


def classes_of(nbhd):
    return {MR.class_of(int(n)) for n in np.asarray(nbhd).ravel()}


# ---- the anchor: multiples 3 and floors -1 are the reference's test ------------------------------------------------------------
@pytest.mark.parametrize("box", [7, 11])
@pytest.mark.parametrize("flat", [False, True], ids=["smooth", "flat94"])
def test_anchor_reference_multiples_give_the_unflagged_pass(ctx, hipmod, flat, box):
    planes = frame(12, 10, 8, **(dict(flat_frac=0.94) if flat else {}))
    S = 8
    want = run(ctx, hipmod, planes, None, box, flag=False)
    assert want["route"] != 9
    got = run(ctx, hipmod, planes, MR.reference(), box)
    assert got["route"] == 9 and got["status"] == hipmod.OK and got["redo_pixels"] == 0
    for k in BITS:
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
    np.testing.assert_allclose(got["mi"], want["mi"], rtol=0, atol=1e-11)           # check_pass's bars
    for k in ("alpha", "beta", "wrc"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12)
    assert (got["sum_nbhd"], got["max_nbhd"]) == (want["sum_nbhd"], want["max_nbhd"])
    classes = classes_of(got["nbhd_size"])
    assert got["launches"] == len(classes)
    if flat:  # the flat proof under a negative floor: the flat pixels keep N = S, as without the flag
        assert (got["nbhd_size"] == S).mean() >= 0.90
    else:
        assert got["nbhd_size"].min() > S


# ---- stage parity on every pixel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_stage_parity_on_every_pixel(ctx, hipmod, oracle, name):
    W, H, S, box, _, scale, reach = CASES[name]
    planes, mt = planes_of(name), MR.published19(scale)
    want = ref_of(oracle, name)
    classes = classes_of(want["nbhd_size"])
    assert set(reach) <= classes, (reach, sorted(classes))              # the frame reaches the kernels it is here for
    got = run(ctx, hipmod, planes, mt, box)
    print("MEMBER %s: N %d .. %d, classes %s" % (name, want["nbhd_size"].min(), want["nbhd_size"].max(), sorted(classes)))
    assert got["status"] == hipmod.OK and got["route"] == 9 and got["redo_pixels"] == 0
    assert got["launches"] == len(classes)                              # one launch per non-empty class, one for the rest list
    assert np.array_equal(got["nbhd_size"], want["nbhd_size"])
    assert np.array_equal(got["member_hash"], want["member_hash"])
    assert np.array_equal(got["mean"], want["mean"]) and np.array_equal(got["stddev"], want["stddev"])
    np.testing.assert_allclose(got["mi"], want["mi"], rtol=0, atol=1e-11)           # check_pass's bars
    for k in ("alpha", "beta", "wrc"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12)
    assert got["max_nbhd"] == want["nbhd_size"].max() and got["sum_nbhd"] == int(want["nbhd_size"].sum())
    assert np.array_equal(ctx.nbhd(W, H), want["nbhd_size"])
    if name.startswith("rest"):
        assert got["max_nbhd"] > 832 and got["launches"] == len(classes - {833}) + 1
    if name.startswith("packed"):   # the smaller floors reject some candidates, and only packed classes are reached
        assert (want["nbhd_size"] < full_window(W, H, S, box)).any()
        assert classes <= {8, 16, 32, 64} and len(classes) >= 2
    # stage 4: the restatement on the device's own stage outputs, every sample, the direct form's bar
    ref = MR.stage4_on(oracle, planes, got, mt, box, SIGMA, EPS)
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(ref))
    cmax = B.cmax_of(planes[2:5])
    bar = B.sample_bar("direct", 12, int(want["nbhd_size"].max()), SIGMA, box)
    worst = B.worst_sample(got["colour"], ref) / cmax
    print("MEMBER %s stage 4: worst %.3e (bar %.3e)" % (name, worst, bar))
    assert worst <= bar, (worst, bar)
    assert np.abs(got["colour"] - want["colour"]).max() <= 1e-4 * cmax              # and the whole restatement, loosely (1e-9 on alpha, beta)


# ---- the flat proof ---------------------------------------------------------------------------------------------------------
def full_window(W, H, S, box):
    b = (box - 1) // 2
    nx = np.minimum(np.arange(W) + b, W - 1) - np.maximum(np.arange(W) - b, 0) + 1
    ny = np.minimum(np.arange(H) + b, H - 1) - np.maximum(np.arange(H) - b, 0) + 1
    return (ny[:, None] * nx[None, :] * S).astype(np.int32)


def test_flat_proof_fires_only_under_a_negative_floor(ctx, hipmod, oracle):
    """zero-variance features everywhere: under preset 1 every candidate is within the floor (N is the full window), under floors
    -1 the strict test rejects them all (N = S)"""
    W, H, S, box = 12, 10, 8, 7
    planes = np.array(frame(W, H, S))
    for k in range(12):
        planes[7 + k] = np.float32(0.125 * (k + 1))
    pub = run(ctx, hipmod, planes, MR.published19(), box, allow_nonfinite=True)
    assert pub["route"] == 9 and np.array_equal(pub["nbhd_size"], full_window(W, H, S, box))
    ref = run(ctx, hipmod, planes, MR.reference(), box, allow_nonfinite=True)
    assert ref["route"] == 9 and (ref["nbhd_size"] == S).all()
    # one zero-variance feature among live ones, its floor alone non-negative: the restatement's lists
    planes = np.array(frame(W, H, S))
    planes[7] = np.float32(0.25)
    mult, floor = MR.published19()
    floor[1:] = -1.0
    want_n, want_codes = MR.counts(oracle, planes, (mult, floor), box)
    got = run(ctx, hipmod, planes, (mult, floor), box, allow_nonfinite=True)
    assert want_n.min() > S and np.array_equal(got["nbhd_size"], want_n)
    assert all(SR.fnv1a_u32(want_codes[(y, x)]) == got["member_hash"][y, x] for y in range(H) for x in range(W))
    floor[0] = -1.0
    assert (run(ctx, hipmod, planes, (mult, floor), box, allow_nonfinite=True)["nbhd_size"] == S).all()


# ---- NaN and infinity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_special_values(ctx, hipmod, oracle, value):
    W, H, S, box = 12, 10, 8, 7
    planes = np.array(frame(W, H, S, flat_frac=0.94))
    planes[7 + 4, 5, 6, 3] = value                                                   # one sample of feature 4 (a world position)
    for mt in (MR.published19(), MR.reference()):
        want_n, want_codes = MR.counts(oracle, planes, mt, box)
        got = run(ctx, hipmod, planes, mt, box, allow_nonfinite=True)
        assert got["route"] == 9
        assert np.array_equal(got["nbhd_size"], want_n)
        assert all(SR.fnv1a_u32(want_codes[(y, x)]) == got["member_hash"][y, x] for y in range(H) for x in range(W))


# ---- other layouts: N, member hash, mean / std ------------------------------------------------------------------------------
LAYOUTS = [(3, 7, True), (4, 18, False)]


@pytest.mark.parametrize("nr,nf,needs_generic", LAYOUTS, ids=["generic-3-7-f16", "compiled-4-18-f16"])
def test_other_layouts(ctx, hipmod, oracle, nr, nf, needs_generic):
    W, H, S, box = 12, 10, 8, 7
    stored = fb.synth_planes(W, H, S, seed=5, n_random=nr, n_feat=nf, dtype="f16", flat_frac=0.5)
    mt = (np.where(np.arange(nf) % 6 >= 3, 30.0, 3.0), np.full(nf, 0.05))
    want = MR.member_pass(oracle, stored.astype(np.float32), mt, box, SIGMA, EPS, n_random=nr, n_feat=nf, weights=False)
    flags = hipmod.MEMBER_TEST_FLAG | (hipmod.FLAG_GENERIC if needs_generic else 0)
    desc = hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=SIGMA, flags=flags, n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16)
    assert hipmod.layout_kernels(desc) == (hipmod.OK, 1 if needs_generic else 0)
    ctx.set_membership(member_cfg(hipmod, mt))
    got = ctx.filter_pass_debug(stored, desc, box=box)
    assert ctx.route() == 9 and got["status"] == hipmod.OK
    assert want["nbhd_size"].max() > 64
    assert np.array_equal(got["nbhd_size"], want["nbhd_size"]) and np.array_equal(got["member_hash"], want["member_hash"])
    assert np.array_equal(got["mean"], want["mean"]) and np.array_equal(got["stddev"], want["stddev"])
    if needs_generic:  # without RPF_FLAG_GENERIC the layout stays refused, flag or no flag
        bad = hipmod.make_desc(W, H, S, policy=EPS, flags=hipmod.MEMBER_TEST_FLAG, n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16)
        with pytest.raises(hipmod.RpfError) as e:
            ctx.filter_pass_debug(stored, bad, box=box)
        assert e.value.status == hipmod.E_UNSUPPORTED


# ---- with the sampled flag: route 8, the draws under the test ---------------------------------------------------------------
@pytest.mark.parametrize("W,H,S,box,D", [(12, 10, 8, 7, 56), (10, 8, 8, 17, 120)], ids=["box7-D56", "box17-D120"])
def test_sampled_pass_applies_the_test_to_its_draws(ctx, hipmod, oracle, W, H, S, box, D):
    planes, mt = frame(W, H, S, flat_frac=0.94), MR.published19()
    want = MR.member_pass(oracle, planes, mt, box, SIGMA, EPS, cfg=(SEED, 0, D))
    ctx.set_sampling(hipmod.make_sampling(SEED, [D]))
    got = run(ctx, hipmod, planes, mt, box, extra=hipmod.SAMPLED_NBHD_FLAG)
    assert got["route"] == 8 and got["status"] == hipmod.OK and got["redo_pixels"] == 0
    assert got["launches"] == len(classes_of(want["nbhd_size"]))
    assert want["nbhd_size"].max() > S
    assert np.array_equal(got["nbhd_size"], want["nbhd_size"]) and np.array_equal(got["member_hash"], want["member_hash"])
    assert np.array_equal(got["mean"], want["mean"]) and np.array_equal(got["stddev"], want["stddev"])
    np.testing.assert_allclose(got["mi"], want["mi"], rtol=0, atol=1e-11)
    for k in ("alpha", "beta", "wrc"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12)
    ref = MR.stage4_on(oracle, planes, got, mt, box, SIGMA, EPS, cfg=(SEED, 0, D))
    cmax = B.cmax_of(planes[2:5])
    assert B.worst_sample(got["colour"], ref) / cmax <= B.sample_bar("direct", 12, int(want["nbhd_size"].max()), SIGMA, box)
    # the member list is a subsequence of the full-box list under the same test
    _, full = MR.counts(oracle, planes, mt, box)
    assert all(SR.is_subsequence(want["codes"][k].tolist(), full[k].tolist()) for k in full)
    # ... and differs from the sampled list under the reference's test (the flat pixels accept nothing there)
    plain = run(ctx, hipmod, planes, None, box, extra=hipmod.SAMPLED_NBHD_FLAG, flag=False)
    assert plain["route"] == 8 and (plain["nbhd_size"] < got["nbhd_size"]).any()


# ---- whole calls ----------------------------------------------------------------------------------------------------------------
def c64_of(c, hipmod, planes, boxes, flags, colour64_in=None):
    _, H, W, S = planes.shape
    desc = hipmod.make_desc(W, H, S, boxes=boxes, policy=EPS, sigma_seed=SIGMA, flags=flags)
    out = c.filter(planes, desc, colour64_in=colour64_in, want_colour64=True)
    assert out[2] == hipmod.OK
    return out[3], c.route(), c.counters()


def test_two_pass_call_equals_two_one_pass_calls(ctx, hipmod):
    planes, F = planes_of("wave"), hipmod.MEMBER_TEST_FLAG
    ctx.set_membership(member_cfg(hipmod, MR.published19()))
    both, route, cn = c64_of(ctx, hipmod, planes, (11, 7), F)
    assert route == 9
    first, _, _ = c64_of(ctx, hipmod, planes, (11,), F)
    second, _, cn2 = c64_of(ctx, hipmod, planes, (7,), F, colour64_in=first)
    assert same_bits(both, second) and not same_bits(both, first)
    assert (cn.sum_nbhd, cn.max_nbhd, cn.redo_pixels) == (cn2.sum_nbhd, cn2.max_nbhd, 0)   # of the last pass
    # the whole-call entry point runs the pass the debug entry runs
    assert same_bits(c64_of(ctx, hipmod, planes, (7,), F)[0], run(ctx, hipmod, planes, None, 7)["colour"])


def need_devices(devices):
    import torch
    if max(devices) >= torch.cuda.device_count():
        pytest.skip("needs %d visible GPUs" % (max(devices) + 1))


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0), (0, 1)])
def test_multi_filter_equals_one_context(ctx, hipmod, devices):
    need_devices(devices)
    planes, cfg = frame(12, 12, 8, seed=3, flat_frac=0.94), member_cfg(hipmod, MR.published19())
    desc = hipmod.make_desc(12, 12, 8, boxes=(7, 7), policy=EPS, sigma_seed=SIGMA, flags=hipmod.MEMBER_TEST_FLAG)
    ctx.set_membership(cfg)
    s1, p1, st1 = ctx.filter(planes, desc)
    c1 = ctx.counters()
    assert ctx.route() == 9 and c1.max_nbhd > 64
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
    desc = hipmod.make_desc(W, H, S, boxes=(7,), policy=EPS, sigma_seed=SIGMA, flags=hipmod.MEMBER_TEST_FLAG)
    ctx.set_membership(cfg)
    one = ctx.filter_film(planes, desc, film)
    assert ctx.route() == 9
    with hipmod.MultiContext(list(devices)) as mc:
        mc.set_membership(cfg)
        two = mc.filter_film(planes, desc, film)
    for a, b in zip(one, two):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the pool's grow path, and the spike pass on top ---------------------------------------------------------------------------
def test_wide_pool_option_forces_the_grow_path_same_bits(ctx, hipmod):
    planes, mt = planes_of("rest"), MR.published19()
    base = run(ctx, hipmod, planes, mt, 11)
    with hipmod.Context(0) as c:
        c.set_option("wide_pool", 1)
        got = run(c, hipmod, planes, mt, 11)
        assert c.counters().options_active == 1
    assert got["route"] == 9 and got["launches"] == base["launches"]
    for k in BITS + ("mi", "alpha", "beta", "wrc", "colour"):
        assert np.array_equal(got[k].view(np.uint8), base[k].view(np.uint8)), k


def test_spike_pass_on_top(ctx, hipmod):
    planes = np.array(planes_of("wave-c"))
    hit = np.random.default_rng(7).random(planes.shape[1:]) < 0.04
    planes[2:5, hit] *= np.float32(1e3)                                              # fireflies
    F = hipmod.MEMBER_TEST_FLAG
    ctx.set_membership(member_cfg(hipmod, MR.published19()))
    plain, route, _ = c64_of(ctx, hipmod, planes, (7,), F)
    ctx.set_spike(1.0, True)
    spiked, route2, _ = c64_of(ctx, hipmod, planes, (7,), F | hipmod.FLAG_SPIKE_CLAMP)
    st = ctx.spike_stats()
    want = spike_ref.apply(plain, 1.0, True)
    assert route == route2 == 9 and st.applied == 1 and st.spike_samples == want["spike_samples"] > 0
    assert same_bits(spiked, want["colour"])


# ---- refusals, from every device entry point, before any device work ----------------------------------------------------------
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
    F, G = hipmod.MEMBER_TEST_FLAG, hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED

    def desc(flags, policy=EPS, S=S):
        return hipmod.make_desc(W, H, S, boxes=(7,), policy=policy, flags=flags)
    with hipmod.Context(0) as c, hipmod.MultiContext([0, 0]) as mc:
        calls = entry_points(c, mc, hipmod, planes, (7,))

        def refused(d, status, word, only=None):
            for name, call in calls.items():
                if only and name not in only:
                    continue
                with pytest.raises(hipmod.RpfError) as e:
                    call(d)
                assert e.value.status == status and word in str(e.value), (name, str(e.value))
        refused(desc(F), hipmod.E_BADARG, "rpf_set_membership")                      # no configuration set
        m0, s0 = c.pixel_stats(planes, desc(F))                                      # ... which an entry point that runs no pass does not ask for
        m1, s1 = c.pixel_stats(planes, desc(0))
        assert np.array_equal(m0, m1) and np.array_equal(s0, s1, equal_nan=True)
        good = hipmod.membership_preset(hipmod.MEMBERSHIP_PUBLISHED_19)
        for k, field, bad in [(0, "mult", 0.0), (3, "mult", -3.0), (11, "mult", np.inf), (5, "mult", np.nan), (39, "mult", 0.0),
                              (2, "floor", np.nan), (7, "floor", np.inf), (39, "floor", np.nan)]:
            cfg = hipmod.membership_preset(hipmod.MEMBERSHIP_PUBLISHED_19)
            getattr(cfg, field)[k] = bad
            for m in (c, mc):
                with pytest.raises(hipmod.RpfError) as e:
                    m.set_membership(cfg)
                assert e.value.status == hipmod.E_BADARG, (k, field, bad)
        for m in (c, mc):
            with pytest.raises(hipmod.RpfError):
                m.set_membership(None)
        refused(desc(F), hipmod.E_BADARG, "rpf_set_membership")                      # a refused configuration is no configuration
        ok = hipmod.membership_preset(hipmod.MEMBERSHIP_PUBLISHED_19)
        ok.floor[2] = -np.inf                                                        # a floor of -inf is a floor below every sigma
        for m in (c, mc):
            m.set_membership(ok)
            m.set_membership(good)
        refused(desc(F, REF_ABORT), hipmod.E_UNSUPPORTED, "REF_ABORT")
        refused(desc(F | hipmod.FLAG_FAST_WEIGHTS), hipmod.E_UNSUPPORTED, "FAST_WEIGHTS")
        refused(desc(F | G | hipmod.FLAG_GENERIC_FAST), hipmod.E_UNSUPPORTED, "GENERIC_FAST")
        refused(desc(F | hipmod.FLAG_GENERIC | hipmod.FLAG_STREAM_FAST), hipmod.E_UNSUPPORTED, "STREAM_FAST")
        # a full-box pass with S > 832: refused on the descriptor alone (the buffers are never looked at), by the entry points whose
        # binding does not check the planes' shape first
        refused(desc(F, S=833), hipmod.E_UNSUPPORTED, "832", only=("rpf_filter_device",))
        # ... and accepted again
        assert c.filter_pass_debug(planes, desc(F), box=7)["status"] == hipmod.OK and c.route() == 9


def test_s_above_832_is_refused_by_every_entry_point(hipmod):
    W, H, S = 2, 2, 833
    planes = fb.synth_planes(W, H, S, seed=11)
    with hipmod.Context(0) as c, hipmod.MultiContext([0, 0]) as mc:
        for m in (c, mc):
            m.set_membership(hipmod.membership_preset(0))
        for name, call in entry_points(c, mc, hipmod, planes, (3,)).items():
            with pytest.raises(hipmod.RpfError) as e:
                call(hipmod.make_desc(W, H, S, boxes=(3,), policy=EPS, flags=hipmod.MEMBER_TEST_FLAG))
            assert e.value.status == hipmod.E_UNSUPPORTED and "832" in str(e.value), (name, str(e.value))


# ---- a call without the flag after a flagged one ----------------------------------------------------------------------------
def test_unflagged_call_after_a_flagged_one_is_a_fresh_context(ctx, hipmod):
    planes = planes_of("wave")
    with hipmod.Context(0) as fresh:
        want = run(fresh, hipmod, planes, None, 7, flag=False)
    flagged = run(ctx, hipmod, planes, MR.published19(), 7)
    got = run(ctx, hipmod, planes, None, 7, flag=False)
    assert flagged["route"] == 9 and got["route"] == want["route"] != 9
    assert (got["launches"], got["redo_pixels"]) == (want["launches"], want["redo_pixels"])
    for k in BITS + ("mi", "alpha", "beta", "wrc", "colour"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
    assert (flagged["nbhd_size"] > got["nbhd_size"]).any()
