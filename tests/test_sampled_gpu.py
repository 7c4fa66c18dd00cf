"""GPU tests of sampled neighbourhoods (RPF_FLAG_SAMPLED_NBHD, rpf_query_route 8) against the numpy
restatement tests/sampled_ref.py, on every pixel of every frame: stage parity per size class, the other layouts, the subset
property, determinism and keys, mixed calls, slabs, the pool's grow path, the spike pass on top, and the refusals of every
device entry point.  EPS policy throughout (a sampled pass under REF_ABORT is refused)."""
import functools

import numpy as np
import pytest

import sampled_ref as SR
import spike_ref
import stage4_bars as B
from raytracer_rpf_amd import feature_buffer as fb

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
SEED = 0x5EED5EED
SIGMA = 0.5                      # an active sigma seed: the filter moves the colours
CAPS = (8, 16, 32, 64, 128, 256, 448, 832)

# name: W, H, S, box, D, generator mode, the size classes (capacities) the frame must reach, extra flags
CASES = {
    "packed32": (12, 10, 8, 7, 24, "smooth", (32,), 0),
    "packed32c": (12, 10, 8, 7, 24, "clustered", (16,), 0),
    "edge64": (12, 10, 8, 7, 56, "smooth", (64,), 0),
    "wave128": (10, 8, 8, 17, 120, "smooth", (128,), 0),
    # S + D = 832, the cap.  The 832 class itself is out of this frame's reach: sigma = 55 / 4 sends all but a few per cent of the
    # draws outside an 8 x 6 buffer, where they are discarded (N stays below 128); "big832" below reaches it
    "wave832": (8, 6, 32, 55, 800, "smooth", (128,), "wide"),
    "big832": (14, 12, 32, 17, 800, "iid", (448, 832), 0),
    "dups": (6, 5, 4, 7, 200, "smooth", (64,), 0),
    "dupsc": (6, 5, 4, 7, 200, "clustered", (128,), 0),
}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def class_of(n):
    return next(c for c in CAPS if n <= c)


@functools.lru_cache(maxsize=None)
def planes_of(name):
    W, H, S, _, _, mode, _, _ = CASES[name]
    if mode == "iid":  # the smooth frame with its features replaced by unit normals, the same law in every pixel: most draws pass
        p = fb.synth_planes(W, H, S, seed=11)
        p[7:] = np.random.default_rng(11).standard_normal(p[7:].shape).astype(np.float32)
    else:
        p = fb.synth_planes(W, H, S, seed=11, mode=mode, **(dict(sigma_f=1e-3, sigma_c=0.01) if mode == "clustered" else {}))
    p.setflags(write=False)
    return p


_refs = {}


def ref_of(oracle, name, seed=SEED, pass_id=0):
    """the restatement of the case's pass: computed once, shared, never modified"""
    key = (name, seed, pass_id)
    if key not in _refs:
        _, _, _, box, D, _, _, _ = CASES[name]
        _refs[key] = SR.sampled_pass(oracle, planes_of(name), (seed, 0, D), pass_id, box, SIGMA, EPS)
    return _refs[key]


def desc_of(hipmod, name, extra=0, **kw):
    W, H, S, _, _, _, _, wide = CASES[name]
    flags = hipmod.SAMPLED_NBHD_FLAG | (hipmod.FLAG_WIDE_NBHD if wide else 0) | extra
    return hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=SIGMA, flags=flags, **kw)


def run(c, hipmod, name, seed=SEED, pass_id0=0, extra=0, colour_in=None):
    _, _, _, box, D, _, _, _ = CASES[name]
    c.set_sampling(hipmod.make_sampling(seed, [D], pass_id0=pass_id0))
    got = c.filter_pass_debug(planes_of(name), desc_of(hipmod, name, extra), box=box, colour_in=colour_in)
    cn = c.counters()
    got.update(route=c.route(), launches=cn.filter_kernel_launches, redo_pixels=cn.redo_pixels)
    return got


# ---- stage parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_stage_parity_on_every_pixel(ctx, hipmod, oracle, name):
    W, H, S, box, D, _, reach, _ = CASES[name]
    want = ref_of(oracle, name)
    classes = {class_of(int(n)) for n in want["nbhd_size"].ravel()}
    assert set(reach) <= classes, (reach, sorted(classes))              # the frame reaches the class kernels it is here for
    got = run(ctx, hipmod, name)
    print("SAMPLED %s: N %d .. %d, classes %s" % (name, want["nbhd_size"].min(), want["nbhd_size"].max(), sorted(classes)))
    assert got["status"] == hipmod.OK and got["route"] == 8 and got["redo_pixels"] == 0
    assert got["launches"] == len(classes)                              # one launch per non-empty class, no rest, no redo
    assert np.array_equal(got["nbhd_size"], want["nbhd_size"])
    assert np.array_equal(got["member_hash"], want["member_hash"])
    assert np.array_equal(got["mean"], want["mean"]) and np.array_equal(got["stddev"], want["stddev"])
    np.testing.assert_allclose(got["mi"], want["mi"], rtol=0, atol=1e-11)           # check_pass's bars
    for k in ("alpha", "beta", "wrc"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12)
    assert got["max_nbhd"] == want["nbhd_size"].max() <= 832 and got["sum_nbhd"] == int(want["nbhd_size"].sum())
    assert np.array_equal(ctx.nbhd(W, H), want["nbhd_size"])
    # stage 4: the restatement on the device's own stage outputs, every sample, the direct form's bar
    ref = SR.stage4_on(oracle, planes_of(name), got, (SEED, 0, D), 0, box, SIGMA, EPS)
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(ref))
    cmax = B.cmax_of(planes_of(name)[2:5])
    bar = B.sample_bar("direct", 12, int(want["nbhd_size"].max()), SIGMA, box)
    worst = B.worst_sample(got["colour"], ref) / cmax
    print("SAMPLED %s stage 4: worst %.3e (bar %.3e)" % (name, worst, bar))
    assert worst <= bar, (worst, bar)
    assert np.abs(got["colour"] - want["colour"]).max() <= 1e-4 * cmax              # and the whole restatement, loosely (1e-9 on alpha, beta)


# ---- other layouts: N, member hash, mean / std ------------------------------------------------------------------------------
LAYOUTS = [(3, 7, True), (4, 18, False)]


@pytest.mark.parametrize("nr,nf,needs_generic", LAYOUTS, ids=["generic-3-7-f16", "compiled-4-18-f16"])
def test_other_layouts(ctx, hipmod, oracle, nr, nf, needs_generic):
    W, H, S, box, D = 12, 10, 8, 7, 24
    stored = fb.synth_planes(W, H, S, seed=5, n_random=nr, n_feat=nf, dtype="f16")
    want = SR.sampled_pass(oracle, stored.astype(np.float32), (SEED, 0, D), 0, box, SIGMA, EPS, n_random=nr, n_feat=nf, weights=False)
    flags = hipmod.SAMPLED_NBHD_FLAG | (hipmod.FLAG_GENERIC if needs_generic else 0)
    desc = hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=SIGMA, flags=flags, n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16)
    assert hipmod.layout_kernels(desc) == (hipmod.OK, 1 if needs_generic else 0)
    ctx.set_sampling(hipmod.make_sampling(SEED, [D]))
    got = ctx.filter_pass_debug(stored, desc, box=box)
    assert ctx.route() == 8 and got["status"] == hipmod.OK
    assert want["nbhd_size"].max() > S
    assert np.array_equal(got["nbhd_size"], want["nbhd_size"]) and np.array_equal(got["member_hash"], want["member_hash"])
    assert np.array_equal(got["mean"], want["mean"]) and np.array_equal(got["stddev"], want["stddev"])
    if needs_generic:  # without RPF_FLAG_GENERIC the layout stays refused, flag or no flag
        bad = hipmod.make_desc(W, H, S, policy=EPS, flags=hipmod.SAMPLED_NBHD_FLAG, n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16)
        with pytest.raises(hipmod.RpfError) as e:
            ctx.filter_pass_debug(stored, bad, box=box)
        assert e.value.status == hipmod.E_UNSUPPORTED


# ---- the member list is a subsequence of the full-box list ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge64", "packed32c"])
def test_subset_of_the_unsampled_neighbourhood(ctx, hipmod, oracle, name):
    W, H, S, box, D, _, _, _ = CASES[name]
    planes = planes_of(name)
    want = ref_of(oracle, name)
    got = run(ctx, hipmod, name)
    full = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=SIGMA), box=box)
    assert ctx.route() != 8
    assert (got["nbhd_size"] <= full["nbhd_size"]).all() and (got["nbhd_size"] < full["nbhd_size"]).any()
    pmean, pstd = oracle.pixel_stats(planes, oracle.make_desc(W, H, S, policy=EPS))
    for y in range(H):
        for x in range(W):
            codes = SR.full_box_codes(planes, pmean, pstd, y, x, box)
            assert SR.fnv1a_u32(codes) == full["member_hash"][y, x]                 # the device's unsampled list
            assert SR.fnv1a_u32(want["codes"][(y, x)]) == got["member_hash"][y, x]  # the device's sampled list
            assert SR.is_subsequence(want["codes"][(y, x)].tolist(), codes)


# ---- determinism and keys -----------------------------------------------------------------------------------------------------
def test_determinism_seed_and_pass_id(ctx, hipmod, oracle):
    a, b = run(ctx, hipmod, "edge64"), run(ctx, hipmod, "edge64")
    for k in ("nbhd_size", "member_hash", "mean", "stddev", "mi", "alpha", "beta", "wrc", "colour", "bin_hash"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    other_seed, other_pass = run(ctx, hipmod, "edge64", seed=SEED + 1), run(ctx, hipmod, "edge64", pass_id0=1)
    assert (other_seed["member_hash"] != a["member_hash"]).any() and (other_pass["member_hash"] != a["member_hash"]).any()
    assert np.array_equal(other_pass["member_hash"], ref_of(oracle, "edge64", pass_id=1)["member_hash"])
    assert np.array_equal(other_seed["member_hash"], ref_of(oracle, "edge64", seed=SEED + 1)["member_hash"])


def c64_of(c, hipmod, planes, boxes, draws, flags, pass_id0=0, colour64_in=None, seed=SEED):
    _, H, W, S = planes.shape
    if draws is not None:
        c.set_sampling(hipmod.make_sampling(seed, draws, pass_id0=pass_id0))
    desc = hipmod.make_desc(W, H, S, boxes=boxes, policy=EPS, sigma_seed=SIGMA, flags=flags)
    out = c.filter(planes, desc, colour64_in=colour64_in, want_colour64=True)
    assert out[2] == hipmod.OK
    return out[3], c.route(), c.counters()


def test_two_pass_call_equals_two_one_pass_calls(ctx, hipmod):
    planes, F = planes_of("packed32"), hipmod.SAMPLED_NBHD_FLAG
    both, route, cn = c64_of(ctx, hipmod, planes, (7, 7), [24, 24], F)
    assert route == 8
    first, _, _ = c64_of(ctx, hipmod, planes, (7,), [24], F, pass_id0=0)
    # the whole-call entry points run the pass the debug entry runs: rpf_filter_ex's colours are the bits of rpf_filter_pass_debug's,
    # which test_stage_parity_on_every_pixel holds to the restatement
    assert same_bits(first, run(ctx, hipmod, "packed32")["colour"])
    second, _, cn2 = c64_of(ctx, hipmod, planes, (7,), [24], F, pass_id0=1, colour64_in=first)
    assert same_bits(both, second) and not same_bits(both, first)
    assert (cn.sum_nbhd, cn.max_nbhd) == (cn2.sum_nbhd, cn2.max_nbhd)              # of the last pass
    wrong, _, _ = c64_of(ctx, hipmod, planes, (7,), [24], F, pass_id0=0, colour64_in=first)   # the pass id is part of the key
    assert not same_bits(both, wrong)


def test_mixed_call_second_pass_runs_as_without_the_flag(ctx, hipmod):
    planes, F = planes_of("packed32"), hipmod.SAMPLED_NBHD_FLAG
    mixed, route, cn = c64_of(ctx, hipmod, planes, (7, 7), [24, 0], F)
    first, r1, _ = c64_of(ctx, hipmod, planes, (7,), [24], F)
    plain, r2, cn2 = c64_of(ctx, hipmod, planes, (7,), None, 0, colour64_in=first)
    assert r1 == 8 and route == r2 and r2 in (0, 1)
    assert same_bits(mixed, plain)
    assert (cn.sum_nbhd, cn.max_nbhd, cn.redo_pixels) == (cn2.sum_nbhd, cn2.max_nbhd, cn2.redo_pixels)
    # draws all zero: the call is the call without the flag
    zero, r0, _ = c64_of(ctx, hipmod, planes, (7,), [0], F)
    none, r3, _ = c64_of(ctx, hipmod, planes, (7,), None, 0)
    assert r0 == r3 and same_bits(zero, none)


# ---- slabs --------------------------------------------------------------------------------------------------------------------
def need_devices(devices):
    import torch
    if max(devices) >= torch.cuda.device_count():
        pytest.skip("needs %d visible GPUs" % (max(devices) + 1))


@functools.lru_cache(maxsize=None)
def slab_planes():
    p = fb.synth_planes(12, 12, 8, seed=3)
    p.setflags(write=False)
    return p


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0), (0, 1), (0, 1, 0)])
def test_multi_filter_equals_one_context(ctx, hipmod, devices):
    need_devices(devices)
    planes, cfg = slab_planes(), hipmod.make_sampling(SEED, [24, 40], pass_id0=3)
    desc = hipmod.make_desc(12, 12, 8, boxes=(7, 7), policy=EPS, sigma_seed=SIGMA, flags=hipmod.SAMPLED_NBHD_FLAG)
    ctx.set_sampling(cfg)
    s1, p1, st1 = ctx.filter(planes, desc)
    c1 = ctx.counters()
    assert ctx.route() == 8 and c1.max_nbhd > 8
    with hipmod.MultiContext(list(devices)) as mc:
        mc.set_sampling(cfg)
        s2, p2, st2 = mc.filter(planes, desc)
        c2 = mc.counters()
        s3, _, _ = mc.filter(planes, desc)                                           # row_origin does not drift between calls
    assert st1 == st2 == hipmod.OK
    assert np.array_equal(s1.view(np.uint32), s2.view(np.uint32)) and np.array_equal(p1.view(np.uint32), p2.view(np.uint32))
    assert np.array_equal(s2.view(np.uint32), s3.view(np.uint32))
    assert (c2.samples_filtered, c2.sum_nbhd, c2.max_nbhd, c2.redo_pixels) == (c1.samples_filtered, c1.sum_nbhd, c1.max_nbhd, 0)


@pytest.mark.parametrize("devices", [(0, 0), (0, 1)])
def test_multi_filter_film_equals_one_context(ctx, hipmod, devices):
    need_devices(devices)
    planes, cfg = np.array(slab_planes()), hipmod.make_sampling(SEED, [24])
    _, H, W, S = planes.shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    planes[0] = (xx[..., None] + (np.arange(S) + 0.5) / S).astype(np.float32)        # pFilm inside its pixel
    planes[1] = (yy[..., None] + 0.5).astype(np.float32)
    film = hipmod.make_film(((0, 0), (W, H)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX), sample_origin=(0, 0))
    desc = hipmod.make_desc(W, H, S, boxes=(7,), policy=EPS, sigma_seed=SIGMA, flags=hipmod.SAMPLED_NBHD_FLAG)
    ctx.set_sampling(cfg)
    one = ctx.filter_film(planes, desc, film)
    assert ctx.route() == 8
    with hipmod.MultiContext(list(devices)) as mc:
        mc.set_sampling(cfg)
        two = mc.filter_film(planes, desc, film)
    for a, b in zip(one, two):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the pool's grow path, and the spike pass on top -----------------------------------------------------------------------------
def test_wide_pool_option_forces_the_grow_path_same_bits(ctx, hipmod):
    base = run(ctx, hipmod, "wave128")
    with hipmod.Context(0) as c:
        c.set_option("wide_pool", 1)
        got = run(c, hipmod, "wave128")
        assert c.counters().options_active == 1
    assert got["route"] == 8 and got["launches"] == base["launches"]
    for k in ("nbhd_size", "member_hash", "bin_hash", "mean", "stddev", "mi", "alpha", "beta", "wrc", "colour"):
        assert np.array_equal(got[k].view(np.uint8), base[k].view(np.uint8)), k


def test_spike_pass_on_top(ctx, hipmod):
    planes = np.array(planes_of("packed32c"))
    hit = np.random.default_rng(7).random(planes.shape[1:]) < 0.04
    planes[2:5, hit] *= np.float32(1e3)                                              # fireflies
    F = hipmod.SAMPLED_NBHD_FLAG
    plain, route, _ = c64_of(ctx, hipmod, planes, (7,), [24], F)
    ctx.set_spike(1.0, True)
    spiked, route2, _ = c64_of(ctx, hipmod, planes, (7,), [24], F | hipmod.FLAG_SPIKE_CLAMP)
    st = ctx.spike_stats()
    want = spike_ref.apply(plain, 1.0, True)
    assert route == route2 == 8 and st.applied == 1 and st.spike_samples == want["spike_samples"] > 0
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
    planes = planes_of("packed32")
    _, H, W, S = planes.shape
    F, G = hipmod.SAMPLED_NBHD_FLAG, hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED

    def desc(flags, policy=EPS):
        return hipmod.make_desc(W, H, S, boxes=(7,), policy=policy, flags=flags)
    with hipmod.Context(0) as c, hipmod.MultiContext([0, 0]) as mc:
        calls = entry_points(c, mc, hipmod, planes, (7,))

        def refused(d, status, word):
            for name, call in calls.items():
                with pytest.raises(hipmod.RpfError) as e:
                    call(d)
                assert e.value.status == status and word in str(e.value), (name, str(e.value))
        refused(desc(F), hipmod.E_BADARG, "rpf_set_sampling")                        # no configuration set
        m0, s0 = c.pixel_stats(planes, desc(F))                                      # ... which an entry point that runs no pass does not ask for
        m1, s1 = c.pixel_stats(planes, desc(0))
        assert np.array_equal(m0, m1) and np.array_equal(s0, s1, equal_nan=True)
        for m in (c, mc):
            with pytest.raises(hipmod.RpfError) as e:
                m.set_sampling(hipmod.make_sampling(1, [24, -1]))                    # a negative draw count
            assert e.value.status == hipmod.E_BADARG
            with pytest.raises(hipmod.RpfError):
                m.set_sampling(None)
        refused(desc(F), hipmod.E_BADARG, "rpf_set_sampling")                        # a refused configuration is no configuration
        for m in (c, mc):
            m.set_sampling(hipmod.make_sampling(1, [832 - S + 1]))
        refused(desc(F), hipmod.E_BADARG, "832")                                     # S + D = 833
        for m in (c, mc):
            m.set_sampling(hipmod.make_sampling(1, [24]))
        refused(desc(F, REF_ABORT), hipmod.E_UNSUPPORTED, "REF_ABORT")
        refused(desc(F | hipmod.FLAG_FAST_WEIGHTS), hipmod.E_UNSUPPORTED, "FAST_WEIGHTS")
        refused(desc(F | G | hipmod.FLAG_GENERIC_FAST), hipmod.E_UNSUPPORTED, "GENERIC_FAST")
        refused(desc(F | hipmod.FLAG_GENERIC | hipmod.FLAG_STREAM_FAST), hipmod.E_UNSUPPORTED, "STREAM_FAST")
        # draws == 0 under REF_ABORT is no sampled pass: accepted, and it runs as without the flag
        for m in (c, mc):
            m.set_sampling(hipmod.make_sampling(1, [0]))
        got = c.filter_pass_debug(planes, desc(F, REF_ABORT), box=7, allow_nonfinite=True)
        assert c.route() in (0, 1) and got["status"] in (hipmod.OK, hipmod.E_NONFINITE)
        # ... and S + D = 832 is accepted
        c.set_sampling(hipmod.make_sampling(1, [832 - S]))
        assert c.filter_pass_debug(planes, desc(F), box=7)["status"] == hipmod.OK and c.route() == 8
