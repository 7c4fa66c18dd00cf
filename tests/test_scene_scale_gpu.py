"""Every kernel family against the oracle at scene-scale magnitudes (tests/scene_scale.py; the frames and what they reach are
asserted on the CPU by tests/test_scene_scale_cpu.py): offset, small-spread features, where the variance E[x^2] - mean^2
cancels and its residue bits decide the 3 sigma membership, every bin id, the flat-quad proof and which REF_ABORT pixel is NaN.
The kernels promise the reference's bits there by issuing the sum and sum-of-squares chains in reference order; this module
holds each body that has such a chain to that promise.

No bar is new.  Every pass goes through rpf_filter_pass_debug and assert_parity: status, nonfinite_pixels, first_bad_pixel and
the NaN pattern of the colours are the oracle's; where the oracle's colours are all finite, check_pass (bit-equal N, member
hash, bin hash, mean and SD, MI within 1e-11, alpha, beta and W_r_c at rtol 1e-9, colours within 1e-4); where they are not,
the same bars with NaN equal to NaN and the colours compared where the oracle's are finite.  Route options are held to bit-equal
stage outputs against the default run, the fp32 pair-weight modes to g <= 16 e32 + 1e-12, stage 4 to the per-sample bars of
tests/stage4_bars.py with the z^2 bound measured on the oracle.  Both policies everywhere.

Measured on the MI355X: every case passes; g / e32 = 0.92 (FAST_WEIGHTS), 0.93 (GENERIC_FAST, STREAM_FAST) at e32 = 6.5e-9;
stage 4 worst sample 3.3e-16 on the fused and packed kernels (bars 1.1e-7 at seed 0.002, 2.3e-11 at 0.5) and 4.2e-16 on route
3 (bar 6.8e-12); rpf_filter over (7, 5) 2.3e-16 from the oracle's two passes.  DESIGN.md section 5 has the planted faults."""
import numpy as np
import pytest

import fast_weights_ref as R
import stage4_bars as B
from test_generic_wave_gpu import desc_for as generic_desc
from test_gpu_parity import REL_L2_BAR, SAME_BITS, STAGE_KEYS, _run_opts, check_pass, rel_l2
from test_scene_scale_cpu import ACTIVE, L19, STAGE4, Z2MAX, all_pixels, geometry, layout, planes, want_of
from test_wide_classes_gpu import desc_of as wide_desc, forced  # noqa: F401  (forced: a fixture)

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
POLICIES = pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
REGRESSION_FACTOR = 16


def fused_desc(hipmod, name, policy, **kw):
    nr, nf, dt = layout(name)
    W, H, S, _ = geometry(name)
    lay = dict(n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16) if dt == "f16" else {}
    assert dt == "f16" or (nr, nf) == (2, 12)
    return hipmod.make_desc(W, H, S, policy=policy, **lay, **kw)


def assert_parity(got, want, hipmod):
    """the oracle's status, counts and NaN pattern; check_pass, with NaN equal to NaN where the oracle leaves pixels non-finite"""
    assert (got["status"] == hipmod.E_NONFINITE) == (want["status"] == 1)
    assert got["nonfinite_pixels"] == want["nonfinite_pixels"] and got["first_bad_pixel"] == want["first_bad_pixel"]
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(want["colour"]))
    assert got["sum_nbhd"] == want["sum_nbhd"] and got["max_nbhd"] == want["max_nbhd"]
    if np.isfinite(want["colour"]).all():
        return check_pass(got, want)
    for k in ("nbhd_size", "member_hash", "bin_hash"):
        assert (got[k] == want[k]).all(), k
    for k in ("mean", "stddev"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    np.testing.assert_allclose(got["mi"], want["mi"], rtol=0, atol=1e-11, equal_nan=True)
    for k in ("alpha", "beta", "wrc"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-12, equal_nan=True)
    fin = np.isfinite(want["colour"])
    r = rel_l2(got["colour"][fin], want["colour"][fin])
    assert r <= REL_L2_BAR, r
    return r


def assert_same_stages(got, base, same_colour_bits):
    for k in STAGE_KEYS:
        assert np.array_equal(got[k], base[k], equal_nan=True), k
    assert got["status"] == base["status"] and got["nonfinite_pixels"] == base["nonfinite_pixels"]
    assert got["first_bad_pixel"] == base["first_bad_pixel"]
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(base["colour"]))
    if same_colour_bits:
        assert np.array_equal(got["colour"], base["colour"], equal_nan=True)
    else:       # another kernel sums the weights of a pixel: same terms, possibly in another order
        m = np.isfinite(base["colour"])
        np.testing.assert_allclose(got["colour"][m], base["colour"][m], rtol=1e-12, atol=1e-300)


_base = {}


def base_run(hipmod, name, policy, seed=0.002):
    """the pass of a fused-route frame with no option set, on a fresh context: run once per session, shared, never modified"""
    key = (name, policy, seed)
    if key not in _base:
        _, _, _, box = geometry(name)
        _base[key] = _run_opts(hipmod, planes(name)[0], fused_desc(hipmod, name, policy, sigma_seed=seed), box)
    return _base[key]


# ---- the fused routes -------------------------------------------------------------------------------------------------------------
# 12 x 9 x 8, box 7: the fused K = 7 kernel (clu2e4, farn, hdr, the controls: N = 72 ... 392), the packed kernels behind the flat
# proof (smo1e3: N = S everywhere) and both together (mix2e3: N = 8 ... 303)
SMALL = ["clu2e4", "smo1e3", "mix2e3", "farn", "hdr", "ctl1e2", "negbig"]
SMALL_OPTIONS = [("packed", 0), ("packed", 1), ("count_first", 0), ("count_first", 1)]


@POLICIES
@pytest.mark.parametrize("name", SMALL)
def test_fused_packed_and_count_first(hipmod, oracle, name, policy):
    """packed 0 / 1 and count_first -1 (the probe: the default run) / 0 / 1: each against the oracle, and bit-identical stage
    outputs between the routes"""
    want = want_of(oracle, name, policy)
    base = base_run(hipmod, name, policy)
    assert base["route"] in (0, 1) and base["options_active"] == 0
    assert_parity(base, want, hipmod)
    _, _, _, box = geometry(name)
    for option, value in SMALL_OPTIONS:
        got = _run_opts(hipmod, planes(name)[0], fused_desc(hipmod, name, policy), box, [(option, value)])
        assert got["options_active"] == 1 and got["route"] == (value if option == "count_first" else got["route"])
        assert_parity(got, want, hipmod)
        assert_same_stages(got, base, option in SAME_BITS)


@POLICIES
@pytest.mark.parametrize("name", ["k13", "b13s3", "s12", "s72", "stream", "half8", "half16"])
def test_other_fused_classes(ctx, hipmod, oracle, name, policy):
    """one-wave K = 13 (16 spp), the unbinned hand-over of box 13 x 3 spp, S no power of two (12 spp at box 5; 72 spp, where
    the stage-1a SD itself is NaN), the streaming kernel (N > 3136), the 27-dim fp16 kernels at 8 and 16 spp"""
    W, H, S, box = geometry(name)
    want = want_of(oracle, name, policy)
    got = ctx.filter_pass_debug(planes(name)[0], fused_desc(hipmod, name, policy), box=box, allow_nonfinite=True)
    assert ctx.route() in ((2,) if box * box * S > 512 else (0, 1))
    assert_parity(got, want, hipmod)
    if name == "stream":
        assert got["max_nbhd"] > B.RESIDENT


BINNED_OPTIONS = [("split_weights", 0), ("split_weights", 1), ("waves_per_pixel", 1), ("waves_per_pixel", 4)]


@POLICIES
@pytest.mark.parametrize("name", ["s32", "s64"])
def test_size_binned_four_wave_and_split(hipmod, oracle, name, policy):
    """12 x 9 x 32 and 10 x 8 x 64 at box 7: the size-binned classes up to K = 25 / K = 49, one launch or the three-launch
    split, one wave or four per pixel"""
    want = want_of(oracle, name, policy)
    base = base_run(hipmod, name, policy)
    assert base["route"] == 2
    assert_parity(base, want, hipmod)
    _, _, _, box = geometry(name)
    for option, value in BINNED_OPTIONS:
        got = _run_opts(hipmod, planes(name)[0], fused_desc(hipmod, name, policy), box, [(option, value)])
        assert got["options_active"] == 1 and got["route"] == 2
        assert_parity(got, want, hipmod)
        assert_same_stages(got, base, option in SAME_BITS)


# ---- the flat proof reached through fp32 quantisation -------------------------------------------------------------------------
@POLICIES
def test_flat_shortcut_by_quantisation(hipmod, oracle, policy):
    """smo1e3: no pixel was planted flat, and stage 1a proves every one of them flat from SDs that are exactly 0.  The prelist
    then leaves nothing for the fused kernel: the launches of the pass are the four packed ones (and the redo launch under
    REF_ABORT) -- no fused launch.  N = S = 8 is a power of two, where the reference's MI of an independent table is an exact 0:
    no pixel goes on the redo list."""
    W, H, S, box = geometry("smo1e3")
    want = want_of(oracle, "smo1e3", policy)
    with hipmod.Context(0) as c:
        got = c.filter_pass_debug(planes("smo1e3")[0], fused_desc(hipmod, "smo1e3", policy), box=box, allow_nonfinite=True)
        cnt, route, nbhd = c.counters(), c.route(), c.nbhd(W, H)
    assert route in (0, 1) and cnt.options_active == 0
    assert cnt.filter_kernel_launches == 4 + (1 if policy == REF_ABORT else 0)
    assert cnt.redo_pixels == 0
    assert np.array_equal(nbhd, want["nbhd_size"]) and (nbhd == S).all()
    assert cnt.sum_nbhd == W * H * S and cnt.max_nbhd == S
    assert_parity(got, want, hipmod)


# ---- the generic routes ---------------------------------------------------------------------------------------------------------
@POLICIES
@pytest.mark.parametrize("route", [3, 4, 5])
@pytest.mark.parametrize("name", ["g37", "g37k13", "half8", "clu2e4", "smo1e3"])
def test_generic_routes(ctx, hipmod, oracle, name, route, policy):
    """routes 3, 4, 5 on the generic layouts (3, 7) fp32 and (4, 18) fp16 and on the reference's layout: the streaming kernel,
    the generic packed kernels (smo1e3, half8: N <= 64) and the generic one-wave kernels (N = 72 ... 784)"""
    W, H, S, box = geometry(name)
    want = want_of(oracle, name, policy)
    got = ctx.filter_pass_debug(planes(name)[0], generic_desc(hipmod, layout(name), W, H, S, route=route, policy=policy), box=box,
                                allow_nonfinite=True)
    assert ctx.route() == route
    assert_parity(got, want, hipmod)


@POLICIES
@pytest.mark.parametrize("route", [6, 7])
@pytest.mark.parametrize("name", ["clu2e4", "smo1e3", "half8"])
def test_wide_routes_forced(forced, hipmod, oracle, name, route, policy):  # noqa: F811
    """small frames forced onto the wide kernels (option "wide"), with and without the size classes"""
    W, H, S, box = geometry(name)
    want = want_of(oracle, name, policy)
    got = forced.filter_pass_debug(planes(name)[0], wide_desc(hipmod, layout(name), W, H, S, policy, classes=route == 7), box=box,
                                   allow_nonfinite=True)
    assert forced.route() == route
    assert_parity(got, want, hipmod)


# ---- the host entries, on a degenerate EPS frame ----------------------------------------------------------------------------------
def test_host_entries(ctx, hipmod, oracle):
    """rpf_filter over boxes (7, 5) against the oracle's two passes; a row slab with its halo, and two slab contexts, equal to
    the one full-frame call bit for bit"""
    name = "clu2e4"
    W, H, S, _ = geometry(name)
    stored, p32 = planes(name)
    desc = hipmod.make_desc(W, H, S, boxes=(7, 5), policy=EPS)
    s1, p1, st, c64 = ctx.filter(stored, desc, want_colour64=True)
    assert st == hipmod.OK
    c = None
    for box in (7, 5):
        c = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=box, policy=EPS), colour_in=c, debug=False)["colour"]
    r = rel_l2(c64, c)
    print("rpf_filter (7, 5) on %s: rel-L2 against the oracle's two passes %.3e" % (name, r))
    assert r <= REL_L2_BAR, r
    with hipmod.MultiContext([0, 0]) as mc:
        s2, p2, st2 = mc.filter(stored, desc)
    assert st2 == hipmod.OK and np.array_equal(s1, s2) and np.array_equal(p1, p2)
    # rows [3, 6) of the frame as a slab with three halo rows either side
    b, a0, a1 = 3, 3, 6
    full = ctx.filter_pass_debug(stored, hipmod.make_desc(W, H, S, policy=EPS), box=7)
    part = ctx.filter_pass_debug(np.ascontiguousarray(stored[:, a0 - b:a1 + b]),
                                 hipmod.make_desc(W, a1 - a0 + 2 * b, S, row_begin=b, row_end=b + a1 - a0, policy=EPS), box=7)
    for k in STAGE_KEYS:
        assert np.array_equal(part[k][b:b + a1 - a0], full[k][a0:a1], equal_nan=True), k
    assert np.array_equal(part["colour"][:, b:b + a1 - a0], full["colour"][:, a0:a1])
    assert np.array_equal(part["colour"][:, :b], stored[2:5, a0 - b:a0].astype(np.float64))      # the halo passes through


# ---- the fp32 pair-weight modes -------------------------------------------------------------------------------------------------
FAST = ["fast_weights", "generic_fast", "stream_fast"]


@pytest.mark.parametrize("mode", FAST)
def test_fp32_pair_weight_modes(ctx, hipmod, oracle, mode):
    """RPF_FLAG_FAST_WEIGHTS (the fused route), RPF_FLAG_GENERIC_FAST (route 5) and RPF_FLAG_STREAM_FAST (route 3) on clu2e4 at
    the active seed under EPS: g, the device's distance from the oracle under the flag, within 16 times e32, that of the numpy
    restatement of the documented fp32 arithmetic on the same frame; every stage output the bits of the run without the flag"""
    name, policy, seed = "clu2e4", EPS, ACTIVE
    W, H, S, box = geometry(name)
    stored, p32 = planes(name)
    want = want_of(oracle, name, policy, seed)
    if mode == "fast_weights":
        flags, route = hipmod.FLAG_FAST_WEIGHTS, None
        mk = lambda f: hipmod.make_desc(W, H, S, policy=policy, sigma_seed=seed, flags=f)     # noqa: E731
    else:
        flags, route = (hipmod.FLAG_GENERIC_FAST, 5) if mode == "generic_fast" else (hipmod.FLAG_STREAM_FAST, 3)
        mk = lambda f: generic_desc(hipmod, L19, W, H, S, route=route, policy=policy, sigma_seed=seed, flags=f)   # noqa: E731
    ref = ctx.filter_pass_debug(stored, mk(0), box=box)
    r_ref = ctx.route()
    got = ctx.filter_pass_debug(stored, mk(flags), box=box)
    assert ctx.route() == r_ref and (route is None or r_ref == route)
    assert_parity(ref, want, hipmod)
    for k in STAGE_KEYS:
        assert got[k].tobytes() == ref[k].tobytes(), k
    assert np.isfinite(got["colour"]).all()
    g = rel_l2(got["colour"], want["colour"])
    y32 = R.stage4(oracle, p32, want, box, seed, all_pixels(name), np.float32, policy).reshape(3, H, W, S)
    e32 = rel_l2(y32, want["colour"])
    d = rel_l2(got["colour"], ref["colour"])
    print("FAST %s on %s seed %g: g = %.3e  e32 = %.3e  g / e32 = %.2f  (fp32 run against fp64 run %.3e)" % (mode, name, seed, g, e32, g / e32, d))
    assert e32 > 0 and g <= REGRESSION_FACTOR * e32 + 1e-12, (g, e32)
    assert d > 1e-10, d                                                    # the flag did switch the pair arithmetic


# ---- stage 4, sample by sample ---------------------------------------------------------------------------------------------------
# the fused K = 7 kernel (clu2e4: N = 72 ... 392; smo1e3 with the packed kernels off: N = 8 on one wave per pixel), the packed
# fused kernel (smo1e3 by default), one generic direct body (route 3: generic::filter_pixel_kernel)
STAGE4_KERNELS = ["default", "packed0", "route3"]


@pytest.mark.parametrize("kernel", STAGE4_KERNELS)
@pytest.mark.parametrize("name,seed", STAGE4, ids=[s[0] for s in STAGE4])
def test_stage4_per_sample(hipmod, oracle, name, seed, kernel):
    """the device's colours against the fp64 restatement evaluated on the device's OWN stage outputs, on every sample: the bar of
    the form the kernel uses -- expanded (with the z^2 bound measured on the oracle, Z2MAX) on the fused routes, direct on
    route 3.  A kernel beyond its bar is a finding; the bar does not move."""
    W, H, S, box = geometry(name)
    stored, p32 = planes(name)
    want = want_of(oracle, name, EPS, seed)
    if kernel == "route3":
        desc, opts, routes = generic_desc(hipmod, L19, W, H, S, route=3, policy=EPS, sigma_seed=seed), [], (3,)
    else:
        desc, opts, routes = fused_desc(hipmod, name, EPS, sigma_seed=seed), ([("packed", 0)] if kernel == "packed0" else []), (0, 1)
    got = _run_opts(hipmod, stored, desc, box, opts)
    assert got["route"] in routes
    assert_parity(got, want, hipmod)
    ref = R.stage4(oracle, p32, got, box, seed, all_pixels(name), np.float64, EPS).reshape(3, H, W, S)
    cin = p32[2:5].astype(np.float64)
    cmax = B.cmax_of(cin)
    nmax = int(got["nbhd_size"].max())
    bar = B.sample_bar(B.ROUTE_FORM[got["route"]], 12, nmax, seed, box, z2max=Z2MAX[name])
    assert np.isfinite(got["colour"]).all() and np.isfinite(ref).all()
    worst = float(np.abs(got["colour"] - ref).max()) / cmax
    print("STAGE4 %s %s route %d: worst %.3e (bar %.3e, %s form, z2max %g), moved %.3f" % (
        name, kernel, got["route"], worst, bar, B.ROUTE_FORM[got["route"]], Z2MAX[name], rel_l2(got["colour"], cin)))
    assert rel_l2(got["colour"], cin) >= 0.05
    assert worst <= bar, (worst, bar)
