"""GPU parity at every kernel-class edge: the frames of tests/planted_nbhd.py put pixels with N = capacity and N = capacity + 1
of every neighbourhood-size class (8, 16, 32, 64 packed | 128, 256, 448, 832, 1600, 3136 LDS-resident | streaming) in front
of every route that can take them.  The classifier and the kernels compare N with the same constants from different source
files; a pixel at capacity fills its kernel's member list, histograms and samples-per-lane to the last slot (and, where the
capacity is a perfect square, B = floor(sqrt(N)) reaches the class maximum as well), a pixel one above must be filed one
class up.  tests/test_planted_nbhd_cpu.py proves on the CPU that the oracle sees the planted sizes.

Every case runs twice: with the reference's sigma seed, at which the filter is the identity on these frames (white-noise
colours: every weight but a sample's own underflows; the discrete outputs, MI, alpha, beta and W_r_c are what is compared
for real), and with planted_nbhd.ACTIVE_SIGMA_SEED, at which the weights are of order one and the colours move by 6 ... 40 %,
so that a member dropped from a weight sum, or a stale slot added to it, shows in the colours as well.

Bars: check_pass and the route-agreement bars of tests/test_gpu_parity.py, unchanged; no tolerance of its own."""
import numpy as np
import pytest

import planted_nbhd as P
from test_gpu_parity import REL_L2_BAR, STAGE_KEYS, check_pass, rel_l2

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
SEEDS = pytest.mark.parametrize("seed", [0.002, P.ACTIVE_SIGMA_SEED], ids=["ref_seed", "active_seed"])
POLICIES = pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
UNBINNED = [f for f, v in P.FRAMES.items() if not v[5]]
BINNED = [f for f, v in P.FRAMES.items() if v[5]]


def geometry(fid):
    """W, H, S, box of a frame"""
    _, S, box, targets, _, _ = P.FRAMES[fid]
    return box * len(targets), box, S, box


def hip_desc(hipmod, fid, policy, **kw):
    nr, nf, dt = P.FRAMES[fid][0]
    W, H, S, _ = geometry(fid)
    lay = dict(n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16) if dt == "f16" else {}
    return hipmod.make_desc(W, H, S, policy=policy, **lay, **kw)


def run(c, hipmod, fid, policy, seed, **kw):
    got = c.filter_pass_debug(P.frame(fid)[0], hip_desc(hipmod, fid, policy, sigma_seed=seed, **kw), box=geometry(fid)[3],
                              allow_nonfinite=True)
    got["route"] = c.route()
    got["redo_pixels"] = c.counters().redo_pixels
    return got


_base = {}


def base(ctx, hipmod, fid, policy, seed):
    """the default-options pass of a frame (what (a) checks against the oracle): run once, shared, never modified"""
    if (fid, policy, seed) not in _base:
        _base[fid, policy, seed] = run(ctx, hipmod, fid, policy, seed)
    return _base[fid, policy, seed]


def moved(oracle, fid, seed):
    """how far the oracle's pass moves the colours of a frame (relative L2, EPS policy)"""
    cin = P.frame(fid)[1][2:5].astype(np.float64)
    return rel_l2(P.oracle_pass(oracle, fid, EPS, seed)["colour"], cin)


def assert_oracle_parity(got, want, hipmod, fid):
    """check_pass on the whole frame where the oracle's colours are finite; where a pixel is NaN (REF_ABORT) the same status,
    NaN pattern, counters and bit-equal discrete outputs; and the PLANTED sizes at the targets"""
    _, _, pixels, targets = P.frame(fid)
    for (y, x), n in zip(pixels, targets):
        assert got["nbhd_size"][y, x] == n, (fid, (y, x), n, int(got["nbhd_size"][y, x]))
    assert (got["status"] == hipmod.E_NONFINITE) == (want["status"] == 1)
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(want["colour"]))
    assert got["nonfinite_pixels"] == want["nonfinite_pixels"] and got["first_bad_pixel"] == want["first_bad_pixel"]
    assert got["max_nbhd"] == want["max_nbhd"] and got["sum_nbhd"] == want["sum_nbhd"]
    if np.isfinite(want["colour"]).all():
        check_pass(got, want)
    else:
        for k in ("nbhd_size", "member_hash", "bin_hash"):
            assert (got[k] == want[k]).all(), k
        fin = np.isfinite(want["colour"])
        assert rel_l2(got["colour"][fin], want["colour"][fin]) <= REL_L2_BAR


# ---- (a) default options against the oracle ------------------------------------------------------------------------------
@SEEDS
@POLICIES
@pytest.mark.parametrize("fid", list(P.FRAMES))
def test_default_route_vs_oracle(ctx, hipmod, oracle, fid, policy, seed):
    want = P.oracle_pass(oracle, fid, policy, seed)
    got = base(ctx, hipmod, fid, policy, seed)
    assert got["route"] == 2 if fid in BINNED else got["route"] in (0, 1)
    assert_oracle_parity(got, want, hipmod, fid)
    if seed == P.ACTIVE_SIGMA_SEED:
        assert moved(oracle, fid, seed) > 0.05      # the colour parity above is not vacuous


# ---- (b) every route that can take the frame -------------------------------------------------------------------------------
ROUTES = ([(f, o, v) for f in UNBINNED for o, v in (("count_first", 0), ("count_first", 1), ("packed", 0))]
          + [(f, "packed", 0) for f in BINNED]
          + [(f, "split_weights", 0) for f in ("B32", "B64", "H64")]
          + [(f, "waves_per_pixel", 1) for f in ("B32", "B64")]
          + [("U8", "binning", 1)])     # the unbinned-size frame through classify_kernel (B16: binning 0 is not valid above 512)


@SEEDS
@pytest.mark.parametrize("fid,option,value", ROUTES)
def test_routes_agree(ctx, hipmod, fid, option, value, seed):
    """bit for bit on every stage output; colours bit for bit, across packed 0 / 1 to rtol 1e-12 (the bar of
    test_packed_small_neighbourhood_kernels; measured with the filter active: up to 10 % of a frame's colours differ there, by
    at most 7.4e-16 relative, and none across any other option).  A fresh context per option: nothing leaks."""
    for policy in (EPS, REF_ABORT):
        ref = base(ctx, hipmod, fid, policy, seed)
        with hipmod.Context(0) as c:
            c.set_option(option, value)
            got = run(c, hipmod, fid, policy, seed)
        if option == "count_first":
            assert got["route"] == value
        elif option == "binning":
            assert got["route"] == 2
        for k in STAGE_KEYS:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (policy, k)
        assert got["status"] == ref["status"] and got["nonfinite_pixels"] == ref["nonfinite_pixels"]
        assert got["first_bad_pixel"] == ref["first_bad_pixel"]
        assert np.array_equal(np.isnan(got["colour"]), np.isnan(ref["colour"]))
        m = np.isfinite(ref["colour"])
        a, b = got["colour"][m], ref["colour"][m]
        print("%s %s=%d policy %d seed %g: %d of %d colours differ, max relative %.3e" % (
            fid, option, value, policy, seed, int((a != b).sum()), a.size,
            float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300), initial=0.0))))
        if option == "packed":
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-300)
        else:
            assert np.array_equal(a, b), (policy, "colour")


# ---- (c) the layout-generic kernel: planted 64 | 65, 128 | 129, 256 | 257 straddle its kChunk = 64 and kThreads = 256 --------
@SEEDS
@POLICIES
@pytest.mark.parametrize("fid", ["U8", "B16", "B40", "H16"])
def test_generic_kernel_vs_oracle(ctx, hipmod, oracle, fid, policy, seed):
    want = P.oracle_pass(oracle, fid, policy, seed)
    got = run(ctx, hipmod, fid, policy, seed, flags=hipmod.FLAG_GENERIC)
    assert got["route"] == 3 and got["redo_pixels"] == 0
    assert_oracle_parity(got, want, hipmod, fid)


# ---- (d) a row slab that is the target row alone --------------------------------------------------------------------------
@SEEDS
@pytest.mark.parametrize("fid", ["U8", "B16"])
def test_target_row_slab_equals_full_frame(ctx, hipmod, fid, seed):
    """rows [b, b + 1): the slab owns the row of the targets and nothing else, every window reaches into halo rows on both
    sides; N, member order and colours of that row are the full-frame run's, bit for bit"""
    b = (geometry(fid)[3] - 1) // 2
    full = base(ctx, hipmod, fid, EPS, seed)
    with hipmod.Context(0) as c:
        part = run(c, hipmod, fid, EPS, seed, row_begin=b, row_end=b + 1)
    for (y, x), n in zip(P.frame(fid)[2], P.frame(fid)[3]):
        assert y == b and part["nbhd_size"][y, x] == n
    for k in ("nbhd_size", "member_hash"):
        assert np.array_equal(part[k][b], full[k][b]), k
    assert np.array_equal(part["colour"][:, b], full["colour"][:, b])
    # the halo rows pass through unfiltered
    cin = P.frame(fid)[1][2:5].astype(np.float64)
    assert np.array_equal(part["colour"][:, :b], cin[:, :b]) and np.array_equal(part["colour"][:, b + 1:], cin[:, b + 1:])


# ---- (e) rpf_filter and rpf_multi_filter ----------------------------------------------------------------------------------
@SEEDS
@pytest.mark.parametrize("fid", ["U8", "B16"])
def test_filter_entries_on_planted_frames(ctx, hipmod, oracle, fid, seed):
    """rpf_filter with a ray weight and rpf_multi_filter on two slabs of device 0: the sample colours of the debug pass
    rounded to fp32, the oracle's largest neighbourhood in the counters.  Both frames are box 7 and 7 rows high: two slabs
    own rows [0, 3) and [3, 7), neither fewer than b = 3, so the multi run takes the one-window-row frame as it is."""
    W, H, S, box = geometry(fid)
    assert H // 2 >= (box - 1) // 2
    planes = P.frame(fid)[0]
    want = P.oracle_pass(oracle, fid, EPS, seed)
    ref = base(ctx, hipmod, fid, EPS, seed)["colour"].astype(np.float32)
    rw = (0.5 + np.random.default_rng(7).random((H, W, S))).astype(np.float32)
    desc = hip_desc(hipmod, fid, EPS, boxes=(box,), sigma_seed=seed)
    with hipmod.Context(0) as c:
        srgb, prgb, st = c.filter(planes, desc, ray_weight=rw)
        assert st == hipmod.OK and c.counters().max_nbhd == want["max_nbhd"]
    assert np.array_equal(srgb, ref)
    want_pix = oracle.pixel_mean(want["colour"], oracle.make_desc(W, H, S), rw)
    assert rel_l2(prgb.astype(np.float64), want_pix) <= REL_L2_BAR
    with hipmod.MultiContext([0, 0]) as mc:
        s2, p2, st2 = mc.filter(planes, desc, ray_weight=rw)
        assert st2 == hipmod.OK and mc.counters().max_nbhd == want["max_nbhd"]
    assert np.array_equal(s2, ref) and np.array_equal(p2, prgb)
