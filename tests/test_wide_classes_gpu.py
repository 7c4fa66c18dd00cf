"""GPU tests of a wide pass dealt by size class (RPF_FLAG_WIDE_NBHD | RPF_FLAG_WIDE_CLASSES, rpf_query_route 7):
generic::wide_count_kernel lists the members of every pixel with N <= 832, generic::filter_packed_kernel (N <= 64) and
generic::filter_wave_kernel (N <= 832) read them, generic::filter_wide_kernel takes the rest list and the redo list.  "Route 6"
below is the same context and buffer with RPF_FLAG_WIDE_NBHD alone.  The input conditions of the fixture
tests/golden/wide_classes.npz are asserted on the CPU by tests/test_wide_classes_cpu.py.

Bars: check_pass of tests/test_gpu_parity.py, unchanged (discrete keys, mean and stddev bit-equal; MI 1e-11; alpha, beta, W_r_c
rtol 1e-9; colours 1e-4 relative L2); everything else is bit equality.  No tolerance of its own."""
import os

import numpy as np
import pytest

import planted_nbhd as P
import wide_classes_frames as F
from test_gpu_parity import REL_L2_BAR, STAGE_KEYS, check_pass, rel_l2

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
POLICIES = pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAPS = (8, 16, 32, 64, 128, 256, 448, 832)
DISCRETE_AND_STATS = ("nbhd_size", "member_hash", "bin_hash", "mean", "stddev")

# ---- the small frames: planted sizes at every class edge, forced onto the wide route by option "wide" = 1 ------------------------
# X8: the fewest columns and pairs, under RPF_FLAG_GENERIC.  B32 (832 | 833 | 1568) is here for the rest class: box 7 at 8 or 16
# spp cannot hold a neighbourhood above 784.
X8 = ((1, 1, "f32"), 8, 7, (8, 9, 64, 65, 128, 129, 392))
SMALL = ["U8", "B16", "U3", "H8", "X8", "B32"]
_x8 = {}


def small(fid):
    """(layout, S, box, targets, stored planes, fp32 planes, target pixels)"""
    if fid == "X8":
        if not _x8:
            planes, pixels = P.plant(8, 7, X8[3], n_random=1, n_feat=1)
            planes.setflags(write=False)
            _x8["f"] = (planes, planes, pixels)
        return X8 + _x8["f"]
    lay, S, box, targets, _, _ = P.FRAMES[fid]
    stored, p32, pixels, _ = P.frame(fid)
    return lay, S, box, targets, stored, p32, pixels


_want = {}


def small_oracle(oracle, fid, policy):
    if fid != "X8":
        return P.oracle_pass(oracle, fid, policy, P.ACTIVE_SIGMA_SEED)
    if policy not in _want:
        lay, S, box, targets, _, p32, _ = small(fid)
        _want[policy] = oracle.filter_pass(p32, oracle.make_desc(box * len(targets), box, S, box=box, policy=policy,
                                                                 sigma_seed=P.ACTIVE_SIGMA_SEED, n_random=1, n_feat=1))
    return _want[policy]


def wide_flags(hipmod, lay, classes):
    compiled = lay in ((2, 12, "f32"), (4, 18, "f16"))
    return hipmod.FLAG_WIDE_NBHD | (hipmod.FLAG_WIDE_CLASSES if classes else 0) | (0 if compiled else hipmod.FLAG_GENERIC)


def desc_of(hipmod, lay, W, H, S, policy, classes=True, **kw):
    nr, nf, dt = lay
    extra = dict(n_random=nr, n_feat=nf) if (nr, nf) != (2, 12) else {}
    if dt == "f16":
        extra["plane_dtype"] = hipmod.PLANES_F16
    kw.setdefault("flags", wide_flags(hipmod, lay, classes))
    return hipmod.make_desc(W, H, S, policy=policy, **extra, **kw)


def run_debug(c, planes, desc, box):
    got = c.filter_pass_debug(planes, desc, box=box, allow_nonfinite=True)
    cnt = c.counters()
    got.update(route=c.route(), launches=cnt.filter_kernel_launches, redo_pixels=cnt.redo_pixels, options_active=cnt.options_active)
    return got


@pytest.fixture(scope="module")
def forced(hipmod):
    """a context on which every pass of a call with the wide flag is a wide pass"""
    with hipmod.Context(0) as c:
        c.set_option("wide", 1)
        yield c


_runs = {}


def small_run(forced, hipmod, fid, policy, classes):
    """a forced wide pass over a small frame: run once per variant, shared, never modified"""
    key = (fid, policy, classes)
    if key not in _runs:
        lay, S, box, targets, stored, _, _ = small(fid)
        d = desc_of(hipmod, lay, box * len(targets), box, S, policy, classes=classes, sigma_seed=P.ACTIVE_SIGMA_SEED)
        _runs[key] = run_debug(forced, stored, d, box)
    return _runs[key]


def expected_launches(n, policy):
    """one per non-empty packed class, one per non-empty one-wave class, one for the rest list, the redo launch"""
    n = np.asarray(n).ravel()
    lo = (0,) + CAPS[:-1]
    k = sum(1 for a, b in zip(lo, CAPS) if ((n > a) & (n <= b)).any()) + (1 if (n > CAPS[-1]).any() else 0)
    return k + (1 if policy == REF_ABORT else 0)


def assert_parity(got, want, hipmod, oracle_side):
    """check_pass where the reference side's colours are finite; where a pixel is NaN (REF_ABORT) the same status, NaN pattern
    and counters, bit-equal discrete outputs, and the colour bar where the reference is finite"""
    if oracle_side:
        assert (got["status"] == hipmod.E_NONFINITE) == (want["status"] == 1)
    else:
        assert got["status"] == want["status"]
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(want["colour"]))
    assert got["nonfinite_pixels"] == want["nonfinite_pixels"] and got["first_bad_pixel"] == want["first_bad_pixel"]
    assert got["max_nbhd"] == want["max_nbhd"] and got["sum_nbhd"] == want["sum_nbhd"]
    if np.isfinite(want["colour"]).all():
        return check_pass(got, want)
    for k in ("nbhd_size", "member_hash", "bin_hash"):
        assert (got[k] == want[k]).all(), k
    fin = np.isfinite(want["colour"])
    r = rel_l2(got["colour"][fin], want["colour"][fin])
    assert r <= REL_L2_BAR, r
    return r


# ---- (a) small frames, live oracle, every class ---------------------------------------------------------------------------------
@POLICIES
@pytest.mark.parametrize("fid", SMALL)
def test_small_frames_vs_oracle(forced, hipmod, oracle, fid, policy):
    want = small_oracle(oracle, fid, policy)
    got = small_run(forced, hipmod, fid, policy, True)
    assert got["route"] == 7 and got["options_active"] == 1
    _, _, _, targets, _, _, pixels = small(fid)
    for (y, x), n in zip(pixels, targets):
        assert got["nbhd_size"][y, x] == n, ((y, x), n, int(got["nbhd_size"][y, x]))
    r = assert_parity(got, want, hipmod, True)
    print("%s policy %d: colours %.3e rel-L2, launches %d, redo %d" % (fid, policy, r, got["launches"], got["redo_pixels"]))
    assert got["launches"] == expected_launches(got["nbhd_size"], policy)
    if policy == REF_ABORT:
        other = small_oracle(oracle, fid, EPS)
        differ = int((want["mi"] != other["mi"]).any(axis=-1).sum())
        print("%s: %d pixels whose oracle MI differs between the policies" % (fid, differ))
        if differ:
            assert got["redo_pixels"] == differ
    else:
        assert got["redo_pixels"] == 0


def test_small_frames_fill_every_class(forced, hipmod):
    """between them: all eight classes and the rest class, and a packed class that ends on a half-empty wave"""
    n = np.concatenate([small_run(forced, hipmod, fid, EPS, True)["nbhd_size"].ravel() for fid in SMALL])
    lo = (0,) + CAPS[:-1]
    assert all(((n > a) & (n <= b)).any() for a, b in zip(lo, CAPS)) and (n > 832).any()
    for fid in ("U8", "H8"):    # N <= 32 at 8 spp: two pixels per wave, an odd count of them
        m = small_run(forced, hipmod, fid, EPS, True)["nbhd_size"]
        assert int(((m > 16) & (m <= 32)).sum()) % 2 == 1


# ---- (b) route 7 against route 6 ------------------------------------------------------------------------------------------------------
@POLICIES
@pytest.mark.parametrize("fid", SMALL)
def test_small_frames_vs_route6(forced, hipmod, fid, policy):
    got = small_run(forced, hipmod, fid, policy, True)
    r6 = small_run(forced, hipmod, fid, policy, False)
    assert got["route"] == 7 and r6["route"] == 6 and r6["launches"] == 1 and r6["redo_pixels"] == 0
    for k in DISCRETE_AND_STATS:
        assert got[k].tobytes() == r6[k].tobytes(), k
    assert_parity(got, r6, hipmod, False)


# ---- (c) a really wide frame: the small classes under a window of 68229 candidates ------------------------------------------------
def wide_desc(hipmod, policy, classes=True, **kw):
    return desc_of(hipmod, (2, 12, "f32"), F.W, F.H, F.S, policy, classes=classes, sigma_seed=F.SIGMA_SEED,
                   row_begin=F.ROW, row_end=F.ROW + 1, **kw)


_wide = {}


def wide_run(ctx, hipmod, policy, classes):
    """the row of the targets, without the option: run once per variant, shared, never modified"""
    if (policy, classes) not in _wide:
        _wide[policy, classes] = run_debug(ctx, F.frame()[0], wide_desc(hipmod, policy, classes), F.BOX)
    return _wide[policy, classes]


def row_of(got, cols=slice(None)):
    d = {k: got[k][F.ROW:F.ROW + 1, cols] for k in STAGE_KEYS}
    d["colour"] = got["colour"][:, F.ROW:F.ROW + 1, cols]
    return d


@POLICIES
def test_wide_frame_vs_route6_and_fixture(ctx, hipmod, policy):
    got = wide_run(ctx, hipmod, policy, True)
    r6 = wide_run(ctx, hipmod, policy, False)
    assert got["route"] == 7 and got["options_active"] == 0 and r6["route"] == 6
    for (y, x), n in zip(F.frame()[1], F.TARGETS):
        assert got["nbhd_size"][y, x] == n
    assert got["launches"] == expected_launches(got["nbhd_size"][F.ROW], policy)
    # route 6 on the same row
    assert got["status"] == r6["status"] and got["nonfinite_pixels"] == r6["nonfinite_pixels"]
    assert got["max_nbhd"] == r6["max_nbhd"] == 66049 and got["sum_nbhd"] == r6["sum_nbhd"]
    a, b = row_of(got), row_of(r6)
    for k in DISCRETE_AND_STATS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.array_equal(np.isnan(a["colour"]), np.isnan(b["colour"]))
    fin = np.isfinite(b["colour"]).all(axis=(0, 3))[0]
    check_pass(row_of(got, fin), row_of(r6, fin))
    # the oracle's row
    g = np.load(os.path.join(GOLD, "wide_classes.npz"))
    p = "eps" if policy == EPS else "ref_abort"
    assert np.array_equal(a["nbhd_size"][0], g["nbhd_size"]) and np.array_equal(a["member_hash"][0], g["member_hash"])
    assert (got["status"] == hipmod.E_NONFINITE) == (int(g["status_" + p]) == 1)
    assert got["nonfinite_pixels"] == int(g["nonfinite_" + p])
    pix = g["pix"]
    want = {k: g[k][None] for k in ("mean", "stddev", "bin_hash")}
    want.update(nbhd_size=g["nbhd_size"][pix][None], member_hash=g["member_hash"][pix][None])
    want.update({k: g["%s_%s" % (k, p)][None] for k in ("mi", "alpha", "beta", "wrc")})
    want["colour"] = g["colour_" + p][:, None]
    mine = row_of(got, pix)
    assert np.array_equal(np.isnan(mine["colour"]), np.isnan(want["colour"]))
    ok = np.isfinite(want["colour"]).all(axis=(0, 3))[0]
    r = check_pass({k: v[..., ok, :] if k == "colour" else v[:, ok] for k, v in mine.items()},
                   {k: v[..., ok, :] if k == "colour" else v[:, ok] for k, v in want.items()})
    print("wide frame, policy %d: %d fixture pixels, colours %.3e rel-L2, redo %d" % (policy, int(ok.sum()), r, got["redo_pixels"]))
    cin = F.frame()[0][2:5].astype(np.float64)
    assert np.array_equal(got["colour"][:, :F.ROW], cin[:, :F.ROW]) and np.array_equal(got["colour"][:, F.ROW + 1:], cin[:, F.ROW + 1:])


# ---- (d) the flat-pixel proof ------------------------------------------------------------------------------------------------------------
FLAT_W, FLAT_H, FLAT_S, FLAT_BOX = 36, 9, 8, 7
FLAT_PIXELS = ((4, 4), (4, 13), (4, 22), (4, 31))   # plain | a NaN sample in the window | a +inf sample in the window | constant +inf


def flat_frame(with_nan=True):
    rng = np.random.default_rng(11)
    planes = rng.random((19, FLAT_H, FLAT_W, FLAT_S)).astype(np.float32)
    planes[0] = (np.arange(FLAT_W)[None, :, None] + rng.random((FLAT_H, FLAT_W, FLAT_S))).astype(np.float32)
    planes[1] = (np.arange(FLAT_H)[:, None, None] + rng.random((FLAT_H, FLAT_W, FLAT_S))).astype(np.float32)
    for y, x in FLAT_PIXELS:
        planes[7, y, x, :] = 0.5                      # feature 0 constant over the own samples: sigma = 0
    (_, _), (by, bx), (cy, cx), (dy, dx) = FLAT_PIXELS
    if with_nan:
        planes[7, by + 1, bx + 2, 3] = np.nan         # passes a zero-width test
    planes[7, cy - 2, cx - 1, 5] = np.inf             # |inf - 0.5| = inf >= 0: rejected
    planes[7, dy, dx, :] = np.inf                     # mean +inf: |inf - inf| = NaN never rejects, nothing is proven
    return planes


@POLICIES
@pytest.mark.parametrize("with_nan", [True, False], ids=["nan_in_frame", "no_nan"])
def test_flat_pixel_proof(forced, hipmod, oracle, policy, with_nan):
    """without the NaN sample the proof holds for the first and the third pixel (no walk); with it every pixel walks"""
    planes = flat_frame(with_nan)
    want = oracle.filter_pass(planes, oracle.make_desc(FLAT_W, FLAT_H, FLAT_S, box=FLAT_BOX, policy=policy))
    lay = (2, 12, "f32")
    got = run_debug(forced, planes, desc_of(hipmod, lay, FLAT_W, FLAT_H, FLAT_S, policy), FLAT_BOX)
    r6 = run_debug(forced, planes, desc_of(hipmod, lay, FLAT_W, FLAT_H, FLAT_S, policy, classes=False), FLAT_BOX)
    assert got["route"] == 7 and r6["route"] == 6
    (ay, ax), (by, bx), (cy, cx), (dy, dx) = FLAT_PIXELS
    assert want["nbhd_size"][ay, ax] == FLAT_S and want["nbhd_size"][cy, cx] == FLAT_S
    assert (want["nbhd_size"][by, bx] == FLAT_S + 1) == with_nan     # the NaN candidate alone joins
    print("policy %d, nan %d: N at the four pixels %s" % (policy, with_nan, [int(want["nbhd_size"][p]) for p in FLAT_PIXELS]))
    for k in ("nbhd_size", "member_hash"):
        assert np.array_equal(got[k], r6[k]), k
        assert np.array_equal(got[k], want[k]), k
    assert got["status"] == r6["status"] and (got["status"] == hipmod.E_NONFINITE) == (want["status"] == 1)
    assert got["sum_nbhd"] == r6["sum_nbhd"] and got["max_nbhd"] == r6["max_nbhd"]


# ---- (e) entry points, on the 57 x 57 x 21 buffer of tests/test_wide_nbhd_gpu.py -------------------------------------------------------
_full = {}
LAY19 = (2, 12, "f32")


def buf57():
    if "planes" not in _full:
        planes, _ = P.plant(F.S, F.BOX, (66049,), seed=0)
        planes.setflags(write=False)
        _full["planes"] = planes
    return _full["planes"]


def desc57(hipmod, classes=True, **kw):
    return desc_of(hipmod, LAY19, F.BOX, F.BOX, F.S, EPS, classes=classes, sigma_seed=F.SIGMA_SEED, **kw)


def full_pass(ctx, hipmod):
    """rpf_filter_ex, one route-7 pass (box 57) over the whole buffer, EPS.  Run once, shared, never modified."""
    if "c64" not in _full:
        srgb, prgb, st, c64 = ctx.filter(buf57(), desc57(hipmod, boxes=(F.BOX,)), want_colour64=True)
        cnt = ctx.counters()
        assert st == hipmod.OK and ctx.route() == 7 and cnt.redo_pixels == 0 and cnt.max_nbhd == 66049
        _full.update(srgb=srgb, prgb=prgb, c64=c64, nbhd=ctx.nbhd(F.BOX, F.BOX), sum_nbhd=cnt.sum_nbhd)
    return _full


def test_entries_vs_route6(ctx, hipmod):
    ref = full_pass(ctx, hipmod)
    _, _, st, c6 = ctx.filter(buf57(), desc57(hipmod, classes=False, boxes=(F.BOX,)), want_colour64=True)
    assert st == hipmod.OK and ctx.route() == 6
    assert rel_l2(ref["c64"], c6) <= REL_L2_BAR
    assert np.array_equal(ctx.nbhd(F.BOX, F.BOX), ref["nbhd"]) and ctx.counters().sum_nbhd == ref["sum_nbhd"]
    a = run_debug(ctx, buf57(), desc57(hipmod, row_begin=F.ROW, row_end=F.ROW + 1), F.BOX)
    b = run_debug(ctx, buf57(), desc57(hipmod, classes=False, row_begin=F.ROW, row_end=F.ROW + 1), F.BOX)
    assert a["route"] == 7 and b["route"] == 6
    for k in ("nbhd_size", "member_hash"):
        assert np.array_equal(a[k][F.ROW], b[k][F.ROW]), k
    # the row slab equals the full frame
    assert a["nbhd_size"][F.ROW, F.ROW] == 66049
    assert np.array_equal(a["colour"][:, F.ROW], ref["c64"][:, F.ROW])


def test_entries_two_passes_equal_two_chained_calls(ctx, hipmod):
    planes = buf57()
    first = full_pass(ctx, hipmod)["c64"]
    _, _, st, both = ctx.filter(planes, desc57(hipmod, boxes=(F.BOX, 7)), want_colour64=True)
    assert st == hipmod.OK and ctx.route() == 2
    _, _, st, second = ctx.filter(planes, desc57(hipmod, boxes=(7,)), colour64_in=first, want_colour64=True)
    assert st == hipmod.OK and ctx.route() == 2
    assert np.array_equal(both, second)
    # the second pass is the one a call without the new flag, and without either flag, runs
    for flags in (hipmod.FLAG_WIDE_NBHD, 0):
        _, _, st, plain = ctx.filter(planes, desc57(hipmod, boxes=(7,), flags=flags), colour64_in=first, want_colour64=True)
        assert st == hipmod.OK and ctx.route() == 2 and np.array_equal(plain, second)


def test_entries_filter_device(ctx, hipmod):
    import torch
    full = full_pass(ctx, hipmod)["c64"]
    dev = torch.device("cuda", 0)
    planes = torch.from_numpy(buf57().copy()).to(dev)
    col = planes[2:5].to(torch.float64).contiguous()
    ctx.filter_device(desc57(hipmod, boxes=(F.BOX,)), planes.data_ptr(), col.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ctx.route() == 7
    assert np.array_equal(col.cpu().numpy(), full)


def test_entries_multi_filter(ctx, hipmod):
    ref = full_pass(ctx, hipmod)
    with hipmod.MultiContext([0, 0]) as mc:
        srgb, prgb, st = mc.filter(buf57(), desc57(hipmod, boxes=(F.BOX,)))
        assert st == hipmod.OK and mc.counters().max_nbhd == 66049
    assert np.array_equal(srgb, ref["srgb"]) and np.array_equal(prgb, ref["prgb"])


def test_entries_filter_film(ctx, hipmod):
    ref = full_pass(ctx, hipmod)
    film = hipmod.make_film(((0, 0), (F.BOX, F.BOX)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX), sample_origin=(0, 0))
    srgb, _, _, _ = ctx.filter_film(buf57(), desc57(hipmod, boxes=(F.BOX,)), film)
    assert ctx.route() == 7
    assert np.array_equal(srgb, ref["srgb"])


# ---- (f) determinism ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", [-1, 1], ids=["default_pool", "pool_of_one"])
def test_determinism_and_pool_growth(ctx, hipmod, pool):
    """pool bases come from an atomic cursor and the class lists from atomics: no result may depend on either.  A pool of one
    entry overflows at the first count launch; the route grows it to the exact size and repeats the launch."""
    runs = []
    for size in (-1, pool):          # two fresh contexts; the second with the hook when the case has one
        with hipmod.Context(0) as c:
            if size >= 0:
                c.set_option("wide_pool", size)
            got = run_debug(c, F.frame()[0], wide_desc(hipmod, REF_ABORT), F.BOX)
            assert got["route"] == 7 and got["options_active"] == (1 if size >= 0 else 0)
            runs.append(got)
    a, b = row_of(runs[0]), row_of(runs[1])
    for k in STAGE_KEYS + ("colour",):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert runs[0]["launches"] == runs[1]["launches"] and runs[0]["redo_pixels"] == runs[1]["redo_pixels"]
    # ... and the session context's run of (c)
    base = row_of(wide_run(ctx, hipmod, REF_ABORT, True))
    for k in STAGE_KEYS + ("colour",):
        assert a[k].tobytes() == base[k].tobytes(), k


# ---- (g) refusals and fall-backs --------------------------------------------------------------------------------------------------------------
def test_flag_without_the_wide_flag_is_refused(ctx, hipmod):
    planes = np.zeros((19, 4, 4, 8), np.float32)
    d = hipmod.make_desc(4, 4, 8, flags=hipmod.FLAG_WIDE_CLASSES)
    assert hipmod.layout_kernels(d) == (hipmod.E_UNSUPPORTED, None)
    with pytest.raises(hipmod.RpfError) as e:
        ctx.filter(planes, d)
    assert e.value.status == hipmod.E_UNSUPPORTED and "RPF_FLAG_WIDE_NBHD" in str(e.value)


def test_more_than_832_spp_is_route_6(ctx, hipmod):
    W, H, S, box = 2, 2, 833, 9      # 9 * 9 * 833 = 67473 > 65535
    planes = np.random.default_rng(5).random((19, H, W, S)).astype(np.float32)
    both = hipmod.FLAG_WIDE_NBHD | hipmod.FLAG_WIDE_CLASSES
    _, _, st, a = ctx.filter(planes, hipmod.make_desc(W, H, S, boxes=(box,), policy=EPS, flags=both), want_colour64=True)
    assert st == hipmod.OK and ctx.route() == 6 and ctx.counters().filter_kernel_launches == 1
    _, _, st, b = ctx.filter(planes, hipmod.make_desc(W, H, S, boxes=(box,), policy=EPS, flags=hipmod.FLAG_WIDE_NBHD), want_colour64=True)
    assert st == hipmod.OK and ctx.route() == 6
    assert a.tobytes() == b.tobytes()


def test_pass_below_the_cap_runs_as_without_the_flags(ctx, hipmod):
    lay, S, box, targets, stored, _, _ = small("U8")
    W, H = box * len(targets), box
    both = hipmod.FLAG_WIDE_NBHD | hipmod.FLAG_WIDE_CLASSES
    a = run_debug(ctx, stored, hipmod.make_desc(W, H, S, policy=EPS, flags=both), box)
    b = run_debug(ctx, stored, hipmod.make_desc(W, H, S, policy=EPS), box)
    assert a["route"] == b["route"] and a["route"] in (0, 1) and a["options_active"] == 0
    for k in STAGE_KEYS + ("colour",):
        assert a[k].tobytes() == b[k].tobytes(), k
