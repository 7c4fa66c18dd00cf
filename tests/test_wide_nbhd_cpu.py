"""Wide neighbourhoods (RPF_FLAG_WIDE_NBHD, 65535 < box * box * S <= 262144), the part that needs no GPU: the flag in
rpf_layout_kernels, rpf_max_nbhd, the wide kernel's k ln k table, and the input conditions of the fixtures
tests/golden/wide_*.npz (tests/golden/make_wide_golden.py wrote them; tests/test_wide_nbhd_gpu.py compares the kernels with
them): the planes the tests rebuild are the planes the oracle saw, the planted sizes are in the oracle's row, no MI value of
a fixture is anywhere near a zero band (the condition under which the oracle is a valid EPS reference above N = 48585, see
DESIGN.md section 11c), and the heavy frame's joint cells hold the counts no 16-bit cell could."""
import os
import time

import numpy as np
import pytest

import wide_frames as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture(fid):
    return np.load(os.path.join(GOLD, "wide_%s.npz" % fid))


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_layout_kernels_with_the_wide_flag(hipmod):
    wide = hipmod.FLAG_WIDE_NBHD
    assert wide == 64
    assert hipmod.layout_kernels(hipmod.make_desc(8, 8, 8, flags=wide)) == (hipmod.OK, 0)
    assert hipmod.layout_kernels(hipmod.make_desc(8, 8, 8, flags=wide, n_random=4, n_feat=18, plane_dtype=hipmod.PLANES_F16)) == (hipmod.OK, 0)
    # any other layout needs RPF_FLAG_GENERIC as before
    d = hipmod.make_desc(8, 8, 8, flags=wide, n_random=3, n_feat=12)
    assert hipmod.layout_kernels(d) == (hipmod.E_UNSUPPORTED, None)
    d.flags = wide | hipmod.FLAG_GENERIC
    assert hipmod.layout_kernels(d) == (hipmod.OK, 1)
    for extra in (hipmod.FLAG_GENERIC_PACKED, hipmod.FLAG_GENERIC_PACKED | hipmod.FLAG_GENERIC_WAVE):
        d.flags = wide | hipmod.FLAG_GENERIC | extra
        assert hipmod.layout_kernels(d) == (hipmod.OK, 1)
    # fp64 throughout
    assert hipmod.layout_kernels(hipmod.make_desc(8, 8, 8, flags=wide | hipmod.FLAG_FAST_WEIGHTS)) == (hipmod.E_UNSUPPORTED, None)
    # and nothing moved without the flag
    assert hipmod.layout_kernels(hipmod.make_desc(8, 8, 8, flags=hipmod.FLAG_FAST_WEIGHTS)) == (hipmod.OK, 0)


def test_max_nbhd(hipmod):
    assert hipmod.max_nbhd(hipmod.make_desc(8, 8, 8)) == (hipmod.OK, 65535)
    assert hipmod.max_nbhd(hipmod.make_desc(8, 8, 8, flags=hipmod.FLAG_GENERIC | hipmod.FLAG_TIMING)) == (hipmod.OK, 65535)
    assert hipmod.max_nbhd(hipmod.make_desc(8, 8, 8, flags=hipmod.FLAG_WIDE_NBHD)) == (hipmod.OK, 262144)
    assert hipmod.max_nbhd(hipmod.make_desc(8, 8, 8, flags=hipmod.FLAG_WIDE_NBHD | hipmod.FLAG_GENERIC)) == (hipmod.OK, 262144)
    assert hipmod.max_nbhd(None) == (hipmod.E_BADARG, None)
    assert hipmod.load().rpf_max_nbhd(None, None) == hipmod.E_BADARG


# ---- the table ---------------------------------------------------------------------------------------------------------------
def _k_ln_k(k, bits):
    """round(k ln k * 2^bits) in long double, as exact Python integers.  Halves round away from zero, as llroundl does: near
    2^62 a long double keeps one fractional bit, so every other entry IS a half (v + 0.5 is exact below 2^63)."""
    k = np.asarray(k, np.longdouble)
    v = np.floor(np.ldexp(k * np.log(np.maximum(k, 1)), bits) + np.longdouble(0.5))
    return [int(x) for x in np.atleast_1d(v)]


def test_wide_table_is_exact_below_2_63(hipmod):
    """T_w[k] = round(k ln k * 2^41), k = 0 .. 2^18: every entry below 2^63, strictly increasing from k = 1, and the entry the
    long-double expression gives -- at every k (compared as long doubles: exact below 2^64), and as integers at the edges."""
    assert np.finfo(np.longdouble).nmant >= 63   # the x87 format the library's own long double has
    n = 1 << 18
    t = hipmod.wide_table(n)
    assert t.shape == (n + 1,) and t.dtype == np.uint64
    assert t[0] == 0 and t[1] == 0 and int(t.max()) < 2 ** 63
    assert (np.diff(t[1:].astype(np.int64)) > 0).all()
    k = np.arange(n + 1, dtype=np.longdouble)
    want = np.floor(np.ldexp(k * np.log(np.maximum(k, 1)), 41) + np.longdouble(0.5))
    assert np.array_equal(t.astype(np.longdouble), want)
    edges = [48585, 48586, 65535, 65536, 262144]
    assert [int(t[e]) for e in edges] == _k_ln_k(edges, 41)
    # the 2^-44 format of the other kernels: 48585 is its last entry below 2^63
    a, b = _k_ln_k([48585, 48586], 44)
    assert a < 2 ** 63 <= b
    # a shorter table is a prefix; the bounds are refused
    assert np.array_equal(hipmod.wide_table(1000), t[:1001])
    for bad in (-1, n + 1):
        with pytest.raises(hipmod.RpfError):
            hipmod.wide_table(bad)


# ---- the fixtures' input conditions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", list(F.FRAMES))
def test_fixture_conditions(fid):
    g = fixture(fid)
    (nr, nf, _), targets = F.FRAMES[fid]
    stored, _, pixels, _ = F.frame(fid)
    W, H = F.geometry(fid)
    ndim, npair = 5 + nr + nf, nf * (nr + 2) + 3 * (nr + 2 + nf)
    assert stored.shape == (ndim, H, W, F.S) and F.BOX * F.BOX * F.S == F.NMAX == 68229
    assert int(g["crc"]) == F.checksum(fid), "the planes rebuilt here are not the planes the oracle filtered"
    assert tuple(g["targets"]) == targets
    assert g["nbhd_size"].shape == (W,) and g["mi"].shape == (W, npair) and g["mean"].shape == (W, ndim)
    for (y, x), n in zip(pixels, targets):
        assert y == F.ROW and g["nbhd_size"][x] == n
    assert g["nbhd_size"].max() <= F.NMAX and g["nbhd_size"].min() >= F.S
    # no table near a zero band: what makes the oracle a valid EPS reference at these sizes
    assert np.abs(g["mi"]).min() > 1e-9
    policies = ("ref_abort",) if fid == "heavy" else ("ref_abort", "eps")
    for p in policies:
        assert int(g["status_" + p]) == 0 and int(g["nonfinite_" + p]) == 0
        assert g["colour_" + p].shape == (3, W, F.S) and np.isfinite(g["colour_" + p]).all()
        cin = stored[2:5, F.ROW].astype(np.float64)
        assert np.linalg.norm(g["colour_" + p] - cin) / np.linalg.norm(cin) > 0.05   # a dropped member shows
    assert ("colour_eps" in g.files) == (fid != "heavy")


def test_main_frame_straddles_every_edge():
    """65535 | 65536: the old cap, the 16-bit cell, B = 255 | 256; 66048 | 66049: B = 256 | 257, the first id no byte holds"""
    n = fixture("main")["nbhd_size"]
    B = np.floor(np.sqrt(n.astype(np.float64))).astype(int)
    assert {65535, 65536, 66049, 68229} <= set(n.tolist())
    assert (n <= 65535).any() and (n > 65535).any()
    assert {255, 256, 257, 261} <= set(B.tolist())
    assert (B <= 255).any() and (B > 256).any()


def test_heavy_frame_cells_exceed_16_bits():
    """the joint cells of the tables (2, 5), (2, 6), (3, 5), (3, 6) of the heavy frame's target, counted with numpy"""
    _, p32, _, (n,) = F.frame("heavy")
    mem = F.members("heavy")
    assert int(mem.sum()) == n == 66049
    common = {c: (p32[c] == F.HEAVY_COMMON)[mem] for c in F.HEAVY_COLUMNS}
    assert int((common[2] & common[5]).sum()) == n - 1 and int((common[2] & common[6]).sum()) == n - 1
    assert int((common[3] & common[5]).sum()) == n - 2 and int((common[3] & common[6]).sum()) == n - 2
    assert n - 2 > 65535
    # the planted frame underneath is untouched where membership is decided
    base, _ = F.P.plant(F.S, F.BOX, (66049,), seed=0)
    assert np.array_equal(base[7:], p32[7:]) and np.array_equal(base[0:2], p32[0:2]) and np.array_equal(base[4], p32[4])


# ---- one live oracle run -------------------------------------------------------------------------------------------------------
def test_fixture_row_recomputed_live(oracle):
    """the (1, 1) frame's row, recomputed by the oracle here (7 columns, 9 pairs: the cheapest frame), equals its fixture"""
    g = fixture("l1_1")
    _, p32, _, _ = F.frame("l1_1")
    W, H = F.geometry("l1_1")
    t0 = time.time()
    r = oracle.filter_pass(p32, oracle.make_desc(W, H, F.S, box=F.BOX, row_begin=F.ROW, row_end=F.ROW + 1,
                                                 policy=oracle.DEGEN_EPS, sigma_seed=F.SIGMA_SEED, n_random=1, n_feat=1))
    print("oracle, 57 pixels of the (1, 1) frame: %.1f s" % (time.time() - t0))
    for k in ("nbhd_size", "mean", "stddev", "mi", "bin_hash", "member_hash"):
        assert np.array_equal(r[k][F.ROW], g[k]), k
    for k in ("alpha", "beta", "wrc"):
        assert np.array_equal(r[k][F.ROW], g[k + "_eps"]), k
    assert np.array_equal(r["colour"][:, F.ROW], g["colour_eps"])
