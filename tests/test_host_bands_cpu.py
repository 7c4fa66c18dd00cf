"""CPU tests of tests/host_bands.py: the band cut against a hand-written table, and the conditions that keep
tests/test_host_bands_gpu.py from passing vacuously -- every frame runs in at least three bands, the bands differ from each other,
neighbourhoods cross the band edges, and the stateful pieces of a banded pass (class lists, redo counts, the NaN flag of the
flat-pixel proof, the member pool) each have something to get wrong.  Computed from the oracle and the numpy restatements alone."""
import numpy as np
import pytest

import host_bands as HB
from host_bands import CASES, EPS, REF_ABORT, REST

ALL = list(CASES)


def test_band_cut_against_a_hand_written_table():
    assert HB.bands(12, (7,)) == [(0, 12)]
    assert HB.bands(31, (7,)) == [(0, 31)]
    assert HB.bands(32, (7,)) == [(0, 16), (16, 32)]
    assert HB.bands(48, (7, 5)) == [(0, 16), (16, 32), (32, 48)]
    assert HB.bands(50, (7, 5)) == [(0, 17), (17, 34), (34, 50)]
    assert HB.bands(150, (7,)) == [(19 * j, min(150, 19 * j + 19)) for j in range(8)]
    assert len(HB.bands(150, (7,))) == 8 and HB.bands(150, (7,))[-1] == (133, 150)
    assert HB.bands(81, (55,)) == [(0, 27), (27, 54), (54, 81)]
    assert HB.bands(81, (55, 7)) == [(0, 27), (27, 54), (54, 81)]
    assert HB.bands(52, (35,)) == [(0, 18), (18, 36), (36, 52)]        # a last band of 16 rows under a halo of 17
    assert HB.bands(40, (5, 55, 5)) == [(0, 20), (20, 40)]              # a middle pass does not shape the cut
    assert HB.bands(4000, (7,))[-1][1] == 4000 and len(HB.bands(4000, (7,))) == 8


def test_launch_rule_on_hand_written_sizes():
    n = np.array([[8, 9, 64, 65], [128, 129, 832, 833]])
    assert HB.class_fill(n, 5) == [1, 1, 0, 1, 2, 1, 0, 1, 1] and HB.class_fill(n, 4) == [1, 1, 0, 1, 5]
    assert HB.pass_launches(3, n, EPS) == 1 and HB.pass_launches(6, n, REF_ABORT) == 1
    assert HB.pass_launches(4, n, EPS) == 4 and HB.pass_launches(4, n, REF_ABORT) == 5
    assert HB.pass_launches(5, n, EPS) == 7 and HB.pass_launches(7, n, REF_ABORT) == 8
    assert HB.pass_launches(8, n[:1, :2], REF_ABORT) == 2 and HB.pass_launches(9, n, EPS) == 7
    assert HB.pass_launches(0, n, EPS) is None and HB.pass_launches(2, n, EPS) is None
    cut = [(0, 1), (1, 2)]
    assert HB.expected_launches(5, [n], cut, EPS) == 4 + 4
    assert HB.expected_launches(5, [n, n, n], cut, EPS) == 2 * (4 + 4) + 7      # a middle pass counts once
    assert HB.expected_launches((5, 3), [n, n], cut, REF_ABORT) == (5 + 5) + 2
    assert HB.expected_launches(5, [n], cut, EPS, rows=(1, 2)) == 4           # a band outside the slab launches nothing
    assert HB.expected_launches((5, 0), [n, n], cut, EPS) is None


def test_case_table():
    assert len(CASES) == 23
    for name, c in CASES.items():
        W, H, S = c.shape
        nr, nf, dt = c.lay
        p = HB.planes_of(name)
        assert p.shape == (5 + nr + nf, H, W, S) and p.dtype == (np.float16 if dt == "f16" else np.float32) and not p.flags.writeable
        assert len(c.routes) == len(c.boxes) and all(b % 2 == 1 for b in c.boxes)
        assert (c.draws is not None) == bool(c.flags & HB.HIP.SAMPLED_NBHD_FLAG)
        assert (c.membership is not None) == bool(c.flags & HB.HIP.MEMBER_TEST_FLAG)
        assert (c.schedule is not None) == bool(c.flags & HB.HIP.SCHEDULE_FLAG)
        assert bool(c.classes) == (c.routes[0] in (4, 5, 7, 8, 9) or c.routes[-1] in (4, 5, 7, 8, 9)) or name.endswith("-mixed"), name
    assert all(g != 1.0 for k in ("gain_c", "gain_f") for g in HB.TWO[k]) and len(set(zip(*HB.TWO.values()))) == 2


@pytest.mark.parametrize("name", ALL)
def test_every_frame_runs_in_at_least_three_bands(name):
    c = CASES[name]
    cut = HB.cut_of(name)
    assert len(cut) >= 3 and cut[0][0] == 0 and cut[-1][1] == c.shape[1]
    assert all(a[1] == b[0] for a, b in zip(cut[:-1], cut[1:]))
    if c.rows:   # the slab begins inside the first band and ends inside the last
        assert cut[0][0] < c.rows[0] < cut[0][1] and cut[-1][0] < c.rows[1] < cut[-1][1]
    if name == "lastband":
        assert cut[-1][1] - cut[-1][0] < (c.boxes[0] - 1) // 2


@pytest.mark.parametrize("name", ALL)
def test_band_populations_differ(oracle, name):
    """a band that walked the lists of the band before it would filter other pixels, on other kernels"""
    for p in HB.banded_passes(name):
        fill = HB.band_fill(oracle, name, p)
        print("BANDS %s pass %d (route %d): pixels per class and rest list, per band: %s" % (name, p, CASES[name].routes[p], fill))
        assert any(f != fill[0] for f in fill[1:]), (name, p, fill)


@pytest.mark.parametrize("name", HB.CLASS_ROUTED)
def test_named_classes_are_filled_in_two_bands(oracle, name):
    c = CASES[name]
    for cap in c.classes:
        ok = False
        for p in HB.banded_passes(name):
            if c.routes[p] not in (4, 5, 7, 8, 9):
                continue
            fill = HB.band_fill(oracle, name, p)
            caps = (HB.CAPS[:4] if c.routes[p] == 4 else HB.CAPS) + (REST,)
            if cap in caps:
                k = sum(1 for f in fill if f[caps.index(cap)])
                ok = ok or k >= (1 if cap == REST else 2)
        assert ok, (name, cap)


def test_rest_lists_where_the_shapes_can_reach_them():
    """a rest list is N > 64 on route 4 and N > 832 elsewhere: box * box * S reaches 832 on the box-55 frame alone"""
    for name in HB.CLASS_ROUTED:
        c = CASES[name]
        can = any(r == 4 or (r in (5, 7, 9) and b * b * c.shape[2] > 832 and name not in HB.RA_CASES) for r, b in zip(c.routes, c.boxes))
        assert (REST in c.classes) == can, name
    assert [n for n in HB.CLASS_ROUTED if REST in CASES[n].classes] == ["g4", "wide7"]


@pytest.mark.parametrize("name", ALL)
def test_neighbourhoods_cross_the_band_edges(oracle, name):
    """on every banded pass, a pixel of band j has a member in a row of band j + 1, and a pixel of band j + 1 one in band j"""
    c = CASES[name]
    W = c.shape[0]
    cut = HB.cut_of(name)
    for p in HB.banded_passes(name):
        for j in range(len(cut) - 1):
            edge = cut[j][1]
            down = any((HB.member_rows(oracle, name, p, edge - 1, x) >= edge).any() for x in range(W))
            up = any((HB.member_rows(oracle, name, p, edge, x) < edge).any() for x in range(W))
            assert down and up, (name, p, j)


@pytest.mark.parametrize("name", HB.RA_CASES)
def test_ref_abort_frame_has_redo_pixels_in_every_band(oracle, name):
    c = CASES[name]
    W, H, S = c.shape
    ref, redo = HB.reference(oracle, name), HB.redo_map(oracle, name)
    n = ref["nbhd"][0]
    assert not HB.is_pow2(n).any() and redo.all()                      # N = 15 * whole pixels, an exactly independent (f0, r0) table
    per_band = [int(redo[r0:r1].sum()) for r0, r1 in HB.cut_of(name)]
    assert all(k > 0 for k in per_band) and ref["redo_pixels"] == sum(per_band) == W * H
    assert ref["redo_pixels"] != per_band[-1]                          # what a count zeroed per band leaves
    assert ref["status"] == 0 and np.isfinite(ref["colour"]).all()
    cin = HB.p32_of(name)[2:5].astype(np.float64)
    assert np.linalg.norm(ref["colour"] - cin) / np.linalg.norm(cin) > 1e-3


def test_nonfinite_frame_is_bad_in_the_first_and_the_last_band(oracle):
    name = "fused19-nonfinite"
    W = CASES[name].shape[0]
    ref, cut = HB.reference(oracle, name), HB.cut_of(name)
    bad = np.isnan(ref["colour"]).any(axis=(0, 3))
    assert ref["status"] == 1 and ref["nonfinite_pixels"] == bad.sum() > 0
    assert ref["first_bad_pixel"] == int(np.flatnonzero(bad.ravel())[0]) and HB.band_of(ref["first_bad_pixel"] // W, cut) == 0
    assert bad[cut[-1][0]:].any() and not bad[cut[1][0]:cut[1][1]].all()
    assert np.isfinite(ref["colour"]).mean() > 0.25                   # and the colour bar has something to hold
    assert ref["redo_pixels"] == 0                                    # (the flat pixels have N = S = 8, a power of two)


def test_nan_frame_reaches_a_flat_pixel_across_the_band_edge(oracle):
    name = "fused19-nan"
    c = CASES[name]
    S, b = c.shape[2], (c.boxes[0] - 1) // 2
    cut, p32 = HB.cut_of(name), HB.p32_of(name)
    (yn, xn, sn), (yi, xi, si) = HB.NAN_AT, HB.INF_AT
    assert yn == yi == cut[1][0]                                      # the first row of band 1
    assert np.isnan(p32[7:10, yn, xn, sn]).all() and np.isnan(p32).sum() == 3
    assert np.isinf(p32[7, yi, xi, si]) and np.isinf(p32).sum() == 1
    n = HB.reference(oracle, name)["nbhd"][0]
    flat = (p32[7:10].max(axis=3) == p32[7:10].min(axis=3)).all(axis=0)                 # zero variance on the normal
    hit = [(y, x) for y in range(yn - b, yn) for x in range(max(xn - b, 0), min(xn + b, c.shape[0] - 1) + 1) if flat[y, x]]
    assert hit and all(HB.band_of(y, cut) == 0 for y, _ in hit)
    assert any(n[y, x] > S for y, x in hit)                          # the oracle accepts the NaN sample into a flat pixel of band 0
    assert (n[flat] == S).sum() > 20                                 # while the flat pixels out of its reach keep N = S


@pytest.mark.parametrize("name", ["s-mem", "s-mem-pool1"])
def test_member_pool_grows_from_band_to_band(oracle, name):
    c = CASES[name]
    W = c.shape[0]
    cut, p32 = HB.cut_of(name), HB.p32_of(name)
    need = HB.pool_need(oracle, name, 0)
    first = [8 * (r1 - r0) * W for r0, r1 in cut]
    print("BANDS %s: pool entries per band of pass 0 %s, eight per pixel %s" % (name, need, first))
    flat = (p32[7:10].max(axis=3) == p32[7:10].min(axis=3)).all(axis=0)
    assert flat[:cut[0][1]].mean() > 0.8 and not flat[cut[0][1]:].any()
    assert need[0] < min(need[1:]) and max(need[1:]) > first[1]
    assert need[0] > first[0]                                        # (and the first band already outgrows the first size)
