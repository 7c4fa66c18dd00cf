"""A wide pass dealt by size class (RPF_FLAG_WIDE_NBHD | RPF_FLAG_WIDE_CLASSES, route 7), the part that needs no GPU: the flag
in rpf_layout_kernels, and the input conditions of the fixture tests/golden/wide_classes.npz
(tests/golden/make_wide_classes_golden.py wrote it; tests/test_wide_classes_gpu.py compares the kernels with it): the planes
the tests rebuild are the planes the oracle saw, the planted sizes are in the oracle's row, every size class that 21 spp can
reach is non-empty in that row, and no fixture pixel of 48586 samples or more has a table near a zero band (the condition
under which the oracle is a valid EPS reference there)."""
import os

import numpy as np

import wide_classes_frames as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture():
    return np.load(os.path.join(GOLD, "wide_classes.npz"))


def test_layout_kernels_with_the_classes_flag(hipmod):
    wide, cls = hipmod.FLAG_WIDE_NBHD, hipmod.FLAG_WIDE_CLASSES
    assert cls == 128
    # the flag modifies the wide flag: refused without it, whatever else is set
    for extra in (0, hipmod.FLAG_GENERIC, hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED | hipmod.FLAG_GENERIC_WAVE, hipmod.FLAG_TIMING):
        assert hipmod.layout_kernels(hipmod.make_desc(8, 8, 8, flags=cls | extra)) == (hipmod.E_UNSUPPORTED, None)
    # with it: the answers of the wide flag alone
    assert hipmod.layout_kernels(hipmod.make_desc(8, 8, 8, flags=wide | cls)) == (hipmod.OK, 0)
    assert hipmod.layout_kernels(hipmod.make_desc(8, 8, 8, flags=wide | cls, n_random=4, n_feat=18, plane_dtype=hipmod.PLANES_F16)) == (hipmod.OK, 0)
    d = hipmod.make_desc(8, 8, 8, flags=wide | cls, n_random=3, n_feat=12)
    assert hipmod.layout_kernels(d) == (hipmod.E_UNSUPPORTED, None)      # a layout without compiled kernels still needs the generic flag
    d.flags = wide | cls | hipmod.FLAG_GENERIC
    assert hipmod.layout_kernels(d) == (hipmod.OK, 1)
    for extra in (hipmod.FLAG_GENERIC_PACKED, hipmod.FLAG_GENERIC_PACKED | hipmod.FLAG_GENERIC_WAVE):   # needed by neither, accepted
        d.flags = wide | cls | hipmod.FLAG_GENERIC | extra
        assert hipmod.layout_kernels(d) == (hipmod.OK, 1)
    assert hipmod.layout_kernels(hipmod.make_desc(8, 8, 8, flags=wide | cls | hipmod.FLAG_FAST_WEIGHTS)) == (hipmod.E_UNSUPPORTED, None)
    assert hipmod.max_nbhd(hipmod.make_desc(8, 8, 8, flags=wide | cls)) == (hipmod.OK, 262144)


def test_fixture_conditions():
    g = fixture()
    planes, pixels = F.frame()
    assert planes.shape == (19, F.H, F.W, F.S) and F.NMAX == 68229 > 65535
    assert int(g["crc"]) == F.checksum(), "the planes rebuilt here are not the planes the oracle filtered"
    assert tuple(g["targets"]) == F.TARGETS
    n, pix = g["nbhd_size"], g["pix"]
    assert n.shape == (F.W,) and g["member_hash"].shape == (F.W,)
    assert np.array_equal(pix, F.fixture_pixels())
    for (y, x), t in zip(pixels, F.TARGETS):
        assert y == F.ROW and n[x] == t
        assert {x - 1, x, x + 1} <= set(pix.tolist())      # the targets and the pixels next to them
    assert n.min() == F.S and n.max() == 66049
    npix = len(pix)
    assert g["mean"].shape == (npix, 19) and g["bin_hash"].shape == (npix, 19)
    for p in ("ref_abort", "eps"):
        assert g["mi_" + p].shape == (npix, 96) and g["colour_" + p].shape == (3, npix, F.S)
        assert int(g["status_" + p]) == 0 and int(g["nonfinite_" + p]) == 0 and np.isfinite(g["colour_" + p]).all()
        cin = planes[2:5, F.ROW][:, pix].astype(np.float64)
        assert np.linalg.norm(g["colour_" + p] - cin) / np.linalg.norm(cin) > 0.05   # a dropped member shows
        # from 48586 samples on the oracle's own table is saturated under EPS: no table of such a pixel near a zero band
        big = n[pix] >= 48586
        assert big.any() and np.abs(g["mi_" + p][big]).min() > 1e-9
    big = n[pix] >= 48586
    assert np.array_equal(g["mi_eps"][big], g["mi_ref_abort"][big])
    assert os.path.getsize(os.path.join(GOLD, "wide_classes.npz")) <= 512 * 1024


def test_row_fills_every_class_21_spp_can_reach():
    """S = 21: no pixel fits N <= 8 or 16; every class from N <= 32 on, and the rest class, is non-empty, and the planted
    sizes sit on both sides of each edge"""
    n = fixture()["nbhd_size"]
    edges = (16, 32, 64, 128, 256, 448, 832)
    for lo, hi in zip(edges[:-1], edges[1:]):
        assert ((n > lo) & (n <= hi)).any(), (lo, hi)
        assert hi in n and hi + 1 in n
    assert (n > 832).any() and (n > 65535).any()
    assert (n <= 832).sum() == 13 and (n > 832).sum() == F.W - 13
