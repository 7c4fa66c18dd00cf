"""CPU tests of the film step: the NumPy restatement of pbrt's AddSample / MergeFilmTile / WriteImage (pbrt_film_ref.py)
checked by hand, pbrt's filter tables from rpf_film_filter_table (host code, no GPU) against the restatement, and the
rpf_film ctypes mirror against include/rpf_hip.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pbrt_film_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_restatement_box_interior_samples_sum_in_order():
    """box r = 0.5, pFilm strictly inside its pixel: each sample reaches its own pixel only, with weight 1; contribSum is the
    fp32 sum of L * rayWeight in sample order and filterWeightSum is S"""
    W, H, S = 5, 4, 6
    rng = np.random.default_rng(1)
    q = np.stack(np.meshgrid(np.arange(W), np.arange(H), indexing="xy"), 0)[..., None].astype(F)
    pf = (q + rng.uniform(0.05, 0.95, (2, H, W, S))).astype(F)
    col = rng.lognormal(0, 2, (3, H, W, S))
    rw = rng.uniform(0.1, 2, (H, W, S)).astype(F)
    t, w, img, _ = R.film(pf, col, (0, 0), ((0, 0), (W, H)), 0.5, 0.5, R.filter_table(R.BOX), rw)
    assert (w == S).all()
    for y in range(H):
        for x in range(W):
            for c in range(3):
                acc = F(0)
                for s in range(S):
                    acc = F(acc + F(F(col[c, y, x, s]) * rw[y, x, s]) * F(1))
                assert t[y, x, c] == acc
    assert np.isfinite(img).all()


def test_restatement_integer_pfilm_lands_in_two_pixels():
    """pFilm.x exactly q: pFilmDiscrete = q - 0.5, Ceil(q - 1) = q - 1 and Floor(q) = q, so pixels q-1 and q both get it"""
    W, H, S = 4, 1, 1
    pf = np.zeros((2, H, W, S), F)
    pf[0, 0, :, 0] = np.arange(W) + F(0.5)
    pf[1] = F(0.5)
    pf[0, 0, 2, 0] = F(2.0)  # on the left edge of pixel 2
    col = np.zeros((3, H, W, S))
    col[:, 0, 2, 0] = 1.0
    t, w, _, _ = R.film(pf, col, (0, 0), ((0, 0), (W, H)), 0.5, 0.5, R.filter_table(R.BOX))
    assert list(w[0]) == [1, 2, 1, 1]  # pixel 1: its own sample and pixel 2's
    assert list(t[0, :, 0]) == [0, 1, 1, 0]


def test_restatement_tables_follow_the_closed_forms():
    r = 2.0
    c = (np.arange(16) + 0.5) * r / 16
    X, Y = np.meshgrid(c, c, indexing="xy")
    assert (R.filter_table(R.BOX) == 1).all()
    np.testing.assert_allclose(R.filter_table(R.TRIANGLE), (r - X) * (r - Y), rtol=1e-6)
    g = lambda v: np.exp(-2 * v * v) - np.exp(-2 * r * r)
    np.testing.assert_allclose(R.filter_table(R.GAUSSIAN), g(X) * g(Y), rtol=0, atol=1e-6)

    def m1(v, B=1 / 3, Cc=1 / 3):
        v = np.abs(2 * v / r)
        return np.where(v > 1, (-B - 6 * Cc) * v ** 3 + (6 * B + 30 * Cc) * v ** 2 + (-12 * B - 48 * Cc) * v + 8 * B + 24 * Cc,
                        (12 - 9 * B - 6 * Cc) * v ** 3 + (-18 + 12 * B + 6 * Cc) * v ** 2 + 6 - 2 * B) / 6
    np.testing.assert_allclose(R.filter_table(R.MITCHELL), m1(X) * m1(Y), rtol=0, atol=1e-6)
    r4 = 4.0
    c4 = (np.arange(16) + 0.5) * r4 / 16
    X4, Y4 = np.meshgrid(c4, c4, indexing="xy")
    ws = lambda v: np.sinc(v) * np.sinc(v / 3)  # np.sinc(v) = sin(pi v) / (pi v)
    np.testing.assert_allclose(R.filter_table(R.SINC), ws(X4) * ws(Y4), rtol=0, atol=1e-6)


@pytest.mark.parametrize("kind,radius,p0,p1", [
    (R.BOX, None, None, None), (R.BOX, (1.5, 0.75), None, None),
    (R.TRIANGLE, None, None, None), (R.TRIANGLE, (1.0, 3.0), None, None),
    (R.GAUSSIAN, None, None, None), (R.GAUSSIAN, (1.5, 2.5), 3.0, None),
    (R.MITCHELL, None, None, None), (R.MITCHELL, (1.25, 2.0), 0.0, 0.5),
    (R.SINC, None, None, None), (R.SINC, (3.0, 4.0), 2.0, None)])
def test_library_filter_table_matches_restatement(hipmod, kind, radius, p0, p1):
    got = hipmod.film_table(kind, radius, p0, p1)
    rx, ry = hipmod._radii(kind, radius)
    want = R.filter_table(kind, rx, ry, p0, p1)
    assert got.dtype == np.float32 and got.shape == (16, 16)
    if kind in (R.GAUSSIAN, R.SINC):  # NumPy's float32 exp / sin are not glibc's expf / sinf
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
    else:
        assert np.array_equal(got, want)


def test_library_filter_table_refusals(hipmod):
    L = hipmod.load()
    t = np.empty(256, np.float32)
    p = t.ctypes.data_as(C.c_void_p)
    nan = float("nan")
    for kind, rx, ry in [(0, 0.0, 1.0), (0, 1.0, -1.0), (2, float("inf"), 2.0), (2, nan, 2.0), (5, 1.0, 1.0), (-1, 1.0, 1.0)]:
        assert L.rpf_film_filter_table(kind, rx, ry, nan, nan, p) == hipmod.E_BADARG
    assert L.rpf_film_filter_table(0, 0.5, 0.5, nan, nan, None) == hipmod.E_BADARG
    assert L.rpf_film_filter_table(0, 0.5, 0.5, nan, nan, p) == hipmod.OK


def test_film_struct_matches_header(hipmod):
    src = open(os.path.join(ROOT, "include", "rpf_hip.h")).read()
    body = re.search(r"typedef struct rpf_film \{(.*?)\} rpf_film;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\b([a-z_0-9]+)\s*(?:\[[^\]]*\])?\s*[,;]", body)
    assert names == [n for n, _ in hipmod.Film._fields_]
    Fm = hipmod.Film
    assert [Fm.sample_x0.offset, Fm.sample_y0.offset, Fm.px0.offset, Fm.py0.offset, Fm.px1.offset, Fm.py1.offset] == [0, 4, 8, 12, 16, 20]
    assert [Fm.radius_x.offset, Fm.radius_y.offset, Fm.max_sample_luminance.offset, Fm.scale.offset, Fm.table.offset] == [24, 28, 32, 36, 40]
    assert C.sizeof(Fm) == 40 + 4 * 256


def test_make_film_takes_pbrt_sample_bounds(hipmod):
    for r in (0.5, 1.5, 2.0, 4.0):
        f = hipmod.make_film(((0, 0), (64, 48)), r, np.ones((16, 16), np.float32))
        (x0, y0), _ = R.sample_bounds(((0, 0), (64, 48)), r, r)
        assert (f.sample_x0, f.sample_y0) == (x0, y0)
    assert R.sample_bounds(((0, 0), (1920, 1080)), 2.0, 2.0) == ((-2, -2), (1922, 1082))
    assert R.sample_bounds(((0, 0), (1920, 1080)), 0.5, 0.5) == ((0, 0), (1920, 1080))


def test_gather_window_bound():
    """the kernel's window: no sample of pixel q = x + k + 1 can reach x unless the rounding gap
    g = (k + 1) - (r + 0.5) is within an ulp of the coordinates, and then the widened window covers it"""
    def touches(q, x, r, d_off):
        d = F(F(q) + F(d_off)) - F(0.5)  # pFilm = q + d_off, d_off in [0, 1]
        return np.ceil(F(d - F(r))) <= x <= np.floor(F(d + F(r)))

    def half_width(r, M):
        k = np.floor(float(r) + 0.5)
        g = (k + 1) - (float(r) + 0.5)
        return int(k) + (1 if g <= M * 2.0 ** -23 else 0)

    for r in [F(0.5), F(1.0), F(1.5), F(2.0), F(4.0), F(1.5) - F(2.0 ** -23), F(2.5) - F(2.0 ** -22), F(0.75)]:
        for x in [0, 7, 8, 100, 1000, 4095, -3]:
            M = abs(x) + 64 + float(r)
            h = half_width(r, M)
            for off in [0.0, 1e-7, 0.5, 1.0]:
                assert not touches(x + h + 1, x, r, off) and not touches(x - h - 1, x, r, 1.0 - off)
    # the case that needs the widening: box r = 1.5 - 2^-23, pFilm exactly q = x + 2 reaches x once half an ulp of x is
    # 2^-23 or more (x >= 2); where 2^-23 is exact (x = 0) it does not
    r = F(1.5) - F(2.0 ** -23)
    assert touches(10, 8, r, 0.0) and touches(4, 2, r, 0.0) and not touches(2, 0, r, 0.0)
    assert half_width(r, 8 + 64) == 2 and np.floor(float(r) + 0.5) == 1
