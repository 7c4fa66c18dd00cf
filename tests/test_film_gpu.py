"""GPU tests of the film step (rpf_filter_film / rpf_film_splat_device): pbrt's AddSample for every sample, MergeFilmTile and
WriteImage, bit for bit against the NumPy restatement (pbrt_film_ref.py) fed the same fp32 colours; end to end with the
filter passes against the oracle; the refusals; determinism and the C++ host mirror."""
import ctypes as C
import os

import numpy as np
import pytest

import pbrt_film_ref as R
from raytracer_rpf_amd import feature_buffer as fb

pytestmark = pytest.mark.gpu

F = np.float32


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def sample_film(W, H, S, origin, seed, int_frac=0.1):
    """pFilm planes [2,H,W,S] in raster coordinates, q + u with u in [0, 1); a share of the samples sits exactly on q or on
    q + 1 (the two ends pbrt's pPixel + Get2D() can reach)"""
    rng = np.random.default_rng(seed)
    q = [F(origin[0]) + np.arange(W, dtype=F)[None, :, None], F(origin[1]) + np.arange(H, dtype=F)[:, None, None]]
    u = rng.random((2, H, W, S)).astype(F)
    pick = rng.random((2, H, W, S))
    u[pick < int_frac / 2] = F(0)
    u[(pick >= int_frac / 2) & (pick < int_frac)] = F(1)
    return np.stack([(q[a] + u[a]).astype(F) for a in range(2)])


def colours(W, H, S, seed, spikes=0.0):
    rng = np.random.default_rng(seed + 1000)
    c = rng.lognormal(-1, 1.5, (3, H, W, S))
    c[:, rng.random((H, W, S)) < 0.03] = 0.0
    if spikes:
        c[:, rng.random((H, W, S)) < spikes] *= 1e4
    return c


def film_device(ctx, hipmod, pf, col64, film, rw=None):
    import torch
    _, H, W, S = pf.shape
    dev = torch.device("cuda", 0)
    dp = torch.from_numpy(np.ascontiguousarray(pf)).to(dev)
    dc = torch.from_numpy(np.ascontiguousarray(col64)).to(dev)
    drw = None if rw is None else torch.from_numpy(np.ascontiguousarray(rw, F)).to(dev)
    ny, nx = film.py1 - film.py0, film.px1 - film.px0
    t = torch.full((ny, nx, 3), float("nan"), dtype=torch.float32, device=dev)
    w = torch.full((ny, nx), float("nan"), dtype=torch.float32, device=dev)
    img = torch.full((ny, nx, 3), float("nan"), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    ctx.film_splat_device(hipmod.make_desc(W, H, S), film, dp.data_ptr(), dc.data_ptr(), None if drw is None else drw.data_ptr(),
                          t.data_ptr(), w.data_ptr(), img.data_ptr(), stream)
    torch.cuda.synchronize()
    return t.cpu().numpy(), w.cpu().numpy(), img.cpu().numpy()


def check_bits(ctx, hipmod, kind, radius, image, crop=None, origin=None, S=8, seed=0, rw_mode=None, max_lum=np.inf,
               scale=1.0, int_frac=0.1, spikes=0.0):
    rx, ry = hipmod._radii(kind, radius)
    table = hipmod.film_table(kind, (rx, ry))
    bounds = crop or ((0, 0), image)
    (x0, y0), (x1, y1) = R.sample_bounds(bounds if origin is None else ((0, 0), image), rx, ry)
    if origin is not None:
        (x0, y0) = origin
    W, H = x1 - x0, y1 - y0
    pf = sample_film(W, H, S, (x0, y0), seed, int_frac)
    col = colours(W, H, S, seed, spikes)
    rw = None
    if rw_mode == "special":
        rng = np.random.default_rng(seed + 7)
        rw = rng.uniform(0.5, 1.5, (H, W, S)).astype(F)
        rw[rng.random((H, W, S)) < 0.1] = F(0)
        tiny = rng.random((H, W, S)) < 0.05
        rw[tiny] = F(1e-30)
        col[:, tiny] = 1e-10  # L * sampleWeight ~ 1e-40: an fp32 denormal, and smaller still after the filter weight
    film = hipmod.make_film(bounds, (rx, ry), table, sample_origin=(x0, y0), max_sample_luminance=max_lum, scale=scale)
    got = film_device(ctx, hipmod, pf, col, film, rw)
    want = R.film(pf, col.astype(F), (x0, y0), bounds, rx, ry, table, rw, max_lum, scale)
    for g, w_, name in zip(got, want, ("contribSum", "filterWeightSum", "image")):
        assert g.shape == w_.shape and np.array_equal(g, w_), (name, np.argwhere(g != w_)[:5])
    assert (got[1] != 0).any()
    return got, want, (pf, col, rw, film)


@pytest.mark.parametrize("kind", [R.BOX, R.TRIANGLE, R.GAUSSIAN, R.MITCHELL, R.SINC])
def test_film_step_bits_every_filter_at_pbrt_defaults(ctx, hipmod, kind):
    check_bits(ctx, hipmod, kind, None, (37, 21), seed=kind)


def test_film_step_bits_box_r15_and_anisotropic_gaussian(ctx, hipmod):
    check_bits(ctx, hipmod, R.BOX, 1.5, (37, 21), seed=11)
    check_bits(ctx, hipmod, R.GAUSSIAN, (1.5, 2.5), (37, 21), seed=12)


def test_film_step_bits_negative_origin_and_crop_window_inside(ctx, hipmod):
    """buffer origin (-2, -2) for a 40 x 30 image (gaussian r = 2), output pixels a crop window strictly inside it: samples
    outside the crop window still reach its border pixels"""
    got, _, _ = check_bits(ctx, hipmod, R.GAUSSIAN, 2.0, (40, 30), crop=((5, 4), (33, 25)), origin=(-2, -2), seed=13)
    assert got[0].shape == (21, 28, 3)


def test_film_step_bits_ray_weights_zero_and_denormal(ctx, hipmod):
    _, want, (pf, col, rw, film) = check_bits(ctx, hipmod, R.MITCHELL, None, (37, 21), seed=14, rw_mode="special")
    lw, _ = R.prepare(col, rw)
    assert ((lw != 0) & (np.abs(lw) < np.finfo(F).tiny)).any()  # denormal products reached the sums


def test_film_step_bits_luminance_clamp_fires(ctx, hipmod):
    _, want, _ = check_bits(ctx, hipmod, R.GAUSSIAN, None, (37, 21), seed=15, max_lum=10.0, spikes=0.02, scale=0.75)
    assert want[3] > 0  # the clamp changed some samples


@pytest.mark.parametrize("S", [1, 8, 32, 64])
def test_film_step_bits_spp(ctx, hipmod, S):
    check_bits(ctx, hipmod, R.SINC if S == 32 else R.GAUSSIAN, None, (70, 9), S=S, seed=20 + S)


def test_film_step_bits_full_width_slab(ctx, hipmod):
    """one 1920 x 6 x 8 slab of a 1080p frame with the gaussian filter (the buffer is 1924 x 10 with its border)"""
    got, _, _ = check_bits(ctx, hipmod, R.GAUSSIAN, None, (1920, 6), seed=30)
    assert got[0].shape == (6, 1920, 3)


def test_film_step_window_widened_by_fp32_rounding(ctx, hipmod):
    """box r = 1.5 - 2^-23: floor(r + 0.5) = 1, yet a sample with pFilm exactly q = x + 2 reaches pixel x (x >= 2) because
    fl(x + 2^-23) rounds to x.  The kernel's window must be 2 wide; a 1-wide window gives other sums."""
    r = float(F(1.5) - F(2.0 ** -23))
    _, want, (pf, col, rw, film) = check_bits(ctx, hipmod, R.BOX, r, (48, 24), crop=((8, 8), (48, 24)), seed=31, int_frac=0.6)
    lw, _ = R.prepare(col, rw)
    narrow = R.splat(pf, lw, (film.sample_x0, film.sample_y0), ((8, 8), (48, 24)), r, r, hipmod.film_table(R.BOX, r),
                     extra=0)
    assert not np.array_equal(narrow[1], want[1])


@pytest.mark.parametrize("boxes", [(7,), (7, 5)])
def test_filter_film_end_to_end(ctx, hipmod, oracle, boxes):
    """rpf_filter_film on a buffer whose origin is (-2, -2) (gaussian r = 2 over a 16 x 10 image): filtered colours against
    the oracle, sample colours equal to rpf_filter's, the film outputs equal to the restatement on those colours and close
    to it on the oracle's"""
    W, H, S = 20, 14, 8
    planes = fb.synth_planes(W, H, S, seed=40, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    planes[0] += F(-2)  # pFilm stays inside each sample's own (raster) pixel
    planes[1] += F(-2)
    rw = (0.5 + np.random.default_rng(3).random((H, W, S))).astype(F)
    desc = hipmod.make_desc(W, H, S, boxes=boxes)
    table = hipmod.film_table(R.GAUSSIAN)
    film = hipmod.make_film(((0, 0), (16, 10)), 2.0, table)
    assert (film.sample_x0, film.sample_y0) == (-2, -2)
    srgb, t, w, img = ctx.filter_film(planes, desc, film, ray_weight=rw)
    s2, _, _, c64 = ctx.filter(planes, desc, ray_weight=rw, want_pixels=False, want_colour64=True)
    assert np.array_equal(srgb, s2) and np.array_equal(srgb, c64.astype(F))
    c = None
    for box in boxes:
        c = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box), colour_in=c, debug=False)["colour"]
    assert rel_l2(c64, c) <= 1e-9
    assert rel_l2(c64, planes[2:5].astype(np.float64)) > 1e-3  # the filter did something
    ref_t, ref_w, ref_img, _ = R.film(planes[0:2], srgb, (-2, -2), ((0, 0), (16, 10)), 2.0, 2.0, table, rw)
    assert np.array_equal(t, ref_t) and np.array_equal(w, ref_w) and np.array_equal(img, ref_img)
    _, _, o_img, _ = R.film(planes[0:2], c, (-2, -2), ((0, 0), (16, 10)), 2.0, 2.0, table, rw)
    assert rel_l2(img, o_img.astype(np.float64)) <= 1e-6


def _small(hipmod, S=4):
    W, H = 12, 9
    planes = fb.synth_planes(W, H, S, seed=50)
    film = hipmod.make_film(((0, 0), (W, H)), 0.5, hipmod.film_table(R.BOX), sample_origin=(0, 0))
    return planes, hipmod.make_desc(W, H, S), film


def _refused(ctx, hipmod, planes, desc, film):
    with pytest.raises(hipmod.RpfError) as e:
        ctx.filter_film(planes, desc, film)
    return e.value


def test_filter_film_refusals(ctx, hipmod):
    planes, desc, film = _small(hipmod)
    bad = planes.copy()
    bad[0, 6, 3, 1] = F(3 + 1.25)  # outside [3, 4]
    bad[1, 1, 5, 0] = F(-0.5)      # outside [1, 2], later in the reference's order (x = 5 > 3)
    e = _refused(ctx, hipmod, bad, desc, film)
    assert e.status == hipmod.E_BADARG and "sample 1 of buffer pixel (x=3, y=6)" in str(e)
    bad = planes.copy()
    bad[1, 2, 7, 3] = F(np.nan)
    e = _refused(ctx, hipmod, bad, desc, film)
    assert e.status == hipmod.E_BADARG and "sample 3 of buffer pixel (x=7, y=2)" in str(e)
    for r in (0.0, -1.0, float("inf"), float("nan")):
        f2 = hipmod.make_film(((0, 0), (12, 9)), (0.5, r), hipmod.film_table(R.BOX), sample_origin=(0, 0))
        assert _refused(ctx, hipmod, planes, desc, f2).status == hipmod.E_BADARG
    f2 = hipmod.make_film(((4, 0), (4, 9)), 0.5, hipmod.film_table(R.BOX), sample_origin=(0, 0))
    assert _refused(ctx, hipmod, planes, desc, f2).status == hipmod.E_BADARG
    sub = hipmod.make_desc(12, 9, 4, row_begin=1)
    assert _refused(ctx, hipmod, planes, sub, film).status == hipmod.E_BADARG
    d27 = hipmod.make_desc(12, 9, 4, n_random=4, n_feat=18, plane_dtype=hipmod.PLANES_F16)
    p27 = np.zeros((27, 9, 12, 4), np.float16)
    p27[0:2] = planes[0:2]
    assert _refused(ctx, hipmod, p27, d27, film).status == hipmod.E_UNSUPPORTED
    # the device entry runs the same check
    with pytest.raises(hipmod.RpfError) as e:
        bad = planes[0:2].copy()
        bad[0, 0, 0, 0] = F(-1)
        film_device(ctx, hipmod, bad, np.ones((3, 9, 12, 4)), film)
    assert e.value.status == hipmod.E_BADARG
    ctx.filter_film(planes, desc, film)  # and the context is still usable


def test_filter_film_deterministic_and_host_mirror(ctx, hipmod):
    """two calls give the same bits; the C++ mirror (PlaneFilm with x0, y0 = the sample origin, RPFFilter::FilterAndSplat)
    gives what ctx.filter_film gives"""
    W, H, S = 21, 13, 8
    x0, y0 = -2, -1
    planes = fb.synth_planes(W, H, S, seed=60, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    planes[0] += F(x0)
    planes[1] += F(y0)
    rw_xys = (0.5 + np.random.default_rng(4).random((W, H, S))).astype(F)  # SamplingFilm order [x][y][s]
    rw = np.ascontiguousarray(rw_xys.transpose(1, 0, 2))
    film = hipmod.make_film(((0, 1), (17, 11)), (2.0, 1.5), hipmod.film_table(R.MITCHELL, (2.0, 1.5)), sample_origin=(x0, y0),
                            max_sample_luminance=3.0, scale=2.0)
    desc = hipmod.make_desc(W, H, S, boxes=(7, 5), policy=hipmod.DEGEN_EPS)
    a = ctx.filter_film(planes, desc, film, ray_weight=rw)
    b = ctx.filter_film(planes, desc, film, ray_weight=rw)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    lib = C.CDLL(os.path.join(os.path.dirname(hipmod.LIB_PATH), "librpf_host.so"))
    aos = fb.planes_to_aos(planes)
    boxes = (C.c_int32 * 2)(7, 5)
    err = C.create_string_buffer(256)
    srgb = np.empty((3, H, W, S), F)
    t, w, img = np.empty((10, 17, 3), F), np.empty((10, 17), F), np.empty((10, 17, 3), F)
    mirror_film = hipmod.make_film(((0, 1), (17, 11)), (2.0, 1.5), hipmod.film_table(R.MITCHELL, (2.0, 1.5)), sample_origin=(0, 0),
                                   max_sample_luminance=3.0, scale=2.0)  # the PlaneFilm supplies the origin
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    st = lib.rpf_host_planefilm_film(vp(aos), vp(rw_xys), W, H, S, x0, y0, boxes, 2, 0, hipmod.DEGEN_EPS, 0,
                                     C.byref(mirror_film), vp(srgb), vp(t), vp(w), vp(img), err, 256)
    assert st == 0, err.value
    for u, v in zip(a, (srgb, t, w, img)):
        assert np.array_equal(u, v)
