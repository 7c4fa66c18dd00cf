"""GPU tests of the film step on row slabs: rpf_multi_filter_film (MultiContext.filter_film) against rpf_filter_film on one
context, bit for bit -- nothing in the arithmetic or its order differs, so no tolerance applies -- its refusals and merged
pFilm check, REF_ABORT, determinism, and the one-process-per-GPU geometry (slabs.film_for_slab + rpf_film_splat_device on
slab buffers whose colour halos were refreshed along hip.halo_plan)."""
import numpy as np
import pytest

import pbrt_film_ref as R
from raytracer_rpf_amd import feature_buffer as fb
from raytracer_rpf_amd import slabs

pytestmark = pytest.mark.gpu

F = np.float32
R15 = float(F(1.5) - F(2.0 ** -23))
W, H, S = 20, 26, 8  # the sample film of every case below; H / 3 = 8 rows per slab >= the deepest halo (4)


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def pfilm_with_edges(W, H, S, origin, seed, int_frac):
    """pFilm planes in raster coordinates, q + u; a share int_frac of the samples sits exactly on q or on q + 1"""
    rng = np.random.default_rng(seed)
    q = [F(origin[0]) + np.arange(W, dtype=F)[None, :, None], F(origin[1]) + np.arange(H, dtype=F)[:, None, None]]
    u = rng.random((2, H, W, S)).astype(F)
    pick = rng.random((2, H, W, S))
    u[pick < int_frac / 2] = F(0)
    u[(pick >= int_frac / 2) & (pick < int_frac)] = F(1)
    return np.stack([(q[a] + u[a]).astype(F) for a in range(2)])


# name -> (filter, radius, pixel bounds, sample origin, boxes, film keywords, ray weights, share of pFilm on pixel edges)
CASES = {
    "gaussian_r2_box7": (R.GAUSSIAN, 2.0, ((0, 0), (16, 22)), (-2, -2), (7,), {}, False, None),
    "gaussian_r2_box7_5": (R.GAUSSIAN, 2.0, ((0, 0), (16, 22)), (-2, -2), (7, 5), {}, False, None),
    "sinc_r4": (R.SINC, 4.0, ((0, 0), (12, 18)), (-4, -4), (7,), {}, False, None),          # film halo 4 > box halo 3
    "box_r05": (R.BOX, 0.5, ((0, 0), (20, 26)), (0, 0), (7, 5), {}, False, None),
    "mitchell_crop": (R.MITCHELL, (2.0, 1.5), ((3, 5), (13, 20)), (-2, -1), (7, 5),
                      dict(max_sample_luminance=3.0, scale=2.0), True, None),
    "box_r15_widened": (R.BOX, R15, ((0, 0), (18, 24)), (-1, -1), (7,), {}, False, 0.6),
}


def make_case(hipmod, name, seed=70):
    kind, radius, bounds, origin, boxes, kw, with_rw, int_frac = CASES[name]
    rx, ry = hipmod._radii(kind, radius)
    planes = fb.synth_planes(W, H, S, seed=seed, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    if int_frac is None:
        planes[0] += F(origin[0])  # pFilm stays inside each sample's own raster pixel
        planes[1] += F(origin[1])
    else:
        planes[0:2] = pfilm_with_edges(W, H, S, origin, seed, int_frac)
    rw = (0.5 + np.random.default_rng(seed + 1).random((H, W, S))).astype(F) if with_rw else None
    table = hipmod.film_table(kind, (rx, ry))
    film = hipmod.make_film(bounds, (rx, ry), table, sample_origin=origin, **kw)
    desc = hipmod.make_desc(W, H, S, boxes=boxes, policy=hipmod.DEGEN_EPS)
    return planes, desc, film, rw, table


_one_context = {}


def one_context(ctx, hipmod, name):
    if name not in _one_context:
        planes, desc, film, rw, _ = make_case(hipmod, name)
        _one_context[name] = ctx.filter_film(planes, desc, film, ray_weight=rw)
    return _one_context[name]


def need_devices(devices):
    import torch
    if max(devices) >= torch.cuda.device_count():
        # two different ordinals take the hipMemcpyPeerAsync branch of the halo refresh: it needs a second GPU
        pytest.skip("needs %d visible GPUs" % (max(devices) + 1))


def assert_same(got, want, equal_nan=False):
    for g, w_, name in zip(got, want, ("sample_rgb", "contribSum", "filterWeightSum", "image")):
        assert g.shape == w_.shape and g.dtype == w_.dtype
        assert np.array_equal(g, w_, equal_nan=equal_nan), (name, np.argwhere(g != w_)[:5])


@pytest.mark.parametrize("devices", [(0,), (0, 0), (0, 0, 0), (0, 1), (0, 1, 0)])
@pytest.mark.parametrize("name", list(CASES))
def test_multi_filter_film_equals_one_context(ctx, hipmod, name, devices):
    need_devices(devices)
    planes, desc, film, rw, _ = make_case(hipmod, name)
    want = one_context(ctx, hipmod, name)
    hy = hipmod.film_window(desc, film)[1]
    for g in range(len(devices)):  # every slab owns at least the depth, so the call is not refused
        slabs.slab_for(H, len(devices), g, max(3, hy))
    with hipmod.MultiContext(list(devices)) as mc:
        got = mc.filter_film(planes, desc, film, ray_weight=rw)
        c = mc.counters()
    assert_same(got, want)
    assert (got[2] != 0).any() and np.isfinite(got[3]).all()
    assert c.samples_filtered == W * H * S * desc.n_box and c.nonfinite_pixels == 0 and c.first_bad_pixel == -1
    assert rel_l2(got[0], planes[2:5].astype(np.float64)) > 1e-3  # the filter did something


def test_multi_filter_film_against_oracle_and_restatement(ctx, hipmod, oracle):
    """the outside yardsticks of test_filter_film_end_to_end on three slabs: colours against the oracle's pass chain, the
    film outputs equal to the restatement on the returned sample colours"""
    name = "mitchell_crop"
    kind, radius, bounds, origin, boxes, kw, _, _ = CASES[name]
    planes, desc, film, rw, table = make_case(hipmod, name)
    with hipmod.MultiContext([0, 0, 0]) as mc:
        srgb, t, w, img = mc.filter_film(planes, desc, film, ray_weight=rw)
    _, _, _, c64 = ctx.filter(planes, desc, ray_weight=rw, want_pixels=False, want_colour64=True)
    assert np.array_equal(srgb, c64.astype(F))
    c = None
    for box in boxes:
        c = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=oracle.DEGEN_EPS), colour_in=c, debug=False)["colour"]
    assert rel_l2(c64, c) <= 1e-9
    # srgb is c64 rounded to fp32: half an ulp, 2^-24 relative per element, on top of the bar above
    assert rel_l2(srgb, c) <= 2.0 ** -24 + 1e-9
    assert rel_l2(srgb, planes[2:5].astype(np.float64)) > 1e-3
    rx, ry = hipmod._radii(kind, radius)
    ref_t, ref_w, ref_img, n_clamped = R.film(planes[0:2], srgb, origin, bounds, rx, ry, table, rw, kw["max_sample_luminance"], kw["scale"])
    assert np.array_equal(t, ref_t) and np.array_equal(w, ref_w) and np.array_equal(img, ref_img)


def test_multi_filter_film_crop_window_inside_one_slab(ctx, hipmod):
    """output pixels that lie within the rows the middle slab owns: the other slabs have no film work, and the result is
    one context's"""
    planes, desc, _, _, table = make_case(hipmod, "gaussian_r2_box7_5")
    film = hipmod.make_film(((2, 8), (14, 13)), 2.0, table, sample_origin=(-2, -2))
    parts = [slabs.film_for_slab(film, slabs.slab_for(H, 3, g, 3), H) for g in range(3)]
    assert parts[0] is None and parts[2] is None and parts[1][1] == (0, 5)
    want = ctx.filter_film(planes, desc, film)
    with hipmod.MultiContext([0, 0, 0]) as mc:
        got = mc.filter_film(planes, desc, film)
    assert got[1].shape == (5, 12, 3)
    assert_same(got, want)
    assert (got[2] != 0).all()


def _refusal(call):
    with pytest.raises(Exception) as e:
        call()
    assert hasattr(e.value, "status"), e.value
    return e.value


def test_multi_filter_film_refusals(ctx, hipmod):
    # a slab thinner than the film halo: sinc r = 4 needs 4 rows, H / devices = 3; the box halo (3) alone fits
    w9, h9 = 12, 9
    p9 = fb.synth_planes(w9, h9, S, seed=71, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    p9[0] += F(-4)
    p9[1] += F(-4)
    d9 = hipmod.make_desc(w9, h9, S, boxes=(7,), policy=hipmod.DEGEN_EPS)
    f9 = hipmod.make_film(((0, 0), (4, 1)), 4.0, hipmod.film_table(R.SINC), sample_origin=(-4, -4))
    assert hipmod.film_window(d9, f9) == (4, 4)
    with hipmod.MultiContext([0, 0, 0]) as mc:
        e = _refusal(lambda: mc.filter_film(p9, d9, f9))
        assert e.status == hipmod.E_BADARG and "thinner than the halo" in str(e) and "film" in str(e)
        s9, _, st = mc.filter(p9, d9)
        assert st == hipmod.OK
        assert np.array_equal(s9, ctx.filter(p9, d9)[0])

    planes, desc, film, rw, _ = make_case(hipmod, "gaussian_r2_box7")
    with hipmod.MultiContext([0, 0, 0]) as mc:   # slabs own rows [0, 8), [8, 17), [17, 26)
        # two offenders: the earlier one in the reference's order (smaller x) in the LAST slab, the later one in the first
        bad = planes.copy()
        bad[0, 22, 3, 1] = F(-2 + 3 + 1.25)
        bad[1, 2, 11, 0] = F(-9.5)
        e1, e2 = _refusal(lambda: ctx.filter_film(bad, desc, film)), _refusal(lambda: mc.filter_film(bad, desc, film))
        assert e1.status == e2.status == hipmod.E_BADARG
        assert "sample 1 of buffer pixel (x=3, y=22)" in str(e1) and str(e2) == str(e1)
        # an offender in a row that one slab holds as halo and the next one owns (row 8), NaN; a later one elsewhere
        bad = planes.copy()
        bad[1, 8, 6, 5] = F(np.nan)
        bad[0, 1, 7, 0] = F(40)
        e1, e2 = _refusal(lambda: ctx.filter_film(bad, desc, film)), _refusal(lambda: mc.filter_film(bad, desc, film))
        assert e1.status == e2.status == hipmod.E_BADARG
        assert "sample 5 of buffer pixel (x=6, y=8)" in str(e1) and str(e2) == str(e1)
        # the same pixel column: the row decides, and the earlier row is the last owned row of slab 0 (halo of slab 1)
        bad = planes.copy()
        bad[0, 7, 9, 2] = F(-5)
        bad[0, 18, 9, 0] = F(-5)
        e1, e2 = _refusal(lambda: ctx.filter_film(bad, desc, film)), _refusal(lambda: mc.filter_film(bad, desc, film))
        assert "sample 2 of buffer pixel (x=9, y=7)" in str(e1) and str(e2) == str(e1)
        # what film_setup refuses for the whole frame, with its status
        for r in (0.0, float("nan")):
            f2 = hipmod.make_film(((0, 0), (16, 22)), (2.0, r), hipmod.film_table(R.GAUSSIAN), sample_origin=(-2, -2))
            assert _refusal(lambda: mc.filter_film(planes, desc, f2)).status == hipmod.E_BADARG
        f2 = hipmod.make_film(((4, 0), (4, 9)), 2.0, hipmod.film_table(R.GAUSSIAN), sample_origin=(-2, -2))
        assert _refusal(lambda: mc.filter_film(planes, desc, f2)).status == hipmod.E_BADARG
        sub = hipmod.make_desc(W, H, S, row_begin=1)
        assert _refusal(lambda: mc.filter_film(planes, sub, film)).status == hipmod.E_BADARG
        d27 = hipmod.make_desc(W, H, S, n_random=4, n_feat=18, plane_dtype=hipmod.PLANES_F16)
        p27 = np.zeros((27, H, W, S), np.float16)
        p27[0:2] = planes[0:2]
        assert _refusal(lambda: mc.filter_film(p27, d27, film)).status == hipmod.E_UNSUPPORTED
        # and the multi context is still usable
        assert_same(mc.filter_film(planes, desc, film, ray_weight=rw), one_context(ctx, hipmod, "gaussian_r2_box7"))


def test_multi_filter_film_ref_abort_nonfinite(ctx, hipmod, oracle):
    """a constant normal under REF_ABORT (0 / 0): the status, the merged counters, and the film step still runs -- the four
    outputs, NaNs included, are one context's"""
    w, h = 12, 16
    planes = fb.synth_planes(w, h, S, seed=5)
    planes[7:10] = np.float32([0.0, 0.0, 1.0])[:, None, None, None]
    want_o = oracle.filter_pass(planes, oracle.make_desc(w, h, S, box=7))
    desc = hipmod.make_desc(w, h, S)
    film = hipmod.make_film(((0, 0), (w, h)), 0.5, hipmod.film_table(R.BOX), sample_origin=(0, 0))
    want = ctx.filter_film(planes, desc, film, allow_nonfinite=True)
    c1 = ctx.counters()
    assert c1.nonfinite_pixels > 0
    with hipmod.MultiContext([0, 0]) as mc:
        e = _refusal(lambda: mc.filter_film(planes, desc, film))
        assert e.status == hipmod.E_NONFINITE
        got = mc.filter_film(planes, desc, film, allow_nonfinite=True)
        c2 = mc.counters()
    assert c2.nonfinite_pixels == want_o["nonfinite_pixels"] == c1.nonfinite_pixels
    assert c2.first_bad_pixel == want_o["first_bad_pixel"] == c1.first_bad_pixel
    assert np.isnan(got[0]).any() and np.isnan(got[1]).any()  # (WriteImage's max(0, v) turns a NaN pixel into 0)
    assert_same(got, want, equal_nan=True)


def test_multi_filter_film_deterministic(hipmod):
    planes, desc, film, rw, _ = make_case(hipmod, "mitchell_crop")
    with hipmod.MultiContext([0, 0, 0]) as mc:
        a = mc.filter_film(planes, desc, film, ray_weight=rw)
        b = mc.filter_film(planes, desc, film, ray_weight=rw)
    assert_same(a, b)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["gaussian_r2_box7", "sinc_r4"])
def test_one_process_per_gpu_geometry_on_the_device(ctx, hipmod, name, world):
    """what a rank of the one-process-per-GPU path does, without torch.distributed: the image cut into slab buffers as
    slabs.slab_for(H, world, rank, max(box halo, film halo)) gives them, one pass per slab with rpf_filter_device, the
    colour halos refreshed by plain tensor copies along hip.halo_plan, then slabs.film_for_slab + rpf_film_splat_device
    per slab: the assembled outputs are rpf_filter_film's on the whole frame"""
    import torch
    planes, desc, film, _, _ = make_case(hipmod, name)
    rw = (0.5 + np.random.default_rng(9).random((H, W, S))).astype(F)
    want = ctx.filter_film(planes, desc, film, ray_weight=rw)
    depth = max(fb.halo_rows(7), slabs.film_halo_rows(desc, film))
    plan_slabs, copies = hipmod.halo_plan(H, world, depth)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    bufs = []
    for rank in range(world):
        slab = slabs.slab_for(H, world, rank, depth)
        assert tuple(slab) == tuple(plan_slabs[rank])
        h_buf, r0, r1 = slabs.buffer_rows(slab)
        lo = slab.row0 - slab.halo_top
        dp = torch.from_numpy(np.ascontiguousarray(planes[:, lo:lo + h_buf])).to(dev)
        drw = torch.from_numpy(np.ascontiguousarray(rw[lo:lo + h_buf])).to(dev)
        dc = dp[2:5].to(torch.float64).contiguous()
        d = hipmod.make_desc(W, h_buf, S, boxes=(7,), row_begin=r0, row_end=r1, policy=hipmod.DEGEN_EPS)
        ctx.filter_device(d, dp.data_ptr(), dc.data_ptr(), stream)
        bufs.append((slab, dp, drw, dc))
    for src, src_row, dst, dst_row, rows in copies:  # a neighbour's owned rows -> this slab's halo
        bufs[dst][3][:, dst_row:dst_row + rows].copy_(bufs[src][3][:, src_row:src_row + rows])
    ny, nx = film.py1 - film.py0, film.px1 - film.px0
    tile = torch.full((ny, nx, 3), float("nan"), dtype=torch.float32, device=dev)
    wsum = torch.full((ny, nx), float("nan"), dtype=torch.float32, device=dev)
    img = torch.full((ny, nx, 3), float("nan"), dtype=torch.float32, device=dev)
    srgb = np.empty((3, H, W, S), F)
    for slab, dp, drw, dc in bufs:
        h_buf, r0, r1 = slabs.buffer_rows(slab)
        srgb[:, slab.row0:slab.row1] = dc[:, r0:r1].float().cpu().numpy()
        part = slabs.film_for_slab(film, slab, H)
        assert part is not None
        f, (o0, o1) = part
        ctx.film_splat_device(hipmod.make_desc(W, h_buf, S), f, dp.data_ptr(), dc.data_ptr(), drw.data_ptr(),
                              tile[o0:o1].data_ptr(), wsum[o0:o1].data_ptr(), img[o0:o1].data_ptr(), stream)
    torch.cuda.synchronize()
    assert_same((srgb, tile.cpu().numpy(), wsum.cpu().numpy(), img.cpu().numpy()), want)
