"""GPU parity: the HIP path (through the C ABI) against the oracle on identical seeded feature buffers.

Bars: bit-exact for integer/index work (neighbourhood membership and order, histogram bin ids) and for the
fp64 statistics whose rounding decides them; MI / alpha / beta within 1e-10; filtered RGB <= 1e-4 relative
L2 (BASELINE.json north_star), in practice ~1e-13.

That norm is taken over a whole frame, and at the reference's sigma seed the filter is close to the identity on most frames
here: the colours then only show that nothing was broken.  Stage 4 is held sample by sample, on filter-active frames of every
route, by tests/test_stage4_per_sample_gpu.py against the bar of tests/stage4_bars.py.
"""
import numpy as np
import pytest

from raytracer_rpf_amd import feature_buffer as fb

pytestmark = pytest.mark.gpu

REL_L2_BAR = 1e-4  # north_star: "<= 1e-4 relative L2 on identical feature buffers"


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def check_pass(got, want, rows=None, ab_rtol=1e-9, sample_bar=None):
    """sample_bar: None, or the bar of tests/stage4_bars.py -- in addition to everything below, every finite colour lies within
    sample_bar * max finite |want colour| of the oracle's (valid where alpha, beta and W_r_c are the oracle's bits: their 1e-9
    slack, times an exponent of up to 745, would otherwise be what is measured)"""
    sl = slice(None) if rows is None else slice(*rows)
    assert (got["nbhd_size"][sl] == want["nbhd_size"][sl]).all()
    assert (got["member_hash"][sl] == want["member_hash"][sl]).all()
    assert (got["bin_hash"][sl] == want["bin_hash"][sl]).all()
    # sequential-order statistics are bit-identical
    assert np.array_equal(got["mean"][sl], want["mean"][sl], equal_nan=True)
    assert np.array_equal(got["stddev"][sl], want["stddev"][sl], equal_nan=True)
    # MI is evaluated over integer counts with a k*ln(k) table instead of per-cell log(): ~1e-15 absolute
    np.testing.assert_allclose(got["mi"][sl], want["mi"][sl], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got["alpha"][sl], want["alpha"][sl], rtol=ab_rtol, atol=1e-12)
    np.testing.assert_allclose(got["beta"][sl], want["beta"][sl], rtol=ab_rtol, atol=1e-12)
    np.testing.assert_allclose(got["wrc"][sl], want["wrc"][sl], rtol=ab_rtol, atol=1e-12)
    r = rel_l2(got["colour"], want["colour"])
    assert r <= REL_L2_BAR, r
    if sample_bar is not None:
        fin = np.isfinite(got["colour"]) & np.isfinite(want["colour"])
        worst = float(np.abs(got["colour"][fin] - want["colour"][fin]).max())
        cmax = float(np.abs(want["colour"][np.isfinite(want["colour"])]).max())
        assert worst <= sample_bar * cmax, (worst / cmax, sample_bar)
    return r


def test_uniform_divisor_division_is_exact(ctx):
    """stage 3a divides by per-column constants with a hoisted reciprocal; it must equal IEEE a/b bit for bit"""
    assert ctx.selftest_udiv(200_000_000, seed=1, mode=0) == 0
    assert ctx.selftest_udiv(50_000_000, seed=2, mode=1) == 0


def test_stage1a_pixel_stats_bit_exact(ctx, hipmod, oracle):
    W, H, S = 37, 21, 8
    planes = fb.synth_planes(W, H, S, seed=3)
    planes[10:13] += 1000.0  # large-mean / small-variance positions
    m, s = ctx.pixel_stats(planes, hipmod.make_desc(W, H, S))
    mo, so = oracle.pixel_stats(planes, oracle.make_desc(W, H, S))
    assert np.array_equal(m, mo)
    assert np.array_equal(s, so, equal_nan=True)


def test_config1_shape_small_neighbourhoods_400x400x8(ctx, hipmod, oracle):
    """BASELINE configs[0] stand-in (400x400, 8 spp, EPS policy): a captured killeroo buffer keeps N = S for ~94 % of its
    pixels and the reference itself aborts on it (F2); pbrt cannot be built here, so the stand-in is the
    seeded generator with an in-pixel jitter small enough that the 3-sigma test rejects nearly every neighbour.  Every
    stage output of the full frame against the oracle."""
    W, H, S = 400, 400, 8
    for sf, lo, hi in ((1e-5, 8.0, 30.0), (3e-3, 20.0, 200.0)):
        planes = fb.synth_planes(W, H, S, seed=1, sigma_f=sf, sigma_c=0.01, mode="smooth")
        got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_EPS), box=7)
        want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7, policy=oracle.DEGEN_EPS))
        check_pass(got, want)
        assert got["nonfinite_pixels"] == want["nonfinite_pixels"] == 0
        mean_n = want["sum_nbhd"] / (W * H)
        assert lo <= mean_n <= hi, mean_n


def test_config3_shape_four_passes_1080p16(ctx, hipmod, oracle):
    """BASELINE configs[2] stand-in: 1920x1080x16 spp, four passes {7,7,5,5}, EPS policy (the reference enables {7}
    only, rpf.cpp:767; the list is this build's).  After EVERY pass: bitwise determinism, every colour inside the
    convex hull of its window's input colours, and the oracle on three full-width rows fed with the colours the
    previous pass left (carried as doubles, rpf.cpp:732)."""
    import torch
    W, H, S = 1920, 1080, 16
    dev = torch.device("cuda", 0)
    planes = fb.synth_planes(W, H, S, xp=fb.torch_backend(dev), mode="clustered", sigma_f=1e-3, sigma_c=0.01).contiguous()
    col = planes[2:5].to(torch.float64).contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    pad = torch.nn.functional.pad
    r0, R = 531, 3
    moved = 0.0
    for box in (7, 7, 5, 5):
        b = (box - 1) // 2
        desc = hipmod.make_desc(W, H, S, boxes=(box,), policy=hipmod.DEGEN_EPS)
        outs = []
        for _ in range(2):
            c = col.clone()
            ctx.filter_device(desc, planes.data_ptr(), c.data_ptr(), stream)
            outs.append(c)
        torch.cuda.synchronize()
        out = outs[0]
        assert torch.equal(out, outs[1])
        cnt = ctx.counters()
        assert cnt.nonfinite_pixels == 0 and S <= cnt.max_nbhd <= box * box * S
        cmin, cmax = col.amin(dim=3), col.amax(dim=3)
        wmin = -torch.nn.functional.max_pool2d(pad(-cmin, (b, b, b, b), value=-1e30), 2 * b + 1, stride=1)
        wmax = torch.nn.functional.max_pool2d(pad(cmax, (b, b, b, b), value=-1e30), 2 * b + 1, stride=1)
        assert bool((out >= wmin[..., None] - 1e-9).all()) and bool((out <= wmax[..., None] + 1e-9).all())
        host = planes[:, r0 - b:r0 + R + b].cpu().numpy()
        cin = col[:, r0 - b:r0 + R + b].cpu().numpy()
        want = oracle.filter_pass(host, oracle.make_desc(W, 2 * b + R, S, box=box, row_begin=b, row_end=b + R,
                                                         policy=oracle.DEGEN_EPS), colour_in=cin, debug=False)["colour"]
        got = out[:, r0:r0 + R].cpu().numpy()
        assert rel_l2(got, want[:, b:b + R]) <= REL_L2_BAR
        moved = max(moved, rel_l2(got, cin[:, b:b + R]))
        col = out
    assert moved > 1e-3   # the passes did something on these rows


def test_config4_shape_full_rank_slab_3840x276x32(ctx, hipmod, oracle):
    """BASELINE configs[3]: 3840x2160x32 spp row-tiled over 8 GPUs -- the buffer of an interior rank: 270 owned rows
    plus 3 halo rows either side (slabs.slab_for(2160, 8, 4, 3)), filtered as that rank filters it: determinism,
    neighbourhood bounds, hull bounds, halo rows untouched, and the oracle on one full-width owned row."""
    import torch
    from raytracer_rpf_amd import slabs
    W, S, b = 3840, 32, 3
    slab = slabs.slab_for(2160, 8, 4, b)
    H, rb, re = slabs.buffer_rows(slab)
    assert (H, rb, re) == (276, 3, 273)
    dev = torch.device("cuda", 0)
    planes = fb.synth_planes(W, H, S, row0=slab.row0 - slab.halo_top, xp=fb.torch_backend(dev), mode="smooth",
                             sigma_f=0.05, sigma_c=1e-4).contiguous()
    col0 = planes[2:5].to(torch.float64).contiguous()
    desc = hipmod.make_desc(W, H, S, row_begin=rb, row_end=re, policy=hipmod.DEGEN_EPS)
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    for _ in range(2):
        c = col0.clone()
        ctx.filter_device(desc, planes.data_ptr(), c.data_ptr(), stream)
        outs.append(c)
    torch.cuda.synchronize()
    out = outs[0]
    assert torch.equal(out, outs[1])
    cnt = ctx.counters()
    assert cnt.samples_filtered == 270 * W * S and cnt.nonfinite_pixels == 0 and S <= cnt.max_nbhd <= 49 * S
    assert cnt.sum_nbhd > 20 * S * W * 270          # the large-neighbourhood regime (four-wave kernels)
    assert torch.equal(out[:, :rb], col0[:, :rb]) and torch.equal(out[:, re:], col0[:, re:])
    pad = torch.nn.functional.pad
    cmin, cmax = col0.amin(dim=3), col0.amax(dim=3)
    wmin = -torch.nn.functional.max_pool2d(pad(-cmin, (b, b, b, b), value=-1e30), 2 * b + 1, stride=1)
    wmax = torch.nn.functional.max_pool2d(pad(cmax, (b, b, b, b), value=-1e30), 2 * b + 1, stride=1)
    assert bool((out >= wmin[..., None] - 1e-9).all()) and bool((out <= wmax[..., None] + 1e-9).all())
    r0 = 140
    host = planes[:, r0 - b:r0 + 1 + b].cpu().numpy()
    want = oracle.filter_pass(host, oracle.make_desc(W, 2 * b + 1, S, box=7, row_begin=b, row_end=b + 1,
                                                     policy=oracle.DEGEN_EPS), debug=False)["colour"][:, b:b + 1]
    assert rel_l2(out[:, r0:r0 + 1].cpu().numpy(), want) <= REL_L2_BAR


def _independent_columns(n, bins):
    """two columns of n values whose `bins`-bin histograms are EXACTLY independent: a has n/bins samples per bin; inside
    every a-bin one sample sits in each of b's higher bins and the rest in b's first: J_ij * n == hx_i * hy_j on every cell"""
    blk = n // bins
    vals = np.arange(bins) / (bins - 1.0)
    a = np.repeat(vals, blk)
    per = [blk - (bins - 1)] + [1] * (bins - 1)
    b = np.tile(np.repeat(vals, per), bins)
    return a, b


def _assert_ref_abort_parity(got, ref, hipmod, indep):
    """REF_ABORT parity on a frame with in-band MI tables: identical status / NaN pattern, identical zero / non-zero
    pattern AND bits of the in-band MI values, every stage output of check_pass where the colours are finite"""
    assert (got["status"] == hipmod.E_NONFINITE) == (ref["status"] == 1)
    assert got["nonfinite_pixels"] == ref["nonfinite_pixels"] and got["first_bad_pixel"] == ref["first_bad_pixel"]
    gi, ri = got["mi"][..., indep], ref["mi"][..., indep]
    assert np.array_equal(gi == 0, ri == 0)
    assert np.array_equal(gi, ri)              # the reference's own residue, bit for bit (rpf_reflog.h)
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(ref["colour"]))
    for k in ("nbhd_size", "member_hash", "bin_hash"):
        assert (got[k] == ref[k]).all()
    assert np.array_equal(got["mean"], ref["mean"]) and np.array_equal(got["stddev"], ref["stddev"])
    np.testing.assert_allclose(got["mi"], ref["mi"], rtol=0, atol=1e-11)
    for k in ("alpha", "beta", "wrc"):        # the weights are quotients OF residues: equal MI bits give equal weights
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-9, atol=1e-12, equal_nan=True)
    fin = np.isfinite(ref["colour"])
    assert rel_l2(got["colour"][fin], ref["colour"][fin]) <= REL_L2_BAR


@pytest.mark.parametrize("S,bins", [(15, 3), (12, 3), (24, 4)])
def test_exactly_independent_table_at_non_power_of_two_n(ctx, hipmod, oracle, S, bins):
    """One pixel, N = S not a power of two, B = floor(sqrt(N)): two column pairs whose joint histograms are EXACTLY
    independent (J_ij * N == hx_i * hy_j).  For N a power of two mi.cpp returns an exact 0 for such a table; otherwise its
    quotients pXY / (pX * pY) round to 1 +- 2.2e-16 and it returns rounding residue, which rpf.cpp:465/470 then divide by
    each other.  REF_ABORT promises the reference's value: the resident kernel hands such a pixel to
    generic::filter_pixel_kernel, which evaluates mi.cpp:66-86 term by term (round 2 returned 0 here and recorded the
    deviation).  EPS: both sides return exactly 0 (the residue contract).  S = 24 takes the size-binned route."""
    W, H = 1, 1
    assert int(np.sqrt(S)) == bins
    a, b = _independent_columns(S, bins)
    rng = np.random.default_rng(3)
    planes = np.empty((19, H, W, S), np.float32)
    for c in range(19):
        planes[c, 0, 0] = rng.permutation(S) / (S - 1.0)                # generic columns
    planes[5, 0, 0], planes[6, 0, 0] = a, b                             # r0, r1
    planes[7, 0, 0], planes[8, 0, 0] = b, a                             # f0, f1
    pa, pb = oracle.pair_table()
    indep = [i for i in range(96) if (pa[i], pb[i]) in ((7, 5), (8, 6))]
    assert len(indep) == 2
    ref = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7))
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S), box=7, allow_nonfinite=True)
    assert (np.abs(ref["mi"][0, 0, indep]) < 1e-15).all()
    assert ctx.counters().redo_pixels == 1
    _assert_ref_abort_parity(got, ref, hipmod, indep)
    e_ref = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7, policy=oracle.DEGEN_EPS))
    e_got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_EPS), box=7)
    assert (e_ref["mi"][0, 0, indep] == 0).all() and (e_got["mi"][0, 0, indep] == 0).all()
    assert ctx.counters().redo_pixels == 0
    check_pass(e_got, e_ref)


def test_independent_tables_in_every_size_class_ref_abort(ctx, hipmod, oracle):
    """An 11x11 frame at 15 spp, box 9, in which EVERY pixel's neighbourhood holds an exactly independent (f0, r0) table at
    a non-power-of-two N: each pixel carries a three-valued column a (5, 5, 5) against a column b with (3, 1, 1) samples per
    a-value, and every other feature is a permutation of the same 15 values in every pixel (same mean and sigma: all
    neighbours pass the 3-sigma test), so a window is a union of whole pixels -- N = 15 * (25 ... 81) = 375 ... 1215: the
    one-wave K = 7 and K = 13 classes and the split route (chains / bins + MI / weights) of the K = 25 class all meet the
    redo path, and pX = 1/3 against pY = 3/5 makes the reference's quotients inexact (real residue).  The whole frame must
    equal the oracle under REF_ABORT: status, NaN pattern, residue bits, weights, colours."""
    W, H, S, box = 11, 11, 15, 9
    rng = np.random.default_rng(17)
    planes = rng.permuted(np.broadcast_to(np.linspace(0.4, 0.6, S), (19, H, W, S)), axis=3).astype(np.float32)
    planes[0] = (np.arange(W)[None, :, None] + rng.random((H, W, S))).astype(np.float32)
    planes[1] = (np.arange(H)[:, None, None] + rng.random((H, W, S))).astype(np.float32)
    a, b = _independent_columns(S, 3)
    planes[5], planes[7] = a.astype(np.float32), b.astype(np.float32)   # r0, f0: the same pattern in every pixel
    pa, pb = oracle.pair_table()
    indep = [i for i in range(96) if (pa[i], pb[i]) == (7, 5)]
    ref = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box))
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S), box=box, allow_nonfinite=True)
    n = ref["nbhd_size"]
    assert n.min() == 25 * S and n.max() == 81 * S and (n == 81 * S).sum() == 9      # whole-pixel windows
    ri = ref["mi"][..., indep]
    assert (np.abs(ri) < 1e-14).all() and (ri != 0).sum() > 20                        # residue, not zeros
    assert ctx.counters().redo_pixels == int(((n & (n - 1)) != 0).sum()) == W * H
    _assert_ref_abort_parity(got, ref, hipmod, indep)


@pytest.mark.parametrize("W,H,S,box,mode,sf,sc", [
    (24, 16, 8, 7, "clustered", 1e-3, 0.01),
    (24, 16, 8, 7, "smooth", 0.05, 1e-4),
    (20, 12, 16, 7, "clustered", 1e-3, 0.01),
    (19, 13, 8, 5, "clustered", 1e-3, 0.01),
    (9, 7, 4, 3, "smooth", 0.05, 1e-4),
    (5, 4, 8, 7, "smooth", 0.05, 1e-4),      # frame smaller than the box: every window is clipped
    (16, 10, 1, 7, "smooth", 0.05, 1e-4),    # one sample per pixel
    (12, 8, 32, 7, "smooth", 0.05, 1e-4),
])
def test_filter_pass_vs_oracle(ctx, hipmod, oracle, W, H, S, box, mode, sf, sc):
    planes = fb.synth_planes(W, H, S, seed=11, sigma_f=sf, sigma_c=sc, mode=mode)
    # EPS policy: small / clipped neighbourhoods hit 0/0 in the reference and box 3 has sigma_p = 0
    pol_h, pol_o = (hipmod.DEGEN_EPS, oracle.DEGEN_EPS)
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=pol_h), box=box)
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=pol_o))
    check_pass(got, want)
    assert got["nonfinite_pixels"] == want["nonfinite_pixels"]


def test_filter_is_active_on_clustered_buffer(ctx, hipmod, oracle):
    """the parity above is not vacuous: the filter moves the colours measurably on this buffer"""
    W, H, S = 24, 16, 8
    planes = fb.synth_planes(W, H, S, seed=11, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S), box=7)
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7))
    cin = planes[2:5].astype(np.float64)
    assert rel_l2(want["colour"], cin) > 1e-3
    assert rel_l2(got["colour"], cin) > 1e-3
    assert check_pass(got, want) < 1e-9
    assert got["status"] == hipmod.OK


def test_ref_abort_status_on_constant_feature(ctx, hipmod, oracle):
    """a feature constant in the neighbourhood gives 0/0 -> NaN; the reference exits (rpf.cpp:702-705),
    the ABI returns RPF_E_NONFINITE and names the lowest offending pixel"""
    W, H, S = 12, 8, 8
    planes = fb.synth_planes(W, H, S, seed=5)
    planes[7:10] = np.float32([0.0, 0.0, 1.0])[:, None, None, None]  # flat surface: constant normal
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S), box=7, allow_nonfinite=True)
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7))
    assert want["status"] == 1 and got["status"] == hipmod.E_NONFINITE
    assert got["nonfinite_pixels"] == want["nonfinite_pixels"] > 0
    assert got["first_bad_pixel"] == want["first_bad_pixel"]
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(want["colour"]))
    # the same buffer completes under the EPS policy, identically on both sides
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_EPS), box=7)
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7, policy=oracle.DEGEN_EPS))
    # EPS residue contract (oracle/rpf_oracle.c mi_scratch, rpf_kernels.hip stage 3b): an MI whose fixed-point integer
    # form lies inside the table's rounding band is exactly 0 on both sides, so alpha / beta / W_r_c agree to rounding
    check_pass(got, want)
    assert np.isfinite(got["colour"]).all()


@pytest.mark.parametrize("W,H,S,box,sf,flat,policy", [
    (40, 24, 8, 7, 1e-5, 0.0, 1),    # N = 8 ... 40: 8 / 4 / 2 / 1 pixels per wave, unbinned route (re-routed by the fused kernel)
    (40, 24, 8, 7, 3e-3, 0.0, 1),    # N up to ~100: some pixels stay on the one-wave kernels, the small ones are re-routed
    (40, 24, 8, 7, 0.05, 0.94, 1),   # the captured-buffer regime: 94 % flat-quad pixels with N = S = 8, the rest large
    (33, 17, 4, 7, 1e-5, 0.0, 1),    # S = 4: N = 4 ... 18; B = 2 at N < 9
    (30, 14, 16, 7, 1e-5, 0.0, 1),   # 16 spp: size-binned route, lists from classify_kernel; N = 18 ... 73
    (24, 10, 32, 5, 1e-5, 0.7, 1),   # 32 spp, box 5: two pixels per wave (N = 32) and one
    (12, 8, 64, 5, 1e-6, 0.7, 1),    # 64 spp: N = 64 exactly -> one pixel per wave on the packed kernel (G = 64)
    (21, 13, 1, 7, 0.05, 0.0, 1),    # one sample per pixel: sigma = 0, N = 1, B = 1
    (40, 24, 8, 7, 1e-5, 0.0, 0),    # REF_ABORT on a buffer that completes
    (40, 24, 8, 7, 0.05, 0.94, 0),   # REF_ABORT on the captured-buffer regime: the reference aborts; same NaN pattern
    (19, 4, 3, 13, 0.02, 0.5, 0),    # box 13 x 3 spp: 507 candidates -> the unbinned route's K = 13 kernel re-routes too (a fuzz find:
                                     # it did not, and NaN pixels of N = S were counted twice)
])
def test_packed_small_neighbourhood_kernels(ctx, hipmod, oracle, W, H, S, box, sf, flat, policy):
    """N <= 64: the packed kernels (several pixels per wavefront, popcount histograms; rpf_packed_impl.inc) against the
    oracle AND against the one-wave-per-pixel kernels (option "packed" = 0): every stage output up to alpha / beta / W_r_c
    the same bits on both routes, colours to rounding."""
    planes = fb.synth_planes(W, H, S, seed=21, sigma_f=sf, sigma_c=0.01, mode="smooth", flat_frac=flat)
    desc = hipmod.make_desc(W, H, S, policy=policy)
    got = ctx.filter_pass_debug(planes, desc, box=box, allow_nonfinite=True)
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=policy))
    small = int((want["nbhd_size"] <= 64).sum())
    assert small > 0.2 * W * H                      # the packed kernels really ran on a good share of the frame
    assert (got["status"] == hipmod.E_NONFINITE) == (want["status"] == 1)
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(want["colour"]))
    assert got["nonfinite_pixels"] == want["nonfinite_pixels"] and got["first_bad_pixel"] == want["first_bad_pixel"]
    if np.isfinite(want["colour"]).all():
        check_pass(got, want)
    with hipmod.Context(0) as c2:
        c2.set_option("packed", 0)
        old = c2.filter_pass_debug(planes, desc, box=box, allow_nonfinite=True)
    for k in ("nbhd_size", "member_hash", "bin_hash", "mean", "stddev", "mi", "alpha", "beta", "wrc"):
        assert np.array_equal(got[k], old[k], equal_nan=True), k
    assert got["status"] == old["status"] and got["nonfinite_pixels"] == old["nonfinite_pixels"]
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(old["colour"]))
    m = np.isfinite(old["colour"])
    np.testing.assert_allclose(got["colour"][m], old["colour"][m], rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("W,H,S,box,sf,flat,ndim,auto", [
    (45, 27, 8, 7, 3e-3, 0.3, 19, None),  # 1080p shape in small: every pixel class of the unbinned route
    (64, 40, 8, 7, 1e-5, 0.0, 19, 1),     # small neighbourhoods everywhere: the probe picks the count-first route
    (64, 40, 8, 7, 0.05, 0.0, 19, 0),     # large ones: the probe keeps stage 1b inside the fused kernel
    (29, 19, 3, 5, 0.02, 0.0, 19, None),  # S not a power of two, box 5, a NaN sample
    (9, 5, 8, 7, 0.05, 0.0, 19, None),    # windows clipped on every side
    (21, 12, 8, 5, 1e-2, 0.3, 27, None),  # 27-dim layout, fp16 planes
])
def test_count_first_route_equals_fused_route(hipmod, oracle, W, H, S, box, sf, flat, ndim, auto):
    """box*box*S <= 512 has two kernel routes: stage 1b inside filter_pixel_kernel (option "count_first" = 0) or as its own
    two-phase launch ahead of the filter kernels (1; nbhd_count_kernel: candidates that fail the first features never have the
    others gathered).  N, member order and everything downstream must be the same bits, whichever the probe picks."""
    kw = dict(n_random=4, n_feat=18, dtype="f16") if ndim == 27 else {}
    lay = dict(n_random=4, n_feat=18, plane_dtype=hipmod.PLANES_F16) if ndim == 27 else {}
    planes = fb.synth_planes(W, H, S, seed=33, sigma_f=sf, sigma_c=0.01, mode="smooth", flat_frac=flat, **kw)
    if flat == 0.0 and auto is None:  # (a NaN mean anywhere switches the stage-1a flat proof off for the frame)
        planes[10, 3, 5, 1 % S] = np.nan  # a NaN feature sample: passes the feature it is NaN in (ops.h:101-104), rejects nobody else
    desc = hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_EPS, **lay)
    res = {}
    for cf in (0, 1, -1):
        with hipmod.Context(0) as c:
            c.set_option("count_first", cf)
            res[cf] = c.filter_pass_debug(planes, desc, box=box, allow_nonfinite=True)
            route = c.route()
        assert route == cf if cf >= 0 else route in (0, 1)
        if cf < 0 and auto is not None:
            assert route == auto
    if ndim == 19:
        want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=oracle.DEGEN_EPS))
        assert np.array_equal(res[0]["nbhd_size"], want["nbhd_size"]) and np.array_equal(res[0]["member_hash"], want["member_hash"])
    for cf in (1, -1):
        for k in ("nbhd_size", "member_hash", "bin_hash", "mean", "stddev", "mi", "alpha", "beta", "wrc", "colour"):
            assert np.array_equal(res[cf][k], res[0][k], equal_nan=True), (cf, k)
        assert res[cf]["status"] == res[0]["status"] and res[cf]["nonfinite_pixels"] == res[0]["nonfinite_pixels"]
    # a row slab: the probe lattice and the count pass start at row_begin, windows reach into the halo rows
    r0, r1 = 2, H - 1
    dslab = hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_EPS, row_begin=r0, row_end=r1, **lay)
    with hipmod.Context(0) as c2:
        c2.set_option("count_first", 1)
        a = c2.filter_pass_debug(planes, dslab, box=box, allow_nonfinite=True)
    for k in ("nbhd_size", "member_hash"):
        assert np.array_equal(a[k][r0:r1], res[0][k][r0:r1]), k
    assert np.array_equal(a["colour"][:, r0:r1], res[0]["colour"][:, r0:r1], equal_nan=True)


@pytest.mark.parametrize("S", [8, 16])
def test_flat_quad_shortcut_and_nan_candidates(ctx, hipmod, oracle, S):
    """Stage 1b's flat-quad shortcut: a pixel with a zero-variance feature rejects every finite candidate (3 sigma = 0, strict
    test), proven from the stage-1a means of the window's pixels instead of testing its samples.  The one candidate that
    passes such a feature is a NaN one (NaN >= 0 is false): a window that holds a NaN sample must take the general test
    and accept it exactly as the reference does.  Membership (size, order) against the oracle on both the unbinned (8 spp)
    and the size-binned (16 spp) route."""
    W, H = 26, 15
    planes = fb.synth_planes(W, H, S, seed=5, sigma_f=0.05, sigma_c=0.01, mode="smooth", flat_frac=0.8)
    planes[7:10, 7, 11, 3] = np.nan     # one sample with a NaN normal (all three flat features) in the middle of the frame
    planes[9, 3, 20, 0] = np.nan        # and one with a single NaN component (still rejected by the other two flat features)
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7, policy=oracle.DEGEN_EPS))
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_EPS), box=7, allow_nonfinite=True)
    n = want["nbhd_size"]
    assert (n == S).mean() > 0.5 and (n > S).sum() > 10
    assert (n[4:11, 8:15] == S + 1).sum() > 5   # the NaN sample was accepted into flat pixels' neighbourhoods
    assert np.array_equal(got["nbhd_size"], n) and np.array_equal(got["member_hash"], want["member_hash"])
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(want["colour"]))
    m = np.isfinite(want["colour"])
    assert rel_l2(got["colour"][m], want["colour"][m]) <= REL_L2_BAR


@pytest.mark.parametrize("beta_map", [0, 1, 2])
def test_beta_numerator_presets(ctx, hipmod, oracle, beta_map):
    W, H, S = 16, 12, 8
    planes = fb.synth_planes(W, H, S, seed=2, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, beta_map=beta_map), box=7)
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7, beta_map=beta_map))
    check_pass(got, want)


def test_row_slab_with_halo_equals_full_frame(ctx, hipmod, oracle):
    """a rank that owns rows [a,b) and holds 3 halo rows either side produces exactly the full-frame rows"""
    W, H, S, b = 20, 24, 8, 3
    planes = fb.synth_planes(W, H, S, seed=9, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    full = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S), box=7)
    a0, a1 = 8, 16
    sub = np.ascontiguousarray(planes[:, a0 - b:a1 + b])
    part = ctx.filter_pass_debug(sub, hipmod.make_desc(W, a1 - a0 + 2 * b, S, row_begin=b, row_end=b + a1 - a0), box=7)
    assert np.array_equal(part["colour"][:, b:b + a1 - a0], full["colour"][:, a0:a1])
    assert np.array_equal(part["nbhd_size"][b:b + a1 - a0], full["nbhd_size"][a0:a1])
    # halo rows pass through unfiltered
    assert np.array_equal(part["colour"][:, :b], sub[2:5, :b].astype(np.float64))


def test_multi_pass_and_pixel_reduction(ctx, hipmod, oracle):
    """rpf_filter(): box list {7,5} then per-pixel mean of colour*rayWeight (rpf.cpp:767-794)"""
    W, H, S = 18, 12, 8
    planes = fb.synth_planes(W, H, S, seed=4, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    rw = (0.5 + np.random.default_rng(0).random((H, W, S))).astype(np.float32)
    srgb, prgb, st = ctx.filter(planes, hipmod.make_desc(W, H, S, boxes=(7, 5)), ray_weight=rw)
    assert st == hipmod.OK
    c = None
    for box in (7, 5):
        r = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box), colour_in=c, debug=False)
        c = r["colour"]
    assert rel_l2(srgb.astype(np.float64), c) <= REL_L2_BAR
    want_pix = oracle.pixel_mean(c, oracle.make_desc(W, H, S), rw)
    assert rel_l2(prgb.astype(np.float64), want_pix) <= REL_L2_BAR
    cnt = ctx.counters()
    # per pass: the fused kernel + the four packed launches over the re-routed small pixels (list sizes stay on the device)
    # + (REF_ABORT) the reference-expression kernel over the redo list, which is empty here
    assert cnt.samples_filtered == W * H * S * 2 and cnt.filter_kernel_launches == 2 * (1 + 4 + 1) and cnt.redo_pixels == 0


def test_multi_pass_with_size_binning(ctx, hipmod, oracle):
    """16 spp (box*box*S > 512: pixels are binned by neighbourhood size); a pass with the same box re-uses the previous
    pass's membership masks and pixel lists (membership depends on the features only)"""
    W, H, S = 15, 11, 16
    planes = fb.synth_planes(W, H, S, seed=12, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    srgb, prgb, st = ctx.filter(planes, hipmod.make_desc(W, H, S, boxes=(7, 7, 5), policy=hipmod.DEGEN_EPS))
    assert st == hipmod.OK
    c = None
    for box in (7, 7, 5):
        c = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=oracle.DEGEN_EPS), colour_in=c, debug=False)["colour"]
    assert rel_l2(srgb.astype(np.float64), c) <= REL_L2_BAR
    assert rel_l2(srgb.astype(np.float64), planes[2:5].astype(np.float64)) > 1e-3


@pytest.mark.parametrize("boxes,rows", [((7,), None), ((7, 5), None), ((5, 7, 5), None), ((5,), (6, 140)), ((7,), (20, 41)),
                                        ((9, 7, 9), None)])  # size-binned, unbinned, size-binned again (8 spp: 648 > 512 >= 392)
def test_host_entry_band_pipeline_equals_serial(ctx, hipmod, oracle, boxes, rows):
    """rpf_filter() on page-locked buffers (rpf_host_alloc) overlaps upload / filter / download over row bands; it
    must give bit-for-bit what the serial sequence (RPF_FLAG_NO_OVERLAP, and any pageable buffer) gives"""
    W, H, S = 40, 150, 8  # 150 rows -> eight bands of 19 rows
    planes = fb.synth_planes(W, H, S, seed=21, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    rw = (0.5 + np.random.default_rng(1).random((H, W, S))).astype(np.float32)
    r0, r1 = rows if rows else (0, H)
    kw = dict(boxes=boxes, row_begin=r0, row_end=r1, policy=hipmod.DEGEN_EPS)
    s_ser, p_ser, st = ctx.filter(planes, hipmod.make_desc(W, H, S, flags=hipmod.FLAG_NO_OVERLAP, **kw), ray_weight=rw)
    assert st == hipmod.OK
    n_serial = ctx.counters().sum_nbhd
    s_pipe, p_pipe, st = ctx.filter(planes, hipmod.make_desc(W, H, S, **kw), ray_weight=rw)
    assert st == hipmod.OK
    cnt = ctx.counters()
    assert cnt.sum_nbhd == n_serial and cnt.samples_filtered == (r1 - r0) * W * S * len(boxes)
    assert np.array_equal(s_pipe, s_ser) and np.array_equal(p_pipe, p_ser)
    # page-locked producer-side buffers
    pin = ctx.host_empty(planes.shape)
    pin[...] = planes
    pin_rw = ctx.host_empty(rw.shape)
    pin_rw[...] = rw
    out_s, out_p = ctx.host_empty(s_ser.shape), ctx.host_empty(p_ser.shape)
    ctx.filter(pin, hipmod.make_desc(W, H, S, **kw), ray_weight=pin_rw, out_samples=out_s, out_pixels=out_p)
    assert ctx.counters().filter_kernel_launches > len(boxes)  # the banded route ran (pageable buffers go serial)
    assert np.array_equal(out_s, s_ser) and np.array_equal(out_p, p_ser)
    s_pipe = out_s
    # rows outside the slab come back unfiltered
    if rows:
        assert np.array_equal(s_pipe[:, :r0], planes[2:5, :r0]) and np.array_equal(s_pipe[:, r1:], planes[2:5, r1:])
    # and the single-pass case against the oracle
    if boxes == (7,) and rows is None:
        want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7), debug=False)["colour"]
        assert rel_l2(s_pipe.astype(np.float64), want) <= REL_L2_BAR


def test_fast_weights_mode_meets_the_bar(ctx, hipmod, oracle):
    """RPF_FLAG_FAST_WEIGHTS: fp32 pair weights; every discrete outcome unchanged, colours within 1e-4 rel-L2"""
    for (W, H, S, mode, sf, sc) in [(24, 16, 8, "clustered", 1e-3, 0.01), (16, 12, 16, "clustered", 1e-3, 0.01),
                                    (24, 16, 8, "smooth", 0.05, 1e-4)]:
        planes = fb.synth_planes(W, H, S, seed=11, sigma_f=sf, sigma_c=sc, mode=mode)
        planes[10:13] += 800.0  # large world coordinates: differences must not be formed in fp32
        got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, flags=hipmod.FLAG_FAST_WEIGHTS), box=7)
        want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7))
        assert (got["nbhd_size"] == want["nbhd_size"]).all() and (got["bin_hash"] == want["bin_hash"]).all()
        np.testing.assert_allclose(got["beta"], want["beta"], rtol=1e-9, atol=1e-12)
        r = rel_l2(got["colour"], want["colour"])
        assert r <= 1e-5, r  # an order of magnitude inside the 1e-4 bar


def test_feature_images_bit_exact(ctx, hipmod, oracle):
    """visualizeSF (rpf.cpp:37-101): the six max-normalised per-pixel-mean feature images, bit for bit"""
    W, H, S = 33, 17, 8
    planes = fb.synth_planes(W, H, S, seed=8)
    planes[13:19, :, :, ::2] = 0.0   # missed second hits: zeros among the samples
    planes[7] = -np.abs(planes[7])   # an all-negative channel: its maximum stays 0 -> the channel normalises to 0
    got = ctx.feature_images(planes, hipmod.make_desc(W, H, S))
    want = oracle.feature_images(planes, oracle.make_desc(W, H, S))
    assert np.array_equal(got, want)
    assert (got[0, ..., 0] == 0).all() and got[2].max() == 1.0


@pytest.mark.parametrize("W,H,S,box", [(10, 8, 64, 7), (14, 10, 8, 9), (12, 9, 2, 7), (21, 6, 8, 7), (13, 9, 32, 7),
                                       (9, 8, 20, 9), (20, 18, 8, 17), (16, 12, 4, 11), (12, 9, 1, 7), (11, 7, 3, 5)])
def test_more_shapes_vs_oracle(ctx, hipmod, oracle, W, H, S, box):
    """the 49-samples-per-lane kernel (64 spp), a 9x9 box, 2 spp (B tiny: replicated-histogram path), a frame
    whose width is not a multiple of anything"""
    planes = fb.synth_planes(W, H, S, seed=23, sigma_f=0.02, sigma_c=0.01, mode="clustered")
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_EPS), box=box)
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=oracle.DEGEN_EPS))
    check_pass(got, want)


@pytest.mark.parametrize("S,nw", [(16, "4"), (32, "1"), (64, "1")])
def test_waves_per_pixel_variants_agree(ctx, hipmod, oracle, S, nw):
    """large neighbourhoods run four waves per pixel by default (32 spp and up), one otherwise; the per-context option
    "waves_per_pixel" forces the other variant: both must reproduce the oracle's discrete outcomes exactly"""
    W, H = 11, 9
    planes = fb.synth_planes(W, H, S, seed=31 + S, sigma_f=0.05, sigma_c=1e-4, mode="smooth")
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7))
    ctx.set_option("waves_per_pixel", int(nw))
    try:
        got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S), box=7)
        assert ctx.counters().options_active == 1
    finally:
        ctx.set_option("waves_per_pixel", 0)
    check_pass(got, want)
    with pytest.raises(hipmod.RpfError):
        ctx.set_option("no_such_option", 1)


@pytest.mark.parametrize("S,mode,layout", [(32, "smooth", 19), (64, "clustered", 19), (32, "smooth", 27), (8, "smooth", 19),
                                           (8, "clustered", 19), (16, "smooth", 19), (16, "clustered", 27)])
def test_far_pair_screen_changes_nothing(ctx, hipmod, S, mode, layout):
    """the four-wave kernels skip the fp64 exponent / exp() of a pair of own samples where an fp32 bound proves that
    every lane's weight underflows to 0.0, the one-wave kernels skip the exp() pass of a sweep step whose fp64 exponents
    all exceed 746: with the screen off the filtered colours must be the same BITS"""
    W, H = 12, 9
    kw = dict(n_random=4, n_feat=18, dtype="f16") if layout == 27 else {}
    planes = fb.synth_planes(W, H, S, seed=57 + S, sigma_f=0.05, sigma_c=1e-3, mode=mode, **kw)
    dkw = dict(n_random=4, n_feat=18, plane_dtype=hipmod.PLANES_F16) if layout == 27 else {}
    desc = hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_EPS, **dkw)
    on = ctx.filter_pass_debug(planes, desc, box=7)
    ctx.set_option("screen", 0)
    try:
        off = ctx.filter_pass_debug(planes, desc, box=7)
        assert ctx.counters().options_active == 1
    finally:
        ctx.set_option("screen", 1)
    assert on["max_nbhd"] > (832 if S >= 32 else 64)  # the four-wave kernels / the one-wave kernels ran
    assert np.array_equal(on["colour"], off["colour"], equal_nan=True)
    assert on["nonfinite_pixels"] == off["nonfinite_pixels"]


def test_far_pair_screen_keeps_nonfinite_colours(ctx, hipmod, oracle):
    """A neighbour whose colour is inf poisons every sum it enters, even with weight 0.0 (0 x inf = NaN, rpf.cpp:692; the
    reference then exits at rpf.cpp:702).  The far-pair screen must not skip such a sample: the same NaN pixels with the
    screen on and off, and the oracle's count."""
    W, H, S = 12, 9, 32
    planes = fb.synth_planes(W, H, S, seed=89, sigma_f=0.05, sigma_c=1e-3, mode="smooth")
    cin = planes[2:5].astype(np.float64)
    cin[1, 4, 6, 5] = np.inf
    desc = hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_EPS)
    on = ctx.filter_pass_debug(planes, desc, box=7, colour_in=cin, debug=False)
    ctx.set_option("screen", 0)
    try:
        off = ctx.filter_pass_debug(planes, desc, box=7, colour_in=cin, debug=False)
    finally:
        ctx.set_option("screen", 1)
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7, policy=oracle.DEGEN_EPS), colour_in=cin, debug=False)
    assert on["max_nbhd"] > 832 and want["nonfinite_pixels"] > 10
    assert on["nonfinite_pixels"] == off["nonfinite_pixels"] == want["nonfinite_pixels"]
    assert np.array_equal(on["colour"], off["colour"], equal_nan=True)
    m = np.isfinite(want["colour"])
    assert np.array_equal(np.isfinite(on["colour"]), m) and rel_l2(on["colour"][m], want["colour"][m]) <= REL_L2_BAR


@pytest.mark.parametrize("S,layout", [(64, 19), (64, 27), (32, 19), (32, 27)])
def test_split_weight_kernel_changes_nothing(ctx, hipmod, S, layout):
    """the 32- and 64-spp size classes run as three kernels (chains; bins + MI; the weights, at two to three times the
    occupancy; per-pixel statistics travel through global memory as doubles): with the split off every stage output and
    the filtered colours must be the same BITS"""
    W, H = 11, 8
    kw = dict(n_random=4, n_feat=18, dtype="f16") if layout == 27 else {}
    planes = fb.synth_planes(W, H, S, seed=91, sigma_f=0.05, sigma_c=1e-3, mode="smooth", **kw)
    dkw = dict(n_random=4, n_feat=18, plane_dtype=hipmod.PLANES_F16) if layout == 27 else {}
    desc = hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_EPS, **dkw)
    on = ctx.filter_pass_debug(planes, desc, box=7)
    assert ctx.counters().options_active == 0
    ctx.set_option("split_weights", 0)
    try:
        off = ctx.filter_pass_debug(planes, desc, box=7)
        assert ctx.counters().options_active == 1
    finally:
        ctx.set_option("split_weights", -1)
    assert on["max_nbhd"] > (1600 if S == 64 else 832)  # the K = 49 / K = 25 class ran
    ctx.set_option("split_chunk", 17)                    # the three launches over 17 list entries at a time (ragged last chunk)
    try:
        chunked = ctx.filter_pass_debug(planes, desc, box=7)
    finally:
        ctx.set_option("split_chunk", 0)
    assert np.array_equal(on["colour"], chunked["colour"], equal_nan=True) and np.array_equal(on["mi"], chunked["mi"], equal_nan=True)
    assert np.array_equal(on["colour"], off["colour"], equal_nan=True)
    for k in ("alpha", "beta", "wrc", "mi", "mean", "stddev"):
        assert np.array_equal(on[k], off[k], equal_nan=True), k
    assert on["nonfinite_pixels"] == off["nonfinite_pixels"]


def test_small_neighbourhood_paths_vs_oracle(ctx, hipmod, oracle):
    """N <= 64 (mi_stage_tiny) and 64 < N <= 128 (mi_stage_deep): tiny in-pixel jitter makes the 3-sigma test
    reject most neighbours, the regime of real path-traced buffers"""
    W, H, S = 30, 14, 8
    seen_tiny = seen_deep = False
    for sf in (1e-5, 2e-3, 8e-3):
        planes = fb.synth_planes(W, H, S, seed=31, sigma_f=sf, sigma_c=0.01, mode="smooth")
        got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_EPS), box=7)
        want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7, policy=oracle.DEGEN_EPS))
        check_pass(got, want)
        nb = want["nbhd_size"]
        seen_tiny |= bool((nb <= 64).any())
        seen_deep |= bool(((nb > 64) & (nb <= 128)).any())
    assert seen_tiny and seen_deep


@pytest.mark.parametrize("S,nmin", [(8, 256), (16, 449)])
def test_degenerate_cells_take_the_full_table_path(ctx, hipmod, oracle, S, nmin):
    """the one-wave kernels (K <= 8, and K = 13: 16 spp) keep the first 128 entries of the k ln k difference table in LDS; a
    pixel in which some histogram cell collects >= 128 samples (here: a two-valued colour channel against a two-valued
    feature, most of every pixel's samples in the same cell of their joint histogram, N ~ 300 / ~ 700) repeats its MI stage
    with the full table -- same results as the oracle"""
    W, H = 14, 10
    planes = fb.synth_planes(W, H, S, seed=41, sigma_f=0.05, sigma_c=1e-4, mode="smooth")
    planes[2] = np.float32(0.5)
    planes[2, :, :, 1] = np.float32(0.9)      # red: 0.9 for sample 1 of every pixel, 0.5 otherwise
    planes[7] = np.float32(0.0)
    planes[7, :, :, 0] = np.float32(1.0)      # n0.x: 1 for sample 0, 0 otherwise (std 0.33 / 0.24: every neighbour passes 3 sigma)
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_EPS), box=7)
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7, policy=oracle.DEGEN_EPS))
    assert want["nbhd_size"].max() >= nmin
    check_pass(got, want)


# ---- BASELINE configs[4]: 27-dim sample vectors (4 random parameters, 18 features), fp16 feature storage -------------
L27 = dict(n_random=4, n_feat=18)


def planes27(W, H, S, **kw):
    """fp16-stored 27-dim buffer and its exact fp32 image (what the oracle reads)"""
    p16 = fb.synth_planes(W, H, S, dtype="f16", **L27, **kw)
    return p16, p16.astype(np.float32)


@pytest.mark.parametrize("W,H,S,box,mode,sf,sc,policy", [
    (14, 10, 8, 7, "clustered", 1e-3, 0.01, 1),
    (14, 10, 8, 7, "smooth", 0.05, 1e-4, 0),     # REF_ABORT on a buffer the reference algebra completes
    (12, 8, 16, 7, "smooth", 0.05, 1e-4, 1),     # K = 13
    (10, 8, 4, 5, "clustered", 1e-3, 0.01, 1),
    (9, 7, 32, 7, "smooth", 0.05, 1e-4, 1),      # four waves per pixel
    (8, 6, 64, 7, "smooth", 0.05, 1e-4, 1),      # the 64 spp kernel of configs[4]
    (7, 5, 1, 7, "smooth", 0.05, 1e-4, 1),
    (30, 12, 8, 7, "smooth", 2e-3, 0.01, 1),     # small neighbourhoods
])
def test_layout27_fp16_filter_pass_vs_oracle(ctx, hipmod, oracle, W, H, S, box, mode, sf, sc, policy):
    """every stage output of the 27-dim / fp16-storage kernels against the oracle run on the same values: 180 MI pairs
    (18 x 6 feature pairs + 3 x 24 colour pairs, rpf.cpp:416-442 with the loop bounds generalised), 23 weighted columns"""
    p16, p32 = planes27(W, H, S, seed=19, sigma_f=sf, sigma_c=sc, mode=mode)
    got = ctx.filter_pass_debug(p16, hipmod.make_desc(W, H, S, policy=policy, plane_dtype=hipmod.PLANES_F16, **L27), box=box,
                                allow_nonfinite=True)
    want = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=box, policy=policy, **L27))
    assert got["mi"].shape[-1] == 180 and got["beta"].shape[-1] == 18 and got["mean"].shape[-1] == 27
    assert got["nonfinite_pixels"] == want["nonfinite_pixels"]
    if np.isfinite(want["colour"]).all():
        check_pass(got, want)
    else:
        for k in ("nbhd_size", "member_hash", "bin_hash"):
            assert (got[k] == want[k]).all()
        assert (np.isfinite(got["colour"]) == np.isfinite(want["colour"])).all()


@pytest.mark.parametrize("beta_map", [0, 1, 2])
def test_layout27_beta_presets_and_activity(ctx, hipmod, oracle, beta_map):
    W, H, S = 16, 12, 8
    p16, p32 = planes27(W, H, S, seed=2, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    got = ctx.filter_pass_debug(p16, hipmod.make_desc(W, H, S, beta_map=beta_map, policy=1, plane_dtype=hipmod.PLANES_F16, **L27), box=7)
    want = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=7, beta_map=beta_map, policy=1, **L27))
    check_pass(got, want)
    assert rel_l2(want["colour"], p32[2:5].astype(np.float64)) > 1e-3   # not the identity


def test_layout27_multi_pass_host_entry_and_stage1a(ctx, hipmod, oracle):
    W, H, S = 15, 11, 8
    p16, p32 = planes27(W, H, S, seed=5, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    d = hipmod.make_desc(W, H, S, boxes=(7, 5), policy=1, plane_dtype=hipmod.PLANES_F16, **L27)
    m, sd = ctx.pixel_stats(p16, d)
    mo, so = oracle.pixel_stats(p32, oracle.make_desc(W, H, S, **L27))
    assert m.shape[-1] == 18 and np.array_equal(m, mo) and np.array_equal(sd, so, equal_nan=True)
    srgb, prgb, st, c64 = ctx.filter(p16, d, want_colour64=True)
    assert st == hipmod.OK
    c = None
    for box in (7, 5):
        c = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=box, policy=1, **L27), colour_in=c, debug=False)["colour"]
    assert rel_l2(c64, c) <= 1e-9
    # the host pipeline's path (page-locked buffers) moves fp16 planes too; 11 rows are ONE band there (a frame below 32 rows is
    # never cut): the cut into several bands, fp16 planes included, is held by tests/test_host_bands_gpu.py
    pin = ctx.host_empty(p16.shape, np.float16)
    pin[...] = p16
    out_s, out_p = ctx.host_empty(srgb.shape), ctx.host_empty(prgb.shape)
    ctx.filter(pin, d, out_samples=out_s, out_pixels=out_p)
    assert np.array_equal(out_s, srgb) and np.array_equal(out_p, prgb)


def test_layout_rejections(ctx, hipmod):
    planes = np.zeros((27, 4, 4, 2), np.float32)
    with pytest.raises(hipmod.RpfError) as e:   # 27 dims exist with fp16 planes only
        ctx.filter(planes, hipmod.make_desc(4, 4, 2, **L27))
    assert e.value.status == hipmod.E_UNSUPPORTED
    with pytest.raises(hipmod.RpfError) as e:
        ctx.filter(np.zeros((25, 4, 4, 2), np.float16), hipmod.make_desc(4, 4, 2, n_random=2, n_feat=18, plane_dtype=hipmod.PLANES_F16))
    assert e.value.status == hipmod.E_UNSUPPORTED


def test_config5_shape_slab_8192x70x64_fp16(ctx, hipmod, oracle):
    """BASELINE configs[4]: 8192 x 8192 x 64 spp, 27 dims, fp16 storage (232 GB of features: a slab at a time, generated
    on the device in row chunks).  One slab of 64 owned rows + 3 halo rows either side: determinism, neighbourhood
    bounds, hull bounds, and the oracle on a 512-pixel-wide cut of one owned row."""
    import torch
    W, S, b, own = 8192, 64, 3, 64
    H = own + 2 * b
    dev = torch.device("cuda", 0)
    planes = fb.synth_planes_chunked(W, H, S, rows_per_chunk=8, row0=4000, xp=fb.torch_backend(dev), mode="smooth",
                                     sigma_f=0.05, sigma_c=1e-4, dtype="f16", **L27).contiguous()
    assert planes.dtype == torch.float16 and planes.shape == (27, H, W, S)
    desc = hipmod.make_desc(W, H, S, row_begin=b, row_end=b + own, policy=hipmod.DEGEN_EPS, plane_dtype=hipmod.PLANES_F16, **L27)
    stream = torch.cuda.current_stream().cuda_stream
    col0 = torch.empty((3, H, W, S), dtype=torch.float64, device=dev)
    ctx.colour_from_planes_device(desc, planes.data_ptr(), col0.data_ptr(), stream)
    torch.cuda.synchronize()
    assert torch.equal(col0, planes[2:5].to(torch.float64))
    outs = []
    for _ in range(2):
        c = col0.clone()
        ctx.filter_device(desc, planes.data_ptr(), c.data_ptr(), stream)
        outs.append(c)
    torch.cuda.synchronize()
    out = outs[0]
    assert torch.equal(out, outs[1])
    cnt = ctx.counters()
    assert cnt.samples_filtered == own * W * S and cnt.nonfinite_pixels == 0 and S <= cnt.max_nbhd <= 49 * S
    pad = torch.nn.functional.pad
    cmin, cmax = col0.amin(dim=3), col0.amax(dim=3)
    wmin = -torch.nn.functional.max_pool2d(pad(-cmin, (b, b, b, b), value=-1e30), 2 * b + 1, stride=1)
    wmax = torch.nn.functional.max_pool2d(pad(cmax, (b, b, b, b), value=-1e30), 2 * b + 1, stride=1)
    assert bool((out >= wmin[..., None] - 1e-9).all()) and bool((out <= wmax[..., None] + 1e-9).all())
    r0, x0, xw = 30, 3000, 512
    host = planes[:, r0 - b:r0 + 1 + b, x0 - b:x0 + xw + b].float().cpu().numpy()
    want = oracle.filter_pass(host, oracle.make_desc(xw + 2 * b, 2 * b + 1, S, box=7, row_begin=b, row_end=b + 1,
                                                     policy=oracle.DEGEN_EPS, **L27), debug=False)["colour"][:, b:b + 1, b:b + xw]
    assert rel_l2(out[:, r0:r0 + 1, x0:x0 + xw].cpu().numpy(), want) <= REL_L2_BAR


@pytest.mark.parametrize("devices,boxes,S", [((0, 0), (7, 5), 8), ((0, 0, 0), (7, 7, 5), 8), ((0, 0), (7,), 16), ((0,), (7, 5), 8),
                                             ((0, 1), (7, 5), 8), ((0, 1, 0), (7, 7, 5), 8)])
def test_multi_context_row_slabs_equal_one_context(ctx, hipmod, oracle, devices, boxes, S):
    """rpf_multi_filter: one caller, one row slab per device entry, colour halo refreshed between passes by device-to-
    device (peer) copies of the neighbours' owned rows.  Rehearsed on the one GPU of this box with several slab contexts
    on device 0: filtered samples, pixel means and merged counters must equal the single-context full-frame call bit for
    bit (the reference filters the whole film every pass, rpf.cpp:732)."""
    import torch
    if max(devices) >= torch.cuda.device_count():
        # the hipMemcpyPeerAsync branch of the halo refresh (two different ordinals) needs a second GPU: unexecuted on the
        # one-GPU boxes this repository is developed on -- the (0, 0) cases above cover the same offsets with plain copies
        pytest.skip("needs %d visible GPUs" % (max(devices) + 1))
    W, H = 21, 37
    planes = fb.synth_planes(W, H, S, seed=3, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    rw = (0.5 + np.random.default_rng(4).random((H, W, S))).astype(np.float32)
    desc = hipmod.make_desc(W, H, S, boxes=boxes, policy=hipmod.DEGEN_EPS)
    s1, p1, st = ctx.filter(planes, desc, ray_weight=rw)
    c1 = ctx.counters()
    with hipmod.MultiContext(list(devices)) as mc:
        assert mc.device_count == len(devices)
        s2, p2, st2 = mc.filter(planes, desc, ray_weight=rw)
        c2 = mc.counters()
    assert st == st2 == hipmod.OK
    assert np.array_equal(s1, s2) and np.array_equal(p1, p2)
    assert (c2.samples_filtered, c2.sum_nbhd, c2.max_nbhd, c2.nonfinite_pixels) == (
        c1.samples_filtered, c1.sum_nbhd, c1.max_nbhd, c1.nonfinite_pixels)
    # and the oracle's multi-pass chain on the whole film
    c = None
    for box in boxes:
        c = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=1), colour_in=c, debug=False)["colour"]
    assert rel_l2(s2.astype(np.float64), c) <= REL_L2_BAR


def test_multi_context_errors_and_nonfinite_pixel(hipmod, oracle):
    W, H, S = 12, 16, 8
    planes = fb.synth_planes(W, H, S, seed=5)
    planes[7:10] = np.float32([0.0, 0.0, 1.0])[:, None, None, None]   # constant normal: 0/0 under REF_ABORT
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7))
    with hipmod.MultiContext([0, 0]) as mc:
        srgb, prgb, st = mc.filter(planes, hipmod.make_desc(W, H, S), allow_nonfinite=True)
        assert st == hipmod.E_NONFINITE
        c = mc.counters()
        assert c.nonfinite_pixels == want["nonfinite_pixels"] and c.first_bad_pixel == want["first_bad_pixel"]
        with pytest.raises(hipmod.RpfError) as e:      # a slab thinner than its neighbours' halo
            mc.filter(planes[:, :4], hipmod.make_desc(W, 4, S, boxes=(7,)))
        assert e.value.status == hipmod.E_BADARG
        with pytest.raises(hipmod.RpfError) as e:      # the slabs are rpf_multi's own
            mc.filter(planes, hipmod.make_desc(W, H, S, row_begin=2, row_end=10))
        assert e.value.status == hipmod.E_BADARG
    with pytest.raises(hipmod.RpfError) as e:
        hipmod.MultiContext([0, 99])
    assert e.value.status == hipmod.E_BADARG


@pytest.mark.parametrize("W,H,S,box,mode,sf,sc", [
    (22, 19, 16, 17, "smooth", 0.05, 1e-4),     # box 17 x 16 spp: N up to 4624 (> 3136: the streaming kernel)
    (38, 36, 8, 35, "smooth", 0.05, 1e-4),      # box 35 x 8 spp: N up to 9800
    (26, 21, 8, 17, "clustered", 1e-3, 0.01),   # box 17, small / mid neighbourhoods: resident classes under a large window
    (13, 11, 8, 55, "smooth", 0.05, 1e-4),      # box 55 on a frame smaller than the box: every window is the whole frame
])
def test_large_boxes_vs_oracle(ctx, hipmod, oracle, W, H, S, box, mode, sf, sc):
    """the reference's commented box list {55, 35, 17, 7} (rpf.cpp:767): neighbourhoods beyond 3136 samples stream
    their member list and bin ids through global scratch (generic::filter_pixel_kernel); pixels of the same pass whose N is
    small still run the LDS-resident kernels.  Every stage output against the oracle."""
    planes = fb.synth_planes(W, H, S, seed=29, sigma_f=sf, sigma_c=sc, mode=mode)
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_EPS), box=box)
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=oracle.DEGEN_EPS))
    check_pass(got, want)
    if box in (17, 35) and mode == "smooth":
        assert want["nbhd_size"].max() > 3136      # the streaming kernel ran


def test_large_box_list_17_7_at_16spp(ctx, hipmod, oracle):
    """the multi-pass entry with a box list that mixes the streaming kernel ({17} at 16 spp) and the resident ones"""
    W, H, S = 21, 20, 16
    planes = fb.synth_planes(W, H, S, seed=30, sigma_f=0.05, sigma_c=1e-4, mode="smooth")
    srgb, prgb, st, c64 = ctx.filter(planes, hipmod.make_desc(W, H, S, boxes=(17, 7), policy=hipmod.DEGEN_EPS), want_colour64=True)
    assert st == hipmod.OK
    c = None
    for box in (17, 7):
        c = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=1), colour_in=c, debug=False)["colour"]
    assert rel_l2(c64, c) <= 1e-9


def test_multi_pass_on_a_sub_slab_is_refused(ctx, hipmod):
    """the reference filters the whole film every pass (rpf.cpp:732); a strict sub-slab with n_box > 1 would read
    unfiltered halo colours in pass 2, so the ABI refuses it (one pass per call + halo exchange, or rpf_filter_multi)"""
    planes = np.zeros((19, 12, 4, 2), np.float32)
    with pytest.raises(hipmod.RpfError) as e:
        ctx.filter(planes, hipmod.make_desc(4, 12, 2, boxes=(7, 5), row_begin=3, row_end=9))
    assert e.value.status == hipmod.E_BADARG and "halo" in str(e.value)
    ctx.filter(planes + 1, hipmod.make_desc(4, 12, 2, boxes=(7,), row_begin=3, row_end=9, policy=hipmod.DEGEN_EPS))


def test_badarg_and_unsupported(ctx, hipmod):
    planes = np.zeros((19, 4, 4, 2), np.float32)
    with pytest.raises(hipmod.RpfError) as e:
        ctx.filter(planes, hipmod.make_desc(4, 4, 2, boxes=(4,)))
    assert e.value.status == hipmod.E_BADARG
    with pytest.raises(hipmod.RpfError) as e:   # box*box*S = 96800 > 65535: beyond the streaming kernel's 16-bit cells
        ctx.filter(np.zeros((19, 4, 4, 32), np.float32), hipmod.make_desc(4, 4, 32, boxes=(55,)))
    assert e.value.status == hipmod.E_UNSUPPORTED


# ---- committed fixtures, host mirror, full-size properties -------------------------------------------
import ctypes as C  # noqa: E402
import os  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", ["e2e_clustered_12x10x8_box7", "e2e_smooth_10x8x8_box7",
                                  "e2e_clustered_8x6x16_box5", "e2e_constnormal_8x6x8_box7_eps"])
def test_gpu_reproduces_committed_fixtures(ctx, hipmod, name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    planes = g["planes"]
    _, H, W, S = planes.shape
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=int(g["policy"])), box=int(g["box"]))
    want = {k: g[k] for k in ("nbhd_size", "member_hash", "bin_hash", "mean", "stddev", "mi", "alpha", "beta", "wrc", "colour")}
    check_pass(got, want)
    assert got["nonfinite_pixels"] == int(g["nonfinite_pixels"])


def test_host_mirror_apply_rpf_filter(hipmod, oracle):
    """the C++ mirror of RPFIntegrator::ApplyRPFFilter(SamplingFilm&, tileSize, box_size): AoS doubles in
    SamplingFilm order in, colour columns replaced, every other column untouched (rpf.cpp:715, 732)"""
    lib = C.CDLL(os.path.join(os.path.dirname(hipmod.LIB_PATH), "librpf_host.so"))
    W, H, S = 14, 9, 8
    planes = fb.synth_planes(W, H, S, seed=6, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    aos = fb.planes_to_aos(planes)
    before = aos.copy()
    boxes = (C.c_int32 * 1)(7)
    err = C.create_string_buffer(256)
    st = lib.rpf_host_apply_filter_aos(aos.ctypes.data_as(C.c_void_p), None, W, H, S, boxes, 1, 0, 0, 0, None, err, 256)
    assert st == 0, err.value
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7), debug=False)["colour"]
    got = np.transpose(aos[..., 2:5], (3, 1, 0, 2))  # [x][y][s][c] -> [c][y][x][s]
    assert rel_l2(got, want) <= REL_L2_BAR
    keep = [0, 1] + list(range(5, 19))
    assert np.array_equal(aos[..., keep], before[..., keep])
    assert rel_l2(got, planes[2:5].astype(np.float64)) > 1e-3  # and the filter did something


def test_host_plane_film_producer_equals_sampling_film(hipmod, oracle):
    """concurrent tile producers AddSample() straight into page-locked SoA planes (PlaneFilm); the
    filtered colours and pixel means equal what the AoS SamplingFilm route gives, bit for bit"""
    lib = C.CDLL(os.path.join(os.path.dirname(hipmod.LIB_PATH), "librpf_host.so"))
    W, H, S = 37, 45, 8
    planes = fb.synth_planes(W, H, S, seed=8, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    rw = (0.5 + np.random.default_rng(2).random((W, H, S))).astype(np.float32)  # SamplingFilm order [x][y][s]
    aos = fb.planes_to_aos(planes)
    boxes = (C.c_int32 * 2)(7, 5)
    err = C.create_string_buffer(256)
    srgb = np.empty((3, H, W, S), np.float32)
    prgb = np.empty((H, W, 3), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    st = lib.rpf_host_planefilm_filter(vp(aos), vp(rw), W, H, S, boxes, 2, 0, 1, 0, vp(srgb), vp(prgb), err, 256)
    assert st == 0, err.value
    aos2 = aos.copy()
    prgb2 = np.empty((H, W, 3), np.float32)
    st = lib.rpf_host_apply_filter_aos(vp(aos2), vp(rw), W, H, S, boxes, 2, 0, 1, 0, vp(prgb2), err, 256)
    assert st == 0, err.value
    got2 = np.transpose(aos2[..., 2:5], (3, 1, 0, 2)).astype(np.float32)
    assert np.array_equal(srgb, got2) and np.array_equal(prgb, prgb2)
    c = None
    for box in (7, 5):
        c = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=1), colour_in=c, debug=False)["colour"]
    assert rel_l2(srgb.astype(np.float64), c) <= REL_L2_BAR


def test_host_mirror_per_box_calls_carry_doubles(hipmod, oracle):
    """the reference's own call shape: one ApplyRPFFilter(film, 16, box) per box size on the same film (rpf.cpp:767-775).
    The film's colours are doubles (sd.h:205-208) and stay doubles across the boundary (rpf_filter_ex), so two calls
    {7}, {5} equal ONE call with the box list {7, 5} bit for bit, and the oracle's two-pass chain to rounding."""
    lib = C.CDLL(os.path.join(os.path.dirname(hipmod.LIB_PATH), "librpf_host.so"))
    W, H, S = 13, 9, 8
    planes = fb.synth_planes(W, H, S, seed=16, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    boxes = (C.c_int32 * 2)(7, 5)
    err = C.create_string_buffer(256)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    per_box, one_call = fb.planes_to_aos(planes), fb.planes_to_aos(planes)
    st = lib.rpf_host_apply_filter_aos(vp(per_box), None, W, H, S, boxes, 2, 0x100, 1, 0, None, err, 256)
    assert st == 0, err.value
    st = lib.rpf_host_apply_filter_aos(vp(one_call), None, W, H, S, boxes, 2, 0, 1, 0, None, err, 256)
    assert st == 0, err.value
    assert np.array_equal(per_box, one_call)
    c = None
    for box in (7, 5):
        c = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=1), colour_in=c, debug=False)["colour"]
    got = np.transpose(per_box[..., 2:5], (3, 1, 0, 2))
    assert rel_l2(got, c) <= 1e-9
    assert np.abs(got - got.astype(np.float32)).max() > 0     # genuinely doubles, not fp32-rounded colours


def test_rpfb_fixture_through_the_hip_path(ctx, hipmod):
    """a committed on-disk feature buffer (.rpfb: header + planes + ray weights) loaded and filtered with
    the box list {7, 5}; expected values are the oracle's (tests/golden/make_golden.py rpfb)"""
    planes, rw = fb.load_rpfb(os.path.join(GOLD, "clustered_10x8x8.rpfb"))
    g = np.load(os.path.join(GOLD, "clustered_10x8x8_expected.npz"))
    _, H, W, S = planes.shape
    assert (W, H, S) == (10, 8, 8) and rw is not None
    desc = hipmod.make_desc(W, H, S, boxes=tuple(int(b) for b in g["boxes"]), policy=int(g["policy"]))
    srgb, prgb, st, c64 = ctx.filter(planes, desc, ray_weight=rw, want_colour64=True)
    assert st == hipmod.OK
    assert rel_l2(c64, g["colour"]) <= 1e-9
    assert rel_l2(srgb.astype(np.float64), g["colour"]) <= REL_L2_BAR
    assert rel_l2(prgb.astype(np.float64), g["pixel_rgb"]) <= REL_L2_BAR
    assert rel_l2(c64, planes[2:5].astype(np.float64)) > 1e-3


@pytest.mark.parametrize("W,H,S,mode,sf,sc,R", [
    (1920, 1080, 8, "clustered", 1e-3, 0.01, 3),   # BASELINE configs[1]
    (3840, 64, 32, "clustered", 1e-3, 0.01, 1),    # same shape, small neighbourhoods: several size classes per pass
    (1920, 48, 64, "smooth", 0.05, 1e-4, 1),       # 64 spp: N ~ 3000
])
def test_full_size_properties(ctx, hipmod, oracle, W, H, S, mode, sf, sc, R):
    """BASELINE-size buffers through size-independent properties: determinism, neighbourhood size bounds,
    convex-combination bounds of every filtered colour, slab == full frame on a band, and the oracle on R full-width
    rows."""
    import torch
    b = 3
    dev = torch.device("cuda", 0)
    planes = fb.synth_planes(W, H, S, xp=fb.torch_backend(dev), mode=mode, sigma_f=sf, sigma_c=sc).contiguous()
    col0 = planes[2:5].to(torch.float64).contiguous()
    desc = hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_EPS)
    outs = []
    for _ in range(2):
        c = col0.clone()
        ctx.filter_device(desc, planes.data_ptr(), c.data_ptr(), torch.cuda.current_stream().cuda_stream)
        outs.append(c)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])                     # bitwise reproducible (integer histogram sums)
    cnt = ctx.counters()
    assert cnt.nonfinite_pixels == 0 and S <= cnt.max_nbhd <= 49 * S
    assert S * W * H <= cnt.sum_nbhd <= 49 * S * W * H
    # every filtered colour is a convex combination of colours inside its 7x7 window
    pad = torch.nn.functional.pad
    cmin = col0.amin(dim=3)
    cmax = col0.amax(dim=3)
    wmin = -torch.nn.functional.max_pool2d(pad(-cmin, (b, b, b, b), value=-1e30), 2 * b + 1, stride=1)
    wmax = torch.nn.functional.max_pool2d(pad(cmax, (b, b, b, b), value=-1e30), 2 * b + 1, stride=1)
    out = outs[0]
    tol = 1e-9
    assert bool((out >= wmin[..., None] - tol).all()) and bool((out <= wmax[..., None] + tol).all())
    # a slab with halo reproduces the same rows
    a0 = H // 2 - min(32, H // 4)
    a1 = a0 + 2 * min(32, H // 4)
    sub = planes[:, a0 - b:a1 + b].contiguous()
    csub = sub[2:5].to(torch.float64).contiguous()
    d2 = hipmod.make_desc(W, a1 - a0 + 2 * b, S, row_begin=b, row_end=b + a1 - a0, policy=hipmod.DEGEN_EPS)
    ctx.filter_device(d2, sub.data_ptr(), csub.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(csub[:, b:b + a1 - a0], out[:, a0:a1])
    # and the oracle agrees on R full-width rows of it
    host = sub[:, :2 * b + R].cpu().numpy()
    want = oracle.filter_pass(host, oracle.make_desc(W, 2 * b + R, S, box=7, row_begin=b, row_end=b + R,
                                                     policy=oracle.DEGEN_EPS), debug=False)["colour"][:, b:b + R]
    got = out[:, a0:a0 + R].cpu().numpy()
    assert rel_l2(got, want) <= REL_L2_BAR
    if mode == "clustered":
        assert rel_l2(got, host[2:5, b:b + R].astype(np.float64)) > 1e-3  # the filter did something


def test_randomised_parity_sweep(ctx, hipmod, oracle):
    """40 random configurations (scripts/fuzz_parity.py runs the same sweep at any length): shapes, 1..64 spp, boxes
    3..11, both generators, both policies, all beta presets; REF_ABORT cases must reproduce the oracle's NaN pattern"""
    rng = np.random.default_rng(424242)
    for _ in range(40):
        box = int(rng.choice([3, 5, 7, 7, 7, 9, 11]))
        smax = max(1, 3136 // (box * box))
        S = int(rng.choice([s for s in (1, 2, 3, 4, 5, 8, 8, 12, 16, 24, 32, 48, 64) if s <= smax]))
        W, H = int(rng.integers(3, 26)), int(rng.integers(2, 18))
        while W * H * S > 40000:
            W, H = max(3, W - 2), max(2, H - 1)
        mode = str(rng.choice(["smooth", "clustered"]))
        sf = float(rng.choice([1e-5, 1e-3, 0.02, 0.05]))
        policy = int(rng.choice([hipmod.DEGEN_EPS, hipmod.DEGEN_EPS, hipmod.DEGEN_REF_ABORT]))
        beta = int(rng.integers(0, 3))
        planes = fb.synth_planes(W, H, S, seed=int(rng.integers(0, 1 << 30)), sigma_f=sf, sigma_c=0.01, mode=mode)
        got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=policy, beta_map=beta), box=box,
                                    allow_nonfinite=True)
        want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=policy, beta_map=beta))
        tag = (W, H, S, box, mode, sf, policy, beta)
        assert got["nonfinite_pixels"] == want["nonfinite_pixels"], tag
        if np.isfinite(want["colour"]).all():
            check_pass(got, want)
        else:
            for k in ("nbhd_size", "member_hash", "bin_hash"):
                assert (got[k] == want[k]).all(), (k, tag)
            assert (np.isfinite(got["colour"]) == np.isfinite(want["colour"])).all(), tag


# ---- route options, non-finite features, the headline regime at full width ------------------------------------------
STAGE_KEYS = ("nbhd_size", "member_hash", "bin_hash", "mean", "stddev", "mi", "alpha", "beta", "wrc")
# options documented as giving the same colour BITS (include/rpf_hip.h rpf_set_option); the others change which kernel, and
# so which order of the weight sums, filters a pixel: their colours agree to rounding
SAME_BITS = ("screen", "split_weights", "split_chunk", "count_first")


def _run_opts(hipmod, planes, desc, box, opts=()):
    """one pass on a fresh context (no option outlives its run), every debug plane"""
    with hipmod.Context(0) as c:
        for name, value in opts:
            c.set_option(name, value)
        got = c.filter_pass_debug(planes, desc, box=box, allow_nonfinite=True)
        got["route"] = c.route()
        got["options_active"] = c.counters().options_active
    return got


def _assert_oracle_parity(got, want, hipmod):
    """check_pass where the oracle's colours are finite; otherwise (REF_ABORT) the oracle's NaN pattern and status"""
    assert (got["status"] == hipmod.E_NONFINITE) == (want["status"] == 1)
    assert got["nonfinite_pixels"] == want["nonfinite_pixels"] and got["first_bad_pixel"] == want["first_bad_pixel"]
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(want["colour"]))
    if np.isfinite(want["colour"]).all():
        check_pass(got, want)
    else:
        for k in ("nbhd_size", "member_hash", "bin_hash"):
            assert (got[k] == want[k]).all(), k
        fin = np.isfinite(want["colour"])
        assert rel_l2(got["colour"][fin], want["colour"][fin]) <= REL_L2_BAR


# name: (W, H, S, box, mode, sigma_f, sigma_c, flat_frac, policy, layout)
ROUTE_BUFFERS = {
    "8spp-b7-flat0": (40, 24, 8, 7, "smooth", 3e-3, 0.01, 0.0, 1, 19),      # unbinned; N = 8 ... 97: count first by the probe
    "8spp-b7-flat94": (40, 24, 8, 7, "smooth", 0.05, 0.01, 0.94, 0, 19),    # unbinned, 94 % flat pixels, REF_ABORT: the oracle's NaNs
    "16spp-b7": (30, 14, 16, 7, "smooth", 3e-3, 0.01, 0.0, 1, 19),          # binned; N = 23 ... 130: packed and one-wave classes
    "32spp-b7-smooth": (11, 9, 32, 7, "smooth", 0.05, 1e-4, 0.0, 1, 19),    # split route, K = 25
    "64spp-b7-smooth": (11, 8, 64, 7, "smooth", 0.05, 1e-4, 0.0, 1, 19),    # split route, K = 49
    "72spp-b5-flat60": (10, 8, 72, 5, "clustered", 1e-3, 0.01, 0.6, 1, 19),  # flat pixels whose N = S = 72 fits no packed class
    "27dim-8spp-b7": (16, 10, 8, 7, "smooth", 3e-3, 0.01, 0.3, 1, 27),      # fp16 planes
    "16spp-b17": (20, 18, 16, 17, "smooth", 0.05, 1e-4, 0.0, 1, 19),        # N up to 4142: the streaming kernel
}
ROUTE_OPTIONS = [("binning", 0), ("binning", 1), ("table_in_lds", 0), ("table_in_lds", 1), ("strip_w", 8), ("strip_w", 128),
                 ("waves_per_pixel", 1), ("waves_per_pixel", 4), ("count_first", 0), ("count_first", 1), ("packed", 0),
                 ("split_weights", 0), ("split_chunk", 17), ("screen", 0)]
# table_in_lds = 1 at 64 spp: the K = 49 kernel's 147 KiB plus the 25 KiB table exceed the 160 KiB of LDS a workgroup may
# have, and the launch is refused (rpf_lds_bytes_required(64, 7) = 150784 without the table)
ROUTE_SKIP = {("64spp-b7-smooth", "table_in_lds", 1)}


_ROUTE_CACHE = {}  # name -> (planes, desc, box, oracle result, default-options run): each buffer is filtered once per session


def _route_buffer(hipmod, oracle, name):
    _cache = _ROUTE_CACHE
    if name not in _cache:
        W, H, S, box, mode, sf, sc, flat, policy, layout = ROUTE_BUFFERS[name]
        kw = dict(L27, dtype="f16") if layout == 27 else {}
        planes = fb.synth_planes(W, H, S, seed=21, sigma_f=sf, sigma_c=sc, mode=mode, flat_frac=flat, **kw)
        lay = dict(L27, plane_dtype=hipmod.PLANES_F16) if layout == 27 else {}
        olay = L27 if layout == 27 else {}
        desc = hipmod.make_desc(W, H, S, policy=policy, **lay)
        want = oracle.filter_pass(planes.astype(np.float32), oracle.make_desc(W, H, S, box=box, policy=policy, **olay))
        _cache[name] = (planes, desc, box, want, _run_opts(hipmod, planes, desc, box))
    return _cache[name]


@pytest.mark.parametrize("name,option,value", [(b, o, v) for b in ROUTE_BUFFERS for o, v in ROUTE_OPTIONS
                                               if (b, o, v) not in ROUTE_SKIP])
def test_route_options_change_nothing(hipmod, oracle, name, option, value):
    """Every route option documented as changing nothing (rpf_set_option), on buffers that reach every kernel route: the run
    with the option against the oracle AND against the default run -- every stage output the same bits, colours the same bits
    where the option promises it, to rounding otherwise."""
    planes, desc, box, want, base = _route_buffer(hipmod, oracle, name)
    got = _run_opts(hipmod, planes, desc, box, [(option, value)])
    assert got["options_active"] == 1
    _assert_oracle_parity(got, want, hipmod)
    _assert_oracle_parity(base, want, hipmod)
    for k in STAGE_KEYS:
        assert np.array_equal(got[k], base[k], equal_nan=True), k
    assert got["status"] == base["status"] and got["nonfinite_pixels"] == base["nonfinite_pixels"]
    assert got["first_bad_pixel"] == base["first_bad_pixel"]
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(base["colour"]))
    if option in SAME_BITS:
        assert np.array_equal(got["colour"], base["colour"], equal_nan=True)
    else:
        # another kernel (or the same kernel with another LDS layout / pixel walk) sums the weights of a pixel: same terms,
        # possibly in another order
        m = np.isfinite(base["colour"])
        np.testing.assert_allclose(got["colour"][m], base["colour"][m], rtol=1e-12, atol=1e-300)
    if name == "72spp-b5-flat60":
        # not vacuous: the oracle moves the colours of the flat pixels (N = S), so a pixel left unfiltered fails above
        flat = want["nbhd_size"] == ROUTE_BUFFERS[name][2]
        cin = planes[2:5].astype(np.float64)
        assert flat.sum() > 10 and np.abs(want["colour"][:, flat] - cin[:, flat]).max() > 1e-3
    if option == "binning" and name in ("8spp-b7-flat0", "8spp-b7-flat94", "27dim-8spp-b7"):
        assert got["route"] == (2 if value else base["route"])


INF_INJECTIONS = ("pixel_inf", "sample_inf", "mixed_inf", "random_inf", "colour_inf")


def _nonflat_pixel(planes, f0, y, x):
    """the first pixel at or right of (y, x) none of whose features is constant over its samples"""
    while (planes[f0:, y, x].astype(np.float64).std(axis=-1) == 0).any():
        x += 1
    return y, x


def _inject_inf(planes, layout, kind):
    """non-finite values where path tracers put them (a miss ray's depth / position): returns the injected pixels"""
    f0 = 5 + (4 if layout == 27 else 2)
    k = f0 + 9                                  # second-hit position x (p1x)
    if kind == "pixel_inf":
        # a whole pixel at +inf in one feature, and two neighbour samples equal to two of its own samples in every feature
        # (the infinite one included): they pass its 3-sigma test, |inf - inf| = NaN never rejects
        y, x = _nonflat_pixel(planes, f0, 5, 6)
        planes[k, y, x, :] = np.inf
        planes[f0:, y, x + 1, 1] = planes[f0:, y, x, 1]
        planes[f0:, y + 1, x, 2] = planes[f0:, y, x, 2]
        return [(y, x), (y, x + 1), (y + 1, x)]
    if kind == "sample_inf":
        planes[k, 4, 7, 3] = np.inf
        return [(4, 7)]
    if kind == "mixed_inf":                     # +inf and -inf in one feature of one pixel: a NaN mean (the nan_flag path)
        planes[k, 6, 8, 0], planes[k, 6, 8, 5] = np.inf, -np.inf
        return [(6, 8)]
    if kind == "random_inf":
        planes[5, 5, 9, 2] = np.inf
        return [(5, 9)]
    planes[3, 6, 5, 4] = np.inf                 # colour_inf: green
    return [(6, 5)]


@pytest.mark.parametrize("kind", INF_INJECTIONS)
@pytest.mark.parametrize("mode,flat", [("smooth", 0.0), ("smooth", 0.5), ("clustered", 0.0), ("clustered", 0.5)])
@pytest.mark.parametrize("layout", [19, 27])
def test_infinite_features_vs_oracle(hipmod, oracle, layout, mode, flat, kind):
    """+-inf in the feature, random-parameter and colour planes, under both policies, on the default route and the count-first
    route: membership (size, order) the oracle's bits everywhere, the oracle's NaN pattern, status and first bad pixel, and
    every stage output where the oracle's colours are finite.  A pixel whose samples hold +inf in a feature has mean +inf and
    (EPS) sigma 0: it is NOT flat -- neighbour samples at +inf in that feature pass its test."""
    W, H, S = 16, 12, 8
    sf, sc = (0.05, 1e-4) if mode == "smooth" else (1e-3, 0.01)
    kw = dict(L27, dtype="f16") if layout == 27 else {}
    planes = fb.synth_planes(W, H, S, seed=61, sigma_f=sf, sigma_c=sc, mode=mode, flat_frac=flat, **kw)
    pix = _inject_inf(planes, layout, kind)
    lay = dict(L27, plane_dtype=hipmod.PLANES_F16) if layout == 27 else {}
    olay = L27 if layout == 27 else {}
    for policy in (hipmod.DEGEN_EPS, hipmod.DEGEN_REF_ABORT):
        want = oracle.filter_pass(planes.astype(np.float32), oracle.make_desc(W, H, S, box=7, policy=policy, **olay))
        if kind == "pixel_inf" and policy == hipmod.DEGEN_EPS:
            assert want["nbhd_size"][pix[0]] > S      # the samples a flat proof resting on "mean is not NaN" drops
        for cf in (-1, 1):
            got = _run_opts(hipmod, planes, hipmod.make_desc(W, H, S, policy=policy, **lay), 7, [("count_first", cf)])
            tag = (policy, cf)
            assert np.array_equal(got["nbhd_size"], want["nbhd_size"]), tag
            assert np.array_equal(got["member_hash"], want["member_hash"]), tag
            assert (got["status"] == hipmod.E_NONFINITE) == (want["status"] == 1), tag
            assert got["nonfinite_pixels"] == want["nonfinite_pixels"], tag
            assert got["first_bad_pixel"] == want["first_bad_pixel"], tag
            assert np.array_equal(np.isnan(got["colour"]), np.isnan(want["colour"])), tag
            if np.isfinite(want["colour"]).all():
                check_pass(got, want)
            else:
                fin = np.isfinite(want["colour"])
                assert rel_l2(got["colour"][fin], want["colour"][fin]) <= REL_L2_BAR, tag


@pytest.mark.parametrize("W,S,R,kclass", [(1920, 8, 2, "K7"), (3840, 32, 1, "K25"), (1920, 64, 1, "K49")])
def test_headline_regime_full_width_stages(ctx, hipmod, oracle, W, S, R, kclass):
    """The bench's buffer (bench.py: mode "smooth", sigma_f 0.05, sigma_c 1e-4), R full-width rows at the frame centre with
    their halo: every stage output against the oracle, not only the colours -- on this buffer the filter barely moves a
    colour, so membership, bins, MI, alpha, beta and W_r_c are what a wrong kernel would change."""
    b = 3
    H = 2 * b + R
    planes = fb.synth_planes(W, H, S, row0=540 - b, mode="smooth", sigma_f=0.05, sigma_c=1e-4)
    rows = (b, b + R)
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, row_begin=b, row_end=b + R, policy=hipmod.DEGEN_EPS), box=7)
    route = ctx.route()
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7, row_begin=b, row_end=b + R, policy=oracle.DEGEN_EPS))
    check_pass(got, want, rows=rows)
    assert rel_l2(got["colour"][:, b:b + R], want["colour"][:, b:b + R]) <= REL_L2_BAR
    assert got["nonfinite_pixels"] == want["nonfinite_pixels"] == 0
    mean_n = want["sum_nbhd"] / (W * R)
    assert got["sum_nbhd"] == want["sum_nbhd"] and got["max_nbhd"] == want["max_nbhd"]
    if kclass == "K7":       # the bench's 1080p x 8 regime: mean N ~ 295 on the fused route's one-wave K = 7 kernel
        assert 64 < got["max_nbhd"] <= 7 * 64 and mean_n > 250 and route == 0
    else:                    # the four-wave classes of the split route: K = 25 (832 < N <= 1600), K = 49 (N > 1600)
        assert mean_n > 832 and route == 2
        if kclass == "K49":
            assert mean_n > 1600


def test_randomised_parity_sweep_flat_wide_nonfinite(hipmod, oracle):
    """A second seeded sweep over what test_randomised_parity_sweep never draws: flat pixels, the 27-dim fp16 layout, 72 spp
    at box 5, one route option per case (each on a fresh context), +-inf / NaN samples.  Same assertions."""
    rng = np.random.default_rng(515151)
    opts = [o for o in ROUTE_OPTIONS]
    for i in range(30):
        box = int(rng.choice([3, 5, 5, 7, 7, 9]))
        smax = max(1, 3136 // (box * box))
        S = int(rng.choice([s for s in (1, 3, 4, 8, 8, 12, 16, 24, 32, 48, 64, 72) if s <= smax]))
        W, H = int(rng.integers(3, 22)), int(rng.integers(2, 15))
        while W * H * S > 30000:
            W, H = max(3, W - 2), max(2, H - 1)
        layout = 27 if i % 4 == 1 else 19
        mode = str(rng.choice(["smooth", "clustered"]))
        sf = float(rng.choice([1e-5, 1e-3, 0.02, 0.05]))
        flat = float(rng.choice([0.0, 0.5, 0.94]))
        policy = int(rng.choice([hipmod.DEGEN_EPS, hipmod.DEGEN_EPS, hipmod.DEGEN_REF_ABORT]))
        beta = int(rng.integers(0, 3))
        opt = opts[int(rng.integers(0, len(opts)))]
        if opt == ("table_in_lds", 1) and box * box * S > 832:
            opt = ("table_in_lds", 0)      # a forced LDS table beside the K = 25 / 49 kernels' LDS can exceed 160 KiB: refused
        if opt == ("waves_per_pixel", 4) and layout == 27:
            opt = ("waves_per_pixel", 1)   # (forced four-wave runs are drawn for the reference layout only)
        kw = dict(L27, dtype="f16") if layout == 27 else {}
        planes = fb.synth_planes(W, H, S, seed=int(rng.integers(0, 1 << 30)), sigma_f=sf, sigma_c=0.01, mode=mode,
                                 flat_frac=flat, **kw)
        f0 = 9 if layout == 27 else 7
        inject = ("none", "nan", "inf_pixel", "inf_sample", "inf_mixed")[int(rng.integers(1, 5))] if i % 3 == 0 else "none"
        y, x, s = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(0, S))
        k = f0 + int(rng.integers(0, 12))
        if inject == "nan":
            planes[k, y, x, s] = np.nan
        elif inject == "inf_pixel":
            planes[k, y, x, :] = np.inf
            planes[f0:, y, (x + 1) % W, s] = planes[f0:, y, x, s]
        elif inject == "inf_sample":
            planes[k, y, x, s] = np.inf
        elif inject == "inf_mixed":
            planes[k, y, x, s], planes[k, y, x, (s + 1) % S] = np.inf, -np.inf
        lay = dict(L27, plane_dtype=hipmod.PLANES_F16) if layout == 27 else {}
        olay = L27 if layout == 27 else {}
        got = _run_opts(hipmod, planes, hipmod.make_desc(W, H, S, policy=policy, beta_map=beta, **lay), box, [opt])
        want = oracle.filter_pass(planes.astype(np.float32), oracle.make_desc(W, H, S, box=box, policy=policy, beta_map=beta, **olay))
        tag = (i, W, H, S, box, layout, mode, sf, flat, policy, beta, opt, inject)
        assert got["nonfinite_pixels"] == want["nonfinite_pixels"], tag
        if np.isfinite(want["colour"]).all():
            check_pass(got, want)
        else:
            for k in ("nbhd_size", "member_hash", "bin_hash"):
                assert (got[k] == want[k]).all(), (k, tag)
            assert (np.isfinite(got["colour"]) == np.isfinite(want["colour"])).all(), tag
