"""The fused kernels keep a neighbourhood as sample offsets relative to the first sample of the pixel's window and gather
through a wave-uniform plane base (Window, csrc/rpf_filter_impl.inc).  What that can break and the small frames of
test_gpu_parity.py do not pin together: a slab whose owned rows start below halo rows (the window origin lies above the owned
rows), origins of either parity, a frame wider than 4096 px (relative offsets past 2^18 elements), the fp16 / 27-dim layout
through the split route's weight kernel (which picks halves of dwords by the parity of the element index), a box-17 window
clipped on every side, and the host's refusal of a window span that does not fit 32 bits."""
import numpy as np
import pytest

from raytracer_rpf_amd import feature_buffer as fb

REL_L2_BAR = 1e-4  # the project's bar on filtered colours; the stage outputs below are compared bit for bit


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def check_stages(got, want, rows=None):
    """membership, bins, mean and SD bit for bit (an offset slip changes them at once); MI, alpha, beta, W_r_c and the colours
    within the bounds test_gpu_parity.check_pass uses"""
    sl = slice(None) if rows is None else slice(*rows)
    for k in ("nbhd_size", "member_hash", "bin_hash"):
        assert (got[k][sl] == want[k][sl]).all(), k
    assert np.array_equal(got["mean"][sl], want["mean"][sl], equal_nan=True)
    assert np.array_equal(got["stddev"][sl], want["stddev"][sl], equal_nan=True)
    np.testing.assert_allclose(got["mi"][sl], want["mi"][sl], rtol=0, atol=1e-11)
    for k in ("alpha", "beta", "wrc"):
        np.testing.assert_allclose(got[k][sl], want[k][sl], rtol=1e-9, atol=1e-12)
    assert rel_l2(got["colour"], want["colour"]) <= REL_L2_BAR
    assert got["sum_nbhd"] == want["sum_nbhd"] and got["max_nbhd"] == want["max_nbhd"]


def test_window_span_refusal_needs_no_device(hipmod):
    """box * W * S * 8 bytes must fit 32 bits; the check is a pure function of the C ABI"""
    L = hipmod.load()
    assert L.rpf_check_window_span(1920, 8, 7) == hipmod.OK
    assert L.rpf_check_window_span(8192, 64, 55) == hipmod.OK
    assert L.rpf_check_window_span(2 ** 26 - 1, 8, 1) == hipmod.OK          # 2^32 - 64 bytes
    assert L.rpf_check_window_span(2 ** 26, 8, 1) == hipmod.E_UNSUPPORTED    # 2^32 bytes
    assert L.rpf_check_window_span(2 ** 22, 4, 33) == hipmod.E_UNSUPPORTED
    assert L.rpf_check_window_span(2 ** 30, 64, 255) == hipmod.E_UNSUPPORTED  # no 32-bit wrap in the product
    for bad in ((0, 8, 7), (16, 0, 7), (16, 8, 0), (-4, 8, 7)):
        assert L.rpf_check_window_span(*bad) == hipmod.E_BADARG


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,S,r0,r1", [(33, 11, 8, 3, 8),      # owned rows right below the halo: origins in row 0
                                         (29, 18, 8, 7, 11),     # ... and deeper in the slab: origins in rows 4 .. 7
                                         (31, 13, 5, 4, 9)])     # odd S and W: window origins of either parity
def test_slab_rows_below_halo_rows(ctx, hipmod, oracle, W, H, S, r0, r1):
    planes = fb.synth_planes(W, H, S, seed=23, row0=100, mode="smooth", sigma_f=0.05, sigma_c=1e-4)
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, row_begin=r0, row_end=r1, policy=hipmod.DEGEN_EPS), box=7)
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7, row_begin=r0, row_end=r1, policy=oracle.DEGEN_EPS))
    check_stages(got, want, rows=(r0, r1))
    assert want["sum_nbhd"] / (W * (r1 - r0)) > 64      # large neighbourhoods: the fused kernel's own stages, not the packed ones
    cin = planes[2:5].astype(np.float64)
    assert np.array_equal(got["colour"][:, :r0], cin[:, :r0]) and np.array_equal(got["colour"][:, r1:], cin[:, r1:])


@pytest.mark.gpu
def test_frame_wider_than_4096_px_full_width_rows(ctx, hipmod, oracle):
    """4160 x 8 spp: a window row is 33 280 samples, the last row of a window starts 199 680 samples past its origin"""
    W, S, b, R = 4160, 8, 3, 2
    H = 2 * b + R
    planes = fb.synth_planes(W, H, S, row0=540 - b, mode="smooth", sigma_f=0.05, sigma_c=1e-4)
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, row_begin=b, row_end=b + R, policy=hipmod.DEGEN_EPS), box=7)
    assert ctx.route() == 0
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7, row_begin=b, row_end=b + R, policy=oracle.DEGEN_EPS))
    check_stages(got, want, rows=(b, b + R))
    assert rel_l2(got["colour"][:, b:b + R], want["colour"][:, b:b + R]) <= REL_L2_BAR
    assert 64 < got["max_nbhd"] <= 7 * 64


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,S,r0,r1", [(15, 11, 8, 3, 8),      # one-wave kernels
                                         (9, 9, 33, 2, 7),       # the split route (chains | bins + MI | weights), odd plane stride
                                         (11, 8, 16, 0, 8)])     # K = 13
def test_layout27_fp16_slab(ctx, hipmod, oracle, W, H, S, r0, r1):
    lay = dict(n_random=4, n_feat=18)
    p16 = fb.synth_planes(W, H, S, seed=29, dtype="f16", mode="smooth", sigma_f=0.05, sigma_c=1e-4, **lay)
    desc = hipmod.make_desc(W, H, S, row_begin=r0, row_end=r1, policy=hipmod.DEGEN_EPS, plane_dtype=hipmod.PLANES_F16, **lay)
    got = ctx.filter_pass_debug(p16, desc, box=7)
    want = oracle.filter_pass(p16.astype(np.float32), oracle.make_desc(W, H, S, box=7, row_begin=r0, row_end=r1,
                                                                     policy=oracle.DEGEN_EPS, **lay))
    check_stages(got, want, rows=(r0, r1))


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,S", [(12, 10, 8), (21, 7, 8)])
def test_clipped_box17_window(ctx, hipmod, oracle, W, H, S):
    """box 17 on a frame smaller than the box in one or both directions: every window is clipped, most on all four sides"""
    planes = fb.synth_planes(W, H, S, seed=31, mode="smooth", sigma_f=0.05, sigma_c=1e-4)
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_EPS), box=17)
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=17, policy=oracle.DEGEN_EPS))
    check_stages(got, want)
