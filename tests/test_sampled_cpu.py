"""CPU tests of sampled neighbourhoods (RPF_FLAG_SAMPLED_NBHD): the host-only entry points
rpf_sampling_table and rpf_sampling_draws against the numpy restatement tests/sampled_ref.py, the slab property of the pixel
key, the refusal table of the new bit through rpf_layout_kernels, the struct and the binding.  No device."""
import ctypes as C
import itertools

import numpy as np
import pytest

import sampled_ref as SR

BOXES = (3, 7, 17, 35, 55)


# ---- the table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", BOXES)
def test_table_shape_order_symmetry_and_formula(hipmod, box):
    T = hipmod.sampling_table(box)
    assert T.dtype == np.uint32 and T.shape == (box - 1,)
    t = T.astype(np.int64)
    assert (np.diff(t) >= 0).all()
    # C_k + C_(box-2-k) = C_(box-1): the thresholds mirror around 2^32 to within the two floors
    assert (np.abs(t + t[::-1] - (1 << 32)) <= 1).all(), np.abs(t + t[::-1] - (1 << 32)).max()
    f64 = SR.table(box, np.float64).astype(np.int64)
    assert (np.abs(t - f64) <= 2).all(), np.abs(t - f64).max()
    assert np.array_equal(T, SR.table(box))                      # the long double restatement: the same bits


def test_table_refusals(hipmod):
    out = (C.c_uint32 * 600)()
    L = hipmod.load()
    for box in (0, -3, 8, 512, 513):
        assert L.rpf_sampling_table(box, out) == hipmod.E_BADARG, box
    assert L.rpf_sampling_table(7, None) == hipmod.E_BADARG
    assert L.rpf_sampling_table(511, out) == hipmod.OK
    assert L.rpf_sampling_table(1, out) == hipmod.OK             # no threshold: every draw is the centre


def test_table_is_gaussian_where_it_matters(hipmod):
    """box 55: the centre column's share is 1 / (sigma sqrt(2 pi)) to the discretisation, sigma = 55 / 4"""
    t = np.concatenate([[0], hipmod.sampling_table(55).astype(np.float64), [2.0 ** 32]])
    share = np.diff(t) / 2.0 ** 32
    assert abs(share[27] - 1 / (13.75 * np.sqrt(2 * np.pi))) < 2e-3 and share.argmax() == 27


# ---- the draws ------------------------------------------------------------------------------------------------------------
CASES = [(6, 5, 4, 7, 200), (12, 10, 8, 17, 120)]
KEYS = [(seed, pid, ro) for seed in (1, 0xC0FFEE123456789A) for pid in (0, 3) for ro in (0, 37)]


@pytest.mark.parametrize("seed,pass_id0,row_origin", KEYS, ids=["s%x-p%d-r%d" % k for k in KEYS])
@pytest.mark.parametrize("W,H,S,box,D", CASES, ids=["%dx%dx%d-b%d-D%d" % c for c in CASES])
def test_draws_equal_the_restatement_on_every_pixel(hipmod, W, H, S, box, D, seed, pass_id0, row_origin):
    """pass index 1 of the configuration: the pass id is pass_id0 + 1 and the count is draws[1]"""
    cfg = hipmod.make_sampling(seed, [5, D], pass_id0=pass_id0, row_origin=row_origin)
    b, seen = (box - 1) // 2, dict(dup=0, edge=0, centre=0)
    for y, x in itertools.product(range(H), range(W)):
        got = hipmod.sampling_draws(cfg, 1, box, W, H, S, x, y)
        want = SR.draws(seed, pass_id0 + 1, row_origin, D, box, W, H, S, x, y)
        assert np.array_equal(got, want), ((x, y), got[:8], want[:8])
        assert (np.diff(got) > 0).all() and (got >= 0).all()
        nx, ny = min(x + b, W - 1) - max(x - b, 0) + 1, min(y + b, H - 1) - max(y - b, 0) + 1
        assert got.size == 0 or got[-1] < (nx * ny - 1) * S
        dx, dy, _ = SR.raw_draws(seed, pass_id0 + 1, row_origin, D, box, S, x, y)
        inside = (x + dx >= 0) & (x + dx < W) & (y + dy >= 0) & (y + dy < H)
        centre = (dx == 0) & (dy == 0)
        seen["edge"] += int((~inside).sum())
        seen["centre"] += int(centre.sum())
        seen["dup"] += int((inside & ~centre).sum()) - got.size
    assert min(seen.values()) > 0, seen                             # duplicates, image-edge discards and centre hits all occur


def test_draws_depend_on_seed_pass_and_row(hipmod):
    W, H, S, box, D = 12, 10, 8, 17, 120
    base = hipmod.sampling_draws(hipmod.make_sampling(5, [D]), 0, box, W, H, S, 6, 5)
    for cfg, p in ((hipmod.make_sampling(6, [D]), 0), (hipmod.make_sampling(5, [D], pass_id0=1), 0),
                   (hipmod.make_sampling(5, [D, D]), 1), (hipmod.make_sampling(5, [D], row_origin=1), 0)):
        assert not np.array_equal(hipmod.sampling_draws(cfg, p, box, W, H, S, 6, 5), base)
    # pass index p with pass_id0 = 0 is pass index 0 with pass_id0 = p
    assert np.array_equal(hipmod.sampling_draws(hipmod.make_sampling(5, [D, D]), 1, box, W, H, S, 6, 5),
                          hipmod.sampling_draws(hipmod.make_sampling(5, [D], pass_id0=1), 0, box, W, H, S, 6, 5))


@pytest.mark.parametrize("n_slabs", [2, 3])
def test_slab_property(hipmod, n_slabs):
    """every owned row of a slab (row_origin = a - ht, b halo rows wherever the image has them) gets the lists of the same row
    of the whole image: the key reads the image row, and with >= b halo rows the window's clipping is the image's"""
    W, H, S, box, D = 9, 24, 4, 7, 60
    b = (box - 1) // 2
    slabs, _ = hipmod.halo_plan(H, n_slabs, b)
    whole = hipmod.make_sampling(11, [D], pass_id0=2)
    for a, e, ht, hb in slabs:
        part = hipmod.make_sampling(11, [D], pass_id0=2, row_origin=a - ht)
        Hs = ht + (e - a) + hb
        for yl, x in itertools.product(range(ht, ht + e - a), range(W)):
            got = hipmod.sampling_draws(part, 0, box, W, Hs, S, x, yl)
            want = hipmod.sampling_draws(whole, 0, box, W, H, S, x, a - ht + yl)
            # the visiting-order index counts the window's rows from its first row: the same rows in slab and image
            assert np.array_equal(got, want), (a, yl, x)


def test_draws_refusals(hipmod):
    L, n = hipmod.load(), C.c_int32(0)
    out = (C.c_int32 * 64)()
    cfg = hipmod.make_sampling(1, [8])

    def call(cfg_p, p, box, W, H, S, x, y, o=out, n_p=None):
        return L.rpf_sampling_draws(cfg_p, p, box, W, H, S, x, y, o, C.byref(n) if n_p is None else n_p)
    ok = (C.byref(cfg), 0, 7, 6, 5, 4, 2, 2)
    assert call(*ok) == hipmod.OK
    assert call(None, *ok[1:]) == hipmod.E_BADARG
    assert call(*ok, o=None) == hipmod.E_BADARG
    for bad in [(-1,) + ok[2:], (8,) + ok[2:], (0, 8) + ok[3:], (0, 513) + ok[3:], (0, 7, 0, 5, 4, 0, 0), (0, 7, 6, 5, 0, 2, 2),
                (0, 7, 6, 5, 4, 6, 2), (0, 7, 6, 5, 4, 2, 5), (0, 7, 6, 5, 4, -1, 2)]:
        assert call(C.byref(cfg), *bad) == hipmod.E_BADARG, bad
    neg = hipmod.make_sampling(1, [-1])
    assert call(C.byref(neg), *ok[1:]) == hipmod.E_BADARG
    zero = hipmod.make_sampling(1, [0])
    assert call(C.byref(zero), *ok[1:]) == hipmod.OK and n.value == 0


# ---- the new bit through rpf_layout_kernels -------------------------------------------------------------------------------
LAYOUTS = [(0, 0, 0), (4, 18, 1), (3, 7, 1), (9, 27, 0)]


@pytest.mark.parametrize("lay", LAYOUTS, ids=["%d-%d-%d" % lay for lay in LAYOUTS])
def test_flag_table_of_the_new_bit(hipmod, lay):
    """words 2048 .. 4095: the answer of the same word without the bit, except that the three fp32 pair-weight flags refuse"""
    nr, nf, dt = lay
    fp32 = hipmod.FLAG_FAST_WEIGHTS | hipmod.FLAG_GENERIC_FAST | hipmod.FLAG_STREAM_FAST
    refused_more = 0
    for flags in range(2048):
        desc = dict(n_random=nr, n_feat=nf, plane_dtype=dt)
        st0, g0 = hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=flags, **desc))
        st1, g1 = hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=flags | hipmod.SAMPLED_NBHD_FLAG, **desc))
        if flags & fp32:
            assert (st1, g1) == (hipmod.E_UNSUPPORTED, None), flags
            refused_more += st0 == hipmod.OK
        else:
            assert (st1, g1) == (st0, g0), flags
    assert refused_more > 0 or (nr, nf) == (9, 27)      # (9, 27): outside RPF_MAX_NDIM, refused with and without


def test_max_nbhd_is_unchanged(hipmod):
    assert hipmod.max_nbhd(hipmod.make_desc(8, 8, 4, flags=hipmod.SAMPLED_NBHD_FLAG)) == (hipmod.OK, 65535)
    assert hipmod.max_nbhd(hipmod.make_desc(8, 8, 4, flags=hipmod.SAMPLED_NBHD_FLAG | hipmod.FLAG_WIDE_NBHD)) == (hipmod.OK, 262144)


# ---- the struct and the binding -------------------------------------------------------------------------------------------
def test_struct_layout_and_exports(hipmod):
    S = hipmod.Sampling
    assert C.sizeof(S) == 48
    assert (S.seed.offset, S.pass_id0.offset, S.row_origin.offset, S.draws.offset) == (0, 8, 12, 16)
    assert C.sizeof(hipmod.Desc) == 104                             # rpf_desc keeps its layout
    L = hipmod.load()
    for sym in ("rpf_set_sampling", "rpf_multi_set_sampling", "rpf_sampling_table", "rpf_sampling_draws"):
        assert sym in hipmod.EXPORTS and hasattr(L, sym)
    s = hipmod.make_sampling(0xFFFFFFFFFFFFFFFF, [1, 2, 3], pass_id0=-2, row_origin=-5)
    assert (s.seed, s.pass_id0, s.row_origin, list(s.draws)) == (0xFFFFFFFFFFFFFFFF, -2, -5, [1, 2, 3, 0, 0, 0, 0, 0])


def test_set_sampling_argument_checks_need_no_device(hipmod):
    L = hipmod.load()
    cfg = hipmod.make_sampling(1, [8])
    assert L.rpf_set_sampling(None, C.byref(cfg)) == hipmod.E_BADARG
    assert L.rpf_multi_set_sampling(None, C.byref(cfg)) == hipmod.E_BADARG


def test_slabs_helpers_refuse_the_flag(hipmod):
    from raytracer_rpf_amd import slabs
    desc = hipmod.make_desc(8, 8, 4, flags=hipmod.SAMPLED_NBHD_FLAG)
    with pytest.raises(NotImplementedError, match="row_origin"):
        slabs.check_desc(desc)
    film = hipmod.make_film(((0, 0), (8, 8)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX))
    with pytest.raises(NotImplementedError):
        slabs.film_halo_rows(desc, film)
    plain = hipmod.make_desc(8, 8, 4)
    assert slabs.check_desc(plain) is plain


# ---- the restatement itself -----------------------------------------------------------------------------------------------
# The two tests below exercise tests/sampled_ref.py alone: self-checks of the yardstick (its decode against a written-out window,
# its member lists against the subset property of the definition).  They pass without the library and are no evidence for it.
def test_restatement_decode_inverts_the_numbering():
    W, H, S, box = 6, 5, 4, 7
    for y, x in itertools.product(range(H), range(W)):
        b = 3
        cells = [(xn, yn) for xn in range(max(x - b, 0), min(x + b, W - 1) + 1) for yn in range(max(y - b, 0), min(y + b, H - 1) + 1)
                 if (xn, yn) != (x, y)]
        want = [(xn, yn, s) for xn, yn in cells for s in range(S)]
        xn, yn, s = SR.decode(np.arange(len(want)), box, W, H, S, x, y)
        assert list(zip(xn.tolist(), yn.tolist(), s.tolist())) == want


def test_restatement_members_are_a_subsequence_of_the_full_box(oracle):
    from raytracer_rpf_amd import feature_buffer as fb
    W, H, S, box, D = 12, 10, 8, 7, 56
    planes = fb.synth_planes(W, H, S, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    pmean, pstd = oracle.pixel_stats(planes, oracle.make_desc(W, H, S, policy=1))
    grew = 0
    for y, x in itertools.product(range(H), range(W)):
        nb, codes, _ = SR.members(planes, pmean, pstd, (9, 0, D), 0, y, x, box)
        full = SR.full_box_codes(planes, pmean, pstd, y, x, box)
        assert SR.is_subsequence(codes.tolist(), full) and nb.shape[0] == len(codes) <= len(full)
        grew += len(codes) > S
    assert grew > 0


def test_key_sums_wrap_mod_2_32(hipmod):
    """pass_id0 + pass and row_origin + y enter the key as uint32: a configuration at the end of the int32 range wraps"""
    W, H, S, box, D, top = 6, 5, 4, 7, 60, 2 ** 31 - 1
    cfg = hipmod.make_sampling(3, [0, D], pass_id0=top, row_origin=top)
    for y, x in itertools.product(range(H), range(W)):
        assert np.array_equal(hipmod.sampling_draws(cfg, 1, box, W, H, S, x, y), SR.draws(3, top + 1, top, D, box, W, H, S, x, y))
