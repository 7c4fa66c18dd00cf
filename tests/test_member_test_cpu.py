"""CPU tests of the membership test (RPF_FLAG_MEMBER_TEST): the presets and the setters' argument checks
(host only), the new bit through rpf_layout_kernels, the binding, the slab helpers' refusal -- and the restatement
tests/member_test_ref.py itself: its reduction to the reference's member lists, and the regime change the feature is for."""
import ctypes as C

import numpy as np
import pytest

import member_test_ref as MR
import sampled_ref as SR
from raytracer_rpf_amd import feature_buffer as fb

EPS = 1


# ---- rpf_membership_preset ----------------------------------------------------------------------------------------------------
def test_presets_values(hipmod):
    ref = hipmod.membership_preset(hipmod.MEMBERSHIP_REFERENCE, 12)
    assert list(ref.mult) == [3.0] * hipmod.MAX_NDIM and list(ref.floor) == [-1.0] * hipmod.MAX_NDIM
    for nf in (1, 7, 34, hipmod.MAX_NDIM):
        m = hipmod.membership_preset(0, nf)
        assert list(m.mult) == [3.0] * hipmod.MAX_NDIM and list(m.floor) == [-1.0] * hipmod.MAX_NDIM
    pub = hipmod.membership_preset(hipmod.MEMBERSHIP_PUBLISHED_19, 12)
    mult, floor = MR.published19()
    assert list(pub.mult)[:12] == mult.tolist() == [3, 3, 3, 30, 30, 30, 3, 3, 3, 30, 30, 30]
    assert list(pub.floor)[:12] == floor.tolist() == [0.1] * 12
    assert list(pub.mult)[12:] == [3.0] * (hipmod.MAX_NDIM - 12) and list(pub.floor)[12:] == [-1.0] * (hipmod.MAX_NDIM - 12)
    rm, rf = MR.reference()
    assert list(ref.mult)[:12] == rm.tolist() and list(ref.floor)[:12] == rf.tolist()


def test_presets_refusals(hipmod):
    L = hipmod.load()
    m = hipmod.Membership()
    assert L.rpf_membership_preset(0, 12, None) == hipmod.E_BADARG
    for kind, nf in [(-1, 12), (2, 12), (0, 0), (0, -3), (0, hipmod.MAX_NDIM + 1), (1, 11), (1, 13), (1, 18)]:
        assert L.rpf_membership_preset(kind, nf, C.byref(m)) == hipmod.E_BADARG, (kind, nf)
        with pytest.raises(hipmod.RpfError) as e:
            hipmod.membership_preset(kind, nf)
        assert e.value.status == hipmod.E_BADARG


def test_struct_layout_exports_and_null_handles(hipmod):
    M = hipmod.Membership
    assert C.sizeof(M) == 2 * 8 * hipmod.MAX_NDIM and (M.mult.offset, M.floor.offset) == (0, 8 * hipmod.MAX_NDIM)
    assert C.sizeof(hipmod.Desc) == 104                             # rpf_desc keeps its layout
    assert hipmod.MEMBER_TEST_FLAG == 4096
    L = hipmod.load()
    for sym in ("rpf_set_membership", "rpf_multi_set_membership", "rpf_membership_preset"):
        assert sym in hipmod.EXPORTS and hasattr(L, sym)
    cfg = hipmod.membership_preset(0)
    assert L.rpf_set_membership(None, C.byref(cfg)) == hipmod.E_BADARG     # no context: no device is asked for
    assert L.rpf_multi_set_membership(None, C.byref(cfg)) == hipmod.E_BADARG
    m = hipmod.make_membership([3, 30], 0.25)
    assert list(m.mult)[:3] == [3.0, 30.0, 3.0] and list(m.floor) == [0.25] * hipmod.MAX_NDIM


# ---- the new bit through rpf_layout_kernels -------------------------------------------------------------------------------
LAYOUTS = [(0, 0, 0), (4, 18, 1), (3, 7, 1), (9, 27, 0)]


@pytest.mark.parametrize("lay", LAYOUTS, ids=["%d-%d-%d" % lay for lay in LAYOUTS])
def test_flag_table_of_the_new_bit(hipmod, lay):
    """words 4096 .. 8191: refused exactly when one of the three fp32 pair-weight flags is set or the word without the bit is
    refused; otherwise the answer of the word without the bit"""
    nr, nf, dt = lay
    fp32 = hipmod.FLAG_FAST_WEIGHTS | hipmod.FLAG_GENERIC_FAST | hipmod.FLAG_STREAM_FAST
    refused_more = 0
    for flags in range(4096):
        desc = dict(n_random=nr, n_feat=nf, plane_dtype=dt)
        st0, g0 = hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=flags, **desc))
        st1, g1 = hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=flags | hipmod.MEMBER_TEST_FLAG, **desc))
        if (flags & fp32) or st0 != hipmod.OK:
            assert (st1, g1) == (hipmod.E_UNSUPPORTED, None), flags
            refused_more += st0 == hipmod.OK
        else:
            assert (st1, g1) == (st0, g0), flags
    assert refused_more > 0 or (nr, nf) == (9, 27)      # (9, 27): outside RPF_MAX_NDIM, refused with and without


def test_max_nbhd_is_unchanged(hipmod):
    assert hipmod.max_nbhd(hipmod.make_desc(8, 8, 4, flags=hipmod.MEMBER_TEST_FLAG)) == (hipmod.OK, 65535)
    assert hipmod.max_nbhd(hipmod.make_desc(8, 8, 4, flags=hipmod.MEMBER_TEST_FLAG | hipmod.FLAG_WIDE_NBHD)) == (hipmod.OK, 262144)


def test_slabs_helpers_refuse_the_flag(hipmod):
    from raytracer_rpf_amd import slabs
    desc = hipmod.make_desc(8, 8, 4, flags=hipmod.MEMBER_TEST_FLAG)
    with pytest.raises(NotImplementedError, match="set_membership"):
        slabs.check_desc(desc)
    film = hipmod.make_film(((0, 0), (8, 8)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX))
    with pytest.raises(NotImplementedError):
        slabs.film_halo_rows(desc, film)
    plain = hipmod.make_desc(8, 8, 4)
    assert slabs.check_desc(plain) is plain


# ---- the restatement -------------------------------------------------------------------------------------------------------
# The tests below exercise tests/member_test_ref.py alone: the yardstick's anchor (with the reference's multiples and floors it
# lists what sampled_ref.full_box_codes, the 3-sigma predicate, lists) and the regime the feature exists for.  They pass without
# the library and are no evidence for it.
def frame(flat):
    return fb.synth_planes(12, 10, 8, seed=11, **(dict(flat_frac=0.94) if flat else {}))


@pytest.mark.parametrize("flat", [False, True], ids=["smooth", "flat94"])
def test_restatement_reduces_to_the_reference_lists(oracle, flat):
    planes, box = frame(flat), 7
    _, H, W, S = planes.shape
    pmean, pstd = oracle.pixel_stats(planes, oracle.make_desc(W, H, S, policy=EPS))
    for y in range(H):
        for x in range(W):
            _, codes = MR.members(planes, pmean, pstd, MR.reference(), y, x, box)
            assert codes.tolist() == SR.full_box_codes(planes, pmean, pstd, y, x, box), (y, x)


def test_predicate_special_values():
    m, sd = np.zeros(1), np.ones(1)
    f = np.array([[0.5], [3.0], [np.nan], [np.inf], [-np.inf]])
    assert MR.rejected(f, m, sd, [3.0], [-1.0]).tolist() == [False, True, False, True, True]
    # a NaN mean or deviation never rejects; a zero deviation rejects all under a negative floor, only beyond a positive one
    assert not MR.rejected(f, np.array([np.nan]), sd, [3.0], [-1.0]).any()
    assert not MR.rejected(f, m, np.array([np.nan]), [3.0], [0.1]).any()
    assert MR.rejected(f, m, np.zeros(1), [3.0], [-1.0]).tolist() == [True, True, False, True, True]
    assert MR.rejected(f, m, np.zeros(1), [3.0], [1.0]).tolist() == [False, True, False, True, True]
    # sd above the floor: the floor plays no part
    assert MR.rejected(f, m, sd, [0.1], [0.9]).tolist() == [True, True, False, True, True]
    # sd at or below the floor: a deviation within the floor is kept although it is beyond the multiple
    assert MR.rejected(f, m, sd, [0.1], [1.0]).tolist() == [False, True, False, True, True]


def test_regime_change_on_the_captured_like_frame(oracle):
    """12x10x8, flat_frac 0.94, box 7: the reference's test leaves N = S on at least 90 % of the pixels; the published preset on
    none, and reaches the one-wave classes 128, 256 and 448"""
    planes, box, S = frame(True), 7, 8
    n_ref, _ = MR.counts(oracle, planes, MR.reference(), box)
    n_pub, _ = MR.counts(oracle, planes, MR.published19(), box)
    assert (n_ref == S).mean() >= 0.90
    assert (n_pub == S).sum() == 0
    classes = {MR.class_of(int(n)) for n in n_pub.ravel()}
    print("regime: N = S on %.1f %% -> %.1f %%, mean N %.1f -> %.1f, classes %s"
          % (100 * (n_ref == S).mean(), 100 * (n_pub == S).mean(), n_ref.mean(), n_pub.mean(), sorted(classes)))
    assert {128, 256, 448} <= classes
