"""CPU tests of RPF_FLAG_SAMPLED_REST (sampled passes with S + draws up to RPF_SAMPLED_MAX = 8192): the
host-only entry point rpf_max_draws, the refusal table of the new bit through rpf_layout_kernels, rpf_sampling_draws at the new
cap against the numpy restatement tests/sampled_ref.py, and the names of the binding.  No device."""
import ctypes as C
import os

import numpy as np
import pytest

import sampled_ref as SR

REST, SAMPLED = 16384, 2048


# ---- rpf_max_draws ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 32, 832, 833, 8192, 9000])
def test_max_draws(hipmod, S):
    plain = hipmod.make_desc(8, 8, S, flags=hipmod.SAMPLED_NBHD_FLAG)
    rest = hipmod.make_desc(8, 8, S, flags=hipmod.SAMPLED_NBHD_FLAG | hipmod.SAMPLED_REST_FLAG)
    assert hipmod.max_draws(plain) == (hipmod.OK, max(0, 832 - S))
    assert hipmod.max_draws(rest) == (hipmod.OK, max(0, 8192 - S))
    assert hipmod.max_draws(hipmod.make_desc(8, 8, S)) == (hipmod.OK, max(0, 832 - S))        # only S and the one flag are read
    assert hipmod.SAMPLED_MAX == 8192


def test_max_draws_refusals(hipmod):
    L, n = hipmod.load(), C.c_int32(-7)
    assert hipmod.max_draws(None) == (hipmod.E_BADARG, None)
    d = hipmod.make_desc(8, 8, 4, flags=hipmod.SAMPLED_REST_FLAG)
    assert L.rpf_max_draws(C.byref(d), None) == hipmod.E_BADARG
    for S in (0, -1):
        d.S = S
        assert L.rpf_max_draws(C.byref(d), C.byref(n)) == hipmod.E_BADARG and n.value == -7, S
    assert "rpf_max_draws" in hipmod.EXPORTS and hasattr(L, "rpf_max_draws")


# ---- the new bit through rpf_layout_kernels -----------------------------------------------------------------------------------
# every layout of the flag table's recording (tests/golden/flag_table.npz, read only)
LAYOUTS = [(0, 0, 0), (2, 12, 0), (4, 18, 1), (4, 18, 0), (2, 12, 1), (3, 7, 0), (1, 1, 0), (8, 27, 1), (9, 27, 0), (0, 0, 2)]


def test_the_layouts_are_those_of_the_flag_table():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flag_table.npz"))
    assert [tuple(l) for l in g["layouts"].tolist()] == LAYOUTS


@pytest.mark.parametrize("lay", LAYOUTS, ids=["%d-%d-%d" % lay for lay in LAYOUTS])
def test_flag_table_of_the_new_bit(hipmod, lay):
    """words 16384 + w, w < 2048: refused without RPF_FLAG_SAMPLED_NBHD; words 16384 + 2048 + w: the answer of 2048 + w"""
    nr, nf, dt = lay
    desc = dict(n_random=nr, n_feat=nf, plane_dtype=dt)
    accepted = 0
    for flags in range(2048):
        assert hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=flags | REST, **desc)) == (hipmod.E_UNSUPPORTED, None), flags
        without = hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=flags | SAMPLED, **desc))
        assert hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=flags | SAMPLED | REST, **desc)) == without, flags
        accepted += without[0] == hipmod.OK
    assert accepted > 0 or (nr, nf, dt) in ((9, 27, 0), (0, 0, 2))   # outside RPF_MAX_NDIM | an unknown plane type: refused with and without


def test_max_nbhd_is_unchanged(hipmod):
    F = hipmod.SAMPLED_NBHD_FLAG | hipmod.SAMPLED_REST_FLAG
    assert hipmod.max_nbhd(hipmod.make_desc(8, 8, 4, flags=F)) == (hipmod.OK, 65535)
    assert hipmod.max_nbhd(hipmod.make_desc(8, 8, 4, flags=F | hipmod.FLAG_WIDE_NBHD)) == (hipmod.OK, 262144)


# ---- rpf_sampling_draws at the new cap ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", [7, 17])
@pytest.mark.parametrize("x,y", [(0, 0), (13, 5), (7, 6)], ids=["corner", "edge", "centre"])
def test_draws_at_the_cap_equal_the_restatement(hipmod, box, x, y):
    W, H, S, D, seed = 14, 12, 32, 8160, 0x5EED5EED
    got = hipmod.sampling_draws(hipmod.make_sampling(seed, [D]), 0, box, W, H, S, x, y)
    want = SR.draws(seed, 0, 0, D, box, W, H, S, x, y)
    assert np.array_equal(got, want) and (np.diff(got) > 0).all()
    assert 0 < got.size < D                              # duplicates and discards: fewer distinct indices than draws


# ---- the names of the binding -------------------------------------------------------------------------------------------------
def test_names(hipmod):
    names = [n for n in dir(hipmod) if n.startswith("FLAG_")]
    assert sorted(getattr(hipmod, n) for n in names) == [1 << k for k in range(11)], names
    assert hipmod.SAMPLED_REST_FLAG == REST and hipmod.SAMPLED_NBHD_FLAG == SAMPLED
