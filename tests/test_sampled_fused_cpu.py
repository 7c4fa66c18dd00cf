"""CPU tests of RPF_FLAG_SAMPLED_FUSED (route 11): the constant and its hip.py name, the new bit through
rpf_layout_kernels over every flag word of the older bits, rpf_max_nbhd / rpf_max_draws, the descriptor's size, the option's name
and range, and the slab helpers' refusal.  Before the feature the constant does not exist, a word with bit 262144 is answered as
the word without it and the option is unknown, so every test here but test_desc_keeps_its_size fails."""
import ctypes as C

import pytest

LAYOUTS = [(0, 0, 0), (4, 18, 1), (3, 7, 1), (9, 27, 0)]
OLDER = 262144   # flag words 0 .. 262143: every bit below the new one


def test_the_constant_and_its_name(hipmod):
    assert hipmod.SAMPLED_FUSED_FLAG == 262144
    # outside the FLAG_* family, for SAMPLED_NBHD_FLAG's reason (tests/test_flag_table_cpu.py holds the family to its bits)
    assert not any(k.startswith("FLAG_") and getattr(hipmod, k) == 262144 for k in dir(hipmod))
    older = (hipmod.SAMPLED_NBHD_FLAG | hipmod.SAMPLED_REST_FLAG | hipmod.MEMBER_TEST_FLAG | hipmod.MEMBER_FUSED_FLAG | hipmod.SCHEDULE_FLAG |
             hipmod.SCHEDULE_FUSED_FLAG | hipmod.PASS_REPORT_FLAG)
    assert hipmod.SAMPLED_FUSED_FLAG & older == 0 and older < OLDER


def test_desc_keeps_its_size(hipmod):
    assert C.sizeof(hipmod.Desc) == 104


@pytest.mark.parametrize("lay", LAYOUTS, ids=["%d-%d-%d" % lay for lay in LAYOUTS])
def test_flag_table_of_the_new_bit(hipmod, lay):
    """every word of the eleven FLAG_* bits, with every combination of the seven newer bits below this one: with the new bit the
    answer is RPF_E_UNSUPPORTED when the word lacks SAMPLED_NBHD_FLAG, otherwise exactly the answer of the word without the bit"""
    nr, nf, dt = lay
    d0 = hipmod.make_desc(8, 8, 4, n_random=nr, n_feat=nf, plane_dtype=dt)
    d1 = hipmod.make_desc(8, 8, 4, n_random=nr, n_feat=nf, plane_dtype=dt)
    F, N = hipmod.SAMPLED_FUSED_FLAG, hipmod.SAMPLED_NBHD_FLAG
    accepted = 0
    for flags in range(OLDER):
        d0.flags, d1.flags = flags, flags | F
        a1 = hipmod.layout_kernels(d1)
        if not flags & N:
            assert a1 == (hipmod.E_UNSUPPORTED, None), flags
        else:
            assert a1 == hipmod.layout_kernels(d0), flags
            accepted += a1[0] == hipmod.OK
    assert accepted > 0 or (nr, nf) == (9, 27)          # (9, 27): outside RPF_MAX_NDIM, refused with and without


def test_max_nbhd_and_max_draws_do_not_read_the_bit(hipmod):
    F, N, R = hipmod.SAMPLED_FUSED_FLAG, hipmod.SAMPLED_NBHD_FLAG, hipmod.SAMPLED_REST_FLAG
    for extra in (0, N, N | R, N | hipmod.FLAG_WIDE_NBHD, N | R | hipmod.MEMBER_TEST_FLAG | hipmod.SCHEDULE_FLAG | hipmod.SCHEDULE_FUSED_FLAG):
        for S in (1, 8, 832, 833, 3136):
            a, b = hipmod.make_desc(8, 8, S, flags=extra), hipmod.make_desc(8, 8, S, flags=extra | F)
            assert hipmod.max_nbhd(a) == hipmod.max_nbhd(b)
            assert hipmod.max_draws(a) == hipmod.max_draws(b)
    # the bound of a sampled pass is check_sampled's, not the route's: 832 without SAMPLED_REST_FLAG, whatever route 11 could hold
    assert hipmod.max_draws(hipmod.make_desc(8, 8, 8, flags=N | F)) == (hipmod.OK, 824)
    assert hipmod.max_draws(hipmod.make_desc(8, 8, 8, flags=N | R | F)) == (hipmod.OK, hipmod.SAMPLED_MAX - 8)
    assert hipmod.max_nbhd(hipmod.make_desc(8, 8, 4, flags=N | F)) == (hipmod.OK, 65535)


def test_option_name_and_range(hipmod):
    assert hipmod.check_option("sampled_fused_stride", -1) == hipmod.OK
    for v in (0, 6, 36, 153, 378, 1024):
        assert hipmod.check_option("sampled_fused_stride", v) == hipmod.OK
    for v in (-2, 1025):
        assert hipmod.check_option("sampled_fused_stride", v) == hipmod.E_BADARG
    # the names that existed answer as rpf_set_option answers them
    assert hipmod.check_option("wide", 1) == hipmod.OK and hipmod.check_option("wide", 0) == hipmod.E_BADARG
    assert hipmod.check_option("no_such_option", 0) == hipmod.E_BADARG


def test_slabs_helpers_refuse_the_flag(hipmod):
    from raytracer_rpf_amd import slabs
    desc = hipmod.make_desc(8, 8, 4, flags=hipmod.SAMPLED_NBHD_FLAG | hipmod.SAMPLED_FUSED_FLAG)
    with pytest.raises(NotImplementedError):
        slabs.check_desc(desc)
    film = hipmod.make_film(((0, 0), (8, 8)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX))
    with pytest.raises(NotImplementedError):
        slabs.film_halo_rows(desc, film)
