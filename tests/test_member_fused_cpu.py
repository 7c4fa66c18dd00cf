"""CPU tests of RPF_FLAG_MEMBER_FUSED (route 10): the constant and its hip.py name, the new bit through
rpf_layout_kernels over every flag word of the older bits, rpf_max_nbhd / rpf_max_draws, the descriptor's size and the slab
helpers' refusal.  Before the feature the constant does not exist and a word with bit 65536 is answered as the word without it,
so every test here but test_desc_keeps_its_size fails."""
import ctypes as C

import pytest

LAYOUTS = [(0, 0, 0), (4, 18, 1), (3, 7, 1), (9, 27, 0)]


def test_the_constant_and_its_name(hipmod):
    assert hipmod.MEMBER_FUSED_FLAG == 65536
    # outside the FLAG_* family, for MEMBER_TEST_FLAG's reason (tests/test_flag_table_cpu.py holds the family to its bits)
    assert not any(k.startswith("FLAG_") and getattr(hipmod, k) == 65536 for k in dir(hipmod))
    assert hipmod.MEMBER_FUSED_FLAG & (hipmod.MEMBER_TEST_FLAG | hipmod.SCHEDULE_FLAG | hipmod.SAMPLED_REST_FLAG | hipmod.PASS_REPORT_FLAG) == 0


def test_desc_keeps_its_size(hipmod):
    assert C.sizeof(hipmod.Desc) == 104


@pytest.mark.parametrize("lay", LAYOUTS, ids=["%d-%d-%d" % lay for lay in LAYOUTS])
def test_flag_table_of_the_new_bit(hipmod, lay):
    """flag words 0 .. 65535: with the new bit the answer is RPF_E_UNSUPPORTED when the word lacks MEMBER_TEST_FLAG, otherwise
    exactly the answer of the word without the bit"""
    nr, nf, dt = lay
    d0 = hipmod.make_desc(8, 8, 4, n_random=nr, n_feat=nf, plane_dtype=dt)
    d1 = hipmod.make_desc(8, 8, 4, n_random=nr, n_feat=nf, plane_dtype=dt)
    F, M = hipmod.MEMBER_FUSED_FLAG, hipmod.MEMBER_TEST_FLAG
    accepted = 0
    for flags in range(65536):
        d0.flags, d1.flags = flags, flags | F
        a0, a1 = hipmod.layout_kernels(d0), hipmod.layout_kernels(d1)
        if not flags & M:
            assert a1 == (hipmod.E_UNSUPPORTED, None), flags
        else:
            assert a1 == a0, flags
            accepted += a1[0] == hipmod.OK
    assert accepted > 0 or (nr, nf) == (9, 27)          # (9, 27): outside RPF_MAX_NDIM, refused with and without


def test_max_nbhd_and_max_draws_do_not_read_the_bit(hipmod):
    F, M = hipmod.MEMBER_FUSED_FLAG, hipmod.MEMBER_TEST_FLAG
    for extra in (0, M, hipmod.FLAG_WIDE_NBHD, M | hipmod.FLAG_WIDE_NBHD, M | hipmod.SAMPLED_NBHD_FLAG | hipmod.SAMPLED_REST_FLAG):
        for S in (1, 8, 832, 833):
            a, b = hipmod.make_desc(8, 8, S, flags=extra), hipmod.make_desc(8, 8, S, flags=extra | F)
            assert hipmod.max_nbhd(a) == hipmod.max_nbhd(b)
            assert hipmod.max_draws(a) == hipmod.max_draws(b)
    assert hipmod.max_nbhd(hipmod.make_desc(8, 8, 4, flags=M | F)) == (hipmod.OK, 65535)


def test_slabs_helpers_refuse_the_flag(hipmod):
    from raytracer_rpf_amd import slabs
    desc = hipmod.make_desc(8, 8, 4, flags=hipmod.MEMBER_TEST_FLAG | hipmod.MEMBER_FUSED_FLAG)
    with pytest.raises(NotImplementedError, match="set_membership"):
        slabs.check_desc(desc)
    film = hipmod.make_film(((0, 0), (8, 8)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX))
    with pytest.raises(NotImplementedError):
        slabs.film_halo_rows(desc, film)
