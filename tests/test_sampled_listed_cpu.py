"""CPU tests of RPF_FLAG_SAMPLED_LISTED (route 12): the constant and its hip.py name, the new bit through
rpf_layout_kernels over every combination of the nine newer bits crossed with a handful of FLAG_* words, rpf_max_nbhd /
rpf_max_draws, the descriptor's size, the option's name and range, and the slab helpers' refusal.  Before the feature the constant
does not exist, a word with bit 524288 is answered as the word without it and the option is unknown, so every test here but
test_desc_keeps_its_size fails."""
import ctypes as C

import pytest

LAYOUTS = [(0, 0, 0), (4, 18, 1), (3, 7, 1), (9, 27, 0)]   # tests/test_sampled_fused_cpu.py's four
NEWER = (2048, 4096, 8192, 16384, 32768, 65536, 131072, 262144, 524288)   # the nine bits above the FLAG_* family


def older_words(hipmod):
    """a fixed handful of FLAG_* words: none, the fp32 flag that sampled passes refuse, each layout-generic route, the wide
    routes, the stream flag with and without what it modifies, the spike clamp, and everything at once"""
    H = hipmod
    gpw = H.FLAG_GENERIC | H.FLAG_GENERIC_PACKED | H.FLAG_GENERIC_WAVE
    return (0, H.FLAG_TIMING | H.FLAG_NO_OVERLAP, H.FLAG_FAST_WEIGHTS, H.FLAG_GENERIC, H.FLAG_GENERIC | H.FLAG_GENERIC_PACKED, gpw,
            gpw | H.FLAG_GENERIC_FAST, H.FLAG_GENERIC_WAVE, H.FLAG_WIDE_NBHD, H.FLAG_WIDE_NBHD | H.FLAG_WIDE_CLASSES, H.FLAG_WIDE_CLASSES,
            H.FLAG_STREAM_FAST, H.FLAG_STREAM_FAST | H.FLAG_WIDE_NBHD, H.FLAG_SPIKE_CLAMP, 2047)


def test_the_constant_and_its_name(hipmod):
    assert hipmod.SAMPLED_LISTED_FLAG == 524288
    assert getattr(hipmod, "SAMPLED_LISTED_FLAG") == 524288 and "SAMPLED_LISTED_FLAG" in dir(hipmod)
    # served by the module's __getattr__ (its _LATER_BITS table), not one more integer of the module's dict:
    # tests/test_schedule_fused_cpu.py::test_constant_and_header counts those
    assert "SAMPLED_LISTED_FLAG" not in vars(hipmod) and hipmod._LATER_BITS["SAMPLED_LISTED_FLAG"] == 524288
    # outside the FLAG_* family, for SAMPLED_NBHD_FLAG's reason (tests/test_flag_table_cpu.py holds the family to its bits)
    assert not any(k.startswith("FLAG_") and getattr(hipmod, k) == 524288 for k in dir(hipmod))
    named = (hipmod.SAMPLED_NBHD_FLAG, hipmod.MEMBER_TEST_FLAG, hipmod.SCHEDULE_FLAG, hipmod.SAMPLED_REST_FLAG, hipmod.PASS_REPORT_FLAG,
             hipmod.MEMBER_FUSED_FLAG, hipmod.SCHEDULE_FUSED_FLAG, hipmod.SAMPLED_FUSED_FLAG, hipmod.SAMPLED_LISTED_FLAG)
    assert named == NEWER
    with pytest.raises(AttributeError):
        hipmod.NO_SUCH_FLAG


def test_desc_keeps_its_size(hipmod):
    assert C.sizeof(hipmod.Desc) == 104


@pytest.mark.parametrize("lay", LAYOUTS, ids=["%d-%d-%d" % lay for lay in LAYOUTS])
def test_flag_table_of_the_new_bit(hipmod, lay):
    """every combination of the nine newer bits (512 words: 256 with the new bit, each against the word without it), crossed with
    the handful of FLAG_* words: with the new bit the answer is RPF_E_UNSUPPORTED when the word lacks SAMPLED_NBHD_FLAG, otherwise
    exactly the answer of the word without the bit"""
    nr, nf, dt = lay
    d0 = hipmod.make_desc(8, 8, 4, n_random=nr, n_feat=nf, plane_dtype=dt)
    d1 = hipmod.make_desc(8, 8, 4, n_random=nr, n_feat=nf, plane_dtype=dt)
    L, N = hipmod.SAMPLED_LISTED_FLAG, hipmod.SAMPLED_NBHD_FLAG
    accepted = words = 0
    for low in older_words(hipmod):
        for combo in range(256):
            flags = low | sum(b for i, b in enumerate(NEWER[:8]) if combo >> i & 1)
            assert not flags & L
            d0.flags, d1.flags = flags, flags | L
            a1 = hipmod.layout_kernels(d1)
            words += 2
            if not flags & N:
                assert a1 == (hipmod.E_UNSUPPORTED, None), flags
            else:
                assert a1 == hipmod.layout_kernels(d0), flags
                accepted += a1[0] == hipmod.OK
    assert words == 512 * len(older_words(hipmod))
    assert accepted > 0 or (nr, nf) == (9, 27)          # (9, 27): outside RPF_MAX_NDIM, refused with and without


def test_the_flag_does_not_need_sampled_fused(hipmod):
    N, L, X = hipmod.SAMPLED_NBHD_FLAG, hipmod.SAMPLED_LISTED_FLAG, hipmod.SAMPLED_FUSED_FLAG
    assert hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=N | L)) == (hipmod.OK, 0)
    assert hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=N | L | X)) == (hipmod.OK, 0)
    assert hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=L | X)) == (hipmod.E_UNSUPPORTED, None)
    assert hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=L)) == (hipmod.E_UNSUPPORTED, None)


def test_max_nbhd_and_max_draws_do_not_read_the_bit(hipmod):
    L, N, R = hipmod.SAMPLED_LISTED_FLAG, hipmod.SAMPLED_NBHD_FLAG, hipmod.SAMPLED_REST_FLAG
    for extra in (0, N, N | R, N | hipmod.FLAG_WIDE_NBHD, N | hipmod.SAMPLED_FUSED_FLAG,
                  N | R | hipmod.MEMBER_TEST_FLAG | hipmod.SCHEDULE_FLAG | hipmod.SCHEDULE_FUSED_FLAG):
        for S in (1, 8, 22, 832, 833, 3136):
            a, b = hipmod.make_desc(8, 8, S, flags=extra), hipmod.make_desc(8, 8, S, flags=extra | L)
            assert hipmod.max_nbhd(a) == hipmod.max_nbhd(b)
            assert hipmod.max_draws(a) == hipmod.max_draws(b)
    # the bounds of a sampled pass are check_sampled's and rpf_max_nbhd's, not the route's: 832 without SAMPLED_REST_FLAG, 65535
    # without FLAG_WIDE_NBHD, whatever route 12 could hold
    assert hipmod.max_draws(hipmod.make_desc(8, 8, 8, flags=N | L)) == (hipmod.OK, 824)
    assert hipmod.max_draws(hipmod.make_desc(8, 8, 8, flags=N | R | L)) == (hipmod.OK, hipmod.SAMPLED_MAX - 8)
    assert hipmod.max_nbhd(hipmod.make_desc(8, 8, 4, flags=N | L)) == (hipmod.OK, 65535)
    assert hipmod.max_nbhd(hipmod.make_desc(8, 8, 4, flags=N | L | hipmod.FLAG_WIDE_NBHD)) == (hipmod.OK, 262144)


def test_option_name_and_range(hipmod):
    assert hipmod.check_option("sampled_listed_stride", -1) == hipmod.OK
    for v in (0, 6, 36, 153, 378, 1024, 1025):
        assert hipmod.check_option("sampled_listed_stride", v) == hipmod.OK
    for v in (-2, 1026):
        assert hipmod.check_option("sampled_listed_stride", v) == hipmod.E_BADARG
    # the names that existed answer as they did
    assert hipmod.check_option("sampled_fused_stride", 1024) == hipmod.OK and hipmod.check_option("sampled_fused_stride", 1025) == hipmod.E_BADARG
    assert hipmod.check_option("wide", 1) == hipmod.OK and hipmod.check_option("wide", 0) == hipmod.E_BADARG
    assert hipmod.check_option("no_such_option", 0) == hipmod.E_BADARG


def test_slabs_helpers_refuse_the_flag(hipmod):
    from raytracer_rpf_amd import slabs
    desc = hipmod.make_desc(8, 8, 4, flags=hipmod.SAMPLED_NBHD_FLAG | hipmod.SAMPLED_LISTED_FLAG)
    with pytest.raises(NotImplementedError):
        slabs.check_desc(desc)
    film = hipmod.make_film(((0, 0), (8, 8)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX))
    with pytest.raises(NotImplementedError):
        slabs.film_halo_rows(desc, film)
