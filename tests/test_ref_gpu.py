"""GPU tests against the COMPILED reference's own output (tests/golden/ref_filter.npz, ref_film.npz: see
test_ref_fixtures.py): the HIP filter passes under REF_ABORT against the real ApplyRPFFilter's colours, and the device film
step against the real pbrt Film.  These compare the HIP path with the reference directly; the comparisons with the oracle
and with the NumPy film restatement are test_gpu_parity.py's and test_film_gpu.py's.  Nothing here needs the reference
tree or oracle/_ref/."""
import ctypes as C
import os

import numpy as np
import pytest

from raytracer_rpf_amd import feature_buffer as fb
from test_film_gpu import film_device
from test_ref_fixtures import FilmCases, FilterCases

pytestmark = pytest.mark.gpu

REL_L2_BAR = 1e-4  # BASELINE north star: "<= 1e-4 relative L2 on identical feature buffers"


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))


@pytest.fixture(scope="module")
def fcases():
    return FilterCases()


@pytest.fixture(scope="module")
def film_cases():
    return FilmCases()


def check_against_reference(fcases, i, colour, status, hipmod, what):
    assert (status == hipmod.E_NONFINITE) == bool(fcases.aborted[i]), (what, fcases.names[i], status)
    if fcases.aborted[i]:
        return None
    assert status == hipmod.OK
    want = fcases.colour(i)
    assert np.array_equal(np.isfinite(colour), np.isfinite(want)), (what, fcases.names[i])
    r = rel_l2(colour, want)
    print("%s %-28s rel-L2 against the reference %.3e (activity %.3e)" % (what, fcases.names[i], r, fcases.activity[i]))
    assert r <= REL_L2_BAR, (what, fcases.names[i], r)
    return r


def test_filter_pass_against_reference(ctx, hipmod, fcases):
    """rpf_filter_pass_debug, one box, policy REF_ABORT: the reference's colours within the bar, every colour finite where
    it completed, E_NONFINITE on exactly the cases where it stopped"""
    n = 0
    for i in range(len(fcases)):
        boxes = fcases.boxes(i)
        if len(boxes) != 1:
            continue
        planes = fcases.planes(i)
        _, H, W, S = planes.shape
        got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_REF_ABORT), box=boxes[0], debug=False,
                                    allow_nonfinite=True)
        check_against_reference(fcases, i, got["colour"], got["status"], hipmod, "filter_pass_debug")
        n += 1
    assert n >= 18


def test_filter_against_reference_every_case_and_box_list(ctx, hipmod, fcases):
    """rpf_filter (the passes of the descriptor's box list, double-precision colours from pass to pass) on every case"""
    lists = 0
    for i in range(len(fcases)):
        planes, boxes = fcases.planes(i), fcases.boxes(i)
        _, H, W, S = planes.shape
        desc = hipmod.make_desc(W, H, S, boxes=tuple(boxes), policy=hipmod.DEGEN_REF_ABORT)
        srgb, _, st, c64 = ctx.filter(planes, desc, want_colour64=True, allow_nonfinite=True)
        r = check_against_reference(fcases, i, c64, st, hipmod, "filter")
        if r is not None:
            assert np.array_equal(srgb, c64.astype(np.float32))
            lists += len(boxes) > 1
    assert lists >= 3


def test_multi_filter_against_reference(hipmod, fcases):
    """rpf_multi_filter on two slabs of device 0: the fp32 sample colours against the reference's within the bar;
    E_NONFINITE where the reference stopped.  A frame whose slabs would be thinner than the halo of its box list is refused
    by rpf_multi (E_BADARG) and is not counted."""
    ran = lists = 0
    with hipmod.MultiContext([0, 0]) as mc:
        for i in range(len(fcases)):
            planes, boxes = fcases.planes(i), fcases.boxes(i)
            _, H, W, S = planes.shape
            desc = hipmod.make_desc(W, H, S, boxes=tuple(boxes), policy=hipmod.DEGEN_REF_ABORT)
            try:
                srgb, _, st = mc.filter(planes, desc, allow_nonfinite=True)
            except hipmod.RpfError as e:
                assert e.status == hipmod.E_BADARG, (fcases.names[i], e)
                continue
            assert (st == hipmod.E_NONFINITE) == bool(fcases.aborted[i]), (fcases.names[i], st)
            if not fcases.aborted[i]:
                want = fcases.colour(i)
                r = rel_l2(srgb, want)
                print("multi_filter %-28s rel-L2 against the reference %.3e" % (fcases.names[i], r))
                assert np.isfinite(srgb).all() and r <= REL_L2_BAR, (fcases.names[i], r)
                ran += 1
                lists += len(boxes) > 1
    assert ran >= 8 and lists >= 1, (ran, lists)


def test_host_mirror_against_reference(hipmod, fcases):
    """the C++ mirror of ApplyRPFFilter (AoS doubles in SamplingFilm order) on the {7, 5} case"""
    i = fcases.names.index("cl_12x10x8_b7_5")
    planes, boxes = fcases.planes(i), fcases.boxes(i)
    _, H, W, S = planes.shape
    lib = C.CDLL(os.path.join(os.path.dirname(hipmod.LIB_PATH), "librpf_host.so"))
    aos = fb.planes_to_aos(planes)
    err = C.create_string_buffer(256)
    st = lib.rpf_host_apply_filter_aos(aos.ctypes.data_as(C.c_void_p), None, W, H, S, (C.c_int32 * len(boxes))(*boxes), len(boxes),
                                       0, 0, 0, None, err, 256)
    assert st == 0, err.value
    got = np.transpose(aos[..., 2:5], (3, 1, 0, 2))  # [x][y][s][c] -> [c][y][x][s]
    r = rel_l2(got, fcases.colour(i))
    print("host mirror %s rel-L2 against the reference %.3e" % (fcases.names[i], r))
    assert r <= REL_L2_BAR


def _film_of(hipmod, c):
    return hipmod.make_film(c["bounds"], (c["rx"], c["ry"]), c["table"], sample_origin=c["origin"],
                            max_sample_luminance=c["max_lum"], scale=c["scale"])


def test_film_step_against_reference_film(ctx, hipmod, film_cases):
    """rpf_film_splat_device with the real Film's own table: tile sums, weight sums and image equal to the real Film's, bit
    for bit, in all eleven cases (all five filters)"""
    for i in range(len(film_cases)):
        c = film_cases.case(i)
        got = film_device(ctx, hipmod, c["pfilm"], c["colour"].astype(np.float64), _film_of(hipmod, c), c["ray_weight"])
        for g, key in zip(got, ("tile_rgb", "tile_weight", "image")):
            assert g.shape == c[key].shape and np.array_equal(g, c[key], equal_nan=True), (c["name"], key, np.argwhere(g != c[key])[:5])


def test_film_step_with_library_table_against_reference_film(ctx, hipmod, film_cases):
    """the same eleven cases with the table rpf_film_filter_table computes (rpf_filter_film needs a box list, so the film
    step's own doorway rpf_film_splat_device is the one without filter passes): nothing of the fixture but the inputs
    reaches the device, and the sums and the image are still the real Film's to the bit"""
    for i in range(len(film_cases)):
        c = film_cases.case(i)
        film = hipmod.make_film(c["bounds"], (c["rx"], c["ry"]), hipmod.film_table(c["kind"], (c["rx"], c["ry"]), c["p0"], c["p1"]),
                                sample_origin=c["origin"], max_sample_luminance=c["max_lum"], scale=c["scale"])
        got = film_device(ctx, hipmod, c["pfilm"], c["colour"].astype(np.float64), film, c["ray_weight"])
        for g, key in zip(got, ("tile_rgb", "tile_weight", "image")):
            assert np.array_equal(g, c[key], equal_nan=True), (c["name"], key)
