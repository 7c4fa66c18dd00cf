"""CPU tests of the spike pass (RPF_FLAG_SPIKE_CLAMP): the restatement tests/spike_ref.py pinned to
hand-worked pixels, its energy balance, the host-only fold rpf_spike_delta against it bit for bit, the binding's additions and
the host mirror's scene-file keys.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import spike_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one_pixel(values, t):
    """a 1 x 1 frame whose three channels all hold `values`"""
    c = np.array([values, values, values], np.float64).reshape(3, 1, 1, len(values))
    return R.apply(c, t)


def test_hand_worked_pixel():
    """S = 4, [1, 1, 1, 100], t = 1: m = 25.75, sd = sqrt(3 * 24.75^2 + 74.25^2) / 2 = 42.87, only |100 - m| = 74.25 exceeds it;
    m' = 3 / 3 = 1, e = 99, delta = 99 / 4"""
    r = one_pixel([1.0, 1.0, 1.0, 100.0], 1.0)
    assert (r["spike_samples"], r["spike_pixels"], r["skipped_pixels"]) == (1, 1, 0)
    assert np.array_equal(r["clamped"], np.ones((3, 1, 1, 4)))
    assert np.array_equal(r["row_sums"], [[99.0, 99.0, 99.0]]) and np.array_equal(r["energy"], [99.0] * 3)
    assert np.array_equal(r["delta"], [24.75] * 3)
    assert np.array_equal(r["colour"], np.full((3, 1, 1, 4), 25.75))  # the pixel's mean is what it was: 103 / 4
    r0 = R.apply(np.array([1.0, 1.0, 1.0, 100.0] * 3).reshape(3, 1, 1, 4), 1.0, preserve_energy=False)
    assert np.array_equal(r0["colour"], np.ones((3, 1, 1, 4))) and np.array_equal(r0["delta"], [24.75] * 3)


def test_two_samples_strict_comparison_and_skip():
    """S = 2, values 1 and 3: |c - m| = 1 = sd exactly, the test is strict, so t = 1 flags nothing; t = 0.5 flags both, the
    pixel is skipped and keeps its colours"""
    r = one_pixel([1.0, 3.0], 1.0)
    assert (r["spike_samples"], r["spike_pixels"], r["skipped_pixels"]) == (0, 0, 0)
    assert np.array_equal(r["colour"][0, 0, 0], [1.0, 3.0])
    r = one_pixel([1.0, 3.0], 0.5)
    assert (r["spike_samples"], r["spike_pixels"], r["skipped_pixels"]) == (0, 0, 1)
    assert np.array_equal(r["colour"][0, 0, 0], [1.0, 3.0]) and np.array_equal(r["delta"], [0.0] * 3)


def test_one_sample_is_never_a_spike():
    for v in (0.0, 1.0, 1e30, -3.5):
        r = one_pixel([v], 1e-6)
        assert (r["spike_samples"], r["spike_pixels"], r["skipped_pixels"]) == (0, 0, 0)
        assert np.array_equal(r["colour"], np.full((3, 1, 1, 1), v))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nonfinite_pixel_is_left_as_it_is(bad):
    """a NaN or an infinite colour on one channel, a firefly on another: nothing is flagged, nothing spreads"""
    c = np.ones((3, 1, 2, 6))
    c[0, 0, 0, 2] = bad
    c[1, 0, 0, 5] = 1e6  # channel 1 alone would flag sample 5
    c[2, 0, 1, 0] = 50.0  # the finite neighbour pixel is clamped as usual
    r = R.apply(c, 1.0)
    assert r["spike_pixels"] == 1 and r["spike_samples"] == 1
    want = c[:, 0, 0] + r["delta"][:, None]
    assert np.array_equal(r["colour"][:, 0, 0], want, equal_nan=True)
    assert np.isfinite(r["delta"]).all() and np.isfinite(r["colour"][:, 0, 1]).all()
    assert np.array_equal(r["clamped"][:, 0, 0], c[:, 0, 0], equal_nan=True)


@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s[2] >= 2] + [(40, 6, 2)])
def test_energy_is_preserved(shape):
    """|fsum(out) - fsum(in)| <= 4 n 2^-53 max|c| per channel, n = W H S: one rounding per recorded difference, per chain step
    and per final add"""
    W, H, S = shape
    c = R.make_frame(W, H, S, seed=100 + S, specials=False)
    r = R.apply(c, 1.0)
    n = W * H * S
    bound = 4.0 * n * 2.0 ** -53 * float(np.abs(c).max())
    for k in range(3):
        err = abs(math.fsum(r["colour"][k].ravel().tolist()) - math.fsum(c[k].ravel().tolist()))
        print("shape", shape, "channel", k, "error", err, "bound", bound, "spike_samples", r["spike_samples"])
        assert err <= bound
    assert r["spike_samples"] > 0  # (at S = 2 as well: a rounded mean leaves one sample further from it than sd)


def test_restatement_is_not_vacuous_on_the_gpu_frames():
    """the frames of tests/test_spike_gpu.py: spikes and a non-zero delta on every frame where t^2 < S - 1, skipped pixels wherever
    the frame plants one (six pixels and more, S >= 2) at t = 1"""
    skipped = 0
    for i, (W, H, S) in enumerate(R.SHAPES):
        c = R.make_frame(W, H, S, seed=i)
        for t in R.THRESHOLDS:
            r = R.apply(c, t)
            skipped += r["skipped_pixels"]
            # (no sample of S lies further than sqrt(S - 1) standard deviations from their mean: t = 2.5 can flag nothing up to S = 7)
            if S - 1 > t * t:
                assert r["spike_samples"] > 0 and r["spike_pixels"] > 0, (W, H, S, t)
                assert (r["delta"] != 0).any() and np.isfinite(r["delta"]).all(), (W, H, S, t)
            if t == 1.0 and W * H >= 6 and S >= 2:
                assert r["skipped_pixels"] > 0, (W, H, S)
            assert not np.isfinite(r["colour"]).all()  # the NaN pixel and the inf sample are still there
    assert skipped > 0


def test_spike_delta_equals_the_restatement_fold(hipmod):
    rng = np.random.default_rng(5)
    cases = [rng.normal(0, 1e3, (17, 3)), -np.abs(rng.normal(0, 1, (5, 3))), np.zeros((4, 3)), np.array([[1e300, -1.0, 0.0]] * 3),
             np.array([[0.1, -0.0, 5.0]]), rng.lognormal(0, 8, (1080, 3)) * rng.choice([-1.0, 1.0], (1080, 3))]
    cases[0][3] = 0.0
    for rows in cases:
        for n in (1, 7, rows.shape[0] * 1920 * 8):
            E, d = hipmod.spike_delta(rows, n)
            E2, d2 = R.fold(rows, n)
            assert np.array_equal(E.view(np.uint64), E2.view(np.uint64)) and np.array_equal(d.view(np.uint64), d2.view(np.uint64))
    L = hipmod.load()
    e, d = np.empty(3), np.empty(3)
    rows = np.zeros((2, 3))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.rpf_spike_delta(None, 2, 6, p(e), p(d)) == hipmod.E_BADARG
    assert L.rpf_spike_delta(p(rows), 2, 6, None, p(d)) == hipmod.E_BADARG
    assert L.rpf_spike_delta(p(rows), 2, 6, p(e), None) == hipmod.E_BADARG
    assert L.rpf_spike_delta(p(rows), 0, 6, p(e), p(d)) == hipmod.E_BADARG
    assert L.rpf_spike_delta(p(rows), 2, 0, p(e), p(d)) == hipmod.E_BADARG
    assert L.rpf_spike_delta(p(rows), -1, 6, p(e), p(d)) == hipmod.E_BADARG


def test_binding_and_abi_additions(hipmod):
    assert hipmod.FLAG_SPIKE_CLAMP == 1024
    flags = [getattr(hipmod, n) for n in dir(hipmod) if n.startswith("FLAG_")]
    assert len(set(flags)) == len(flags)  # the new bit collides with no other flag
    # rpf_spike_stats: 3 int64, 6 doubles, a float and an int32
    assert C.sizeof(hipmod.SpikeStats) == 3 * 8 + 6 * 8 + 4 + 4 and hipmod.SpikeStats.applied.offset == 76
    for name in ("rpf_set_spike", "rpf_multi_set_spike", "rpf_query_spike", "rpf_multi_query_spike", "rpf_spike_clamp_device",
                 "rpf_colour_add_device", "rpf_spike_delta"):
        assert name in hipmod.EXPORTS and hasattr(hipmod.load(), name)
    # the flag is independent of every route flag: the layout answers are those of the same flags without it
    for fl in (0, hipmod.FLAG_GENERIC, hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED, hipmod.FLAG_WIDE_NBHD, hipmod.FLAG_GENERIC_PACKED,
               hipmod.FLAG_FAST_WEIGHTS | hipmod.FLAG_GENERIC):
        for lay in (dict(), dict(n_random=3, n_feat=5)):
            a = hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=fl, **lay))
            b = hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=fl | hipmod.FLAG_SPIKE_CLAMP, **lay))
            assert a == b
        assert hipmod.max_nbhd(hipmod.make_desc(8, 8, 4, flags=fl)) == hipmod.max_nbhd(hipmod.make_desc(8, 8, 4, flags=fl | hipmod.FLAG_SPIKE_CLAMP))


def test_host_mirror_spike_keys(hipmod):
    """RPFParams::ParseSpike through its C doorway: the defaults, the accepted values, the refused thresholds"""
    lib = C.CDLL(os.path.join(os.path.dirname(hipmod.LIB_PATH), "librpf_host.so"))
    f = lib.rpf_host_parse_spike_params
    f.restype = C.c_int32
    f.argtypes = [C.c_int32, C.c_double, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_char_p, C.c_int32]

    def parse(clamp, thr, energy):
        a, b, c_, err = C.c_int32(-1), C.c_double(-1), C.c_int32(-1), C.create_string_buffer(256)
        st = f(clamp, thr, energy, C.byref(a), C.byref(b), C.byref(c_), err, 256)
        return st, (a.value, b.value, c_.value), err.value.decode()

    assert parse(0, 1.0, 1) == (0, (0, 1.0, 1), "")  # what a scene file without the keys gives
    assert parse(1, 2.5, 0) == (0, (1, 2.5, 0), "")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        st, _, msg = parse(1, bad, 1)
        assert st == -1 and "spikethreshold" in msg
    # Parse keeps its signature and knows nothing of the new keys
    g = lib.rpf_host_parse_params
    g.restype = C.c_int32
    n, be, err = C.c_int32(0), C.c_int32(-1), C.create_string_buffer(256)
    boxes = (C.c_int32 * 8)()
    assert g(None, 0, b"hip", boxes, C.byref(n), C.byref(be), err, 256) == 0 and n.value == 1 and boxes[0] == 7
