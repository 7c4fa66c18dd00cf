"""CPU tests of RPF_FLAG_SCHEDULE_FUSED: the constant and its hip.py name, the new bit through
rpf_layout_kernels / rpf_max_nbhd / rpf_max_draws on every word of the seventeen older bits, and the frames of
tests/test_schedule_fused_gpu.py -- the size classes each reaches and the share of clamped and of open entries at its gains, from
the oracle (the reference's test) or tests/member_test_ref.py (the configured test), so that the GPU cases are known to exercise
both arms of the clamp on the kernels they are here for.

The table below is the GPU file's too.  Needs no device."""
import functools
import os
import re

import numpy as np
import pytest

import member_test_ref as MR
import schedule_ref as SRf
from raytracer_rpf_amd import feature_buffer as fb

EPS = 1
SIGMA = 0.5
SHARE = 0.05   # the least share of clamped, and of open, entries a parity case must have (alpha, and beta's factor)
CAPS = (8, 16, 32, 64, 128, 256, 448, 832, 1600, 3136)   # the resident classes of routes 0 to 2 and 10
STREAM = 65535                                           # the name of the streaming class
FLAT = dict(flat_frac=0.94)

# name: W, H, S, box, generator arguments, the membership test (None: the reference's 3 sigma; else the floors as a multiple of
# preset 1's), (gain_c, gain_f), the classes the frame is here for, whether both arms of the clamp must hold SHARE of the entries
CASES = {
    "packed": (6, 5, 6, 3, dict(), None, (1.15, 1.6), (16, 32, 64), True),
    "wave": (12, 10, 8, 7, dict(), None, (1.15, 1.6), (64, 128, 256, 448), True),
    "b11": (16, 13, 8, 11, dict(), None, (1.15, 1.6), (128, 256, 448, 832, 1600), True),       # nmax 968: the split classes
    "b15s16": (16, 15, 16, 15, dict(), None, (1.8, 1.6), (832, 1600, 3136, STREAM), True),
    "b17s16": (18, 17, 16, 17, dict(), None, (2.0, 1.6), (1600, 3136, STREAM), True),          # > 4096 candidates
    "m-k7": (12, 10, 8, 7, FLAT, 1.0, (1.1, 2.0), (128, 256, 448), True),
    "m-b11": (16, 13, 8, 11, FLAT, 1.0, (1.1, 2.0), (448, 832, 1600), True),
    "m-b15s16": (16, 15, 16, 15, FLAT, 1.0, (1.8, 2.0), (1600, 3136, STREAM), True),
    "m-packed": (6, 5, 2, 5, dict(), 0.1, (1.8, 1.8), (8, 16, 32), True),
    # class 8 without the membership test: N = 2 .. 6, almost every MI of such a pixel is degenerate (a NaN that EPS turns into 0:
    # W_r = 0, alpha = 1), so neither arm of the clamp holds a share worth asserting: the frame is here for the bit checks of the
    # G = 8 packed kernel alone
    "packed8": (6, 5, 2, 5, dict(), None, (1.15, 1.6), (8,), False),
}
REFERENCE_ROWS = [n for n, c in CASES.items() if c[5] is None]
MEMBER_ROWS = [n for n, c in CASES.items() if c[5] is not None]


@functools.lru_cache(maxsize=None)
def frame(W, H, S, seed=11, **kw):
    p = fb.synth_planes(W, H, S, seed=seed, **kw)
    p.setflags(write=False)
    return p


def planes_of(name):
    W, H, S, _, kw, _, _, _, _ = CASES[name]
    return frame(W, H, S, **kw)


def mt_of(name):
    scale = CASES[name][5]
    return None if scale is None else MR.published19(scale)


def class_of(n):
    return next((c for c in CAPS if n <= c), STREAM)


def classes_of(nbhd):
    return {class_of(int(n)) for n in np.asarray(nbhd).ravel()}


_restated = {}


def restated(oracle, name):
    """(nbhd_size, mi) of the case's unscheduled pass by the oracle or the membership restatement: computed once, shared, never modified"""
    if name not in _restated:
        W, H, S, box = CASES[name][:4]
        if mt_of(name) is None:
            want = oracle.filter_pass(planes_of(name), oracle.make_desc(W, H, S, box=box, policy=EPS, sigma_seed=SIGMA))
        else:
            want = MR.member_pass(oracle, planes_of(name), mt_of(name), box, SIGMA, EPS)
        _restated[name] = (want["nbhd_size"], want["mi"])
    return _restated[name]


# ---- the frames of the GPU file ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_cases_reach_their_classes_and_both_arms_of_the_clamp(oracle, name):
    n, mi = restated(oracle, name)
    gc, gf = CASES[name][6]
    ac, ao = SRf.shares(mi, gc, "c", 1e-10)
    bc, bo = SRf.shares(mi, gf, "f", 1e-10)
    classes = classes_of(n)
    print("SCHEDULE_FUSED %s: N %d .. %d, classes %s, gains (%g, %g): alpha clamped / open %.3f / %.3f, beta factor %.3f / %.3f" % (
        name, n.min(), n.max(), sorted(classes), gc, gf, ac, ao, bc, bo))
    assert set(CASES[name][7]) <= classes, (CASES[name][7], sorted(classes))
    if CASES[name][8]:
        assert min(ac, ao) >= SHARE and min(bc, bo) >= SHARE, (ac, ao, bc, bo)
    else:
        assert n.max() <= 8 and (~(np.abs(mi) > 0)).mean() > 0.5                  # (exempt from SHARE: see CASES)


# ---- the constant -----------------------------------------------------------------------------------------------------------------
def test_constant_and_header(hipmod):
    assert hipmod.SCHEDULE_FUSED_FLAG == 131072
    assert not any(getattr(hipmod, n) == 131072 for n in dir(hipmod) if n.startswith("FLAG_"))
    older = [v for n, v in vars(hipmod).items() if (n.startswith("FLAG_") or n.endswith("_FLAG")) and isinstance(v, int) and n != "SCHEDULE_FUSED_FLAG"]
    assert len(older) == 17 and sum(older) == 131071 and all(hipmod.SCHEDULE_FUSED_FLAG & v == 0 for v in older)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rpf_hip.h")).read()
    m = re.search(r"\bRPF_FLAG_SCHEDULE_FUSED\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == hipmod.SCHEDULE_FUSED_FLAG


# ---- rpf_layout_kernels, rpf_max_nbhd, rpf_max_draws ---------------------------------------------------------------------------------
def test_layout_kernels_on_every_word_of_the_older_bits(hipmod):
    """with the new bit: RPF_E_UNSUPPORTED where the word lacks RPF_FLAG_SCHEDULE, else the answer of the word without the bit"""
    X, F = hipmod.SCHEDULE_FUSED_FLAG, hipmod.SCHEDULE_FLAG
    d = hipmod.make_desc(12, 10, 8)
    refused = accepted = 0
    for w in range(1 << 17):
        d.flags = w | X
        got = hipmod.layout_kernels(d)
        if not (w & F):
            assert got[0] == hipmod.E_UNSUPPORTED, w
            refused += 1
            continue
        d.flags = w
        assert got == hipmod.layout_kernels(d), w
        accepted += got[0] == hipmod.OK
    assert refused == 1 << 16 and accepted > 0
    d.flags = X
    L = hipmod.load()
    import ctypes as C
    g = C.c_int32(-7)
    assert L.rpf_layout_kernels(C.byref(d), C.byref(g)) == hipmod.E_UNSUPPORTED and g.value == -7


def test_layout_kernels_on_a_generic_layout(hipmod):
    """the word list of tests/test_schedule_cpu.py, on the reference layout and on one only the layout-generic kernels take"""
    X, F = hipmod.SCHEDULE_FUSED_FLAG, hipmod.SCHEDULE_FLAG
    words = [0, hipmod.FLAG_GENERIC, hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED, hipmod.FLAG_WIDE_NBHD, hipmod.FLAG_FAST_WEIGHTS,
             hipmod.FLAG_GENERIC_PACKED, hipmod.FLAG_GENERIC | hipmod.FLAG_STREAM_FAST, hipmod.MEMBER_TEST_FLAG, hipmod.SAMPLED_NBHD_FLAG,
             hipmod.FLAG_GENERIC | hipmod.FLAG_FAST_WEIGHTS, hipmod.MEMBER_TEST_FLAG | hipmod.MEMBER_FUSED_FLAG]
    for w in words:
        for lay in (dict(), dict(n_random=3, n_feat=7), dict(n_random=4, n_feat=18, plane_dtype=hipmod.PLANES_F16)):
            plain, sched = hipmod.make_desc(12, 10, 8, flags=w, **lay), hipmod.make_desc(12, 10, 8, flags=w | F, **lay)
            alone, both = hipmod.make_desc(12, 10, 8, flags=w | X, **lay), hipmod.make_desc(12, 10, 8, flags=w | F | X, **lay)
            assert hipmod.layout_kernels(alone)[0] == hipmod.E_UNSUPPORTED, (w, lay)
            assert hipmod.layout_kernels(both) == hipmod.layout_kernels(sched) == hipmod.layout_kernels(plain), (w, lay)
            for d in (alone, both):                                                   # neither reads the bit
                assert hipmod.max_nbhd(d) == hipmod.max_nbhd(plain), (w, lay)
                assert hipmod.max_draws(d) == hipmod.max_draws(plain), (w, lay)
