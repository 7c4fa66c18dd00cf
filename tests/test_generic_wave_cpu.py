"""The one-wave generic route's device-free surface (RPF_FLAG_GENERIC | RPF_FLAG_GENERIC_PACKED | RPF_FLAG_GENERIC_WAVE,
rpf_query_route 5): the flag's value, rpf_layout_kernels' truth table with it, and -- against the oracle, on the CPU -- what
tests/test_generic_wave_gpu.py takes for granted about its frames, so that a GPU failure is never a property of the input.
The frames are built here and imported by the GPU file."""
import os
import re

import numpy as np
import pytest

import planted_nbhd as P
from raytracer_rpf_amd import feature_buffer as fb
from test_gpu_parity import INF_INJECTIONS, _independent_columns, _inject_inf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, REF_ABORT = 1, 0

LAYOUTS = [(1, 1, "f32"), (3, 7, "f32"), (5, 13, "f16"), (8, 27, "f32"), (2, 12, "f32"), (4, 18, "f16")]
CAPS = (8, 16, 32, 64, 128, 256, 448, 832)       # four packed lane classes, four one-wave classes; beyond: the rest list
# id: layout (None: every entry of LAYOUTS), S, box, planted N per target
FRAMES = {
    "E16": (None, 16, 7, (16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 448, 449, 784)),
    "E32": ((3, 7, "f32"), 32, 7, (832, 833, 1568)),                 # the last wave class | the streaming kernel
    "E72": ((3, 7, "f32"), 72, 3, (72, 128, 129, 448, 449, 648)),    # S > 64: no packed pixel
}
# pixels per class (<= 8, 16, 32, 64, 128, 256, 448, 832, rest) as the oracle counts them
E16_CLASSES = {
    (1, 1, "f32"): [0, 1, 2, 2, 2, 6, 196, 428, 0],
    (3, 7, "f32"): [0, 1, 2, 2, 2, 64, 429, 137, 0],
    (5, 13, "f16"): [0, 1, 2, 2, 32, 358, 196, 46, 0],
    (8, 27, "f32"): [0, 1, 2, 35, 260, 173, 126, 40, 0],
    (2, 12, "f32"): [0, 1, 2, 2, 19, 328, 241, 44, 0],
    (4, 18, "f16"): [0, 1, 2, 4, 149, 290, 149, 42, 0],
}
E32_CLASSES = [0, 0, 0, 0, 0, 0, 7, 83, 57]
E72_CLASSES = [0, 0, 0, 0, 2, 3, 38, 11, 0]
RESIDUE_LAY, RESIDUE_W, RESIDUE_BOX = (3, 7, "f32"), 3, 7
RESIDUE_S = (99, 143)                            # class N <= 128 | class N <= 256


def lay_ids(v):
    return "%d-%d-%s" % v if isinstance(v, tuple) else None


def stored_and_image(p32, lay):
    """the stored planes (an f16 layout is rounded once) and their exact fp32 image, which is what the oracle reads"""
    stored = p32.astype(np.float16) if lay[2] == "f16" else p32
    p32 = stored.astype(np.float32)
    stored.setflags(write=False)
    p32.setflags(write=False)
    return stored, p32


def class_counts(n):
    """pixels per class: N <= 8, 16, 32, 64, 128, 256, 448, 832, rest"""
    out, lo = [], 0
    for cap in CAPS:
        out.append(int(((n > lo) & (n <= cap)).sum()))
        lo = cap
    return out + [int((n > lo).sum())]


def geometry(fid):
    _, S, box, targets = FRAMES[fid]
    return box * len(targets), box, S, box       # W, H, S, box


_frames = {}


def frame(fid, lay):
    """(stored planes, fp32 image, target pixels) of a planted frame: built once per layout, read-only"""
    if (fid, lay) not in _frames:
        _, S, box, targets = FRAMES[fid]
        p32, pixels = P.plant(S, box, targets, n_random=lay[0], n_feat=lay[1], seed=0)
        _frames[fid, lay] = stored_and_image(p32, lay) + (pixels,)
    return _frames[fid, lay]


_want = {}


def frame_oracle(oracle, fid, lay, policy, sigma_seed=0.002):
    """the oracle's pass of a planted frame: computed once per session, shared, never modified"""
    key = (fid, lay, policy, sigma_seed)
    if key not in _want:
        W, H, S, box = geometry(fid)
        _want[key] = oracle.filter_pass(frame(fid, lay)[1], oracle.make_desc(W, H, S, box=box, policy=policy, sigma_seed=sigma_seed,
                                                                             n_random=lay[0], n_feat=lay[1]))
    return _want[key]


_residue = {}


def residue_frame(oracle, S):
    """3 x 1 x S in the (3, 7, f32) layout: every column of every pixel a permutation of k / (S - 1); pFilm.x = pixel +
    uniform; r0 and f0 carry the exactly independent pair of columns, the same pattern in every pixel; the last feature is
    shifted by 16 per pixel, so nobody accepts a neighbour and N = S.  Returns (stored planes, fp32 image, index of the
    independent pair)."""
    if S not in _residue:
        nr, nf, _ = RESIDUE_LAY
        W, ndim = RESIDUE_W, 5 + nr + nf
        rng = np.random.default_rng(3)
        planes = np.empty((ndim, 1, W, S), np.float32)
        for c in range(ndim):
            for x in range(W):
                planes[c, 0, x] = rng.permutation(S) / (S - 1.0)
        planes[0, 0] = (np.arange(W)[:, None] + rng.random((W, S))).astype(np.float32)
        a, b = _independent_columns(S, int(np.sqrt(S)))
        planes[5, 0], planes[5 + nr, 0] = a.astype(np.float32), b.astype(np.float32)
        planes[ndim - 1, 0] += (16.0 * np.arange(W, dtype=np.float32))[:, None]
        pa, pb = oracle.pair_table(nr, nf)
        indep = [i for i in range(len(pa)) if (pa[i], pb[i]) == (5 + nr, 5)]
        assert len(indep) == 1
        _residue[S] = stored_and_image(planes, RESIDUE_LAY) + (indep,)
    return _residue[S]


_residue_want = {}


def residue_oracle(oracle, S, policy):
    if (S, policy) not in _residue_want:
        nr, nf, _ = RESIDUE_LAY
        _residue_want[S, policy] = oracle.filter_pass(residue_frame(oracle, S)[1],
                                                      oracle.make_desc(RESIDUE_W, 1, S, box=RESIDUE_BOX, policy=policy, n_random=nr, n_feat=nf))
    return _residue_want[S, policy]


INF_SHAPE = (16, 12, 8, 7)                       # W, H, S, box


def inf_frame(kind):
    """the smooth reference-layout frame of the non-finite cases with `kind` injected: (planes, injected pixels)"""
    W, H, S, _ = INF_SHAPE
    planes = fb.synth_planes(W, H, S, seed=61, sigma_f=0.05, sigma_c=1e-4, mode="smooth")
    return planes, _inject_inf(planes, 19, kind)


# ---- the flag and the truth table --------------------------------------------------------------------------------------------
def test_flag_matches_the_header_and_is_a_bit_of_its_own(hipmod):
    with open(os.path.join(ROOT, "include", "rpf_hip.h")) as f:
        m = re.search(r"\bRPF_FLAG_GENERIC_WAVE\s*=\s*(\d+)", f.read())
    assert m and hipmod.FLAG_GENERIC_WAVE == int(m.group(1)) == 32
    others = hipmod.FLAG_TIMING | hipmod.FLAG_FAST_WEIGHTS | hipmod.FLAG_NO_OVERLAP | hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED
    assert hipmod.FLAG_GENERIC_WAVE & others == 0


@pytest.mark.parametrize("lay,flags,want", [
    (dict(n_random=2, n_feat=12, plane_dtype=0), "GPW", ("OK", 1)),
    (dict(n_random=4, n_feat=18, plane_dtype=1), "GPW", ("OK", 1)),
    (dict(n_random=1, n_feat=1), "GPW", ("OK", 1)),
    (dict(n_random=8, n_feat=27), "GPW", ("OK", 1)),
    (dict(), "GPWT", ("OK", 1)),
    (dict(n_random=9, n_feat=27), "GPW", ("E_UNSUPPORTED", None)),               # 41 dims
    (dict(), "W", ("E_UNSUPPORTED", None)),                                      # the flag modifies G | P
    (dict(n_random=3, n_feat=7), "W", ("E_UNSUPPORTED", None)),
    (dict(n_random=3, n_feat=7), "GW", ("E_UNSUPPORTED", None)),
    (dict(n_random=3, n_feat=7), "PW", ("E_UNSUPPORTED", None)),
    (dict(), "GPWF", ("E_UNSUPPORTED", None)),                                   # the generic kernels are fp64 throughout
])
def test_layout_kernels_truth_table_with_the_wave_flag(hipmod, lay, flags, want):
    bits = {"G": hipmod.FLAG_GENERIC, "P": hipmod.FLAG_GENERIC_PACKED, "W": hipmod.FLAG_GENERIC_WAVE, "F": hipmod.FLAG_FAST_WEIGHTS,
            "T": hipmod.FLAG_TIMING}
    st, generic = hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=sum(bits[c] for c in flags), **lay))
    assert (st, generic) == (getattr(hipmod, want[0]), want[1])


# ---- input conditions of the GPU tests, against the oracle -----------------------------------------------------------------
@pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
@pytest.mark.parametrize("lay", LAYOUTS, ids=lay_ids)
def test_e16_targets_classes_and_status(oracle, lay, policy):
    want = frame_oracle(oracle, "E16", lay, policy)
    n = want["nbhd_size"]
    assert [int(n[y, x]) for y, x in frame("E16", lay)[2]] == list(FRAMES["E16"][3])
    cc = class_counts(n)
    assert cc == E16_CLASSES[lay], cc
    assert all(k > 0 for k in cc[1:8]) and cc[8] == 0     # every wave class and every occupied packed class is non-empty
    assert want["status"] == 0 and np.isfinite(want["colour"]).all()


@pytest.mark.parametrize("lay", LAYOUTS, ids=lay_ids)
def test_e16_active_seed_moves_the_colours(oracle, lay):
    want = frame_oracle(oracle, "E16", lay, EPS, P.ACTIVE_SIGMA_SEED)
    cin = frame("E16", lay)[1][2:5].astype(np.float64)
    assert np.isfinite(want["colour"]).all()
    assert np.linalg.norm(want["colour"] - cin) / np.linalg.norm(cin) > 0.10


@pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
@pytest.mark.parametrize("fid,classes", [("E32", E32_CLASSES), ("E72", E72_CLASSES)])
def test_e32_e72_targets_and_classes(oracle, fid, classes, policy):
    lay = FRAMES[fid][0]
    want = frame_oracle(oracle, fid, lay, policy)
    n = want["nbhd_size"]
    assert [int(n[y, x]) for y, x in frame(fid, lay)[2]] == list(FRAMES[fid][3])
    assert class_counts(n) == classes
    # E72's box of 3 gives sigma_p = 3 / 4 = 0 (rpf.cpp:531, integer division): every pixel's weights are NaN, EPS falls back
    # to the input colour and REF_ABORT reports all 54 pixels
    if fid == "E72":
        assert want["status"] == (0 if policy == EPS else 1) and want["nonfinite_pixels"] == 54
        assert np.isnan(want["colour"]).all() == (policy == REF_ABORT)
    else:
        assert want["status"] == 0 and np.isfinite(want["colour"]).all()


@pytest.mark.parametrize("S", RESIDUE_S)
def test_residue_frames(oracle, S):
    _, _, indep = residue_frame(oracle, S)
    ref = residue_oracle(oracle, S, REF_ABORT)
    assert (ref["nbhd_size"] == S).all() and ref["nbhd_size"].size == RESIDUE_W
    ri = ref["mi"][..., indep]
    assert (ri != 0).all() and (np.abs(ri) < 1e-14).all()              # real residue in all three pixels
    assert (residue_oracle(oracle, S, EPS)["mi"][..., indep] == 0).all()


@pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
@pytest.mark.parametrize("kind", INF_INJECTIONS)
def test_inf_frame_neighbourhoods_are_wave_sized(oracle, kind, policy):
    """the injected pixels and their window neighbours run on the one-wave kernels: N in (64, 832].  One exception, which no
    frame at 8 spp can avoid: under EPS a pixel with an infinite own sample ("pixel_inf", "sample_inf") has its NaN sigma
    clamped to 0, rejects every finite candidate and keeps N <= 17 -- a packed class; every other pixel of its window is
    wave-sized, and under REF_ABORT (a NaN limit never rejects) so is the pixel itself."""
    W, H, S, box = INF_SHAPE
    planes, pix = inf_frame(kind)
    n = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=policy))["nbhd_size"]
    wave = (n > 64) & (n <= 832)
    small_own = policy == EPS and kind in ("pixel_inf", "sample_inf")
    b = (box - 1) // 2
    for y, x in pix:
        assert bool(wave[y, x]) != small_own, (kind, y, x, n[y, x])
        if small_own:
            assert n[y, x] <= 17
        ok = wave.copy()
        for yy, xx in pix:
            ok[yy, xx] = True
        assert ok[max(y - b, 0):y + b + 1, max(x - b, 0):x + b + 1].all(), (kind, y, x)
