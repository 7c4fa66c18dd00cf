"""The packed generic route's device-free surface (RPF_FLAG_GENERIC | RPF_FLAG_GENERIC_PACKED, rpf_query_route 4): the flag's
value, rpf_layout_kernels' truth table with it, and -- against the oracle, on the CPU -- what tests/test_generic_packed_gpu.py
takes for granted about its frames, so that a GPU failure is never a property of the input.  The frames are built here and
imported by the GPU file."""
import os
import re

import numpy as np
import pytest

import planted_nbhd as P
from test_gpu_parity import _independent_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, REF_ABORT = 1, 0

EDGE_LAYOUTS = [(1, 1, "f32"), (3, 7, "f32"), (5, 13, "f16"), (8, 27, "f32"), (2, 12, "f32"), (4, 18, "f16")]
EDGE_S, EDGE_BOX, EDGE_TARGETS = 8, 7, (8, 9, 16, 17, 32, 33, 64, 65, 24)
RESIDUE_LAYOUTS = [(3, 7, "f32"), (5, 13, "f16")]
RESIDUE_CASES = {"A": (9, 15), "B": (3, 35)}   # W, S: class N <= 16 (two full waves and a quarter) | class N <= 64
RESIDUE_BOX = 7
PACKED_CAPS = (8, 16, 32, 64)


def lay_ids(v):
    return "%d-%d-%s" % v if isinstance(v, tuple) else None


def stored_and_image(p32, lay):
    """the stored planes (an f16 layout is rounded once) and their exact fp32 image, which is what the oracle reads"""
    stored = p32.astype(np.float16) if lay[2] == "f16" else p32
    p32 = stored.astype(np.float32)
    stored.setflags(write=False)
    p32.setflags(write=False)
    return stored, p32


_edge = {}


def edge_frame(lay):
    """(stored planes, fp32 image, target pixels) of the class-edge frame: built once per layout, read-only"""
    if lay not in _edge:
        p32, pixels = P.plant(EDGE_S, EDGE_BOX, EDGE_TARGETS, n_random=lay[0], n_feat=lay[1], seed=0)
        _edge[lay] = stored_and_image(p32, lay) + (pixels,)
    return _edge[lay]


def edge_geometry():
    return EDGE_BOX * len(EDGE_TARGETS), EDGE_BOX, EDGE_S, EDGE_BOX   # W, H, S, box


_edge_want = {}


def edge_oracle(oracle, lay, policy, sigma_seed=0.002):
    """the oracle's pass of the edge frame: computed once per session, shared, never modified"""
    key = (lay, policy, sigma_seed)
    if key not in _edge_want:
        W, H, S, box = edge_geometry()
        _edge_want[key] = oracle.filter_pass(edge_frame(lay)[1], oracle.make_desc(W, H, S, box=box, policy=policy, sigma_seed=sigma_seed,
                                                                                  n_random=lay[0], n_feat=lay[1]))
    return _edge_want[key]


def class_counts(n):
    """pixels per class: N <= 8, <= 16, <= 32, <= 64, rest"""
    out, lo = [], 0
    for cap in PACKED_CAPS:
        out.append(int(((n > lo) & (n <= cap)).sum()))
        lo = cap
    return out + [int((n > lo).sum())]


_residue = {}


def residue_frame(oracle, lay, case):
    """W x 1 x S: every column of every pixel a permutation of k / (S - 1); pFilm.x = pixel + uniform; r0 and f0 carry the
    exactly independent pair of columns, the same pattern in every pixel; the last feature is shifted by 16 per pixel, so
    nobody accepts a neighbour and N = S.  Returns (stored planes, fp32 image, index of the independent pair)."""
    key = (lay, case)
    if key not in _residue:
        nr, nf, _ = lay
        W, S = RESIDUE_CASES[case]
        ndim = 5 + nr + nf
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
        _residue[key] = stored_and_image(planes, lay) + (indep,)
    return _residue[key]


_residue_want = {}


def residue_oracle(oracle, lay, case, policy):
    key = (lay, case, policy)
    if key not in _residue_want:
        W, S = RESIDUE_CASES[case]
        _residue_want[key] = oracle.filter_pass(residue_frame(oracle, lay, case)[1],
                                                oracle.make_desc(W, 1, S, box=RESIDUE_BOX, policy=policy, n_random=lay[0], n_feat=lay[1]))
    return _residue_want[key]


# ---- the flag and the truth table --------------------------------------------------------------------------------------------
def test_flag_matches_the_header_and_is_a_bit_of_its_own(hipmod):
    with open(os.path.join(ROOT, "include", "rpf_hip.h")) as f:
        m = re.search(r"\bRPF_FLAG_GENERIC_PACKED\s*=\s*(\d+)", f.read())
    assert m and hipmod.FLAG_GENERIC_PACKED == int(m.group(1)) == 16
    others = hipmod.FLAG_TIMING | hipmod.FLAG_FAST_WEIGHTS | hipmod.FLAG_NO_OVERLAP | hipmod.FLAG_GENERIC
    assert hipmod.FLAG_GENERIC_PACKED & others == 0


@pytest.mark.parametrize("lay,flags,want", [
    (dict(n_random=2, n_feat=12, plane_dtype=0), "GP", ("OK", 1)),
    (dict(n_random=4, n_feat=18, plane_dtype=1), "GP", ("OK", 1)),
    (dict(n_random=1, n_feat=1), "GP", ("OK", 1)),
    (dict(n_random=8, n_feat=27), "GP", ("OK", 1)),
    (dict(n_random=9, n_feat=27), "GP", ("E_UNSUPPORTED", None)),                # 41 dims
    (dict(n_random=2, n_feat=12, plane_dtype=0), "P", ("E_UNSUPPORTED", None)),  # the flag modifies the generic one
    (dict(n_random=3, n_feat=7), "P", ("E_UNSUPPORTED", None)),
    (dict(), "GPF", ("E_UNSUPPORTED", None)),                                    # the generic kernels are fp64 throughout
    (dict(), "PF", ("E_UNSUPPORTED", None)),
    (dict(), "GPT", ("OK", 1)),
])
def test_layout_kernels_truth_table_with_the_packed_flag(hipmod, lay, flags, want):
    bits = {"G": hipmod.FLAG_GENERIC, "P": hipmod.FLAG_GENERIC_PACKED, "F": hipmod.FLAG_FAST_WEIGHTS, "T": hipmod.FLAG_TIMING}
    st, generic = hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=sum(bits[c] for c in flags), **lay))
    assert (st, generic) == (getattr(hipmod, want[0]), want[1])


# ---- input conditions of the GPU tests, against the oracle -----------------------------------------------------------------
@pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
@pytest.mark.parametrize("lay", EDGE_LAYOUTS, ids=lay_ids)
def test_edge_frame_targets_classes_and_status(oracle, lay, policy):
    pixels = edge_frame(lay)[2]
    want = edge_oracle(oracle, lay, policy)
    n = want["nbhd_size"]
    assert [int(n[y, x]) for y, x in pixels] == list(EDGE_TARGETS)
    cc = class_counts(n)
    # the only wave of each of the first three classes runs partly empty.  (With the 27 features of the widest layout the
    # pushed candidates spread so thinly that three more bystanders of the windows end below 33 samples: the oracle counts
    # six pixels in the class N <= 32 there -- three whole waves; the five other layouts cover the half-empty wave.)
    assert cc[:3] == ([1, 2, 6] if lay == (8, 27, "f32") else [1, 2, 3]) and cc[3] >= 2 and cc[4] >= 200, cc
    assert want["status"] == 0 and np.isfinite(want["colour"]).all()


@pytest.mark.parametrize("lay", EDGE_LAYOUTS, ids=lay_ids)
def test_edge_frame_active_seed_moves_the_colours(oracle, lay):
    want = edge_oracle(oracle, lay, EPS, P.ACTIVE_SIGMA_SEED)
    cin = edge_frame(lay)[1][2:5].astype(np.float64)
    assert np.isfinite(want["colour"]).all()
    assert np.linalg.norm(want["colour"] - cin) / np.linalg.norm(cin) > 0.10


@pytest.mark.parametrize("lay", RESIDUE_LAYOUTS, ids=lay_ids)
def test_residue_frames(oracle, lay):
    _, _, indep = residue_frame(oracle, lay, "A")
    ref = residue_oracle(oracle, lay, "A", REF_ABORT)
    assert (ref["nbhd_size"] == 15).all() and ref["nbhd_size"].size == 9
    ri = ref["mi"][..., indep]
    assert (ri != 0).all() and (np.abs(ri) < 1e-14).all()              # real residue in all nine pixels
    assert (residue_oracle(oracle, lay, "A", EPS)["mi"][..., indep] == 0).all()
    _, _, indep = residue_frame(oracle, lay, "B")
    for policy in (EPS, REF_ABORT):
        ref = residue_oracle(oracle, lay, "B", policy)
        assert (ref["nbhd_size"] == 35).all() and ref["nbhd_size"].size == 3
        assert (ref["mi"][..., indep] == 0).all()                      # the redo rule fires; the reference's value is exactly 0
