"""CPU tests of the frame tests/test_listed_routes_gpu.py runs through the listed-member routes (7, 8 and 9: a count kernel lists
each pixel's members into a pool, the pixels are dealt into eight size classes and a rest class): the oracle and the numpy
restatement of the sampled gather alone, no GPU.  What the GPU file takes for granted about its input is settled here: the planted
neighbourhood sizes sit on either side of every class edge of the one-wave kernels, a full-box pass fills all eight classes and
the rest class, and the sampled pass fills all eight classes and leaves the rest class empty."""
import numpy as np
import pytest

import planted_nbhd as P
import sampled_ref as SR

EPS, REF_ABORT = 1, 0
S, BOX = 8, 11
TARGETS = (8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 448, 449, 832, 833, 968)
SAMPLING = (12345, 0, 824)                       # seed, row origin, draws: S + D = 832, the bound of a sampled pass
CAPS = (8, 16, 32, 64, 128, 256, 448, 832)       # the eight classes; beyond the last: the rest class

_cache = {}


def frame():
    """(planes [19, 11, 187, 8] fp32, target pixels): built once, read-only"""
    if "frame" not in _cache:
        planes, pixels = P.plant(S=S, box=BOX, targets=TARGETS, seed=0)
        planes.setflags(write=False)
        _cache["frame"] = (planes, pixels)
    return _cache["frame"]


def full_box(oracle, policy):
    """the oracle's full-box pass of the frame under a policy: computed once, shared, never modified"""
    if ("full", policy) not in _cache:
        planes, _ = frame()
        _, H, W, _ = planes.shape
        _cache["full", policy] = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=BOX, policy=policy,
                                                                             sigma_seed=P.ACTIVE_SIGMA_SEED))
    return _cache["full", policy]


def sampled(oracle):
    """the restatement's sampled pass of the frame (sizes, hashes, mean and sigma; no weights): computed once, shared"""
    if "sampled" not in _cache:
        _cache["sampled"] = SR.sampled_pass(oracle, frame()[0], SAMPLING, pass_id=0, box=BOX, weights=False)
    return _cache["sampled"]


def class_fill(nbhd):
    """pixels per class, the eight classes then the rest class"""
    n = np.asarray(nbhd).ravel()
    edges = (0,) + CAPS + (np.iinfo(np.int32).max,)
    return [int(((n > lo) & (n <= hi)).sum()) for lo, hi in zip(edges[:-1], edges[1:])]


def test_frame_shape():
    planes, pixels = frame()
    assert planes.shape == (19, 11, 187, 8) and planes.dtype == np.float32 and len(pixels) == len(TARGETS)
    assert planes.shape[1] * planes.shape[2] == 2057
    for cap in CAPS:                              # N = capacity and N = capacity + 1 of every class are planted
        assert cap in TARGETS and cap + 1 in TARGETS, cap
    assert max(TARGETS) == BOX * BOX * S


@pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
def test_full_box_pass_fills_every_class_and_the_rest(oracle, policy):
    _, pixels = frame()
    want = full_box(oracle, policy)
    n = want["nbhd_size"]
    assert [int(n[y, x]) for y, x in pixels] == list(TARGETS)
    fill = class_fill(n)
    print("LISTED full box, policy %d: class fill %s | rest %d" % (policy, fill[:-1], fill[-1]))
    assert sum(fill) == n.size == 2057 and n.min() >= S
    assert all(c > 0 for c in fill), fill        # eight class launches and the rest launch
    assert np.isfinite(want["colour"]).all()


def test_sampled_pass_fills_every_class_and_no_rest(oracle):
    n = sampled(oracle)["nbhd_size"]
    fill = class_fill(n)
    print("LISTED sampled: class fill %s | rest %d" % (fill[:-1], fill[-1]))
    assert sum(fill) == n.size == 2057 and n.min() >= S
    assert all(c > 0 for c in fill[:-1]), fill   # eight class launches
    assert fill[-1] == 0 and n.max() <= S + SAMPLING[2] == 832
    assert (n <= full_box(oracle, EPS)["nbhd_size"]).all()   # the sampled list is a subsequence of the full-box list
