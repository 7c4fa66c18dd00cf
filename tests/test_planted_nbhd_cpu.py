"""CPU tests of the planted frames (tests/planted_nbhd.py): the oracle alone, no GPU.  What tests/test_class_boundaries_gpu.py
takes for granted about its inputs is settled here: every target pixel has exactly the planted neighbourhood size, and the
frames of the unbinned route leave the last wavefront of every shared-wave packed class partly filled."""
import numpy as np
import pytest

import planted_nbhd as P

EPS, REF_ABORT = 1, 0


@pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
@pytest.mark.parametrize("fid", list(P.FRAMES))
def test_oracle_sees_the_planted_sizes(oracle, fid, policy):
    _, S, box, targets, _, _ = P.FRAMES[fid]
    _, _, pixels, planted = P.frame(fid)
    want = P.oracle_pass(oracle, fid, policy)
    n = want["nbhd_size"]
    assert n.shape == (box, box * len(targets)) and planted == targets
    assert [int(n[y, x]) for y, x in pixels] == list(targets)
    assert n.min() >= S and n.max() <= box * box * S
    if policy == EPS:
        assert want["status"] == 0 and np.isfinite(want["colour"]).all()


def test_every_class_edge_is_planted():
    """N = capacity and N = capacity + 1 of every size class are among the targets, on the compiled routes that reach them"""
    planted = set(n for v in P.FRAMES.values() for n in v[3])
    for cap in P.CAPACITIES:
        assert cap in planted and cap + 1 in planted, cap
    binned = set(n for v in P.FRAMES.values() if v[5] for n in v[3])
    for cap in P.CAPACITIES[1:]:          # (16 spp is the fewest samples the size-binned route starts at: N >= 16)
        assert cap in binned and cap + 1 in binned, cap
    for fid, (_, S, box, targets, _, is_binned) in P.FRAMES.items():
        assert (box * box * S > 512) == is_binned, fid   # the route route_pass picks by default


@pytest.mark.parametrize("fid", [f for f, v in P.FRAMES.items() if not v[5] and v[1] in (8, 2)])
def test_packed_classes_end_in_a_partly_filled_wave(oracle, fid):
    """the packed kernels N <= 8 / 16 / 32 filter 8 / 4 / 2 pixels per wavefront: a class whose pixel count is no multiple of
    that runs a last wave with pixels missing, the one that would read its list past the end"""
    n = P.oracle_pass(oracle, fid, EPS)["nbhd_size"]
    lo = 0
    for cap, per_wave in P.PACKED_PIXELS_PER_WAVE.items():
        count = int(((n > lo) & (n <= cap)).sum())
        assert count % per_wave != 0, (fid, cap, count)
        lo = cap


def test_plant_refuses_what_it_cannot_plant():
    with pytest.raises(ValueError):
        P.plant(1, 7, (1,))
    with pytest.raises(ValueError):
        P.plant(8, 7, (7,))            # below S: the own samples are always members
    with pytest.raises(ValueError):
        P.plant(8, 7, (393,))          # above box * box * S
    planes, pixels = P.plant(4, 3, (4, 36), n_random=3, n_feat=7, seed=5)
    assert planes.shape == (15, 3, 6, 4) and planes.dtype == np.float32 and pixels == [(1, 1), (1, 4)]
