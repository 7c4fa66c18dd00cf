"""RPF_FLAG_GENERIC_FAST's device-free surface (fp32 pair weights on the packed and one-wave layout-generic kernels, routes 4 and
5): the flag's value, rpf_layout_kernels' truth table with it, the frame G72, and -- against the oracle, on the CPU -- the
numpy yardstick of the fp32 arithmetic (tests/fast_weights_ref.py, layout-generic) on every frame tests/test_generic_fast_gpu.py
holds the device to: the class-edge frame at 8 spp (tests/test_generic_packed_cpu.py) and E16 (tests/test_generic_wave_cpu.py)
in six layouts, E32 and G72 in (3, 7, f32), on the target row, under both policies and both sigma seeds.

  * the fp64 form of the yardstick IS the oracle's stage 4: e64 <= 1e-12 relative L2 (measured: <= 1.4e-15);
  * the fp32 form lies e32 <= 1e-6 from the oracle; at the active seed 0 < e32 and the pass moves the row's colours by more
    than 5 %, so the GPU's bar g <= 16 * e32 + 1e-12 is neither vacuous nor loose (16 * e32 stays below 0.2 % of the 1e-4
    contract).

Measured (e32 at the active seed | colours moved | e32 at the reference's seed; the two policies agree to 0.1e-9):

  edge frame, 8 spp   six layouts    8.1e-9 ... 1.24e-8   10 ... 47 %   0
  E16                 six layouts    6.6e-9 ... 1.00e-8   13 ... 47 %   0; (1, 1, f32): 9.8e-14
  E32                 (3, 7, f32)    8.2e-9               37 %          0
  G72                 (3, 7, f32)    5.9e-9               39 %          1.5e-12

G72 exists because E72 has a box of 3, hence sigma_p = 3 / 4 = 0 (integer division, rpf.cpp:531): the yardstick divides by
zero there and the frame is all-NaN under REF_ABORT.  The frames and the yardstick rows are built here and imported by the GPU
file."""
import os
import re

import numpy as np
import pytest

import fast_weights_ref as R
import planted_nbhd as P
from test_generic_packed_cpu import EDGE_LAYOUTS, edge_frame, edge_geometry, edge_oracle
from test_generic_wave_cpu import FRAMES, LAYOUTS, class_counts, frame, frame_oracle, geometry, lay_ids, stored_and_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, REF_ABORT = 1, 0
SEEDS = pytest.mark.parametrize("seed", [0.002, P.ACTIVE_SIGMA_SEED], ids=["ref_seed", "active_seed"])
POLICIES = pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])

G72_LAY, G72_S, G72_BOX = (3, 7, "f32"), 72, 5
G72_TARGETS = (72, 128, 129, 448, 449, 832, 833, 1000)
G72_CLASSES = [0, 0, 0, 0, 2, 1, 1, 93, 103]
assert EDGE_LAYOUTS == LAYOUTS

# the yardstick's rows: (frame, layout) for every case of the table above
ROWS = ([("edge", lay) for lay in LAYOUTS] + [("E16", lay) for lay in LAYOUTS] + [("E32", (3, 7, "f32")), ("G72", G72_LAY)])


def row_ids(v):
    return "%s-%d-%d-%s" % ((v[0],) + v[1]) if isinstance(v, tuple) and isinstance(v[0], str) else None


_g72 = {}


def g72_frame():
    """(stored planes, fp32 image, target pixels) of G72: built once, read-only"""
    if not _g72:
        p32, pixels = P.plant(G72_S, G72_BOX, G72_TARGETS, n_random=G72_LAY[0], n_feat=G72_LAY[1], seed=0)
        _g72[0] = stored_and_image(p32, G72_LAY) + (pixels,)
    return _g72[0]


def any_geometry(fid):
    """W, H, S, box of "edge", "G72" or a frame of tests/test_generic_wave_cpu.py"""
    if fid == "edge":
        return edge_geometry()
    if fid == "G72":
        return G72_BOX * len(G72_TARGETS), G72_BOX, G72_S, G72_BOX
    return geometry(fid)


def any_frame(fid, lay):
    if fid == "edge":
        return edge_frame(lay)
    if fid == "G72":
        assert lay == G72_LAY
        return g72_frame()
    return frame(fid, lay)


_g72_want = {}


def any_oracle(oracle, fid, lay, policy, seed=0.002):
    """the oracle's pass of a frame: computed once per session, shared, never modified"""
    if fid == "edge":
        return edge_oracle(oracle, lay, policy, seed)
    if fid == "G72":
        if (policy, seed) not in _g72_want:
            W, H, S, box = any_geometry(fid)
            _g72_want[policy, seed] = oracle.filter_pass(g72_frame()[1], oracle.make_desc(W, H, S, box=box, policy=policy, sigma_seed=seed,
                                                                                         n_random=lay[0], n_feat=lay[1]))
        return _g72_want[policy, seed]
    return frame_oracle(oracle, fid, lay, policy, seed)


_rows = {}


def yardstick_row(oracle, fid, lay, policy, seed, dtype):
    """stage 4 of tests/fast_weights_ref.py on every pixel of the target row y = b: colours [3, W, S]; computed once per
    session, shared, never modified"""
    key = (fid, lay, policy, seed, np.dtype(dtype).name)
    if key not in _rows:
        W, H, S, box = any_geometry(fid)
        b = (box - 1) // 2
        want = any_oracle(oracle, fid, lay, policy, seed)
        r = R.stage4(oracle, any_frame(fid, lay)[1], want, box, seed, [(b, x) for x in range(W)], dtype, policy, lay[0], lay[1])
        r.setflags(write=False)
        _rows[key] = r
    return _rows[key]


def yardstick_distance(oracle, fid, lay, policy, seed, dtype):
    """rel-L2 of yardstick_row against the oracle's colours of that row, over the entries the oracle leaves finite"""
    b = (any_geometry(fid)[3] - 1) // 2
    ref = any_oracle(oracle, fid, lay, policy, seed)["colour"][:, b]
    fin = np.isfinite(ref)
    return R.rel_l2(yardstick_row(oracle, fid, lay, policy, seed, dtype)[fin], ref[fin])


# ---- 1. the flag ---------------------------------------------------------------------------------------------------------------
def test_flag_matches_the_header_and_is_a_bit_of_its_own(hipmod):
    with open(os.path.join(ROOT, "include", "rpf_hip.h")) as f:
        m = re.search(r"\bRPF_FLAG_GENERIC_FAST\s*=\s*(\d+)", f.read())
    assert m and hipmod.FLAG_GENERIC_FAST == int(m.group(1)) == 256
    others = (hipmod.FLAG_TIMING | hipmod.FLAG_FAST_WEIGHTS | hipmod.FLAG_NO_OVERLAP | hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED
              | hipmod.FLAG_GENERIC_WAVE | hipmod.FLAG_WIDE_NBHD | hipmod.FLAG_WIDE_CLASSES)
    assert hipmod.FLAG_GENERIC_FAST & others == 0


# ---- 2. the truth table ----------------------------------------------------------------------------------------------------------
TABLE_LAYOUTS = [dict(n_random=2, n_feat=12, plane_dtype=0), dict(n_random=4, n_feat=18, plane_dtype=1), dict(n_random=3, n_feat=7)]
ACCEPTED = ["GPX", "GPWX", "GPXT", "GPWXT"]
REFUSED = ["X", "GX", "PX", "GWX", "GPXF", "GPXN"]      # N: RPF_FLAG_WIDE_NBHD


def flag_bits(hipmod, letters):
    bits = {"G": hipmod.FLAG_GENERIC, "P": hipmod.FLAG_GENERIC_PACKED, "W": hipmod.FLAG_GENERIC_WAVE, "F": hipmod.FLAG_FAST_WEIGHTS,
            "T": hipmod.FLAG_TIMING, "N": hipmod.FLAG_WIDE_NBHD, "X": hipmod.FLAG_GENERIC_FAST}
    return sum(bits[c] for c in letters)


@pytest.mark.parametrize("lay", TABLE_LAYOUTS, ids=["2-12-f32", "4-18-f16", "3-7-f32"])
@pytest.mark.parametrize("flags,want", [(f, ("OK", 1)) for f in ACCEPTED] + [(f, ("E_UNSUPPORTED", None)) for f in REFUSED])
def test_layout_kernels_truth_table_with_the_fast_flag(hipmod, lay, flags, want):
    st, generic = hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=flag_bits(hipmod, flags), **lay))
    assert (st, generic) == (getattr(hipmod, want[0]), want[1])


# ---- 3. the yardstick against the oracle -------------------------------------------------------------------------------------------
@SEEDS
@POLICIES
@pytest.mark.parametrize("row", ROWS, ids=row_ids)
def test_yardstick_distances(oracle, row, policy, seed):
    fid, lay = row
    e64 = yardstick_distance(oracle, fid, lay, policy, seed, np.float64)
    e32 = yardstick_distance(oracle, fid, lay, policy, seed, np.float32)
    b = (any_geometry(fid)[3] - 1) // 2
    ref = any_oracle(oracle, fid, lay, policy, seed)["colour"][:, b]
    cin = any_frame(fid, lay)[1][2:5, b].astype(np.float64)
    fin = np.isfinite(ref)
    moved = R.rel_l2(ref[fin], cin[fin])
    print("%s %s policy %d seed %g: e64 = %.3e  e32 = %.3e  moved %.1f %%" % (fid, lay, policy, seed, e64, e32, 100 * moved))
    assert fin.all()
    assert e64 <= 1e-12, e64
    assert e32 <= 1e-6, e32
    if seed == P.ACTIVE_SIGMA_SEED:
        assert e32 > 0          # the weights are of order one: fp32 arithmetic shows
        assert moved > 0.05     # ... on colours that the pass moves


# ---- 4. G72 ---------------------------------------------------------------------------------------------------------------------------
@POLICIES
def test_g72_targets_classes_and_status(oracle, policy):
    want = any_oracle(oracle, "G72", G72_LAY, policy)
    n = want["nbhd_size"]
    assert n.shape == (5, 40)
    assert [int(n[y, x]) for y, x in g72_frame()[2]] == list(G72_TARGETS)
    assert class_counts(n) == G72_CLASSES
    assert want["status"] == 0 and np.isfinite(want["colour"]).all()
    assert np.isfinite(any_oracle(oracle, "G72", G72_LAY, policy, P.ACTIVE_SIGMA_SEED)["colour"]).all()
    assert FRAMES["E72"][2] == 3 and G72_BOX // 4 == 1      # the frame it stands in for has sigma_p = 0; this one has sigma_p = 1
