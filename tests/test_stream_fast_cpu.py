"""RPF_FLAG_STREAM_FAST's device-free surface (Y below: fp32 pair weights on generic::filter_pixel_kernel and
generic::filter_wide_kernel, and on every kernel of a wide pass): the flag's value, rpf_layout_kernels' truth table with it, and
-- against the oracle, on the CPU -- the numpy yardstick of the fp32 arithmetic (tests/fast_weights_ref.py, dtype float32, form
"direct") on every frame tests/test_stream_fast_gpu.py holds the device to.  The frames and the yardstick rows are built here
and imported by the GPU file.

  * the fp64 form of the yardstick IS the oracle's stage 4: e64 <= 1e-12 relative L2;
  * the fp32 form at the active seed lies 5e-10 <= e32 <= 1e-4 / 16 from the oracle, so the GPU's bar g <= 16 * e32 + 1e-12 is
    neither vacuous nor wider than the contract.

Frames: the rows of tests/test_generic_fast_cpu.py (edge and E16 in six layouts, E32, G72); two planted frames in (3, 7, f32)
whose S lies below and across the sweep width of the fp32 stage 4, S3 = plant(3, 5, (3, 4, 60, 75)) and S21 = plant(21, 5, (21,
22, 100, 525)), and S21C, S21 with colour channel 1 constant over the frame (SD == 0 on a weighted column; membership does not
read colours); the wide fixtures main, l1_1, l4_18h, l17_18 at their targets plus every 8th pixel of the row, and the
wide-classes fixture at its fixture pixels.

S21 has a box of 5, not 3: a box of 3 has sigma_p = 3 // 4 = 0 (integer division, rpf.cpp:531), the exponent of a sample's own
pair is 0 / 0 and every colour of the frame is NaN under REF_ABORT and the input under EPS -- the reason G72 stands in for E72
in tests/test_generic_fast_cpu.py.  S = 21 leaves a remainder of 5 at sweeps of 8 and of 16 at either box."""
import os
import re

import numpy as np
import pytest

import fast_weights_ref as R
import planted_nbhd as P
import wide_classes_frames as WC
import wide_frames as WF
from test_generic_fast_cpu import ROWS as FAST_ROWS
from test_generic_fast_cpu import TABLE_LAYOUTS, any_frame, any_geometry, any_oracle, row_ids, yardstick_distance, yardstick_row
from test_generic_wave_cpu import stored_and_image
from test_wide_nbhd_gpu import want_row as wide_want_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EPS, REF_ABORT = 1, 0
ACTIVE = P.ACTIVE_SIGMA_SEED
POLICIES = pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
E64_BAR, E32_MIN, E32_MAX = 1e-12, 5e-10, 1e-4 / 16

# ---- the planted frames of the sweep width -------------------------------------------------------------------------------------
SWEEP_LAY = (3, 7, "f32")
# id: S, box, targets
SWEEP_FRAMES = {"S3": (3, 5, (3, 4, 60, 75)), "S21": (21, 5, (21, 22, 100, 525)), "S21C": (21, 5, (21, 22, 100, 525))}
_sweep, _sweep_want = {}, {}


def sweep_geometry(fid):
    S, box, targets = SWEEP_FRAMES[fid]
    return box * len(targets), box, S, box       # W, H, S, box


def sweep_frame(fid):
    """(stored planes, fp32 image, target pixels): built once, read-only"""
    if fid not in _sweep:
        S, box, targets = SWEEP_FRAMES[fid]
        p32, pixels = P.plant(S, box, targets, n_random=SWEEP_LAY[0], n_feat=SWEEP_LAY[1], seed=0)
        if fid == "S21C":
            p32[3] = np.float32(0.25)            # colour channel 1: SD == 0 in every neighbourhood
        _sweep[fid] = stored_and_image(p32, SWEEP_LAY) + (pixels,)
    return _sweep[fid]


def sweep_oracle(oracle, fid, policy, seed=ACTIVE):
    if (fid, policy, seed) not in _sweep_want:
        W, H, S, box = sweep_geometry(fid)
        _sweep_want[fid, policy, seed] = oracle.filter_pass(sweep_frame(fid)[1], oracle.make_desc(
            W, H, S, box=box, policy=policy, sigma_seed=seed, n_random=SWEEP_LAY[0], n_feat=SWEEP_LAY[1]))
    return _sweep_want[fid, policy, seed]


_sweep_rows = {}


def sweep_yardstick(oracle, fid, policy, seed, dtype):
    """stage 4 of tests/fast_weights_ref.py on the target row of a sweep frame: colours [3, W, S]; once per session"""
    key = (fid, policy, seed, np.dtype(dtype).name)
    if key not in _sweep_rows:
        W, H, S, box = sweep_geometry(fid)
        b = (box - 1) // 2
        r = R.stage4(oracle, sweep_frame(fid)[1], sweep_oracle(oracle, fid, policy, seed), box, seed, [(b, x) for x in range(W)], dtype,
                     policy, SWEEP_LAY[0], SWEEP_LAY[1])
        r.setflags(write=False)
        _sweep_rows[key] = r
    return _sweep_rows[key]


def sweep_distance(oracle, fid, policy, seed, dtype):
    b = (sweep_geometry(fid)[3] - 1) // 2
    ref = sweep_oracle(oracle, fid, policy, seed)["colour"][:, b]
    fin = np.isfinite(ref)
    return R.rel_l2(sweep_yardstick(oracle, fid, policy, seed, dtype)[fin], ref[fin])


# ---- the wide fixtures: frame-shaped stage outputs of the row of the targets, the checked pixels, the yardstick on them -----------
WIDE_FIDS = ["main", "l1_1", "l4_18h", "l17_18"]
_wide = {}


def _frame_shaped(row, H, ROW):
    full = {}
    for k, v in row.items():
        col = k == "colour"
        a = np.zeros(((3, H) if col else (H,)) + v.shape[2 if col else 1:], v.dtype)
        if col:
            a[:, ROW] = v[:, 0]
        else:
            a[ROW] = v[0]
        full[k] = a
    return full


def wide_case(fid, policy):
    """(p32 planes, layout, frame-shaped oracle outputs of the fixture, checked columns of the row) of a wide fixture: fid one of
    WIDE_FIDS (targets plus every 8th pixel of the row) or "classes" (tests/golden/wide_classes.npz: its fixture pixels, the only
    ones it holds stage outputs for).  Once per session, read-only."""
    if (fid, policy) not in _wide:
        if fid == "classes":
            g = np.load(os.path.join(GOLD, "wide_classes.npz"))
            p = "eps" if policy == EPS else "ref_abort"
            pix = g["pix"]
            assert np.array_equal(pix, WC.fixture_pixels())
            row = {}
            for k, src in (("mean", "mean"), ("stddev", "stddev"), ("alpha", "alpha_" + p), ("beta", "beta_" + p), ("wrc", "wrc_" + p)):
                a = np.zeros((1, WC.W) + g[src].shape[1:], g[src].dtype)
                a[0, pix] = g[src]
                row[k] = a
            row["nbhd_size"] = g["nbhd_size"][None]
            c = np.full((3, 1, WC.W, WC.S), np.nan)
            c[:, 0, pix] = g["colour_" + p]
            row["colour"] = c
            _wide[fid, policy] = (WC.frame()[0], (2, 12, "f32"), _frame_shaped(row, WC.H, WC.ROW), [int(x) for x in pix])
        else:
            _, p32, pixels, _ = WF.frame(fid)
            W, H = WF.geometry(fid)
            xs = sorted(set(range(0, W, 8)) | {x for _, x in pixels})
            _wide[fid, policy] = (p32, WF.FRAMES[fid][0], _frame_shaped(wide_want_row(fid, policy), H, WF.ROW), xs)
    return _wide[fid, policy]


_wide_rows = {}


def wide_yardstick(oracle, fid, policy, dtype):
    """colours [3, checked pixels, S] of the yardstick on a wide fixture's checked pixels (about 0.15 s per pixel at N = 68229)"""
    key = (fid, policy, np.dtype(dtype).name)
    if key not in _wide_rows:
        p32, lay, want, xs = wide_case(fid, policy)
        fin = [x for x in xs if np.isfinite(want["colour"][:, WF.ROW, x]).all()]      # (a REF_ABORT NaN pixel has no yardstick)
        r = np.full((3, len(xs), WF.S), np.nan)
        if fin:
            r[:, [xs.index(x) for x in fin]] = R.stage4(oracle, p32, want, WF.BOX, WF.SIGMA_SEED, [(WF.ROW, x) for x in fin], dtype, policy,
                                                        lay[0], lay[1])
        r.setflags(write=False)
        _wide_rows[key] = r
    return _wide_rows[key]


def wide_reference(fid, policy):
    """the oracle's colours [3, checked pixels, S] of the fixture"""
    _, _, want, xs = wide_case(fid, policy)
    return want["colour"][:, WF.ROW, xs]


def per_pixel(a, b):
    """rel-L2 per checked pixel of [3, pixels, S] arrays (NaN where b is not finite)"""
    out = np.full(a.shape[1], np.nan)
    for i in range(a.shape[1]):
        if np.isfinite(b[:, i]).all():
            out[i] = R.rel_l2(a[:, i], b[:, i])
    return out


# ---- 1. the flag -----------------------------------------------------------------------------------------------------------------
def flag_bits(hipmod, letters):
    bits = {"G": hipmod.FLAG_GENERIC, "P": hipmod.FLAG_GENERIC_PACKED, "W": hipmod.FLAG_GENERIC_WAVE, "F": hipmod.FLAG_FAST_WEIGHTS,
            "T": hipmod.FLAG_TIMING, "N": hipmod.FLAG_WIDE_NBHD, "C": hipmod.FLAG_WIDE_CLASSES, "X": hipmod.FLAG_GENERIC_FAST,
            "Y": hipmod.FLAG_STREAM_FAST}
    return sum(bits[c] for c in letters)


def test_flag_matches_the_header_and_is_a_bit_of_its_own(hipmod):
    with open(os.path.join(ROOT, "include", "rpf_hip.h")) as f:
        m = re.search(r"\bRPF_FLAG_STREAM_FAST\s*=\s*(\d+)", f.read())
    assert m and hipmod.FLAG_STREAM_FAST == int(m.group(1)) == 512
    assert hipmod.FLAG_STREAM_FAST & (hipmod.FLAG_NO_OVERLAP | flag_bits(hipmod, "GPWFTNCX")) == 0


# ---- 2. the truth table ------------------------------------------------------------------------------------------------------------
ACCEPTED = ["GY", "GPY", "GPWY", "GPWXY", "NY", "NCY", "GNCY", "GPWNCY"]
REFUSED = ["Y", "PY", "FY", "GFY", "NFY", "GPXNY", "CY"]
# rows of the older tables, without Y: (flags, accepted on a compiled layout, on (3, 7))
OLDER = [("", True, False), ("G", True, True), ("GP", True, True), ("GPW", True, True), ("GPWX", True, True), ("N", True, False),
         ("NC", True, False), ("GNC", True, True), ("F", None, False), ("GF", False, False), ("NF", False, False), ("GPXN", False, False),
         ("C", False, False), ("X", False, False), ("GX", False, False), ("P", False, False), ("GW", False, False)]
LAY_IDS = ["2-12-f32", "4-18-f16", "3-7-f32"]


@pytest.mark.parametrize("lay", TABLE_LAYOUTS, ids=LAY_IDS)
@pytest.mark.parametrize("flags", ACCEPTED)
def test_truth_table_accepted_with_the_answer_of_the_same_flags_without_y(hipmod, lay, flags):
    base = hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=flag_bits(hipmod, flags.replace("Y", "")), **lay))
    got = hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=flag_bits(hipmod, flags), **lay))
    compiled = lay.get("n_feat") != 7
    if "G" in flags or compiled:
        assert base == (hipmod.OK, 1 if "G" in flags else 0)
    else:       # (3, 7) needs G as before
        assert base == (hipmod.E_UNSUPPORTED, None)
    assert got == base


@pytest.mark.parametrize("lay", TABLE_LAYOUTS, ids=LAY_IDS)
@pytest.mark.parametrize("flags", REFUSED)
def test_truth_table_refused(hipmod, lay, flags):
    """fails on a library without the flag: bit 512 alone is ignored there and `Y` returns RPF_OK"""
    assert hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=flag_bits(hipmod, flags), **lay)) == (hipmod.E_UNSUPPORTED, None)


@pytest.mark.parametrize("lay", TABLE_LAYOUTS, ids=LAY_IDS)
def test_truth_table_without_y_nothing_moved(hipmod, lay):
    compiled, ref19 = lay.get("n_feat") != 7, lay.get("n_feat") == 12
    for flags, on_compiled, on_37 in OLDER:
        ok = on_37 if not compiled else (ref19 if on_compiled is None else on_compiled)      # F alone: the 19-dim layout only
        want = (hipmod.OK, 1 if "G" in flags else 0) if ok else (hipmod.E_UNSUPPORTED, None)
        assert hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=flag_bits(hipmod, flags), **lay)) == want, flags


# ---- 3. the yardstick's own distances ------------------------------------------------------------------------------------------------
@POLICIES
@pytest.mark.parametrize("row", FAST_ROWS, ids=row_ids)
def test_yardstick_distances_route3_rows(oracle, row, policy):
    fid, lay = row
    e64 = yardstick_distance(oracle, fid, lay, policy, ACTIVE, np.float64)
    e32 = yardstick_distance(oracle, fid, lay, policy, ACTIVE, np.float32)
    print("%s %s policy %d: e64 = %.3e  e32 = %.3e" % (fid, lay, policy, e64, e32))
    assert e64 <= E64_BAR and E32_MIN <= e32 <= E32_MAX, (e64, e32)


@POLICIES
@pytest.mark.parametrize("fid", sorted(SWEEP_FRAMES))
def test_yardstick_distances_sweep_frames(oracle, fid, policy):
    W, H, S, box = sweep_geometry(fid)
    want = sweep_oracle(oracle, fid, policy)
    assert [int(want["nbhd_size"][y, x]) for y, x in sweep_frame(fid)[2]] == list(SWEEP_FRAMES[fid][2])
    assert S % 8 != 0 and S % 16 != 0 and box // 4 == 1
    if fid == "S21C":       # membership does not depend on colours
        assert np.array_equal(want["nbhd_size"], sweep_oracle(oracle, "S21", policy)["nbhd_size"])
        assert (want["stddev"][..., 3] == 0).all()
        if policy == REF_ABORT:     # a constant channel has MI 0 with everything: alpha is 0 / 0 and the reference exits
            assert want["status"] == 1 and want["nonfinite_pixels"] > 0
            return                  # (the GPU test holds the device under Y to the status and NaN pattern of its base run)
    b = (box - 1) // 2
    if fid == "S3" and policy == REF_ABORT:     # at 3 spp the oracle leaves pixels NaN under REF_ABORT (the reference exits there)
        assert want["status"] == 1 and np.isfinite(want["colour"][:, b]).any()     # ... the distances are over the finite entries
    else:
        assert want["status"] == 0 and np.isfinite(want["colour"]).all()
    e64 = sweep_distance(oracle, fid, policy, ACTIVE, np.float64)
    e32 = sweep_distance(oracle, fid, policy, ACTIVE, np.float32)
    print("%s policy %d: e64 = %.3e  e32 = %.3e" % (fid, policy, e64, e32))
    assert e64 <= E64_BAR and E32_MIN <= e32 <= E32_MAX, (e64, e32)


@POLICIES
@pytest.mark.parametrize("fid", WIDE_FIDS + ["classes"])
def test_yardstick_distances_wide_fixtures(oracle, fid, policy):
    ref = wide_reference(fid, policy)
    fin = np.isfinite(ref).all(axis=(0, 2))
    y64, y32 = wide_yardstick(oracle, fid, policy, np.float64), wide_yardstick(oracle, fid, policy, np.float32)
    e64, e32 = R.rel_l2(y64[:, fin], ref[:, fin]), R.rel_l2(y32[:, fin], ref[:, fin])
    px = per_pixel(y32, ref)[fin]
    print("wide %s policy %d: %d pixels (%d finite), e64 = %.3e  e32 = %.3e  per pixel %.2e ... %.2e" % (
        fid, policy, len(fin), int(fin.sum()), e64, e32, px.min(), px.max()))
    assert fin.any() and (fid == "classes" or fin.all())
    assert e64 <= E64_BAR and E32_MIN <= e32 <= E32_MAX, (e64, e32)
    assert (px >= E32_MIN).all() and (px <= E32_MAX).all()
