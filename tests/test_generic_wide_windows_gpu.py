"""GPU tests of the generic class routes on windows of 65 to 1024 acceptance words (rpf_query_route 13, 5, 4 and 3; DESIGN.md
section 11g): the word prefix of generic::filter_quad_kernel's stage 1b past one step of 64 words, its popcount stride, its deal
of words to the waves and its clamp at 1024 words; the serial walk of generic::filter_wave_kernel and the rank select of
generic::filter_packed_kernel over hundreds of words; generic::nbhd_count_kernel on windows of 17 to 181 pixels across, and on
frame-clipped windows that write half or a quarter of their stride.  The frames, and what is taken for granted about them -- the
planted sizes, where the members lie among the words -- are built and asserted on the CPU by tests/test_generic_wide_windows_cpu.py.

Every frame is filtered and compared on its target row only (row_begin = ty, row_end = ty + 1, on the device and in the oracle).
"Route 3" is the same context and buffer with RPF_FLAG_GENERIC alone, "route 5" the same without RPF_FLAG_GENERIC_QUAD.  No
tolerance is new: check_pass's bars, _assert_ref_abort_parity, REL_L2_BAR, the direct form's per-sample bar of
tests/stage4_bars.py, or bit equality."""
import numpy as np
import pytest

import fast_weights_ref as R
import planted_nbhd as P
import stage4_bars as B
from test_generic_quad_gpu import desc_for, expected_launches
from test_generic_wave_gpu import bits_equal, desc_for as wave_desc_for, expected_launches as wave_expected_launches, run_debug
from test_generic_wide_windows_cpu import (ACTIVE_FRAMES, CASE_IDS, CASES, DEFAULT_LAY, DENSE, FRAMES, dense_frame, frame, frame_oracle,
                                           geometry, row_of, target_row)
from test_gpu_parity import REL_L2_BAR, STAGE_KEYS, _assert_ref_abort_parity, check_pass, rel_l2
from test_stage4_per_sample_cpu import at

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
DISCRETE_AND_STATS = ("nbhd_size", "member_hash", "bin_hash", "mean", "stddev")
ROUTE_QUAD = 13
OWN_CONTEXT = ("W181",)           # its mask buffer is 181 * 543 pixels * 1024 words * 8 B = 805 MB: not the session context's to keep


def row_desc(hipmod, fid, lay, route=ROUTE_QUAD, **kw):
    W, H, S, _ = geometry(fid)
    ty = target_row(fid)
    make = wave_desc_for if route == 4 else desc_for
    return make(hipmod, lay, W, H, S, route=route, row_begin=ty, row_end=ty + 1, **kw)


def row_run(c, hipmod, fid, lay, policy, sigma_seed=0.002, route=ROUTE_QUAD):
    """a pass over the target row of a frame on context c, cut to that row"""
    return row_of(run_debug(c, frame(fid, lay)[0], row_desc(hipmod, fid, lay, route, policy=policy, sigma_seed=sigma_seed), geometry(fid)[3]),
                  target_row(fid))


_got = {}


def frame_run(ctx, hipmod, fid, lay, policy, sigma_seed=0.002, route=ROUTE_QUAD):
    """row_run on the session context: run once per variant, shared, never modified"""
    key = (fid, lay, policy, sigma_seed, route)
    if key not in _got:
        _got[key] = row_run(ctx, hipmod, fid, lay, policy, sigma_seed, route)
    return _got[key]


def check_routes_13_5_3(run, hipmod, oracle, fid, lay, policy):
    """run(route) -> the row's outputs.  Route 13 against the oracle and route 3; route 5, and what route 13 shares with it"""
    want = frame_oracle(oracle, fid, lay, policy)
    n = want["nbhd_size"]
    xs = [x for _, x in frame(fid, lay)[2]]
    got, r5, r3 = run(ROUTE_QUAD), run(5), run(3)
    assert (got["route"], r5["route"], r3["route"]) == (ROUTE_QUAD, 5, 3)
    assert got["launches"] == expected_launches(hipmod, lay, n, policy)
    assert r5["launches"] == wave_expected_launches(n, policy) and r3["launches"] == 1
    for g in (got, r5, r3):
        assert [int(g["nbhd_size"][0, x]) for x in xs] == list(FRAMES[fid][3])
    if policy == EPS:
        for g in (got, r5, r3):
            assert g["status"] == hipmod.OK
            check_pass(g, want)
        bits_equal(got, r3, STAGE_KEYS)                          # the same integers, the same statements
        bits_equal(r5, r3, STAGE_KEYS)
        assert got["redo_pixels"] == r5["redo_pixels"] == 0
        # the pixels the four-wave classes do not take run the kernels of route 5: its colours too
        others = (n <= 832) | (n > 3136)
        assert others.any() and (~others).any()
        assert got["colour"][:, others].tobytes() == r5["colour"][:, others].tobytes()
        assert rel_l2(got["colour"], r5["colour"]) <= REL_L2_BAR
    else:
        for g in (got, r5):
            _assert_ref_abort_parity(g, want, hipmod, [])      # (no planted independent pair: its discrete keys, stats, weights, colours)
            check_pass(g, want)
            bits_equal(g, r3, DISCRETE_AND_STATS)


# ---- a. every frame and layout on routes 13, 5 and 3 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fid,lay", [c for c in CASES if c[0] not in OWN_CONTEXT], ids=[i for c, i in zip(CASES, CASE_IDS) if c[0] not in OWN_CONTEXT])
def test_wide_windows_vs_oracle_route3_and_route5(ctx, hipmod, oracle, fid, lay):
    check_routes_13_5_3(lambda route: frame_run(ctx, hipmod, fid, lay, EPS, route=route), hipmod, oracle, fid, lay, EPS)


def test_w31_ref_abort_parity_and_the_redo_launch(ctx, hipmod, oracle):
    check_routes_13_5_3(lambda route: frame_run(ctx, hipmod, "W31", DEFAULT_LAY, REF_ABORT, route=route), hipmod, oracle, "W31", DEFAULT_LAY,
                        REF_ABORT)
    n = frame_oracle(oracle, "W31", DEFAULT_LAY, REF_ABORT)["nbhd_size"]
    eps = frame_run(ctx, hipmod, "W31", DEFAULT_LAY, EPS)
    assert frame_run(ctx, hipmod, "W31", DEFAULT_LAY, REF_ABORT)["launches"] == eps["launches"] + 1 == expected_launches(hipmod, DEFAULT_LAY, n, EPS) + 1


def test_w31_on_route_4_rank_select_across_120_words(ctx, hipmod, oracle):
    """RPF_FLAG_GENERIC | RPF_FLAG_GENERIC_PACKED: the targets 8 and 64 are the packed kernel's, whose lanes select their rank
    among 120 words; 65 and everything above are the rest list's"""
    lay = DEFAULT_LAY
    want = frame_oracle(oracle, "W31", lay, EPS)
    n = want["nbhd_size"]
    got = frame_run(ctx, hipmod, "W31", lay, EPS, route=4)
    r3 = frame_run(ctx, hipmod, "W31", lay, EPS, route=3)
    assert got["route"] == 4 and got["status"] == hipmod.OK
    packed = [int(((n > lo) & (n <= hi)).sum()) for lo, hi in ((0, 8), (8, 16), (16, 32), (32, 64))]
    assert packed[0] > 0 and packed[3] > 0 and int((n > 64).sum()) > 0
    assert got["launches"] == sum(1 for k in packed if k) + 1
    xs = [x for _, x in frame("W31", lay)[2]]
    assert [int(got["nbhd_size"][0, x]) for x in xs] == list(FRAMES["W31"][3])
    assert FRAMES["W31"][3][:3] == (8, 64, 65)
    check_pass(got, want)
    bits_equal(got, r3, STAGE_KEYS)
    rest = n > 64                                                    # ... on the kernel of route 3: its colours too
    assert got["colour"][:, rest].tobytes() == r3["colour"][:, rest].tobytes()


# ---- b. weights of order one: every sample of the target row within the direct form's bar ---------------------------------------
@pytest.mark.parametrize("fid", ACTIVE_FRAMES)
def test_active_seed_stage4_per_sample(ctx, hipmod, oracle, fid):
    """tests/test_generic_quad_gpu.py::test_active_seed_stage4_per_sample with `pixels` the target row: the colours against the fp64
    restatement of tests/fast_weights_ref.py evaluated on the device's own stage outputs, every finite sample within
    stage4_bars.sample_bar("direct", ...) at the largest neighbourhood of the row"""
    lay, seed = DEFAULT_LAY, P.ACTIVE_SIGMA_SEED
    W, H, S, box = geometry(fid)
    ty = target_row(fid)
    want = frame_oracle(oracle, fid, lay, EPS, seed)
    stored, p32, _ = frame(fid, lay)
    full = run_debug(ctx, stored, row_desc(hipmod, fid, lay, policy=EPS, sigma_seed=seed), box)      # whole-frame arrays: stage4 indexes [y, x]
    got = row_of(full, ty)
    assert got["route"] == ROUTE_QUAD and got["status"] == hipmod.OK
    assert got["launches"] == expected_launches(hipmod, lay, want["nbhd_size"], EPS)
    check_pass(got, want)
    pixels = [(ty, x) for x in range(W)]
    ref = R.stage4(oracle, p32, full, box, seed, pixels, np.float64, EPS, lay[0], lay[1])
    mine = at(full["colour"], pixels)
    assert np.array_equal(np.isnan(mine), np.isnan(ref))
    cmax = B.cmax_of(p32[2:5].astype(np.float64))
    n = got["nbhd_size"][0]
    assert ((n > 832) & (n <= 3136)).any()
    bar = B.sample_bar("direct", lay[1], n.max(), seed, box)
    both = np.isfinite(mine) & np.isfinite(ref)
    dist = np.where(both, np.abs(mine - ref), 0.0).max(axis=(0, 2)) / cmax
    worst = int(np.argmax(dist))
    print("STAGE4 %s route 13: worst %.3e (bar %.3e) at pixel %s N %d; %d samples" % (fid, dist[worst], bar, pixels[worst], n[worst], int(both.sum())))
    assert both.all() and (dist <= bar).all(), (float(dist[worst]), bar)


# ---- c. 1024 words, the clamp: a context of its own ---------------------------------------------------------------------------------
def test_w181_at_the_clamp_of_1024_words(hipmod, oracle):
    fid, lay = "W181", DEFAULT_LAY
    with hipmod.Context(0) as own:
        check_routes_13_5_3(lambda route: row_run(own, hipmod, fid, lay, EPS, route=route), hipmod, oracle, fid, lay, EPS)


# ---- d. the words of a stride that the count pass does not write -------------------------------------------------------------------
def test_stale_words_behind_a_clipped_window_change_nothing(hipmod):
    """generic::nbhd_count_kernel writes ceil(ncand / 64) words of a pixel's stride.  One context filters C55 (which sizes the mask
    buffer: it only ever grows), then the dense frame, whose count pass fills that buffer's front with full words
    (tests/test_generic_wide_windows_cpu.py), then K55 and C55: 280 and 185 words of their targets' strides are then stale.  The
    same bits as on a fresh context, on routes 13 and 5"""
    lay = DEFAULT_LAY
    S, box, targets = DENSE
    fresh = {}
    for fid in ("K55", "C55"):
        with hipmod.Context(0) as c:
            for route in (ROUTE_QUAD, 5):
                fresh[fid, route] = row_run(c, hipmod, fid, lay, EPS, P.ACTIVE_SIGMA_SEED, route)
    with hipmod.Context(0) as c:
        row_run(c, hipmod, "C55", lay, EPS)
        dense = run_debug(c, dense_frame(), desc_for(hipmod, lay, box * len(targets), box, S, policy=EPS), box)
        b, Wd = box // 2, box * len(targets)
        span = lambda v, size: np.minimum(v + b, size - 1) - np.maximum(v - b, 0) + 1      # noqa: E731
        assert dense["route"] == ROUTE_QUAD                       # every candidate passes: N = S times the pixels of the clipped window
        assert np.array_equal(dense["nbhd_size"], S * span(np.arange(box), box)[:, None] * span(np.arange(Wd), Wd)[None, :])
        for fid in ("K55", "C55"):
            for route in (ROUTE_QUAD, 5):
                got = row_run(c, hipmod, fid, lay, EPS, P.ACTIVE_SIGMA_SEED, route)
                assert got["route"] == route == fresh[fid, route]["route"] and got["launches"] == fresh[fid, route]["launches"]
                bits_equal(got, fresh[fid, route], STAGE_KEYS + ("colour",))


# ---- e. the stride changes from pass to pass of one call ------------------------------------------------------------------------------
@pytest.mark.parametrize("boxes", [(55, 7), (7, 55)], ids=["55-7", "7-55"])
def test_two_passes_of_378_and_6_words(ctx, hipmod, oracle, boxes):
    """rpf_filter_ex on W55's planes: 378 words a pixel under box 55, 6 under box 7, in one mask buffer.  A call of two passes is
    refused on a row slab (RPF_E_BADARG: a sub-slab is filtered one pass per call), so the device filters the whole frame, and the
    comparison is on the target row: the oracle's first pass runs on the rows the second pass reads from there -- every other row
    of its colours is NaN, so a read of one would show -- its second on the target row alone"""
    fid, lay, seed = "W55", DEFAULT_LAY, P.ACTIVE_SIGMA_SEED
    W, H, S, _ = geometry(fid)
    ty = target_row(fid)
    stored, p32, _ = frame(fid, lay)
    with pytest.raises(hipmod.RpfError) as e:
        ctx.filter(stored, row_desc(hipmod, fid, lay, boxes=boxes, policy=EPS, sigma_seed=seed))
    assert e.value.status == hipmod.E_BADARG
    d = lambda bx: desc_for(hipmod, lay, W, H, S, boxes=bx, policy=EPS, sigma_seed=seed)      # noqa: E731
    two = ctx.filter(stored, d(boxes), want_colour64=True)
    assert two[2] == hipmod.OK and ctx.route() == ROUTE_QUAD
    one = ctx.filter(stored, d(boxes[:1]), want_colour64=True)
    again = ctx.filter(stored, d(boxes[1:]), colour64_in=one[3], want_colour64=True)
    assert one[2] == again[2] == hipmod.OK and ctx.route() == ROUTE_QUAD
    assert again[3].tobytes() == two[3].tobytes()
    assert np.array_equal(two[0], two[3].astype(np.float32))
    b2 = (boxes[1] - 1) // 2
    r0, r1 = max(ty - b2, 0), min(ty + b2, H - 1) + 1
    okw = dict(policy=EPS, sigma_seed=seed, n_random=lay[0], n_feat=lay[1])
    o1 = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=boxes[0], row_begin=r0, row_end=r1, **okw), debug=False)["colour"]
    assert rel_l2(one[3][:, r0:r1], o1[:, r0:r1]) <= REL_L2_BAR
    c1 = np.full_like(o1, np.nan)
    c1[:, r0:r1] = o1[:, r0:r1]
    o2 = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=boxes[1], row_begin=ty, row_end=ty + 1, **okw), colour_in=c1,
                            debug=False)["colour"][:, ty:ty + 1]
    assert np.isfinite(o2).all()
    assert rel_l2(two[3][:, ty:ty + 1], o2) <= REL_L2_BAR


# ---- f. run-to-run determinism -----------------------------------------------------------------------------------------------------------
def test_run_to_run_determinism_on_w55(ctx, hipmod):
    """the order of the class lists comes from atomics: no result may depend on it"""
    for policy in (EPS, REF_ABORT):
        a = row_run(ctx, hipmod, "W55", DEFAULT_LAY, policy, P.ACTIVE_SIGMA_SEED)
        b = row_run(ctx, hipmod, "W55", DEFAULT_LAY, policy, P.ACTIVE_SIGMA_SEED)
        assert a["route"] == ROUTE_QUAD and a["launches"] == b["launches"]
        bits_equal(a, b, STAGE_KEYS + ("colour",))
