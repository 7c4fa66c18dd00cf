"""GPU tests of RPF_FLAG_STREAM_FAST (Y below): the fp32 pair-weight instantiations generic::filter_pixel_kernel<T, true> (route
3, the rest lists of routes 4 / 5) and generic::filter_wide_kernel<T, true> (route 6, the rest list of route 7), and on route 7
the FAST instantiations of the packed and one-wave class kernels reading listed members.  G = RPF_FLAG_GENERIC, P = ..._PACKED,
W = ..._WAVE, X = RPF_FLAG_GENERIC_FAST, N = RPF_FLAG_WIDE_NBHD, C = RPF_FLAG_WIDE_CLASSES.  Every frame's input conditions and the
yardstick's own distance from the oracle are asserted on the CPU by tests/test_stream_fast_cpu.py; "base" is the same context,
buffer and flags without Y.

Bars (those of tests/test_generic_fast_gpu.py; none fitted to what the kernels give):
  contract    colours under Y against the oracle <= REL_L2_BAR (1e-4), wherever the oracle is finite.
  regression  g <= 16 * e32 + 1e-12: g the device under Y against the oracle, e32 the numpy fp32 restatement
              (tests/fast_weights_ref.py, float32, "direct") against the oracle over the same samples; on the wide rows per
              checked pixel as well as over the set.
  discrete    STAGE_KEYS, route, launches and redo_pixels bit-equal to the base run.
  fp64 parts  the redo list, every pass on the fused routes, and on routes 4 / 5 the classes: colours bit-equal to the base.
  really fp32 at the active seed the colours under Y differ from the base by more than 1e-10 rel-L2 over the pixels an fp32
              kernel filtered.

Measured on the MI355X at the active seed (DESIGN.md section 11f has the table): g / e32 = 0.84 ... 1.05 over the cases of route 3
and the rest lists (g = 4.7e-9 ... 1.29e-8), 0.97 ... 1.13 over the checked pixels of a wide row (per pixel 0.71 ... 1.39), the
whole-frame distance from the oracle at most 1.28e-8; at the reference's seed g = 0 wherever e32 = 0."""
import numpy as np
import pytest

import pbrt_film_ref as FR
import planted_nbhd as P
import test_wide_classes_gpu as TC
import test_wide_nbhd_gpu as TW
import wide_classes_frames as WC
import wide_frames as WF
from test_film_gpu import film_device
from test_generic_fast_cpu import G72_LAY, any_frame, any_geometry, any_oracle, yardstick_distance, yardstick_row
from test_generic_layout_gpu import buffers
from test_generic_packed_cpu import RESIDUE_BOX as PK_RESIDUE_BOX
from test_generic_packed_cpu import RESIDUE_CASES, RESIDUE_LAYOUTS
from test_generic_packed_cpu import residue_frame as pk_residue_frame
from test_generic_wave_cpu import (FRAMES, INF_SHAPE, LAYOUTS, RESIDUE_BOX, RESIDUE_LAY, RESIDUE_S, RESIDUE_W, inf_frame, lay_ids,
                                   residue_frame)
from test_generic_wave_gpu import entry_frame
from test_gpu_parity import INF_INJECTIONS, REL_L2_BAR, STAGE_KEYS, check_pass, rel_l2
from test_stream_fast_cpu import (REFUSED, SWEEP_FRAMES, SWEEP_LAY, WIDE_FIDS, flag_bits, per_pixel, sweep_distance, sweep_frame,
                                  sweep_geometry, sweep_oracle, sweep_yardstick, wide_case, wide_reference, wide_yardstick)

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
ACTIVE = P.ACTIVE_SIGMA_SEED
SEEDS = pytest.mark.parametrize("seed", [0.002, ACTIVE], ids=["ref_seed", "active_seed"])
POLICIES = pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
REGRESSION_FACTOR = 16


def desc_for(hipmod, lay, W, H, S, letters, **kw):
    nr, nf, dt = lay
    return hipmod.make_desc(W, H, S, n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16 if dt == "f16" else hipmod.PLANES_F32,
                            flags=flag_bits(hipmod, letters), **kw)


def run_debug(c, planes, desc, box):
    got = c.filter_pass_debug(planes, desc, box=box, allow_nonfinite=True)
    cnt = c.counters()
    got.update(route=c.route(), launches=cnt.filter_kernel_launches, redo_pixels=cnt.redo_pixels)
    return got


def bits_equal(a, b, keys):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


def discrete_equal(got, ref, route):
    assert got["route"] == ref["route"] == route
    assert got["launches"] == ref["launches"] and got["redo_pixels"] == ref["redo_pixels"]
    assert got["sum_nbhd"] == ref["sum_nbhd"] and got["max_nbhd"] == ref["max_nbhd"]
    bits_equal(got, ref, STAGE_KEYS)


_got = {}


def frame_run(ctx, hipmod, fid, lay, policy, seed, letters):
    """a pass over a frame of tests/test_generic_fast_cpu.py or a sweep frame: run once per variant, shared, never modified"""
    key = (fid, lay, policy, seed, letters)
    if key not in _got:
        if fid in SWEEP_FRAMES:
            (W, H, S, box), planes = sweep_geometry(fid), sweep_frame(fid)[0]
        else:
            (W, H, S, box), planes = any_geometry(fid), any_frame(fid, lay)[0]
        _got[key] = run_debug(ctx, planes, desc_for(hipmod, lay, W, H, S, letters, policy=policy, sigma_seed=seed), box)
    return _got[key]


def five_bars_route3(ctx, hipmod, oracle, fid, lay, policy, seed):
    """G | Y against G and the yardstick: every pixel of the pass is fp32"""
    sweep = fid in SWEEP_FRAMES
    W, H, S, box = sweep_geometry(fid) if sweep else any_geometry(fid)
    b = (box - 1) // 2
    want = sweep_oracle(oracle, fid, policy, seed) if sweep else any_oracle(oracle, fid, lay, policy, seed)
    ref = frame_run(ctx, hipmod, fid, lay, policy, seed, "G")
    got = frame_run(ctx, hipmod, fid, lay, policy, seed, "GY")
    discrete_equal(got, ref, 3)
    assert got["launches"] == 1 and got["redo_pixels"] == 0
    # (S3 under REF_ABORT: the oracle itself leaves pixels NaN at 3 spp; the status and the NaN pattern are held to its)
    assert got["status"] == ref["status"] and (got["status"] == hipmod.E_NONFINITE) == (want["status"] == 1)
    assert got["nonfinite_pixels"] == ref["nonfinite_pixels"] == want["nonfinite_pixels"]
    assert got["first_bad_pixel"] == ref["first_bad_pixel"]
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(want["colour"]))
    assert np.array_equal(got["nbhd_size"], want["nbhd_size"])
    fin = np.isfinite(want["colour"])
    assert fin[:, b].any()
    whole = rel_l2(got["colour"][fin], want["colour"][fin])
    assert np.isfinite(got["colour"][fin]).all() and whole <= REL_L2_BAR, whole
    finr = fin[:, b]
    g = rel_l2(got["colour"][:, b][finr], want["colour"][:, b][finr])
    e32 = sweep_distance(oracle, fid, policy, seed, np.float32) if sweep else yardstick_distance(oracle, fid, lay, policy, seed, np.float32)
    print("Y %s %s G policy %d seed %g: g = %.3e  e32 = %.3e  g / e32 = %s  whole frame %.3e" % (
        fid, lay_ids(lay), policy, seed, g, e32, "%.2f" % (g / e32) if e32 > 0 else "-", whole))
    assert g <= REGRESSION_FACTOR * e32 + 1e-12, (g, e32)
    if seed == ACTIVE:
        d = rel_l2(got["colour"][:, b][finr], ref["colour"][:, b][finr])
        assert d > 1e-10, d
    return got, ref, want


# ---- 4. route 3 whole ----------------------------------------------------------------------------------------------------------------
ROUTE3_CASES = [("edge", lay) for lay in LAYOUTS] + [("E16", lay) for lay in LAYOUTS] + [("E32", FRAMES["E32"][0]), ("G72", G72_LAY)]


@SEEDS
@POLICIES
@pytest.mark.parametrize("case", ROUTE3_CASES, ids=lambda v: "%s-%s" % (v[0], lay_ids(v[1])))
def test_route3_whole_pass_is_fp32(ctx, hipmod, oracle, case, policy, seed):
    fid, lay = case
    got, _, want = five_bars_route3(ctx, hipmod, oracle, fid, lay, policy, seed)
    n = want["nbhd_size"]
    assert fid not in ("edge", "E16") or (n < 256).any()        # threads that hold no member
    assert fid != "E32" or any_geometry(fid)[2] == 32
    assert fid != "G72" or any_geometry(fid)[2] % 16 == 8


# ---- 5. S below and across the sweep width -----------------------------------------------------------------------------------------
@SEEDS
@POLICIES
@pytest.mark.parametrize("fid", ["S3", "S21"])
def test_sweep_width_frames(ctx, hipmod, oracle, fid, policy, seed):
    five_bars_route3(ctx, hipmod, oracle, fid, SWEEP_LAY, policy, seed)
    S = sweep_geometry(fid)[2]
    assert (S < 8) if fid == "S3" else (S % 8 == 5 and S % 16 == 5)


# ---- 6. the rest list only ---------------------------------------------------------------------------------------------------------------
@POLICIES
@pytest.mark.parametrize("fid", ["E32", "G72"])
def test_rest_list_only(ctx, hipmod, oracle, fid, policy):
    lay = FRAMES["E32"][0] if fid == "E32" else G72_LAY
    W, H, S, box = any_geometry(fid)
    b = (box - 1) // 2
    want = any_oracle(oracle, fid, lay, policy, ACTIVE)
    ref = frame_run(ctx, hipmod, fid, lay, policy, ACTIVE, "GPW")
    got = frame_run(ctx, hipmod, fid, lay, policy, ACTIVE, "GPWY")
    discrete_equal(got, ref, 5)
    assert got["status"] == ref["status"] == hipmod.OK
    rest = want["nbhd_size"] > 832
    assert rest[b].any() and (~rest[b]).any()
    assert got["colour"][:, ~rest].tobytes() == ref["colour"][:, ~rest].tobytes()         # the classes: steered by X alone
    y32 = yardstick_row(oracle, fid, lay, policy, ACTIVE, np.float32)
    wr, gr = want["colour"][:, b][:, rest[b]], got["colour"][:, b][:, rest[b]]
    assert np.isfinite(wr).all()
    g, e32 = rel_l2(gr, wr), rel_l2(y32[:, rest[b]], wr)
    print("Y %s GPW policy %d, rest list of the target row (%d pixels): g = %.3e  e32 = %.3e  g / e32 = %.2f" % (
        fid, policy, int(rest[b].sum()), g, e32, g / e32))
    assert g <= REGRESSION_FACTOR * e32 + 1e-12, (g, e32)
    assert rel_l2(gr, ref["colour"][:, b][:, rest[b]]) > 1e-10
    # with both flags every pixel is fp32: the classes are those of G P W X, the rest list that of G P W Y
    both = frame_run(ctx, hipmod, fid, lay, policy, ACTIVE, "GPWXY")
    x = frame_run(ctx, hipmod, fid, lay, policy, ACTIVE, "GPWX")
    discrete_equal(both, ref, 5)
    fin = np.isfinite(want["colour"])
    assert rel_l2(both["colour"][fin], want["colour"][fin]) <= REL_L2_BAR
    gb = rel_l2(both["colour"][:, b], want["colour"][:, b])
    eb = yardstick_distance(oracle, fid, lay, policy, ACTIVE, np.float32)
    assert gb <= REGRESSION_FACTOR * eb + 1e-12, (gb, eb)
    assert both["colour"][:, ~rest].tobytes() == x["colour"][:, ~rest].tobytes()
    assert both["colour"][:, rest].tobytes() == got["colour"][:, rest].tobytes()


# ---- 7. SD == 0 on a weighted column -------------------------------------------------------------------------------------------------
def test_constant_colour_channel_eps(ctx, hipmod, oracle):
    got, ref, want = five_bars_route3(ctx, hipmod, oracle, "S21C", SWEEP_LAY, EPS, ACTIVE)
    assert (got["stddev"][..., 3] == 0).all()


def test_constant_colour_channel_ref_abort(ctx, hipmod):
    got = frame_run(ctx, hipmod, "S21C", SWEEP_LAY, REF_ABORT, ACTIVE, "GY")
    ref = frame_run(ctx, hipmod, "S21C", SWEEP_LAY, REF_ABORT, ACTIVE, "G")
    discrete_equal(got, ref, 3)
    assert got["status"] == ref["status"]
    assert got["nonfinite_pixels"] == ref["nonfinite_pixels"] and got["first_bad_pixel"] == ref["first_bad_pixel"]
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(ref["colour"]))
    fin = np.isfinite(ref["colour"])
    if fin.any():
        assert rel_l2(got["colour"][fin], ref["colour"][fin]) <= REL_L2_BAR


# ---- 8. non-finite inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", INF_INJECTIONS)
def test_infinite_features_vs_oracle(ctx, hipmod, oracle, kind):
    """the assertions of tests/test_generic_fast_gpu.py::test_infinite_features_vs_oracle under G | Y (the numpy fp32 form keeps the
    oracle's NaN pattern on all five injections under both policies)"""
    W, H, S, box = INF_SHAPE
    planes, pix = inf_frame(kind)
    for policy in (hipmod.DEGEN_EPS, hipmod.DEGEN_REF_ABORT):
        want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=policy))
        got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=policy, flags=flag_bits(hipmod, "GY")), box=box, allow_nonfinite=True)
        assert ctx.route() == 3
        tag = (policy,)
        assert np.array_equal(got["nbhd_size"], want["nbhd_size"]), tag
        assert np.array_equal(got["member_hash"], want["member_hash"]), tag
        assert (got["status"] == hipmod.E_NONFINITE) == (want["status"] == 1), tag
        assert got["nonfinite_pixels"] == want["nonfinite_pixels"], tag
        assert got["first_bad_pixel"] == want["first_bad_pixel"], tag
        assert np.array_equal(np.isnan(got["colour"]), np.isnan(want["colour"])), tag
        if np.isfinite(want["colour"]).all():
            check_pass(got, want)
        else:
            fin = np.isfinite(want["colour"])
            assert rel_l2(got["colour"][fin], want["colour"][fin]) <= REL_L2_BAR, tag


# ---- 9. the redo list --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", RESIDUE_S)
def test_wave_residue_frames_are_redone_in_fp64(ctx, hipmod, oracle, S):
    planes = residue_frame(oracle, S)[0]
    got = run_debug(ctx, planes, desc_for(hipmod, RESIDUE_LAY, RESIDUE_W, 1, S, "GPWY", policy=REF_ABORT), RESIDUE_BOX)
    ref = run_debug(ctx, planes, desc_for(hipmod, RESIDUE_LAY, RESIDUE_W, 1, S, "GPW", policy=REF_ABORT), RESIDUE_BOX)
    discrete_equal(got, ref, 5)
    assert got["redo_pixels"] == RESIDUE_W > 0            # every pixel of the frame is redone
    bits_equal(got, ref, ("colour",))


@pytest.mark.parametrize("case", ["A", "B"])
@pytest.mark.parametrize("lay", RESIDUE_LAYOUTS, ids=lay_ids)
def test_packed_residue_frames_are_redone_in_fp64(ctx, hipmod, oracle, lay, case):
    W, S = RESIDUE_CASES[case]
    planes = pk_residue_frame(oracle, lay, case)[0]
    got = run_debug(ctx, planes, desc_for(hipmod, lay, W, 1, S, "GPWY", policy=REF_ABORT), PK_RESIDUE_BOX)
    ref = run_debug(ctx, planes, desc_for(hipmod, lay, W, 1, S, "GPW", policy=REF_ABORT), PK_RESIDUE_BOX)
    discrete_equal(got, ref, 5)
    assert got["redo_pixels"] == W > 0
    bits_equal(got, ref, ("colour",))


# ---- 10. route 6 ---------------------------------------------------------------------------------------------------------------------------
_wide = {}


def wide_y(ctx, hipmod, fid, policy):
    if (fid, policy) not in _wide:
        _wide[fid, policy] = TW.run_row(ctx, hipmod, fid, policy, flags=TW.flags_of(hipmod, fid) | hipmod.FLAG_STREAM_FAST)
    return _wide[fid, policy]


def per_pixel_regression(oracle, fid, policy, got_px, label):
    """got_px [3, checked pixels, S]: the regression bar per checked pixel and over the set, where the oracle is finite"""
    ref = wide_reference(fid, policy)
    y32 = wide_yardstick(oracle, fid, policy, np.float32)
    fin = np.isfinite(ref).all(axis=(0, 2))
    g, e32 = rel_l2(got_px[:, fin], ref[:, fin]), rel_l2(y32[:, fin], ref[:, fin])
    gp, ep = per_pixel(got_px, ref)[fin], per_pixel(y32, ref)[fin]
    print("Y %s policy %d, %d pixels: g = %.3e  e32 = %.3e  g / e32 = %.2f  per pixel g / e32 = %.2f ... %.2f" % (
        label, policy, int(fin.sum()), g, e32, g / e32, (gp / ep).min(), (gp / ep).max()))
    assert g <= REGRESSION_FACTOR * e32 + 1e-12, (g, e32)
    assert (gp <= REGRESSION_FACTOR * ep + 1e-12).all(), (gp, ep)


@POLICIES
@pytest.mark.parametrize("fid", WIDE_FIDS)
def test_route6_vs_fixture(ctx, hipmod, oracle, fid, policy):
    got, ref = wide_y(ctx, hipmod, fid, policy), TW.base(ctx, hipmod, fid, policy)
    TW.assert_wide_pass(got, hipmod, fid)
    discrete_equal(got, ref, 6)
    assert got["status"] == ref["status"]
    want = TW.want_row(fid, policy)
    row = TW.row_of(got)
    r = rel_l2(row["colour"], want["colour"])
    assert np.isfinite(want["colour"]).all() and r <= REL_L2_BAR, r
    xs = wide_case(fid, policy)[3]
    per_pixel_regression(oracle, fid, policy, got["colour"][:, WF.ROW, xs], "route 6 " + fid)
    assert rel_l2(got["colour"][:, WF.ROW], ref["colour"][:, WF.ROW]) > 1e-10


def test_route6_heavy_cells(ctx, hipmod):
    got = wide_y(ctx, hipmod, "heavy", REF_ABORT)
    TW.assert_wide_pass(got, hipmod, "heavy")
    discrete_equal(got, TW.base(ctx, hipmod, "heavy", REF_ABORT), 6)
    check_pass(TW.row_of(got), TW.want_row("heavy", REF_ABORT))      # MI and the discrete outputs as without Y; colours: the contract


# ---- 11. route 7 ---------------------------------------------------------------------------------------------------------------------------
@POLICIES
def test_route7_classes_and_rest(ctx, hipmod, oracle, policy):
    ref = TC.wide_run(ctx, hipmod, policy, True)
    flags = TC.wide_flags(hipmod, (2, 12, "f32"), True) | hipmod.FLAG_STREAM_FAST
    got = TC.run_debug(ctx, WC.frame()[0], TC.wide_desc(hipmod, policy, True, flags=flags), WC.BOX)
    discrete_equal(got, ref, 7)
    assert got["status"] == ref["status"] and got["nonfinite_pixels"] == ref["nonfinite_pixels"]
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(ref["colour"]))
    for (y, x), n in zip(WC.frame()[1], WC.TARGETS):
        assert got["nbhd_size"][y, x] == n
    xs = wide_case("classes", policy)[3]
    assert {x for _, x in WC.frame()[1]} <= set(xs)                    # every class's targets, 833 and 66049 among them
    per_pixel_regression(oracle, "classes", policy, got["colour"][:, WC.ROW, xs], "route 7")
    n = got["nbhd_size"][WC.ROW]
    fin = np.isfinite(ref["colour"][:, WC.ROW]).all(axis=(0, 2))
    for name, sel in (("class", n <= 832), ("rest", n > 832)):
        sel = sel & fin
        d = rel_l2(got["colour"][:, WC.ROW][:, sel], ref["colour"][:, WC.ROW][:, sel])
        print("route 7 policy %d: %d %s pixels, distance from the base %.3e (redo %d)" % (policy, int(sel.sum()), name, d, got["redo_pixels"]))
        assert sel.any() and d > 1e-10, (name, d)


# ---- 12. one text ------------------------------------------------------------------------------------------------------------------------
@POLICIES
def test_forced_wide_pass_gives_route3_bits(hipmod, policy):
    planes, _ = TW.small_frame()
    W, H, S = 2 * WF.BOX, WF.BOX, 14
    kw = dict(policy=policy, sigma_seed=WF.SIGMA_SEED, row_begin=WF.ROW, row_end=WF.ROW + 1)
    with hipmod.Context(0) as c:
        ref = run_debug(c, planes, hipmod.make_desc(W, H, S, flags=flag_bits(hipmod, "GY"), **kw), WF.BOX)
        c.set_option("wide", 1)
        got = run_debug(c, planes, hipmod.make_desc(W, H, S, flags=flag_bits(hipmod, "GNY"), **kw), WF.BOX)
        base = run_debug(c, planes, hipmod.make_desc(W, H, S, flags=flag_bits(hipmod, "GN"), **kw), WF.BOX)
    assert ref["route"] == 3 and got["route"] == 6 and base["route"] == 6
    assert got["status"] == ref["status"]
    bits_equal(got, ref, STAGE_KEYS + ("colour",))
    assert rel_l2(got["colour"][:, WF.ROW], base["colour"][:, WF.ROW]) > 1e-10


# ---- 13. untouched passes ------------------------------------------------------------------------------------------------------------------
_full = {}


def full_pass_y(ctx, hipmod):
    """rpf_filter_ex, one wide pass (box 57) over the 57 x 57 x 21 buffer of tests/test_wide_nbhd_gpu.py under N | Y, EPS"""
    if not _full:
        d = TW.desc_of(hipmod, "heavy", EPS, boxes=(WF.BOX,), flags=flag_bits(hipmod, "NY"))
        srgb, prgb, st, c64 = ctx.filter(TW.buf57(), d, want_colour64=True)
        cnt = ctx.counters()
        assert st == hipmod.OK and ctx.route() == 6 and cnt.filter_kernel_launches == 1 and cnt.redo_pixels == 0
        _full.update(d=d, srgb=srgb, prgb=prgb, c64=c64)
    return _full


def test_second_pass_of_a_wide_call_is_untouched(ctx, hipmod):
    planes, ny = TW.buf57(), flag_bits(hipmod, "NY")
    first = full_pass_y(ctx, hipmod)["c64"]
    assert rel_l2(first, TW.full_pass(ctx, hipmod)["c64"]) > 1e-10          # pass 1 really is fp32 ...
    assert rel_l2(first, TW.full_pass(ctx, hipmod)["c64"]) <= REL_L2_BAR
    _, _, st, both = ctx.filter(planes, TW.desc_of(hipmod, "heavy", EPS, boxes=(WF.BOX, 7), flags=ny), want_colour64=True)
    assert st == hipmod.OK and ctx.route() == 2
    launches = ctx.counters().filter_kernel_launches
    _, _, st, second = ctx.filter(planes, TW.desc_of(hipmod, "heavy", EPS, boxes=(7,)), colour64_in=first, want_colour64=True)
    assert st == hipmod.OK and ctx.route() == 2                             # ... and pass 2 runs as without Y
    assert np.array_equal(both, second)
    _, _, st, _ = ctx.filter(planes, TW.desc_of(hipmod, "heavy", EPS, boxes=(WF.BOX, 7)), want_colour64=True)
    assert ctx.route() == 2 and ctx.counters().filter_kernel_launches == launches


@POLICIES
def test_fused_routes_and_their_streaming_class_are_untouched(ctx, hipmod, policy):
    (lay, S, box, targets, _, _), (stored, _, pixels, _) = P.FRAMES["B40"], P.frame("B40")
    W, H = box * len(targets), box
    assert max(targets) > 3136 and lay == (2, 12, "f32")
    ref = run_debug(ctx, stored, hipmod.make_desc(W, H, S, policy=policy, sigma_seed=ACTIVE, flags=flag_bits(hipmod, "N")), box)
    got = run_debug(ctx, stored, hipmod.make_desc(W, H, S, policy=policy, sigma_seed=ACTIVE, flags=flag_bits(hipmod, "NY")), box)
    assert got["route"] == ref["route"] and ref["route"] in (0, 1, 2)
    assert got["launches"] == ref["launches"] and got["redo_pixels"] == ref["redo_pixels"] and got["status"] == ref["status"]
    for (y, x), n in zip(pixels, targets):
        assert got["nbhd_size"][y, x] == n
    bits_equal(got, ref, STAGE_KEYS + ("colour",))


# ---- 14. entry points ----------------------------------------------------------------------------------------------------------------------
ENTRY_LAY = (3, 7, "f32")
_entry = {}


def entry_filter(ctx, hipmod):
    """the two-pass filter call under G | Y that every other entry point must reproduce: run once, shared"""
    if not _entry:
        W, H, S = 15, 12, 8
        planes, p32 = entry_frame()
        d = desc_for(hipmod, ENTRY_LAY, W, H, S, "GY", boxes=(7, 5), policy=EPS)
        srgb, prgb, st, c64 = ctx.filter(planes, d, want_colour64=True)
        assert st == hipmod.OK and ctx.route() == 3
        _entry.update(planes=planes, p32=p32, d=d, srgb=srgb, prgb=prgb, c64=c64)
    return _entry


def test_entries_two_passes_pinned_and_multi_context(ctx, hipmod, oracle):
    W, H, S = 15, 12, 8
    e = entry_filter(ctx, hipmod)
    c = None
    for box in (7, 5):
        c = oracle.filter_pass(e["p32"], oracle.make_desc(W, H, S, box=box, policy=EPS, n_random=3, n_feat=7), colour_in=c, debug=False)["colour"]
    assert rel_l2(e["c64"], c) <= REL_L2_BAR
    assert np.array_equal(e["srgb"], e["c64"].astype(np.float32))
    _, _, _, c64_ref = ctx.filter(e["planes"], desc_for(hipmod, ENTRY_LAY, W, H, S, "G", boxes=(7, 5), policy=EPS), want_colour64=True)
    assert rel_l2(c64_ref, c) <= 1e-9 and not np.array_equal(c64_ref, e["c64"])        # really fp32
    # page-locked buffers take the host pipeline's path; 12 rows are ONE band there (a frame below 32 rows is never cut), so this is the
    # serial order on the pipeline's streams -- the cut into several bands is held by tests/test_host_bands_gpu.py
    pin = ctx.host_empty(e["planes"].shape, e["planes"].dtype)
    pin[...] = e["planes"]
    out_s, out_p = ctx.host_empty(e["srgb"].shape), ctx.host_empty(e["prgb"].shape)
    ctx.filter(pin, e["d"], out_samples=out_s, out_pixels=out_p)
    assert ctx.route() == 3
    assert np.array_equal(out_s, e["srgb"]) and np.array_equal(out_p, e["prgb"])
    with hipmod.MultiContext([0, 0]) as mc:                                              # two slabs on one device
        s2, p2, st2 = mc.filter(e["planes"], e["d"])
    assert st2 == hipmod.OK
    assert np.array_equal(s2, e["srgb"]) and np.array_equal(p2, e["prgb"])


def test_entries_row_slab(ctx, hipmod):
    W, H, S = 15, 12, 8
    planes = entry_filter(ctx, hipmod)["planes"]
    full = run_debug(ctx, planes, desc_for(hipmod, ENTRY_LAY, W, H, S, "GY", policy=EPS), 7)
    part = run_debug(ctx, planes, desc_for(hipmod, ENTRY_LAY, W, H, S, "GY", policy=EPS, row_begin=3, row_end=9), 7)
    assert full["route"] == 3 and part["route"] == 3
    assert np.array_equal(part["colour"][:, 3:9], full["colour"][:, 3:9])
    assert np.array_equal(part["colour"][:, :3], planes[2:5, :3].astype(np.float64))
    s_full, _, _ = ctx.filter(planes, desc_for(hipmod, ENTRY_LAY, W, H, S, "GY", boxes=(7,), policy=EPS), want_pixels=False)
    s_part, _, _ = ctx.filter(planes, desc_for(hipmod, ENTRY_LAY, W, H, S, "GY", boxes=(7,), policy=EPS, row_begin=3, row_end=9), want_pixels=False)
    assert np.array_equal(s_part[:, 3:9], s_full[:, 3:9])
    assert np.array_equal(s_full, full["colour"].astype(np.float32))


def test_entries_filter_film_and_filter_device(ctx, hipmod):
    import torch
    W, H, S = 15, 12, 8
    e = entry_filter(ctx, hipmod)
    planes, d = e["planes"], e["d"]
    rw = (0.5 + np.random.default_rng(3).random((H, W, S))).astype(np.float32)
    film = hipmod.make_film(((0, 0), (W, H)), 0.5, hipmod.film_table(FR.BOX))
    srgb, t, w, img = ctx.filter_film(planes, d, film, ray_weight=rw)
    assert ctx.route() == 3
    assert np.array_equal(srgb, e["srgb"])
    t2, w2, img2 = film_device(ctx, hipmod, planes[0:2], e["c64"], film, rw)
    assert np.array_equal(t, t2) and np.array_equal(w, w2) and np.array_equal(img, img2)
    dev = torch.device("cuda", 0)
    dp = torch.from_numpy(np.ascontiguousarray(planes)).to(dev)
    col = dp[2:5].to(torch.float64).contiguous()
    ctx.filter_device(d, dp.data_ptr(), col.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ctx.route() == 3
    assert np.array_equal(col.cpu().numpy(), e["c64"])


def test_entries_wide_buffer(ctx, hipmod):
    """the 57 x 57 x 21 buffer under N | Y: a row slab, rpf_filter_device, two slab contexts and rpf_filter_film on the bits of
    the one-context call"""
    import torch
    ref = full_pass_y(ctx, hipmod)
    part = ctx.filter_pass_debug(TW.buf57(), TW.desc_of(hipmod, "heavy", EPS, row_begin=WF.ROW, row_end=WF.ROW + 1, flags=flag_bits(hipmod, "NY")), box=WF.BOX)
    assert ctx.route() == 6 and np.array_equal(part["colour"][:, WF.ROW], ref["c64"][:, WF.ROW])
    dev = torch.device("cuda", 0)
    planes = torch.from_numpy(TW.buf57().copy()).to(dev)
    col = planes[2:5].to(torch.float64).contiguous()
    ctx.filter_device(ref["d"], planes.data_ptr(), col.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ctx.route() == 6 and np.array_equal(col.cpu().numpy(), ref["c64"])
    with hipmod.MultiContext([0, 0]) as mc:
        srgb, prgb, st = mc.filter(TW.buf57(), ref["d"])
    assert st == hipmod.OK and np.array_equal(srgb, ref["srgb"]) and np.array_equal(prgb, ref["prgb"])
    W, H = WF.geometry("heavy")
    film = hipmod.make_film(((0, 0), (W, H)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX), sample_origin=(0, 0))
    srgb, _, _, _ = ctx.filter_film(TW.buf57(), ref["d"], film)
    assert ctx.route() == 6 and np.array_equal(srgb, ref["srgb"])


def test_run_to_run_determinism(ctx, hipmod):
    lay = (3, 7, "f32")
    W, H, S, box = any_geometry("E16")
    for policy, letters in ((EPS, "GY"), (REF_ABORT, "GPWXY")):
        d = desc_for(hipmod, lay, W, H, S, letters, policy=policy, sigma_seed=ACTIVE)
        a = run_debug(ctx, any_frame("E16", lay)[0], d, box)
        b = run_debug(ctx, any_frame("E16", lay)[0], d, box)
        bits_equal(a, b, STAGE_KEYS + ("colour",))
    a = TW.row_of(wide_y(ctx, hipmod, "l1_1", EPS))
    with hipmod.Context(0) as c:
        b = TW.row_of(TW.run_row(c, hipmod, "l1_1", EPS, flags=TW.flags_of(hipmod, "l1_1") | hipmod.FLAG_STREAM_FAST))
    for k in STAGE_KEYS + ("colour",):
        assert np.array_equal(a[k], b[k]), k


def test_refusals_on_a_live_context(ctx, hipmod):
    lay, (W, H, S) = (3, 7, "f32"), (6, 5, 4)
    planes, _ = buffers(lay, W, H, S, seed=5, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    ctx.filter_pass_debug(planes, desc_for(hipmod, lay, W, H, S, "GY", policy=EPS), box=3)
    before = ctx.counters().filter_kernel_launches
    assert before == 1 and ctx.route() == 3
    for letters in REFUSED:
        d = hipmod.make_desc(W, H, S, n_random=3, n_feat=7, policy=EPS, flags=flag_bits(hipmod, letters))
        for call in (lambda: ctx.filter_pass_debug(planes, d, box=3), lambda: ctx.filter(planes, d)):
            with pytest.raises(hipmod.RpfError) as e:
                call()
            assert e.value.status == hipmod.E_UNSUPPORTED, letters
            assert ctx.counters().filter_kernel_launches == before and ctx.route() == 3, letters
