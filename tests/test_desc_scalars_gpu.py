"""GPU tests of the two descriptor fields stage 3c reads, rpf_desc.beta_map and rpf_desc.eps, on every route: the table of
tests/desc_scalars.py, one test per row, the combos (1, 1e-10), (2, 1e-10), (0, 0.0123), (1, 0.0123), (2, 0.0123) looped inside.
Every pass is one rpf_filter_pass_debug on a planted frame (tests/planted_nbhd.py); tests/test_desc_scalars_cpu.py settles on
the CPU that the oracle's stage 3c is the restatement's under every combo, that every combo moves alpha or beta on every frame,
and that the frames' gains reach both arms of the clamp at either eps.

Per row, in order: the (0, 1e-10) pass; each combo under check_stage3c (alpha, beta, W_r_c are tests/schedule_ref.py on the
device's own MI: bit for bit, every pixel), check_against_default (nothing in front of stage 3c, no counter and no route moves)
and assert_planted (the classes the row names were reached); alpha, beta and W_r_c against the oracle's, restated from the
oracle's MI, at rtol 1e-9 / atol 1e-12 (tests/test_class_edges_routes_gpu.py:301); and, for (2, 0.0123), stage 4 on the target
row: schedule_ref.stage4_on on the device's own outputs under assert_row_stage4 of tests/test_class_edges_routes_gpu.py, with
the bar of the form the row's kernels use (tests/stage4_bars.py: the compiled kernels expanded, the layout-generic ones direct,
which is the tighter bar).  No tolerance of its own.  Each row prints one line "DESC <row> route r: ...".

Which body of stage 3c (A rpf_filter_impl.inc, B rpf_packed_impl.inc, C rpf_generic_stream_stages.inc, D rpf_generic_packed.hip,
E rpf_generic_wave.hip, F rpf_generic_quad.hip), which build and which classes a row reaches; "+gains" marks the rows that run
a second time under the frame's gains (RPF_FLAG_SCHEDULE, and RPF_FLAG_SCHEDULE_FUSED on the compiled kernels: the scheduled
builds, the `sched` branch of the generic bodies):

  row                          route  bodies  build / kernels                                   classes (planted N)
  compiled-U8          +gains  0 / 1  A B     d19 plain | scheduled; packed, one-wave           8 .. 65
  compiled-U8-binning1 +gains  2      A B     d19 size-binned                                   8 .. 65
  compiled-B16         +gains  2      A B     d19 one-wave classes                              16 .. 784
  compiled-B32         +gains  2      A       d19 four-wave / split K = 25                      832 | 833, 1568
  compiled-B32-split_weights0 +gains 2    A       d19 K = 25 unsplit                                832 | 833, 1568
  compiled-B64         +gains  2      A       d19 K = 49                                        1600 | 1601, 3135, 3136
  compiled-B40         +gains  2      A C     d19 resident | generic::filter_pixel_kernel       3136 | 3137, 3240
  compiled-H8          +gains  0 / 1  A B     d27 packed, one-wave                              8 .. 392
  compiled-H16         +gains  2      A       d27 mid                                           448 | 449, 784
  compiled-H64         +gains  2      A       d27 large                                         1600 | 1601, 3136
  r10-B16, r10-H16             10     A B     d19 / d27 member builds; bit-equal to route 2     as compiled-B16 / -H16
  r12-SP8 .. r12-SPH32 +gains  12     A B     d19 / d27 listed | listed-scheduled               8 .. 129, 256 .. 833, 833 .. 2400
  r11-SP8, r11-SPH16           11     A B     d19 / d27 behind acceptance masks; equal to 12    8 .. 129
  g3-U8, g3-B40        +gains  3      C       generic::filter_pixel_kernel                      8 .. 65; 3136 .. 3240
  g4-U8                +gains  4      D C     generic packed, rest list                         8 .. 64 | 65
  g5-B16               +gains  5      D E     generic packed and one-wave                       16 .. 784
  g13-B32 / B64 / H64  +gains  13     E F     generic four-wave, classes 1600 and 3136          832 | 833 .. 3136
  w6-U8, w7-U8         +gains  6, 7   C; DEC  generic::filter_wide_kernel; wide classes         8 .. 65
  r8-SP8, r8-SP16      +gains  8      D E C   listed members, rest launch                       8 .. 129; 256 .. 833
  r9-B16               +gains  9      D E     under planted_nbhd.nonref                         16 .. 784
  g3 / g4 / g5 -L1x3, -L3x5, -L8x27   3 4 5   C D E   layouts (1, 3) f32, (3, 5) f16, (8, 27) f32   8 .. 65
  g13-Q1x3, -Q3x5, -Q8x27      13     E F     the same layouts at B32's targets (class 1600)    832 | 833, 1568
  ...-FAST_WEIGHTS (U8, B32)   0/1, 2 A B     fp32 instantiations of the compiled kernels (a scheduled pass is refused)
  g5-B16-GENERIC_FAST  +gains  5      D E     fp32 instantiations, their `sched` branch
  g3-U8-STREAM_FAST    +gains  3      C       fp32 instantiation of generic::filter_pixel_kernel, its `sched` branch
  w6-U8-STREAM_FAST    +gains  6      C       fp32 instantiation of generic::filter_wide_kernel, its `sched` branch

Beside the table: the redo launch under REF_ABORT (presets 1 and 2 against the oracle; eps is not read), eps = 0 under EPS
(IEEE: NaN alpha and W_r_c, every colour falls back), and the refusal of a NaN or negative eps.

One deviation from the oracle's eps = 0 pattern (alpha[..., 0] and W_r_c NaN, everything else finite), on the route-8 row alone:
the sampled frame SP8 has, beside its targets, one pixel with N = S = 8 -- two bins a column -- on which further sums of MI are
exactly 0, so further entries of alpha and beta are 0 / 0 as well (the restatement over rpf_oracle_cf_weights gives the same on
the CPU).  There "everything else is finite" is not asserted; the NaN pattern of every plane is still the restatement's on the
device's own MI (check_stage3c), every colour falls back and every pixel is counted."""
import numpy as np
import pytest

import desc_scalars as D
import planted_nbhd as P
import schedule_ref as SRf
import test_class_edges_routes_gpu as CE
from desc_scalars import COMBOS, DEFAULT, EPS, REF_ABORT, SIGMA, STAGE4_COMBO, check_against_default, check_stage3c, same, same_or_nan
from test_gpu_parity import REL_L2_BAR, STAGE_KEYS, _assert_ref_abort_parity, rel_l2
from test_planted_routes_cpu import member_row, sampled_row
from test_wide_classes_gpu import forced, wide_flags  # noqa: F401  (forced: a fixture)

pytestmark = pytest.mark.gpu

PLANES = STAGE_KEYS + ("colour",)


def flags_of(hipmod, row, f):
    g, p, w = hipmod.FLAG_GENERIC, hipmod.FLAG_GENERIC_PACKED, hipmod.FLAG_GENERIC_WAVE
    sampled = hipmod.SAMPLED_NBHD_FLAG | (hipmod.SAMPLED_REST_FLAG if f.sampling and f.S + f.sampling[1] > 832 else 0)
    flags = {"compiled": 0, "r10": hipmod.MEMBER_TEST_FLAG | hipmod.MEMBER_FUSED_FLAG, "r9": hipmod.MEMBER_TEST_FLAG,
             "r8": sampled, "r11": sampled | hipmod.SAMPLED_FUSED_FLAG, "r12": sampled | hipmod.SAMPLED_LISTED_FLAG,
             "g3": g, "g4": g | p, "g5": g | p | w, "g13": g | p | w | hipmod.GENERIC_QUAD_FLAG,
             "w6": wide_flags(hipmod, f.lay, False), "w7": wide_flags(hipmod, f.lay, True)}[row.mode]
    if row.fast:
        flags |= {"FAST_WEIGHTS": hipmod.FLAG_FAST_WEIGHTS, "GENERIC_FAST": hipmod.FLAG_GENERIC_FAST, "STREAM_FAST": hipmod.FLAG_STREAM_FAST}[row.fast]
    return flags


def run_pass(c, hipmod, row, beta_map, eps, f=None, policy=EPS, gains="row", allow_nonfinite=False):
    """one rpf_filter_pass_debug of a row's frame under (beta_map, eps): the runner tests/test_schedule_fused_gpu.py::run is for
    its hard-coded descriptor.  Gains: under RPF_FLAG_SCHEDULE with the entry (SIGMA, gains), the descriptor's own seed the
    reference's; without: the descriptor's seed is SIGMA"""
    f = D.frame(row.fid) if f is None else f
    gains = row.gains if gains == "row" else gains
    nr, nf, dt = f.lay
    flags = flags_of(hipmod, row, f)
    mt = D.membership_of(row)
    if mt is not None:
        c.set_membership(hipmod.make_membership(mt[0].tolist(), mt[1].tolist()))
    if f.sampling is not None:
        c.set_sampling(hipmod.make_sampling(f.sampling[0], [f.sampling[1]]))
    if gains is not None:
        c.set_schedule(hipmod.make_schedule(SIGMA, *gains))
        flags |= hipmod.SCHEDULE_FLAG | (hipmod.SCHEDULE_FUSED_FLAG if row.mode in D.SCHEDULED_FUSED else 0)
    lay = dict(n_random=nr, n_feat=nf) if (nr, nf) != (2, 12) else {}
    if dt == "f16":
        lay["plane_dtype"] = hipmod.PLANES_F16
    desc = hipmod.make_desc(f.W, f.H, f.S, policy=policy, sigma_seed=SIGMA if gains is None else 0.002, flags=flags, beta_map=beta_map,
                            eps=eps, **lay)
    with CE.options(c, **row.opts):
        got = c.filter_pass_debug(f.stored, desc, box=f.box, allow_nonfinite=allow_nonfinite)
        cn = c.counters()
        got.update(route=c.route(), launches=cn.filter_kernel_launches, redo_pixels=cn.redo_pixels)
    return got


def planted(got, row, f):
    """CE.assert_planted for any frame of the table: the planted N at every target, on one of the row's routes"""
    sizes = [int(got["nbhd_size"][y, x]) for y, x in f.pixels]
    assert got["route"] in row.routes and sizes == list(f.targets), (row.id, got["route"], row.routes, sizes, f.targets)


def oracle_mi(oracle, row, f):
    """(MI, rows) the oracle parity runs on: the oracle's default pass (whole frame), or -- sampled passes and the test that is not
    the reference's have no oracle pass -- the restatement's target row"""
    b = (f.box - 1) // 2
    if f.sampling is not None:
        return sampled_row(oracle, row.fid)["mi"][b], b
    if row.mode == "r9":
        return member_row(oracle, row.fid, "nonref", weights=True)["mi"][b], b
    return D.oracle_pass(oracle, f)["mi"], slice(None)


def stage4(oracle, row, f, got, base, label):
    """stage 4 of one pass on the target row: (worst distance, its bar), relative to cmax"""
    nr, nf, _ = f.lay
    b = (f.box - 1) // 2
    cfg = None if f.sampling is None else (f.sampling[0], 0, f.sampling[1])
    nmax = None if f.sampling is None else min(f.box * f.box * f.S, f.S + f.sampling[1])
    ref = SRf.stage4_on(oracle, f.p32, got, SIGMA, f.box, EPS, mt=D.membership_of(row), cfg=cfg, rows=[b], n_random=nr, n_feat=nf)
    worst = CE.assert_row_stage4(got, ref, f.p32[2:5], b, f.box, label, nmax=nmax, n_feat=nf, form=D.form_of(row))
    assert np.isfinite(got["colour"][:, b]).all()
    assert not same(got["colour"][:, b], base["colour"][:, b]), label    # the combo reached the colours
    return worst


def check_row(c, hipmod, oracle, row, stage4_too=True):
    """the (0, 1e-10) pass and the five combos of a row; returns {combo: pass}"""
    f = D.frame(row.fid)
    nr, nf, _ = f.lay
    base = run_pass(c, hipmod, row, *DEFAULT)
    assert base["status"] == hipmod.OK
    planted(base, row, f)
    check_stage3c(base, *DEFAULT, row.gains, nr, nf)
    mi, sl = oracle_mi(oracle, row, f)
    gc, gf = row.gains or (1.0, 1.0)
    runs, worst = {DEFAULT: base}, None
    for beta_map, eps in COMBOS:
        got = run_pass(c, hipmod, row, beta_map, eps)
        assert got["status"] == hipmod.OK and got["nonfinite_pixels"] == 0, (row.id, beta_map, eps)
        planted(got, row, f)
        check_stage3c(got, beta_map, eps, row.gains, nr, nf)
        check_against_default(got, base, same_eps=runs.get((0, eps)))
        if nf == 3 and beta_map == 1:                   # no gap and no D_r_fk term: presets 0 and 1 are one statement
            for k in PLANES:
                assert same(got[k], runs[0, eps][k]), k
        else:
            assert not same(got["alpha"], base["alpha"]) or not same(got["beta"], base["beta"]), (row.id, beta_map, eps)
        want = SRf.alpha_beta(mi, gc, gf, beta_map, eps, nr, nf)         # the oracle's stage 3c, restated from its MI
        for k, w in zip(("alpha", "beta", "wrc"), want):
            np.testing.assert_allclose(got[k][sl], w, rtol=1e-9, atol=1e-12, err_msg="%s %s (%d, %g)" % (row.id, k, beta_map, eps))
        runs[beta_map, eps] = got
    if stage4_too:
        worst = stage4(oracle, row, f, runs[STAGE4_COMBO], base, "DESC %s (%d, %g)" % ((row.id,) + STAGE4_COMBO))
    print("DESC %s route %d: %d launches, %d combos, planted N %s, stage 4 worst %s" % (
        row.id, base["route"], base["launches"], len(COMBOS), "/".join(str(n) for n in f.targets),
        "not restated (fp32 weights)" if worst is None else "%.3e (bar %.3e, %s)" % (worst + (D.form_of(row),))))
    return runs


def context_of(row, ctx, forced):  # noqa: F811
    return forced if row.mode in ("w6", "w7") else ctx


TABLE = [r for r in D.ROWS if r.fast is None and r.mode not in ("r10", "r11")]
ANCHORED = [r for r in D.ROWS if r.mode in ("r10", "r11")]
FAST = [r for r in D.ROWS if r.fast is not None]
ids = lambda rows: [r.id for r in rows]  # noqa: E731


@pytest.mark.parametrize("row", TABLE, ids=ids(TABLE))
def test_every_route_reads_beta_map_and_eps(ctx, forced, hipmod, oracle, row):  # noqa: F811
    check_row(context_of(row, ctx, forced), hipmod, oracle, row)


@pytest.mark.parametrize("row", ANCHORED, ids=ids(ANCHORED))
def test_routes_10_and_11_equal_their_anchor_under_every_combo(ctx, hipmod, oracle, row):
    """route 10 under the reference's test is route 2, route 11 is route 12: the same code behind another list, every plane and
    the colours bit for bit under every combo"""
    anchor = next(r for r in D.ROWS if r.fid == row.fid and r.mode == {"r10": "compiled", "r11": "r12"}[row.mode] and r.gains is None and not r.opts)
    runs = check_row(ctx, hipmod, oracle, row)
    for combo, got in runs.items():
        want = run_pass(ctx, hipmod, anchor, *combo)
        assert want["route"] in anchor.routes
        CE.assert_same_pass(got, want)


@pytest.mark.parametrize("row", FAST, ids=ids(FAST))
def test_fp32_weights_keep_stage_3c_in_fp64(ctx, forced, hipmod, oracle, row):  # noqa: F811
    """under each fp32-weights flag stage 3c is the restatement's bits (check_row), and the colours of every combo lie within
    REL_L2_BAR of the same pass without the flag -- the bar tests/test_fast_weights_gpu.py, tests/test_generic_fast_gpu.py and
    tests/test_stream_fast_gpu.py hold the flag's colours to -- and are not its bits on the target row: the mode really is fp32.
    The rows with gains run RPF_FLAG_SCHEDULE on both sides: the `sched` branch of the fp32 instantiations"""
    c = context_of(row, ctx, forced)
    runs = check_row(c, hipmod, oracle, row, stage4_too=False)
    b = (D.frame(row.fid).box - 1) // 2
    for combo, got in runs.items():
        ref = run_pass(c, hipmod, row._replace(fast=None), *combo)
        for k in STAGE_KEYS:
            assert same(got[k], ref[k]), (k, combo)
        d = rel_l2(got["colour"], ref["colour"])
        assert not same(got["colour"][:, b], ref["colour"][:, b]) and d <= REL_L2_BAR, (combo, d)


# ---- e. the redo launch under REF_ABORT -------------------------------------------------------------------------------------------
REDO_ROWS = [D.Row("redo-" + m, "redo", m, {}, (r,), "", None, None) for m, r in (("compiled", 2), ("g3", 3), ("g5", 5), ("g13", 13))]


def redo_run(c, hipmod, row, beta_map, eps):
    return run_pass(c, hipmod, row, beta_map, eps, f=D.redo_frame(), policy=REF_ABORT, allow_nonfinite=True)


@pytest.mark.parametrize("row", REDO_ROWS, ids=ids(REDO_ROWS))
def test_redo_launch_reads_the_preset_and_not_eps(ctx, hipmod, oracle, row):
    """the frame of tests/test_gpu_parity.py::test_independent_tables_in_every_size_class_ref_abort: every pixel a class kernel
    filters is on the redo list, which generic::filter_pixel_kernel (body C) filters again"""
    W, H, S, box = D.REDO_SHAPE
    planes = D.redo_frame().p32
    pa, pb = oracle.pair_table()
    indep = [i for i in range(96) if (pa[i], pb[i]) == (7, 5)]
    n = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, sigma_seed=SIGMA))["nbhd_size"]
    assert (((n & (n - 1)) != 0).sum()) == W * H
    # who meets the in-band table: every class kernel; the generic filter kernel evaluates the reference's MI itself
    redo = {"compiled": W * H, "g3": 0, "g5": int((n <= 832).sum()), "g13": int((n <= 3136).sum())}[row.mode]
    base = None
    for beta_map in (0, 1, 2):
        ref = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, beta_map=beta_map, sigma_seed=SIGMA))
        got = redo_run(ctx, hipmod, row, beta_map, 1e-10)
        assert got["route"] in row.routes and got["redo_pixels"] == redo, (got["route"], got["redo_pixels"], redo)
        _assert_ref_abort_parity(got, ref, hipmod, indep)
        other = redo_run(ctx, hipmod, row, beta_map, 0.0123)             # the policy ignores the field
        for k in PLANES:
            assert same_or_nan(got[k], other[k]) if got[k].dtype == np.float64 else same(got[k], other[k]), (k, beta_map)
        assert (other["route"], other["launches"], other["redo_pixels"]) == (got["route"], got["launches"], got["redo_pixels"])
        if base is None:
            base = got
        else:
            assert not same_or_nan(got["beta"], base["beta"]) and same_or_nan(got["alpha"], base["alpha"])
    print("DESC %s route %d: %d launches, %d redo pixels, presets 0 / 1 / 2 x eps 1e-10 / 0.0123" % (row.id, base["route"], base["launches"], redo))


# ---- f. eps = 0 under EPS is IEEE ----------------------------------------------------------------------------------------------------
def _nan_rows():
    def row(fid, mode, routes, opts=None, gains=None, fast=None):
        name = "%s-%s" % (mode, fid) + ("-binning1" if opts else "") + ("-gains" if gains else "") + ("-" + fast if fast else "")
        return D.Row(name, fid, mode, opts or {}, routes, "", gains, fast)
    return [row("U8", "compiled", (0, 1)), row("U8", "compiled", (2,), dict(binning=1)), row("H8", "compiled", (0, 1)),
            row("U8", "compiled", (0, 1), gains=P.GAINS["U8"]), row("U8", "compiled", (2,), dict(binning=1), gains=P.GAINS["U8"]),
            row("U8", "g3", (3,)), row("U8", "g4", (4,)), row("U8", "g5", (5,)), row("U8", "w6", (6,)), row("SP8", "r8", (8,)),
            row("B32", "g13", (13,)), row("U8", "compiled", (0, 1), fast="FAST_WEIGHTS"), row("U8", "g5", (5,), fast="GENERIC_FAST")]


NAN_ROWS = _nan_rows()


@pytest.mark.parametrize("row", NAN_ROWS, ids=ids(NAN_ROWS))
def test_eps_zero_is_ieee_on_the_device(ctx, forced, hipmod, row):  # noqa: F811
    """colour plane 2 constant: its MI with everything is 0, so with eps = 0 the first W_r_c is 0 / 0.  What the oracle gives
    (tests/test_desc_scalars_cpu.py): alpha[..., 0] and W_r_c NaN on every pixel, beta finite, every colour the input's bits,
    status OK, every pixel counted; with eps 1e-10 or 0.0123 nothing is NaN and the colours move.  A NaN stays a NaN through
    schedule_factor"""
    c = context_of(row, ctx, forced)
    f = D.nan_frame(row.fid)
    nr, nf, _ = f.lay
    cin = f.p32[2:5].astype(np.float64)
    got = run_pass(c, hipmod, row, 0, 0.0, f=f, allow_nonfinite=True)
    planted(got, row, f)
    assert got["status"] == hipmod.OK and got["nonfinite_pixels"] == f.W * f.H
    assert np.isnan(got["alpha"][..., 0]).all() and np.isnan(got["wrc"]).all()
    if f.sampling is None:      # (a sampled frame has pixels of N = S = 8 beside the targets, two bins a column: other sums are 0 too.
        # The oracle has no sampled pass to settle that on; the NaN pattern is the restatement's on the device's MI, below)
        assert np.isfinite(got["alpha"][..., 1:]).all() and np.isfinite(got["beta"]).all()
    check_stage3c(got, 0, 0.0, row.gains, nr, nf)
    assert np.array_equal(got["colour"], cin)
    for eps in (1e-10, 0.0123):
        fin = run_pass(c, hipmod, row, 0, eps, f=f, allow_nonfinite=True)
        assert fin["status"] == hipmod.OK and fin["nonfinite_pixels"] == 0
        assert all(np.isfinite(fin[k]).all() for k in ("alpha", "beta", "wrc", "colour"))
        check_stage3c(fin, 0, eps, row.gains, nr, nf)
        for k in D.BITS:
            if k != "wrc":
                assert same(fin[k], got[k]), k
        assert rel_l2(fin["colour"], cin) > 0.05
    print("DESC eps0 %s route %d: %d launches, %d pixels fall back" % (row.id, got["route"], got["launches"], got["nonfinite_pixels"]))


# ---- the refusal ----------------------------------------------------------------------------------------------------------------------
def test_nan_or_negative_eps_is_refused_under_eps_alone(ctx, hipmod):
    f = D.frame("U8")

    def desc(eps, policy, **kw):
        return hipmod.make_desc(f.W, f.H, f.S, boxes=(f.box,), policy=policy, sigma_seed=SIGMA, eps=eps, **kw)
    want = ctx.filter_pass_debug(f.stored, desc(1e-10, REF_ABORT), box=f.box, allow_nonfinite=True)
    before = bytes(ctx.counters())
    for eps in (float("nan"), -1e-10, -0.0123, float("-inf")):
        for flags in (0, hipmod.FLAG_GENERIC):
            for call in (lambda d: ctx.filter_pass_debug(f.stored, d, box=f.box), lambda d: ctx.filter(f.stored, d),
                         lambda d: ctx.filter_device(d, None, None)):
                with pytest.raises(hipmod.RpfError) as e:
                    call(desc(eps, EPS, flags=flags))
                assert e.value.status == hipmod.E_BADARG and "eps" in str(e.value), str(e.value)
        assert bytes(ctx.counters()) == before                           # before any device work
    for eps in (0.0, -0.0, 5e-324, 1e-10, 0.0123, 1e300, float("inf")):  # a zero, +inf and every positive value
        got = ctx.filter_pass_debug(f.stored, desc(eps, EPS), box=f.box, allow_nonfinite=True)
        assert got["status"] == hipmod.OK
        check_stage3c(got, 0, eps, None, 2, 12)
    for eps in (float("nan"), -1.0, 0.0123):                             # REF_ABORT does not read the field
        got = ctx.filter_pass_debug(f.stored, desc(eps, REF_ABORT), box=f.box, allow_nonfinite=True)
        assert got["status"] == want["status"]
        for k in PLANES:
            assert same_or_nan(got[k], want[k]) if got[k].dtype == np.float64 else same(got[k], want[k]), (k, eps)
