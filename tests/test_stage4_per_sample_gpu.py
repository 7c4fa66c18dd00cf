"""Every route's filtered colours, sample by sample: stage 4 (the S x N pair weights and the blend) of every kernel that has a
stage-4 body of its own -- rpf_filter_impl.inc, rpf_packed_impl.inc, rpf_generic_stream_stages.inc (the one text of
rpf_generic.hip and rpf_generic_wide.hip), rpf_generic_packed.hip, rpf_generic_wave.hip -- against the fp64 numpy restatement of tests/fast_weights_ref.py evaluated on the
DEVICE's own stage 1 to 3 outputs.  check_pass holds those outputs to the oracle (bit for bit, 1e-11, 1e-9); what is left
between got["colour"] and stage4(planes, got) is the device's pair arithmetic and blend alone, and it is held to the
worst-case rounding bound of tests/stage4_bars.py on EVERY finite sample of the checked pixels: the whole target row of a
planted frame, every pixel of a synthetic frame.  A norm over the frame (check_pass's 1e-4) cannot see one wrong sample, and at
the reference's sigma seed the filter is the identity on most frames of the suite; every frame here is filter-active
(tests/test_stage4_per_sample_cpu.py asserts rel-L2(oracle output, input) >= 0.05 on the checked pixels of each).

The restatement is always evaluated in the direct form; the bar is the one of the form the kernel uses (stage4_bars.py:
fused and packed fused kernels expanded, every generic kernel direct; on a fused route a neighbourhood above 3136 samples
runs on the generic streaming kernel and takes the direct bar).  No bar is fitted: a case that exceeds it is a finding.

Every case asserts the route rpf_query_route reports, and prints one line "STAGE4 <case> route r: worst d (bar b)".
Measured on the MI355X: DESIGN.md section 5."""
import numpy as np
import pytest

import fast_weights_ref as R
import stage4_bars as B
import wide_frames as WF
from test_generic_wave_gpu import desc_for as wave_desc
from test_gpu_parity import _assert_oracle_parity, check_pass
from test_stage4_per_sample_cpu import (EDGE_LAY, FUSED_PLANTED, R3_LAYOUTS, R3_SHAPES, SECOND_BOX, SYNTH, at, case_oracle,
                                        edge_case, planted_case, r3_case, synth_case, wide_main_case, wide_small_case)
from test_generic_packed_cpu import EDGE_LAYOUTS, lay_ids
from test_generic_wave_cpu import LAYOUTS as WAVE_LAYOUTS
from test_wide_classes_gpu import SMALL as WIDE_SMALL, desc_of as wide_desc, forced  # noqa: F401  (forced: a fixture)
from test_wide_nbhd_gpu import desc_of as wide_main_desc, row_of as wide_main_row, want_row as wide_main_want

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
POLICIES = pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])


def fused_desc(hipmod, case, policy, **kw):
    nr, nf, dt = case.lay
    lay = dict(n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16) if dt == "f16" else {}
    return hipmod.make_desc(case.W, case.H, case.S, policy=policy, sigma_seed=case.seed, **lay, **kw)


def generic_desc(hipmod, case, policy, route, **kw):
    """routes 3, 4, 5 (G, G | P, G | P | W) in the case's layout"""
    return wave_desc(hipmod, case.lay, case.W, case.H, case.S, route=route, policy=policy, sigma_seed=case.seed, **kw)


def per_pixel_bars(case, got, route):
    """sample bar (relative to cmax) of every checked pixel: the form of the kernel that filtered it, at the largest
    neighbourhood among the checked pixels of that form"""
    n = np.array([int(got["nbhd_size"][y, x]) for y, x in case.pixels])
    form = np.array([B.ROUTE_FORM[route]] * len(n), dtype=object)
    if B.ROUTE_FORM[route] == "expanded":
        form[n > B.RESIDENT] = "direct"         # the streaming size class: generic::filter_pixel_kernel
    bars = np.empty(len(n))
    for f in set(form):
        bars[form == f] = B.sample_bar(f, case.lay[1], n[form == f].max(), case.seed, case.box_used)
    return bars


class _Run:
    """a case with the box of this pass (a second pass filters with another box than the frame was planted for)"""

    def __init__(self, case, box):
        self.__dict__.update(case._asdict())
        self.box_used = box


def assert_stage4(c, hipmod, oracle, case, desc, want, routes, label, policy=EPS, box=None, colour64=None, want_slice=None):
    """one debug pass of `case` on context `c`; the route; check_pass (or, where the oracle's colours are not all finite, its
    NaN pattern and status); the member counts of the restatement; every finite sample of the checked pixels within the bar
    of the restatement on the device's own stage outputs; equal NaN patterns.  Returns (got, worst / cmax)."""
    run = _Run(case, case.box if box is None else box)
    got = c.filter_pass_debug(case.stored, desc, box=run.box_used, colour_in=colour64, allow_nonfinite=True)
    route = c.route()
    assert route in routes, (label, route, routes)
    if want_slice is None:
        _assert_oracle_parity(got, want, hipmod)
    else:
        check_pass(want_slice(got), want)
    cin = case.p32[2:5].astype(np.float64) if colour64 is None else np.asarray(colour64, np.float64)
    # (stage4 asserts that got["nbhd_size"] is its own member count at every checked pixel)
    ref = R.stage4(oracle, case.p32, got, run.box_used, case.seed, case.pixels, np.float64, policy, case.lay[0], case.lay[1],
                   colour64=colour64)
    mine = at(got["colour"], case.pixels)
    assert np.array_equal(np.isnan(mine), np.isnan(ref)), label
    cmax = B.cmax_of(cin)
    bars = per_pixel_bars(run, got, route)
    both = np.isfinite(mine) & np.isfinite(ref)
    dist = np.where(both, np.abs(mine - ref), 0.0).max(axis=(0, 2)) / cmax          # per checked pixel
    worst = int(np.argmax(dist / bars))
    print("STAGE4 %s route %d: worst %.3e (bar %.3e) at pixel %s N %d; %d samples" % (
        label, route, dist[worst], bars[worst], case.pixels[worst], int(got["nbhd_size"][case.pixels[worst]]), int(both.sum())))
    assert both.any(), label
    assert (dist <= bars).all(), (label, float(dist[worst]), float(bars[worst]))
    return got, float(dist.max())


def fused_routes(case):
    """what rpf_query_route answers for a fused pass: size-binned (2) when box * box * S > 512, else fused or count-first as
    the probe decides"""
    return (0, 1) if case.box * case.box * case.S <= 512 else (2,)


# ---- fused routes, default options ---------------------------------------------------------------------------------------------------
@POLICIES
@pytest.mark.parametrize("fid", FUSED_PLANTED)
def test_fused_routes_planted(ctx, hipmod, oracle, fid, policy):
    case = planted_case(fid)
    want = case_oracle(oracle, case, policy)
    got, _ = assert_stage4(ctx, hipmod, oracle, case, fused_desc(hipmod, case, policy), want, fused_routes(case),
                           "fused %s p%d" % (fid, policy), policy)
    n = np.array([got["nbhd_size"][y, x] for y, x in case.pixels])
    assert (n > B.RESIDENT).any() == (fid in ("B40", "B17"))       # the streaming kernel behind the fused route


# frame, option, value, routes: every option that changes which kernel runs stage 4
OPTIONS = ([("U8", "count_first", v, (v,)) for v in (0, 1)] + [("U8", "packed", v, (0, 1)) for v in (0, 1)]
           + [("U8", "split_weights", v, (0, 1)) for v in (0, 1)]
           + [("B16", "packed", v, (2,)) for v in (0, 1)] + [("B16", "waves_per_pixel", 4, (2,))]
           + [("B16", "split_weights", v, (2,)) for v in (0, 1)]
           + [(f, "split_weights", 0, (2,)) for f in ("B32", "B64")] + [(f, "waves_per_pixel", 1, (2,)) for f in ("B32", "B64")])


@pytest.mark.parametrize("fid,option,value,routes", OPTIONS, ids=["%s-%s%d" % o[:3] for o in OPTIONS])
def test_fused_route_options(hipmod, oracle, fid, option, value, routes):
    """a fresh context per option, as _run_opts does (nothing leaks)"""
    case = planted_case(fid)
    want = case_oracle(oracle, case, EPS)
    with hipmod.Context(0) as c:
        c.set_option(option, value)
        assert_stage4(c, hipmod, oracle, case, fused_desc(hipmod, case, EPS), want, routes, "fused %s %s=%d" % (fid, option, value))
        assert c.counters().options_active == 1


# ---- clipped windows and odd shapes: the fused route and route 3 ---------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", 3])
@pytest.mark.parametrize("W,H,S,box,mode", SYNTH, ids=["%s-%dx%dx%d-b%d" % ((s[4],) + s[:4]) for s in SYNTH])
def test_clipped_windows_and_odd_shapes(ctx, hipmod, oracle, W, H, S, box, mode, route):
    case = synth_case(W, H, S, box, mode)
    want = case_oracle(oracle, case, EPS)
    if route == 3:
        desc, routes = generic_desc(hipmod, case, EPS, 3), (3,)
    else:
        desc, routes = fused_desc(hipmod, case, EPS), fused_routes(case)
    assert_stage4(ctx, hipmod, oracle, case, desc, want, routes, "%s %s" % (route, case.name))


# ---- generic routes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", R3_LAYOUTS, ids=lay_ids)
@pytest.mark.parametrize("name", list(R3_SHAPES))
def test_route3_shapes_and_layouts(ctx, hipmod, oracle, name, lay):
    case = r3_case(name, lay)
    assert_stage4(ctx, hipmod, oracle, case, generic_desc(hipmod, case, EPS, 3), case_oracle(oracle, case, EPS), (3,), "r3 %s" % case.name)


R45 = ([(4, "edge", lay) for lay in EDGE_LAYOUTS] + [(5, "edge", EDGE_LAY)] + [(5, "E16", lay) for lay in WAVE_LAYOUTS]
       + [(5, "E32", EDGE_LAY), (5, "S72", EDGE_LAY), (4, "E16", EDGE_LAY)])


@pytest.mark.parametrize("route,fid,lay", R45, ids=["r%d-%s-%s" % (r, f, lay_ids(lay)) for r, f, lay in R45])
def test_routes_4_and_5_edge_frames(ctx, hipmod, oracle, route, fid, lay):
    """S72 stands in for E72 (box 3: sigma_p = 0, the filter is the identity): at 72 spp a pass has no packed pixel and
    rpf_query_route still answers 5"""
    case = edge_case(fid, lay)
    assert_stage4(ctx, hipmod, oracle, case, generic_desc(hipmod, case, EPS, route), case_oracle(oracle, case, EPS), (route,),
                  "r%d %s" % (route, case.name))


def forced_desc(hipmod, case, policy, classes, **kw):
    return wide_desc(hipmod, case.lay, case.W, case.H, case.S, policy, classes=classes, sigma_seed=case.seed, **kw)


@pytest.mark.parametrize("route", [6, 7])
@pytest.mark.parametrize("fid", WIDE_SMALL)
def test_routes_6_and_7_small_frames(forced, hipmod, oracle, fid, route):  # noqa: F811
    case = wide_small_case(fid)
    assert_stage4(forced, hipmod, oracle, case, forced_desc(hipmod, case, EPS, route == 7), case_oracle(oracle, case, EPS), (route,),
                  "r%d %s" % (route, fid))


def test_route_6_wide_main_target_row(ctx, hipmod, oracle):
    """box 57 at 21 spp, neighbourhoods of 65535 ... 68229 samples: the row of the targets against the restatement (on the
    cut of the row that wide_main_case documents), and check_pass against the oracle's whole row in
    tests/golden/wide_main.npz"""
    case, targets = wide_main_case(), WF.frame("main")[3]
    desc = wide_main_desc(hipmod, "main", EPS, row_begin=WF.ROW, row_end=WF.ROW + 1)
    got, _ = assert_stage4(ctx, hipmod, oracle, case, desc, wide_main_want("main", EPS), (6,), "r6 wide_main", want_slice=wide_main_row)
    assert got["max_nbhd"] == max(targets)


# ---- beta_map 1 and 2 on the routes whose stage-3c bodies have their own preset switch ------------------------------------------------
@pytest.mark.parametrize("beta_map", [1, 2])
@pytest.mark.parametrize("route", [4, 5, 6, 7])
def test_beta_presets_on_routes_4_to_7(ctx, forced, hipmod, oracle, route, beta_map):  # noqa: F811
    if route in (4, 5):
        case = edge_case("edge" if route == 4 else "E16")
        c, desc = ctx, generic_desc(hipmod, case, EPS, route, beta_map=beta_map)
    else:
        case = wide_small_case("U8")
        c, desc = forced, forced_desc(hipmod, case, EPS, route == 7, beta_map=beta_map)
    want = case_oracle(oracle, case, EPS, beta_map=beta_map)
    base = case_oracle(oracle, case, EPS)
    assert not np.array_equal(want["beta"], base["beta"])           # the preset changes beta on this frame
    assert_stage4(c, hipmod, oracle, case, desc, want, (route,), "r%d %s beta_map %d" % (route, case.name, beta_map))


# ---- second pass: the colours of a box-7 pass as colour_in of a box-5 pass -------------------------------------------------------------
@pytest.mark.parametrize("family", ["fused", 3, 4, 5, 6])
def test_second_pass(ctx, forced, hipmod, oracle, family):  # noqa: F811
    case = planted_case("U8") if family in ("fused", 6) else edge_case("edge")
    if family == "fused":
        c, desc, routes = ctx, fused_desc(hipmod, case, EPS), (0, 1)
    elif family == 6:
        c, desc, routes = forced, forced_desc(hipmod, case, EPS, False), (6,)
    else:
        c, desc, routes = ctx, generic_desc(hipmod, case, EPS, family), (family,)
    first = c.filter_pass_debug(case.stored, desc, box=case.box, debug=False, allow_nonfinite=True)["colour"]
    assert c.route() in routes and np.isfinite(first).all()
    kw = dict(n_random=case.lay[0], n_feat=case.lay[1]) if case.lay[:2] != (2, 12) else {}
    want = oracle.filter_pass(case.p32, oracle.make_desc(case.W, case.H, case.S, box=SECOND_BOX, policy=EPS, sigma_seed=case.seed, **kw),
                              colour_in=first)
    got, _ = assert_stage4(c, hipmod, oracle, case, desc, want, routes, "%s pass 2 %s" % (family, case.name), box=SECOND_BOX,
                           colour64=first)
    assert R.rel_l2(at(got["colour"], case.pixels), at(first, case.pixels)) >= 0.05      # the second pass is active as well
