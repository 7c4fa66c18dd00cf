"""GPU parity at every kernel-class edge on routes 10, 11 and 12 and on the scheduled builds: what tests/
test_class_boundaries_gpu.py does for routes 0 to 3, for the kernels behind RPF_FLAG_MEMBER_FUSED, RPF_FLAG_SAMPLED_FUSED,
RPF_FLAG_SAMPLED_LISTED and RPF_FLAG_SCHEDULE_FUSED.  The frames of tests/planted_nbhd.py put pixels at N = capacity and
N = capacity + 1 of every class a route can reach, and -- on the sampled routes -- at N = S + D = nmax, the pass's own bound, from
which routes 11 and 12 size their class kernels and to which the listed stage 1b cuts its copy.  tests/test_planted_routes_cpu.py
proves on the CPU that the restatements see the planted sizes, that the gains reach both arms of the clamp and that the filter is
active.

(a) route 10 on the full-box frames: under the reference's test the oracle and the unflagged route 2, bit for bit; under a test that
    is not the reference's, tests/member_test_ref.py on the target row and route 9 for the bin ids.
(b) the scheduled builds on the same frames: routes 0 / 1, 2 and 10.
(c) routes 11 and 12 on the sampled frames, against tests/sampled_ref.py on the target row, route 8 and each other, with and
    without gains.
(d) a row slab that is the target row alone.

EPS policy throughout (these routes refuse REF_ABORT: one assertion per route), the active sigma seed 0.5, and the reference's
0.002 in (a).  A Python restatement runs on the target row alone; device runs are compared on the whole frame.  Bars: bit equality,
check_pass / REL_L2_BAR, stage4_bars.sample_bar and the MI and weight bars of tests/test_sampled_gpu.py; no tolerance of its own.

check_scheduled_row states tests/test_schedule_fused_gpu.py::check_scheduled for a planted frame: that function looks its classes up
in its own table of frames and restates stage 4 on every pixel; here the classes are the planted ones and stage 4 is restated on the
target row."""
import numpy as np
import pytest

import member_test_ref as MR
import planted_nbhd as P
import sampled_ref as SR
import schedule_ref as SRf
import stage4_bars as B
import test_schedule_fused_gpu as SF
from test_class_boundaries_gpu import assert_oracle_parity, geometry
from planted_nbhd import GAINS, ROUTE10_FRAMES, SAMPLED_GAINS, class_of, nonref
from test_gpu_parity import STAGE_KEYS, rel_l2
from test_planted_routes_cpu import SHARE, layout, member_row, sampled_geometry, sampled_row

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
SIGMA = P.ACTIVE_SIGMA_SEED
FRONT = ("nbhd_size", "member_hash", "mean", "stddev")
BITS = FRONT + ("bin_hash",)
ALL = STAGE_KEYS + ("colour",)
DEFAULTS = dict(binning=-1, split_weights=-1, packed=-1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class options:
    """options set on a shared context, put back on exit"""

    def __init__(self, c, **kw):
        self.c, self.kw = c, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.c.set_option(k, v)

    def __exit__(self, *a):
        for k in self.kw:
            self.c.set_option(k, DEFAULTS[k])


def lay_of(hipmod, fid, table=None):
    nr, nf, dt = (table or P.FRAMES)[fid][0]
    return dict(n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16) if dt == "f16" else {}


def finish(c, got):
    cn = c.counters()
    got.update(route=c.route(), launches=cn.filter_kernel_launches, redo_pixels=cn.redo_pixels)
    return got


def classes_of(nbhd):
    return {class_of(int(n)) for n in np.asarray(nbhd).ravel()}


def assert_planted(got, fid, route, table=None):
    """the planted size at every target, printed with its class and the route"""
    _, _, pixels, targets = (P.frame if table is None else P.sampled_frame)(fid)
    sizes = [int(got["nbhd_size"][y, x]) for y, x in pixels]
    print("%s route %d: planted N / class %s" % (fid, route, " ".join("%d/%d" % (n, class_of(n)) for n in targets)))
    assert got["route"] == route and sizes == list(targets), (fid, route, got["route"], sizes, targets)


def assert_same_pass(a, b, keys=ALL):
    for k in keys:
        assert same_bits(a[k], b[k]), k
    assert (a["sum_nbhd"], a["max_nbhd"], a["launches"], a["redo_pixels"]) == (b["sum_nbhd"], b["max_nbhd"], b["launches"], b["redo_pixels"])


def assert_row_stage4(got, ref, colour_in, row, box, label, nmax=None, n_feat=12, form="expanded"):
    """every sample of the target row within the per-sample bar of the form its pixel's kernel uses (nmax: one bar for the row, from
    the pass's bound, on the sampled routes); ref: the restatement's stage 4 on the device's own stage outputs.  form: the form of
    the kernels of the resident classes (the compiled kernels, which this module runs: expanded; a layout-generic route: direct,
    the tighter bar).  Returns (worst distance, its bar), relative to cmax"""
    g, r, n = got["colour"][:, row], ref[:, row], got["nbhd_size"][row]
    assert np.array_equal(np.isnan(g), np.isnan(r))
    both = np.isfinite(g) & np.isfinite(r)
    dist = np.where(both, np.abs(g - r), 0.0).max(axis=(0, 2)) / B.cmax_of(colour_in)      # per pixel of the row
    bars = np.empty(n.shape)
    if nmax is not None:
        assert n.max() <= nmax <= B.RESIDENT
        bars[:] = B.sample_bar(form, n_feat, nmax, SIGMA, box)
    else:
        for fm, sel in ((form, n <= B.RESIDENT), ("direct", n > B.RESIDENT)):
            if sel.any():
                bars[sel] = B.sample_bar(fm, n_feat, int(n[sel].max()), SIGMA, box)
    worst = int(np.argmax(dist / bars))
    print("%s stage 4 on the target row: worst %.3e (bar %.3e) at x %d, N %d" % (label, dist[worst], bars[worst], worst, n[worst]))
    assert both.any() and (dist <= bars).all(), (float(dist[worst]), float(bars[worst]))
    moved = rel_l2(g, colour_in[:, row].astype(np.float64))            # the `moved` condition on the device's own row: the bar is not vacuous
    assert moved > 0.05, moved
    return float(dist[worst]), float(bars[worst])


# ---- (a) route 10 on the planted full-box frames -------------------------------------------------------------------------------------
def member_run(c, hipmod, fid, mt, fused=True, member=True, seed=SIGMA, **kw):
    """one pass of a full-box planted frame: under the membership test mt on route 10 (fused) or 9, or -- member False -- unflagged"""
    W, H, S, box = geometry(fid)
    if member:
        c.set_membership(hipmod.make_membership(mt[0].tolist(), mt[1].tolist()))
    flags = (hipmod.MEMBER_TEST_FLAG | (hipmod.MEMBER_FUSED_FLAG if fused else 0)) if member else 0
    desc = hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=seed, flags=flags, **lay_of(hipmod, fid), **kw)
    return finish(c, c.filter_pass_debug(P.frame(fid)[0], desc, box=box))


_r10 = {}


def route10(ctx, hipmod, fid, seed=SIGMA):
    """the route-10 pass of a frame under the reference's multiples and floors: run once, shared, never modified"""
    if (fid, seed) not in _r10:
        _r10[fid, seed] = member_run(ctx, hipmod, fid, MR.reference(layout(fid)[1]), seed=seed)
    return _r10[fid, seed]


@pytest.mark.parametrize("seed", [0.002, SIGMA], ids=["ref_seed", "active_seed"])
@pytest.mark.parametrize("fid", ROUTE10_FRAMES)
def test_route_10_reference_test_is_the_oracle_and_route_2(ctx, hipmod, oracle, fid, seed):
    got = route10(ctx, hipmod, fid, seed)
    assert got["status"] == hipmod.OK and got["redo_pixels"] == 0
    assert_planted(got, fid, 10)
    assert got["launches"] == len(classes_of(got["nbhd_size"]))          # one launch per non-empty class of the eleven
    assert_oracle_parity(got, P.oracle_pass(oracle, fid, EPS, seed), hipmod, fid)
    with options(ctx, binning=1):                                        # the anchor: the unflagged size-binned route, every plane
        want = member_run(ctx, hipmod, fid, None, member=False, seed=seed)
    assert want["route"] == 2
    assert_same_pass(got, want)
    if fid == "B40":
        assert got["max_nbhd"] > B.RESIDENT                              # 3137 and 3240: the streaming class behind route 10


@pytest.mark.parametrize("fid,option,value", [(f, "packed", 0) for f in ROUTE10_FRAMES] + [(f, "split_weights", 0) for f in ("B32", "B64")])
def test_route_10_options_agree(ctx, hipmod, fid, option, value):
    """tests/test_class_boundaries_gpu.py::test_routes_agree on route 10: every stage output bit for bit, the colours bit for bit
    (across packed 0 / 1: that test's rtol 1e-12)"""
    ref = route10(ctx, hipmod, fid)
    with options(ctx, **{option: value}):
        got = member_run(ctx, hipmod, fid, MR.reference(layout(fid)[1]))
    assert_planted(got, fid, 10)
    assert got["status"] == hipmod.OK
    for k in STAGE_KEYS:
        assert same_bits(got[k], ref[k]), k
    if option == "packed":
        np.testing.assert_allclose(got["colour"], ref["colour"], rtol=1e-12, atol=1e-300)
    else:
        assert same_bits(got["colour"], ref["colour"])


@pytest.mark.parametrize("fid", ROUTE10_FRAMES)
def test_route_10_under_another_test(ctx, hipmod, oracle, fid):
    """multiples that differ from feature to feature, every floor negative: the planted sizes stand, lists and statistics of the
    target row are the restatement's, the bin ids route 9's"""
    box = P.FRAMES[fid][2]
    b, mt = (box - 1) // 2, nonref(layout(fid)[1])
    want = member_row(oracle, fid, "nonref")
    got = member_run(ctx, hipmod, fid, mt)
    assert got["status"] == hipmod.OK and got["redo_pixels"] == 0
    assert_planted(got, fid, 10)
    assert got["launches"] == len(classes_of(got["nbhd_size"]))
    for k in FRONT:
        assert np.array_equal(got[k][b], want[k][b]), k
    r9 = member_run(ctx, hipmod, fid, mt, fused=False)
    assert r9["route"] == 9
    for k in BITS:
        assert same_bits(got[k], r9[k]), k


# ---- (b) the scheduled builds at the edges -------------------------------------------------------------------------------------------
def check_scheduled_row(oracle, hipmod, fid, base, got, routes, label, mt=None):
    """check_scheduled of tests/test_schedule_fused_gpu.py on a planted frame: the scheduled pass `got` against the gains-(1, 1)
    pass `base` of the same call, stage 3c against tests/schedule_ref.py on the device's own MI, stage 4 on the target row"""
    (gc, gf), box = GAINS[fid], P.FRAMES[fid][2]
    nr, nf = layout(fid)
    b = (box - 1) // 2
    assert got["status"] == hipmod.OK and got["route"] == base["route"] and got["route"] in routes, (got["route"], base["route"], routes)
    assert_planted(got, fid, got["route"])
    for k in ("launches", "redo_pixels", "sum_nbhd", "max_nbhd"):
        assert got[k] == base[k], k
    for k in SF.BITS:                                                    # stages 1 to 3b and W_r_c: the gains-(1, 1) run's bits
        assert SF.same(got[k], base[k]), k
    ac, ao = SRf.shares(got["mi"][b], gc, "c", 1e-10, nr, nf)
    bc, bo = SRf.shares(got["mi"][b], gf, "f", 1e-10, nr, nf)
    print("%s: route %d, %d launches, target row: alpha clamped / open %.3f / %.3f, beta factor %.3f / %.3f" % (
        label, got["route"], got["launches"], ac, ao, bc, bo))
    a1, b1, w1 = SRf.alpha_beta(base["mi"], 1.0, 1.0, 0, 1e-10, nr, nf)  # the control: gains (1, 1) is the unscheduled statement
    assert SF.same_or_nan(base["alpha"], a1) and SF.same_or_nan(base["beta"], b1) and SF.same_or_nan(base["wrc"], w1)
    a, bt, w = SRf.alpha_beta(got["mi"], gc, gf, 0, 1e-10, nr, nf)       # stage 3c on the device's own MI: bit for bit, every pixel
    assert SF.same_or_nan(got["alpha"], a) and SF.same_or_nan(got["beta"], bt) and SF.same_or_nan(got["wrc"], w)
    with np.errstate(invalid="ignore"):
        assert not (got["alpha"] < 0).any() and not (got["beta"] < 0).any()
    assert min(ac, ao) >= SHARE and min(bc, bo) >= SHARE, (ac, ao, bc, bo)
    assert not SF.same(got["alpha"], base["alpha"]) and not SF.same(got["beta"], base["beta"]) and (got["alpha"][b] == 0).any()
    assert not SF.same(got["colour"][:, b], base["colour"][:, b])
    p32 = P.frame(fid)[1]
    ref = SRf.stage4_on(oracle, p32, got, SIGMA, box, EPS, mt=mt, rows=[b], n_random=nr, n_feat=nf)
    assert_row_stage4(got, ref, p32[2:5], b, box, label, n_feat=nf)


SCHEDULED = [(f, how) for f in ROUTE10_FRAMES for how in (("default", "binning1") if geometry(f)[2] * geometry(f)[3] ** 2 <= 512 else ("default",))]
_sched = {}


@pytest.mark.parametrize("fid,how", SCHEDULED, ids=["%s-%s" % c for c in SCHEDULED])
def test_scheduled_builds_on_routes_0_to_2(ctx, hipmod, oracle, fid, how):
    _, _, S, box = geometry(fid)
    planes, lay = P.frame(fid)[0], lay_of(hipmod, fid)
    with options(ctx, **({} if how == "default" else dict(binning=1))):
        base = SF.run(ctx, hipmod, planes, box, (1.0, 1.0), lay=lay)
        got = SF.run(ctx, hipmod, planes, box, GAINS[fid], lay=lay)
    binned = how == "binning1" or box * box * S > 512
    check_scheduled_row(oracle, hipmod, fid, base, got, (2,) if binned else (0, 1), "%s, %s" % (fid, how))
    if binned:
        _sched[fid] = got


@pytest.mark.parametrize("fid", ROUTE10_FRAMES)
def test_scheduled_builds_on_route_10(ctx, hipmod, oracle, fid):
    box = geometry(fid)[3]
    planes, lay, mt = P.frame(fid)[0], lay_of(hipmod, fid), MR.reference(layout(fid)[1])
    base = SF.run(ctx, hipmod, planes, box, (1.0, 1.0), mt=mt, lay=lay)
    got = SF.run(ctx, hipmod, planes, box, GAINS[fid], mt=mt, lay=lay)
    check_scheduled_row(oracle, hipmod, fid, base, got, (10,), "%s, route 10" % fid, mt=mt)
    assert got["launches"] == len(classes_of(got["nbhd_size"]))
    assert_same_pass(base, route10(ctx, hipmod, fid))                    # gains (1, 1) with the entry's seed: the unscheduled pass
    if fid not in _sched:
        with options(ctx, binning=1):
            _sched[fid] = SF.run(ctx, hipmod, planes, box, GAINS[fid], lay=lay)
    assert _sched[fid]["route"] == 2
    assert_same_pass(got, _sched[fid])                                   # the anchor with gains: the scheduled route 2, every plane


# ---- (c) routes 11 and 12 on the sampled frames --------------------------------------------------------------------------------------
def sampled_run(c, hipmod, fid, mode, gains=None, **kw):
    """one pass of a sampled frame: mode "plain" route 8, "fused" route 11, "listed" route 12; gains: under RPF_FLAG_SCHEDULE |
    RPF_FLAG_SCHEDULE_FUSED with the entry (SIGMA, gains) -- the descriptor's own seed is then the reference's"""
    W, H, S, box, D, sseed = sampled_geometry(fid)
    c.set_sampling(hipmod.make_sampling(sseed, [D]))
    flags = (hipmod.SAMPLED_NBHD_FLAG | (hipmod.SAMPLED_FUSED_FLAG if mode == "fused" else 0) | (hipmod.SAMPLED_LISTED_FLAG if mode == "listed" else 0) |
             (hipmod.SAMPLED_REST_FLAG if S + D > 832 else 0))
    if gains is not None:
        c.set_schedule(hipmod.make_schedule(SIGMA, *gains))
        flags |= hipmod.SCHEDULE_FLAG | hipmod.SCHEDULE_FUSED_FLAG
    desc = hipmod.make_desc(W, H, S, policy=EPS, sigma_seed=SIGMA if gains is None else 0.002, flags=flags,
                            **lay_of(hipmod, fid, P.SAMPLED_FRAMES), **kw)
    return finish(c, c.filter_pass_debug(P.sampled_frame(fid)[0], desc, box=box))


_s12 = {}


def route12(ctx, hipmod, fid):
    """the route-12 pass of a sampled frame: run once, shared, never modified"""
    if fid not in _s12:
        _s12[fid] = sampled_run(ctx, hipmod, fid, "listed")
    return _s12[fid]


@pytest.mark.parametrize("fid", list(P.SAMPLED_FRAMES))
def test_routes_11_and_12_on_the_sampled_frames(ctx, hipmod, oracle, fid):
    W, H, S, box, D, sseed = sampled_geometry(fid)
    _, p32, pixels, targets = P.sampled_frame(fid)
    nr, nf = layout(fid, P.SAMPLED_FRAMES)
    b, nmax = (box - 1) // 2, min(box * box * S, S + D)
    want = sampled_row(oracle, fid)
    got = route12(ctx, hipmod, fid)
    r11 = sampled_run(ctx, hipmod, fid, "fused")
    nbhd11 = ctx.nbhd(W, H)
    for g, route in ((got, 12), (r11, 11)):
        assert g["status"] == hipmod.OK and g["redo_pixels"] == 0
        assert_planted(g, fid, route, P.SAMPLED_FRAMES)
        assert g["launches"] == len(classes_of(g["nbhd_size"])), (route, g["launches"], sorted(classes_of(g["nbhd_size"])))
        assert g["max_nbhd"] == g["nbhd_size"].max() <= nmax and g["sum_nbhd"] == int(g["nbhd_size"].sum())
        # the restatement on the target row
        for k in FRONT:
            assert np.array_equal(g[k][b], want[k][b]), (route, k)
    assert np.array_equal(nbhd11, r11["nbhd_size"]) and [int(nbhd11[y, x]) for y, x in pixels] == list(targets)
    np.testing.assert_allclose(got["mi"][b], want["mi"][b], rtol=0, atol=1e-11)      # the bars of tests/test_sampled_gpu.py
    for k in ("alpha", "beta", "wrc"):
        np.testing.assert_allclose(got[k][b], want[k][b], rtol=1e-9, atol=1e-12)
    ref = SR.stage4_on(oracle, p32, got, (sseed, 0, D), 0, box, SIGMA, EPS, rows=[b], n_random=nr, n_feat=nf)
    assert_row_stage4(got, ref, p32[2:5], b, box, "%s route 12" % fid, nmax=nmax, n_feat=nf)
    # route 11 against route 12: the same code behind the same list, every stage output and the colours on the whole frame
    assert_same_pass(got, r11)
    # route 8: the same call without the route's bit
    r8 = sampled_run(ctx, hipmod, fid, "plain")
    assert r8["route"] == 8
    for k in BITS:
        assert same_bits(got[k], r8[k]), k
    assert (got["sum_nbhd"], got["max_nbhd"]) == (r8["sum_nbhd"], r8["max_nbhd"])
    again = sampled_run(ctx, hipmod, fid, "listed")                      # ... and what the context reports after a route-12 pass
    assert np.array_equal(ctx.nbhd(W, H), again["nbhd_size"]) and same_bits(again["nbhd_size"], got["nbhd_size"])
    if fid == "SP32":
        assert S + D == 3136 and (box * box - 1) * S > 4096              # the cap; one-wave instantiations on route 11
    if fid in P.NMAX_FRAMES:   # the pixel whose list is as long as the pass allows has all of it, the last pool entry included
        full = [(y, x) for (y, x), n in zip(pixels, targets) if n == nmax]
        assert full
        for y, x in full:
            codes = want["codes"][(y, x)]
            assert len(codes) == nmax == got["nbhd_size"][y, x] == r11["nbhd_size"][y, x]
            assert got["member_hash"][y, x] == r11["member_hash"][y, x] == SR.fnv1a_u32(codes)
            assert got["member_hash"][y, x] != SR.fnv1a_u32(codes[:-1])
            print("%s: pixel (%d, %d) at N = S + D = nmax = %d (class %d) has its full list on routes 11 and 12" % (fid, y, x, nmax, class_of(nmax)))


@pytest.mark.parametrize("fid", list(P.SAMPLED_FRAMES))
def test_scheduled_listed_builds_on_the_sampled_frames(ctx, hipmod, oracle, fid):
    _, _, S, box, D, sseed = sampled_geometry(fid)
    nr, nf = layout(fid, P.SAMPLED_FRAMES)
    b, nmax = (box - 1) // 2, min(box * box * S, S + D)
    gc, gf = SAMPLED_GAINS[fid]
    p32 = P.sampled_frame(fid)[1]
    base = sampled_run(ctx, hipmod, fid, "listed", gains=(1.0, 1.0))
    got = sampled_run(ctx, hipmod, fid, "listed", gains=(gc, gf))
    r11 = sampled_run(ctx, hipmod, fid, "fused", gains=(gc, gf))
    for g in (base, got, r11):
        assert g["status"] == hipmod.OK and g["redo_pixels"] == 0
    assert_planted(base, fid, 12, P.SAMPLED_FRAMES)
    assert_planted(got, fid, 12, P.SAMPLED_FRAMES)
    assert_planted(r11, fid, 11, P.SAMPLED_FRAMES)
    assert_same_pass(got, r11)                                           # 11 equals 12 with gains
    assert_same_pass(base, route12(ctx, hipmod, fid))                    # gains (1, 1) with the entry's seed: the unscheduled pass
    for k in SF.BITS:
        assert SF.same(got[k], base[k]), k
    assert (got["launches"], got["sum_nbhd"], got["max_nbhd"]) == (base["launches"], base["sum_nbhd"], base["max_nbhd"])
    a, bt, w = SRf.alpha_beta(got["mi"], gc, gf, 0, 1e-10, nr, nf)       # stage 3c on the device's own MI: bit for bit, every pixel
    assert SF.same_or_nan(got["alpha"], a) and SF.same_or_nan(got["beta"], bt) and SF.same_or_nan(got["wrc"], w)
    ac, ao = SRf.shares(got["mi"][b], gc, "c", 1e-10, nr, nf)
    bc, bo = SRf.shares(got["mi"][b], gf, "f", 1e-10, nr, nf)
    print("%s scheduled, routes 12 and 11, target row: alpha clamped / open %.3f / %.3f, beta factor %.3f / %.3f" % (fid, ac, ao, bc, bo))
    assert min(ac, ao) >= SHARE and min(bc, bo) >= SHARE, (ac, ao, bc, bo)
    assert not SF.same(got["alpha"], base["alpha"]) and not SF.same(got["beta"], base["beta"])
    assert not SF.same(got["colour"][:, b], base["colour"][:, b])
    ref = SRf.stage4_on(oracle, p32, got, SIGMA, box, EPS, cfg=(sseed, 0, D), rows=[b], n_random=nr, n_feat=nf)
    assert_row_stage4(got, ref, p32[2:5], b, box, "%s scheduled route 12" % fid, nmax=nmax, n_feat=nf)


# ---- (d) a row slab that is the target row alone -------------------------------------------------------------------------------------
def assert_slab(part, full, pixels, targets, b, colour_in):
    for (y, x), n in zip(pixels, targets):
        assert y == b and part["nbhd_size"][y, x] == n
    for k in ("nbhd_size", "member_hash"):
        assert np.array_equal(part[k][b], full[k][b]), k
    assert same_bits(part["colour"][:, b], full["colour"][:, b])
    cin = colour_in.astype(np.float64)                                   # the halo rows pass through unfiltered
    assert np.array_equal(part["colour"][:, :b], cin[:, :b]) and np.array_equal(part["colour"][:, b + 1:], cin[:, b + 1:])


@pytest.mark.parametrize("fid", ["B16"])
def test_target_row_slab_on_route_10(ctx, hipmod, fid):
    b = (P.FRAMES[fid][2] - 1) // 2
    full = route10(ctx, hipmod, fid)
    with hipmod.Context(0) as c:
        part = member_run(c, hipmod, fid, MR.reference(layout(fid)[1]), row_begin=b, row_end=b + 1)
    assert part["route"] == 10
    assert_slab(part, full, P.frame(fid)[2], P.frame(fid)[3], b, P.frame(fid)[1][2:5])


@pytest.mark.parametrize("mode,route", [("fused", 11), ("listed", 12)])
@pytest.mark.parametrize("fid", ["SP8", "NM64"])
def test_target_row_slab_on_the_sampled_routes(ctx, hipmod, fid, mode, route):
    b = (P.SAMPLED_FRAMES[fid][2] - 1) // 2
    full = route12(ctx, hipmod, fid)                                     # (route 11 gives the same bits: group (c))
    with hipmod.Context(0) as c:
        part = sampled_run(c, hipmod, fid, mode, row_begin=b, row_end=b + 1)
    assert part["route"] == route
    assert_slab(part, full, P.sampled_frame(fid)[2], P.sampled_frame(fid)[3], b, P.sampled_frame(fid)[1][2:5])


# ---- REF_ABORT is refused on each of the routes ---------------------------------------------------------------------------------------
def test_ref_abort_is_refused_on_routes_10_11_and_12(ctx, hipmod):
    W, H, S, box = geometry("U8")
    mt = MR.reference()
    ctx.set_membership(hipmod.make_membership(mt[0].tolist(), mt[1].tolist()))
    ctx.set_sampling(hipmod.make_sampling(P.SAMPLING_SEED, [24]))
    for flags in (hipmod.MEMBER_TEST_FLAG | hipmod.MEMBER_FUSED_FLAG, hipmod.SAMPLED_NBHD_FLAG | hipmod.SAMPLED_FUSED_FLAG,
                  hipmod.SAMPLED_NBHD_FLAG | hipmod.SAMPLED_LISTED_FLAG):
        with pytest.raises(hipmod.RpfError) as e:
            ctx.filter_pass_debug(P.frame("U8")[0], hipmod.make_desc(W, H, S, policy=REF_ABORT, flags=flags), box=box)
        assert e.value.status == hipmod.E_UNSUPPORTED and "REF_ABORT" in str(e.value)
