"""RPF_FLAG_FAST_WEIGHTS on every kernel class and entry point: the fp32 pair-weight mode selects its own instantiations
filter_pixel_kernel<K, T_IN_LDS, FAST = true, NW> and its own host routing (no packed kernels, no split route); the frames of
tests/planted_nbhd.py put a neighbourhood at and one above every class edge in front of each of them.

Bars (none of its own beyond these):
  contract    FAST colours against the oracle <= REL_L2_BAR (1e-4, include/rpf_hip.h) over the whole frame, wherever the
              oracle is finite.
  regression  on the check set (every pixel of the target row): g = rel-L2 of the device's FAST colours against the oracle,
              e32 = the same for the CPU restatement of the documented fp32 arithmetic (tests/fast_weights_ref.py;
              tests/test_fast_weights_cpu.py holds e32 to (0, 1e-6] at the active seed): g <= 16 * e32 + 1e-12.
              1e-12 is the suite's route-agreement rounding bar: at the reference's seed the filter is the identity on these
              frames, e32 is exactly 0 and the device must be exact to rounding as well.  16: the device forms exp as
              v_exp_f32 of a product with log2(e) rounded in fp32, which adds about E * 2^-24 to a weight's relative error
              where numpy's expf adds 2^-24, and it multiplies by 1 / SD where the restatement divides; for the weights that
              carry the sums (E of order 1 to 10) that is up to an order of magnitude on one of several error terms.
  discrete    every stage output (STAGE_KEYS) of a FAST run is BIT-equal to the fp64 run's: the flag changes stage 4 only.
  options     FAST runs under different route options: stage outputs, status and NaN pattern bit-equal, finite colours to
              rtol 1e-12 (the same fp32 weights, the fp64 sums possibly in another order).

Which instantiation (K, T_IN_LDS, NW) each case of test_every_fast_instantiation reaches.  K is the class's samples per
lane (N <= 64: 1 | 128: 2 | 256: 4 | 448: 7 | 832: 13 | 1600: 25 | 3136: 49; an unbinned frame runs one kernel for
box * box * S), NW = 4 from K = 25 up unless the window holds more than 4096 candidates (box 17), T_IN_LDS by default 0 on one
wave and, on four waves, 1 where the table costs no resident workgroup (rpf_kernels.hip table_in_lds):

  U8   table_in_lds t = 0 | 1        unbinned, 392 candidates: (7, t, 1)
  U3   table_in_lds t = 0 | 1        unbinned, 507 candidates: (13, t, 1)
  B16  table_in_lds t = 0 | 1        N = 16 ... 784: (1, t, 1) (2, t, 1) (4, t, 1) (7, t, 1) (13, t, 1)
  B32  table_in_lds t = 0 | 1        N = 300 ... 1568: (7, t, 1) (13, t, 1) (25, t, 4); by default (25, 1, 4)
  B64  table_in_lds t = 0 | 1        N = 580 ... 3136: (13, t, 1) (25, t, 4) (49, t, 4); by default (25, 0, 4) (49, 1, 4)
  B17  table_in_lds t = 0 | 1        a window of 4608 candidates, one wave throughout: (7, t, 1) (13, t, 1) (25, t, 1) (49, t, 1)
  B16  waves_per_pixel 4             (13, 1, 4): the table fits beside two resident workgroups
  B16  waves_per_pixel 4 + table_in_lds 0      (13, 0, 4) -- the one instantiation no single option reaches
  B32  waves_per_pixel 1             (25, 0, 1)
  B64  waves_per_pixel 1             (25, 0, 1) (49, 0, 1)
  U8   binning 1                     the unbinned-size frame through the class lists (N = 8 ... 187): (1, 0, 1) (2, 0, 1) (4, 0, 1)
  B32, B64  split_weights 0          a no-op: FAST never splits, though the hand-over buffer of the split route is allocated

Together: K in {1, 2, 4, 7} x T_IN_LDS in {0, 1} on one wave (8), K in {13, 25, 49} x {0, 1} x NW in {1, 4} (12): all
twenty.  No combination of the list is refused for LDS: the largest, K = 49 on four waves at 64 spp with the table, takes
rpf_lds_bytes_required(64, 7) = 150784 bytes (125696 + the table's 25088) of the 163840 a workgroup may have
(test_largest_fast_working_set_fits holds that figure); nothing is skipped.

Measured on the MI355X, active seed (DESIGN.md section 4 has the table): g / e32 = 0.68 ... 1.07 over the nine frames and both
policies (g = 5.1e-9 ... 1.28e-8), the whole-frame distance from the oracle at most 1.3e-8; at the reference's seed g = 0.
Across the route options of test_every_fast_instantiation no colour differed from the default-options FAST run."""
import numpy as np
import pytest

import fast_weights_ref as R
import planted_nbhd as P
from test_class_boundaries_gpu import assert_oracle_parity, base, geometry, hip_desc, moved, run
from test_gpu_parity import (INF_INJECTIONS, REL_L2_BAR, STAGE_KEYS, _assert_ref_abort_parity, _independent_columns,
                             _inject_inf, rel_l2)
from raytracer_rpf_amd import feature_buffer as fb

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
SEEDS = pytest.mark.parametrize("seed", [0.002, P.ACTIVE_SIGMA_SEED], ids=["ref_seed", "active_seed"])
POLICIES = pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
FRAMES19 = [f for f, v in P.FRAMES.items() if v[0] == (2, 12, "f32")]
BINNED = [f for f in FRAMES19 if P.FRAMES[f][5]]
MAX_RESIDENT = P.CAPACITIES[-1]         # neighbourhoods above it stream through the fp64 generic kernel, FAST or not
REGRESSION_FACTOR = 16

_fast = {}


def fast(ctx, hipmod, fid, policy, seed):
    """the FAST default-options pass of a frame on the session context: run once, shared, never modified"""
    if (fid, policy, seed) not in _fast:
        _fast[fid, policy, seed] = run(ctx, hipmod, fid, policy, seed, flags=hipmod.FLAG_FAST_WEIGHTS)
    return _fast[fid, policy, seed]


def samples_per_lane(fid, n, binned):
    """K of the kernel that filters a pixel of neighbourhood size n (0: the streaming kernel)"""
    W, H, S, box = geometry(fid)
    nmax = box * box * S
    if binned:
        if n > MAX_RESIDENT:
            return 0
        nmax = min(nmax, min(c for c in P.CAPACITIES if n <= c))
    return min(k for k in (1, 2, 4, 7, 13, 25, 49) if (nmax + 63) // 64 <= k)


# ---- (a) every class edge under FAST ------------------------------------------------------------------------------------------
@SEEDS
@POLICIES
@pytest.mark.parametrize("fid", FRAMES19)
def test_every_class_edge_under_fast(ctx, hipmod, oracle, fid, policy, seed):
    want = P.oracle_pass(oracle, fid, policy, seed)
    ref = base(ctx, hipmod, fid, policy, seed)
    got = fast(ctx, hipmod, fid, policy, seed)
    assert got["route"] == 2 if fid in BINNED else got["route"] in (0, 1)
    for k in STAGE_KEYS:        # the flag changes stage 4 alone: everything up to alpha, beta, W_r_c is the fp64 run's bits
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
    assert got["redo_pixels"] == ref["redo_pixels"]
    assert_oracle_parity(got, want, hipmod, fid)            # planted sizes, status, NaN pattern, counters, the contract
    # the regression bar on the check set
    b = (geometry(fid)[3] - 1) // 2
    fin = np.isfinite(want["colour"][:, b])
    g = rel_l2(got["colour"][:, b][fin], want["colour"][:, b][fin])
    e32 = R.row_distance(oracle, fid, policy, seed, np.float32)
    print("FAST %s policy %d seed %g: g = %.3e  e32 = %.3e  g / e32 = %s  whole frame %.3e" % (
        fid, policy, seed, g, e32, "%.2f" % (g / e32) if e32 > 0 else "-",
        rel_l2(got["colour"][np.isfinite(want["colour"])], want["colour"][np.isfinite(want["colour"])])))
    assert g <= REGRESSION_FACTOR * e32 + 1e-12, (g, e32)
    if seed == P.ACTIVE_SIGMA_SEED:
        assert moved(oracle, fid, seed) > 0.05              # none of the colour bars is vacuous
    # neighbourhoods above 3136 samples stay on the fp64 streaming kernel: the fp64 run's colours, to rounding
    big = want["nbhd_size"] > MAX_RESIDENT
    assert big.any() == (fid in ("B40", "B17"))
    if big.any():
        m = np.isfinite(want["colour"][:, big])
        assert rel_l2(got["colour"][:, big][m], want["colour"][:, big][m]) <= REL_L2_BAR
        np.testing.assert_allclose(got["colour"][:, big][m], ref["colour"][:, big][m], rtol=1e-12, atol=1e-300)


# ---- (b) every FAST instantiation ----------------------------------------------------------------------------------------------
# frame, options, the K classes the case must populate (see the module docstring for T_IN_LDS and NW)
INSTANTIATIONS = ([("U8", (("table_in_lds", v),), (7,)) for v in (0, 1)]
                  + [("U3", (("table_in_lds", v),), (13,)) for v in (0, 1)]
                  + [("B16", (("table_in_lds", v),), (1, 2, 4, 7, 13)) for v in (0, 1)]
                  + [("B32", (("table_in_lds", v),), (13, 25)) for v in (0, 1)]
                  + [("B64", (("table_in_lds", v),), (25, 49)) for v in (0, 1)]
                  + [("B17", (("table_in_lds", v),), (13, 25, 49)) for v in (0, 1)]
                  + [("B16", (("waves_per_pixel", 4),), (13,)),
                     ("B16", (("waves_per_pixel", 4), ("table_in_lds", 0)), (13,)),
                     ("B32", (("waves_per_pixel", 1),), (25,)),
                     ("B64", (("waves_per_pixel", 1),), (25, 49)),
                     ("U8", (("binning", 1),), (1, 2, 4)),
                     ("B32", (("split_weights", 0),), (25,)),
                     ("B64", (("split_weights", 0),), (25, 49))])


def test_largest_fast_working_set_fits(hipmod):
    """K = 49 on four waves at 64 spp, the D table in LDS (B64, table_in_lds 1 -- also that class's default): the figure the
    module docstring quotes, inside the 160 KiB of a workgroup, so that no case of INSTANTIATIONS is refused for LDS"""
    assert hipmod.lds_bytes_required(64, 7) == 150784 <= 160 * 1024


@SEEDS
@pytest.mark.parametrize("fid,options,classes", INSTANTIATIONS,
                         ids=["%s-%s" % (f, "+".join("%s%d" % o for o in opts)) for f, opts, _ in INSTANTIATIONS])
def test_every_fast_instantiation(ctx, hipmod, fid, options, classes, seed):
    """a fresh context per option set (nothing leaks) against the FAST default-options run of the session context"""
    binned = fid in BINNED or ("binning", 1) in options
    for policy in (EPS, REF_ABORT):
        ref = fast(ctx, hipmod, fid, policy, seed)
        with hipmod.Context(0) as c:
            for name, value in options:
                c.set_option(name, value)
            got = run(c, hipmod, fid, policy, seed, flags=hipmod.FLAG_FAST_WEIGHTS)
            assert c.counters().options_active == 1
        assert got["route"] == 2 if binned else got["route"] in (0, 1)
        reached = {samples_per_lane(fid, int(n), binned) for n in np.unique(got["nbhd_size"])}
        assert set(classes) <= reached, (classes, reached)
        for k in STAGE_KEYS:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (policy, k)
        assert got["status"] == ref["status"] and got["nonfinite_pixels"] == ref["nonfinite_pixels"]
        assert got["first_bad_pixel"] == ref["first_bad_pixel"] and got["redo_pixels"] == ref["redo_pixels"]
        assert np.array_equal(np.isnan(got["colour"]), np.isnan(ref["colour"]))
        m = np.isfinite(ref["colour"])
        a, b = got["colour"][m], ref["colour"][m]
        print("FAST %s %s policy %d seed %g: %d of %d colours differ, max relative %.3e" % (
            fid, options, policy, seed, int((a != b).sum()), a.size,
            float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300), initial=0.0))))
        if options == (("split_weights", 0),):
            assert np.array_equal(a, b), policy             # FAST never splits: the very same launches
        else:
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-300)


# ---- (c) non-finite inputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", INF_INJECTIONS)
@pytest.mark.parametrize("mode,flat", [("smooth", 0.5), ("clustered", 0.0)])
def test_infinite_features_under_fast(ctx, hipmod, oracle, mode, flat, kind):
    """the 19-dim buffer and the injections of test_infinite_features_vs_oracle, both policies"""
    W, H, S = 16, 12, 8
    sf, sc = (0.05, 1e-4) if mode == "smooth" else (1e-3, 0.01)
    planes = fb.synth_planes(W, H, S, seed=61, sigma_f=sf, sigma_c=sc, mode=mode, flat_frac=flat)
    _inject_inf(planes, 19, kind)
    for policy in (EPS, REF_ABORT):
        want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7, policy=policy))
        got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=policy, flags=hipmod.FLAG_FAST_WEIGHTS), box=7,
                                    allow_nonfinite=True)
        assert np.array_equal(got["nbhd_size"], want["nbhd_size"]), policy
        assert np.array_equal(got["member_hash"], want["member_hash"]), policy
        assert (got["status"] == hipmod.E_NONFINITE) == (want["status"] == 1), policy
        assert got["nonfinite_pixels"] == want["nonfinite_pixels"], policy
        assert got["first_bad_pixel"] == want["first_bad_pixel"], policy
        assert np.array_equal(np.isnan(got["colour"]), np.isnan(want["colour"])), policy
        fin = np.isfinite(want["colour"])
        assert rel_l2(got["colour"][fin], want["colour"][fin]) <= REL_L2_BAR, policy


# ---- (d) the redo path -----------------------------------------------------------------------------------------------------------
def one_pixel_independent(oracle, S, bins):
    """the buffer of test_exactly_independent_table_at_non_power_of_two_n: one pixel, two exactly independent column pairs"""
    a, b = _independent_columns(S, bins)
    rng = np.random.default_rng(3)
    planes = np.empty((19, 1, 1, S), np.float32)
    for c in range(19):
        planes[c, 0, 0] = rng.permutation(S) / (S - 1.0)
    planes[5, 0, 0], planes[6, 0, 0] = a, b
    planes[7, 0, 0], planes[8, 0, 0] = b, a
    pa, pb = oracle.pair_table()
    return planes, [i for i in range(96) if (pa[i], pb[i]) in ((7, 5), (8, 6))]


def every_pixel_independent(oracle):
    """the 11 x 11 x 15 frame, box 9, of test_independent_tables_in_every_size_class_ref_abort: an exactly independent
    (f0, r0) table at a non-power-of-two N in EVERY pixel"""
    W, H, S = 11, 11, 15
    rng = np.random.default_rng(17)
    planes = rng.permuted(np.broadcast_to(np.linspace(0.4, 0.6, S), (19, H, W, S)), axis=3).astype(np.float32)
    planes[0] = (np.arange(W)[None, :, None] + rng.random((H, W, S))).astype(np.float32)
    planes[1] = (np.arange(H)[:, None, None] + rng.random((H, W, S))).astype(np.float32)
    a, b = _independent_columns(S, 3)
    planes[5], planes[7] = a.astype(np.float32), b.astype(np.float32)
    pa, pb = oracle.pair_table()
    return planes, [i for i in range(96) if (pa[i], pb[i]) == (7, 5)]


@pytest.mark.parametrize("S,bins", [(15, 3), (12, 3), (24, 4)])
def test_fast_keeps_the_redo_list_one_pixel(ctx, hipmod, oracle, S, bins):
    """REF_ABORT promises the reference's own MI residue, alpha, beta and W_r_c; the flag leaves "everything that decides
    discrete outcomes (membership, bins, MI)" unchanged: the redo pixel is handed to the reference-expression kernel under
    FAST as well (and filtered there whole, in fp64)"""
    planes, indep = one_pixel_independent(oracle, S, bins)
    ref = oracle.filter_pass(planes, oracle.make_desc(1, 1, S, box=7))
    assert (np.abs(ref["mi"][0, 0, indep]) < 1e-15).all()
    plain = ctx.filter_pass_debug(planes, hipmod.make_desc(1, 1, S), box=7, allow_nonfinite=True)
    assert ctx.counters().redo_pixels == 1
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(1, 1, S, flags=hipmod.FLAG_FAST_WEIGHTS), box=7, allow_nonfinite=True)
    assert ctx.counters().redo_pixels == 1
    _assert_ref_abort_parity(got, ref, hipmod, indep)
    for k in STAGE_KEYS:
        assert np.array_equal(got[k], plain[k], equal_nan=True), k


def test_fast_keeps_the_redo_list_every_size_class(ctx, hipmod, oracle):
    planes, indep = every_pixel_independent(oracle)
    W, H, S, box = 11, 11, 15, 9
    ref = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box))
    ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S), box=box, allow_nonfinite=True)
    assert ctx.counters().redo_pixels == W * H
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, flags=hipmod.FLAG_FAST_WEIGHTS), box=box, allow_nonfinite=True)
    assert ctx.counters().redo_pixels == W * H
    _assert_ref_abort_parity(got, ref, hipmod, indep)


def test_redo_count_does_not_outlive_its_call(ctx, hipmod, oracle):
    """one context: an fp64 REF_ABORT call that redoes 121 pixels, then FAST calls on a frame that redoes none"""
    planes, _ = every_pixel_independent(oracle)
    seed = P.ACTIVE_SIGMA_SEED
    fid = next(f for f in ("U8", "U12", "B16") if base(ctx, hipmod, f, REF_ABORT, seed)["redo_pixels"] == 0)
    with hipmod.Context(0) as c:
        c.filter_pass_debug(planes, hipmod.make_desc(11, 11, 15), box=9, allow_nonfinite=True)
        assert c.counters().redo_pixels == 121
        assert run(c, hipmod, fid, REF_ABORT, seed, flags=hipmod.FLAG_FAST_WEIGHTS)["redo_pixels"] == 0
        assert run(c, hipmod, fid, EPS, seed, flags=hipmod.FLAG_FAST_WEIGHTS)["redo_pixels"] == 0


# ---- (e) entry points ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", ["U8", "B16"])
def test_filter_entries_under_fast(ctx, hipmod, oracle, fid):
    W, H, S, box = geometry(fid)
    seed, F = P.ACTIVE_SIGMA_SEED, hipmod.FLAG_FAST_WEIGHTS
    planes, p32 = P.frame(fid)[0], P.frame(fid)[1]
    rw = (0.5 + np.random.default_rng(7).random((H, W, S))).astype(np.float32)
    # rpf_filter, boxes (7, 5): two chained debug passes, the second fed the doubles the first left
    one = hip_desc(hipmod, fid, EPS, sigma_seed=seed, flags=F)
    p1 = ctx.filter_pass_debug(planes, one, box=7, debug=False)["colour"]
    assert np.array_equal(p1, fast(ctx, hipmod, fid, EPS, seed)["colour"])
    p2 = ctx.filter_pass_debug(planes, one, box=5, colour_in=p1, debug=False)["colour"]
    with hipmod.Context(0) as c:
        srgb, prgb, st = c.filter(planes, hip_desc(hipmod, fid, EPS, boxes=(7, 5), sigma_seed=seed, flags=F), ray_weight=rw)
        assert st == hipmod.OK
    assert np.array_equal(srgb, p2.astype(np.float32))
    w1 = P.oracle_pass(oracle, fid, EPS, seed)["colour"]
    w2 = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=5, policy=EPS, sigma_seed=seed), colour_in=w1, debug=False)["colour"]
    assert rel_l2(srgb.astype(np.float64), w2) <= REL_L2_BAR
    assert rel_l2(prgb.astype(np.float64), oracle.pixel_mean(w2, oracle.make_desc(W, H, S), rw)) <= REL_L2_BAR
    # rpf_multi_filter on two slabs of device 0 against the one-context call
    d7 = hip_desc(hipmod, fid, EPS, boxes=(7,), sigma_seed=seed, flags=F)
    with hipmod.Context(0) as c:
        s1, q1, st1 = c.filter(planes, d7, ray_weight=rw)
    with hipmod.MultiContext([0, 0]) as mc:
        s2, q2, st2 = mc.filter(planes, d7, ray_weight=rw)
    assert st1 == st2 == hipmod.OK
    assert np.array_equal(s1, p1.astype(np.float32))
    assert np.array_equal(s2, s1) and np.array_equal(q2, q1)
    # a row slab that is the target row alone
    b = (box - 1) // 2
    full = fast(ctx, hipmod, fid, EPS, seed)
    with hipmod.Context(0) as c:
        part = run(c, hipmod, fid, EPS, seed, flags=F, row_begin=b, row_end=b + 1)
    for k in ("nbhd_size", "member_hash"):
        assert np.array_equal(part[k][b], full[k][b]), k
    assert np.array_equal(part["colour"][:, b], full["colour"][:, b])
    cin = p32[2:5].astype(np.float64)
    assert np.array_equal(part["colour"][:, :b], cin[:, :b]) and np.array_equal(part["colour"][:, b + 1:], cin[:, b + 1:])


# ---- (f) refusals ------------------------------------------------------------------------------------------------------------------
def test_fast_refused_on_the_27_dim_layout(ctx, hipmod):
    """no fp32 instantiation of the 27-dim kernels exists: every filter entry point answers RPF_E_UNSUPPORTED, naming the
    flag, before any device work (rpf_layout_kernels), and the context filters on as if nothing had happened"""
    fid = "H8"
    W, H, S, box = geometry(fid)
    planes = P.frame(fid)[0]
    F = hipmod.FLAG_FAST_WEIGHTS
    desc = hip_desc(hipmod, fid, EPS, flags=F)
    assert hipmod.layout_kernels(desc) == (hipmod.E_UNSUPPORTED, None)
    film = hipmod.make_film(((0, 0), (W, H)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX))

    def refused(call):
        with pytest.raises(hipmod.RpfError) as e:
            call()
        assert e.value.status == hipmod.E_UNSUPPORTED, str(e.value)
        assert "RPF_FLAG_FAST_WEIGHTS" in str(e.value), str(e.value)

    u8 = base(ctx, hipmod, "U8", EPS, P.ACTIVE_SIGMA_SEED)
    with hipmod.Context(0) as c:
        refused(lambda: c.filter(planes, desc))
        refused(lambda: c.filter_pass_debug(planes, desc, box=box))
        refused(lambda: c.filter_film(planes, desc, film))
        again = run(c, hipmod, "U8", EPS, P.ACTIVE_SIGMA_SEED)
        for k in STAGE_KEYS + ("colour",):
            assert np.array_equal(again[k], u8[k], equal_nan=True), k
        d8 = hip_desc(hipmod, "U8", EPS, boxes=(7,), sigma_seed=P.ACTIVE_SIGMA_SEED)
        s1, q1, _ = c.filter(P.frame("U8")[0], d8)
    with hipmod.MultiContext([0, 0]) as mc:
        refused(lambda: mc.filter(planes, desc))
        s2, q2, st = mc.filter(P.frame("U8")[0], d8)
        assert st == hipmod.OK
    assert np.array_equal(s1, u8["colour"].astype(np.float32))
    assert np.array_equal(s2, s1) and np.array_equal(q2, q1)
