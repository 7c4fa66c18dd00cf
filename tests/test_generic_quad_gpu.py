"""GPU tests of the four-wave generic route (RPF_FLAG_GENERIC | RPF_FLAG_GENERIC_PACKED | RPF_FLAG_GENERIC_WAVE |
RPF_FLAG_GENERIC_QUAD, rpf_query_route 13): neighbourhoods of 832 < N <= 3136 samples on
generic::filter_quad_kernel (classes 1600 and 3136, where the layout's carve-up fits them), N <= 832 as on route 5, the rest on
generic::filter_pixel_kernel.  Every frame's input conditions are asserted against the oracle on the CPU by
tests/test_generic_quad_cpu.py.  "Route 3" below is the same context and buffer with RPF_FLAG_GENERIC alone, "route 5" the same
without the new flag.  No tolerance is new: check_pass's bars, _assert_ref_abort_parity, REL_L2_BAR, the direct form's per-sample
bar of tests/stage4_bars.py, or bit equality."""
import numpy as np
import pytest

import fast_weights_ref as R
import pass_report_ref as PR
import pbrt_film_ref as FR
import planted_nbhd as P
import stage4_bars as B
from test_film_gpu import film_device
from test_generic_layout_gpu import buffers
from test_generic_quad_cpu import (DEFAULT_LAY, FRAMES, INF_SHAPE, LAYOUTS, NO_3136, RESIDUE_BOX, RESIDUE_LAY, SCHED_LAY, class_counts,
                                   frame, frame_oracle, geometry, inf_frame, residue_big_frame, residue_frame, residue_oracle)
from test_generic_wave_cpu import lay_ids
from test_generic_wave_gpu import bits_equal, check_pass_or_nan_pattern, run_debug
from test_gpu_parity import INF_INJECTIONS, REL_L2_BAR, STAGE_KEYS, _assert_ref_abort_parity, check_pass, rel_l2
from test_schedule_gpu import check_scheduled, run as sched_run
from test_stage4_per_sample_cpu import at

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
POLICIES = pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
DISCRETE_AND_STATS = ("nbhd_size", "member_hash", "bin_hash", "mean", "stddev")
ROUTE_QUAD = 13


def flags_of(hipmod, route):
    """route 13: G | P | W | Q; 5: G | P | W; 3: G"""
    g, p, w = hipmod.FLAG_GENERIC, hipmod.FLAG_GENERIC_PACKED, hipmod.FLAG_GENERIC_WAVE
    return {13: g | p | w | hipmod.GENERIC_QUAD_FLAG, 5: g | p | w, 3: g}[route]


def desc_for(hipmod, lay, W, H, S, route=ROUTE_QUAD, **kw):
    nr, nf, dt = lay
    return hipmod.make_desc(W, H, S, n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16 if dt == "f16" else hipmod.PLANES_F32,
                            flags=kw.pop("flags", 0) | flags_of(hipmod, route), **kw)


def quad_classes(hipmod, lay):
    """the classes route 13 deals a layout: ten, or as many as its carve-up fits"""
    d = desc_for(hipmod, lay, 8, 8, 4)
    return 8 + sum(1 for cap in (1600, 3136) if hipmod.generic_quad_carve(d, cap)[0] == hipmod.OK)


def expected_launches(hipmod, lay, n, policy):
    """one per non-empty class list, one for the rest list, the redo launch"""
    return sum(1 for k in class_counts(n, quad_classes(hipmod, lay)) if k) + (1 if policy == REF_ABORT else 0)


_got = {}


def frame_run(ctx, hipmod, fid, lay, policy, sigma_seed=0.002, route=ROUTE_QUAD):
    """a pass over a planted frame: run once per variant, shared, never modified"""
    key = (fid, lay, policy, sigma_seed, route)
    if key not in _got:
        W, H, S, box = geometry(fid)
        _got[key] = run_debug(ctx, frame(fid, lay)[0], desc_for(hipmod, lay, W, H, S, route=route, policy=policy, sigma_seed=sigma_seed), box)
    return _got[key]


# ---- 1. the class edges at 40 spp under box 9 --------------------------------------------------------------------------------------
@POLICIES
@pytest.mark.parametrize("lay", LAYOUTS, ids=lay_ids)
def test_q40_vs_oracle_and_route3(ctx, hipmod, oracle, lay, policy):
    want = frame_oracle(oracle, "Q40", lay, policy)
    got = frame_run(ctx, hipmod, "Q40", lay, policy)
    assert got["route"] == ROUTE_QUAD and got["status"] == hipmod.OK
    assert got["launches"] == expected_launches(hipmod, lay, want["nbhd_size"], policy)
    for (y, x), n in zip(frame("Q40", lay)[2], FRAMES["Q40"][2]):
        assert got["nbhd_size"][y, x] == n
    check_pass(got, want)
    r3 = frame_run(ctx, hipmod, "Q40", lay, policy, route=3)
    assert r3["route"] == 3 and r3["launches"] == 1
    bits_equal(got, r3, DISCRETE_AND_STATS)
    if policy == EPS:
        bits_equal(got, r3, ("mi", "alpha", "beta", "wrc"))   # the same integers, the same statements
        assert got["redo_pixels"] == 0


def test_q40_layout_without_the_3136_class(ctx, hipmod, oracle):
    """(17, 18, f32), 40 dims: the carve-up fits 1600 and not 3136, so the targets 1601 ... 3240 are the rest list's"""
    lay = NO_3136
    assert quad_classes(hipmod, lay) == 9
    want = frame_oracle(oracle, "Q40", lay, EPS)
    got = frame_run(ctx, hipmod, "Q40", lay, EPS)
    assert got["route"] == ROUTE_QUAD and got["status"] == hipmod.OK
    cc = class_counts(want["nbhd_size"], 9)
    assert cc[8] > 0 and cc[9] > 0
    assert got["launches"] == sum(1 for k in cc if k)
    for (y, x), n in zip(frame("Q40", lay)[2], FRAMES["Q40"][2]):
        assert got["nbhd_size"][y, x] == n
    check_pass(got, want)
    r3 = frame_run(ctx, hipmod, "Q40", lay, EPS, route=3)
    bits_equal(got, r3, STAGE_KEYS)
    rest = want["nbhd_size"] > 1600                             # ... on the kernel of route 3: its colours too
    assert got["colour"][:, rest].tobytes() == r3["colour"][:, rest].tobytes()


# ---- 2. without the flag nothing changes; with it, only the pixels of the new classes do ---------------------------------------
@pytest.mark.parametrize("fid,lay", [("Q40", (3, 7, "f32")), ("Q40", (4, 18, "f16")), ("Q32", DEFAULT_LAY), ("Q64", DEFAULT_LAY)],
                         ids=lambda v: lay_ids(v) if isinstance(v, tuple) else v)
def test_unflagged_call_is_route_5_and_the_other_pixels_keep_its_bits(ctx, hipmod, oracle, fid, lay):
    W, H, S, box = geometry(fid)
    quad = frame_run(ctx, hipmod, fid, lay, EPS)                 # a flagged call first: it leaves nothing behind
    d5 = desc_for(hipmod, lay, W, H, S, route=5, policy=EPS, sigma_seed=0.002)
    r5 = run_debug(ctx, frame(fid, lay)[0], d5, box)
    with hipmod.Context(0) as fresh:
        f5 = run_debug(fresh, frame(fid, lay)[0], d5, box)
    assert r5["route"] == f5["route"] == 5 and r5["launches"] == f5["launches"] and r5["redo_pixels"] == f5["redo_pixels"] == 0
    n = r5["nbhd_size"]
    assert r5["launches"] == sum(1 for k in class_counts(n, 8) if k)
    bits_equal(r5, f5, STAGE_KEYS + ("colour",))
    # the flagged call: every stage output is route 5's on every pixel, the colours on every pixel the new classes do not take
    assert quad["route"] == ROUTE_QUAD
    bits_equal(quad, r5, STAGE_KEYS)
    others = (n <= 832) | (n > 3136)
    assert others.any() and (~others).any()
    assert quad["colour"][:, others].tobytes() == r5["colour"][:, others].tobytes()
    assert rel_l2(quad["colour"], r5["colour"]) <= REL_L2_BAR


# ---- 3. weights of order one: every sample of the target row within the direct form's bar ---------------------------------------
@pytest.mark.parametrize("fid", ["Q32", "Q64"])
def test_active_seed_stage4_per_sample(ctx, hipmod, oracle, fid):
    """tests/test_stage4_per_sample_gpu.py's assertion on route 13: the colours against the fp64 restatement of
    tests/fast_weights_ref.py evaluated on the device's own stage outputs, every finite sample of the target row within
    stage4_bars.sample_bar("direct", ...) at the largest neighbourhood of the row"""
    lay, seed = DEFAULT_LAY, P.ACTIVE_SIGMA_SEED
    W, H, S, box = geometry(fid)
    want = frame_oracle(oracle, fid, lay, EPS, seed)
    got = frame_run(ctx, hipmod, fid, lay, EPS, seed)
    assert got["route"] == ROUTE_QUAD and got["status"] == hipmod.OK
    assert got["launches"] == expected_launches(hipmod, lay, want["nbhd_size"], EPS)
    check_pass(got, want)
    stored, p32, _ = frame(fid, lay)
    b = (box - 1) // 2
    pixels = [(b, x) for x in range(W)]
    ref = R.stage4(oracle, p32, got, box, seed, pixels, np.float64, EPS, lay[0], lay[1])
    mine = at(got["colour"], pixels)
    assert np.array_equal(np.isnan(mine), np.isnan(ref))
    cmax = B.cmax_of(p32[2:5].astype(np.float64))
    n = np.array([int(got["nbhd_size"][y, x]) for y, x in pixels])
    assert ((n > 832) & (n <= 3136)).any()
    bar = B.sample_bar("direct", lay[1], n.max(), seed, box)
    both = np.isfinite(mine) & np.isfinite(ref)
    dist = np.where(both, np.abs(mine - ref), 0.0).max(axis=(0, 2)) / cmax
    worst = int(np.argmax(dist))
    print("STAGE4 %s route 13: worst %.3e (bar %.3e) at pixel %s N %d; %d samples" % (fid, dist[worst], bar, pixels[worst], n[worst], int(both.sum())))
    assert both.all() and (dist <= bar).all(), (float(dist[worst]), bar)


# ---- 4. 832 < S <= 3136 with no neighbours; S > 3136 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,S,cls", [(4, 4, 900, 8), (2, 2, 1601, 9)], ids=["S900", "S1601"])
def test_more_than_832_spp_has_empty_packed_and_wave_classes(ctx, hipmod, oracle, W, H, S, cls):
    """box 1: N = S on every pixel, one class, one launch.  (sigma_p = 1 // 4 = 0, rpf.cpp:531: every weight is NaN and EPS falls
    back to the input colour, in the oracle too; the stage outputs are compared for real)"""
    lay = DEFAULT_LAY
    planes, p32 = buffers(lay, W, H, S, seed=19, sigma_f=0.05, sigma_c=1e-4, mode="smooth")
    want = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=1, policy=EPS, n_random=lay[0], n_feat=lay[1]))
    got = run_debug(ctx, planes, desc_for(hipmod, lay, W, H, S, policy=EPS), 1)
    assert got["route"] == ROUTE_QUAD and got["launches"] == 1 and (got["nbhd_size"] == S).all()
    assert class_counts(got["nbhd_size"])[cls] == W * H
    check_pass_or_nan_pattern(got, want, hipmod)
    assert got["nonfinite_pixels"] == want["nonfinite_pixels"]
    r3 = run_debug(ctx, planes, desc_for(hipmod, lay, W, H, S, route=3, policy=EPS), 1)
    assert r3["route"] == 3
    bits_equal(got, r3, STAGE_KEYS)


def test_more_than_3136_spp_is_route_3(ctx, hipmod):
    lay, (W, H, S, box) = DEFAULT_LAY, (2, 1, 3137, 1)
    planes, _ = buffers(lay, W, H, S, seed=19, sigma_f=0.05, sigma_c=1e-4, mode="smooth")
    got = run_debug(ctx, planes, desc_for(hipmod, lay, W, H, S, policy=EPS), box)
    r3 = run_debug(ctx, planes, desc_for(hipmod, lay, W, H, S, route=3, policy=EPS), box)
    assert got["route"] == 3 and got["launches"] == 1
    bits_equal(got, r3, STAGE_KEYS + ("colour",))


# ---- 5. REF_ABORT residue through both new classes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["r", "b"], ids=["15spp-class1600", "45spp-class3136"])
def test_ref_abort_residue_and_redo_list(ctx, hipmod, oracle, which):
    planes, p32, indep = residue_frame(oracle) if which == "r" else residue_big_frame(oracle)
    _, H, W, S = p32.shape
    ref = residue_oracle(oracle, which, REF_ABORT)
    n = ref["nbhd_size"]
    got = run_debug(ctx, planes, desc_for(hipmod, RESIDUE_LAY, W, H, S, policy=REF_ABORT), RESIDUE_BOX)
    assert got["route"] == ROUTE_QUAD
    # every pixel of a class kernel meets the in-band table at a non-power-of-two N; the rest list is route 3's kernel's own work
    assert got["redo_pixels"] == int((n <= 3136).sum()) > 0
    assert ((n > 832) & (n <= 1600)).any() and (which == "r" or ((n > 1600) & (n <= 3136)).any())
    assert got["launches"] == expected_launches(hipmod, RESIDUE_LAY, n, REF_ABORT)
    _assert_ref_abort_parity(got, ref, hipmod, indep)
    e_ref = residue_oracle(oracle, which, EPS)
    e_got = run_debug(ctx, planes, desc_for(hipmod, RESIDUE_LAY, W, H, S, policy=EPS), RESIDUE_BOX)
    assert (e_got["mi"][..., indep] == 0).all() and e_got["route"] == ROUTE_QUAD and e_got["redo_pixels"] == 0
    check_pass(e_got, e_ref)


# ---- 6. non-finite inputs on pixels of class 1600 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", INF_INJECTIONS)
def test_quad_infinite_features_vs_oracle(ctx, hipmod, oracle, kind):
    W, H, S, box = INF_SHAPE
    planes, pix = inf_frame(kind)
    for policy in (hipmod.DEGEN_EPS, hipmod.DEGEN_REF_ABORT):
        want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=policy))
        got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=policy, flags=flags_of(hipmod, ROUTE_QUAD)), box=box,
                                    allow_nonfinite=True)
        assert ctx.route() == ROUTE_QUAD
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


# ---- 7. a scheduled pass ---------------------------------------------------------------------------------------------------------------------
def test_scheduled_pass_on_q32(ctx, hipmod, oracle):
    """RPF_FLAG_SCHEDULE with gains other than 1 (planted_nbhd.GAINS of the same planes, B32) against tests/schedule_ref.py: the
    unflagged run's bits up to W_r_c, alpha and beta bit for bit from the device's own MI, every sample within the direct bar"""
    W, H, S, box = geometry("Q32")
    planes = frame("Q32", SCHED_LAY)[0]
    gains, extra = P.GAINS["B32"], flags_of(hipmod, ROUTE_QUAD)
    base = sched_run(ctx, hipmod, planes, box, None, extra)
    got = sched_run(ctx, hipmod, planes, box, hipmod.make_schedule(0.5, *gains), extra, seed=0.002)
    assert got["max_nbhd"] == 1568
    check_scheduled(oracle, hipmod, planes, box, gains, base, got, ROUTE_QUAD, "Q32, route 13")


# ---- 8. entry points --------------------------------------------------------------------------------------------------------------------------
def q32():
    W, H, S, box = geometry("Q32")
    stored, p32, _ = frame("Q32", DEFAULT_LAY)
    return W, H, S, box, stored, p32


def test_filter_ex_two_passes_against_the_oracle_after_each(ctx, hipmod, oracle):
    W, H, S, box, planes, p32 = q32()
    seed = P.ACTIVE_SIGMA_SEED
    kw = dict(n_random=DEFAULT_LAY[0], n_feat=DEFAULT_LAY[1])
    o1 = frame_oracle(oracle, "Q32", DEFAULT_LAY, EPS, seed)["colour"]
    o2 = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=box, policy=EPS, sigma_seed=seed, **kw), colour_in=o1, debug=False)["colour"]
    one = ctx.filter(planes, desc_for(hipmod, DEFAULT_LAY, W, H, S, boxes=(box,), policy=EPS, sigma_seed=seed), want_colour64=True)
    assert one[2] == hipmod.OK and ctx.route() == ROUTE_QUAD
    assert rel_l2(one[3], o1) <= REL_L2_BAR
    d2 = desc_for(hipmod, DEFAULT_LAY, W, H, S, boxes=(box, box), policy=EPS, sigma_seed=seed)
    two = ctx.filter(planes, d2, want_colour64=True)
    assert two[2] == hipmod.OK and ctx.route() == ROUTE_QUAD
    assert rel_l2(two[3], o2) <= REL_L2_BAR
    assert np.array_equal(two[0], two[3].astype(np.float32))
    assert ctx.counters().filter_kernel_launches == 2 * frame_run(ctx, hipmod, "Q32", DEFAULT_LAY, EPS, seed)["launches"]
    # the second pass alone, fed the first call's colours: the same bits as the two-pass call
    again = ctx.filter(planes, desc_for(hipmod, DEFAULT_LAY, W, H, S, boxes=(box,), policy=EPS, sigma_seed=seed), colour64_in=one[3],
                       want_colour64=True)
    assert again[3].tobytes() == two[3].tobytes()


def test_row_slab_multi_context_and_film(ctx, hipmod):
    W, H, S, box, planes, _ = q32()
    seed = P.ACTIVE_SIGMA_SEED
    full = frame_run(ctx, hipmod, "Q32", DEFAULT_LAY, EPS, seed)
    part = run_debug(ctx, planes, desc_for(hipmod, DEFAULT_LAY, W, H, S, policy=EPS, sigma_seed=seed, row_begin=2, row_end=5), box)
    assert part["route"] == ROUTE_QUAD
    assert ((full["nbhd_size"][2:5] > 832) & (full["nbhd_size"][2:5] <= 3136)).any()
    assert np.array_equal(part["colour"][:, 2:5], full["colour"][:, 2:5])
    assert np.array_equal(part["nbhd_size"][2:5], full["nbhd_size"][2:5])
    assert np.array_equal(part["colour"][:, :2], planes[2:5, :2].astype(np.float64))      # the other rows pass through
    # two slabs on one device against the one-context call
    d = desc_for(hipmod, DEFAULT_LAY, W, H, S, boxes=(box,), policy=EPS, sigma_seed=seed)
    rw = (0.5 + np.random.default_rng(3).random((H, W, S))).astype(np.float32)
    srgb, prgb, st, c64 = ctx.filter(planes, d, ray_weight=rw, want_colour64=True)
    assert st == hipmod.OK and ctx.route() == ROUTE_QUAD and c64.tobytes() == full["colour"].tobytes()
    with hipmod.MultiContext([0, 0]) as mc:
        s2, p2, st2 = mc.filter(planes, d, ray_weight=rw)
    assert st2 == hipmod.OK
    assert np.array_equal(s2, srgb) and np.array_equal(p2, prgb)
    # the film step behind the same passes
    film = hipmod.make_film(((0, 0), (W, H)), 0.5, hipmod.film_table(FR.BOX))
    fs, t, w, img = ctx.filter_film(planes, d, film, ray_weight=rw)
    assert ctx.route() == ROUTE_QUAD
    assert np.array_equal(fs, srgb)
    t2, w2, img2 = film_device(ctx, hipmod, planes[0:2], c64, film, rw)
    assert np.array_equal(t, t2) and np.array_equal(w, w2) and np.array_equal(img, img2)


def test_pass_report_changes_no_colour_and_equals_the_restatement(ctx, hipmod):
    W, H, S, box, planes, _ = q32()
    seed = P.ACTIVE_SIGMA_SEED
    dbg = frame_run(ctx, hipmod, "Q32", DEFAULT_LAY, EPS, seed)
    on = desc_for(hipmod, DEFAULT_LAY, W, H, S, boxes=(box,), policy=EPS, sigma_seed=seed, flags=hipmod.PASS_REPORT_FLAG)
    out = ctx.filter(planes, on, want_colour64=True)
    rep, rows, cn, route = ctx.pass_report(0), ctx.pass_report_rows(0), ctx.counters(), ctx.route()
    assert route == ROUTE_QUAD == rep.route and out[3].tobytes() == dbg["colour"].tobytes()
    assert cn.filter_kernel_launches == dbg["launches"]
    want = PR.rows(planes[2:5].astype(np.float64), dbg["colour"], dbg["nbhd_size"], dbg["alpha"], dbg["beta"], dbg["wrc"], 0, None)
    assert len(rows) == len(want) == H
    for y, (g, w) in enumerate(zip(rows, want)):
        assert PR.differing(PR.of_ctypes(g), w) == [], ("row", y)
    assert rep.applied == 1 and rep.rows == H and PR.differing(PR.of_ctypes(rep.total), PR.fold(want)) == []
    assert (rep.total.sum_nbhd, rep.total.max_nbhd) == (cn.sum_nbhd, cn.max_nbhd) and cn.max_nbhd == 1568


# ---- 9. run-to-run determinism -----------------------------------------------------------------------------------------------------------------
def test_run_to_run_determinism(ctx, hipmod):
    """the order of the class lists comes from atomics: no result may depend on it"""
    W, H, S, box = geometry("Q40")
    lay = DEFAULT_LAY
    for policy in (EPS, REF_ABORT):
        d = desc_for(hipmod, lay, W, H, S, policy=policy, sigma_seed=P.ACTIVE_SIGMA_SEED)
        a = run_debug(ctx, frame("Q40", lay)[0], d, box)
        b = run_debug(ctx, frame("Q40", lay)[0], d, box)
        assert a["route"] == ROUTE_QUAD
        bits_equal(a, b, STAGE_KEYS + ("colour",))


# ---- 10. refusals on a context -------------------------------------------------------------------------------------------------------------------
def test_quad_flag_refusals(ctx, hipmod):
    lay, (W, H, S) = DEFAULT_LAY, (6, 5, 4)
    planes, _ = buffers(lay, W, H, S, seed=5, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    ctx.filter_pass_debug(planes, desc_for(hipmod, lay, W, H, S, policy=EPS), box=3)
    before = ctx.counters().filter_kernel_launches
    assert before >= 1 and ctx.route() == ROUTE_QUAD
    Q = hipmod.GENERIC_QUAD_FLAG
    nr, nf, _ = lay
    words = [Q, hipmod.FLAG_GENERIC | Q, hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED | Q,
             hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_WAVE | Q, hipmod.FLAG_GENERIC_PACKED | hipmod.FLAG_GENERIC_WAVE | Q,
             flags_of(hipmod, ROUTE_QUAD) | hipmod.FLAG_FAST_WEIGHTS, flags_of(hipmod, ROUTE_QUAD) | hipmod.FLAG_GENERIC_FAST,
             flags_of(hipmod, ROUTE_QUAD) | hipmod.FLAG_STREAM_FAST]
    for word in words:
        d = hipmod.make_desc(W, H, S, n_random=nr, n_feat=nf, flags=word, policy=EPS)
        for call in (lambda: ctx.filter_pass_debug(planes, d, box=3), lambda: ctx.filter(planes, d)):
            with pytest.raises(hipmod.RpfError) as e:
                call()
            assert e.value.status == hipmod.E_UNSUPPORTED, word
            assert "RPF_FLAG_GENERIC_QUAD" in str(e.value), word
            assert ctx.counters().filter_kernel_launches == before
