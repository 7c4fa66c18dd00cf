"""GPU tests of the one-wave generic route (RPF_FLAG_GENERIC | RPF_FLAG_GENERIC_PACKED | RPF_FLAG_GENERIC_WAVE,
rpf_query_route 5): neighbourhoods of 64 < N <= 832 samples on generic::filter_wave_kernel, N <= 64 on
generic::filter_packed_kernel, both behind generic::nbhd_count_kernel, the rest on generic::filter_pixel_kernel.  Every
frame's input conditions are asserted against the oracle on the CPU by tests/test_generic_wave_cpu.py.  "Route 3" below is
the same context and buffer with RPF_FLAG_GENERIC alone.  No tolerance is new: check_pass's bars, _assert_ref_abort_parity,
REL_L2_BAR, or bit equality."""
import numpy as np
import pytest

import pbrt_film_ref as R
import planted_nbhd as P
from test_film_gpu import film_device
from test_generic_layout_gpu import buffers
from test_generic_wave_cpu import (FRAMES, INF_SHAPE, LAYOUTS, RESIDUE_BOX, RESIDUE_LAY, RESIDUE_S, RESIDUE_W, class_counts, frame,
                                   frame_oracle, geometry, inf_frame, lay_ids, residue_frame, residue_oracle)
from test_gpu_parity import (INF_INJECTIONS, REL_L2_BAR, STAGE_KEYS, _assert_ref_abort_parity, check_pass, rel_l2)
from test_ref_fixtures import FilterCases
from test_ref_gpu import check_against_reference

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
POLICIES = pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
DISCRETE_AND_STATS = ("nbhd_size", "member_hash", "bin_hash", "mean", "stddev")
COMPILED = [(2, 12, "f32"), (4, 18, "f16")]


def desc_for(hipmod, lay, W, H, S, route=5, **kw):
    """route 5: G | P | W; 4: G | P; 3: G; 0: the fused kernels"""
    nr, nf, dt = lay
    add = {5: hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED | hipmod.FLAG_GENERIC_WAVE,
           4: hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED, 3: hipmod.FLAG_GENERIC, 0: 0}[route]
    return hipmod.make_desc(W, H, S, n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16 if dt == "f16" else hipmod.PLANES_F32,
                            flags=kw.pop("flags", 0) | add, **kw)


def run_debug(ctx, planes, desc, box):
    got = ctx.filter_pass_debug(planes, desc, box=box, allow_nonfinite=True)
    c = ctx.counters()
    got.update(route=ctx.route(), launches=c.filter_kernel_launches, redo_pixels=c.redo_pixels)
    return got


def expected_launches(n, policy):
    """one per non-empty packed class, one per non-empty wave class, one for the rest list, the redo launch"""
    return sum(1 for k in class_counts(n) if k) + (1 if policy == REF_ABORT else 0)


def bits_equal(a, b, keys, where=None):
    for k in keys:
        x, y = (a[k], b[k]) if where is None else (a[k][where], b[k][where])
        assert x.tobytes() == y.tobytes(), k


_got = {}


def frame_run(ctx, hipmod, fid, lay, policy, sigma_seed=0.002, route=5):
    """a pass over a planted frame: run once per variant, shared, never modified"""
    key = (fid, lay, policy, sigma_seed, route)
    if key not in _got:
        W, H, S, box = geometry(fid)
        _got[key] = run_debug(ctx, frame(fid, lay)[0], desc_for(hipmod, lay, W, H, S, route=route, policy=policy, sigma_seed=sigma_seed), box)
    return _got[key]


def check_pass_or_nan_pattern(got, want, hipmod):
    """check_pass; where the oracle's colours are not finite (it reports the pixels), the same status, count, first pixel and
    NaN pattern instead of a norm over NaNs, and every other bar of check_pass as it stands"""
    if np.isfinite(want["colour"]).all():
        assert got["status"] == hipmod.OK
        check_pass(got, want)
        return
    assert (got["status"] == hipmod.E_NONFINITE) == (want["status"] == 1)
    assert got["nonfinite_pixels"] == want["nonfinite_pixels"] and got["first_bad_pixel"] == want["first_bad_pixel"]
    nan = np.isnan(want["colour"])
    assert np.array_equal(np.isnan(got["colour"]), nan)
    check_pass(dict(got, colour=np.where(nan, 0.0, got["colour"])), dict(want, colour=np.where(nan, 0.0, want["colour"])))


# ---- 1. class edges at 16 spp ---------------------------------------------------------------------------------------------
@POLICIES
@pytest.mark.parametrize("lay", LAYOUTS, ids=lay_ids)
def test_e16_vs_oracle_and_route3(ctx, hipmod, oracle, lay, policy):
    want = frame_oracle(oracle, "E16", lay, policy)
    got = frame_run(ctx, hipmod, "E16", lay, policy)
    assert got["route"] == 5 and got["status"] == hipmod.OK
    assert got["launches"] == expected_launches(want["nbhd_size"], policy)
    for (y, x), n in zip(frame("E16", lay)[2], FRAMES["E16"][3]):
        assert got["nbhd_size"][y, x] == n
    check_pass(got, want)
    r3 = frame_run(ctx, hipmod, "E16", lay, policy, route=3)
    assert r3["route"] == 3 and r3["launches"] == 1
    bits_equal(got, r3, DISCRETE_AND_STATS)
    if policy == EPS:
        bits_equal(got, r3, ("mi", "alpha", "beta", "wrc"))   # the same integers, the same statements
        assert got["redo_pixels"] == 0


@POLICIES
@pytest.mark.parametrize("lay", COMPILED, ids=lay_ids)
def test_e16_compiled_layouts_vs_fused_route(ctx, hipmod, lay, policy):
    got = frame_run(ctx, hipmod, "E16", lay, policy)
    fused = frame_run(ctx, hipmod, "E16", lay, policy, route=0)
    assert got["route"] == 5 and fused["route"] in (0, 1, 2)
    bits_equal(got, fused, DISCRETE_AND_STATS)


# ---- 2. weights of order one ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", LAYOUTS, ids=lay_ids)
def test_e16_active_seed(ctx, hipmod, oracle, lay):
    """a member dropped from, or a stale slot added to, a weight sum shows in the colours"""
    want = frame_oracle(oracle, "E16", lay, EPS, P.ACTIVE_SIGMA_SEED)
    got = frame_run(ctx, hipmod, "E16", lay, EPS, P.ACTIVE_SIGMA_SEED)
    assert got["route"] == 5
    check_pass(got, want)


# ---- 3. the edge to the streaming kernel, and S > 64 --------------------------------------------------------------------------
@POLICIES
@pytest.mark.parametrize("fid", ["E32", "E72"])
def test_e32_e72_vs_oracle_and_route3(ctx, hipmod, oracle, fid, policy):
    """E72 under REF_ABORT: a box of 3 makes sigma_p = 0 (rpf.cpp:531) and every colour NaN in the oracle too
    (tests/test_generic_wave_cpu.py); the colour norm of check_pass is then taken where the oracle is finite -- nowhere -- and
    the status, the count, the first pixel and the NaN pattern are compared instead."""
    lay = FRAMES[fid][0]
    want = frame_oracle(oracle, fid, lay, policy)
    got = frame_run(ctx, hipmod, fid, lay, policy)
    assert got["route"] == 5
    assert got["launches"] == expected_launches(want["nbhd_size"], policy)
    for (y, x), n in zip(frame(fid, lay)[2], FRAMES[fid][3]):
        assert got["nbhd_size"][y, x] == n
    check_pass_or_nan_pattern(got, want, hipmod)
    r3 = frame_run(ctx, hipmod, fid, lay, policy, route=3)
    assert r3["route"] == 3
    bits_equal(got, r3, DISCRETE_AND_STATS)
    if fid == "E32":     # the rest list runs on the kernel of route 3
        rest = want["nbhd_size"] > 832
        assert rest.sum() == 57
        bits_equal(got, r3, STAGE_KEYS, where=rest)
        assert got["colour"][:, rest].tobytes() == r3["colour"][:, rest].tobytes()


# ---- 4. REF_ABORT residue -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", RESIDUE_S)
def test_ref_abort_residue_and_redo_list(ctx, hipmod, oracle, S):
    planes, _, indep = residue_frame(oracle, S)
    ref = residue_oracle(oracle, S, REF_ABORT)
    got = run_debug(ctx, planes, desc_for(hipmod, RESIDUE_LAY, RESIDUE_W, 1, S, policy=REF_ABORT), RESIDUE_BOX)
    assert got["route"] == 5 and got["redo_pixels"] == RESIDUE_W
    assert got["launches"] == 2                            # one class, and the redo launch
    _assert_ref_abort_parity(got, ref, hipmod, indep)
    assert np.isfinite(got["colour"]).all() == np.isfinite(ref["colour"]).all()
    e_ref = residue_oracle(oracle, S, EPS)
    e_got = run_debug(ctx, planes, desc_for(hipmod, RESIDUE_LAY, RESIDUE_W, 1, S, policy=EPS), RESIDUE_BOX)
    assert (e_ref["mi"][..., indep] == 0).all() and (e_got["mi"][..., indep] == 0).all()
    assert e_got["route"] == 5 and e_got["redo_pixels"] == 0 and e_got["launches"] == 1
    check_pass(e_got, e_ref)


# ---- 5. non-finite inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", INF_INJECTIONS)
def test_wave_infinite_features_vs_oracle(ctx, hipmod, oracle, kind):
    W, H, S, box = INF_SHAPE
    planes, pix = inf_frame(kind)
    for policy in (hipmod.DEGEN_EPS, hipmod.DEGEN_REF_ABORT):
        want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=policy))
        if kind == "pixel_inf" and policy == hipmod.DEGEN_EPS:
            assert want["nbhd_size"][pix[0]] > S
        flags = hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED | hipmod.FLAG_GENERIC_WAVE
        got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=policy, flags=flags), box=box, allow_nonfinite=True)
        assert ctx.route() == 5
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


# ---- 6. entry points ---------------------------------------------------------------------------------------------------------------
ENTRY_LAY = (3, 7, "f32")


def entry_frame():
    return buffers(ENTRY_LAY, 15, 12, 8, seed=5, sigma_f=0.05, sigma_c=1e-4, mode="smooth")


def test_entries_multi_pass_pinned_and_multi_context(ctx, hipmod, oracle):
    W, H, S = 15, 12, 8
    planes, p32 = entry_frame()
    d = desc_for(hipmod, ENTRY_LAY, W, H, S, boxes=(7, 5), policy=EPS)
    srgb, prgb, st, c64 = ctx.filter(planes, d, want_colour64=True)
    assert st == hipmod.OK and ctx.route() == 5
    c = None
    for box in (7, 5):
        c = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=box, policy=EPS, n_random=3, n_feat=7), colour_in=c,
                               debug=False)["colour"]
    assert rel_l2(c64, c) <= 1e-9
    assert np.array_equal(srgb, c64.astype(np.float32))
    # page-locked buffers take the host pipeline's path; 12 rows are ONE band there (a frame below 32 rows is never cut), so this is the
    # serial order on the pipeline's streams -- the cut into several bands is held by tests/test_host_bands_gpu.py
    pin = ctx.host_empty(planes.shape, planes.dtype)
    pin[...] = planes
    out_s, out_p = ctx.host_empty(srgb.shape), ctx.host_empty(prgb.shape)
    ctx.filter(pin, d, out_samples=out_s, out_pixels=out_p)
    assert ctx.route() == 5
    assert np.array_equal(out_s, srgb) and np.array_equal(out_p, prgb)
    # two slabs on one device
    with hipmod.MultiContext([0, 0]) as mc:
        s2, p2, st2 = mc.filter(planes, d)
    assert st2 == hipmod.OK
    assert np.array_equal(s2, srgb) and np.array_equal(p2, prgb)


def test_entries_row_slab(ctx, hipmod):
    W, H, S = 15, 12, 8
    planes, _ = entry_frame()
    full = run_debug(ctx, planes, desc_for(hipmod, ENTRY_LAY, W, H, S, policy=EPS), 7)
    part = run_debug(ctx, planes, desc_for(hipmod, ENTRY_LAY, W, H, S, policy=EPS, row_begin=3, row_end=9), 7)
    assert full["route"] == 5 and part["route"] == 5
    assert ((full["nbhd_size"] > 64) & (full["nbhd_size"] <= 832)).mean() > 0.9      # the wave kernels filter this frame
    assert np.array_equal(part["colour"][:, 3:9], full["colour"][:, 3:9])
    assert np.array_equal(part["nbhd_size"][3:9], full["nbhd_size"][3:9])
    assert np.array_equal(part["colour"][:, :3], planes[2:5, :3].astype(np.float64))      # the other rows pass through


def test_entries_filter_film_box_filter(ctx, hipmod):
    W, H, S = 15, 12, 8
    planes, _ = entry_frame()
    rw = (0.5 + np.random.default_rng(3).random((H, W, S))).astype(np.float32)
    d = desc_for(hipmod, ENTRY_LAY, W, H, S, boxes=(7, 5), policy=EPS)
    film = hipmod.make_film(((0, 0), (W, H)), 0.5, hipmod.film_table(R.BOX))
    assert (film.sample_x0, film.sample_y0) == (0, 0)
    srgb, t, w, img = ctx.filter_film(planes, d, film, ray_weight=rw)
    assert ctx.route() == 5
    s2, _, _, c64 = ctx.filter(planes, d, ray_weight=rw, want_pixels=False, want_colour64=True)
    assert np.array_equal(srgb, s2)
    t2, w2, img2 = film_device(ctx, hipmod, planes[0:2], c64, film, rw)
    assert np.array_equal(t, t2) and np.array_equal(w, w2) and np.array_equal(img, img2)


# ---- 7. run-to-run determinism -------------------------------------------------------------------------------------------------------
def test_run_to_run_determinism(ctx, hipmod):
    """the order of the class lists comes from atomics: no result may depend on it"""
    lay = (3, 7, "f32")
    W, H, S, box = geometry("E16")
    for policy in (EPS, REF_ABORT):
        d = desc_for(hipmod, lay, W, H, S, policy=policy, sigma_seed=P.ACTIVE_SIGMA_SEED)
        a = run_debug(ctx, frame("E16", lay)[0], d, box)
        b = run_debug(ctx, frame("E16", lay)[0], d, box)
        assert a["route"] == 5
        bits_equal(a, b, STAGE_KEYS + ("colour",))


# ---- 8. S > 832 -------------------------------------------------------------------------------------------------------------------------
def test_more_than_832_spp_is_route_3(ctx, hipmod):
    lay, (W, H, S, box) = (3, 7, "f32"), (5, 4, 840, 1)
    planes, _ = buffers(lay, W, H, S, seed=19, sigma_f=0.05, sigma_c=1e-4, mode="smooth")
    got = run_debug(ctx, planes, desc_for(hipmod, lay, W, H, S, policy=EPS), box)
    r3 = run_debug(ctx, planes, desc_for(hipmod, lay, W, H, S, route=3, policy=EPS), box)
    assert got["route"] == 3 and got["launches"] == 1
    bits_equal(got, r3, STAGE_KEYS + ("colour",))


# ---- 9. refusals on a context --------------------------------------------------------------------------------------------------------------
def test_wave_flag_refusals(ctx, hipmod):
    lay, (W, H, S) = (3, 7, "f32"), (6, 5, 4)
    planes, _ = buffers(lay, W, H, S, seed=5, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    ctx.filter_pass_debug(planes, desc_for(hipmod, lay, W, H, S, policy=EPS), box=3)
    before = ctx.counters().filter_kernel_launches
    assert before >= 1 and ctx.route() == 5
    W_, F_ = hipmod.FLAG_GENERIC_WAVE, hipmod.FLAG_FAST_WEIGHTS
    for d in (desc_for(hipmod, lay, W, H, S, route=3, flags=W_, policy=EPS),                      # G | W
              desc_for(hipmod, lay, W, H, S, route=0, flags=W_ | hipmod.FLAG_GENERIC_PACKED, policy=EPS),   # P | W
              desc_for(hipmod, lay, W, H, S, flags=F_, policy=EPS)):                              # G | P | W | F
        for call in (lambda: ctx.filter_pass_debug(planes, d, box=3), lambda: ctx.filter(planes, d)):
            with pytest.raises(hipmod.RpfError) as e:
                call()
            assert e.value.status == hipmod.E_UNSUPPORTED
            assert ctx.counters().filter_kernel_launches == before


# ---- 10. against the compiled reference ---------------------------------------------------------------------------------------------------
def test_wave_pass_against_reference(ctx, hipmod):
    """the one-pass FilterCases fixtures of the compiled reference through G | P | W under REF_ABORT (the loop of
    test_generic_layout_gpu.py::test_generic_pass_against_reference with the three flags)"""
    fcases = FilterCases()
    flags = hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED | hipmod.FLAG_GENERIC_WAVE
    n = 0
    for i in range(len(fcases)):
        boxes = fcases.boxes(i)
        if len(boxes) != 1:
            continue
        planes = fcases.planes(i)
        _, H, W, S = planes.shape
        desc = hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_REF_ABORT, flags=flags)
        got = ctx.filter_pass_debug(planes, desc, box=boxes[0], debug=False, allow_nonfinite=True)
        assert ctx.route() == 5
        check_against_reference(fcases, i, got["colour"], got["status"], hipmod, "wave filter_pass_debug")
        n += 1
    assert n >= 18
