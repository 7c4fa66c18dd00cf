"""GPU tests of the packed generic route (RPF_FLAG_GENERIC | RPF_FLAG_GENERIC_PACKED, rpf_query_route 4): neighbourhoods of
N <= 64 samples on generic::filter_packed_kernel behind generic::nbhd_count_kernel, the rest on generic::filter_pixel_kernel.
Every frame's input conditions are asserted against the oracle on the CPU by tests/test_generic_packed_cpu.py.  "Route 3"
below is the same context and buffer with RPF_FLAG_GENERIC alone.  No tolerance is new: check_pass's bars,
_assert_ref_abort_parity, REL_L2_BAR, or bit equality."""
import numpy as np
import pytest

import pbrt_film_ref as R
import planted_nbhd as P
from raytracer_rpf_amd import feature_buffer as fb
from test_film_gpu import film_device
from test_generic_layout_gpu import buffers, shape_case
from test_generic_packed_cpu import (EDGE_LAYOUTS, RESIDUE_BOX, RESIDUE_CASES, RESIDUE_LAYOUTS, class_counts, edge_frame,
                                     edge_geometry, edge_oracle, lay_ids, residue_frame, residue_oracle, stored_and_image)
from test_gpu_parity import (INF_INJECTIONS, REL_L2_BAR, STAGE_KEYS, _assert_ref_abort_parity, _inject_inf, check_pass,
                             rel_l2)

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
POLICIES = pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
DISCRETE_AND_STATS = ("nbhd_size", "member_hash", "bin_hash", "mean", "stddev")


def desc_for(hipmod, lay, W, H, S, packed=True, generic=True, **kw):
    nr, nf, dt = lay
    flags = kw.pop("flags", 0) | (hipmod.FLAG_GENERIC if generic else 0) | (hipmod.FLAG_GENERIC_PACKED if packed else 0)
    return hipmod.make_desc(W, H, S, n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16 if dt == "f16" else hipmod.PLANES_F32,
                            flags=flags, **kw)


def run_debug(ctx, planes, desc, box):
    got = ctx.filter_pass_debug(planes, desc, box=box, allow_nonfinite=True)
    c = ctx.counters()
    got.update(route=ctx.route(), launches=c.filter_kernel_launches, redo_pixels=c.redo_pixels)
    return got


def expected_launches(n, policy):
    return sum(1 for k in class_counts(n) if k) + (1 if policy == REF_ABORT else 0)


def bits_equal(a, b, keys):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


_edge_got = {}


def edge_run(ctx, hipmod, lay, policy, sigma_seed=0.002, packed=True, generic=True):
    """a pass over the edge frame: run once per variant, shared, never modified"""
    key = (lay, policy, sigma_seed, packed, generic)
    if key not in _edge_got:
        W, H, S, box = edge_geometry()
        d = desc_for(hipmod, lay, W, H, S, packed=packed, generic=generic, policy=policy, sigma_seed=sigma_seed)
        _edge_got[key] = run_debug(ctx, edge_frame(lay)[0], d, box)
    return _edge_got[key]


# ---- 1. class edges -------------------------------------------------------------------------------------------------------
@POLICIES
@pytest.mark.parametrize("lay", EDGE_LAYOUTS, ids=lay_ids)
def test_class_edges_vs_oracle_and_route3(ctx, hipmod, oracle, lay, policy):
    want = edge_oracle(oracle, lay, policy)
    got = edge_run(ctx, hipmod, lay, policy)
    assert got["route"] == 4 and got["status"] == hipmod.OK
    assert got["launches"] == expected_launches(want["nbhd_size"], policy)
    for (y, x), n in zip(edge_frame(lay)[2], P.FRAMES["U8"][3]):
        assert got["nbhd_size"][y, x] == n
    check_pass(got, want)
    r3 = edge_run(ctx, hipmod, lay, policy, packed=False)
    assert r3["route"] == 3 and r3["launches"] == 1
    bits_equal(got, r3, DISCRETE_AND_STATS)
    if policy == EPS:
        bits_equal(got, r3, ("mi",))            # both form it as ldexp(f, -44) / N from the same integers
        bits_equal(got, r3, ("alpha", "beta", "wrc"))   # ... and the weights from it by the same statements
        assert got["redo_pixels"] == 0


@pytest.mark.parametrize("lay", EDGE_LAYOUTS, ids=lay_ids)
def test_class_edges_active_seed(ctx, hipmod, oracle, lay):
    """weights of order one: a member dropped from, or a stale slot added to, a weight sum shows in the colours"""
    want = edge_oracle(oracle, lay, EPS, P.ACTIVE_SIGMA_SEED)
    got = edge_run(ctx, hipmod, lay, EPS, P.ACTIVE_SIGMA_SEED)
    assert got["route"] == 4
    check_pass(got, want)


@POLICIES
@pytest.mark.parametrize("lay", [(2, 12, "f32"), (4, 18, "f16")], ids=lay_ids)
def test_class_edges_compiled_layouts_vs_fused_route(ctx, hipmod, lay, policy):
    got = edge_run(ctx, hipmod, lay, policy)
    fused = edge_run(ctx, hipmod, lay, policy, packed=False, generic=False)
    assert got["route"] == 4 and fused["route"] in (0, 1)
    bits_equal(got, fused, DISCRETE_AND_STATS)


# ---- 2. whole waves and an empty rest list --------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [(3, 7, "f32"), (5, 13, "f16")], ids=lay_ids)
def test_whole_waves_and_empty_rest_list(ctx, hipmod, oracle, lay):
    planes, _, want = shape_case(oracle, lay, "E")       # 30 x 12 x 8, smooth 2e-3 / 0.01, flat_frac 0.5, box 7, EPS
    cc = class_counts(want["nbhd_size"])
    assert cc[4] == 0 and all(k > 0 for k in cc[:4]), cc
    got = run_debug(ctx, planes, desc_for(hipmod, lay, 30, 12, 8, policy=EPS), 7)
    assert got["route"] == 4 and got["launches"] == 4
    check_pass(got, want)


# ---- 3. no packed pixel, and S > 64 -----------------------------------------------------------------------------------------
def test_no_packed_pixel_runs_the_rest_list_alone(ctx, hipmod, oracle):
    lay, (W, H, S, box) = (3, 7, "f32"), (5, 4, 8, 7)
    planes, p32 = buffers(lay, W, H, S, seed=19, sigma_f=0.05, sigma_c=1e-4, mode="smooth")
    n = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=box, policy=EPS, n_random=3, n_feat=7), debug=True)["nbhd_size"]
    assert n.min() > 64
    got = run_debug(ctx, planes, desc_for(hipmod, lay, W, H, S, policy=EPS), box)
    r3 = run_debug(ctx, planes, desc_for(hipmod, lay, W, H, S, packed=False, policy=EPS), box)
    assert got["route"] == 4 and got["launches"] == 1 and r3["route"] == 3
    bits_equal(got, r3, STAGE_KEYS + ("colour",))        # the same kernel runs the same pixels


def test_more_than_64_spp_is_route_3(ctx, hipmod):
    lay, (W, H, S, box) = (3, 7, "f32"), (5, 4, 72, 3)
    planes, _ = buffers(lay, W, H, S, seed=19, sigma_f=0.05, sigma_c=1e-4, mode="smooth")
    got = run_debug(ctx, planes, desc_for(hipmod, lay, W, H, S, policy=EPS), box)
    r3 = run_debug(ctx, planes, desc_for(hipmod, lay, W, H, S, packed=False, policy=EPS), box)
    assert got["route"] == 3 and got["launches"] == 1
    bits_equal(got, r3, STAGE_KEYS + ("colour",))


# ---- 4. smallest and fullest groups ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [(3, 7, "f32"), (8, 27, "f32")], ids=lay_ids)
def test_one_sample_per_pixel(ctx, hipmod, oracle, lay):
    planes, _, want = shape_case(oracle, lay, "D")       # 7 x 5 x 1, box 7, EPS
    assert (want["nbhd_size"] == 1).all()                # B = 1
    got = run_debug(ctx, planes, desc_for(hipmod, lay, 7, 5, 1, policy=EPS), 7)
    assert got["route"] == 4 and got["launches"] == 1
    check_pass(got, want)


@pytest.mark.parametrize("lay", [(3, 7, "f32"), (8, 27, "f32")], ids=lay_ids)
def test_all_64_lanes_of_a_group(ctx, hipmod, oracle, lay):
    S, box, targets = 64, 3, (64, 65, 128)
    p32, pixels = P.plant(S, box, targets, n_random=lay[0], n_feat=lay[1], seed=0)
    planes, p32 = stored_and_image(p32, lay)
    W, H = box * len(targets), box
    want = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=box, policy=EPS, n_random=lay[0], n_feat=lay[1]))
    assert [int(want["nbhd_size"][y, x]) for y, x in pixels] == list(targets)
    got = run_debug(ctx, planes, desc_for(hipmod, lay, W, H, S, policy=EPS), box)
    assert got["route"] == 4 and got["launches"] == expected_launches(want["nbhd_size"], EPS)
    check_pass(got, want)


# ---- 5. REF_ABORT residue -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A", "B"])
@pytest.mark.parametrize("lay", RESIDUE_LAYOUTS, ids=lay_ids)
def test_ref_abort_residue_and_redo_list(ctx, hipmod, oracle, lay, case):
    W, S = RESIDUE_CASES[case]
    planes, _, indep = residue_frame(oracle, lay, case)
    ref = residue_oracle(oracle, lay, case, REF_ABORT)
    got = run_debug(ctx, planes, desc_for(hipmod, lay, W, 1, S, policy=REF_ABORT), RESIDUE_BOX)
    assert got["route"] == 4 and got["redo_pixels"] == W
    assert got["launches"] == 2                            # one class, and the redo launch
    _assert_ref_abort_parity(got, ref, hipmod, indep)
    e_ref = residue_oracle(oracle, lay, case, EPS)
    e_got = run_debug(ctx, planes, desc_for(hipmod, lay, W, 1, S, policy=EPS), RESIDUE_BOX)
    assert (e_ref["mi"][..., indep] == 0).all() and (e_got["mi"][..., indep] == 0).all()
    assert e_got["route"] == 4 and e_got["redo_pixels"] == 0 and e_got["launches"] == 1
    check_pass(e_got, e_ref)


# ---- 6. non-finite inputs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", INF_INJECTIONS)
def test_packed_infinite_features_vs_oracle(ctx, hipmod, oracle, kind):
    W, H, S = 16, 12, 8
    planes = fb.synth_planes(W, H, S, seed=61, sigma_f=1e-3, sigma_c=0.01, mode="clustered", flat_frac=0.5)
    pix = _inject_inf(planes, 19, kind)
    for policy in (hipmod.DEGEN_EPS, hipmod.DEGEN_REF_ABORT):
        want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7, policy=policy))
        if kind == "pixel_inf" and policy == hipmod.DEGEN_EPS:
            assert want["nbhd_size"][pix[0]] > S
        got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=policy, flags=hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED),
                                    box=7, allow_nonfinite=True)
        assert ctx.route() == 4
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


# ---- 7. entry points -----------------------------------------------------------------------------------------------------------
ENTRY_LAY = (3, 7, "f32")


def entry_frame():
    return buffers(ENTRY_LAY, 15, 12, 8, seed=5, sigma_f=1e-3, sigma_c=0.01, mode="clustered")


def test_entries_multi_pass_pinned_and_multi_context(ctx, hipmod, oracle):
    W, H, S = 15, 12, 8
    planes, p32 = entry_frame()
    d = desc_for(hipmod, ENTRY_LAY, W, H, S, boxes=(7, 5), policy=EPS)
    srgb, prgb, st, c64 = ctx.filter(planes, d, want_colour64=True)
    assert st == hipmod.OK and ctx.route() == 4
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
    assert ctx.route() == 4
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
    assert full["route"] == 4 and part["route"] == 4
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
    assert ctx.route() == 4
    s2, _, _, c64 = ctx.filter(planes, d, ray_weight=rw, want_pixels=False, want_colour64=True)
    assert np.array_equal(srgb, s2)
    assert rel_l2(c64, planes[2:5].astype(np.float64)) > 1e-3
    t2, w2, img2 = film_device(ctx, hipmod, planes[0:2], c64, film, rw)
    assert np.array_equal(t, t2) and np.array_equal(w, w2) and np.array_equal(img, img2)


# ---- 8. run-to-run determinism ---------------------------------------------------------------------------------------------------
def test_run_to_run_determinism(ctx, hipmod):
    """the order of the class lists comes from atomics: no result may depend on it"""
    lay = (3, 7, "f32")
    W, H, S, box = edge_geometry()
    for policy in (EPS, REF_ABORT):
        d = desc_for(hipmod, lay, W, H, S, policy=policy, sigma_seed=P.ACTIVE_SIGMA_SEED)
        a = run_debug(ctx, edge_frame(lay)[0], d, box)
        b = run_debug(ctx, edge_frame(lay)[0], d, box)
        assert a["route"] == 4
        bits_equal(a, b, STAGE_KEYS + ("colour",))


# ---- 9. refusals on a context ------------------------------------------------------------------------------------------------------
def test_packed_flag_refusals(ctx, hipmod):
    lay, (W, H, S) = (3, 7, "f32"), (6, 5, 4)
    planes, _ = buffers(lay, W, H, S, seed=5, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    ctx.filter_pass_debug(planes, desc_for(hipmod, lay, W, H, S, policy=EPS), box=3)
    before = ctx.counters().filter_kernel_launches
    assert before >= 1 and ctx.route() == 4
    P_, F_ = hipmod.FLAG_GENERIC_PACKED, hipmod.FLAG_FAST_WEIGHTS
    for d in (desc_for(hipmod, lay, W, H, S, packed=True, generic=False, policy=EPS),             # P alone
              desc_for(hipmod, lay, W, H, S, flags=F_, policy=EPS),                               # G | P | F
              hipmod.make_desc(W, H, S, policy=EPS, flags=P_)):                                   # P alone, compiled layout
        p = planes if d.n_random else np.zeros((19, H, W, S), np.float32)
        for call in (lambda: ctx.filter_pass_debug(p, d, box=3), lambda: ctx.filter(p, d)):
            with pytest.raises(hipmod.RpfError) as e:
                call()
            assert e.value.status == hipmod.E_UNSUPPORTED
            assert ctx.counters().filter_kernel_launches == before
