"""GPU tests of the layout-generic route (RPF_FLAG_GENERIC, rpf_query_route 3): any (n_random, n_feat, plane type) against
the oracle, stage by stage; the two compiled layouts on the generic kernels against their fused routes and against the
compiled reference's fixtures; the reference's rounding residue evaluated in place; non-finite inputs; every entry point
that reaches the pass loop; the refusals; and the same filter kernel behind the compiled routes, where it walks a pixel
list (the streaming size class, the REF_ABORT redo list).  No tolerance is new: check_pass's bars, or bit equality."""
import numpy as np
import pytest

import pbrt_film_ref as R
from raytracer_rpf_amd import feature_buffer as fb
from test_film_gpu import film_device
from test_gpu_parity import (INF_INJECTIONS, REL_L2_BAR, _assert_ref_abort_parity, _independent_columns, _inject_inf,
                             check_pass, rel_l2)
from test_ref_fixtures import FilterCases
from test_ref_gpu import check_against_reference

pytestmark = pytest.mark.gpu

LAYOUTS = [(1, 1, "f32"), (1, 3, "f32"), (3, 7, "f32"), (2, 12, "f16"), (4, 18, "f32"), (5, 13, "f16"), (8, 27, "f32")]
SMOOTH, CLUSTERED = ("smooth", 0.05, 1e-4), ("clustered", 1e-3, 0.01)
EPS, REF_ABORT = 1, 0
# name: W, H, S, box, (mode, sigma_f, sigma_c), policy, flat_frac
SHAPES = {
    "A": (14, 10, 8, 7, CLUSTERED, EPS, 0.0),
    "B": (12, 8, 16, 7, SMOOTH, EPS, 0.0),                  # N up to 784: several staging chunks
    "C": (14, 10, 8, 7, SMOOTH, REF_ABORT, 0.0),            # the oracle completes it for every layout
    "D": (7, 5, 1, 7, SMOOTH, EPS, 0.0),                    # S = 1
    "E": (30, 12, 8, 7, ("smooth", 2e-3, 0.01), EPS, 0.5),  # small neighbourhoods
    "G": (9, 7, 64, 7, SMOOTH, EPS, 0.0),                   # nmax = 3136
    "B32": (9, 7, 32, 7, SMOOTH, EPS, 0.0),
}


def lay_ids(v):
    return "%d-%d-%s" % v if isinstance(v, tuple) else None


def hip_desc(hipmod, lay, W, H, S, generic=True, **kw):
    nr, nf, dt = lay
    flags = kw.pop("flags", 0) | (hipmod.FLAG_GENERIC if generic else 0)
    return hipmod.make_desc(W, H, S, n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16 if dt == "f16" else hipmod.PLANES_F32,
                            flags=flags, **kw)


def buffers(lay, W, H, S, **kw):
    """the stored planes (fp32 or fp16) and their exact fp32 image, which is what the oracle reads"""
    nr, nf, dt = lay
    p = fb.synth_planes(W, H, S, n_random=nr, n_feat=nf, dtype=dt, **kw)
    return p, p.astype(np.float32)


_shape_cache = {}


def shape_case(oracle, lay, name, seed=19):
    """buffer and oracle pass of a named shape: computed once, shared by the tests that need it, never modified"""
    key = (lay, name, seed)
    if key not in _shape_cache:
        W, H, S, box, (mode, sf, sc), policy, flat = SHAPES[name]
        p, p32 = buffers(lay, W, H, S, seed=seed, sigma_f=sf, sigma_c=sc, mode=mode, flat_frac=flat)
        want = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=box, policy=policy, n_random=lay[0], n_feat=lay[1]))
        p.setflags(write=False)
        _shape_cache[key] = (p, p32, want)
    return _shape_cache[key]


def run_debug(ctx, hipmod, lay, name, planes, generic=True):
    W, H, S, box, _, policy, _ = SHAPES[name]
    got = ctx.filter_pass_debug(planes, hip_desc(hipmod, lay, W, H, S, generic=generic, policy=policy), box=box)
    got["route"] = ctx.route()
    got["launches"] = ctx.counters().filter_kernel_launches
    return got


# ---- 1. every stage output against the oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "G"])
@pytest.mark.parametrize("lay", LAYOUTS, ids=lay_ids)
def test_every_stage_vs_oracle(ctx, hipmod, oracle, lay, name):
    nr, nf, _ = lay
    planes, p32, want = shape_case(oracle, lay, name)
    S = SHAPES[name][2]
    assert np.isfinite(want["colour"]).all() and want["status"] == 0      # (C: REF_ABORT completes on this buffer)
    got = run_debug(ctx, hipmod, lay, name, planes)
    assert got["route"] == 3 and got["launches"] == 1 and got["status"] == hipmod.OK
    assert got["mi"].shape[-1] == nf * (nr + 2) + 3 * (nr + 2 + nf)        # RPF_NPAIR_OF
    assert got["beta"].shape[-1] == nf and got["mean"].shape[-1] == 5 + nr + nf
    check_pass(got, want)
    assert got["sum_nbhd"] == int(want["nbhd_size"].sum()) and got["max_nbhd"] == int(want["nbhd_size"].max())
    if name == "A":
        assert rel_l2(want["colour"], p32[2:5].astype(np.float64)) > 1e-3     # the filter is active
    if name == "E":
        assert (want["nbhd_size"] == S).mean() >= 0.4
    if name == "G":
        assert want["nbhd_size"].max() > 2500


# ---- 2. neighbourhoods beyond LDS residency ---------------------------------------------------------------------------
SHAPES["BOX17"] = (22, 19, 16, 17, SMOOTH, EPS, 0.0)        # N up to 4624: member list and bin ids in the HBM slots


@pytest.mark.parametrize("lay,seed", [((3, 7, "f32"), 19), ((2, 12, "f32"), 29)], ids=["3-7-f32", "19dim-seed29"])
def test_neighbourhoods_beyond_lds_residency(ctx, hipmod, oracle, lay, seed):
    """box 17 at 16 spp: N above 3136, member list and bin ids in the HBM slots"""
    planes, _, want = shape_case(oracle, lay, "BOX17", seed=seed)
    assert want["nbhd_size"].max() > 3136
    got = run_debug(ctx, hipmod, lay, "BOX17", planes)
    assert got["route"] == 3
    check_pass(got, want)


# ---- 3. the flag on the compiled layouts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "B32"])
@pytest.mark.parametrize("lay", [(2, 12, "f32"), (4, 18, "f16")], ids=lay_ids)
def test_flag_on_compiled_layouts(ctx, hipmod, oracle, lay, name):
    planes, _, want = shape_case(oracle, lay, name)
    fused = run_debug(ctx, hipmod, lay, name, planes, generic=False)
    gen = run_debug(ctx, hipmod, lay, name, planes, generic=True)
    assert gen["route"] == 3 and fused["route"] != 3
    for k in ("nbhd_size", "member_hash", "bin_hash", "mean", "stddev"):
        assert np.array_equal(gen[k], fused[k], equal_nan=k in ("mean", "stddev")), k
    check_pass(fused, want)
    check_pass(gen, want)


# ---- 4. against the compiled reference --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fcases():
    return FilterCases()


def test_generic_pass_against_reference(ctx, hipmod, fcases):
    n = 0
    for i in range(len(fcases)):
        boxes = fcases.boxes(i)
        if len(boxes) != 1:
            continue
        planes = fcases.planes(i)
        _, H, W, S = planes.shape
        desc = hipmod.make_desc(W, H, S, policy=hipmod.DEGEN_REF_ABORT, flags=hipmod.FLAG_GENERIC)
        got = ctx.filter_pass_debug(planes, desc, box=boxes[0], debug=False, allow_nonfinite=True)
        assert ctx.route() == 3
        check_against_reference(fcases, i, got["colour"], got["status"], hipmod, "generic filter_pass_debug")
        n += 1
    assert n >= 18


def test_generic_filter_against_reference_every_case_and_box_list(ctx, hipmod, fcases):
    for i in range(len(fcases)):
        planes, boxes = fcases.planes(i), fcases.boxes(i)
        _, H, W, S = planes.shape
        desc = hipmod.make_desc(W, H, S, boxes=tuple(boxes), policy=hipmod.DEGEN_REF_ABORT, flags=hipmod.FLAG_GENERIC)
        srgb, _, st, c64 = ctx.filter(planes, desc, want_colour64=True, allow_nonfinite=True)
        assert ctx.route() == 3
        if check_against_reference(fcases, i, c64, st, hipmod, "generic filter") is not None:
            assert np.array_equal(srgb, c64.astype(np.float32))
            assert ctx.counters().filter_kernel_launches == len(boxes)


# ---- 5. the reference's rounding residue -------------------------------------------------------------------------------------
def independent_frame(oracle, lay, W, H, S):
    """the frame of test_independent_tables_in_every_size_class_ref_abort for any layout: every feature of every pixel is a
    permutation of the same S values (all neighbours pass the 3-sigma test: windows are unions of whole pixels), r0 and f0
    carry the exactly independent pair of columns.  Returns the stored planes, their fp32 image and the pair's index."""
    nr, nf, dt = lay
    rng = np.random.default_rng(17)
    planes = rng.permuted(np.broadcast_to(np.linspace(0.4, 0.6, S), (5 + nr + nf, H, W, S)), axis=3).astype(np.float32)
    planes[0] = (np.arange(W)[None, :, None] + rng.random((H, W, S))).astype(np.float32)
    planes[1] = (np.arange(H)[:, None, None] + rng.random((H, W, S))).astype(np.float32)
    a, b = _independent_columns(S, 3)
    planes[5], planes[5 + nr] = a.astype(np.float32), b.astype(np.float32)   # r0, f0: the same pattern in every pixel
    if dt == "f16":
        planes = planes.astype(np.float16)
    pa, pb = oracle.pair_table(nr, nf)
    indep = [i for i in range(len(pa)) if (pa[i], pb[i]) == (5 + nr, 5)]
    assert len(indep) == 1
    return planes, planes.astype(np.float32), indep


@pytest.mark.parametrize("lay", [(3, 7, "f32"), (2, 12, "f32")], ids=lay_ids)
def test_rounding_residue_in_place_ref_abort(ctx, hipmod, oracle, lay):
    """the construction of test_independent_tables_in_every_size_class_ref_abort: every pixel's (f0, r0) table is exactly
    independent at a non-power-of-two N; the generic kernel evaluates mi.cpp:66-86 in place (no redo list)"""
    nr, nf, _ = lay
    W, H, S, box = 11, 11, 15, 9
    planes, _, indep = independent_frame(oracle, lay, W, H, S)
    ref = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, n_random=nr, n_feat=nf))
    got = ctx.filter_pass_debug(planes, hip_desc(hipmod, lay, W, H, S), box=box, allow_nonfinite=True)
    assert ctx.route() == 3
    n = ref["nbhd_size"]
    assert n.min() == 25 * S and n.max() == 81 * S
    ri = ref["mi"][..., indep]
    assert (np.abs(ri) < 1e-14).all() and (ri != 0).sum() > 20                        # residue, not zeros
    assert ctx.counters().redo_pixels == 0
    _assert_ref_abort_parity(got, ref, hipmod, indep)


# ---- 6. non-finite inputs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", INF_INJECTIONS)
@pytest.mark.parametrize("mode,flat", [("smooth", 0.0), ("clustered", 0.5)])
def test_generic_infinite_features_vs_oracle(ctx, hipmod, oracle, mode, flat, kind):
    W, H, S = 16, 12, 8
    sf, sc = (0.05, 1e-4) if mode == "smooth" else (1e-3, 0.01)
    planes = fb.synth_planes(W, H, S, seed=61, sigma_f=sf, sigma_c=sc, mode=mode, flat_frac=flat)
    pix = _inject_inf(planes, 19, kind)
    for policy in (hipmod.DEGEN_EPS, hipmod.DEGEN_REF_ABORT):
        want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7, policy=policy))
        if kind == "pixel_inf" and policy == hipmod.DEGEN_EPS:
            assert want["nbhd_size"][pix[0]] > S
        got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=policy, flags=hipmod.FLAG_GENERIC), box=7,
                                    allow_nonfinite=True)
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


# ---- 7. entries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", [(3, 7, "f32"), (5, 13, "f16")], ids=lay_ids)
def test_entries_stats_multi_pass_and_pinned(ctx, hipmod, oracle, lay):
    nr, nf, dt = lay
    W, H, S = 15, 11, 8
    planes, p32 = buffers(lay, W, H, S, seed=5, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    d = hip_desc(hipmod, lay, W, H, S, boxes=(7, 5), policy=EPS)
    m, sd = ctx.pixel_stats(planes, d)
    mo, so = oracle.pixel_stats(p32, oracle.make_desc(W, H, S, n_random=nr, n_feat=nf))
    assert m.shape[-1] == nf and np.array_equal(m, mo) and np.array_equal(sd, so, equal_nan=True)
    srgb, prgb, st, c64 = ctx.filter(planes, d, want_colour64=True)
    assert st == hipmod.OK and ctx.route() == 3 and ctx.counters().filter_kernel_launches == 2
    c = None
    for box in (7, 5):
        c = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=box, policy=EPS, n_random=nr, n_feat=nf), colour_in=c,
                               debug=False)["colour"]
    assert rel_l2(c64, c) <= 1e-9
    assert np.array_equal(srgb, c64.astype(np.float32))
    # page-locked buffers take the host pipeline's path; 11 rows are ONE band there (a frame below 32 rows is never cut), so this is the
    # serial order on the pipeline's streams -- the cut into several bands is held by tests/test_host_bands_gpu.py
    pin = ctx.host_empty(planes.shape, planes.dtype)
    pin[...] = planes
    out_s, out_p = ctx.host_empty(srgb.shape), ctx.host_empty(prgb.shape)
    ctx.filter(pin, d, out_samples=out_s, out_pixels=out_p)
    assert ctx.route() == 3
    assert np.array_equal(out_s, srgb) and np.array_equal(out_p, prgb)


@pytest.mark.parametrize("lay", [(3, 7, "f32"), (5, 13, "f16")], ids=lay_ids)
def test_entries_row_slab_and_multi_context(ctx, hipmod, lay):
    W, H, S = 15, 12, 8
    planes, _ = buffers(lay, W, H, S, seed=5, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    full = ctx.filter_pass_debug(planes, hip_desc(hipmod, lay, W, H, S, policy=EPS), box=7)
    part = ctx.filter_pass_debug(planes, hip_desc(hipmod, lay, W, H, S, policy=EPS, row_begin=3, row_end=9), box=7)
    assert ctx.route() == 3
    assert np.array_equal(part["colour"][:, 3:9], full["colour"][:, 3:9])
    assert np.array_equal(part["nbhd_size"][3:9], full["nbhd_size"][3:9])
    assert np.array_equal(part["colour"][:, :3], planes[2:5, :3].astype(np.float64))      # the other rows pass through
    W, H = 14, 16
    planes, _ = buffers(lay, W, H, S, seed=5, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    d = hip_desc(hipmod, lay, W, H, S, boxes=(7, 5), policy=EPS)
    s1, p1, st1 = ctx.filter(planes, d)
    with hipmod.MultiContext([0, 0]) as mc:
        s2, p2, st2 = mc.filter(planes, d)
    assert st1 == st2 == hipmod.OK
    assert np.array_equal(s1, s2) and np.array_equal(p1, p2)


def test_entries_filter_film(ctx, hipmod):
    """gaussian r = 2 over an 11 x 7 image: the sample film is 15 x 11 with origin (-2, -2)"""
    lay = (3, 7, "f32")
    W, H, S = 15, 11, 8
    planes, _ = buffers(lay, W, H, S, seed=5, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    planes[0] += np.float32(-2)
    planes[1] += np.float32(-2)
    rw = (0.5 + np.random.default_rng(3).random((H, W, S))).astype(np.float32)
    d = hip_desc(hipmod, lay, W, H, S, boxes=(7, 5), policy=EPS)
    film = hipmod.make_film(((0, 0), (11, 7)), 2.0, hipmod.film_table(R.GAUSSIAN))
    assert (film.sample_x0, film.sample_y0) == (-2, -2)
    srgb, t, w, img = ctx.filter_film(planes, d, film, ray_weight=rw)
    assert ctx.route() == 3
    s2, _, _, c64 = ctx.filter(planes, d, ray_weight=rw, want_pixels=False, want_colour64=True)
    assert np.array_equal(srgb, s2)
    assert rel_l2(c64, planes[2:5].astype(np.float64)) > 1e-3
    t2, w2, img2 = film_device(ctx, hipmod, planes[0:2], c64, film, rw)
    assert np.array_equal(t, t2) and np.array_equal(w, w2) and np.array_equal(img, img2)
    # the film entries keep refusing fp16 planes
    lay16 = (5, 13, "f16")
    p16, _ = buffers(lay16, W, H, S, seed=5, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    with pytest.raises(hipmod.RpfError) as e:
        ctx.filter_film(p16, hip_desc(hipmod, lay16, W, H, S, policy=EPS), film)
    assert e.value.status == hipmod.E_UNSUPPORTED


# ---- 8. refusals with a context -----------------------------------------------------------------------------------------------
def test_generic_refusals(ctx, hipmod):
    def refused(planes, desc):
        with pytest.raises(hipmod.RpfError) as e:
            ctx.filter(planes, desc)
        return e.value.status
    z = lambda nd, dt=np.float32: np.zeros((nd, 4, 4, 2), dt)
    assert refused(z(15), hip_desc(hipmod, (3, 7, "f32"), 4, 4, 2, generic=False)) == hipmod.E_UNSUPPORTED
    assert refused(z(41), hip_desc(hipmod, (9, 27, "f32"), 4, 4, 2)) == hipmod.E_UNSUPPORTED
    assert refused(z(15), hip_desc(hipmod, (3, 7, "f32"), 4, 4, 2, flags=hipmod.FLAG_FAST_WEIGHTS)) == hipmod.E_UNSUPPORTED
    assert refused(z(19), hipmod.make_desc(4, 4, 2, flags=hipmod.FLAG_GENERIC | hipmod.FLAG_FAST_WEIGHTS)) == hipmod.E_UNSUPPORTED
    # and the same descriptors through the device-free entry
    assert hipmod.layout_kernels(hip_desc(hipmod, (3, 7, "f32"), 4, 4, 2, generic=False))[0] == hipmod.E_UNSUPPORTED
    assert hipmod.layout_kernels(hip_desc(hipmod, (3, 7, "f32"), 4, 4, 2)) == (hipmod.OK, 1)


# ---- 9. seeded sweep --------------------------------------------------------------------------------------------------------
def sweep_cases():
    rng = np.random.RandomState(20261017)
    out = []
    for i in range(40):
        nr = int(rng.randint(1, 9)); nf = int(rng.randint(1, min(27, 35 - nr) + 1))
        dt = ("f32", "f16")[int(rng.randint(2))]
        S = int((1, 2, 3, 4, 5, 8, 12, 16, 32)[int(rng.randint(9))])
        box = int((5, 7, 9)[int(rng.randint(3))])
        W = int(rng.randint(5, 17)); H = int(rng.randint(5, 13))
        mode = ("smooth", "clustered")[int(rng.randint(2))]
        pol = int(rng.randint(2)) if S >= 8 else 1; bm = int(rng.randint(3))
        flat = (0.0, 0.5)[int(rng.randint(2))] if pol == 1 else 0.0
        out.append((i, nr, nf, dt, S, box, W, H, mode, pol, bm, flat))
    return out


@pytest.mark.parametrize("case", sweep_cases(), ids=lambda c: "%02d-nr%d-nf%d-%s-S%d-box%d" % c[:6])
def test_seeded_sweep(ctx, hipmod, oracle, case):
    i, nr, nf, dt, S, box, W, H, mode, pol, bm, flat = case
    sf, sc = (0.05, 1e-4) if mode == "smooth" else (1e-3, 0.01)
    lay = (nr, nf, dt)
    planes, p32 = buffers(lay, W, H, S, seed=100 + i, sigma_f=sf, sigma_c=sc, mode=mode, flat_frac=flat)
    want = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=box, policy=pol, beta_map=bm, n_random=nr, n_feat=nf))
    assert np.isfinite(want["colour"]).all()       # a non-finite oracle colour here is a failure, not a skip
    got = ctx.filter_pass_debug(planes, hip_desc(hipmod, lay, W, H, S, policy=pol, beta_map=bm), box=box)
    assert ctx.route() == 3
    check_pass(got, want)


# ---- 10. the same kernel behind the compiled routes: a pixel list instead of the rows --------------------------------------
COMPILED = [(2, 12, "f32"), (4, 18, "f16")]


@pytest.mark.parametrize("lay", COMPILED, ids=lay_ids)
def test_streaming_class_walks_its_list_next_to_resident_classes(ctx, hipmod, oracle, lay):
    """box 17 at 16 spp without the flag: the size-binned route gives the pixels with N > 3136 to the streaming kernel as a
    list, the others to the resident kernels.  With the flag the same kernel walks the rows: on the listed pixels every
    output is the same bits."""
    planes, _, want = shape_case(oracle, lay, "BOX17", seed=29)
    binned = run_debug(ctx, hipmod, lay, "BOX17", planes, generic=False)
    rows = run_debug(ctx, hipmod, lay, "BOX17", planes, generic=True)
    assert binned["route"] == 2 and rows["route"] == 3
    big = want["nbhd_size"] > 3136
    assert big.any() and not big.all()
    for k in ("nbhd_size", "member_hash", "bin_hash", "mean", "stddev", "mi", "alpha", "beta", "wrc"):
        assert binned[k][big].tobytes() == rows[k][big].tobytes(), k
    assert binned["colour"][:, big].tobytes() == rows["colour"][:, big].tobytes()
    check_pass(binned, want)


@pytest.mark.parametrize("lay", COMPILED, ids=lay_ids)
def test_redo_list_longer_than_its_grid(ctx, hipmod, oracle, lay):
    """REF_ABORT on a 16x12 frame whose every pixel joins the redo list: 192 entries for the 128 workgroups of the redo
    launch (list size read on the device, entries e, e + grid, ...; nmax = 1215: member list and bin ids in LDS)"""
    nr, nf, _ = lay
    W, H, S, box = 16, 12, 15, 9
    planes, p32, indep = independent_frame(oracle, lay, W, H, S)
    ref = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=box, n_random=nr, n_feat=nf))
    got = ctx.filter_pass_debug(planes, hip_desc(hipmod, lay, W, H, S, generic=False), box=box, allow_nonfinite=True)
    assert ctx.route() == 2
    assert ctx.counters().redo_pixels > 128
    ri = ref["mi"][..., indep]
    assert (np.abs(ri) < 1e-14).all() and (ri != 0).sum() > 20                        # residue, not zeros
    _assert_ref_abort_parity(got, ref, hipmod, indep)


def test_empty_redo_list_writes_nothing(ctx, hipmod, oracle):
    """REF_ABORT on a plain smooth buffer: no pixel joins the redo list, and the redo launch (a fixed grid that reads a
    count of zero on the device) leaves the resident kernels' results alone"""
    W, H, S = 12, 10, 8
    planes = fb.synth_planes(W, H, S, seed=19, sigma_f=0.05, sigma_c=1e-4, mode="smooth")
    want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=7))
    assert want["status"] == 0
    got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S), box=7)
    assert ctx.route() != 3 and ctx.counters().redo_pixels == 0 and got["status"] == hipmod.OK
    check_pass(got, want)
