"""GPU tests of RPF_FLAG_GENERIC_FAST (X below): the fp32 pair-weight instantiations generic::filter_packed_kernel<T, G, true>
(N <= 64) and generic::filter_wave_kernel<T, true> (64 < N <= 832) behind G | P and G | P | W (G = RPF_FLAG_GENERIC, P =
..._PACKED, W = ..._WAVE).  Every frame's input conditions and the yardstick's own distance from the oracle are asserted on
the CPU by tests/test_generic_fast_cpu.py; "the run without X" is the same context, buffer and flags without the flag.

Bars (none of its own beyond these):
  contract    colours under X against the oracle <= REL_L2_BAR (1e-4, include/rpf_hip.h) over the whole frame, wherever the
              oracle is finite.
  regression  on the target row: g = rel-L2 of the device's colours under X against the oracle, e32 = the same for the numpy
              restatement of the documented fp32 arithmetic (tests/fast_weights_ref.py): g <= 16 * e32 + 1e-12, the bar of
              tests/test_fast_weights_gpu.py (the factor pays for the reciprocal of SD, log2 e folded into the coefficients,
              the fused multiply-add and the base-2 hardware exponential; 1e-12 is the suite's route-agreement rounding bar).
  discrete    every stage output (STAGE_KEYS), the launches and redo_pixels of a run under X are those of the run without X,
              bit for bit: the flag changes stage 4 alone.
  fp64 parts  the rest list, the redo list and a pass that falls back to route 3: colours bit-equal to the run without X.
  really fp32 at the active seed the colours under X differ from the run without X by more than 1e-10 relative L2 over the
              target-row pixels of an fp32 class (two fp64 runs agree to 1e-12; every e32 is >= 5.9e-9).

Measured on the MI355X, active seed (DESIGN.md section 11e has the table): g / e32 = 0.26 ... 1.04 over all cases of (a) and
(b) and both policies (g = 2.0e-9 ... 1.29e-8; the small ratios are frames whose target row holds many rest-list pixels), the
whole-frame distance from the oracle at most 1.28e-8; at the reference's seed g = 9.7e-14 on E16 (1, 1, f32), where e32 =
9.8e-14, 2e-18 on G72 and 0 elsewhere."""
import numpy as np
import pytest

import pbrt_film_ref as FR
import planted_nbhd as P
from test_film_gpu import film_device
from test_generic_fast_cpu import (G72_LAY, REFUSED, any_frame, any_geometry, any_oracle, flag_bits, yardstick_distance)
from test_generic_layout_gpu import buffers
from test_generic_packed_cpu import RESIDUE_BOX as PK_RESIDUE_BOX
from test_generic_packed_cpu import RESIDUE_CASES, RESIDUE_LAYOUTS
from test_generic_packed_cpu import residue_frame as pk_residue_frame
from test_generic_packed_cpu import residue_oracle as pk_residue_oracle
from test_generic_wave_cpu import (FRAMES, INF_SHAPE, LAYOUTS, RESIDUE_BOX, RESIDUE_LAY, RESIDUE_S, RESIDUE_W, class_counts, inf_frame,
                                   lay_ids, residue_frame, residue_oracle)
from test_generic_wave_gpu import entry_frame
from test_gpu_parity import INF_INJECTIONS, REL_L2_BAR, STAGE_KEYS, _assert_ref_abort_parity, check_pass, rel_l2

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = 1, 0
SEEDS = pytest.mark.parametrize("seed", [0.002, P.ACTIVE_SIGMA_SEED], ids=["ref_seed", "active_seed"])
POLICIES = pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
REGRESSION_FACTOR = 16


def desc_for(hipmod, lay, W, H, S, wave=True, fast=True, **kw):
    """G | P, with W (wave) and with X (fast)"""
    nr, nf, dt = lay
    flags = kw.pop("flags", 0) | hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED
    flags |= (hipmod.FLAG_GENERIC_WAVE if wave else 0) | (hipmod.FLAG_GENERIC_FAST if fast else 0)
    return hipmod.make_desc(W, H, S, n_random=nr, n_feat=nf, plane_dtype=hipmod.PLANES_F16 if dt == "f16" else hipmod.PLANES_F32,
                            flags=flags, **kw)


def run_debug(ctx, planes, desc, box):
    got = ctx.filter_pass_debug(planes, desc, box=box, allow_nonfinite=True)
    c = ctx.counters()
    got.update(route=ctx.route(), launches=c.filter_kernel_launches, redo_pixels=c.redo_pixels)
    return got


def bits_equal(a, b, keys):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


_got = {}


def frame_run(ctx, hipmod, fid, lay, policy, seed, wave, fast):
    """a pass over a frame: run once per variant, shared, never modified"""
    key = (fid, lay, policy, seed, wave, fast)
    if key not in _got:
        W, H, S, box = any_geometry(fid)
        _got[key] = run_debug(ctx, any_frame(fid, lay)[0], desc_for(hipmod, lay, W, H, S, wave=wave, fast=fast, policy=policy, sigma_seed=seed), box)
    return _got[key]


def check_fast_against_base_and_yardstick(ctx, hipmod, oracle, fid, lay, policy, seed, wave):
    """the assertions of (a): route, counters, stage outputs, contract, regression bar, the rest list, really fp32"""
    W, H, S, box = any_geometry(fid)
    b = (box - 1) // 2
    want = any_oracle(oracle, fid, lay, policy, seed)
    ref = frame_run(ctx, hipmod, fid, lay, policy, seed, wave, False)
    got = frame_run(ctx, hipmod, fid, lay, policy, seed, wave, True)
    assert got["route"] == ref["route"] == (5 if wave else 4)
    assert got["launches"] == ref["launches"] and got["redo_pixels"] == ref["redo_pixels"]
    assert got["status"] == ref["status"] == hipmod.OK
    bits_equal(got, ref, STAGE_KEYS)
    fin = np.isfinite(want["colour"])
    whole = rel_l2(got["colour"][fin], want["colour"][fin])
    assert np.isfinite(got["colour"][fin]).all() and whole <= REL_L2_BAR, whole
    finr = fin[:, b]
    g = rel_l2(got["colour"][:, b][finr], want["colour"][:, b][finr])
    e32 = yardstick_distance(oracle, fid, lay, policy, seed, np.float32)
    print("X %s %s %s policy %d seed %g: g = %.3e  e32 = %.3e  g / e32 = %s  whole frame %.3e" % (
        fid, lay_ids(lay), "G|P|W" if wave else "G|P", policy, seed, g, e32, "%.2f" % (g / e32) if e32 > 0 else "-", whole))
    assert g <= REGRESSION_FACTOR * e32 + 1e-12, (g, e32)
    n = want["nbhd_size"]
    assert np.array_equal(got["nbhd_size"], n)
    rest = n > (832 if wave else 64)            # the rest list: generic::filter_pixel_kernel, fp64
    assert got["colour"][:, rest].tobytes() == ref["colour"][:, rest].tobytes()
    if seed == P.ACTIVE_SIGMA_SEED:
        f32row = ~rest[b]
        assert f32row.any()
        d = rel_l2(got["colour"][:, b][:, f32row], ref["colour"][:, b][:, f32row])
        assert d > 1e-10, d                      # the mode really is fp32
    return got, ref, want


# ---- (a) class edges ----------------------------------------------------------------------------------------------------------
EDGE_CASES = ([("edge", lay, False) for lay in LAYOUTS] + [("edge", lay, True) for lay in LAYOUTS] + [("E16", lay, True) for lay in LAYOUTS]
              + [("E16", (3, 7, "f32"), False), ("E16", (4, 18, "f16"), False)])


def case_ids(v):
    return "%s-%s-%s" % (v[0], lay_ids(v[1]), "gpw" if v[2] else "gp")


@SEEDS
@POLICIES
@pytest.mark.parametrize("case", EDGE_CASES, ids=case_ids)
def test_class_edges_under_the_fast_flag(ctx, hipmod, oracle, case, policy, seed):
    fid, lay, wave = case
    got, _, want = check_fast_against_base_and_yardstick(ctx, hipmod, oracle, fid, lay, policy, seed, wave)
    cc = class_counts(want["nbhd_size"])
    assert any(cc[:4]) and (not wave or fid == "edge" or all(cc[4:8]))      # packed pixels; on E16 every one-wave class as well


# ---- (b) E32, G72, and the passes that fall back to route 3 ----------------------------------------------------------------------
@SEEDS
@POLICIES
@pytest.mark.parametrize("fid", ["E32", "G72"])
def test_e32_g72_under_the_fast_flag(ctx, hipmod, oracle, fid, policy, seed):
    lay = FRAMES["E32"][0] if fid == "E32" else G72_LAY
    _, _, want = check_fast_against_base_and_yardstick(ctx, hipmod, oracle, fid, lay, policy, seed, True)
    cc = class_counts(want["nbhd_size"])
    assert cc[7] > 0 and cc[8] > 0                    # class 832 against the rest list
    assert fid != "G72" or not any(cc[:4])            # route 5 with no packed pixel


@POLICIES
def test_g72_without_the_wave_flag_is_route_3(ctx, hipmod, policy):
    got = frame_run(ctx, hipmod, "G72", G72_LAY, policy, P.ACTIVE_SIGMA_SEED, False, True)
    ref = frame_run(ctx, hipmod, "G72", G72_LAY, policy, P.ACTIVE_SIGMA_SEED, False, False)
    assert got["route"] == ref["route"] == 3 and got["launches"] == ref["launches"]
    bits_equal(got, ref, STAGE_KEYS + ("colour",))


def test_more_than_832_spp_is_route_3(ctx, hipmod):
    lay, (W, H, S, box) = (3, 7, "f32"), (5, 4, 840, 1)
    planes, _ = buffers(lay, W, H, S, seed=19, sigma_f=0.05, sigma_c=1e-4, mode="smooth")
    got = run_debug(ctx, planes, desc_for(hipmod, lay, W, H, S, policy=EPS), box)
    ref = run_debug(ctx, planes, desc_for(hipmod, lay, W, H, S, fast=False, policy=EPS), box)
    assert got["route"] == ref["route"] == 3 and got["launches"] == ref["launches"] == 1
    bits_equal(got, ref, STAGE_KEYS + ("colour",))


# ---- (c) E72: sigma_p = 0 -------------------------------------------------------------------------------------------------------------
@POLICIES
def test_e72_nan_pattern_as_without_the_flag(ctx, hipmod, policy):
    lay = FRAMES["E72"][0]
    got = frame_run(ctx, hipmod, "E72", lay, policy, 0.002, True, True)
    ref = frame_run(ctx, hipmod, "E72", lay, policy, 0.002, True, False)
    assert got["route"] == ref["route"] == 5
    assert got["status"] == ref["status"]
    assert got["nonfinite_pixels"] == ref["nonfinite_pixels"] and got["first_bad_pixel"] == ref["first_bad_pixel"]
    assert np.array_equal(np.isnan(got["colour"]), np.isnan(ref["colour"]))
    assert np.isnan(ref["colour"]).all() == (policy == REF_ABORT)
    fin = np.isfinite(ref["colour"])
    assert np.isfinite(got["colour"][fin]).all()
    if fin.any():
        assert rel_l2(got["colour"][fin], ref["colour"][fin]) <= REL_L2_BAR
    bits_equal(got, ref, STAGE_KEYS)


# ---- (d) non-finite inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", INF_INJECTIONS)
def test_infinite_features_vs_oracle(ctx, hipmod, oracle, kind):
    """the assertions of tests/test_generic_wave_gpu.py::test_wave_infinite_features_vs_oracle under G | P | W | X (the numpy
    fp32 form keeps the oracle's NaN pattern on all five injections under both policies, so the device is held to the oracle's)"""
    W, H, S, box = INF_SHAPE
    planes, pix = inf_frame(kind)
    for policy in (hipmod.DEGEN_EPS, hipmod.DEGEN_REF_ABORT):
        want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=policy))
        if kind == "pixel_inf" and policy == hipmod.DEGEN_EPS:
            assert want["nbhd_size"][pix[0]] > S
        got = ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, policy=policy, flags=flag_bits(hipmod, "GPWX")), box=box, allow_nonfinite=True)
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


# ---- (e) the redo list -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", RESIDUE_S)
def test_wave_residue_frames_are_redone_in_fp64(ctx, hipmod, oracle, S):
    planes, _, indep = residue_frame(oracle, S)
    want = residue_oracle(oracle, S, REF_ABORT)
    got = run_debug(ctx, planes, desc_for(hipmod, RESIDUE_LAY, RESIDUE_W, 1, S, policy=REF_ABORT), RESIDUE_BOX)
    ref = run_debug(ctx, planes, desc_for(hipmod, RESIDUE_LAY, RESIDUE_W, 1, S, fast=False, policy=REF_ABORT), RESIDUE_BOX)
    assert got["route"] == ref["route"] == 5
    assert got["redo_pixels"] == ref["redo_pixels"] == RESIDUE_W and got["launches"] == ref["launches"] == 2
    _assert_ref_abort_parity(got, want, hipmod, indep)
    bits_equal(got, ref, STAGE_KEYS + ("colour",))      # the redo launch filters those pixels whole, in fp64


@pytest.mark.parametrize("case", ["A", "B"])
@pytest.mark.parametrize("lay", RESIDUE_LAYOUTS, ids=lay_ids)
def test_packed_residue_frames_are_redone_in_fp64(ctx, hipmod, oracle, lay, case):
    W, S = RESIDUE_CASES[case]
    planes, _, indep = pk_residue_frame(oracle, lay, case)
    want = pk_residue_oracle(oracle, lay, case, REF_ABORT)
    got = run_debug(ctx, planes, desc_for(hipmod, lay, W, 1, S, wave=False, policy=REF_ABORT), PK_RESIDUE_BOX)
    ref = run_debug(ctx, planes, desc_for(hipmod, lay, W, 1, S, wave=False, fast=False, policy=REF_ABORT), PK_RESIDUE_BOX)
    assert got["route"] == ref["route"] == 4
    assert got["redo_pixels"] == ref["redo_pixels"] == W and got["launches"] == ref["launches"] == 2
    _assert_ref_abort_parity(got, want, hipmod, indep)
    bits_equal(got, ref, STAGE_KEYS + ("colour",))


# ---- (f) entry points --------------------------------------------------------------------------------------------------------------------
ENTRY_LAY = (3, 7, "f32")
_entry = {}


def entry_filter(ctx, hipmod):
    """the two-pass filter call under G | P | W | X that every other entry point must reproduce: run once, shared"""
    if not _entry:
        W, H, S = 15, 12, 8
        planes, p32 = entry_frame()
        d = desc_for(hipmod, ENTRY_LAY, W, H, S, boxes=(7, 5), policy=EPS)
        srgb, prgb, st, c64 = ctx.filter(planes, d, want_colour64=True)
        assert st == hipmod.OK and ctx.route() == 5
        _entry.update(planes=planes, p32=p32, d=d, srgb=srgb, prgb=prgb, c64=c64)
    return _entry


def test_entries_filter_pinned_and_multi_context(ctx, hipmod, oracle):
    W, H, S = 15, 12, 8
    e = entry_filter(ctx, hipmod)
    c = None
    for box in (7, 5):
        c = oracle.filter_pass(e["p32"], oracle.make_desc(W, H, S, box=box, policy=EPS, n_random=3, n_feat=7), colour_in=c,
                               debug=False)["colour"]
    assert rel_l2(e["c64"], c) <= REL_L2_BAR
    assert np.array_equal(e["srgb"], e["c64"].astype(np.float32))
    # really fp32: not the bits of the call without X
    _, _, _, c64_ref = ctx.filter(e["planes"], desc_for(hipmod, ENTRY_LAY, W, H, S, fast=False, boxes=(7, 5), policy=EPS), want_colour64=True)
    assert rel_l2(c64_ref, c) <= 1e-9 and not np.array_equal(c64_ref, e["c64"])
    # page-locked buffers take the host pipeline's path; 12 rows are ONE band there (a frame below 32 rows is never cut), so this is the
    # serial order on the pipeline's streams -- the cut into several bands is held by tests/test_host_bands_gpu.py
    pin = ctx.host_empty(e["planes"].shape, e["planes"].dtype)
    pin[...] = e["planes"]
    out_s, out_p = ctx.host_empty(e["srgb"].shape), ctx.host_empty(e["prgb"].shape)
    ctx.filter(pin, e["d"], out_samples=out_s, out_pixels=out_p)
    assert ctx.route() == 5
    assert np.array_equal(out_s, e["srgb"]) and np.array_equal(out_p, e["prgb"])
    # two slabs on one device
    with hipmod.MultiContext([0, 0]) as mc:
        s2, p2, st2 = mc.filter(e["planes"], e["d"])
    assert st2 == hipmod.OK
    assert np.array_equal(s2, e["srgb"]) and np.array_equal(p2, e["prgb"])


def test_entries_row_slab(ctx, hipmod):
    """a slab is filtered one pass per call: rows [3, 9) of the first pass give the bits of the whole-frame first pass"""
    W, H, S = 15, 12, 8
    planes = entry_filter(ctx, hipmod)["planes"]
    full = run_debug(ctx, planes, desc_for(hipmod, ENTRY_LAY, W, H, S, policy=EPS), 7)
    part = run_debug(ctx, planes, desc_for(hipmod, ENTRY_LAY, W, H, S, policy=EPS, row_begin=3, row_end=9), 7)
    assert full["route"] == 5 and part["route"] == 5
    assert np.array_equal(part["colour"][:, 3:9], full["colour"][:, 3:9])
    assert np.array_equal(part["colour"][:, :3], planes[2:5, :3].astype(np.float64))      # the other rows pass through
    # ... and through rpf_filter: the slab's rows are the bits of the whole-frame call
    s_full, _, _ = ctx.filter(planes, desc_for(hipmod, ENTRY_LAY, W, H, S, boxes=(7,), policy=EPS), want_pixels=False)
    s_part, _, _ = ctx.filter(planes, desc_for(hipmod, ENTRY_LAY, W, H, S, boxes=(7,), policy=EPS, row_begin=3, row_end=9), want_pixels=False)
    assert ctx.route() == 5
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
    assert ctx.route() == 5
    assert np.array_equal(srgb, e["srgb"])
    t2, w2, img2 = film_device(ctx, hipmod, planes[0:2], e["c64"], film, rw)
    assert np.array_equal(t, t2) and np.array_equal(w, w2) and np.array_equal(img, img2)
    dev = torch.device("cuda", 0)
    dp = torch.from_numpy(np.ascontiguousarray(planes)).to(dev)
    col = dp[2:5].to(torch.float64).contiguous()
    ctx.filter_device(d, dp.data_ptr(), col.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ctx.route() == 5
    assert np.array_equal(col.cpu().numpy(), e["c64"])


# ---- (g) run-to-run determinism ------------------------------------------------------------------------------------------------------------
def test_run_to_run_determinism(ctx, hipmod):
    """the order of the class lists comes from atomics: no result may depend on it"""
    lay = (3, 7, "f32")
    W, H, S, box = any_geometry("E16")
    for policy in (EPS, REF_ABORT):
        d = desc_for(hipmod, lay, W, H, S, policy=policy, sigma_seed=P.ACTIVE_SIGMA_SEED)
        a = run_debug(ctx, any_frame("E16", lay)[0], d, box)
        b = run_debug(ctx, any_frame("E16", lay)[0], d, box)
        assert a["route"] == 5
        bits_equal(a, b, STAGE_KEYS + ("colour",))


# ---- (h) refusals on a live context ----------------------------------------------------------------------------------------------------------
def test_fast_flag_refusals(ctx, hipmod):
    lay, (W, H, S) = (3, 7, "f32"), (6, 5, 4)
    planes, _ = buffers(lay, W, H, S, seed=5, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    ctx.filter_pass_debug(planes, desc_for(hipmod, lay, W, H, S, policy=EPS), box=3)
    before = ctx.counters().filter_kernel_launches
    assert before >= 1 and ctx.route() == 5
    for letters in REFUSED:
        d = hipmod.make_desc(W, H, S, n_random=3, n_feat=7, policy=EPS, flags=flag_bits(hipmod, letters))
        for call in (lambda: ctx.filter_pass_debug(planes, d, box=3), lambda: ctx.filter(planes, d)):
            with pytest.raises(hipmod.RpfError) as e:
                call()
            assert e.value.status == hipmod.E_UNSUPPORTED, letters
            assert ctx.counters().filter_kernel_launches == before, letters
