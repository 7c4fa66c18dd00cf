"""The four-wave generic route's device-free surface (RPF_FLAG_GENERIC | RPF_FLAG_GENERIC_PACKED | RPF_FLAG_GENERIC_WAVE |
RPF_FLAG_GENERIC_QUAD, rpf_query_route 13): the flag's value and where its name lives, rpf_layout_kernels'
answers with it, the LDS carve-up query rpf_generic_quad_carve, and -- against the oracle, on the CPU -- what
tests/test_generic_quad_gpu.py takes for granted about its frames, so that a GPU failure is never a property of the input.
The frames are built here and imported by the GPU file."""
import ctypes
import os
import re

import numpy as np
import pytest

import planted_nbhd as P
from raytracer_rpf_amd import feature_buffer as fb
from test_generic_wave_cpu import lay_ids, stored_and_image
from test_gpu_parity import INF_INJECTIONS, _independent_columns, _inject_inf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, REF_ABORT = 1, 0
LDS_LIMIT = 160 * 1024                           # max_lds_per_block of the library
MAX_NDIM = 40

LAYOUTS = [(2, 12, "f32"), (4, 18, "f16"), (3, 7, "f32"), (1, 1, "f32"), (8, 27, "f16")]
NO_3136 = (17, 18, "f32")                        # 40 dims: the bin ids alone are 125 KB at 3136
CAPS = (8, 16, 32, 64, 128, 256, 448, 832, 1600, 3136)     # ten class capacities; beyond: the rest list
# id: S, box, planted N per target (one row of planted windows each)
FRAMES = {
    "Q40": (40, 9, (832, 833, 1600, 1601, 3136, 3137, 3240)),
    "Q32": (32, 7, (832, 833, 1568)),
    "Q64": (64, 7, (1600, 1601, 3135, 3136)),
}
DEFAULT_LAY = (3, 7, "f32")                      # the layout of the cases the issue names no layout for
SCHED_LAY = (2, 12, "f32")                       # tests/schedule_ref.py restates the 19-dim layout
RESIDUE_LAY, RESIDUE_BOX = (3, 7, "f32"), 9
# REF_ABORT residue through both new classes: W x 11 x 15 at box 9, every window a union of whole pixels, N = 15 * (25 ... 81)
RESIDUE_SHAPE = (11, 11, 15)
INF_SHAPE = (16, 12, 32, 7)                      # W, H, S, box: smooth, interior windows hold 49 * 32 = 1568 candidates


def class_counts(n, n_classes=10):
    """pixels per class: N <= 8, ..., up to CAPS[n_classes - 1], then the rest list"""
    out, lo = [], 0
    for cap in CAPS[:n_classes]:
        out.append(int(((n > lo) & (n <= cap)).sum()))
        lo = cap
    return out + [int((n > lo).sum())]


def geometry(fid):
    S, box, targets = FRAMES[fid]
    return box * len(targets), box, S, box       # W, H, S, box


_frames = {}


def frame(fid, lay):
    """(stored planes, fp32 image, target pixels) of a planted frame: built once per layout, read-only"""
    if (fid, lay) not in _frames:
        S, box, targets = FRAMES[fid]
        p32, pixels = P.plant(S, box, targets, n_random=lay[0], n_feat=lay[1], seed=0)
        _frames[fid, lay] = stored_and_image(p32, lay) + (pixels,)
    return _frames[fid, lay]


_want = {}


def frame_oracle(oracle, fid, lay, policy, sigma_seed=0.002):
    """the oracle's pass of a planted frame: computed once per session, shared, never modified"""
    key = (fid, lay, policy, sigma_seed)
    if key not in _want:
        W, H, S, box = geometry(fid)
        _want[key] = oracle.filter_pass(frame(fid, lay)[1], oracle.make_desc(W, H, S, box=box, policy=policy, sigma_seed=sigma_seed,
                                                                             n_random=lay[0], n_feat=lay[1]))
    return _want[key]


_residue = {}


def residue_frame(oracle):
    """test_gpu_parity.py::test_independent_tables_in_every_size_class_ref_abort's frame in the (3, 7, f32) layout: every pixel
    carries an exactly independent (f0, r0) table at a non-power-of-two N, every other column is a permutation of the same 15
    values, so a window is a union of whole pixels: N = 15 * (25 ... 81) = 375 ... 1215.  Returns (stored planes, fp32 image,
    index of the independent pair)."""
    if "r" not in _residue:
        nr, nf, _ = RESIDUE_LAY
        W, H, S = RESIDUE_SHAPE
        ndim = 5 + nr + nf
        rng = np.random.default_rng(17)
        planes = rng.permuted(np.broadcast_to(np.linspace(0.4, 0.6, S), (ndim, H, W, S)), axis=3).astype(np.float32)
        planes[0] = (np.arange(W)[None, :, None] + rng.random((H, W, S))).astype(np.float32)
        planes[1] = (np.arange(H)[:, None, None] + rng.random((H, W, S))).astype(np.float32)
        a, b = _independent_columns(S, 3)
        planes[5], planes[5 + nr] = a.astype(np.float32), b.astype(np.float32)   # r0, f0: the same pattern in every pixel
        pa, pb = oracle.pair_table(nr, nf)
        indep = [i for i in range(len(pa)) if (pa[i], pb[i]) == (5 + nr, 5)]
        assert len(indep) == 1
        _residue["r"] = stored_and_image(planes, RESIDUE_LAY) + (indep,)
    return _residue["r"]


def residue_big_frame(oracle):
    """the same construction at 45 spp (three copies of the 15-sample pattern per pixel): N = 45 * (25 ... 81) = 1125 ... 3645,
    so the class N <= 3136 meets the redo path too.  The independence is exact at any whole number of copies."""
    if "b" not in _residue:
        nr, nf, _ = RESIDUE_LAY
        W, H, S = 9, 9, 45
        ndim = 5 + nr + nf
        rng = np.random.default_rng(18)
        planes = rng.permuted(np.broadcast_to(np.linspace(0.4, 0.6, S), (ndim, H, W, S)), axis=3).astype(np.float32)
        planes[0] = (np.arange(W)[None, :, None] + rng.random((H, W, S))).astype(np.float32)
        planes[1] = (np.arange(H)[:, None, None] + rng.random((H, W, S))).astype(np.float32)
        a, b = _independent_columns(15, 3)
        planes[5], planes[5 + nr] = np.tile(a, 3).astype(np.float32), np.tile(b, 3).astype(np.float32)
        pa, pb = oracle.pair_table(nr, nf)
        indep = [i for i in range(len(pa)) if (pa[i], pb[i]) == (5 + nr, 5)]
        _residue["b"] = stored_and_image(planes, RESIDUE_LAY) + (indep,)
    return _residue["b"]


_residue_want = {}


def residue_oracle(oracle, which, policy):
    if (which, policy) not in _residue_want:
        nr, nf, _ = RESIDUE_LAY
        p32 = (residue_frame(oracle) if which == "r" else residue_big_frame(oracle))[1]
        _, H, W, S = p32.shape
        _residue_want[which, policy] = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=RESIDUE_BOX, policy=policy, n_random=nr, n_feat=nf))
    return _residue_want[which, policy]


def inf_frame(kind):
    """a smooth reference-layout frame at 32 spp with `kind` injected: (planes, injected pixels)"""
    W, H, S, _ = INF_SHAPE
    planes = fb.synth_planes(W, H, S, seed=61, sigma_f=0.05, sigma_c=1e-4, mode="smooth")
    return planes, _inject_inf(planes, 19, kind)


def make_desc_of(hipmod, lay, flags):
    return hipmod.make_desc(8, 8, 4, flags=flags, n_random=lay[0], n_feat=lay[1],
                            plane_dtype=hipmod.PLANES_F16 if lay[2] == "f16" else hipmod.PLANES_F32)


# ---- the flag, the header, the binding ---------------------------------------------------------------------------------------------
def test_flag_value_header_and_where_the_name_lives(hipmod):
    with open(os.path.join(ROOT, "include", "rpf_hip.h")) as f:
        text = f.read()
    m = re.search(r"\bRPF_FLAG_GENERIC_QUAD\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == 1048576 == 1 << 20
    assert getattr(hipmod, "GENERIC_QUAD_FLAG") == 1048576 and hipmod.GENERIC_QUAD_FLAG == 1048576
    assert "GENERIC_QUAD_FLAG" in dir(hipmod)
    assert "GENERIC_QUAD_FLAG" not in vars(hipmod)          # (not a module-level integer: the census of test_schedule_fused_cpu.py)
    others = [v for k, v in vars(hipmod).items() if isinstance(v, int) and not isinstance(v, bool) and (k.endswith("_FLAG") or k.startswith("FLAG_"))]
    others += [hipmod.SAMPLED_FUSED_FLAG, hipmod.SAMPLED_LISTED_FLAG]
    assert all(hipmod.GENERIC_QUAD_FLAG & v == 0 for v in others)
    assert re.search(r"int32_t\s+rpf_generic_quad_carve\(const rpf_desc \*desc, int32_t capacity, int32_t \*workgroups_per_cu_out,\s*int64_t \*lds_bytes_out\);", text)
    assert "rpf_generic_quad_carve" in hipmod.EXPORTS and hasattr(hipmod.load(), "rpf_generic_quad_carve")
    assert "13" in hipmod.Context.route.__doc__ and "GENERIC_QUAD_FLAG" in hipmod.Context.route.__doc__


TABLE_LAYOUTS = [(2, 12, "f32"), (4, 18, "f16"), (3, 7, "f32")]


@pytest.mark.parametrize("lay", TABLE_LAYOUTS, ids=lay_ids)
@pytest.mark.parametrize("flags,want", [
    ("GPWQ", ("OK", 1)),
    ("GPWQT", ("OK", 1)),
    ("Q", ("E_UNSUPPORTED", None)),              # refused without all three of G, P, W
    ("GQ", ("E_UNSUPPORTED", None)),
    ("GPQ", ("E_UNSUPPORTED", None)),
    ("GWQ", ("E_UNSUPPORTED", None)),
    ("PWQ", ("E_UNSUPPORTED", None)),
    ("GPWQF", ("E_UNSUPPORTED", None)),          # RPF_FLAG_FAST_WEIGHTS
    ("GPWQC", ("E_UNSUPPORTED", None)),          # RPF_FLAG_GENERIC_FAST
    ("GPWQS", ("E_UNSUPPORTED", None)),          # RPF_FLAG_STREAM_FAST
    ("GPWC", ("OK", 1)),                         # ... which stay accepted without the new flag
    ("GPWS", ("OK", 1)),
])
def test_layout_kernels_answers_with_the_quad_flag(hipmod, lay, flags, want):
    bits = {"G": hipmod.FLAG_GENERIC, "P": hipmod.FLAG_GENERIC_PACKED, "W": hipmod.FLAG_GENERIC_WAVE, "Q": hipmod.GENERIC_QUAD_FLAG,
            "F": hipmod.FLAG_FAST_WEIGHTS, "C": hipmod.FLAG_GENERIC_FAST, "S": hipmod.FLAG_STREAM_FAST, "T": hipmod.FLAG_TIMING}
    st, generic = hipmod.layout_kernels(make_desc_of(hipmod, lay, sum(bits[c] for c in flags)))
    assert (st, generic) == (getattr(hipmod, want[0]), want[1])


def test_the_new_rows_are_the_only_change(hipmod):
    """every flag word below the new bit that carries G | P | W answers the same with the bit, unless one of the new rows refuses
    it: RPF_FLAG_FAST_WEIGHTS (refused before), RPF_FLAG_GENERIC_FAST, RPF_FLAG_STREAM_FAST"""
    Q = hipmod.GENERIC_QUAD_FLAG
    gpw = hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED | hipmod.FLAG_GENERIC_WAVE
    refusing = hipmod.FLAG_FAST_WEIGHTS | hipmod.FLAG_GENERIC_FAST | hipmod.FLAG_STREAM_FAST
    lay = (3, 7, "f32")
    checked = changed = 0
    d = make_desc_of(hipmod, lay, 0)
    for word in range(Q):
        if word & gpw != gpw:
            continue
        d.flags = word
        without = hipmod.layout_kernels(d)
        d.flags = word | Q
        with_q = hipmod.layout_kernels(d)
        checked += 1
        if word & refusing:
            assert with_q == (hipmod.E_UNSUPPORTED, None), word
            changed += without != with_q
        else:
            assert with_q == without, word
    assert checked == Q // 8 and changed > 0
    # ... and a word without all three is refused with the bit whatever else it carries
    for word in (0, hipmod.FLAG_GENERIC, hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED, gpw & ~hipmod.FLAG_GENERIC):
        assert hipmod.layout_kernels(make_desc_of(hipmod, lay, word | Q)) == (hipmod.E_UNSUPPORTED, None)


# ---- the carve-up ---------------------------------------------------------------------------------------------------------------------
def own_of(cap):
    """own samples per sweep of stage 4: four in the class 1600 (two workgroups per CU by registers), eight in the class 3136 (one)"""
    return 4 if cap == 1600 else 8


def builder_bytes(nr, nf, cap, hists):
    """the arithmetic of generic_quad_carve (csrc/rpf_generic_quad.hip), restated: bytes of one workgroup with `hists` histograms
    per wave"""
    own = own_of(cap)
    up16 = lambda v: (v + 15) & ~15      # noqa: E731
    ndim, npair, nwt = 5 + nr + nf, nf * (nr + 2) + 3 * (nr + 2 + nf), 5 + nf
    o = up16((cap + 1) * 8)
    o = up16(o + 2 * npair)
    o += up16(cap * 4)
    o += up16(max(1024 * 4, ndim * 129 * 8, ndim * cap, own * nwt * 8))
    bmax = int(np.sqrt(cap))
    o += up16(4 * hists * ((bmax * bmax + 1) // 2) * 4)
    o += (8 * ndim + npair + 2 * nf + 20) * 8 + 4 * own * 4 * 8 + 16
    return up16(o)


def test_carve_fits_where_the_arithmetic_says_and_never_exceeds_the_limit(hipmod):
    n = 0
    for nr in range(1, MAX_NDIM - 5):
        for nf in range(1, MAX_NDIM - 5 - nr + 1):
            for dt in (hipmod.PLANES_F32, hipmod.PLANES_F16):
                d = hipmod.make_desc(8, 8, 4, n_random=nr, n_feat=nf, plane_dtype=dt)
                for cap in (1600, 3136):
                    fits = [h for h in (1, 2, 4) if builder_bytes(nr, nf, cap, h) <= LDS_LIMIT]
                    st, wg, lds = hipmod.generic_quad_carve(d, cap)
                    if fits:
                        assert st == hipmod.OK and 1 <= wg <= 2 and lds <= LDS_LIMIT, (nr, nf, cap, st, wg, lds)
                        assert lds in [builder_bytes(nr, nf, cap, h) for h in fits] and wg == min(8 // own_of(cap), LDS_LIMIT // lds)
                    else:
                        assert (st, wg, lds) == (hipmod.E_UNSUPPORTED, None, None), (nr, nf, cap)
                    if cap == 1600:
                        assert fits, (nr, nf)                      # every layout within RPF_MAX_NDIM gets the class N <= 1600
                    n += 1
    assert n == 2 * 2 * sum(MAX_NDIM - 5 - nr for nr in range(1, MAX_NDIM - 5))


def test_carve_answers(hipmod):
    d = lambda lay: make_desc_of(hipmod, lay, 0)      # noqa: E731
    assert hipmod.generic_quad_carve(d(NO_3136), 3136) == (hipmod.E_UNSUPPORTED, None, None)
    assert hipmod.generic_quad_carve(d(NO_3136), 1600)[0] == hipmod.OK
    assert hipmod.generic_quad_carve(d((8, 27, "f16")), 3136)[0] == hipmod.E_UNSUPPORTED     # 40 dims, whatever the plane type
    for lay in LAYOUTS[:4]:
        for cap in (1600, 3136):
            st, wg, lds = hipmod.generic_quad_carve(d(lay), cap)
            assert st == hipmod.OK and wg >= 1 and 0 < lds <= LDS_LIMIT
    for cap in (832, 0, -1, 1599, 3137, 65535):
        assert hipmod.generic_quad_carve(d((2, 12, "f32")), cap)[0] == hipmod.E_BADARG
    assert hipmod.generic_quad_carve(None, 1600)[0] == hipmod.E_BADARG
    assert hipmod.generic_quad_carve(hipmod.make_desc(8, 8, 4, n_random=9, n_feat=27), 1600)[0] == hipmod.E_UNSUPPORTED   # 41 dims
    assert hipmod.load().rpf_generic_quad_carve(ctypes.byref(d((2, 12, "f32"))), 1600, None, None) == hipmod.OK       # either output may be NULL


# ---- input conditions of the GPU tests, against the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("lay", LAYOUTS + [NO_3136], ids=lay_ids)
def test_q40_targets_and_classes(oracle, lay):
    want = frame_oracle(oracle, "Q40", lay, EPS)
    n = want["nbhd_size"]
    assert [int(n[y, x]) for y, x in frame("Q40", lay)[2]] == list(FRAMES["Q40"][2])
    cc = class_counts(n)
    assert cc[8] > 0 and cc[9] > 0 and cc[10] > 0 and sum(cc) == n.size       # both new classes and the rest list are non-empty
    assert want["status"] == 0 and np.isfinite(want["colour"]).all()


@pytest.mark.parametrize("fid,lay", [("Q32", DEFAULT_LAY), ("Q32", SCHED_LAY), ("Q64", DEFAULT_LAY)])
def test_q32_q64_targets_and_active_seed(oracle, fid, lay):
    want = frame_oracle(oracle, fid, lay, EPS, P.ACTIVE_SIGMA_SEED)
    n = want["nbhd_size"]
    assert [int(n[y, x]) for y, x in frame(fid, lay)[2]] == list(FRAMES[fid][2])
    cc = class_counts(n)
    assert cc[8] > 0 and (cc[9] > 0) == (fid == "Q64") and cc[10] == 0
    b = (FRAMES[fid][1] - 1) // 2
    cin = frame(fid, lay)[1][2:5, b].astype(np.float64)
    assert np.isfinite(want["colour"]).all()
    assert np.linalg.norm(want["colour"][:, b] - cin) / np.linalg.norm(cin) >= 0.05     # the filter is active on the target row


@pytest.mark.parametrize("which,lo,hi", [("r", 8, 8), ("b", 8, 9)])
def test_residue_frames_reach_the_new_classes(oracle, which, lo, hi):
    p32, indep = (residue_frame(oracle) if which == "r" else residue_big_frame(oracle))[1:]
    ref = residue_oracle(oracle, which, REF_ABORT)
    n = ref["nbhd_size"]
    S = p32.shape[3]
    assert n.min() == 25 * S and n.max() == 81 * S and ((n & (n - 1)) != 0).all()
    cc = class_counts(n)
    assert all(cc[c] > 0 for c in range(lo, hi + 1)), cc
    ri = ref["mi"][..., indep]
    assert (np.abs(ri) < 1e-13).all() and (ri != 0).sum() > 20                      # residue, not zeros
    assert (residue_oracle(oracle, which, EPS)["mi"][..., indep] == 0).all()


@pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
@pytest.mark.parametrize("kind", INF_INJECTIONS)
def test_inf_frame_neighbourhoods_are_of_class_1600(oracle, kind, policy):
    """the injected pixels and their window neighbours run on the four-wave kernel of class 1600: N in (832, 1600].  The one
    exception of tests/test_generic_wave_cpu.py stands: under EPS a pixel with an infinite own sample ("pixel_inf", "sample_inf")
    has its NaN sigma clamped to 0, rejects every finite candidate and keeps a small N; every other pixel of its window is of
    the class, and under REF_ABORT (a NaN limit never rejects) so is the pixel itself."""
    W, H, S, box = INF_SHAPE
    planes, pix = inf_frame(kind)
    n = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=policy))["nbhd_size"]
    quad = (n > 832) & (n <= 1600)
    small_own = policy == EPS and kind in ("pixel_inf", "sample_inf")
    b = (box - 1) // 2
    for y, x in pix:
        assert bool(quad[y, x]) != small_own, (kind, y, x, n[y, x])
        ok = quad.copy()
        for yy, xx in pix:
            ok[yy, xx] = True
        inner = ok[max(y - b, b):min(y + b + 1, H - b), max(x - b, b):min(x + b + 1, W - b)]     # (a clipped window holds fewer pixels)
        assert inner.all(), (kind, y, x)
