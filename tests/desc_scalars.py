"""The two descriptor fields stage 3c reads -- rpf_desc.beta_map and rpf_desc.eps -- on every route: the combos, the case table
and the checkers that tests/test_desc_scalars_cpu.py (the oracle and the restatement alone) and tests/test_desc_scalars_gpu.py
(the kernels) share.  A plain helper module, like planted_nbhd.py.

Stage 3c (alpha, beta, W_r_c from the MI vector; rpf.cpp:444-487) is written out six times in csrc/ (bodies A to F below), and
tests/schedule_ref.py::alpha_beta restates it with the sums in the kernels' order of additions.  check_stage3c holds a pass to
that restatement on the pass's OWN MI, bit for bit on every pixel; check_against_default holds everything in front of stage 3c to
the pass with the default fields.  Neither has a tolerance.

Bodies:  A rpf_filter_impl.inc   B rpf_packed_impl.inc   C rpf_generic_stream_stages.inc   D rpf_generic_packed.hip
         E rpf_generic_wave.hip   F rpf_generic_quad.hip"""
import collections

import numpy as np

import member_test_ref as MR
import planted_nbhd as P
import schedule_ref as SRf
from test_gpu_parity import _independent_columns
from test_schedule_fused_gpu import BITS, same, same_or_nan

EPS, REF_ABORT = 1, 0
SIGMA = P.ACTIVE_SIGMA_SEED
DEFAULT = (0, 1e-10)                                    # what the rest of the suite runs
# (beta_map, eps).  0.0123 is no power of two and eight orders from the default
COMBOS = [(1, 1e-10), (2, 1e-10), (0, 0.0123), (1, 0.0123), (2, 0.0123)]
STAGE4_COMBO = (2, 0.0123)                              # the one combo whose colours are restated


def check_stage3c(got, beta_map, eps, gains, nR, nF):
    """alpha, beta and W_r_c of the pass `got` (a dict as hip.Context.filter_pass_debug returns it) are schedule_ref.alpha_beta on
    got's own MI under (beta_map, eps) and the gains (None: (1, 1)): equal NaN patterns, every other entry bit for bit"""
    gc, gf = (1.0, 1.0) if gains is None else gains
    a, b, w = SRf.alpha_beta(got["mi"], gc, gf, beta_map, eps, nR, nF)
    for k, want in (("alpha", a), ("beta", b), ("wrc", w)):
        assert same_or_nan(got[k], want), (k, beta_map, eps, gains)


def check_against_default(got, base, same_eps=None):
    """`got` under some (beta_map, eps) against the (0, 1e-10) pass `base` of the same route and gains: neither field reaches
    stages 1 to 3b, the route or the counters.  same_eps: a pass at got's eps under another preset -- W_r_c does not read the
    preset"""
    for k in BITS:
        if k != "wrc":
            assert same(got[k], base[k]), k
    if same_eps is not None:
        assert same_or_nan(got["wrc"], same_eps["wrc"]), "wrc"
    for k in ("route", "launches", "redo_pixels", "sum_nbhd", "max_nbhd"):
        assert got[k] == base[k], (k, got[k], base[k])


# ---- frames -----------------------------------------------------------------------------------------------------------------------
# three more layouts planted with U8's targets (L*), and with B32's for the four-wave classes of route 13 (Q*):
#   (1, 3) f32   no gap and no D_r_fk term: presets 0 and 1 give the same bits
#   (3, 5) f16   preset 0 reaches D_r_fk[0] at k = 4; preset 1 is zero from k = 3 on
#   (8, 27) f32  40 dims, the widest
LAYOUTS = {"1x3": (1, 3, "f32"), "3x5": (3, 5, "f16"), "8x27": (8, 27, "f32")}
LAYOUT_FRAMES = {**{"L" + k: (lay, 8, 7, P.FRAMES["U8"][3]) for k, lay in LAYOUTS.items()},
                 **{"Q" + k: (lay, 32, 7, P.FRAMES["B32"][3]) for k, lay in LAYOUTS.items()}}

Frame = collections.namedtuple("Frame", "fid stored p32 pixels targets lay S box W H sampling")
_frames = {}


def frame(fid):
    """a frame of planted_nbhd.FRAMES, planted_nbhd.SAMPLED_FRAMES or LAYOUT_FRAMES; built once, read-only"""
    if fid not in _frames:
        if fid in P.FRAMES:
            lay, S, box, targets = P.FRAMES[fid][:4]
            stored, p32, pixels, _ = P.frame(fid)
            sampling = None
        elif fid in P.SAMPLED_FRAMES:
            lay, S, box, D, sseed, targets, _ = P.SAMPLED_FRAMES[fid]
            stored, p32, pixels, _ = P.sampled_frame(fid)
            sampling = (sseed, D)
        else:
            lay, S, box, targets = LAYOUT_FRAMES[fid]
            p32, pixels = P.plant(S, box, targets, lay[0], lay[1])
            stored = p32.astype(np.float16) if lay[2] == "f16" else p32
            p32 = stored.astype(np.float32)
            stored.setflags(write=False)
            p32.setflags(write=False)
            sampling = None
        _frames[fid] = Frame(fid, stored, p32, pixels, tuple(targets), lay, S, box, box * len(targets), box, sampling)
    return _frames[fid]


def nan_frame(fid):
    """section f: the frame with colour plane 2 set to the constant 0.25.  Colour is not in the membership test, so the planted
    sizes stand; a constant colour has MI 0 with everything, so with eps = 0 its W_r_c is 0 / 0"""
    key = "nan:" + fid
    if key not in _frames:
        f = frame(fid)
        stored = np.array(f.stored)
        stored[2] = 0.25
        p32 = stored.astype(np.float32)
        stored.setflags(write=False)
        p32.setflags(write=False)
        _frames[key] = f._replace(fid=key, stored=stored, p32=p32)
    return _frames[key]


REDO_SHAPE = (11, 11, 15, 9)                            # W, H, S, box


def redo_frame():
    """the frame of tests/test_gpu_parity.py::test_independent_tables_in_every_size_class_ref_abort, statement for statement:
    11 x 11 x 15, box 9, every pixel on the redo list under REF_ABORT"""
    if "redo" not in _frames:
        W, H, S, box = REDO_SHAPE
        rng = np.random.default_rng(17)
        planes = rng.permuted(np.broadcast_to(np.linspace(0.4, 0.6, S), (19, H, W, S)), axis=3).astype(np.float32)
        planes[0] = (np.arange(W)[None, :, None] + rng.random((H, W, S))).astype(np.float32)
        planes[1] = (np.arange(H)[:, None, None] + rng.random((H, W, S))).astype(np.float32)
        a, b = _independent_columns(S, 3)
        planes[5], planes[7] = a.astype(np.float32), b.astype(np.float32)
        planes.setflags(write=False)
        _frames["redo"] = Frame("redo", planes, planes, [], (), (2, 12, "f32"), S, box, W, H, None)
    return _frames["redo"]


def gains_of(fid):
    """the gains that clamp on a frame: planted_nbhd.GAINS / SAMPLED_GAINS (None: the frame has none)"""
    return P.GAINS.get(fid, P.SAMPLED_GAINS.get(fid))


_oracle = {}


def oracle_pass(oracle, f, beta_map=0, eps=1e-10):
    """the oracle's full-box pass of a frame under EPS at the active seed: computed once per session, shared, never modified"""
    key = (f.fid, beta_map, eps)
    if key not in _oracle:
        if f.fid in P.FRAMES and (beta_map, eps) == DEFAULT:
            _oracle[key] = P.oracle_pass(oracle, f.fid, EPS, SIGMA)
        else:
            nr, nf, _ = f.lay
            lay = dict(n_random=nr, n_feat=nf) if (nr, nf) != (2, 12) else {}
            _oracle[key] = oracle.filter_pass(f.p32, oracle.make_desc(f.W, f.H, f.S, box=f.box, policy=EPS, sigma_seed=SIGMA,
                                                                      beta_map=beta_map, eps=eps, **lay))
    return _oracle[key]


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# mode: how the descriptor and the context state are built (run_pass of tests/test_desc_scalars_gpu.py):
#   compiled  no route flag (routes 0 / 1, or 2); opts: context options      r10  MEMBER_TEST | MEMBER_FUSED under MR.reference
#   r12 / r11 / r8  SAMPLED_NBHD | LISTED / | FUSED / alone                  r9   MEMBER_TEST under planted_nbhd.nonref
#   g3 g4 g5 g13    the layout-generic flags                                 w6 w7  the wide flags on the `forced` context
# fast: None, or the fp32-weights flag of the row ("FAST_WEIGHTS", "GENERIC_FAST", "STREAM_FAST")
# gains: None, or the frame's gains: the row then runs under RPF_FLAG_SCHEDULE (| RPF_FLAG_SCHEDULE_FUSED on the compiled kernels)
Row = collections.namedtuple("Row", "id fid mode opts routes bodies gains fast")
SCHEDULED_FUSED = ("compiled", "r10", "r11", "r12")     # modes whose scheduled pass needs RPF_FLAG_SCHEDULE_FUSED


def _rows():
    out = []

    def add(fid, mode, routes, bodies, opts=None, with_gains=True, fast=None, tag=None):
        name = "%s-%s" % (tag or mode, fid) + "".join("-%s%d" % kv for kv in (opts or {}).items()) + ("-" + fast if fast else "")
        out.append(Row(name, fid, mode, opts or {}, routes, bodies, None, fast))
        if with_gains:
            out.append(Row(name + "-gains", fid, mode, opts or {}, routes, bodies, gains_of(fid), fast))

    # a. the compiled routes, plain and scheduled builds
    add("U8", "compiled", (0, 1), "AB")
    add("U8", "compiled", (2,), "AB", dict(binning=1))
    add("B16", "compiled", (2,), "AB")                  # one-wave classes to 832
    add("B32", "compiled", (2,), "A")                   # K = 25
    add("B32", "compiled", (2,), "A", dict(split_weights=0))
    add("B64", "compiled", (2,), "A")                   # K = 49
    add("B40", "compiled", (2,), "AC")                  # 3136 | 3137, 3240: the streaming class
    add("H8", "compiled", (0, 1), "AB")                 # the d27 builds
    add("H16", "compiled", (2,), "A")
    add("H64", "compiled", (2,), "A")
    # b. routes 10, 11, 12: the member, listed and listed-scheduled builds
    add("B16", "r10", (10,), "AB", with_gains=False)
    add("H16", "r10", (10,), "A", with_gains=False)
    for fid in ("SP8", "SP16", "SP32", "SPH16", "SPH32"):
        add(fid, "r12", (12,), "AB" if fid in ("SP8", "SPH16") else "A")
    add("SP8", "r11", (11,), "AB", with_gains=False)
    add("SPH16", "r11", (11,), "AB", with_gains=False)
    # c. the layout-generic routes
    add("U8", "g3", (3,), "C")
    add("B40", "g3", (3,), "C")
    add("U8", "g4", (4,), "DC")
    add("B16", "g5", (5,), "DE")
    add("B32", "g13", (13,), "EF")                      # class 1600
    add("B64", "g13", (13,), "F")                       # class 3136
    add("H64", "g13", (13,), "F")
    add("U8", "w6", (6,), "C")
    add("U8", "w7", (7,), "DEC")
    add("SP8", "r8", (8,), "DE")
    add("SP16", "r8", (8,), "EC")
    add("B16", "r9", (9,), "DE")
    for k in LAYOUTS:
        for mode, route, bodies in (("g3", 3, "C"), ("g4", 4, "DC"), ("g5", 5, "DE")):
            add("L" + k, mode, (route,), bodies, with_gains=False)
    for k in LAYOUTS:                                   # rpf_generic_quad_carve offers each of the three the class 1600
        add("Q" + k, "g13", (13,), "EF", with_gains=False)
    # d. the fp32 pair weights, gains as the flag allows: a scheduled pass with RPF_FLAG_FAST_WEIGHTS is refused (the scheduled
    # builds of the compiled kernels are fp64), the generic flags take RPF_FLAG_SCHEDULE: the `sched` branch of C, D and E in
    # their fp32 instantiations
    add("U8", "compiled", (0, 1), "AB", with_gains=False, fast="FAST_WEIGHTS")
    add("B32", "compiled", (2,), "A", with_gains=False, fast="FAST_WEIGHTS")
    add("B16", "g5", (5,), "DE", fast="GENERIC_FAST")
    add("U8", "g3", (3,), "C", fast="STREAM_FAST")
    add("U8", "w6", (6,), "C", fast="STREAM_FAST")
    return out


ROWS = _rows()
FRAME_IDS = sorted(set(r.fid for r in ROWS))
assert len(set(r.id for r in ROWS)) == len(ROWS)


def membership_of(row):
    """the membership test of a row's route (None: the reference's full box or the draws alone)"""
    if row.mode not in ("r10", "r9"):
        return None
    nf = frame(row.fid).lay[1]
    return MR.reference(nf) if row.mode == "r10" else P.nonref(nf)


def form_of(row):
    """the form of stage 4 of the kernels that filter a row's resident pixels (tests/stage4_bars.py): the compiled kernels
    expanded, every layout-generic kernel direct"""
    return "expanded" if row.mode in SCHEDULED_FUSED else "direct"
