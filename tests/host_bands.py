"""The row-band host pipeline (rpf_filter from page-locked buffers: run_host_pipeline in csrc/rpf_api.hip) held to the serial call:
the cut into bands restated, the documented launch rule applied per band, the frames and cases tests/test_host_bands_gpu.py runs,
and the independent reference of each case.  A plain helper module, no GPU: tests/test_host_bands_cpu.py settles what the GPU
file takes for granted about the frames, from the oracle and the numpy restatements alone.

The first and the last pass of a banded call are filtered band by band -- one route_pass per band, so one count-and-deal step,
one set of class lists, masks and counts, one redo count, one probe per band -- and a middle pass once over the slab."""
import collections
import functools

import numpy as np

import member_test_ref as MR
import sampled_ref as SR
import schedule_ref as SRf
import test_pass_sequences_cpu as T
import test_schedule_cpu as SC
from raytracer_rpf_amd import feature_buffer as fb
from raytracer_rpf_amd import hip as HIP  # the flag words and Python-side helpers only: nothing here loads the library

EPS, REF_ABORT = 1, 0
CAPS = (8, 16, 32, 64, 128, 256, 448, 832)   # the capacities of the size classes of routes 4 / 5 / 7 / 8 / 9
REST = 833                                   # the name of the rest list in a case's `classes`
SAMPLING_SEED = T.SAMPLING_SEED
RAY_WEIGHT_SEED = 1

G = HIP.FLAG_GENERIC
GP = G | HIP.FLAG_GENERIC_PACKED
GPW = GP | HIP.FLAG_GENERIC_WAVE
WIDE = HIP.FLAG_WIDE_NBHD
WIDE_CLASSES = WIDE | HIP.FLAG_WIDE_CLASSES
L19, L27, L37, L37H = (2, 12, "f32"), (4, 18, "f16"), (3, 7, "f32"), (3, 7, "f16")
# tests/test_schedule_gpu.py's TWO: a different entry per pass, no gain of 1
TWO = dict(seed=[0.5, 0.25], gain_c=[1.15, 1.3], gain_f=[1.6, 1.15])


# ---- the cut ---------------------------------------------------------------------------------------------------------------------
def bands(H, boxes):
    """the row bands [(r0, r1), ...] of a frame of H rows under a box list: about eight, never thinner than 16 rows or than the
    halo of the first or the last box, whichever is widest (run_host_pipeline)"""
    min_rows = max(16, (boxes[0] - 1) // 2, (boxes[-1] - 1) // 2)
    nb0 = min(8, max(1, H // min_rows))
    bh = -(-H // nb0)
    nb = -(-H // bh)
    return [(j * bh, min(H, (j + 1) * bh)) for j in range(nb)]


def band_of(y, cut):
    return next(j for j, (r0, r1) in enumerate(cut) if r0 <= y < r1)


# ---- the launch rule -----------------------------------------------------------------------------------------------------------
def class_fill(n, route):
    """pixels per list of a class-routed pass over the sizes n: the classes of the route, then its rest list.  Route 4 deals into
    the four packed classes and lists N > 64; routes 5 / 7 / 8 / 9 into all eight and list N > 832"""
    n = np.asarray(n).ravel()
    caps = CAPS[:4] if route == 4 else CAPS
    edges = (0,) + caps
    return [int(((n > lo) & (n <= hi)).sum()) for lo, hi in zip(edges[:-1], edges[1:])] + [int((n > caps[-1]).sum())]


def pass_launches(route, n, policy):
    """rpf_hip.h, the comment above rpf_query_counters, for ONE route_pass over the pixels whose sizes are n (not empty): routes 3
    and 6 one launch; routes 4 / 5 / 7 / 8 / 9 one per non-empty class and one for a non-empty rest list; under REF_ABORT one
    redo launch on routes 4 / 5 / 7.  None for a pass on the compiled kernels (routes 0 / 1 / 2: the rule there depends on options
    and on a probe, and the GPU file asks for more launches than the serial call instead)"""
    if route in (3, 6):
        return 1
    if route not in (4, 5, 7, 8, 9):
        return None
    return sum(1 for k in class_fill(n, route) if k) + (1 if policy == REF_ABORT and route in (4, 5, 7) else 0)


def expected_launches(route, nbhd_last_by_pass, cut, policy, rows=None):
    """filter_kernel_launches of a call: the rule per band for the first and the last pass and once for a middle pass.  route: one
    route, or one per pass; nbhd_last_by_pass: the N map [H, W] of every pass, by the reference; cut: bands(); rows: the slab
    (row_begin, row_end) -- a band without a row of the slab launches nothing.  None when a pass runs on the compiled kernels"""
    n_pass = len(nbhd_last_by_pass)
    routes = [route] * n_pass if np.isscalar(route) else list(route)
    H = nbhd_last_by_pass[0].shape[0]
    a, b = rows if rows is not None else (0, H)
    total = 0
    for p, (r, n) in enumerate(zip(routes, nbhd_last_by_pass)):
        pieces = cut if p in (0, n_pass - 1) else [(0, H)]
        for r0, r1 in pieces:
            r0, r1 = max(r0, a), min(r1, b)
            if r1 <= r0:
                continue
            k = pass_launches(r, n[r0:r1], policy)
            if k is None:
                return None
            total += k
    return total


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# routes: the route of every pass as rpf_query_route names it (0: the compiled kernels, whichever of 0 / 1 / 2 the pass takes)
# classes: the lists the case is there for (capacities, REST), each non-empty in at least two bands -- REST in at least one
Case = collections.namedtuple("Case", "name lay shape boxes flags policy frame options draws membership schedule rows sigma_seed routes classes")


def _case(name, lay, shape, boxes, flags, policy, frame, routes, options=(), draws=None, membership=None, schedule=None, rows=None,
          sigma_seed=0.002, classes=()):
    return Case(name, lay, shape, tuple(boxes), flags, policy, frame, tuple(options), draws, membership, schedule, rows, sigma_seed,
                tuple(routes), tuple(classes))


_MEM = HIP.SAMPLED_NBHD_FLAG | HIP.MEMBER_TEST_FLAG
CASES = collections.OrderedDict((c.name, c) for c in (
    _case("fused19-ra", L19, (5, 48, 15), (9,), 0, REF_ABORT, "planted", (0,), sigma_seed=0.5),
    _case("fused19-nonfinite", L19, (6, 48, 8), (7,), 0, REF_ABORT, "constant", (0,)),
    _case("fused19-nan", L19, (8, 48, 8), (7,), 0, EPS, "nan", (0,)),
    _case("fused27", L27, (6, 48, 8), (7, 5), 0, EPS, "clustered", (0, 0)),
    _case("fused27-split", L27, (4, 48, 32), (7, 5), 0, EPS, "clustered", (0, 0)),
    _case("g3", L37H, (6, 50, 8), (7, 5), G, EPS, "clustered", (3, 3)),
    _case("g4", L37, (8, 48, 8), (7, 5, 7), GP, EPS, "blend", (4, 4, 4), classes=(16, 32, 64, REST)),
    _case("g5", L37, (8, 48, 8), (7, 5, 7), GPW, EPS, "blend", (5, 5, 5), classes=(16, 32, 64, 128, 256, 448)),
    _case("g5-ra", L19, (5, 48, 15), (9,), GPW, REF_ABORT, "planted", (5,), sigma_seed=0.5, classes=(448, 832)),
    _case("g5-fast", L37H, (8, 48, 8), (7, 5), GPW | HIP.FLAG_GENERIC_FAST | HIP.FLAG_STREAM_FAST, EPS, "blend", (5, 5),
          classes=(16, 32, 64, 128, 256, 448)),
    _case("g5-slab", L37, (8, 48, 8), (7,), GPW, EPS, "blend", (5,), rows=(10, 41), classes=(16, 32, 64, 128, 256, 448)),
    _case("wide6", L19, (4, 81, 22), (55,), WIDE, EPS, "groups", (6,), sigma_seed=0.5),
    _case("wide7", L19, (4, 81, 22), (55,), WIDE_CLASSES, EPS, "groups", (7,), sigma_seed=0.5, classes=(32, 64, 128, 256, 448, 832, REST)),
    _case("wide7-mixed", L19, (4, 81, 22), (55, 7), WIDE_CLASSES, EPS, "groups", (7, 0), sigma_seed=0.5),
    _case("wide7-hook", L19, (8, 48, 8), (7, 5, 7), WIDE_CLASSES, EPS, "blend", (7, 7, 7), options=(("wide", 1),),
          classes=(16, 32, 64, 128, 256, 448)),
    _case("wide7-hook-pool1", L19, (8, 48, 8), (7, 5, 7), WIDE_CLASSES, EPS, "blend", (7, 7, 7), options=(("wide", 1), ("wide_pool", 1)),
          classes=(16, 32, 64, 128, 256, 448)),
    _case("wide7-ra", L19, (5, 48, 15), (9,), WIDE_CLASSES, REF_ABORT, "planted", (7,), options=(("wide", 1),), sigma_seed=0.5,
          classes=(448, 832)),
    _case("s8", L19, (6, 48, 8), (17, 7), HIP.SAMPLED_NBHD_FLAG, EPS, "smooth", (8, 8), draws=(120, 24), sigma_seed=0.5,
          classes=(16, 32, 64, 128)),
    _case("s8-mixed", L19, (6, 48, 8), (7, 7), HIP.SAMPLED_NBHD_FLAG, EPS, "smooth", (8, 0), draws=(24, 0), sigma_seed=0.5),
    _case("s-mem", L19, (6, 48, 8), (7, 7, 7), _MEM, EPS, "flat-band0", (8, 9, 8), draws=(40, 0, 40), membership="published19",
          sigma_seed=0.5, classes=(16, 32, 64)),
    _case("s-mem-pool1", L19, (6, 48, 8), (7, 7, 7), _MEM, EPS, "flat-band0", (8, 9, 8), options=(("wide_pool", 1),), draws=(40, 0, 40),
          membership="published19", sigma_seed=0.5, classes=(16, 32, 64)),
    _case("sched", L19, (8, 48, 8), (7, 5), GPW | HIP.SCHEDULE_FLAG, EPS, "smooth", (5, 5), schedule=TWO, classes=(128, 256, 448)),
    _case("lastband", L19, (4, 52, 4), (35,), 0, EPS, "clustered", (0,)),
))
CLASS_ROUTED = [n for n, c in CASES.items() if c.classes]
RA_CASES = ("fused19-ra", "g5-ra", "wide7-ra")
BLEND_SEED, BLEND_SIGMA_F = 12, 4e-3
CLUSTERED = dict(sigma_f=1e-3, sigma_c=0.01, mode="clustered")
FRAME_SEED = 21
NAN_AT, INF_AT = (16, 4, 3), (16, 1, 5)         # (y, x, s) of the NaN normal and of the +inf feature of the "nan" frame
GROUP_SIZES = (1, 2, 4, 9, 16, 30, 44)          # pixels per group of the "groups" frame: N = 22 * the group's pixels in the window


def blended(lay, W, H, S, seed=BLEND_SEED, sigma_f=BLEND_SIGMA_F):
    """test_pass_sequences_cpu.blended for any layout: clustered tiles and smooth tiles of jitter sigma_f, 3 x 3 pixels each"""
    nr, nf, dt = lay
    if lay == L19:
        return T.blended(W, H, S, seed, sigma_f)
    a = fb.synth_planes(W, H, S, seed=seed, sigma_f=1e-3, sigma_c=0.01, mode="clustered", n_random=nr, n_feat=nf, dtype=dt)
    b = fb.synth_planes(W, H, S, seed=seed, sigma_f=sigma_f, sigma_c=0.01, mode="smooth", n_random=nr, n_feat=nf, dtype=dt)
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where(((xx // 3 + yy // 3) % 2 == 0)[None, :, :, None], a, b)


def planted_independent(W, H, S):
    """the frame of test_gpu_parity.test_independent_tables_in_every_size_class_ref_abort at another shape: every pixel carries an
    exactly independent (f0, r0) table, every neighbour passes every 3-sigma test, so N = S * (pixels of the window)"""
    from test_gpu_parity import _independent_columns
    rng = np.random.default_rng(17)
    planes = rng.permuted(np.broadcast_to(np.linspace(0.4, 0.6, S), (19, H, W, S)), axis=3).astype(np.float32)
    planes[0] = (np.arange(W)[None, :, None] + rng.random((H, W, S))).astype(np.float32)
    planes[1] = (np.arange(H)[:, None, None] + rng.random((H, W, S))).astype(np.float32)
    a, b = _independent_columns(S, 3)
    planes[5], planes[7] = a.astype(np.float32), b.astype(np.float32)
    return planes


def group_frame(W, H, S):
    """a planted_nbhd-style frame for a window taller than a band: every column of every pixel is a permutation of the same S
    values, and the pixels are dealt, in raster order, into groups of GROUP_SIZES pixels (repeated); the first feature of a group
    lies 10 away from every other group's, so a pixel's neighbourhood is the pixels of its own group inside its window"""
    rng = np.random.default_rng(5)
    planes = rng.permuted(np.broadcast_to(np.linspace(0.4, 0.6, S), (19, H, W, S)), axis=3).astype(np.float32)
    planes[0] = (np.arange(W)[None, :, None] + rng.random((H, W, S))).astype(np.float32)
    planes[1] = (np.arange(H)[:, None, None] + rng.random((H, W, S))).astype(np.float32)
    planes[2:5] = rng.random((3, H, W, S)).astype(np.float32)
    group, g, left = np.empty(W * H, np.int64), 0, 0
    for i in range(W * H):
        if left == 0:
            g, left = g + 1, GROUP_SIZES[g % len(GROUP_SIZES)]
        group[i], left = g, left - 1
    planes[7] += np.float32(10.0) * group.reshape(H, W, 1).astype(np.float32)
    return planes


@functools.lru_cache(maxsize=None)
def _frame(kind, lay, shape, boxes):
    W, H, S = shape
    nr, nf, dt = lay
    lay_kw = dict(n_random=nr, n_feat=nf, dtype=dt)
    if kind == "planted":
        p = planted_independent(W, H, S)
    elif kind == "constant":
        # test_gpu_parity.test_ref_abort_status_on_constant_feature, extended: the constant normal on the first and the last ten
        # rows, so that the rows between keep finite colours
        p = fb.synth_planes(W, H, S, seed=5)
        for rows in (slice(0, 10), slice(H - 10, H)):
            p[7:10, rows] = np.float32([0.0, 0.0, 1.0])[:, None, None, None]
    elif kind == "nan":
        p = fb.synth_planes(W, H, S, seed=5, sigma_f=0.05, sigma_c=0.01, mode="smooth", flat_frac=0.5)
        y, x, s = NAN_AT
        p[7:10, y, x, s] = np.nan       # a NaN normal: the one candidate a flat pixel's zero-variance features accept
        y, x, s = INF_AT
        p[7, y, x, s] = np.inf
    elif kind == "clustered":
        p = fb.synth_planes(W, H, S, seed=FRAME_SEED, **CLUSTERED, **lay_kw)
    elif kind == "smooth":
        p = np.array(SC.frame(W, H, S, seed=3))
    elif kind == "blend":
        p = np.array(blended(lay, W, H, S))
    elif kind == "groups":
        p = group_frame(W, H, S)
    else:
        assert kind == "flat-band0"
        # flat quads in band 0 only, their first normal component half a unit apart on the two colours of a checkerboard: under
        # the published test a flat pixel accepts the flat pixels of its own colour (the floor is 0.1) and lists about half of
        # what a pixel of the other bands lists
        flat, plain = SC.frame(W, H, S, seed=3, flat_frac=0.94), SC.frame(W, H, S, seed=3)
        r1 = bands(H, boxes)[0][1]
        p = np.concatenate([flat[:, :r1], plain[:, r1:]], axis=1)
        yy, xx = np.mgrid[0:r1, 0:W]
        p[7, :r1] += np.float32(0.5) * ((xx + yy) % 2).astype(np.float32)[:, :, None]
    p = np.ascontiguousarray(p)
    p.setflags(write=False)
    return p


def planes_of(name):
    """the stored planes of a case (fp32 or fp16): built once, read-only"""
    c = CASES[name]
    return _frame(c.frame, c.lay, c.shape, c.boxes)


def p32_of(name):
    """their exact fp32 image: what the oracle and the restatements read"""
    return planes_of(name).astype(np.float32)


def ray_weight_of(name):
    W, H, S = CASES[name].shape
    return (0.5 + np.random.default_rng(RAY_WEIGHT_SEED).random((H, W, S))).astype(np.float32)


def cut_of(name):
    c = CASES[name]
    return bands(c.shape[1], c.boxes)


def membership_of(name):
    return MR.published19() if CASES[name].membership == "published19" else None


def layout_kw(name):
    nr, nf, _ = CASES[name].lay
    return dict(n_random=nr, n_feat=nf) if (nr, nf) != (2, 12) else {}


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def is_pow2(n):
    return (n & (n - 1)) == 0


_reference = {}


def reference(oracle, name):
    """the independent reference of a case: the chain of its passes, each fed the fp64 colours of the one before -- the oracle's
    filter pass; for a sampled pass, a pass under the membership test or a scheduled pass, the numpy restatement the GPU tests of
    that flag use.  dict: colour [3, H, W, S] fp64, nbhd (the N map of every pass), status (1: a non-finite colour under
    REF_ABORT), nonfinite_pixels (all passes), first_bad_pixel, redo_pixels (the last pass's: the pixels of the slab with an
    exactly independent histogram pair at an N that is no power of two, on a route that keeps a redo list).  Computed once."""
    if name in _reference:
        return _reference[name]
    c = CASES[name]
    W, H, S = c.shape
    p32, mt, lay = p32_of(name), membership_of(name), layout_kw(name)
    r0, r1 = c.rows if c.rows else (0, H)
    colour, nbhd, status, bad, first = None, [], 0, 0, -1
    last = None
    for p, box in enumerate(c.boxes):
        D = c.draws[p] if c.draws else 0
        cfg = (SAMPLING_SEED, 0, D) if D > 0 else None
        if c.schedule is not None:
            entry = (c.schedule["seed"][p], c.schedule["gain_c"][p], c.schedule["gain_f"][p])
            r = SRf.scheduled_pass(oracle, p32, entry, box, policy=c.policy, colour64=colour, mt=mt, cfg=cfg, pass_id=p)
        elif mt is not None:
            r = MR.member_pass(oracle, p32, mt, box, seed_sigma=c.sigma_seed, policy=c.policy, colour64=colour, cfg=cfg, pass_id=p)
        elif cfg is not None:
            r = SR.sampled_pass(oracle, p32, cfg, p, box, seed_sigma=c.sigma_seed, policy=c.policy, colour64=colour)
        else:
            r = oracle.filter_pass(p32, oracle.make_desc(W, H, S, box=box, row_begin=r0, row_end=r1, policy=c.policy,
                                                         sigma_seed=c.sigma_seed, **lay), colour_in=colour)
            status = max(status, int(r["status"]))
            if r["nonfinite_pixels"]:
                first = int(r["first_bad_pixel"]) if first < 0 else min(first, int(r["first_bad_pixel"]))
            bad += int(r["nonfinite_pixels"])
        colour, last = r["colour"], r
        nbhd.append(np.array(r["nbhd_size"]))
    redo = 0
    if c.policy == REF_ABORT and c.routes[-1] in (0, 4, 5, 7):
        redo = int(redo_map(oracle, name)[r0:r1].sum())
    colour.setflags(write=False)
    _reference[name] = dict(colour=colour, nbhd=nbhd, status=status, nonfinite_pixels=bad, first_bad_pixel=first, redo_pixels=redo,
                            last=last)
    return _reference[name]


_redo = {}


def redo_map(oracle, name):
    """[H, W] bool: the pixels of a one-pass REF_ABORT case that the reference-expression kernel filters again -- N no power of
    two and a histogram pair that is exactly independent, which under the EPS policy is an MI of exactly 0 on the oracle's side
    (the residue contract of oracle/rpf_oracle.c, mi_scratch)"""
    if name not in _redo:
        c = CASES[name]
        assert len(c.boxes) == 1 and c.policy == REF_ABORT
        W, H, S = c.shape
        e = oracle.filter_pass(p32_of(name), oracle.make_desc(W, H, S, box=c.boxes[0], policy=EPS, sigma_seed=c.sigma_seed, **layout_kw(name)))
        n = e["nbhd_size"]
        _redo[name] = (~is_pow2(n)) & (e["mi"] == 0).any(axis=-1)
    return _redo[name]


def banded_passes(name):
    """the passes of a case that run band by band: the first and the last"""
    return sorted({0, len(CASES[name].boxes) - 1})


def band_fill(oracle, name, p):
    """per band of pass p: the pixels per list (class_fill) of the band's rows inside the slab"""
    c = CASES[name]
    n = reference(oracle, name)["nbhd"][p]
    a, b = c.rows if c.rows else (0, c.shape[1])
    return [class_fill(n[max(r0, a):min(r1, b)], c.routes[p] if c.routes[p] in (4, 5, 7, 8, 9) else 5) for r0, r1 in cut_of(name)]


def member_rows(oracle, name, p, y, x):
    """the image rows of the members of pixel (y, x) on pass p, by the numpy restatement of the pass's membership"""
    c = CASES[name]
    W, H, S = c.shape
    nr, nf, _ = c.lay
    p32 = p32_of(name)
    pmean, pstd = MR.stats_of(oracle, p32, EPS, nr, nf)
    box, D = c.boxes[p], (c.draws[p] if c.draws else 0)
    mt = membership_of(name)
    cfg = (SAMPLING_SEED, 0, D) if D > 0 else None
    _, codes = MR.members(p32, pmean, pstd, mt if mt is not None else MR.reference(nf), y, x, box, nr, nf, None, cfg, p)
    return y - (box - 1) // 2 + (np.asarray(codes) // S) % box


def pool_need(oracle, name, p):
    """per band of pass p of a listed-member case: the pool entries its count step lists (N - S over the band's pixels)"""
    S = CASES[name].shape[2]
    n = reference(oracle, name)["nbhd"][p]
    return [int((n[r0:r1] - S).sum()) for r0, r1 in cut_of(name)]
