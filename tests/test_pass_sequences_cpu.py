"""Box lists that return to an earlier box: the frames, the table of sequences tests/test_pass_sequences_gpu.py runs, and what that
file takes for granted about them, settled here from the oracle and the numpy restatements alone (never the library under test).

Several pieces of a context's state live for a whole call and not for one pass: the size-binned route's membership cache
(bin_valid: class counts on the host, pixel lists and acceptance masks on the device), the class counts, the grow-only member
pool and its cursor, the redo list, the uploaded sampling and membership tables.  A sequence here makes a later pass meet what an
earlier pass of another route left behind; the conditions below are what makes such a meeting able to go wrong:

* compiled-layout sequences (a size-binned box and an unbinned one): at the unbinned box at least 10 % of the pixels have
  N <= 64 -- the unbinned route then rewrites their acceptance masks, at its own stride, and the packed lists -- and at least
  10 % have S < N <= 64 (masks with bits set); at the size-binned box the pixels fall into at least three size classes, one
  of them packed and one a one-wave class; at least 10 % of the pixels have a different N at the two boxes; the mask strides
  of the two boxes differ.
* sampled sequences: at least half the pixels have N > S on every sampled pass.
* membership sequences: the full-box pass lists at least four times the members (N - S, summed over the pixels) of the sampled
  pass before it, so the member pool grows inside the call.

The frame of the compiled-layout sequences: feature_buffer.synth_planes in clustered mode, the generator arguments of
tests/test_gpu_parity.py, on the 3 x 3 pixel tiles of one colour of a checkerboard and the same generator's smooth mode with a
small jitter on the others.  Clustered mode alone has N <= 64 on at most 1 % of the pixels at these shapes (nearly every pixel
straddles both modes, so its 3-sigma band takes the whole window), and smooth mode alone leaves the colours where they were
(1e-13 relative L2 where a tenth of its pixels have N <= 64);
side by side the smooth tiles keep small neighbourhoods (their band rejects the clustered samples) while the clustered tiles
keep large ones and a filter that moves the colours."""
import collections
import functools

import numpy as np
import pytest

import member_test_ref as MR
import sampled_ref as SR
import test_listed_routes_cpu as LR
import test_schedule_cpu as SC
from raytracer_rpf_amd import feature_buffer as fb
from raytracer_rpf_amd import hip as HIP  # the flag words and Python-side helpers only: nothing here loads the library

EPS, REF_ABORT = 1, 0
SHARE = 0.10
CAPS = (8, 16, 32, 64, 128, 256, 448, 832, 1600, 3136)   # the resident classes of the compiled kernels; beyond: streaming
PACKED, ONE_WAVE = CAPS[:4], CAPS[4:8]
GPW = HIP.FLAG_GENERIC | HIP.FLAG_GENERIC_PACKED | HIP.FLAG_GENERIC_WAVE
SAMPLING_SEED = 0x5EED5EED
# tests/test_schedule_gpu.py's TWO, extended to four entries, none with a gain of 1
FOUR = dict(seed=[0.5, 0.25, 0.125, 0.0625], gain_c=[1.15, 1.3, 1.45, 1.6], gain_f=[1.6, 1.15, 1.3, 1.45])

# frame: (generator, its arguments) -- "blend": blended() below; "schedule": test_schedule_cpu.frame; "listed":
#   test_listed_routes_cpu.frame
# variants: (label, policy, options of the context); options: set on every context of every variant
Sequence = collections.namedtuple("Sequence", "name shape flags boxes draws frame sigma_seed membership schedule spike options variants")


def _seq(name, shape, flags, boxes, frame, draws=None, sigma_seed=0.002, membership=None, schedule=None, spike=False, options=(),
         variants=(("eps", EPS, ()),)):
    return Sequence(name, shape, flags, boxes, draws, frame, sigma_seed, membership, schedule, spike, tuple(options), tuple(variants))


BLEND = ("blend", dict(seed=12, sigma_f=4e-3))
_W, _H = LR.frame()[0].shape[2], LR.frame()[0].shape[1]
SEQUENCES = collections.OrderedDict((s.name, s) for s in (
    # binned, unbinned, cached-or-not
    _seq("aba16", (15, 11, 16), 0, (7, 5, 7), BLEND, variants=(("eps", EPS, ()), ("ref_abort", REF_ABORT, ()))),
    _seq("aba8", (15, 11, 8), 0, (9, 7, 9), BLEND,
         variants=(("eps", EPS, ()), ("count_first0", EPS, (("count_first", 0),)), ("count_first1", EPS, (("count_first", 1),)),
                   ("packed0", EPS, (("packed", 0),)))),
    # legitimate reuse, invalidation, recount, reuse again
    _seq("aabab16", (15, 11, 16), 0, (7, 7, 5, 7, 7), BLEND),
    # unbinned, binned, unbinned
    _seq("bab8", (15, 11, 8), 0, (7, 9, 7), BLEND),
    # route 8, binned, route 8, binned recount
    _seq("s-bin", (12, 12, 8), HIP.SAMPLED_NBHD_FLAG, (9, 9, 9, 9), ("schedule", dict(seed=3)), draws=(40, 0, 40, 0)),
    # route 5, route 8, route 5
    _seq("s-gpw", (12, 12, 8), HIP.SAMPLED_NBHD_FLAG | GPW, (7, 7, 7), ("schedule", dict(seed=3)), draws=(0, 40, 0)),
    # routes 8, 9, 8
    _seq("s-mem", (12, 12, 8), HIP.SAMPLED_NBHD_FLAG | HIP.MEMBER_TEST_FLAG, (7, 7, 7), ("schedule", dict(seed=3, flat_frac=0.94)),
         draws=(40, 0, 40), membership="published19", variants=(("eps", EPS, ()), ("wide_pool1", EPS, (("wide_pool", 1),)))),
    # route 7 back to 7
    _seq("w-back", (_W, _H, LR.S), HIP.FLAG_WIDE_NBHD | HIP.FLAG_WIDE_CLASSES, (LR.BOX, 7, LR.BOX), ("listed", {}),
         sigma_seed=LR.P.ACTIVE_SIGMA_SEED, options=(("wide", 1),)),
    # the one-call published pipeline: routes 8, 8, 9, 9, then the spike pass
    _seq("pipeline", (14, 12, 8), HIP.SAMPLED_NBHD_FLAG | HIP.MEMBER_TEST_FLAG | HIP.SCHEDULE_FLAG | HIP.FLAG_SPIKE_CLAMP, (11, 7, 5, 5),
         ("schedule", dict(seed=3, flat_frac=0.94)), draws=(64, 40, 0, 0), membership="published19", schedule=FOUR, spike=True),
))
COMPILED = [n for n, s in SEQUENCES.items() if s.flags == 0]
SAMPLED = [n for n, s in SEQUENCES.items() if s.flags & HIP.SAMPLED_NBHD_FLAG]
MEMBER = [n for n, s in SEQUENCES.items() if s.flags & HIP.MEMBER_TEST_FLAG]
CASES = [(n, v[0]) for n, s in SEQUENCES.items() for v in s.variants]


@functools.lru_cache(maxsize=None)
def blended(W, H, S, seed, sigma_f):
    """clustered tiles (the arguments of tests/test_gpu_parity.py) and smooth tiles of jitter sigma_f, 3 x 3 pixels each: read-only"""
    a = fb.synth_planes(W, H, S, seed=seed, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    b = fb.synth_planes(W, H, S, seed=seed, sigma_f=sigma_f, sigma_c=0.01, mode="smooth")
    yy, xx = np.mgrid[0:H, 0:W]
    p = np.where(((xx // 3 + yy // 3) % 2 == 0)[None, :, :, None], a, b)
    p.setflags(write=False)
    return p


def planes_of(name):
    """the frame of a sequence: built once, read-only"""
    s = SEQUENCES[name]
    W, H, S = s.shape
    kind, kw = s.frame
    if kind == "blend":
        return blended(W, H, S, **kw)
    if kind == "schedule":
        return SC.frame(W, H, S, **kw)
    assert kind == "listed"
    return LR.frame()[0]


def variant_of(name, label):
    """(policy, options of the context: the sequence's, then the variant's)"""
    s = SEQUENCES[name]
    _, policy, opts = next(v for v in s.variants if v[0] == label)
    return policy, s.options + tuple(opts)


def membership_of(name):
    """the (mult, floor) of the restatement, or None"""
    return MR.published19() if SEQUENCES[name].membership == "published19" else None


def binned(box, S):
    return box * box * S > 512


def mask_stride(box, S):
    """u64 acceptance masks per pixel of a pass on the compiled kernels: one bit per candidate of the window"""
    return max(1, ((box * box - 1) * S + 63) // 64)


def class_of(n):
    return next((c for c in CAPS if n <= c), CAPS[-1] + 1)


_sizes = {}


def sizes(oracle, name, box):
    """N of every pixel of the sequence's frame at a box by the oracle (it depends on the features only): computed once, shared"""
    s = SEQUENCES[name]
    key = (s.shape, s.frame[0], tuple(sorted(s.frame[1].items())), box)
    if key not in _sizes:
        W, H, S = s.shape
        _sizes[key] = oracle.filter_pass(planes_of(name), oracle.make_desc(W, H, S, box=box, policy=EPS))["nbhd_size"]
    return _sizes[key]


_listed = {}


def listed_sizes(oracle, name, p):
    """N of every pixel on pass p of a sampled and / or membership sequence, by the restatements"""
    if (name, p) not in _listed:
        s = SEQUENCES[name]
        mt, D, box = membership_of(name), (s.draws[p] if s.draws else 0), s.boxes[p]
        cfg = (SAMPLING_SEED, 0, D) if D > 0 else None
        if mt is not None:
            n, _ = MR.counts(oracle, planes_of(name), mt, box, cfg=cfg, pass_id=p)
        else:
            assert cfg is not None
            n = SR.sampled_pass(oracle, planes_of(name), cfg, pass_id=p, box=box, weights=False)["nbhd_size"]
        _listed[name, p] = n
    return _listed[name, p]


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def test_table_shape():
    assert list(SEQUENCES) == ["aba16", "aba8", "aabab16", "bab8", "s-bin", "s-gpw", "s-mem", "w-back", "pipeline"]
    for name, s in SEQUENCES.items():
        W, H, S = s.shape
        assert planes_of(name).shape == (19, H, W, S) and planes_of(name).dtype == np.float32 and not planes_of(name).flags.writeable
        assert 1 <= len(s.boxes) <= HIP.MAX_BOXES and all(b % 2 == 1 for b in s.boxes)
        assert s.draws is None or len(s.draws) == len(s.boxes)
        assert (s.draws is not None) == bool(s.flags & HIP.SAMPLED_NBHD_FLAG)
        assert (s.membership is not None) == bool(s.flags & HIP.MEMBER_TEST_FLAG)
        assert (s.schedule is not None) == bool(s.flags & HIP.SCHEDULE_FLAG) and s.spike == bool(s.flags & HIP.FLAG_SPIKE_CLAMP)
        if name != "w-back":
            assert W <= 15 and H <= 12, name
        # every sequence returns to a box, or to a route, it has left
        assert any(s.boxes[i] == s.boxes[j] and any(b != s.boxes[i] for b in s.boxes[i + 1:j])
                   for i in range(len(s.boxes)) for j in range(i + 2, len(s.boxes))) or (s.draws and len(set(s.draws)) > 1), name
    assert all(len(v) == 4 and all(g != 1.0 for g in v) for k, v in FOUR.items() if k != "seed")
    assert FOUR["seed"][:2] == [0.5, 0.25] and FOUR["gain_c"][:2] == [1.15, 1.3] and FOUR["gain_f"][:2] == [1.6, 1.15]


def test_compiled_sequences_alternate_between_the_binned_and_the_unbinned_route():
    want = {"aba16": [1, 0, 1], "aba8": [1, 0, 1], "aabab16": [1, 1, 0, 1, 1], "bab8": [0, 1, 0]}
    for name in COMPILED:
        s = SEQUENCES[name]
        assert [int(binned(b, s.shape[2])) for b in s.boxes] == want[name], name
        small, large = min(s.boxes), max(s.boxes)
        assert mask_stride(small, s.shape[2]) != mask_stride(large, s.shape[2])   # a mask kept from one is misread by the other
    assert [int(binned(b, 8)) for b in SEQUENCES["s-bin"].boxes] == [1, 1, 1, 1]   # its unsampled passes are size-binned


# ---- compiled-layout sequences -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", COMPILED)
def test_compiled_frames_can_show_a_stale_cache(oracle, name):
    s = SEQUENCES[name]
    S = s.shape[2]
    small, large = min(s.boxes), max(s.boxes)
    ns, nl = sizes(oracle, name, small), sizes(oracle, name, large)
    rewritten, with_bits, differ = float((ns <= 64).mean()), float(((ns > S) & (ns <= 64)).mean()), float((ns != nl).mean())
    classes = sorted({class_of(int(v)) for v in nl.ravel()})
    print("SEQUENCE %s: box %d: N <= 64 on %.3f of the pixels, S < N <= 64 on %.3f | box %d: classes %s | N differs on %.3f" % (
        name, small, rewritten, with_bits, large, classes, differ))
    assert not binned(small, S) and binned(large, S)
    assert rewritten >= SHARE and with_bits >= SHARE and differ >= SHARE
    assert len(classes) >= 3 and set(classes) & set(PACKED) and set(classes) & set(ONE_WAVE)


@pytest.mark.parametrize("name", ["aba16", "aba8"])
def test_compiled_frames_move_under_the_oracle(oracle, name):
    """the chain of oracle passes the GPU file compares with is not the identity on these frames"""
    s = SEQUENCES[name]
    W, H, S = s.shape
    planes, c = planes_of(name), None
    for box in s.boxes:
        c = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=box, policy=EPS), colour_in=c, debug=False)["colour"]
    cin = planes[2:5].astype(np.float64)
    moved = float(np.linalg.norm(c - cin) / np.linalg.norm(cin))
    print("SEQUENCE %s: the oracle's chain moves the colours by %.3e relative L2" % (name, moved))
    assert moved > 1e-3 and np.isfinite(c).all()


# ---- sampled sequences ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SAMPLED)
def test_sampled_passes_find_neighbours(oracle, name):
    s = SEQUENCES[name]
    S = s.shape[2]
    assert all(S + d <= 832 for d in s.draws)
    for p, d in enumerate(s.draws):
        if d == 0:
            continue
        n = listed_sizes(oracle, name, p)
        share = float((n > S).mean())
        print("SEQUENCE %s pass %d (box %d, %d draws): N %d .. %d, N > S on %.3f of the pixels" % (name, p, s.boxes[p], d, n.min(), n.max(), share))
        assert share >= 0.5 and n.max() <= S + d


# ---- membership sequences ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MEMBER)
def test_full_box_pass_outgrows_the_sampled_pass_before_it(oracle, name):
    s = SEQUENCES[name]
    S = s.shape[2]
    p = next(i for i in range(1, len(s.boxes)) if s.draws[i] == 0 and s.draws[i - 1] > 0)
    before, full = listed_sizes(oracle, name, p - 1), listed_sizes(oracle, name, p)
    listed_before, listed_full = int((before - S).sum()), int((full - S).sum())
    print("SEQUENCE %s: pass %d lists %d members, the full-box pass %d lists %d (%.1f times)" % (
        name, p - 1, listed_before, p, listed_full, listed_full / max(listed_before, 1)))
    assert listed_before > 0 and listed_full >= 4 * listed_before
    assert listed_full > 8 * before.size    # more than the pool's first size of eight entries per pixel


# ---- the wide sequence -----------------------------------------------------------------------------------------------------------------
def test_wide_sequence_changes_its_classes_between_the_boxes(oracle):
    """w-back: the middle pass deals the pixels of test_listed_routes_cpu's frame into other classes than the passes around it"""
    full = LR.full_box(oracle, EPS)["nbhd_size"]
    mid = sizes(oracle, "w-back", 7)
    a, b = LR.class_fill(full), LR.class_fill(mid)
    differ = float((full != mid).mean())
    print("SEQUENCE w-back: class fill at box %d %s, at box 7 %s, N differs on %.3f of the pixels" % (LR.BOX, a, b, differ))
    assert a != b and differ >= SHARE
