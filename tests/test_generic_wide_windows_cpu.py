"""Windows of 65 to 1024 acceptance words on the generic class routes (rpf_query_route 3, 4, 5 and 13): the
frames of tests/test_generic_wide_windows_gpu.py, built here and imported there, and -- against the oracle and in numpy, no device
-- what that file takes for granted about them, so that a GPU failure is never a property of the input.

Every frame is one row of planted windows (tests/planted_nbhd.py), H = box, and is filtered and compared on the TARGET ROW only
(row_begin = ty, row_end = ty + 1 on the device and in the oracle): the targets carry the planted N, the other pixels of the row
have pushed own samples and N in the thousands to tens of thousands -- the rest list's work, and the oracle's cost.

What a wide window exercises and a narrow one cannot (csrc/rpf_generic_quad.hip stage 1b, rpf_generic_wave.hip, rpf_generic_packed.hip,
generic::nbhd_count_kernel): the 64-words-a-step prefix of the word popcounts with its carry, the 256-thread popcount stride, the
deal of words to four waves, the clamp at 1024 words, the serial walk and the rank select over hundreds of words, and a stride
much longer than the words a frame-clipped window writes.  A wrong prefix or base leaves nbhd_size right and the members in the
wrong slots, so the frames must place members where each of these would show: the occupancy conditions below are that argument.
The visiting order is restated here in numpy (make_window / candidate_offset of csrc/rpf_generic_common.h) and pinned by the
oracle's member_hash."""
import hashlib

import numpy as np
import pytest

import planted_nbhd as P
from test_generic_quad_cpu import CAPS, class_counts
from test_generic_wave_cpu import lay_ids, stored_and_image

EPS, REF_ABORT = 1, 0

# id: S, box, placement (None: centre; (ty, dx): plant(at=...)), planted N per target, seed
FRAMES = {
    "B17": (16, 17, None, P.FRAMES["B17"][3], P.FRAMES["B17"][4]),          # planted_nbhd's own frame, (2, 12, f32)
    "W31": (8, 31, None, (8, 64, 65, 832, 833, 1600, 1601, 3136, 3137), 0),
    "W55": (8, 55, None, (64, 832, 833, 1600, 1601, 3136, 3137), 0),
    "W181": (2, 181, None, (832, 1600, 3136), 0),                           # box * box * S = 65522: 1024 words, the clamp
    "C55": (8, 55, (0, 27), (832, 1600, 3136), 0),                          # top edge: 28 of 55 window rows
    "K55": (8, 55, (0, 0), (1600,), 0),                                     # corner: 28 x 28 window pixels
}
LAYOUTS = {
    "B17": [(2, 12, "f32")],
    "W31": [(3, 7, "f32"), (4, 18, "f16"), (8, 27, "f16")],                 # histograms per wave 2, 1, 4; the last has no class 3136
    "W55": [(3, 7, "f32"), (4, 18, "f16")],
    "W181": [(3, 7, "f32")],
    "C55": [(3, 7, "f32")],
    "K55": [(3, 7, "f32")],
}
DEFAULT_LAY = (3, 7, "f32")
CASES = [(fid, lay) for fid, lays in LAYOUTS.items() for lay in lays]
CASE_IDS = ["%s-%s" % (fid, lay_ids(lay)) for fid, lay in CASES]
# acceptance words of a pixel's stride (mask_stride of csrc/rpf_api_routes.hip) and of the targets' windows where the frame clips them
STRIDE = {"B17": 72, "W31": 120, "W55": 378, "W181": 1024, "C55": 378, "K55": 378}
CLIPPED_NWORDS = {"C55": 193, "K55": 98}
QD_MAX_WORDS = 1024                                                         # kQdMaxWords of csrc/rpf_generic_quad.hip
ACTIVE_FRAMES = ("W31", "W55", "C55")                                       # run at P.ACTIVE_SIGMA_SEED as well
# the frame whose count pass leaves full words behind for the stale-word test: Q40's geometry (40 spp, box 9), nothing pushed -- every
# candidate of every window passes -- and wide enough that its mask buffer covers the target rows of C55 and K55
DENSE = (40, 9, (3240,) * 16)


def mask_stride(box, S):
    return max(1, ((box * box - 1) * S + 63) // 64)


def geometry(fid):
    S, box, _, targets, _ = FRAMES[fid]
    return box * len(targets), box, S, box       # W, H, S, box


def target_row(fid):
    _, box, at, _, _ = FRAMES[fid]
    return (box - 1) // 2 if at is None else at[0]


_frames = {}


def frame(fid, lay):
    """(stored planes, fp32 image, target pixels) of a frame: built once per layout, read-only"""
    if (fid, lay) not in _frames:
        S, box, at, targets, seed = FRAMES[fid]
        if fid == "B17":
            assert lay == P.FRAMES["B17"][0]
            stored, p32, pixels, _ = P.frame("B17")
            _frames[fid, lay] = (stored, p32, pixels)
        else:
            p32, pixels = P.plant(S, box, targets, n_random=lay[0], n_feat=lay[1], seed=seed, at=at)
            _frames[fid, lay] = stored_and_image(p32, lay) + (pixels,)
    return _frames[fid, lay]


def dense_frame():
    if "dense" not in _frames:
        S, box, targets = DENSE
        p32, _ = P.plant(S, box, targets, n_random=DEFAULT_LAY[0], n_feat=DEFAULT_LAY[1], seed=0)
        p32.setflags(write=False)
        _frames["dense"] = p32
    return _frames["dense"]


def row_of(d, ty):
    """the arrays of a pass's outputs cut to row ty (colour: [3, 1, W, S]), as copies -- the whole-frame arrays are not kept; the
    scalars as they are"""
    out = {}
    for k, v in d.items():
        if isinstance(v, np.ndarray) and v.ndim >= 2:
            out[k] = (v[:, ty:ty + 1] if k == "colour" else v[ty:ty + 1]).copy()
        else:
            out[k] = v
    return out


_want = {}


def frame_oracle(oracle, fid, lay, policy, sigma_seed=0.002):
    """the oracle's pass over the target row of a frame, cut to that row: computed once per session, shared, never modified"""
    key = (fid, lay, policy, sigma_seed)
    if key not in _want:
        W, H, S, box = geometry(fid)
        ty = target_row(fid)
        d = oracle.make_desc(W, H, S, box=box, row_begin=ty, row_end=ty + 1, policy=policy, sigma_seed=sigma_seed, n_random=lay[0],
                             n_feat=lay[1])
        _want[key] = row_of(oracle.filter_pass(frame(fid, lay)[1], d), ty)
    return _want[key]


# ---- the visiting order of stage 1b, restated (make_window / candidate_offset of csrc/rpf_generic_common.h) -------------------------
def make_window(x, y, b, W, H, S):
    x0, x1, y0, y1 = max(x - b, 0), min(x + b, W - 1), max(y - b, 0), min(y + b, H - 1)
    nyv = y1 - y0 + 1
    return dict(x0=x0, y0=y0, nyv=nyv, centre_rank=(x - x0) * nyv + (y - y0), ncand=((x1 - x0 + 1) * nyv - 1) * S)


def candidates(win, S):
    """(yn, xn, s) of candidates 0 .. ncand - 1: xn outer, yn inner, s innermost, the centre pixel skipped"""
    qq = np.arange(win["ncand"])
    cell = qq // S
    s = qq - cell * S
    cell = cell + (cell >= win["centre_rank"])
    ix = cell // win["nyv"]
    iy = cell - ix * win["nyv"]
    return win["y0"] + iy, win["x0"] + ix, s


def fnv1a_u32(h, v):
    for i in range(4):
        h = ((h ^ ((v >> (8 * i)) & 0xff)) * 16777619) & 0xffffffff
    return h


_words = {}


def acceptance(oracle, fid, lay):
    """per target: (nwords, members per acceptance word [nwords], member_hash of the list those words give), from the oracle's
    per-pixel mean and sigma and the test of generic::nbhd_count_kernel: rejected on feature k iff |f - m| >= sd * 3"""
    if (fid, lay) not in _words:
        W, H, S, box = geometry(fid)
        b, f0 = (box - 1) // 2, 5 + lay[0]
        p32, pixels = frame(fid, lay)[1:]
        pmean, pstd = oracle.pixel_stats(p32, oracle.make_desc(W, H, S, box=box, policy=EPS, n_random=lay[0], n_feat=lay[1]))
        out = []
        for y, x in pixels:
            win = make_window(x, y, b, W, H, S)
            yn, xn, s = candidates(win, S)
            f = p32[f0:, yn, xn, s].astype(np.float64)                                   # [nF, ncand]
            ok = ~(np.abs(f - pmean[y, x][:, None]) >= (pstd[y, x] * 3.0)[:, None]).any(axis=0)
            nwords = (win["ncand"] + 63) >> 6
            bits = np.zeros(nwords * 64, bool)
            bits[:win["ncand"]] = ok
            h = 2166136261
            for sm in range(S):
                h = fnv1a_u32(h, (b * box + b) * S + sm)
            for code in (((xn[ok] - x + b) * box + (yn[ok] - y + b)) * S + s[ok]).tolist():
                h = fnv1a_u32(h, code)
            out.append((nwords, bits.reshape(nwords, 64).sum(axis=1), h))
        _words[fid, lay] = out
    return _words[fid, lay]


# ---- 1. plant(at=...) ----------------------------------------------------------------------------------------------------------------
# sha256 of plant()'s float32 planes, taken from the commit before `at` existed
PARENT_SHA256 = {
    "U8": "d6de50b25c9cba18a90910874671975f366cee627edc754462e281049c23aac7",
    "B17": "2f48a62b47b2bd102e8ee8424282737ae1928d4184d66c0307d943a3584e805e",
    "H16": "a1ac73d4275f29ff62c00847c3a4a52df26e54d4de713aa940e53295e6fc32d1",
}


@pytest.mark.parametrize("fid", list(PARENT_SHA256))
def test_centre_placement_is_byte_identical_to_the_parent(fid):
    (nr, nf, _), S, box, targets, seed, _ = P.FRAMES[fid]
    planes, pixels = P.plant(S, box, targets, n_random=nr, n_feat=nf, seed=seed)
    assert hashlib.sha256(planes.tobytes()).hexdigest() == PARENT_SHA256[fid]
    b = (box - 1) // 2
    assert pixels == [(b, t * box + b) for t in range(len(targets))]
    again, pix2 = P.plant(S, box, targets, n_random=nr, n_feat=nf, seed=seed, at=None)
    assert again.tobytes() == planes.tobytes() and pix2 == pixels


def test_plant_at_places_and_refuses():
    planes, pixels = P.plant(4, 5, (4, 20, 60), n_random=3, n_feat=7, seed=1, at=(0, 2))       # dx = b: any number of blocks
    assert planes.shape == (15, 5, 15, 4) and pixels == [(0, 2), (0, 7), (0, 12)]
    assert P.plant(4, 5, (24,), at=(4, 0))[1] == [(4, 0)]                                       # one block: first and last
    assert P.plant(4, 5, (24,), at=(3, 4))[1] == [(3, 4)]
    for ty in range(5):
        assert P.plant(4, 5, (4, 4), at=(ty, 2))[1] == [(ty, 2), (ty, 7)]                       # any row
    for at in ((0, 1), (0, 3), (2, 0), (2, 4)):                                                 # dx != b with another block beside
        with pytest.raises(ValueError):
            P.plant(4, 5, (4, 4), at=at)
    for at in ((5, 2), (-1, 2), (0, 5), (0, -1)):                                               # outside the block
        with pytest.raises(ValueError):
            P.plant(4, 5, (8,), at=at)
    # the candidates are the clipped window's: a corner target of box 5 has 3 x 3 - 1 pixels of candidates, an edge one 3 x 5 - 1
    P.plant(4, 5, (4 + 8 * 4,), at=(0, 0))
    with pytest.raises(ValueError):
        P.plant(4, 5, (4 + 8 * 4 + 1,), at=(0, 0))
    P.plant(4, 5, (4 + 14 * 4,), at=(0, 2))
    with pytest.raises(ValueError):
        P.plant(4, 5, (4 + 14 * 4 + 1,), at=(0, 2))


def test_frame_table_strides_and_clipped_windows():
    assert set(FRAMES) == set(LAYOUTS) == set(STRIDE)
    for fid, (S, box, at, targets, _) in FRAMES.items():
        W, H, _, _ = geometry(fid)
        assert mask_stride(box, S) == STRIDE[fid] and 64 < STRIDE[fid] <= QD_MAX_WORDS, fid
        assert H == box and box * box * S <= 65535, fid                  # (above: a wide pass, routes 6 and 7)
        pixels = frame(fid, LAYOUTS[fid][0])[2]
        assert [p[0] for p in pixels] == [target_row(fid)] * len(targets)
        b = (box - 1) // 2
        for y, x in pixels:
            nwords = (make_window(x, y, b, W, H, S)["ncand"] + 63) >> 6
            assert nwords == CLIPPED_NWORDS.get(fid, STRIDE[fid]), fid
    assert STRIDE["W181"] == QD_MAX_WORDS and 181 * 181 * 2 == 65522
    assert P.FRAMES["B17"][0] == LAYOUTS["B17"][0] and P.FRAMES["B17"][1:3] == FRAMES["B17"][:2]


# ---- 2. the planted sizes and the census of the target row, against the oracle -------------------------------------------------------
@pytest.mark.parametrize("fid,lay", CASES, ids=CASE_IDS)
def test_targets_have_their_planted_n_and_the_row_reaches_every_list(oracle, fid, lay):
    want = frame_oracle(oracle, fid, lay, EPS)
    targets = FRAMES[fid][3]
    n = want["nbhd_size"]
    W, _, S, box = geometry(fid)
    assert n.shape == (1, W)
    assert [int(n[0, x]) for _, x in frame(fid, lay)[2]] == list(targets)
    assert n.min() >= S and n.max() <= box * box * S
    cc = class_counts(n)
    for t in targets:
        if t <= CAPS[-1]:
            assert cc[CAPS.index(P.class_of(t))] > 0, (fid, t)
    assert cc[10] > 0 and sum(cc) == W                                    # ... and the rest list has work
    assert want["status"] == 0 and np.isfinite(want["colour"]).all()


def test_w31_under_ref_abort(oracle):
    want = frame_oracle(oracle, "W31", DEFAULT_LAY, REF_ABORT)
    n = want["nbhd_size"]
    assert [int(n[0, x]) for _, x in frame("W31", DEFAULT_LAY)[2]] == list(FRAMES["W31"][3])
    assert np.array_equal(n, frame_oracle(oracle, "W31", DEFAULT_LAY, EPS)["nbhd_size"])


@pytest.mark.parametrize("fid", ACTIVE_FRAMES)
def test_active_seed_moves_the_colours_of_the_target_row(oracle, fid):
    lay, ty = DEFAULT_LAY, target_row(fid)
    want = frame_oracle(oracle, fid, lay, EPS, P.ACTIVE_SIGMA_SEED)
    cin = frame(fid, lay)[1][2:5, ty:ty + 1].astype(np.float64)
    assert np.isfinite(want["colour"]).all()
    assert np.linalg.norm(want["colour"] - cin) / np.linalg.norm(cin) >= 0.05
    assert np.array_equal(want["nbhd_size"], frame_oracle(oracle, fid, lay, EPS)["nbhd_size"])


# ---- 3. the acceptance words: the restated order pinned by member_hash, then where the members lie --------------------------------
@pytest.mark.parametrize("fid,lay", CASES, ids=CASE_IDS)
def test_restated_words_give_the_oracles_members(oracle, fid, lay):
    want = frame_oracle(oracle, fid, lay, EPS)
    S, targets = FRAMES[fid][0], FRAMES[fid][3]
    for (y, x), t, (nwords, per_word, h) in zip(frame(fid, lay)[2], targets, acceptance(oracle, fid, lay)):
        assert S + int(per_word.sum()) == t == int(want["nbhd_size"][0, x]), (fid, x)
        assert h == int(want["member_hash"][0, x]), (fid, x)


@pytest.mark.parametrize("fid,lay", CASES, ids=CASE_IDS)
def test_members_lie_where_a_wrong_carry_stride_or_deal_would_show(oracle, fid, lay):
    """for every target above 832 (the four-wave classes and the first of the rest list): every 64-word step of the prefix holds
    a member, the last step too -- a dropped or doubled carry moves members; every residue w mod 4 holds a member -- each wave's
    deal; on W55 and W181, whose windows have more than 256 words, some word >= 256 holds one -- the popcount stride of 256
    threads; on W181 some word >= 960 -- the last step below the clamp"""
    checked = 0
    for t, (nwords, per_word, _) in zip(FRAMES[fid][3], acceptance(oracle, fid, lay)):
        if t <= 832:
            continue
        for w0 in range(0, nwords, 64):
            assert per_word[w0:w0 + 64].sum() > 0, (fid, t, w0)
        for r in range(4):
            assert per_word[r::4].sum() > 0, (fid, t, r)
        if fid in ("W55", "W181"):               # (C55's clipped windows end at word 192: no word >= 256 can hold a member)
            assert nwords > 256 and per_word[256:].sum() > 0, (fid, t)
        if fid == "W181":
            assert nwords == QD_MAX_WORDS and per_word[960:].sum() > 0, t
        # ... and the members interleave with rejected candidates: no word of the window is full
        assert per_word.max() < 64
        checked += 1
    assert checked == sum(1 for t in FRAMES[fid][3] if t > 832) > 0


def test_clipped_windows_use_half_and_a_quarter_of_the_stride(oracle):
    for fid in ("C55", "K55"):
        for nwords, per_word, _ in acceptance(oracle, fid, DEFAULT_LAY):
            assert nwords == CLIPPED_NWORDS[fid] < STRIDE[fid] and len(per_word) == nwords
    # C55's words run past 192 = three whole steps: the fourth step is one word of 24 candidates
    assert CLIPPED_NWORDS["C55"] == 3 * 64 + 1


# ---- 4. the frame that leaves full words behind -------------------------------------------------------------------------------------------
def test_dense_frame_fills_the_words_behind_the_clipped_windows(oracle):
    """every candidate of every window of the dense frame passes (a bound over the whole frame: the largest |f - m| of any sample
    against any pixel's mean is below three times the smallest sigma), so generic::nbhd_count_kernel writes a full word for every 64
    candidates; laid over the same buffer, the strides of C55's and K55's targets beyond their own nwords hold such words"""
    S, box, targets = DENSE
    W, H = box * len(targets), box
    p32 = dense_frame()
    nr, nf, _ = DEFAULT_LAY
    pmean, pstd = oracle.pixel_stats(p32, oracle.make_desc(W, H, S, box=box, policy=EPS, n_random=nr, n_feat=nf))
    f = p32[5 + nr:].astype(np.float64)
    for k in range(nf):
        reach = max(f[k].max() - pmean[..., k].min(), pmean[..., k].max() - f[k].min())
        assert reach < 3.0 * pstd[..., k].min(), k
    b, dense_stride = (box - 1) // 2, mask_stride(box, S)
    assert dense_stride == 50
    full_words = np.zeros((H, W), np.int64)                               # words the dense pass writes as ~0 per pixel
    for y in range(H):
        for x in range(W):
            full_words[y, x] = make_window(x, y, b, W, H, S)["ncand"] // 64
    full_words = full_words.reshape(-1)
    for fid in ("C55", "K55"):
        Wf, Hf, Sf, boxf = geometry(fid)
        ty = target_row(fid)
        assert (ty * Wf + Wf) * STRIDE[fid] <= H * W * dense_stride          # the dense buffer covers the whole target row
        for (y, x), (nwords, _, _) in zip(frame(fid, DEFAULT_LAY)[2], acceptance(oracle, fid, DEFAULT_LAY)):
            g = (y * Wf + x) * STRIDE[fid] + np.arange(nwords, STRIDE[fid])
            stale_full = (g % dense_stride) < full_words[g // dense_stride]
            assert stale_full.sum() >= (STRIDE[fid] - nwords) // 2, (fid, x, int(stale_full.sum()))
