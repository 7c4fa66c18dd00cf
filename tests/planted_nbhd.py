"""Frames whose neighbourhood sizes are PLANTED: plant() builds a feature buffer in which chosen pixels have exactly the
neighbourhood size N asked for, so a test can put N on either side of every kernel-class edge (class_capacity 8, 16, 32, 64,
128, 256, 448, 832, 1600, 3136 | streaming) instead of taking whatever the 3-sigma test yields on a synthetic frame.

A plain helper module (like pbrt_film_ref.py): tests/test_planted_nbhd_cpu.py checks the frames against the oracle on the
CPU, tests/test_class_boundaries_gpu.py runs them through the kernels.

How a size is planted.  The frame is one row of disjoint box x box windows, one per target; the target pixel is its window's
centre, so its window is the whole of its own box and nobody else's.  Every column of every pixel starts as a permutation of
the same S values: all pixels share mean and sigma (up to the rounding of a sum taken in another order), and every sample
passes every pixel's 3-sigma test -- N would be box * box * S everywhere.  Then, per window, as many candidates as must go are
pushed 10 away on ONE feature each: such a sample fails the target's test on that feature and on no other.  The target's
own samples are never touched, so its statistics stay and it keeps exactly the N asked for; the members lie scattered over
the window and interleave with rejected candidates in the reference's visiting order.  The window's other pixels, some of
whose own samples were pushed, get wide sigmas on some features and assorted N: they are compared like every pixel.

Targets off the centre (plant(at=(ty, dx)); tests/test_generic_wide_windows_cpu.py, tests/test_generic_wide_windows_gpu.py).  Every
target sits at row ty of the frame and column t * box + dx of its block, so the frame clips its window: the kernels see a window
whose candidate count, and so whose number of acceptance words, is well below what the box alone allows.  The candidates are the
block's pixels inside the clipped window, and N is planted among them as above.  A placement whose clipped window would reach
into another block is refused (ValueError): dx != b is possible only where the frame's edge does the clipping -- dx <= b on the
first block, dx >= b on the last -- and as every target shares dx, only on a frame of one target; any row 0 <= ty < box is
allowed, the frame being one block high.  at=None is the centre placement, unchanged to the byte: the calls on the random
generator come in the same order (tests/test_generic_wide_windows_cpu.py holds U8, B17 and H16 to recorded hashes).

Sampled passes (routes 8, 11 and 12: tests/test_planted_routes_cpu.py, tests/test_class_edges_routes_gpu.py).  plant_sampled()
plants the same way among the DRAWS of a target: its candidates are the distinct surviving draws of sampled_ref.draws, of which
as many as must go are pushed, so the target keeps S + (draws not pushed) members.  Two edges meet on such a pass: the class
capacity, as above, and the pass's own bound nmax = S + D, the longest list any pixel can have, from which the class kernels are
sized: the NM frames put a target whose D draws are all distinct -- nothing pushed -- at N = S + D, where nmax is a class capacity
(16, 64) and where it lies inside a class (100 in class 128), and one at S + D - 1 beside it.
Left out: N = 3136 on a sampled pass.  S + D <= 3136 would need 3000-odd draws without one repeat; the longest list found over
seeds and pixels is 2773, at S = 64.  The upper edge of the last resident class is held on routes 2 and 10 alone (B64, B40, B17).
"""
import numpy as np

# class_capacity of csrc/rpf_kernels.hip: the largest N of each size class (beyond the last one: the streaming kernel)
CAPACITIES = (8, 16, 32, 64, 128, 256, 448, 832, 1600, 3136)
PACKED_PIXELS_PER_WAVE = {8: 8, 16: 4, 32: 2}   # packed class capacity -> pixels per wavefront (64: one)

# id: layout (n_random, n_feat, plane type), S, box, planted N per target, seed, size-binned route?
# (the closing 24 of U8 and H8 makes the pixel count of the packed class N <= 32 odd -- 17, 24, 32 -- so that its last wave,
# two pixels wide, runs half empty: test_planted_nbhd_cpu.py holds the counts of the three shared-wave classes to that)
FRAMES = {
    "U8": ((2, 12, "f32"), 8, 7, (8, 9, 16, 17, 32, 33, 64, 65, 24), 0, False),
    "U2": ((2, 12, "f32"), 2, 7, (2, 8, 9, 16, 17, 98), 0, False),
    "U3": ((2, 12, "f32"), 3, 13, (3, 8, 9, 64, 65, 448, 449, 507), 0, False),                  # the unbinned K = 13 kernel
    "U12": ((2, 12, "f32"), 12, 5, (12, 16, 17, 256, 257, 300), 0, False),                      # the unbinned K = 7 kernel
    "B16": ((2, 12, "f32"), 16, 7, (16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 448, 449, 784), 0, True),
    "B32": ((2, 12, "f32"), 32, 7, (832, 833, 1568), 0, True),                                  # four-wave / split K = 25
    "B64": ((2, 12, "f32"), 64, 7, (1600, 1601, 3135, 3136), 0, True),                          # K = 25 | K = 49
    "B40": ((2, 12, "f32"), 40, 9, (3136, 3137, 3240), 0, True),                                # resident | streaming
    "B17": ((2, 12, "f32"), 16, 17, (832, 833, 1600, 1601, 3136, 3137), 0, True),               # window > 4096: one-wave K = 25 / 49
    "H8": ((4, 18, "f16"), 8, 7, (8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 392, 24), 0, False),
    "H16": ((4, 18, "f16"), 16, 7, (448, 449, 784), 0, True),
    "H64": ((4, 18, "f16"), 64, 7, (1600, 1601, 3136), 0, True),
}


def plant(S, box, targets, n_random=2, n_feat=12, seed=0, at=None):
    """float32 planes [5 + n_random + n_feat, box, box * len(targets), S] and the target pixels [(y, x), ...]: pixel
    targets[t]'s neighbourhood under a box x box window holds exactly targets[t] samples (S <= targets[t] <= the samples of
    its window: box * box * S at the centre, fewer where the frame clips the window).

    at: None -- every target at the centre of its block -- or (ty, dx): every target at row ty of the frame and column
    t * box + dx of its block; see the module docstring for what is refused."""
    if S < 2:
        raise ValueError("S >= 2: one sample per pixel has sigma = 0 and accepts nobody")
    nt, b = len(targets), (box - 1) // 2
    H, W, ndim, f0 = box, box * nt, 5 + n_random + n_feat, 5 + n_random
    if at is not None:
        aty, adx = at
        if not (0 <= aty < box and 0 <= adx < box):
            raise ValueError("at = (%d, %d) outside the block [0, %d) x [0, %d)" % (aty, adx, box, box))
        # the window of a target off its block's centre column reaches into the next block unless the frame's edge clips it
        if adx < b and nt != 1:
            raise ValueError("at: dx = %d < b = %d reaches into the block to the left of every target but the first" % (adx, b))
        if adx > b and nt != 1:
            raise ValueError("at: dx = %d > b = %d reaches into the block to the right of every target but the last" % (adx, b))
    rng = np.random.default_rng(seed)
    planes = rng.permuted(np.broadcast_to(np.linspace(0.4, 0.6, S), (ndim, H, W, S)), axis=3).astype(np.float32)
    planes[0] = (np.arange(W)[None, :, None] + rng.random((H, W, S))).astype(np.float32)
    planes[1] = (np.arange(H)[:, None, None] + rng.random((H, W, S))).astype(np.float32)
    planes[2:5] = rng.random((3, H, W, S)).astype(np.float32)
    pixels = []
    for t, n in enumerate(targets):
        ty, tx = (b, t * box + b) if at is None else (at[0], t * box + at[1])
        pixels.append((ty, tx))
        # the block's pixels inside the window clipped to the frame (at the centre: the whole block)
        ys = range(max(ty - b, 0), min(ty + b, H - 1) + 1)
        xs = range(max(tx - b, t * box), min(tx + b, (t + 1) * box - 1) + 1)
        cand = [(y, x, s) for y in ys for x in xs for s in range(S) if (y, x) != (ty, tx)]
        n_reject = len(cand) - (n - S)
        if not 0 <= n_reject <= len(cand):
            raise ValueError("target %d: N = %d outside [S, S + candidates] = [%d, %d]" % (t, n, S, S + len(cand)))
        chosen = rng.permutation(len(cand))[:n_reject]
        feats = rng.integers(0, n_feat, n_reject)
        for i, (ci, k) in enumerate(zip(chosen, feats)):
            y, x, s = cand[ci]
            planes[f0 + k, y, x, s] += np.float32(10.0 if i % 2 == 0 else -10.0)
    return planes, pixels


# id: layout, S, box, draws D, sampling seed, planted N per target, planting seed.  Distinct surviving draws at the targets (what a
# planted N cannot exceed, S added): SP8 156 .. 177, SP16 1233 .. 1270, SP32 and SPH32 2451 .. 2474, SPH16 191 .. 210; tests/
# test_planted_routes_cpu.py holds the planted sizes.  SP32: (17 * 17 - 1) * 32 > 4096 candidates, the one-wave instantiations on
# route 11.  NM*: N = S + D = nmax at the targets whose D draws are all distinct, S + D - 1 beside them.
SAMPLING_SEED = 0x5EED5EED
SAMPLED_FRAMES = {
    "SP8": ((2, 12, "f32"), 8, 7, 248, SAMPLING_SEED, (8, 9, 16, 17, 32, 33, 64, 65, 128, 129), 0),
    "SP16": ((2, 12, "f32"), 16, 17, 1584, SAMPLING_SEED, (256, 257, 448, 449, 832, 833), 0),
    "SP32": ((2, 12, "f32"), 32, 17, 3104, SAMPLING_SEED, (1600, 1601, 833, 2400), 0),          # S + D = 3136, the cap
    "SPH16": ((4, 18, "f16"), 16, 7, 240, SAMPLING_SEED, (16, 17, 64, 65, 128, 129), 0),        # the d27 builds
    "SPH32": ((4, 18, "f16"), 32, 17, 3104, SAMPLING_SEED, (833, 1600, 1601, 2400), 0),         # ... their K = 25 and K = 49 parts
    "NM16": ((2, 12, "f32"), 8, 7, 8, SAMPLING_SEED, (16, 15, 16, 8, 9, 16, 13, 15, 14, 16, 16, 15), 0),   # nmax = capacity 16
    "NM64": ((2, 12, "f32"), 8, 17, 56, SAMPLING_SEED, (33, 32, 63, 33, 63, 64, 63, 62, 64), 0),           # nmax = capacity 64
    "NM100": ((2, 12, "f32"), 8, 17, 92, SAMPLING_SEED + 1, (65, 64, 99, 98, 96, 100), 0),                 # nmax = 100 inside class 128
}
NMAX_FRAMES = ("NM16", "NM64", "NM100")


# ---- what tests/test_planted_routes_cpu.py proves and tests/test_class_edges_routes_gpu.py runs -----------------------------------------
ROUTE10_FRAMES = ("U8", "B16", "B32", "B64", "B40", "B17", "H8", "H16", "H64")
# (gain_c, gain_f) of the scheduled cases, per frame: chosen on the oracle's MI of the target row so that clamped and open entries
# of alpha, and of beta's factor, each hold tests/test_schedule_fused_cpu.py's SHARE (asserted in tests/test_planted_routes_cpu.py).  On a planted frame W_r_c and W_r_f of a row lie in a narrow band (the colours are white noise, every pixel has the
# same law), so one pair of gains cannot serve every frame: each gain is near 1 / (the row's median ratio)
GAINS = {"U8": (2.4, 2.2), "B16": (2.1, 2.0), "B32": (2.0, 1.9), "B64": (2.0, 1.93), "B40": (2.3, 2.2), "B17": (4.0, 3.0),
         "H8": (1.65, 1.6), "H16": (1.68, 1.58), "H64": (1.505, 1.473)}
SAMPLED_GAINS = {"SP8": (2.25, 2.05), "SP16": (2.9, 2.5), "SP32": (2.35, 2.2), "NM16": (1.9, 1.75), "NM64": (2.1, 2.0),
                 "NM100": (2.05, 2.0), "SPH16": (1.49, 1.43), "SPH32": (1.69, 1.65)}


def nonref(n_feat=12):
    """a membership test that is not the reference's: multiples 2.5 .. 47.5 that differ from feature to feature, every floor
    negative (no floor ever applies: a candidate is rejected on k iff |f - m| >= mult_k sd).  On a planted frame the unpushed
    values lie within 1.6 sd of the mean and a push is beyond 100 sd, so the planted sizes stand: asserted in
    tests/test_planted_routes_cpu.py, not assumed"""
    k = np.arange(n_feat)
    return 2.5 + 2.5 * ((7 * k) % 19), -0.25 - 0.125 * k


def class_of(n):
    """the capacity of the size class of a neighbourhood of n samples (65535: the streaming class)"""
    return next((c for c in CAPACITIES if n <= c), 65535)


def plant_sampled(S, box, targets, D, sampling_seed, pass_id=0, n_random=2, n_feat=12, seed=0):
    """plant() for a sampled pass of D draws under `sampling_seed`: float32 planes [5 + n_random + n_feat, box, box * len(targets),
    S] and the target pixels; pixel targets[t] keeps exactly targets[t] members: its S own samples and that many of its distinct
    surviving draws (S <= targets[t] <= S + their number), the other draws pushed 10 away on one feature each"""
    import sampled_ref as SR     # (here, not at module level: sampled_ref imports fast_weights_ref, which imports this module)
    if S < 2:
        raise ValueError("S >= 2: one sample per pixel has sigma = 0 and accepts nobody")
    nt, b = len(targets), (box - 1) // 2
    H, W, ndim, f0 = box, box * nt, 5 + n_random + n_feat, 5 + n_random
    rng = np.random.default_rng(seed)
    planes = rng.permuted(np.broadcast_to(np.linspace(0.4, 0.6, S), (ndim, H, W, S)), axis=3).astype(np.float32)
    planes[0] = (np.arange(W)[None, :, None] + rng.random((H, W, S))).astype(np.float32)
    planes[1] = (np.arange(H)[:, None, None] + rng.random((H, W, S))).astype(np.float32)
    planes[2:5] = rng.random((3, H, W, S)).astype(np.float32)
    pixels = []
    for t, n in enumerate(targets):
        ty, tx = b, t * box + b
        pixels.append((ty, tx))
        qq = SR.draws(sampling_seed, pass_id, 0, D, box, W, H, S, tx, ty)
        xn, yn, sn = SR.decode(qq, box, W, H, S, tx, ty)
        assert not ((xn == tx) & (yn == ty)).any()                      # a draw on the centre pixel does not survive
        n_reject = len(qq) - (n - S)
        if not 0 <= n_reject <= len(qq):
            raise ValueError("target %d: N = %d outside [S, S + distinct draws] = [%d, %d]" % (t, n, S, S + len(qq)))
        chosen = rng.permutation(len(qq))[:n_reject]
        feats = rng.integers(0, n_feat, n_reject)
        for i, (ci, k) in enumerate(zip(chosen, feats)):
            planes[f0 + k, yn[ci], xn[ci], sn[ci]] += np.float32(10.0 if i % 2 == 0 else -10.0)
    return planes, pixels


_cache = {}
_sampled_cache = {}


def sampled_frame(fid):
    """(stored planes, their fp32 image for the restatement, target pixels, planted sizes) of SAMPLED_FRAMES[fid]; built once,
    read-only.  An f16 layout is rounded once, as in frame()"""
    if fid not in _sampled_cache:
        (nr, nf, dt), S, box, D, sseed, targets, seed = SAMPLED_FRAMES[fid]
        p32, pixels = plant_sampled(S, box, targets, D, sseed, n_random=nr, n_feat=nf, seed=seed)
        stored = p32.astype(np.float16) if dt == "f16" else p32
        p32 = stored.astype(np.float32)
        stored.setflags(write=False)
        p32.setflags(write=False)
        _sampled_cache[fid] = (stored, p32, pixels, targets)
    return _sampled_cache[fid]


def frame(fid):
    """(stored planes, their fp32 image for the oracle, target pixels, planted sizes) of FRAMES[fid]; built once, read-only.
    An f16 layout is rounded once: the device reads the halves, the oracle the same halves widened."""
    if fid not in _cache:
        (nr, nf, dt), S, box, targets, seed, _ = FRAMES[fid]
        p32, pixels = plant(S, box, targets, n_random=nr, n_feat=nf, seed=seed)
        stored = p32.astype(np.float16) if dt == "f16" else p32
        p32 = stored.astype(np.float32)
        stored.setflags(write=False)
        p32.setflags(write=False)
        _cache[fid] = (stored, p32, pixels, targets)
    return _cache[fid]


# The colours of a planted frame are white noise and its features spread evenly, so at the reference's sigma seed (0.002:
# sigma_c^2 = sigma_f^2 ~ 1e-5 in z-space) every weight but a sample's own underflows and the filter is the IDENTITY: the
# discrete outputs, MI, alpha, beta and W_r_c are compared for real, the colours only show that nothing was broken.  With
# this seed the weights are of order one (the oracle moves the colours by 6 ... 40 %), and a member dropped from, or a stale
# slot added to, a weight sum shows in the colours.
# Where stage 4 is actually held -- sample by sample, against a bar derived from the roundings -- is
# tests/test_stage4_per_sample_gpu.py (tests/stage4_bars.py), at this seed.
ACTIVE_SIGMA_SEED = 0.5

_want = {}


def oracle_pass(oracle, fid, policy, sigma_seed=0.002):
    """the oracle's filter pass of a frame under a policy: computed once per session, shared, never modified"""
    if (fid, policy, sigma_seed) not in _want:
        (nr, nf, _), S, box, targets, _, _ = FRAMES[fid]
        _, p32, _, _ = frame(fid)
        lay = dict(n_random=nr, n_feat=nf) if (nr, nf) != (2, 12) else {}
        _want[fid, policy, sigma_seed] = oracle.filter_pass(p32, oracle.make_desc(box * len(targets), box, S, box=box, policy=policy,
                                                                                  sigma_seed=sigma_seed, **lay))
    return _want[fid, policy, sigma_seed]
