"""The frames of the wide-neighbourhood tests (RPF_FLAG_WIDE_NBHD: 65535 < box * box * S <= 262144).

A plain helper module, like planted_nbhd.py, shared by tests/golden/make_wide_golden.py (which runs the oracle on them once and
writes the fixtures), tests/test_wide_nbhd_cpu.py and tests/test_wide_nbhd_gpu.py.  Every frame is planted_nbhd.plant() at
S = 21, box 57 (box * box * S = 68229): 57 rows of 57 pixels per target.  The oracle takes a third of a second per pixel at
this size, so only the row of the targets (ROW) is filtered, on the GPU as in the fixtures.

  main    layout (2, 12) fp32, targets 65535 | 65536 (the old cap, the 16-bit cell, B = 255 | 256), 66049 (B = 257: the first
          bin id no byte holds; the row's other pixels lie on both sides of it) and 68229 (a full window)
  l1_1    layout (1, 1) fp32, target 66049: the fewest columns and pairs
  l4_18h  layout (4, 18) fp16, target 66049: the second compiled layout
  l17_18  layout (17, 18) fp32, target 66049: 40 dims, the most pairs
  heavy   layout (2, 12) fp32, target 66049, with columns made constant but for own samples of the target (see heavy())
"""
import zlib

import numpy as np

import planted_nbhd as P

S, BOX = 21, 57
ROW = (BOX - 1) // 2            # 28: the row of the targets
NMAX = BOX * BOX * S            # 68229
SIGMA_SEED = P.ACTIVE_SIGMA_SEED

# id: (n_random, n_feat, plane type), targets
FRAMES = {
    "main": ((2, 12, "f32"), (65535, 65536, 66049, 68229)),
    "l1_1": ((1, 1, "f32"), (66049,)),
    "l4_18h": ((4, 18, "f16"), (66049,)),
    "l17_18": ((17, 18, "f32"), (66049,)),
    "heavy": ((2, 12, "f32"), (66049,)),
}

# heavy(): the columns made near-constant, and the own samples of the target that keep another value in each
HEAVY_COMMON, HEAVY_OTHER = np.float32(0.5), np.float32(0.75)
HEAVY_COLUMNS = {5: (3,), 6: (3,), 2: (3,), 3: (3, 11)}


def heavy(planes, pixels):
    """Joint histogram cells that no 16-bit counter holds.  The two random parameters (columns 5 and 6) and the first colour
    channel (column 2) are HEAVY_COMMON everywhere but for own sample 3 of the target; the second colour channel (column 3)
    but for own samples 3 and 11.  None of these columns takes part in the 3-sigma test, so membership is untouched.  The MI
    pairs are (feature, random | position) and (colour, random | position | feature) -- no pair joins two random parameters,
    which is why colour columns are part of it: the tables (2, 5) and (2, 6) hold one cell of N - 1 counts and one of 1, the
    tables (3, 5) and (3, 6) one cell of N - 2 and two of 1.  The outliers coincide on purpose: two near-constant columns with
    DIFFERENT outliers would be independent to within 1 / N^2, a table near the zero band, which the fixtures must not hold."""
    (ty, tx), = pixels
    for col, own in HEAVY_COLUMNS.items():
        planes[col] = HEAVY_COMMON
        for s in own:
            planes[col, ty, tx, s] = HEAVY_OTHER
    return planes


_cache = {}


def frame(fid):
    """(stored planes, their fp32 image for the oracle, target pixels, planted sizes); built once, read-only"""
    if fid not in _cache:
        (nr, nf, dt), targets = FRAMES[fid]
        p32, pixels = P.plant(S, BOX, targets, n_random=nr, n_feat=nf, seed=0)
        if fid == "heavy":
            p32 = heavy(p32, pixels)
        stored = p32.astype(np.float16) if dt == "f16" else p32
        p32 = stored.astype(np.float32)
        stored.setflags(write=False)
        p32.setflags(write=False)
        _cache[fid] = (stored, p32, pixels, targets)
    return _cache[fid]


def checksum(fid):
    """CRC-32 of the stored planes' bytes: a numpy whose generator gave other planes would not silently move the input"""
    return zlib.crc32(frame(fid)[0].tobytes()) & 0xffffffff


def geometry(fid):
    """W, H of a frame"""
    return BOX * len(FRAMES[fid][1]), BOX


def members(fid):
    """boolean [H, W, S]: the neighbourhood of the (single) target of a one-target frame, by the 3-sigma test in numpy.  The
    planted rejections lie 10 away from a spread of 0.2, nowhere near the test's edge, so the order of the sums cannot matter."""
    (nr, nf, _), _ = FRAMES[fid]
    _, p32, ((ty, tx),), _ = frame(fid)
    f = p32[5 + nr:].astype(np.float64)
    own = f[:, ty, tx, :]
    m, sd = own.mean(axis=1), own.std(axis=1)
    ok = (np.abs(f - m[:, None, None, None]) < 3.0 * sd[:, None, None, None]).all(axis=0)
    ok[ty, tx, :] = True
    return ok
