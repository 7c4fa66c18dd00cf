"""The really wide frame of the route-7 tests (RPF_FLAG_WIDE_NBHD | RPF_FLAG_WIDE_CLASSES): planted_nbhd.plant() at S = 21,
box 57 (box * box * S = 68229 > 65535), the geometry of wide_frames.py, with targets on both sides of every class edge that
S = 21 can reach -- 32 | 33, 64 | 65, 128 | 129, 256 | 257, 448 | 449, 832 | 833 -- the smallest size (N = S) and a target of
66049.  The middle pairs are there because the row's other pixels all have N in the thousands: without them the classes
N <= 256 and N <= 448 would be empty.

A plain helper module, shared by tests/golden/make_wide_classes_golden.py (which runs the oracle on the row of the targets once
and writes tests/golden/wide_classes.npz), tests/test_wide_classes_cpu.py and tests/test_wide_classes_gpu.py."""
import zlib

import numpy as np

import planted_nbhd as P

S, BOX = 21, 57
ROW = (BOX - 1) // 2
NMAX = BOX * BOX * S
SIGMA_SEED = P.ACTIVE_SIGMA_SEED
SEED = 0
TARGETS = (21, 32, 33, 64, 65, 128, 129, 256, 257, 448, 449, 832, 833, 66049)
W, H = BOX * len(TARGETS), BOX

_cache = {}


def frame():
    """(planes, target pixels): built once, read-only"""
    if not _cache:
        planes, pixels = P.plant(S, BOX, TARGETS, seed=SEED)
        planes.setflags(write=False)
        _cache["f"] = (planes, pixels)
    return _cache["f"]


def checksum():
    return zlib.crc32(frame()[0].tobytes()) & 0xffffffff


def fixture_pixels():
    """the columns of ROW the fixture holds stage outputs for: the targets, the pixels next to them, and every 16th pixel"""
    xs = set(range(0, W, 16))
    for _, x in frame()[1]:
        xs.update((x - 1, x, x + 1))
    return np.array(sorted(xs), np.int32)
