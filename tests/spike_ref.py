"""NumPy / plain-Python restatement of the spike pass (include/rpf_hip.h, RPF_FLAG_SPIKE_CLAMP), and the
frames the spike tests share.

Every chain of the definition is an explicit Python loop over IEEE doubles in the stated order (np.sum is pairwise: never
used for a chain); the first term of a chain is its first element (c_0 + c_1 + ..., not 0 + c_0 + ...), `/` is Python's
correctly rounded division, sqrt is math.sqrt.  A pixel whose standard deviation is NaN on any channel (it holds a NaN or an
infinite colour) flags nothing."""
import math

import numpy as np

# (W, H, S) of the GPU tests of the two halves; the last one takes the direct form of the clamp kernel (S > 1024)
SHAPES = [(5, 3, 7), (16, 4, 8), (7, 5, 1), (3, 2, 2), (9, 4, 21), (4, 3, 64), (2, 2, 1030)]
SLAB_SHAPES = [(5, 3, 7), (9, 4, 21)]  # run again with row_begin = 1, row_end = H - 1
THRESHOLDS = [1.0, 2.5]


def _chain(values):
    acc = values[0]
    for v in values[1:]:
        acc = acc + v
    return acc


def pixel(c, t):
    """one pixel: c = three lists of S floats (modified in place when 0 < n < S).  Returns (n, [e_0, e_1, e_2])"""
    S = len(c[0])
    dS = float(S)
    m, thr = [0.0] * 3, [0.0] * 3
    nan_pixel = False
    for k in range(3):
        m[k] = _chain(c[k]) / dS
        q = _chain([(v - m[k]) * (v - m[k]) for v in c[k]])
        sd = math.sqrt(q / dS) if not (q != q) else float("nan")
        thr[k] = t * sd
        nan_pixel = nan_pixel or sd != sd
    e = [0.0, 0.0, 0.0]
    if nan_pixel:
        return 0, e
    spike = [any(abs(c[k][s] - m[k]) > thr[k] for k in range(3)) for s in range(S)]
    n = sum(spike)
    if n == 0 or n == S:
        return n, e
    dK = float(S - n)
    for k in range(3):
        mp = _chain([c[k][s] for s in range(S) if not spike[s]]) / dK
        e[k] = _chain([c[k][s] - mp for s in range(S) if spike[s]])
        for s in range(S):
            if spike[s]:
                c[k][s] = mp
    return n, e


def fold(row_sums, n_samples):
    """E_k = the row sums in row order, delta_k = E_k / n_samples: what rpf_spike_delta computes"""
    rows = np.asarray(row_sums, np.float64)
    E = np.array([_chain([float(v) for v in rows[:, k]]) for k in range(3)])
    with np.errstate(all="ignore"):
        return E, E / np.float64(n_samples)


def clamp(colour, t, row_begin=0, row_end=None):
    """the clamp half on rows [row_begin, row_end): (colour', row_sums [rows][3], counts dict)"""
    colour = np.array(colour, np.float64)
    _, H, W, S = colour.shape
    row_end = H if row_end is None else row_end
    rows = np.zeros((max(row_end - row_begin, 0), 3))
    cnt = dict(spike_samples=0, spike_pixels=0, skipped_pixels=0)
    for y in range(row_begin, row_end):
        es = []
        for x in range(W):
            c = [colour[k, y, x].tolist() for k in range(3)]
            n, e = pixel(c, float(t))
            if 0 < n < S:
                cnt["spike_samples"] += n
                cnt["spike_pixels"] += 1
                for k in range(3):
                    colour[k, y, x] = c[k]
            elif n == S and n > 0:
                cnt["skipped_pixels"] += 1
            es.append(e)
        for k in range(3):
            rows[y - row_begin, k] = _chain([e[k] for e in es])
    return colour, rows, cnt


def add(colour, delta, row_begin=0, row_end=None):
    """c += delta_k on rows [row_begin, row_end): all three channels, or none when every delta is 0"""
    colour = np.array(colour, np.float64)
    row_end = colour.shape[1] if row_end is None else row_end
    if all(float(d) == 0.0 for d in delta):
        return colour
    with np.errstate(all="ignore"):
        for k in range(3):
            colour[k, row_begin:row_end] = colour[k, row_begin:row_end] + np.float64(delta[k])
    return colour


def apply(colour, t=1.0, preserve_energy=True, row_begin=0, row_end=None):
    """the whole pass: dict(colour, clamped, row_sums, energy, delta, spike_samples, spike_pixels, skipped_pixels)"""
    _, H, W, S = np.shape(colour)
    row_end = H if row_end is None else row_end
    clamped, rows, cnt = clamp(colour, t, row_begin, row_end)
    out = dict(cnt, clamped=clamped, row_sums=rows, colour=clamped, energy=np.zeros(3), delta=np.zeros(3))
    if row_end > row_begin:
        out["energy"], out["delta"] = fold(rows, (row_end - row_begin) * W * S)
        if preserve_energy:
            out["colour"] = add(clamped, out["delta"], row_begin, row_end)
    return out


def _skip_pixel(S):
    """three channel rows of a pixel whose every sample is flagged at t = 1 (n == S: skipped), S >= 2.
    S >= 3: channel 0 holds +-a alternating on the first 2h samples (2h = the largest even number <= S - 1: mean 0,
    sd = a sqrt(2h / S) < a, so those 2h are flagged), channel 1 flags the one or two that are left the same way.
    S == 2: a pair whose mean is rounded, so that one sample of it is flagged; the swapped pair on the next channel flags
    the other (with an exact mean |c - m| = sd for both samples, and sqrt(fl(d * d)) = d in binary floating point)."""
    c = np.full((3, S), 0.25)
    if S == 2:
        # 1 + (1 + 3u), u = 2^-52, is not a double: the sum rounds to 2 + 4u, m = 1 + 2u, and the two samples lie 2u and u from
        # it with sd = sqrt(2.5) u between the two: channel 0 flags sample 0, channel 1 (the pair swapped) sample 1
        c[0] = [1.0, 1.0 + 3 * 2.0 ** -52]
        c[1] = [1.0 + 3 * 2.0 ** -52, 1.0]
        return c
    h2 = (S - 1) // 2 * 2
    c[0, :h2] = 0.25 + 8.0 * np.where(np.arange(h2) % 2 == 0, 1.0, -1.0)
    rest = S - h2
    c[1, h2:] = [0.25 + 8.0] if rest == 1 else [0.25 + 8.0, 0.25 - 8.0]
    return c


def make_frame(W, H, S, seed, specials=True):
    """fp64 colours [3,H,W,S]: seeded lognormal, 5 % of the samples multiplied by 1e3 (the planted fireflies).  specials: a pixel
    with a NaN on ONE channel of one sample and a firefly on another channel, a pixel with an infinite sample, a constant pixel,
    a -0.0 sample, and (six pixels and more, S >= 2) a pixel every sample of which is flagged at t = 1."""
    rng = np.random.default_rng(seed)
    c = rng.lognormal(-1.0, 1.0, (3, H, W, S))
    c[:, rng.random((H, W, S)) < 0.05] *= 1e3
    if not specials:
        return c
    order = rng.permutation(H * W)
    pos = [(int(i) // W, int(i) % W) for i in order]
    y, x = pos[0]
    c[0, y, x, S // 2] = np.nan
    c[1, y, x, 0] *= 1e4  # would be flagged on channel 1 if the NaN on channel 0 did not stop the pixel
    y, x = pos[1]
    c[2, y, x, S - 1] = np.inf
    y, x = pos[2]
    c[:, y, x, :] = np.array([0.5, 0.25, 0.125])[:, None]
    if H * W >= 6 and S >= 2:
        y, x = pos[3]
        c[:, y, x, :] = _skip_pixel(S)
        y, x = pos[4]
        c[1, y, x, 0] = -0.0
    return c
