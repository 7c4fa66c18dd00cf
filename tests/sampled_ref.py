"""Sampled neighbourhoods (RPF_FLAG_SAMPLED_NBHD) restated in numpy: the draws of a pixel's key in
uint64 arithmetic, the member list they name, and the per-pixel pass composed from leaves that exist -- oracle.pixel_stats, the
3-sigma predicate of fast_weights_ref.neighbourhood, rpf_oracle_mean_std, normalisation with SD == 0 giving 0,
rpf_oracle_cf_weights and fast_weights_ref.pixel_colours(..., np.float64, form="direct").

A plain helper module (like fast_weights_ref.py and spike_ref.py): tests/test_sampled_cpu.py holds rpf_sampling_table /
rpf_sampling_draws to it, tests/test_sampled_gpu.py the device.  Nothing here calls the library under test."""
import numpy as np

import fast_weights_ref as R

EPS = 1
G = np.uint64(0x9E3779B97F4A7C15)
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
U32 = np.uint64(0xFFFFFFFF)


def mix(z):
    """the SplitMix64 finaliser on uint64 scalars or arrays (wrapping multiplies)"""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z ^ (z >> np.uint64(30))
        z = z * M1
        z = z ^ (z >> np.uint64(27))
        z = z * M2
        z = z ^ (z >> np.uint64(31))
    return z


def table(box, dtype=np.longdouble):
    """T[k] = floor(2^32 C_k / C_(box-1)), k = 0 .. box - 2, C_k = sum_{j <= k} exp(-(j - b)^2 / (2 sigma^2)), sigma = box / 4;
    dtype: the precision of the formula (the library's is long double)"""
    b, sigma = (box - 1) // 2, dtype(box) / dtype(4)
    acc, c = dtype(0), []
    for j in range(box):
        dj = dtype(j - b)
        acc = acc + np.exp(-(dj * dj) / (dtype(2) * sigma * sigma))
        c.append(acc)
    return np.array([int(np.floor(np.ldexp(c[k] / c[box - 1], 32))) for k in range(box - 1)], np.uint64).astype(np.uint32)


_tables = {}


def _table(box):
    if box not in _tables:
        _tables[box] = table(box).astype(np.uint64)
    return _tables[box]


def pixel_key(seed, pass_id, row_origin, x, y):
    with np.errstate(over="ignore"):
        h = mix(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + G)
    h = mix(h ^ np.uint64(pass_id & 0xFFFFFFFF))
    h = mix(h ^ np.uint64((row_origin + y) & 0xFFFFFFFF))
    return mix(h ^ np.uint64(x & 0xFFFFFFFF))


def raw_draws(seed, pass_id, row_origin, D, box, S, x, y):
    """(dx, dy, s) of the D draws of buffer pixel (x, y), in draw order, before any discard: int64 arrays"""
    T, b = _table(box), (box - 1) // 2
    q = np.arange(1, D + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        r = mix(pixel_key(seed, pass_id, row_origin, x, y) + q * G)
    r2 = mix(r ^ G)
    ix = (T[None, :] <= (r & U32)[:, None]).sum(axis=1)
    iy = (T[None, :] <= (r >> np.uint64(32))[:, None]).sum(axis=1)
    s = ((r2 & U32) * np.uint64(S)) >> np.uint64(32)
    return ix.astype(np.int64) - b, iy.astype(np.int64) - b, s.astype(np.int64)


def draws(seed, pass_id, row_origin, D, box, W, H, S, x, y):
    """the distinct surviving visiting-order indices qq of buffer pixel (x, y), ascending (what rpf_sampling_draws returns): a draw
    outside the buffer or on the centre pixel is discarded with no redraw; qq numbers the window xn outer, yn inner, centre
    skipped, then s"""
    dx, dy, s = raw_draws(seed, pass_id, row_origin, D, box, S, x, y)
    b = (box - 1) // 2
    xn, yn = x + dx, y + dy
    ok = (xn >= 0) & (xn < W) & (yn >= 0) & (yn < H) & ~((xn == x) & (yn == y))
    x0, y0, y1 = max(x - b, 0), max(y - b, 0), min(y + b, H - 1)
    nyv = y1 - y0 + 1
    cell = (xn - x0) * nyv + (yn - y0)
    cell = np.where(cell > (x - x0) * nyv + (y - y0), cell - 1, cell)
    return np.unique((cell * S + s)[ok]).astype(np.int64)


def decode(qq, box, W, H, S, x, y):
    """(xn, yn, s) of visiting-order indices of pixel (x, y): candidate_offset of rpf_generic_common.h"""
    b = (box - 1) // 2
    x0, y0, y1 = max(x - b, 0), max(y - b, 0), min(y + b, H - 1)
    nyv = y1 - y0 + 1
    qq = np.asarray(qq, np.int64)
    cell, s = qq // S, qq % S
    cell = np.where(cell >= (x - x0) * nyv + (y - y0), cell + 1, cell)
    return x0 + cell // nyv, y0 + cell % nyv, s


def fnv1a_u32(codes):
    h = 2166136261
    for v in codes:
        for i in range(4):
            h = ((h ^ ((int(v) >> (8 * i)) & 0xFF)) * 16777619) & 0xFFFFFFFF
    return h


def members(planes, pmean, pstd, cfg, pass_id, y, x, box, n_random=2, n_feat=12, colour64=None):
    """(rows [N, ndim] fp64, member codes [N], accepted qq) of pixel (y, x): the own samples, then the distinct draws that fail
    no feature's |f - m| >= 3 sd test (a NaN never rejects) in ascending qq -- built like fast_weights_ref.neighbourhood.
    cfg = (seed, row_origin, D); colour64 replaces columns 2..4"""
    seed, row_origin, D = cfg
    _, H, W, S = planes.shape
    b, f0 = (box - 1) // 2, 5 + n_random
    own = planes[:, y, x, :].T.astype(np.float64)
    codes = [(b * box + b) * S + s for s in range(S)]
    qq = draws(seed, pass_id, row_origin, D, box, W, H, S, x, y) if D > 0 else np.zeros(0, np.int64)
    xn, yn, s = decode(qq, box, W, H, S, x, y)
    cand = planes[:, yn, xn, s].T.astype(np.float64)                       # [n, ndim]
    if colour64 is not None:
        c64 = np.asarray(colour64, np.float64)
        own[:, 2:5] = c64[:, y, x, :].T
        cand[:, 2:5] = c64[:, yn, xn, s].T
    with np.errstate(invalid="ignore"):
        keep = ~(np.abs(cand[:, f0:] - pmean[y, x]) >= pstd[y, x] * 3).any(axis=-1)
    codes += [int(v) for v in (((xn - x + b) * box + (yn - y + b)) * S + s)[keep]]
    return np.concatenate([own, cand[keep]], axis=0), np.array(codes, np.int64), qq[keep]


def full_box_codes(planes, pmean, pstd, y, x, box, n_random=2, n_feat=12):
    """member codes of the unsampled neighbourhood of pixel (y, x), in order (the list a sampled list is a subsequence of)"""
    _, H, W, S = planes.shape
    b, f0 = (box - 1) // 2, 5 + n_random
    codes = [(b * box + b) * S + s for s in range(S)]
    for xn in range(max(x - b, 0), min(x + b, W - 1) + 1):
        for yn in range(max(y - b, 0), min(y + b, H - 1) + 1):
            if xn == x and yn == y:
                continue
            f = planes[f0:, yn, xn, :].T.astype(np.float64)
            with np.errstate(invalid="ignore"):
                keep = ~(np.abs(f - pmean[y, x]) >= pstd[y, x] * 3).any(axis=-1)
            codes += [((xn - x + b) * box + (yn - y + b)) * S + int(s) for s in np.nonzero(keep)[0]]
    return codes


def is_subsequence(a, b):
    it = iter(b)
    return all(any(v == w for w in it) for v in a)


def sampled_pass(oracle, planes, cfg, pass_id, box, seed_sigma=0.002, policy=EPS, beta_map=0, eps=1e-10, n_random=2, n_feat=12,
                 colour64=None, weights=True, rows=None):
    """one sampled pass over every pixel of fp32 (or fp16-valued) `planes` [ndim, H, W, S]: nbhd_size, member_hash, mean, stddev
    and -- weights, the 19-dim layout only: rpf_oracle_cf_weights is 19-dim -- mi, alpha, beta, wrc, colour; `codes`: the member
    codes of every pixel.  cfg = (seed, row_origin, D); rows: restate these rows alone (the others stay zero)"""
    p32 = np.ascontiguousarray(planes, np.float32)
    nd, H, W, S = p32.shape
    lay = dict(n_random=n_random, n_feat=n_feat) if (n_random, n_feat) != (2, 12) else {}
    pmean, pstd = oracle.pixel_stats(p32, oracle.make_desc(W, H, S, policy=policy, **lay))
    out = dict(nbhd_size=np.zeros((H, W), np.int32), member_hash=np.zeros((H, W), np.uint32), mean=np.zeros((H, W, nd)),
               stddev=np.zeros((H, W, nd)), codes={})
    if weights:
        assert (n_random, n_feat) == (2, 12)
        out.update(mi=np.zeros((H, W, 96)), alpha=np.zeros((H, W, 3)), beta=np.zeros((H, W, 12)), wrc=np.zeros((H, W)),
                   colour=np.zeros((3, H, W, S)))
    for y in (range(H) if rows is None else rows):
        for x in range(W):
            nb, codes, _ = members(p32, pmean, pstd, cfg, pass_id, y, x, box, n_random, n_feat, colour64)
            M, SD = oracle.mean_std(nb)
            if policy == EPS:
                SD = np.where(np.isnan(SD), 0.0, SD)
            out["nbhd_size"][y, x], out["member_hash"][y, x] = nb.shape[0], fnv1a_u32(codes)
            out["mean"][y, x], out["stddev"][y, x], out["codes"][(y, x)] = M, SD, codes
            if not weights:
                continue
            with np.errstate(invalid="ignore", divide="ignore"):
                z = np.where(SD == 0, 0.0, (nb - M) / SD)
            a, bt, w, mi = oracle.cf_weights(z, beta_map, policy, eps)
            out["alpha"][y, x], out["beta"][y, x], out["wrc"][y, x], out["mi"][y, x] = a, bt, w, mi
            out["colour"][:, y, x, :] = R.pixel_colours(nb, S, M, SD, a, bt, w, box, seed_sigma, policy, np.float64, form="direct")
    return out


def stage4_on(oracle, planes, got, cfg, pass_id, box, seed_sigma, policy=EPS, colour64=None, rows=None, n_random=2, n_feat=12):
    """fast_weights_ref.stage4 for a sampled pass: the colours of every pixel from the restatement's member rows and the stage
    outputs `got` (the device's own: the design of tests/test_stage4_per_sample_gpu.py); [3, H, W, S]"""
    p32 = np.ascontiguousarray(planes, np.float32)
    _, H, W, S = p32.shape
    lay = dict(n_random=n_random, n_feat=n_feat) if (n_random, n_feat) != (2, 12) else {}
    pmean, pstd = oracle.pixel_stats(p32, oracle.make_desc(W, H, S, policy=policy, **lay))
    out = np.empty((3, H, W, S)) if rows is None else np.zeros((3, H, W, S))
    for y in (range(H) if rows is None else rows):
        for x in range(W):
            nb, _, _ = members(p32, pmean, pstd, cfg, pass_id, y, x, box, n_random, n_feat, colour64)
            assert nb.shape[0] == got["nbhd_size"][y, x], ((y, x), nb.shape[0], int(got["nbhd_size"][y, x]))
            out[:, y, x, :] = R.pixel_colours(nb, S, got["mean"][y, x], got["stddev"][y, x], got["alpha"][y, x], got["beta"][y, x],
                                              got["wrc"][y, x], box, seed_sigma, policy, np.float64, n_random, n_feat, form="direct")
    return out
