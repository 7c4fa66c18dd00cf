"""The membership test of RPF_FLAG_MEMBER_TEST restated in numpy, and the per-pixel pass composed from
leaves that exist -- oracle.pixel_stats, the predicate below, oracle.mean_std, normalisation with SD == 0 giving 0,
oracle.cf_weights and fast_weights_ref.pixel_colours(..., np.float64, form="direct").  Candidates: every sample of the box in
the reference's visiting order, or -- cfg given -- the draws of sampled_ref.draws.

A plain helper module (like sampled_ref.py): tests/test_member_test_cpu.py holds the host half of the library to it,
tests/test_member_test_gpu.py the device.  Nothing here calls the library under test."""
import numpy as np

import fast_weights_ref as R
import sampled_ref as SR

EPS = 1
CAPS = (8, 16, 32, 64, 128, 256, 448, 832)


def reference(n_feat=12):
    """multiples 3, floors -1: the reference's test (rpf_membership_preset kind 0)"""
    return np.full(n_feat, 3.0), np.full(n_feat, -1.0)


def published19(floor_scale=1.0):
    """multiples 3, 30 on the world positions (features 3..5, 9..11), floors 0.1 (rpf_membership_preset kind 1), the floors
    times floor_scale"""
    mult = np.full(12, 3.0)
    mult[3:6] = mult[9:12] = 30.0
    return mult, np.full(12, 0.1 * floor_scale)


def rejected(f, m, sd, mult, floor):
    """[n] bool: candidates with feature rows f [n, nF] that some feature rejects, for a pixel with mean m and deviation sd:
    a = |f - m|, lim = sd * mult, fl = -inf where sd > floor else floor; rejected on k iff a >= lim and a > fl.  Comparisons
    with a NaN are false"""
    f, m, sd = np.asarray(f, np.float64), np.asarray(m, np.float64), np.asarray(sd, np.float64)
    mult, floor = np.asarray(mult, np.float64), np.asarray(floor, np.float64)
    with np.errstate(invalid="ignore"):
        a = np.abs(f - m)
        lim = sd * mult
        fl = np.where(sd > floor, -np.inf, floor)
        return ((a >= lim) & (a > fl)).any(axis=-1)


def class_of(n):
    return next((c for c in CAPS if n <= c), 833)   # 833: the rest list


def candidates(box, W, H, S, x, y, cfg=None, pass_id=0):
    """visiting-order indices qq of the candidates of pixel (x, y), ascending: the whole window, or the draws of cfg = (seed,
    row_origin, D)"""
    if cfg is not None:
        seed, row_origin, D = cfg
        return SR.draws(seed, pass_id, row_origin, D, box, W, H, S, x, y) if D > 0 else np.zeros(0, np.int64)
    b = (box - 1) // 2
    nx = min(x + b, W - 1) - max(x - b, 0) + 1
    ny = min(y + b, H - 1) - max(y - b, 0) + 1
    return np.arange((nx * ny - 1) * S, dtype=np.int64)


def members(planes, pmean, pstd, mt, y, x, box, n_random=2, n_feat=12, colour64=None, cfg=None, pass_id=0):
    """(rows [N, ndim] fp64, member codes [N]) of pixel (y, x): the own samples, then the candidates no feature rejects, in
    visiting order.  mt = (mult, floor); colour64 replaces columns 2..4"""
    _, H, W, S = planes.shape
    b, f0 = (box - 1) // 2, 5 + n_random
    own = planes[:, y, x, :].T.astype(np.float64)
    codes = [(b * box + b) * S + s for s in range(S)]
    qq = candidates(box, W, H, S, x, y, cfg, pass_id)
    xn, yn, s = SR.decode(qq, box, W, H, S, x, y)
    cand = planes[:, yn, xn, s].T.astype(np.float64)
    if colour64 is not None:
        c64 = np.asarray(colour64, np.float64)
        own[:, 2:5] = c64[:, y, x, :].T
        cand[:, 2:5] = c64[:, yn, xn, s].T
    keep = ~rejected(cand[:, f0:], pmean[y, x], pstd[y, x], mt[0][:n_feat], mt[1][:n_feat])
    codes += [int(v) for v in (((xn - x + b) * box + (yn - y + b)) * S + s)[keep]]
    return np.concatenate([own, cand[keep]], axis=0), np.array(codes, np.int64)


def stats_of(oracle, planes, policy=EPS, n_random=2, n_feat=12):
    p32 = np.ascontiguousarray(planes, np.float32)
    _, H, W, S = p32.shape
    lay = dict(n_random=n_random, n_feat=n_feat) if (n_random, n_feat) != (2, 12) else {}
    return oracle.pixel_stats(p32, oracle.make_desc(W, H, S, policy=policy, **lay))


def counts(oracle, planes, mt, box, n_random=2, n_feat=12, cfg=None, pass_id=0, rows=None):
    """(N [H, W], member codes per pixel) without the later stages"""
    p32 = np.ascontiguousarray(planes, np.float32)
    _, H, W, S = p32.shape
    pmean, pstd = stats_of(oracle, p32, EPS, n_random, n_feat)
    n, codes = np.zeros((H, W), np.int32), {}
    for y in (range(H) if rows is None else rows):
        for x in range(W):
            _, c = members(p32, pmean, pstd, mt, y, x, box, n_random, n_feat, None, cfg, pass_id)
            n[y, x], codes[(y, x)] = len(c), c
    return n, codes


def member_pass(oracle, planes, mt, box, seed_sigma=0.002, policy=EPS, beta_map=0, eps=1e-10, n_random=2, n_feat=12,
                colour64=None, weights=True, cfg=None, pass_id=0, rows=None):
    """one pass over every pixel of fp32 (or fp16-valued) `planes` [ndim, H, W, S] under the test mt = (mult, floor): nbhd_size,
    member_hash, mean, stddev and -- weights, the 19-dim layout only -- mi, alpha, beta, wrc, colour; `codes`: the member codes
    of every pixel.  rows (here, in counts and in stage4_on): restate these rows alone, the others stay zero"""
    p32 = np.ascontiguousarray(planes, np.float32)
    nd, H, W, S = p32.shape
    pmean, pstd = stats_of(oracle, p32, policy, n_random, n_feat)
    out = dict(nbhd_size=np.zeros((H, W), np.int32), member_hash=np.zeros((H, W), np.uint32), mean=np.zeros((H, W, nd)),
               stddev=np.zeros((H, W, nd)), codes={})
    if weights:
        assert (n_random, n_feat) == (2, 12)
        out.update(mi=np.zeros((H, W, 96)), alpha=np.zeros((H, W, 3)), beta=np.zeros((H, W, 12)), wrc=np.zeros((H, W)),
                   colour=np.zeros((3, H, W, S)))
    for y in (range(H) if rows is None else rows):
        for x in range(W):
            nb, codes = members(p32, pmean, pstd, mt, y, x, box, n_random, n_feat, colour64, cfg, pass_id)
            M, SD = oracle.mean_std(nb)
            if policy == EPS:
                SD = np.where(np.isnan(SD), 0.0, SD)
            out["nbhd_size"][y, x], out["member_hash"][y, x] = nb.shape[0], SR.fnv1a_u32(codes)
            out["mean"][y, x], out["stddev"][y, x], out["codes"][(y, x)] = M, SD, codes
            if not weights:
                continue
            with np.errstate(invalid="ignore", divide="ignore"):
                z = np.where(SD == 0, 0.0, (nb - M) / SD)
            a, bt, w, mi = oracle.cf_weights(z, beta_map, policy, eps)
            out["alpha"][y, x], out["beta"][y, x], out["wrc"][y, x], out["mi"][y, x] = a, bt, w, mi
            out["colour"][:, y, x, :] = R.pixel_colours(nb, S, M, SD, a, bt, w, box, seed_sigma, policy, np.float64, form="direct")
    return out


def stage4_on(oracle, planes, got, mt, box, seed_sigma, policy=EPS, colour64=None, cfg=None, pass_id=0, rows=None):
    """fast_weights_ref's stage 4 for a pass under the test: the colours of every pixel from the restatement's member rows and
    the stage outputs `got` (the device's own: the design of tests/test_stage4_per_sample_gpu.py); [3, H, W, S]"""
    p32 = np.ascontiguousarray(planes, np.float32)
    _, H, W, S = p32.shape
    pmean, pstd = stats_of(oracle, p32, policy)
    out = np.empty((3, H, W, S)) if rows is None else np.zeros((3, H, W, S))
    for y in (range(H) if rows is None else rows):
        for x in range(W):
            nb, _ = members(p32, pmean, pstd, mt, y, x, box, colour64=colour64, cfg=cfg, pass_id=pass_id)
            assert nb.shape[0] == got["nbhd_size"][y, x], ((y, x), nb.shape[0], int(got["nbhd_size"][y, x]))
            out[:, y, x, :] = R.pixel_colours(nb, S, got["mean"][y, x], got["stddev"][y, x], got["alpha"][y, x], got["beta"][y, x],
                                              got["wrc"][y, x], box, seed_sigma, policy, np.float64, form="direct")
    return out
