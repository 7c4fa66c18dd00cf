"""The per-pass schedule of RPF_FLAG_SCHEDULE restated in numpy: stage 3c from a pixel's MI vector with the
sums in the kernels' order of additions, the two presets, and the per-pixel pass composed from leaves that exist --
oracle.pixel_stats, fast_weights_ref.neighbourhood or member_test_ref.members, oracle.mean_std, oracle.cf_weights (for the MI
alone), alpha_beta below and fast_weights_ref.pixel_colours(..., np.float64, form="direct").

A plain helper module (like member_test_ref.py): tests/test_schedule_cpu.py holds the host half of the library and this
restatement to the oracle, tests/test_schedule_gpu.py the device to this restatement.  Nothing here calls the library under
test."""
import numpy as np

import fast_weights_ref as R
import member_test_ref as MR

EPS = 1
BETA_REF_GCC11_O3, BETA_REF_GCC11_O2, BETA_PAPER = 0, 1, 2
MAX_BOXES = 8


def preset(kind, S):
    """(seed[8], gain_c[8], gain_f[8]) of rpf_schedule_preset: kind 0 the reference (0.002, 1, 1), kind 1 "published, from
    memory": seed[t] = sqrt(8 v_t / S), v_0 = 0.02, v_t = 0.002 otherwise; gain_c[t] = 2 (1 + 0.1 t); gain_f[t] = 1 + 0.1 t --
    in doubles, in exactly these expressions"""
    if kind == 0:
        return np.full(MAX_BOXES, 0.002), np.ones(MAX_BOXES), np.ones(MAX_BOXES)
    if kind != 1 or S <= 0:
        raise ValueError((kind, S))
    seed, gc, gf = np.empty(MAX_BOXES), np.empty(MAX_BOXES), np.empty(MAX_BOXES)
    for t in range(MAX_BOXES):
        v_t = 0.02 if t == 0 else 0.002
        seed[t] = np.sqrt(np.float64(8.0 * v_t / float(S)))
        gc[t] = 2.0 * (1.0 + 0.1 * t)
        gf[t] = 1.0 + 0.1 * t
    return seed, gc, gf


def _chain(terms):
    """0.0 + t0 + t1 + ... left to right, as `double D = 0.0; for (...) D += t;` rounds it"""
    acc = np.zeros_like(terms[0])
    for t in terms:
        acc = acc + t
    return acc


def ratios(mi, eps_or_0, n_random=2, n_feat=12):
    """the sums and ratios of stage 3c from MI vectors [..., npair] in call order (rpf.cpp:416-442: feature k against the nR
    random parameters and the 2 positions; colour c against the random parameters, the positions and the nF features): a dict
    with W_r_c [..., 3], W_r_f [..., nF], D_f_ck [..., 3], D_r_fk [..., nF], D_cf_k [..., nF] and den [...]"""
    mi = np.asarray(mi, np.float64)
    nR, nF = n_random, n_feat
    nAnc, npairF, npairC = nR + 2, nF * (nR + 2), nR + 2 + nF
    assert mi.shape[-1] == npairF + 3 * npairC
    with np.errstate(invalid="ignore", divide="ignore"):
        Drf = np.stack([_chain([mi[..., k * nAnc + l] for l in range(nR)]) for k in range(nF)], -1)
        Dpf = np.stack([_chain([mi[..., k * nAnc + nR + l] for l in range(2)]) for k in range(nF)], -1)
        Dcf = np.stack([_chain([mi[..., npairF + c * npairC + nAnc + k] for c in range(3)]) for k in range(nF)], -1)
        Drc = np.stack([_chain([mi[..., npairF + c * npairC + l] for l in range(nR)]) for c in range(3)], -1)
        Dpc = np.stack([_chain([mi[..., npairF + c * npairC + nR + l] for l in range(2)]) for c in range(3)], -1)
        Dfc = np.stack([_chain([mi[..., npairF + c * npairC + nAnc + j] for j in range(nF)]) for c in range(3)], -1)
        D_f_c, D_r_c, D_p_c = (_chain([D[..., i] for i in range(3)]) for D in (Dfc, Drc, Dpc))
        den = D_f_c + D_r_c + D_p_c + eps_or_0
        W_r_c = Drc / (Drc + Dpc + eps_or_0)
        W_r_f = Drf / (Drf + Dpf + eps_or_0)
    return dict(W_r_c=W_r_c, W_r_f=W_r_f, D_f_ck=Dfc, D_r_fk=Drf, D_cf_k=Dcf, den=den)


def numerators(r, beta_map, n_feat=12):
    """NUM_k of beta_k: the PAPER sum, or the reference's stack rule (k < 3: D_f_ck, a gap of zeros, then D_r_fk)"""
    if beta_map == BETA_PAPER:
        return r["D_cf_k"]
    gap = 8 if beta_map == BETA_REF_GCC11_O2 else 4
    cols = []
    for k in range(n_feat):
        cols.append(r["D_f_ck"][..., k] if k < 3 else (np.zeros_like(r["den"]) if k < gap else r["D_r_fk"][..., k - gap]))
    return np.stack(cols, -1)


def factor(g, w):
    """clamp0(1 - g * w): one rounding for the product, one for the difference; a NaN stays a NaN (v < 0 is false)"""
    with np.errstate(invalid="ignore"):
        t = np.float64(g) * np.asarray(w, np.float64)
        v = 1.0 - t
        return np.where(v < 0, 0.0, v)


def alpha_beta(mi, gain_c, gain_f, beta_map, eps_or_0, n_random=2, n_feat=12):
    """(alpha [..., 3], beta [..., nF], wrc [...]) of stage 3c under gains (gain_c, gain_f).  Gains of exactly 1 take the
    unscheduled statements (alpha = 1 - W, beta = (1 - W) * (NUM / den)), as the library does"""
    r = ratios(mi, eps_or_0, n_random, n_feat)
    num = numerators(r, beta_map, n_feat)
    with np.errstate(invalid="ignore", divide="ignore"):
        wcf = num / r["den"][..., None]
        if gain_c == 1.0 and gain_f == 1.0:
            alpha, beta = 1 - r["W_r_c"], (1 - r["W_r_f"]) * wcf
        else:
            alpha, beta = factor(gain_c, r["W_r_c"]), factor(gain_f, r["W_r_f"]) * wcf
        wrc = _chain([r["W_r_c"][..., i] for i in range(3)]) / 3
    return alpha, beta, wrc


def shares(mi, gain, which, eps_or_0, n_random=2, n_feat=12):
    """(clamped, open) shares of the entries of alpha (which = "c") or of beta's factor (which = "f") under `gain`: 1 - g W < 0, and
    0 < 1 - g W < 1"""
    w = ratios(mi, eps_or_0, n_random, n_feat)["W_r_c" if which == "c" else "W_r_f"]
    with np.errstate(invalid="ignore"):
        v = 1.0 - np.float64(gain) * w
        return float((v < 0).mean()), float(((v > 0) & (v < 1)).mean())


def pixel_colours(nb, S, M, SD, alpha, beta, wrc, box, seed, policy, n_random=2, n_feat=12):
    """fast_weights_ref.pixel_colours(..., np.float64, form="direct").  A box below 4 has sigma_p = box // 4 = 0 (rpf.cpp:531:
    integer division), and that function forms 1 / (2 sigma_p^2) in Python floats, which raise where IEEE arithmetic gives inf:
    for such a box the same statements follow here with the quotient in numpy doubles.  (inf * 0 = NaN: an own sample meets
    itself at distance 0, its weight and so its colour are NaN, and under EPS the colour falls back to the input.)"""
    if box // 4 > 0:
        return R.pixel_colours(nb, S, M, SD, alpha, beta, wrc, box, seed, policy, np.float64, n_random, n_feat, form="direct")
    cols = R.weighted_columns(n_random, n_feat)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        z = np.where(SD == 0, 0.0, (nb - M) / SD)[:, cols]
        sigma_p = np.float64(box // 4)
        sigma_c2 = seed * seed / (1 - wrc) / (1 - wrc)
        coef = np.concatenate([np.full(2, np.float64(1.0) / (2 * sigma_p * sigma_p)), alpha / (2 * sigma_c2), beta / (2 * sigma_c2)])
        E = np.zeros((S, nb.shape[0]))
        for k in range(len(cols)):
            d = z[:S, k, None] - z[None, :, k]
            E += (d * d) * coef[k]
        w = np.exp(-E)
        c = nb[:, 2:5]
        prime = (w @ c) / w.sum(axis=1)[:, None]
    if policy == EPS:
        prime = np.where(np.isnan(prime), c[:S], prime)
    return prime.T


def scheduled_pass(oracle, planes, entry, box, policy=EPS, beta_map=0, eps=1e-10, colour64=None, mt=None, cfg=None, pass_id=0):
    """one pass over every pixel of fp32 `planes` [19, H, W, S] under the schedule entry (seed, gain_c, gain_f): nbhd_size, mean,
    stddev, mi, alpha, beta, wrc, colour.  Members: the reference's full box (mt None, cfg None), or member_test_ref.members under
    the test mt = (mult, floor) and / or the draws cfg = (seed, row_origin, D) of pass `pass_id`"""
    seed, gc, gf = entry
    p32 = np.ascontiguousarray(planes, np.float32)
    nd, H, W, S = p32.shape
    pmean, pstd = MR.stats_of(oracle, p32, policy)
    e = eps if policy == EPS else 0.0
    out = dict(nbhd_size=np.zeros((H, W), np.int32), mean=np.zeros((H, W, nd)), stddev=np.zeros((H, W, nd)), mi=np.zeros((H, W, 96)),
               alpha=np.zeros((H, W, 3)), beta=np.zeros((H, W, 12)), wrc=np.zeros((H, W)), colour=np.zeros((3, H, W, S)))
    for y in range(H):
        for x in range(W):
            if mt is None and cfg is None:
                nb = R.neighbourhood(p32, pmean, pstd, y, x, box, colour64=colour64)
            else:
                nb, _ = MR.members(p32, pmean, pstd, mt if mt is not None else MR.reference(), y, x, box, colour64=colour64, cfg=cfg,
                                   pass_id=pass_id)
            M, SD = oracle.mean_std(nb)
            if policy == EPS:
                SD = np.where(np.isnan(SD), 0.0, SD)
            with np.errstate(invalid="ignore", divide="ignore"):
                z = np.where(SD == 0, 0.0, (nb - M) / SD)
            _, _, _, mi = oracle.cf_weights(z, beta_map, policy, eps)
            a, bt, w = alpha_beta(mi, gc, gf, beta_map, e)
            out["nbhd_size"][y, x], out["mean"][y, x], out["stddev"][y, x], out["mi"][y, x] = nb.shape[0], M, SD, mi
            out["alpha"][y, x], out["beta"][y, x], out["wrc"][y, x] = a, bt, w
            out["colour"][:, y, x, :] = pixel_colours(nb, S, M, SD, a, bt, w, box, seed, policy)
    return out


def stage4_on(oracle, planes, got, seed, box, policy=EPS, colour64=None, mt=None, cfg=None, pass_id=0, rows=None, n_random=2, n_feat=12):
    """fast_weights_ref's stage 4 on the stage outputs `got` (the device's own: mean, stddev, alpha, beta, wrc) and the
    restatement's member rows; [3, H, W, S].  rows: restate these rows alone, the others stay zero"""
    p32 = np.ascontiguousarray(planes, np.float32)
    _, H, W, S = p32.shape
    pmean, pstd = MR.stats_of(oracle, p32, policy, n_random, n_feat)
    out = np.empty((3, H, W, S)) if rows is None else np.zeros((3, H, W, S))
    for y in (range(H) if rows is None else rows):
        for x in range(W):
            if mt is None and cfg is None:
                nb = R.neighbourhood(p32, pmean, pstd, y, x, box, n_random, n_feat, colour64=colour64)
            else:
                nb, _ = MR.members(p32, pmean, pstd, mt if mt is not None else MR.reference(n_feat), y, x, box, n_random, n_feat,
                                   colour64=colour64, cfg=cfg, pass_id=pass_id)
            assert nb.shape[0] == got["nbhd_size"][y, x], ((y, x), nb.shape[0], int(got["nbhd_size"][y, x]))
            out[:, y, x, :] = pixel_colours(nb, S, got["mean"][y, x], got["stddev"][y, x], got["alpha"][y, x], got["beta"][y, x],
                                            got["wrc"][y, x], box, seed, policy, n_random, n_feat)
    return out
