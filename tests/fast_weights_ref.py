"""Stage 4 (the S x N pair weights and the blend, rpf.cpp:637-717) restated in numpy for chosen pixels, with the precision
of the pair arithmetic as an argument: the CPU yardstick of RPF_FLAG_FAST_WEIGHTS.

A plain helper module (like pbrt_film_ref.py and planted_nbhd.py): tests/test_fast_weights_cpu.py proves the fp64 form
against the oracle and bounds the fp32 form's distance from it, tests/test_fast_weights_gpu.py holds the device's fp32 mode
to a small multiple of that distance.

Written from stage 4a / 4b of oracle/rpf_oracle.c, on the oracle's own stage outputs (mean, stddev, alpha, beta, W_r_c of the
pass): what is restated is the weight arithmetic alone.

  dtype = float64   everything in fp64: the oracle's colours to rounding (another order of the sums, one exp of the summed
                    exponent where the oracle multiplies three).
  dtype = float32   the arithmetic DESIGN.md section 4 documents for the flag: z = (x - M) / SD is formed in fp64 and rounded
                    to fp32, the coefficients 1 / (2 sigma_p^2), alpha / (2 sigma_c^2), beta / (2 sigma_f^2) are formed in
                    fp64 and rounded to fp32; differences, squares and the weighted sum over the 17 weighted columns in
                    fp32; ONE fp32 exp of the summed exponent; the weights widened to fp64, both sums and the quotient in
                    fp64.

Nothing here knows how the kernel orders its work (lanes, sweeps, fused multiply-adds, the reciprocal of SD, the base-2
hardware exponential): those are what the factor of the regression bar in test_fast_weights_gpu.py pays for."""
import numpy as np

import planted_nbhd as P

EPS, REF_ABORT = 1, 0


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def weighted_columns(n_random=2, n_feat=12):
    """columns of the sample vector that carry weight: pFilm (2), colour (3), the features; the random parameters carry none"""
    return np.array([0, 1, 2, 3, 4] + [5 + n_random + k for k in range(n_feat)])


def neighbourhood(planes, pmean, pstd, y, x, box, n_random=2, n_feat=12, colour64=None):
    """the member samples of pixel (y, x) as rows [N, ndim] in fp64, in the oracle's order: the own samples, then the window
    x outer / y inner / s, every candidate that fails no feature's |f - m| >= 3 sd test (a NaN never rejects); colour64
    (three fp64 planes [3, H, W, S], the colours an earlier pass left) replaces columns 2..4"""
    _, H, W, S = planes.shape
    b, f0 = (box - 1) // 2, 5 + n_random
    x0, x1, y0, y1 = max(x - b, 0), min(x + b, W - 1), max(y - b, 0), min(y + b, H - 1)
    win = planes[:, y0:y1 + 1, x0:x1 + 1, :].transpose(2, 1, 3, 0).astype(np.float64)      # [x, y, s, dim]
    if colour64 is not None:
        win[..., 2:5] = np.asarray(colour64, np.float64)[:, y0:y1 + 1, x0:x1 + 1, :].transpose(2, 1, 3, 0)
    with np.errstate(invalid="ignore"):
        rejected = (np.abs(win[..., f0:] - pmean[y, x]) >= pstd[y, x] * 3).any(axis=-1)
    keep = ~rejected
    keep[x - x0, y - y0, :] = False
    return np.concatenate([win[x - x0, y - y0], win[keep]], axis=0)


def pixel_colours(nb, S, M, SD, alpha, beta, wrc, box, seed, policy, dtype, n_random=2, n_feat=12, fallback=True,
                  form="direct", mutate=None):
    """filtered colours [3, S] of the pixel whose neighbourhood is nb (own samples first); fallback: under the EPS policy a NaN
    colour is replaced by the sample's input colour, as the oracle does.

    form = "direct"    E_ij = sum_k cz_k (z_ik - z_jk)^2, term by term: the oracle's and the generic kernels' expression.
    form = "expanded"  E_ij = A_i + B_j + sum_k u_ik z_jk with cz_k = weight_k / (2 sigma^2), A_i = sum_k cz_k z_ik^2,
                       B_j = sum_k cz_k z_jk^2, u_ik = -2 cz_k z_ik (the fused kernels).  Used by
                       the CPU checks of the per-sample bar (tests/stage4_bars.py) alone.

    mutate: None, or a function w[S, N] -> w[S, N] applied to the fp64 weights before the sums -- the planted faults of
    tests/test_stage4_per_sample_cpu.py; no other caller passes it."""
    if form not in ("direct", "expanded"):
        raise ValueError(form)
    cols = weighted_columns(n_random, n_feat)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where(SD == 0, 0.0, (nb - M) / SD)[:, cols]
        sigma_p = float(box // 4)
        sigma_c2 = seed * seed / (1 - wrc) / (1 - wrc)                                   # = sigma_f^2
        coef = np.concatenate([np.full(2, 1 / (2 * sigma_p * sigma_p)), alpha / (2 * sigma_c2), beta / (2 * sigma_c2)])
        z, coef = z.astype(dtype), coef.astype(dtype)
        if form == "direct":
            E = np.zeros((S, nb.shape[0]), dtype)
            for k in range(len(cols)):
                d = z[:S, k, None] - z[None, :, k]
                E += (d * d) * coef[k]
        else:
            B = np.zeros(nb.shape[0], dtype)
            for k in range(len(cols)):
                B += (coef[k] * z[:, k]) * z[:, k]
            E = B[:S, None] + B[None, :]                                                  # A_i: the same sum of the same products
            for k in range(len(cols)):
                E += (dtype(-2.0) * (coef[k] * z[:S, k]))[:, None] * z[None, :, k]
        assert E.dtype == dtype
        w = np.exp(-E)
        assert w.dtype == dtype
        w = w.astype(np.float64)
        if mutate is not None:
            w = mutate(w)
        c = nb[:, 2:5]
        prime = (w @ c) / w.sum(axis=1)[:, None]                                          # [S, 3]
    if policy == EPS and fallback:
        prime = np.where(np.isnan(prime), c[:S], prime)
    return prime.T


def stage4(oracle, planes, want, box, seed, pixels, dtype, policy=EPS, n_random=2, n_feat=12, fallback=True, colour64=None,
           form="direct", mutate=None):
    """colours [3, len(pixels), S] of `pixels` = [(y, x), ...] of the fp32 `planes`, from the debug outputs `want` of a pass
    over them (box, sigma seed, policy and layout as given to that pass).

    `want` is any dict with nbhd_size, mean, stddev, alpha, beta, wrc.  The oracle's outputs make this the restatement of the
    oracle's stage 4.  The DEVICE's own debug outputs work as they stand, and that is the point of the design of
    tests/test_stage4_per_sample_gpu.py: check_pass already holds the device's stage 1 to 3 outputs to the oracle, so what
    remains between the device's colours and stage4(..., got, ..., np.float64) is the device's pair arithmetic and blend alone
    -- the 1e-9 slack allowed on alpha / beta, times an exponent of up to 745, does not pollute the comparison.

    colour64: three fp64 planes, the colours an earlier pass left: a second pass reads them both as the blended values and
    as the colour columns of z (planes[2:5] is then not read).  form: see pixel_colours.  mutate(w, index of the pixel in
    `pixels`) -> w: a planted fault (tests/test_stage4_per_sample_cpu.py)."""
    _, H, W, S = planes.shape
    lay = dict(n_random=n_random, n_feat=n_feat) if (n_random, n_feat) != (2, 12) else {}
    pmean, pstd = oracle.pixel_stats(planes, oracle.make_desc(W, H, S, policy=policy, **lay))    # (EPS clamps a NaN sigma to 0)
    out = np.empty((3, len(pixels), S))
    for i, (y, x) in enumerate(pixels):
        nb = neighbourhood(planes, pmean, pstd, y, x, box, n_random, n_feat, colour64)
        assert nb.shape[0] == want["nbhd_size"][y, x], ((y, x), nb.shape[0], int(want["nbhd_size"][y, x]))
        out[:, i] = pixel_colours(nb, S, want["mean"][y, x], want["stddev"][y, x], want["alpha"][y, x], want["beta"][y, x],
                                  want["wrc"][y, x], box, seed, policy, dtype, n_random, n_feat, fallback, form,
                                  None if mutate is None else (lambda w, i=i: mutate(w, i)))
    return out


_rows = {}


def target_row(oracle, fid, policy, seed, dtype):
    """the check set of a planted frame -- every pixel of the target row y = b, which holds all targets -- through stage4:
    colours [3, W, S]; computed once per session, shared, never modified"""
    key = (fid, policy, seed, np.dtype(dtype).name)
    if key not in _rows:
        (nr, nf, _), S, box, targets, _, _ = P.FRAMES[fid]
        b, W = (box - 1) // 2, box * len(targets)
        want = P.oracle_pass(oracle, fid, policy, seed)
        r = stage4(oracle, P.frame(fid)[1], want, box, seed, [(b, x) for x in range(W)], dtype, policy, nr, nf)
        r.setflags(write=False)
        _rows[key] = r
    return _rows[key]


def row_distance(oracle, fid, policy, seed, dtype):
    """rel-L2 of target_row against the oracle's colours of that row, over the entries the oracle leaves finite"""
    b = (P.FRAMES[fid][2] - 1) // 2
    ref = P.oracle_pass(oracle, fid, policy, seed)["colour"][:, b]
    fin = np.isfinite(ref)
    return rel_l2(target_row(oracle, fid, policy, seed, dtype)[fin], ref[fin])
