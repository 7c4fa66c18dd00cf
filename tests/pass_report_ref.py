"""NumPy restatement of the per-pass activity report (RPF_FLAG_PASS_REPORT).  IEEE fp64, every sum a serial
chain whose first term is its first element; numpy's elementwise + and * round once each and never contract, so the records below
compare bit for bit with the library's.

A record is a dict: the doubles as float64 arrays (moved2, in2, pix_moved2, pix_in2, alpha_sum [3]; wrc_sum []; beta_sum
[MAX_NDIM]) and the counts as int64 (sum_nbhd, own_only_pixels, class_pixels [9], unchanged_samples, nonfinite_samples,
nonfinite_pixels, weights_nonfinite, alpha_zero [3], beta_zero [MAX_NDIM], min_nbhd, max_nbhd)."""
import numpy as np

MAX_NDIM = 40
CAPS = (8, 16, 32, 64, 128, 256, 448, 832)      # class_capacity(0 .. 7): the bounds of the routes' size classes
DOUBLES = ("moved2", "in2", "pix_moved2", "pix_in2", "alpha_sum", "wrc_sum", "beta_sum")
COUNTS = ("sum_nbhd", "own_only_pixels", "class_pixels", "unchanged_samples", "nonfinite_samples", "nonfinite_pixels",
          "weights_nonfinite", "alpha_zero", "beta_zero")
FIELDS = DOUBLES + COUNTS + ("min_nbhd", "max_nbhd")


def chain(v, axis):
    """v[0] + v[1] + ... along `axis`, in that order"""
    v = np.moveaxis(np.asarray(v, np.float64), axis, 0)
    acc = v[0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for t in v[1:]:
            acc = acc + t
    return acc


def pixel_values(a, b):
    """a, b: float64 [3, R, W, S] -> (values [R, W, 12] = m_k | i_k | pm_k | pi_k with +0.0 on bad pixels, unchanged samples [R, W],
    samples that hold a non-finite value [R, W])"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        m, i2, pa, pb = chain(d * d, -1), chain(a * a, -1), chain(a, -1), chain(b, -1)
        dp = pb - pa
        pm, pi = dp * dp, pa * pa
    bad_s = ~(np.isfinite(a).all(axis=0) & np.isfinite(b).all(axis=0))                      # [R, W, S]
    nonfinite = bad_s.sum(axis=-1).astype(np.int64)
    unchanged = (a.view(np.uint64) == b.view(np.uint64)).all(axis=0).sum(axis=-1).astype(np.int64)
    vals = np.moveaxis(np.concatenate([m, i2, pm, pi]), 0, -1)                               # [R, W, 12]
    vals = np.where((nonfinite > 0)[..., None], 0.0, vals)
    return vals, unchanged, nonfinite


def weight_chain(w):
    """w: float64 [W, K] -> (chain over x of the finite entries, +0.0 for the others [K]; entries == 0.0 [K]; non-finite entries)"""
    fin = np.isfinite(w)
    return chain(np.where(fin, w, 0.0), 0), (w == 0.0).sum(axis=0).astype(np.int64), int((~fin).sum())


def rows(a, b, nbhd, alpha, beta, wrc, row_begin=0, row_end=None):
    """The row records of rows [row_begin, row_end): a, b float64 [3, H, W, S]; nbhd int [H, W]; alpha [H, W, 3], beta [H, W, n_feat],
    wrc [H, W] float64, each may be None (its fields are then zero)"""
    _, H, W, S = a.shape
    r1 = H if row_end is None else row_end
    vals, unchanged, nonfinite = pixel_values(a[:, row_begin:r1], b[:, row_begin:r1])
    out = []
    for i, y in enumerate(range(row_begin, r1)):
        rec = {k: np.zeros(3) for k in ("moved2", "in2", "pix_moved2", "pix_in2", "alpha_sum")}
        rec.update(wrc_sum=np.zeros(()), beta_sum=np.zeros(MAX_NDIM), alpha_zero=np.zeros(3, np.int64), beta_zero=np.zeros(MAX_NDIM, np.int64))
        s = chain(vals[i], 0)
        rec["moved2"], rec["in2"], rec["pix_moved2"], rec["pix_in2"] = s[0:3], s[3:6], s[6:9], s[9:12]
        bad_w = 0
        if alpha is not None:
            rec["alpha_sum"], rec["alpha_zero"], n = weight_chain(np.asarray(alpha, np.float64)[y])
            bad_w += n
        if beta is not None:
            bt = np.asarray(beta, np.float64)[y]
            rec["beta_sum"][:bt.shape[1]], rec["beta_zero"][:bt.shape[1]], n = weight_chain(bt)
            bad_w += n
        if wrc is not None:
            s1, _, n = weight_chain(np.asarray(wrc, np.float64)[y][:, None])
            rec["wrc_sum"] = s1[0]
            bad_w += n
        n_y = np.asarray(nbhd)[y].astype(np.int64)
        cls = np.searchsorted(np.array(CAPS), n_y, side="left")                              # first c with N <= CAPS[c]; 8: above
        rec.update(sum_nbhd=np.int64(n_y.sum()), own_only_pixels=np.int64((n_y == S).sum()),
                   class_pixels=np.bincount(cls, minlength=9).astype(np.int64), unchanged_samples=np.int64(unchanged[i].sum()),
                   nonfinite_samples=np.int64(nonfinite[i].sum()), nonfinite_pixels=np.int64((nonfinite[i] > 0).sum()),
                   weights_nonfinite=np.int64(bad_w), min_nbhd=np.int64(n_y.min()), max_nbhd=np.int64(n_y.max()))
        out.append(rec)
    return out


def fold(recs):
    """the rows folded in their order: doubles as a chain, counts summed, min_nbhd / max_nbhd the minimum / maximum"""
    t = {k: np.array(recs[0][k]) for k in FIELDS}
    for r in recs[1:]:
        with np.errstate(invalid="ignore", over="ignore"):
            for k in DOUBLES:
                t[k] = t[k] + r[k]
        for k in COUNTS:
            t[k] = t[k] + r[k]
        t["min_nbhd"], t["max_nbhd"] = np.minimum(t["min_nbhd"], r["min_nbhd"]), np.maximum(t["max_nbhd"], r["max_nbhd"])
    return t


def of_ctypes(row):
    """a hip.ReportRow as a record"""
    rec = {}
    for k in FIELDS:
        v = getattr(row, k)
        rec[k] = np.array(v if np.isscalar(v) else list(v), np.float64 if k in DOUBLES else np.int64)
    return rec


def to_ctypes(hipmod, rec):
    row = hipmod.ReportRow()
    for k in FIELDS:
        v = np.asarray(rec[k])
        if v.ndim == 0:
            setattr(row, k, v.item())
        else:
            dst = getattr(row, k)
            for i, x in enumerate(v.tolist()):
                dst[i] = x
    return row


def differing(x, y):
    """the fields in which two records differ: doubles by their 64 bits, counts by value"""
    bad = []
    for k in FIELDS:
        dt = np.float64 if k in DOUBLES else np.int64
        u, v = np.asarray(x[k], dt), np.asarray(y[k], dt)
        if u.shape != v.shape or u.tobytes() != v.tobytes():
            bad.append(k)
    return bad


def moved_rel_l2(rec):
    """relative L2 the pass moved the samples by: sqrt(sum_k moved2 / sum_k in2)"""
    return float(np.sqrt(np.sum(rec["moved2"]) / np.sum(rec["in2"])))
