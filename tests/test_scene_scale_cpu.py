"""The scene-scale frames of tests/scene_scale.py on the CPU, no GPU: the frames of tests/test_scene_scale_gpu.py are named
here and imported by the GPU file, and what that file takes for granted is asserted here on the oracle alone.  These are
conditions on the frames, not measurements of a kernel: a frame that misses one gets another seed, scale or shape.

  degeneracy   under REF_ABORT one frame has NaN neighbourhood SDs in >= 1 % of its (pixel, column) entries and an N that spans
               several class_capacity classes; one has every pixel at N = S through exactly-zero stage-1a SDs with no planted
               flat pixel; one has a NaN stage-1a SD (72 spp: S no power of two and large enough that the sum of squares
               rounds).  Under EPS the same frames have only finite colours.
  controls     far at 1e-2 and neg_big: no NaN, no zero SD, the N of the untransformed frame to within a few samples.
  sensitivity  numpy restatements of stage 1a and of the neighbourhood mean / SD on the oracle's member lists reproduce the
               oracle's bits; with the sums taken pairwise (np.sum), or with the last expression contracted into one fused
               multiply-add (round(q/n) - m*m evaluated exactly in fractions.Fraction and rounded once, what a compiler's
               contraction of ops.h:141 gives), a discrete outcome -- an SD that is NaN or zero, a 3 sigma verdict, a bin id --
               changes in at least one pixel of EVERY degenerate frame and in NO pixel of the untransformed frame of the same
               seed.  That pair of facts is what the scene-scale frames see and the O(1) frames cannot.
  stage 4      the frames of the per-sample stage-4 check move the checked colours by >= 5 % in the oracle; the largest z^2
               over their members (Z2MAX) is measured here from the oracle's mean and SD and handed to the expanded-form bar of
               tests/stage4_bars.py, which needs a bound on z^2 where its derivation otherwise uses z^2 < N.

Measured here.  Degeneracy: clu2e4 under REF_ABORT has 5.4 % NaN neighbourhood SDs, 65 of 108 pixels non-finite, N = 72 ... 392
(three size classes), and 6.4 % exactly-zero SDs under EPS; smo1e3 has 8.6 % exactly-zero stage-1a SDs, every pixel at N = S and
108 of 108 non-finite under REF_ABORT, and EPS moves its colours by 7.1 %; s72 has 18 NaN stage-1a SDs of 960; the controls have
a mean N of 204.8 (far at 1e-2) and 206.5 (neg_big) against 206.1.  Largest z^2: 7 (= N - 1) on smo1e3, 67.8 on clu2e4 (N up to
392).  Sensitivity, pixels of the frame in which a discrete outcome changes, of 108 | 108 | 80 | 108 (every one of them a
stage-2 SD pattern or bin id, in s72 also 9 | 6 stage-1a SD patterns; no 3 sigma verdict changes on these frames):

  fault        clu2e4   smo1e3   s72     farn    plain clustered / smooth
  pairwise     80       0 (*)    19      58      0
  contracted   42       1        36      62      0

(*) not a miss of the frame: at N = S = 8 every sum over an offset column is exact, so no order of summation changes a bit
(ORDER_FREE below proves it by comparing the statistics themselves); the all-N = S frame on which the order shows is s72.
"""
import fractions

import numpy as np
import pytest

import fast_weights_ref as R
import planted_nbhd as P
import scene_scale as SS
import stage4_bars as B

EPS, REF_ABORT = 1, 0
L19, G37, H27 = (2, 12, "f32"), (3, 7, "f32"), (4, 18, "f16")
ACTIVE = P.ACTIVE_SIGMA_SEED
MIN_ACTIVITY = 0.05

# name: profile, scale (far only), generator mode, W, H, S, box, layout
FRAMES = {
    # -- 12 x 9 x 8, box 7: the fused K = 7 kernel, the packed kernels, the count-first route
    "clu2e4": ("far", 2e-4, "clustered", 12, 9, 8, 7, L19),       # NaN neighbourhood SDs (REF_ABORT), zero SDs (EPS)
    "smo1e3": ("far", 1e-3, "smooth", 12, 9, 8, 7, L19),          # every pixel N = S: stage-1a SDs exactly 0 by quantisation
    "ctl1e2": ("far", 1e-2, "smooth", 12, 9, 8, 7, L19),          # control
    "negbig": ("neg_big", None, "smooth", 12, 9, 8, 7, L19),      # control
    "mix2e3": ("far", 2e-3, "smooth", 12, 9, 8, 7, L19),          # between the two: most pixels flat, the rest N up to 303
    "farn": ("far_n", None, "clustered", 12, 9, 8, 7, L19),
    "hdr": ("hdr", None, "clustered", 12, 9, 8, 7, L19),
    "plain_c": (None, None, "clustered", 12, 9, 8, 7, L19),       # the untransformed frames of the same seed
    "plain_s": (None, None, "smooth", 12, 9, 8, 7, L19),
    # -- the other kernel classes
    "k13": ("far", 2e-4, "clustered", 12, 9, 16, 7, L19),         # one-wave K = 13
    "b13s3": ("far", 2e-4, "clustered", 14, 6, 3, 13, L19),       # box 13 x 3 spp: the unbinned hand-over
    "s32": ("far", 2e-4, "clustered", 12, 9, 32, 7, L19),         # size-binned classes, four-wave, split, K = 25
    "s64": ("far", 2e-4, "clustered", 10, 8, 64, 7, L19),         # K = 49
    "stream": ("far", 2e-4, "clustered", 22, 19, 16, 17, L19),    # N > 3136: the streaming kernel
    "half8": ("half", None, "clustered", 12, 9, 8, 7, H27),       # d27 fp16
    "half16": ("half", None, "clustered", 12, 9, 16, 7, H27),
    "g37": ("far", 2e-4, "clustered", 12, 9, 8, 7, G37),          # the generic layouts (routes 3, 4, 5)
    "g37k13": ("far", 2e-4, "clustered", 12, 9, 16, 7, G37),      # ... with one-wave classes for route 5
    "gh27": ("half", None, "clustered", 12, 9, 8, 7, H27),
    "s12": ("far", 2e-4, "clustered", 10, 8, 12, 5, L19),         # S no power of two
    "s72": ("far", 2e-4, "smooth", 10, 8, 72, 5, L19),            # ... and the S that gives a NaN stage-1a SD
}
DEGENERATE = ["clu2e4", "smo1e3", "s72", "farn"]
# (fault, frame) pairs on which the fault provably changes nothing.  smo1e3 has N = S = 8 in every pixel, and a column of fp32
# values k * ulp of one binade (k < 2^24) has squares k^2 * ulp^2 < 2^48 ulp^2: a sum of eight fits 51 bits, so every sum of x
# and of x^2 over an offset column (pFilm, the positions) of the frame is exact in fp64, in any order.  A sum of squares can
# round only beyond 32 terms, which is why the stage-1a NaN needs 72 spp; s72 is the frame with N = S everywhere on which the
# pairwise fault is required.
ORDER_FREE = {("pairwise", "smo1e3")}
UNTRANSFORMED = {"clustered": "plain_c", "smooth": "plain_s"}
# frame, sigma seed of the per-sample stage-4 check (EPS): smo1e3 is active at the reference's seed, clu2e4 at the suite's
STAGE4 = [("smo1e3", 0.002), ("clu2e4", ACTIVE)]


def geometry(name):
    return FRAMES[name][3:7]


def layout(name):
    return FRAMES[name][7]


def planes(name):
    """(stored planes, their fp32 image) of a named frame"""
    prof, scale, mode, W, H, S, _, lay = FRAMES[name]
    return SS.frame(prof, W, H, S, scale=scale, mode=mode, lay=lay) if prof is not None else \
        SS.frame(None, W, H, S, mode=mode, lay=lay)


_want = {}


def want_of(oracle, name, policy, seed=0.002, box=None):
    """the oracle's pass of a named frame: computed once per session, shared, never modified"""
    key = (name, policy, seed, box)
    if key not in _want:
        W, H, S, fbox = geometry(name)
        _want[key] = oracle.filter_pass(planes(name)[1], oracle.make_desc(W, H, S, box=box or fbox, policy=policy, sigma_seed=seed,
                                                                          **SS.oracle_kw(layout(name))))
    return _want[key]


def all_pixels(name):
    W, H, _, _ = geometry(name)
    return [(y, x) for y in range(H) for x in range(W)]


def class_of(n):
    return int(np.searchsorted(P.CAPACITIES, n))


# ---- the frames themselves ----------------------------------------------------------------------------------------------------
def test_profiles_round_once_and_keep_what_they_promise():
    """one rounding of the fp64 image; the fp16 frames keep distinct pixel positions and a few distinct values per neighbourhood"""
    src = SS.source(12, 9, 8)
    stored, p32 = SS.frame("far", 12, 9, 8, scale=1e-3)
    want = (SS.OFF[0] + 1e-3 * src[10].astype(np.float64)).astype(np.float32)
    assert stored.dtype == np.float32 and np.array_equal(stored[10], want) and np.array_equal(p32, stored)
    assert np.array_equal(stored[0], (src[0].astype(np.float64) + SS.PFILM[0]).astype(np.float32))
    assert np.array_equal(stored[2:10], src[2:10])                      # colours, random parameters, normals: untouched
    h16, h32 = planes("half8")
    assert h16.dtype == np.float16 and h32.dtype == np.float32 and np.array_equal(h32, h16.astype(np.float32))
    fx = h32[0].reshape(9, 12, 8)
    centre = (np.arange(12) + SS.HALF_PFILM[0] + 0.5)[None, :, None]
    assert (np.abs(fx - centre) <= 0.5).all() and fx.max() < 64             # inside its own pixel, on fp16's 1/32 grid
    assert len(np.unique(fx[0, 0])) >= 6                                    # ... which still tells a pixel's samples apart
    for c, _ in SS.position_columns(4, 18):
        distinct = [len(np.unique(h32[c, y:y + 7, x:x + 7])) for y in (0, 2) for x in (0, 5)]
        assert 2 <= min(distinct) and max(distinct) <= 8, (c, distinct)       # a few distinct values: ties are the rule
    assert SS.position_columns(3, 7) == [(11, 0), (12, 1), (13, 2)]
    hdr = planes("hdr")[1]
    black = (hdr[2:5] == 0).all(axis=0)
    assert 0.15 < black.mean() < 0.35 and hdr[2:5].max() > 500 and ((hdr[2:5] == 0).any(axis=0) == black).all()


# ---- degeneracy reached ---------------------------------------------------------------------------------------------------------
def test_nan_neighbourhood_sds_across_size_classes(oracle):
    w = want_of(oracle, "clu2e4", REF_ABORT)
    share = float(np.isnan(w["stddev"]).mean())
    classes = {class_of(n) for n in w["nbhd_size"].ravel()}
    print("clu2e4 REF_ABORT: NaN SD share %.4f, N %d ... %d, classes %s, non-finite pixels %d" % (
        share, w["nbhd_size"].min(), w["nbhd_size"].max(), sorted(classes), w["nonfinite_pixels"]))
    assert share >= 0.01 and len(classes) >= 2
    assert w["status"] == 1 and 0 < w["nonfinite_pixels"] < 12 * 9          # a NaN pattern, not a NaN frame
    e = want_of(oracle, "clu2e4", EPS)
    assert np.isfinite(e["colour"]).all() and float((e["stddev"] == 0).mean()) >= 0.01


def test_every_pixel_flat_by_quantisation(oracle):
    """no planted flat pixel (flat_frac = 0): the scale alone rounds all S samples of a feature to one fp32 value in enough
    pixels that the 3 sigma test (|f - m| >= 0) rejects every candidate everywhere"""
    W, H, S, _ = geometry("smo1e3")
    p32 = planes("smo1e3")[1]
    _, sd = oracle.pixel_stats(p32, oracle.make_desc(W, H, S))
    w = want_of(oracle, "smo1e3", REF_ABORT)
    print("smo1e3: stage-1a SDs exactly 0: %.4f; non-finite pixels under REF_ABORT %d" % ((sd == 0).mean(), w["nonfinite_pixels"]))
    assert (w["nbhd_size"] == S).all() and (sd == 0).any(axis=-1).all() and not np.isnan(sd).any()
    assert w["nonfinite_pixels"] == W * H
    assert np.isfinite(want_of(oracle, "smo1e3", EPS)["colour"]).all()


def test_mixed_frame_reaches_packed_and_one_wave_kernels(oracle):
    """mix2e3: flat pixels (N = S, the packed kernels) next to neighbourhoods of hundreds of samples, NaN pixels among them"""
    w = want_of(oracle, "mix2e3", REF_ABORT)
    n = w["nbhd_size"]
    assert 0.5 < (n == 8).mean() < 0.95 and (n > 64).sum() >= 5
    assert 0 < w["nonfinite_pixels"] < n.size


def test_nan_stage1a_sd(oracle):
    W, H, S, _ = geometry("s72")
    p32 = planes("s72")[1]
    _, sd = oracle.pixel_stats(p32, oracle.make_desc(W, H, S))
    _, sd_eps = oracle.pixel_stats(p32, oracle.make_desc(W, H, S, policy=EPS))
    print("s72: NaN stage-1a SDs %d of %d" % (np.isnan(sd).sum(), sd.size))
    assert np.isnan(sd).any() and S & (S - 1) != 0
    assert np.array_equal(sd_eps, np.where(np.isnan(sd), 0.0, sd))          # EPS: a NaN sigma is a zero sigma
    assert np.isfinite(want_of(oracle, "s72", EPS)["colour"]).all()


@pytest.mark.parametrize("name", [n for n in FRAMES if n not in ("ctl1e2", "negbig", "plain_c", "plain_s")])
def test_eps_completes_every_frame(oracle, name):
    """whatever REF_ABORT makes of a frame, EPS leaves only finite colours"""
    w = want_of(oracle, name, EPS)
    assert w["status"] == 0 and np.isfinite(w["colour"]).all()


@pytest.mark.parametrize("name", ["ctl1e2", "negbig"])
def test_controls_are_not_degenerate(oracle, name):
    base = want_of(oracle, "plain_s", REF_ABORT)["nbhd_size"]
    W, H, S, _ = geometry(name)
    _, sd = oracle.pixel_stats(planes(name)[1], oracle.make_desc(W, H, S))
    for policy in (REF_ABORT, EPS):
        w = want_of(oracle, name, policy)
        assert w["status"] == 0 and np.isfinite(w["colour"]).all()
        assert not np.isnan(w["stddev"]).any() and (w["stddev"] != 0).all()
    assert not np.isnan(sd).any() and (sd != 0).all()
    n = w["nbhd_size"]
    print("%s: mean N %.1f against %.1f, largest |dN| %d" % (name, n.mean(), base.mean(), np.abs(n - base).max()))
    assert abs(n.mean() - base.mean()) <= 3 and abs(np.median(n) - np.median(base)) <= 3


def test_streaming_frame_is_degenerate_and_streams(oracle):
    w = want_of(oracle, "stream", REF_ABORT)
    assert w["nbhd_size"].max() > B.RESIDENT and np.isnan(w["stddev"]).any()


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------
def _serial(rows):
    n = rows.shape[0]
    m = np.add.accumulate(rows, axis=0)[-1] / n
    q = np.add.accumulate(rows * rows, axis=0)[-1]
    return m, q / n


def stats_serial(rows):
    """ops.h:111-144 / rpf_oracle_mean_std: both chains serial, sqrt(q / n - m * m) with every operation rounded"""
    m, qn = _serial(rows)
    with np.errstate(invalid="ignore"):
        return m, np.sqrt(qn - m * m)


def stats_pairwise(rows):
    """planted fault: the two sums taken pairwise (np.sum over a contiguous axis)"""
    cols = np.ascontiguousarray(rows.T)
    n = rows.shape[0]
    m = cols.sum(axis=1) / n
    with np.errstate(invalid="ignore"):
        return m, np.sqrt((cols * cols).sum(axis=1) / n - m * m)


def stats_contracted(rows):
    """planted fault: q / n - m * m as one fused multiply-add, fma(-m, m, q / n): the product exact, one rounding"""
    m, qn = _serial(rows)
    var = np.array([float(fractions.Fraction(float(a)) - fractions.Fraction(float(b)) ** 2) for a, b in zip(qn, m)])
    with np.errstate(invalid="ignore"):
        return m, np.sqrt(var)


def bin_ids(nb, M, SD):
    """stage 3a (mi.cpp:14-16 on the normalised columns): [N, ndim] ids, B = floor(sqrt(N))"""
    n = nb.shape[0]
    bins = max(int(np.sqrt(n)), 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where(SD == 0, 0.0, (nb - M) / SD)
    ids = np.zeros(z.shape, np.int64)
    for c in range(z.shape[1]):
        if np.isnan(z[:, c]).any():
            continue
        lo, hi = z[:, c].min(), z[:, c].max()
        if hi != lo:
            ids[:, c] = np.clip(((z[:, c] - lo) / (hi - lo) * bins).astype(np.int64), 0, bins - 1)
    return ids


def outcomes(oracle, name, stats):
    """the discrete outcomes of a frame under a statistics function, per pixel: (the NaN pattern and the zero pattern of the
    stage-1a SDs, the 3 sigma verdicts of the window, the NaN / zero pattern of the neighbourhood SDs and every bin id on the
    ORACLE's member list) as bytes, plus the stage-1a and stage-2 (mean, SD) for the self-check of the serial form"""
    W, H, S, box = geometry(name)
    p32 = planes(name)[1]
    nr, nf, _ = layout(name)
    f0 = 5 + nr
    om, osd = oracle.pixel_stats(p32, oracle.make_desc(W, H, S, **SS.oracle_kw(layout(name))))
    pm, psd = np.empty_like(om), np.empty_like(osd)
    for y, x in all_pixels(name):
        pm[y, x], psd[y, x] = stats(p32[f0:, y, x, :].T.astype(np.float64))
    out, M2, SD2 = [], [], []
    for y, x in all_pixels(name):
        mine = R.neighbourhood(p32, pm, psd, y, x, box, nr, nf)            # the verdicts under `stats`
        nb = R.neighbourhood(p32, om, osd, y, x, box, nr, nf)              # the oracle's member list
        M, SD = stats(nb)
        M2.append(M)
        SD2.append(SD)
        out.append((np.isnan(psd[y, x]).tobytes() + (psd[y, x] == 0).tobytes(), mine.tobytes(),
                    np.isnan(SD).tobytes() + (SD == 0).tobytes() + bin_ids(nb, M, SD).tobytes()))
    return out, (pm, psd, np.array(M2).reshape(H, W, -1), np.array(SD2).reshape(H, W, -1))


_outcomes = {}


def outcomes_of(oracle, name, fault):
    if (name, fault) not in _outcomes:
        _outcomes[name, fault] = outcomes(oracle, name, {"serial": stats_serial, "pairwise": stats_pairwise,
                                                         "contracted": stats_contracted}[fault])
    return _outcomes[name, fault]


@pytest.mark.parametrize("name", DEGENERATE + ["plain_c", "plain_s"])
def test_serial_restatement_is_the_oracle(oracle, name):
    """the restatement the faults are planted in reproduces the oracle's stage-1a and stage-2 statistics bit for bit"""
    W, H, S, _ = geometry(name)
    _, (pm, psd, M, SD) = outcomes_of(oracle, name, "serial")
    om, osd = oracle.pixel_stats(planes(name)[1], oracle.make_desc(W, H, S))
    w = want_of(oracle, name, REF_ABORT)
    assert np.array_equal(pm, om) and np.array_equal(psd, osd, equal_nan=True)
    assert np.array_equal(M, w["mean"]) and np.array_equal(SD, w["stddev"], equal_nan=True)


@pytest.mark.parametrize("fault", ["pairwise", "contracted"])
def test_planted_faults_show_on_degenerate_frames_only(oracle, fault):
    for name in DEGENERATE:
        base, ref = outcomes_of(oracle, name, "serial")
        bad, alt = outcomes_of(oracle, name, fault)
        if (fault, name) in ORDER_FREE:
            # every sum over an offset column is exact, so no order of summation can change a bit of it: the statistics of
            # those columns are the serial ones (the all-N = S frame on which the order of the sums does show is s72)
            f = [c - 7 for c, _ in SS.position_columns(2, 12)]
            cols = [f, f, [0, 1] + [c + 7 for c in f], [0, 1] + [c + 7 for c in f]]
            assert all(np.array_equal(a[..., c], b[..., c], equal_nan=True) for a, b, c in zip(ref, alt, cols)) and base == bad
            continue
        changed = [sum(a[k] != b[k] for a, b in zip(base, bad)) for k in range(3)]
        either = sum(a != b for a, b in zip(base, bad))
        print("%s on %s: pixels with a changed outcome %d of %d (stage-1a SD pattern %d, 3 sigma verdicts %d, stage-2 SD pattern "
              "or bin ids %d)" % (fault, name, either, len(base), changed[0], changed[1], changed[2]))
        assert either >= 1, (fault, name)
    for name in {UNTRANSFORMED[FRAMES[n][2]] for n in DEGENERATE}:
        base, _ = outcomes_of(oracle, name, "serial")
        bad, _ = outcomes_of(oracle, name, fault)
        assert base == bad, (fault, name)


# ---- stage 4: activity, and the z^2 the expanded bar needs ----------------------------------------------------------------------
def z2max_of(oracle, name, stages, policy=EPS):
    """the largest z^2 over the weighted columns of every member of every pixel, from the mean and SD of `stages`"""
    W, H, S, box = geometry(name)
    nr, nf, _ = layout(name)
    p32 = planes(name)[1]
    pm, psd = oracle.pixel_stats(p32, oracle.make_desc(W, H, S, policy=policy, **SS.oracle_kw(layout(name))))
    cols = R.weighted_columns(nr, nf)
    worst = 0.0
    for y, x in all_pixels(name):
        nb = R.neighbourhood(p32, pm, psd, y, x, box, nr, nf)
        M, SD = stages["mean"][y, x], stages["stddev"][y, x]
        with np.errstate(invalid="ignore", divide="ignore"):
            z = np.where(SD == 0, 0.0, (nb - M) / SD)[:, cols]
        worst = max(worst, float(np.nanmax(z * z)))
    return worst


# measured by test_stage4_frames_are_active_and_z2max (which asserts them): the z^2 bound handed to the expanded-form bar
Z2MAX = {"smo1e3": 7.0, "clu2e4": 68.0}


@pytest.mark.parametrize("name,seed", STAGE4)
def test_stage4_frames_are_active_and_z2max(oracle, name, seed):
    w = want_of(oracle, name, EPS, seed)
    cin = planes(name)[1][2:5].astype(np.float64)
    activity = R.rel_l2(w["colour"], cin)
    z2 = z2max_of(oracle, name, w)
    n = int(w["nbhd_size"].max())
    print("%s seed %g: activity %.3f, largest z^2 %.6g (largest N %d), expanded bar %.3e, with z^2 < N %.3e" % (
        name, seed, activity, z2, n, B.sample_bar("expanded", 12, n, seed, 7, z2max=Z2MAX[name]), B.sample_bar("expanded", 12, n, seed, 7)))
    assert np.isfinite(w["colour"]).all() and activity >= MIN_ACTIVITY
    assert z2 <= Z2MAX[name] <= 1.01 * z2 + 1, (z2, Z2MAX[name])       # the recorded bound is the measured one, rounded up
    # the restatement, in both forms, sits far inside its bar on the oracle's own stage outputs
    pixels = all_pixels(name)
    ref = w["colour"].reshape(3, -1, geometry(name)[2])
    for form in ("direct", "expanded"):
        got = R.stage4(oracle, planes(name)[1], w, 7, seed, pixels, np.float64, EPS, form=form)
        bar = B.sample_bar(form, 12, n, seed, 7, z2max=Z2MAX[name])
        assert B.worst_sample(got, ref) / B.cmax_of(cin) <= bar / 100, form


def test_z2max_defaults_to_n():
    """the new argument leaves every existing bar where it was"""
    for n in (8, 392, 3136):
        for seed in (0.5, 0.05):
            assert B.sample_bar("expanded", 12, n, seed, 7) == B.sample_bar("expanded", 12, n, seed, 7, z2max=n)
            assert B.sample_bar("direct", 12, n, seed, 7) == B.sample_bar("direct", 12, n, seed, 7, z2max=5.0)
    assert B.sample_bar("expanded", 12, 392, 0.5, 7, z2max=10 * 392) > B.sample_bar("expanded", 12, 392, 0.5, 7)
