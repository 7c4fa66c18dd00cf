#!/usr/bin/env python3
"""Generates the committed golden fixtures under tests/golden/.  Run in the build container (needs
/root/reference to build oracle/_ref/libref_mi.so):   python tests/golden/make_golden.py

  ref_mi.npz     known answers of the REAL reference code: MutualInformation / computeHistogram /
                 computeJointHistogram (mi.cpp) on vectors of length 1..392 incl. constant vectors, ties on bin
                 edges, value == max, heavy duplicates.
  ref_ops.npz    known answers of the REAL ops.h templates: getMean/getStdDev (12 and 19 columns, incl.
                 large-mean/small-variance rows), the 3-sigma test as rpf.cpp:577-580 composes it,
                 SampleData::normalized as sd.h:229-232 composes it.
  e2e_*.npz      small feature buffers (inputs stored verbatim) with the outputs of oracle/rpf_oracle.c:
                 filtered colours, N, member/bin hashes, alpha, beta, W_r_c, MI.  These files pin GPU <-> oracle
                 stage by stage and guard the oracle against regressions; the oracle itself is pinned to the
                 reference by the two files above (its leaves) and by ref_filter.npz (the whole pass).
  ref_filter.npz the REAL RPFIntegrator::ApplyRPFFilter (oracle/ref_filter_harness.cpp: rpf.cpp compiled with the
                 glog / OpenEXR stand-ins of oracle/ref_stub/) on small feature buffers: its output colours for one
                 box and for box lists, or the fact that it stopped on a NaN colour
                 (python tests/golden/make_golden.py reffilter).
  ref_film.npz   the REAL pbrt Film (oracle/ref_film_harness.cpp): tile sums, weight sums and written image of
                 eleven film cases over the five pixel filters, and forty Film::filterTable arrays
                 (python tests/golden/make_golden.py reffilm).

  clustered_10x8x8.rpfb (+ _expected.npz)   an on-disk feature buffer in the .rpfb wire format and the oracle's
                 two-pass result on it.
  ref_checks.npz known answers of the REAL reference code on the inputs of test_oracle.py's randomised and
                 stage-3 / stage-4a checks (python tests/golden/make_golden.py refchecks).
  ref_nonfinite.npz  known answers of the REAL ops.h templates on infinite values: getMean / getStdDev of columns
                 holding +inf, -inf and both, and the 3-sigma test with infinite features and means
                 (python tests/golden/make_golden.py nonfinite).

Fixtures are data only: inputs and expected outputs.
"""
import io
import os
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import rpf_pkg  # noqa: E402

rpf_pkg.load()
import pyoracle as O  # noqa: E402
from raytracer_rpf_amd import feature_buffer as fb  # noqa: E402


def mi_cases(rng):
    cases = []
    for n in (1, 2, 3, 4, 8, 9, 15, 16, 17, 50, 100, 289, 392):
        x = rng.normal(size=n)
        cases += [(x, rng.normal(size=n)), (x, 0.7 * x + 0.3 * rng.normal(size=n)), (x, np.full(n, 1.25)),
                  (np.full(n, -3.0), np.full(n, 2.0)), (np.round(x * 2) / 2, np.round(rng.normal(size=n))),
                  (np.linspace(0.0, 1.0, n), np.linspace(1.0, 0.0, n) ** 2),                  # exact bin edges, value == max
                  (rng.integers(0, 3, n).astype(float), rng.integers(0, 2, n).astype(float)),  # {0,1,2} x {0,1}: ties
                  (np.float32(rng.random(n)).astype(float), np.float32(rng.random(n) * 1000).astype(float))]
    return cases


def rpfb_fixture():
    """clustered_10x8x8.rpfb: an on-disk feature buffer (feature_buffer.save_rpfb, with a ray-weight plane) and the
    oracle's two-pass {7, 5} result on it (filtered colours + pixel means): closes the loop file -> HIP path."""
    W, H, S = 10, 8, 8
    planes = fb.synth_planes(W, H, S, seed=77, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    rw = (0.5 + np.random.default_rng(77).random((H, W, S))).astype(np.float32)
    fb.save_rpfb(os.path.join(HERE, "clustered_10x8x8.rpfb"), planes, rw)
    c = None
    for box in (7, 5):
        c = O.filter_pass(planes, O.make_desc(W, H, S, box=box, policy=O.DEGEN_EPS, n_threads=1), colour_in=c,
                          debug=False)["colour"]
    pix = O.pixel_mean(c, O.make_desc(W, H, S), rw)
    np.savez_compressed(os.path.join(HERE, "clustered_10x8x8_expected.npz"), colour=c, pixel_rgb=pix,
                        boxes=np.array([7, 5], np.int32), policy=O.DEGEN_EPS,
                        source="oracle/rpf_oracle.c, EPS policy, beta map REF_GCC11_O3, on clustered_10x8x8.rpfb")
    cin = planes[2:5].astype(np.float64)
    print("clustered_10x8x8.rpfb  %.1f KB, activity %.3e" % (
        os.path.getsize(os.path.join(HERE, "clustered_10x8x8.rpfb")) / 1024, np.linalg.norm(c - cin) / np.linalg.norm(cin)))


def ref_checks_fixture():
    """ref_checks.npz: the compiled reference's answers on the inputs of tests/test_oracle.py's randomised MI / mean-std
    check, its stage-3 pixels (neighbourhood size, mean, stddev, 96 MI values from the reference's own 3-sigma test,
    getMean / getStdDev, normalisation and MutualInformation) and its stage-4a weighted distances.  Inputs stored verbatim,
    so those tests run without the compiled reference."""
    out = {}
    # ---- randomised MI and mean / stddev ------------------------------------------------------------
    rng = np.random.default_rng(5)
    xs, ys, lens, mis = [], [], [], []
    for n in (1, 2, 5, 8, 49, 64, 200, 392, 784):
        for t in range(12):
            x = rng.normal(size=n)
            y = rng.normal(size=n) + (t % 3) * 0.5 * x
            if t % 4 == 0:
                x = np.round(x * 3) / 3
            if t % 6 == 0:
                y = np.full(n, 0.25)
            xs.append(x); ys.append(y); lens.append(n); mis.append(O.ref_mi(x, y))
    out.update(mi_x=np.concatenate(xs), mi_y=np.concatenate(ys), mi_n=np.array(lens, np.int32), mi=np.array(mis))
    for nc in (12, 19):
        r = np.float32(rng.normal(size=(300, nc)) * 0.02 + 500).astype(float)
        out["ms%d_rows" % nc] = r
        out["ms%d_mean" % nc], out["ms%d_std" % nc] = O.ref_mean_std(r)

    # ---- stage 3 of three pixels --------------------------------------------------------------------
    W, H, S, box = 9, 8, 8, 7
    planes = fb.synth_planes(W, H, S, seed=13, sigma_f=1e-3, sigma_c=0.01, mode="clustered")
    pa, pb = O.pair_table()
    b = (box - 1) // 2
    mean12, sd12 = O.pixel_stats(planes, O.make_desc(W, H, S))
    pixels = ((4, 4), (0, 0), (7, 3))
    cnt, ms, ss, mi3 = [], [], [], []
    for (y, x) in pixels:
        rows = [planes[:, y, x, s].astype(float) for s in range(S)]
        for xn in range(x - b, x + b + 1):
            for yn in range(y - b, y + b + 1):
                if (xn, yn) == (x, y) or not (0 <= xn < W and 0 <= yn < H):
                    continue
                for s in range(S):
                    v = planes[:, yn, xn, s].astype(float)
                    if O.ref_within_3std(v[7:], mean12[y, x], sd12[y, x]):
                        rows.append(v)
        rows = np.array(rows)
        m, s = O.ref_mean_std(rows)
        z = np.stack([O.ref_normalize(v, m, s) for v in rows])
        cnt.append(len(rows)); ms.append(m); ss.append(s)
        mi3.append([O.ref_mi(z[:, a], z[:, bb]) for a, bb in zip(pa, pb)])
    out.update(s3_planes=planes, s3_pixels=np.array(pixels, np.int32), s3_nbhd=np.array(cnt, np.int32),
               s3_mean=np.array(ms), s3_std=np.array(ss), s3_mi=np.array(mi3))

    # ---- stage 4a weighted squared distances --------------------------------------------------------
    planes = planes.copy()
    planes[10:13] += 700.0
    r = O.filter_pass(planes, O.make_desc(W, H, S, box=box, n_threads=1))
    rng = np.random.default_rng(9)
    own, oth, al, be, d = [], [], [], [], []
    for (y, x) in ((4, 4), (0, 0), (7, 3), (2, 8)):
        m, s = r["mean"][y, x], r["stddev"][y, x]
        zo = np.stack([O.ref_normalize(planes[:, y, x, i].astype(float), m, s) for i in range(S)])
        zn = np.stack([O.ref_normalize(planes[:, (y + dy) % H, (x + dx) % W, i].astype(float), m, s)
                       for dy, dx, i in rng.integers(0, 4, size=(24, 3))])
        a, bt = r["alpha"][y, x], r["beta"][y, x]
        own.append(zo); oth.append(zn); al.append(a); be.append(bt)
        d.append([[O.ref_weighted_sqdist(zi, zj, a, bt) for zj in np.concatenate([zo, zn])] for zi in zo])
    out.update(s4_own=np.array(own), s4_other=np.array(oth), s4_alpha=np.array(al), s4_beta=np.array(be), s4_d=np.array(d))
    z = rng.normal(size=(2, 19))
    nf_a, nf_b, nf_d = [], [], []
    for a in (np.array([np.nan, 1.0, 2.0]), np.array([np.inf, 0.0, -1.0])):
        bt = np.concatenate([a, rng.normal(size=9)])
        nf_a.append(a); nf_b.append(bt); nf_d.append(O.ref_weighted_sqdist(z[0], z[1], a, bt))
    out.update(s4nf_z=z, s4nf_alpha=np.array(nf_a), s4nf_beta=np.array(nf_b), s4nf_d=np.array(nf_d))
    np.savez_compressed(os.path.join(HERE, "ref_checks.npz"), **out,
                        source="MutualInformation() of mi.cpp and the ops.h templates of the reference, "
                               "g++ 11.4 -O3 -std=gnu++11; inputs stored verbatim")
    print("ref_checks.npz  %.1f KB" % (os.path.getsize(os.path.join(HERE, "ref_checks.npz")) / 1024))


def ref_nonfinite_fixture():
    """ref_nonfinite.npz: the compiled reference's getMean / getStdDev and 3-sigma test where a value is infinite (a miss
    ray's depth or position; an fp16 feature above 65504).  Inputs stored verbatim."""
    out = {}
    rng = np.random.default_rng(31)
    inf = np.inf
    for nc, n in ((12, 8), (19, 24)):
        r = np.float32(rng.normal(size=(n, nc)) * 0.1 + 0.5).astype(float)
        r[3, 0] = inf                          # one +inf sample
        r[5, 1] = -inf                         # one -inf sample
        r[2, 2], r[6, 2] = inf, -inf           # both: the mean is NaN
        r[:, 3] = inf                          # every sample +inf
        r[:, 4] = -inf                         # every sample -inf
        r[1, 5], r[4, 5] = inf, inf            # two +inf samples
        r[0, 6] = np.nan                       # a NaN next to them
        out["ms%d_rows" % nc] = r
        out["ms%d_mean" % nc], out["ms%d_std" % nc] = O.ref_mean_std(r)
    # the 3-sigma test (rpf.cpp:577-580): feature 0 of each row is the case, features 1..11 sit inside 3 sigma
    cases = [  # (f, m, sd)
        (inf, inf, 0.0),        # a candidate at +inf against a pixel whose mean is +inf (EPS: NaN sigma clamped to 0)
        (inf, inf, np.nan),     # ... REF_ABORT keeps that sigma NaN
        (-inf, -inf, 0.0),
        (-inf, inf, 0.0),
        (inf, -inf, 0.0),
        (inf, 0.5, 0.0),        # +inf against a finite mean, sigma 0
        (-inf, 0.5, 0.0),
        (inf, 0.5, 0.2),        # ... and a finite sigma
        (inf, 0.5, inf),
        (inf, 0.5, np.nan),
        (0.5, inf, 0.0),        # a finite candidate against a mean of +inf
        (0.5, inf, np.nan),
        (0.5, -inf, 0.0),
        (0.5, inf, inf),
        (inf, inf, inf),
        (np.nan, inf, 0.0),
        (inf, np.nan, 0.0),
        (0.5, 0.5, 0.0),        # the finite zero-sigma case the flat proof rests on
        (0.5, 0.5, inf),
        (1e308, -1e308, 0.0),   # |f - m| overflows to inf
    ]
    f = np.float32(rng.normal(size=(len(cases), 12)) * 0.01).astype(float)
    mean = np.zeros((len(cases), 12))
    sd = np.full((len(cases), 12), 0.6)
    for i, (fv, mv, sv) in enumerate(cases):
        f[i, 0], mean[i, 0], sd[i, 0] = fv, mv, sv
    out["w3_f"], out["w3_mean"], out["w3_sd"] = f, mean, sd
    out["w3_pass"] = np.array([O.ref_within_3std(f[i], mean[i], sd[i]) for i in range(len(cases))])
    path = os.path.join(HERE, "ref_nonfinite.npz")
    with np.errstate(invalid="ignore", over="ignore"):
        np.savez_compressed(path, **out, source="getMean / getStdDev / allLessThan of the reference's ops.h, "
                                                "g++ 11.4 -O3 -std=gnu++11; inputs stored verbatim")
    print("ref_nonfinite.npz  %.1f KB" % (os.path.getsize(path) / 1024))


def save_npz_stable(path, **arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes on every run"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def _compiler():
    return subprocess.run(["g++", "--version"], stdout=subprocess.PIPE).stdout.decode().splitlines()[0].strip()


REF_FLAGS = "-O3 -std=gnu++11 -ffp-contract=off, glog / OpenEXR stand-ins of oracle/ref_stub"

# (name, W, H, S, boxes, mode, sigma_f, sigma_c, seed, edit).  A case whose name another case gives as `planes_of` shares
# that case's planes.  edit: None | "constnormal" | ("set", plane, y, x, s, value)
REF_FILTER_CASES = [
    # single pass: boxes 5, 7, 9, 17; 8, 16, 32 spp; clustered (the filter changes the colours) and smooth (route coverage)
    ("cl_12x10x8_b7", 12, 10, 8, (7,), "clustered", 1e-3, 0.01, 7, None),
    ("cl_8x6x16_b5", 8, 6, 16, (5,), "clustered", 1e-3, 0.01, 7, None),
    ("cl_10x8x8_b5", 10, 8, 8, (5,), "clustered", 1e-3, 0.01, 11, None),
    ("sm_10x8x8_b7", 10, 8, 8, (7,), "smooth", 0.05, 1e-4, 7, None),
    ("cl_12x12x8_b17", 12, 12, 8, (17,), "clustered", 1e-3, 0.01, 3, None),
    ("sm_6x5x32_b9", 6, 5, 32, (9,), "smooth", 0.05, 1e-4, 5, None),
    ("cl_8x8x8_b9", 8, 8, 8, (9,), "clustered", 1e-3, 0.01, 9, None),
    ("sm_8x6x16_b7", 8, 6, 16, (7,), "smooth", 0.05, 1e-4, 13, None),
    # box lists: the colours of one pass are the next pass's, in double precision
    ("cl_12x10x8_b7_5", "cl_12x10x8_b7", (7, 5)),
    ("cl_10x8x8_b7_7_5", "cl_10x8x8_b5", (7, 7, 5)),
    ("cl_12x12x8_b17_7", "cl_12x12x8_b17", (17, 7)),
    # frames smaller than the window, few samples per pixel
    ("cl_3x2x8_b7", 3, 2, 8, (7,), "clustered", 1e-3, 0.01, 1, None),
    ("cl_2x5x8_b5", 2, 5, 8, (5,), "clustered", 1e-3, 0.01, 8, None),
    ("cl_4x3x4_b5", 4, 3, 4, (5,), "clustered", 1e-3, 0.01, 8, None),
    ("cl_4x4x4_b7", 4, 4, 4, (7,), "clustered", 1e-3, 0.01, 9, None),
    ("sm_3x3x4_b7", 3, 3, 4, (7,), "smooth", 0.05, 1e-4, 8, None),
    # the reference stops on these (a NaN colour): SURVEY F2
    ("abort_constnormal_8x6x8_b7", 8, 6, 8, (7,), "smooth", 0.05, 1e-4, 7, "constnormal"),
    ("abort_box3_6x5x8", 6, 5, 8, (3,), "clustered", 1e-3, 0.01, 5, None),
    ("abort_inf_6x5x8_b5", 6, 5, 8, (5,), "clustered", 1e-3, 0.01, 6, ("set", 11, 2, 3, 1, np.inf)),
    ("abort_nan_6x5x8_b7", 6, 5, 8, (7,), "smooth", 0.05, 1e-4, 6, ("set", 16, 1, 4, 5, np.nan)),
    ("abort_6x5x2_b7", 6, 5, 2, (7,), "clustered", 1e-3, 0.01, 3, None),
    ("abort_7x5x1_b7", 7, 5, 1, (7,), "clustered", 1e-3, 0.01, 4, None),
    ("abort_5x4x3_b7", 5, 4, 3, (7,), "clustered", 1e-3, 0.01, 2, None),
    ("abort_second_pass_8x6x4_b7_3", 8, 6, 4, (7, 3), "clustered", 1e-3, 0.01, 12, None),
]


def check_ref_filter_conditions(names, aborted, activity, nbhd_max):
    """what the fixture set must hold (asserted here and again by tests/test_ref_fixtures.py)"""
    done = ~aborted
    assert aborted.sum() >= 6, "at least six aborting cases"
    assert (activity[done] > 1e-3).sum() * 2 >= done.sum(), "half of the completing cases must change the colours by > 1e-3"
    assert (nbhd_max[done] > 1024).any(), "a completing case with a neighbourhood above 1024 samples"
    assert (nbhd_max[done] <= 64).any(), "a completing case whose neighbourhoods are all <= 64 samples"


def ref_filter_fixture():
    """ref_filter.npz: inputs verbatim, and what the compiled reference's ApplyRPFFilter made of them"""
    out, planes_by_name = {}, {}
    names, aborted, activity, nbhd_max = [], [], [], []
    for i, case in enumerate(REF_FILTER_CASES):
        if len(case) == 3:
            name, planes_of, boxes = case
            planes = planes_by_name[planes_of]
            out["planes_of_%d" % i] = np.int32(names.index(planes_of))
        else:
            name, W, H, S, boxes, mode, sf, sc, seed, edit = case
            planes = fb.synth_planes(W, H, S, seed=seed, sigma_f=sf, sigma_c=sc, mode=mode)
            if edit == "constnormal":
                planes[7:10] = np.float32([0.0, 0.0, 1.0])[:, None, None, None]
            elif edit is not None:
                _, c, y, x, smp, v = edit
                planes[c, y, x, smp] = v
            planes_by_name[name] = planes
            out["planes_%d" % i] = planes
        _, H, W, S = planes.shape
        colour, status = O.ref_filter(planes, boxes, n_threads=1)
        if status == 0:  # (where the reference stops it is run with one thread only: see pyoracle.ref_filter)
            assert np.array_equal(colour, O.ref_filter(planes, boxes, n_threads=4)[0]), (name, "1 and 4 threads differ")
        out["boxes_%d" % i] = np.array(boxes, np.int32)
        r = O.filter_pass(planes, O.make_desc(W, H, S, box=boxes[0], policy=O.DEGEN_EPS, n_threads=1))
        cin = planes[2:5].astype(np.float64)
        if status == 0:
            out["colour_%d" % i] = colour
            act = float(np.linalg.norm(colour - cin) / np.linalg.norm(cin))
        else:
            act = 0.0
        names.append(name); aborted.append(status != 0); activity.append(act); nbhd_max.append(int(r["nbhd_size"].max()))
        print("%-30s %s  first-pass N %4d..%4d  activity %.3e" % (name, "ABORTS" if status else "done  ",
                                                                 r["nbhd_size"].min(), r["nbhd_size"].max(), act))
        assert (status != 0) == name.startswith("abort_"), name
    aborted, activity, nbhd_max = np.array(aborted), np.array(activity), np.array(nbhd_max, np.int32)
    check_ref_filter_conditions(names, aborted, activity, nbhd_max)
    path = os.path.join(HERE, "ref_filter.npz")
    save_npz_stable(path, names=np.array(names), aborted=aborted, activity=activity, nbhd_max=nbhd_max, **out,
                    source="RPFIntegrator::ApplyRPFFilter of the reference (rpf.cpp, whole), %s %s, 1 thread (4 threads give "
                           "the same bits); inputs stored verbatim" % (_compiler(), REF_FLAGS))
    print("ref_filter.npz  %.1f KB" % (os.path.getsize(path) / 1024))


# kinds as in tests/pbrt_film_ref.py: box, triangle, gaussian, mitchell, windowed sinc
FILM_DEFAULT_RADIUS = (0.5, 2.0, 2.0, 2.0, 4.0)
FILM_DEFAULT_PARAMS = ((0.0, 0.0), (0.0, 0.0), (2.0, 0.0), (1.0 / 3.0, 1.0 / 3.0), (3.0, 0.0))
# (name, kind, radius | None, params | None, resolution, pixel bounds, S, options)
REF_FILM_CASES = [
    ("box_default", 0, None, None, (10, 7), ((0, 0), (10, 7)), 3, {}),
    ("triangle_default", 1, None, None, (10, 7), ((0, 0), (10, 7)), 3, {}),
    ("gaussian_default", 2, None, None, (10, 7), ((0, 0), (10, 7)), 3, {}),
    ("mitchell_default", 3, None, None, (10, 7), ((0, 0), (10, 7)), 3, {}),
    ("sinc_default", 4, None, None, (10, 7), ((0, 0), (10, 7)), 2, {}),
    ("gaussian_anisotropic", 2, (1.5, 2.5), (1.25, 0.0), (10, 7), ((0, 0), (10, 7)), 3, {}),
    ("mitchell_crop", 3, (2.0, 1.5), (0.5, 0.25), (16, 12), ((3, 2), (12, 9)), 3, {}),
    ("box_r15_crop", 0, (1.5, 1.5), None, (16, 12), ((5, 0), (16, 7)), 4, {}),
    ("gaussian_clamp_scale", 2, None, None, (10, 7), ((0, 0), (10, 7)), 3, dict(spikes=0.05, max_lum=10.0, scale=0.75)),
    ("triangle_zero_ray_weight", 1, None, None, (10, 7), ((0, 0), (10, 7)), 3, dict(rw="special")),
    ("sinc_integer_and_centre_pfilm", 4, (2.5, 3.0), (2.0, 0.0), (10, 7), ((0, 0), (10, 7)), 3, dict(int_frac=0.7, centre=0.2)),
]


def _film_inputs(W, H, S, origin, seed, int_frac=0.1, centre=0.0, spikes=0.0, rw=None, **_):
    """pFilm = q + u in raster coordinates, u in [0, 1) with a share exactly 0, 1 (the ends pPixel + Get2D() reaches) or 0.5;
    fp32-exact log-normal colours with zeros and optional spikes; ray weights with zeros and tiny values"""
    rng = np.random.default_rng(seed)
    F = np.float32
    q = [F(origin[0]) + np.arange(W, dtype=F)[None, :, None], F(origin[1]) + np.arange(H, dtype=F)[:, None, None]]
    u = rng.random((2, H, W, S)).astype(F)
    pick = rng.random((2, H, W, S))
    u[pick < int_frac / 2] = F(0)
    u[(pick >= int_frac / 2) & (pick < int_frac)] = F(1)
    u[(pick >= int_frac) & (pick < int_frac + centre)] = F(0.5)
    pf = np.stack([(q[a] + u[a]).astype(F) for a in range(2)])
    col = rng.lognormal(-1, 1.5, (3, H, W, S))
    col[:, rng.random((H, W, S)) < 0.03] = 0.0
    if spikes:
        col[:, rng.random((H, W, S)) < spikes] *= 1e4
    w = None
    if rw == "special":
        w = rng.uniform(0.5, 1.5, (H, W, S)).astype(F)
        w[rng.random((H, W, S)) < 0.15] = F(0)
        tiny = rng.random((H, W, S)) < 0.05
        w[tiny] = F(1e-30)
        col[:, tiny] = 1e-10
    return pf, col.astype(F), w


def ref_film_table_requests():
    rng = np.random.default_rng(404)
    F = np.float32
    req = [(k, FILM_DEFAULT_RADIUS[k], FILM_DEFAULT_RADIUS[k]) + FILM_DEFAULT_PARAMS[k] for k in range(5)]
    for i in range(35):
        k = i % 5
        rx, ry = (float(F(v)) for v in rng.uniform(0.5, 5.0, 2))
        p = {0: (0.0, 0.0), 1: (0.0, 0.0), 2: (float(F(rng.uniform(0.25, 4.0))), 0.0),
             3: (float(F(rng.uniform(0.0, 1.0))), float(F(rng.uniform(0.0, 1.0)))), 4: (float(F(rng.uniform(1.0, 5.0))), 0.0)}[k]
        req.append((k, rx, ry) + p)
    return req


def ref_film_fixture():
    """ref_film.npz: inputs verbatim, and the real Film's table, tile sums, weight sums and image"""
    import pbrt_film_ref as R
    out, names, clamp_fired = {}, [], False
    for i, (name, kind, radius, params, res, bounds, S, opt) in enumerate(REF_FILM_CASES):
        rx, ry = (FILM_DEFAULT_RADIUS[kind],) * 2 if radius is None else radius
        p0, p1 = FILM_DEFAULT_PARAMS[kind] if params is None else params
        (sx0, sy0), (sx1, sy1) = R.sample_bounds(bounds, rx, ry)
        W, H = sx1 - sx0, sy1 - sy0
        pf, col, rw = _film_inputs(W, H, S, (sx0, sy0), 100 + i, **opt)
        max_lum, scale = opt.get("max_lum", np.inf), opt.get("scale", 1.0)
        r = O.ref_film(kind, (rx, ry), (p0, p1), res, bounds, pf, col, rw, max_lum, scale)
        assert r["sample_bounds"] == ((sx0, sy0), (sx1, sy1)), (name, r["sample_bounds"])
        assert (r["tile_weight"] != 0).any()
        _, n_clamped = R.prepare(col, rw, max_lum)
        clamp_fired |= n_clamped > 0
        out["i_%d" % i] = np.array([kind, W, H, S, res[0], res[1], bounds[0][0], bounds[0][1], bounds[1][0], bounds[1][1],
                                    sx0, sy0], np.int32)
        out["f_%d" % i] = np.array([rx, ry, p0, p1, max_lum, scale], np.float32)
        out["pfilm_%d" % i], out["colour_%d" % i] = pf, col
        if rw is not None:
            out["ray_weight_%d" % i] = rw
        for k in ("table", "tile_rgb", "tile_weight", "image"):
            out["%s_%d" % (k, i)] = r[k]
        names.append(name)
        print("%-32s buffer %2dx%2dx%d  clamped samples %d" % (name, W, H, S, n_clamped))
    assert clamp_fired, "the luminance clamp must fire in at least one case"
    req = ref_film_table_requests()
    tables = O.ref_film_tables(req)
    path = os.path.join(HERE, "ref_film.npz")
    save_npz_stable(path, names=np.array(names), **out, table_requests=np.array(req, np.float32), tables=tables,
                    source="Film / FilmTile (film.h, film.cpp) and filters/*.cpp of the reference, %s %s; "
                           "inputs stored verbatim" % (_compiler(), REF_FLAGS))
    print("ref_film.npz  %.1f KB" % (os.path.getsize(path) / 1024))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "rpfb":
        O.build(force=False)
        return rpfb_fixture()
    if len(sys.argv) > 1 and sys.argv[1] == "nonfinite":
        O.build(force=False)
        if not O.ref_available():
            sys.exit("oracle/_ref/libref_mi.so missing: build it from the reference sources first (oracle/Makefile)")
        return ref_nonfinite_fixture()
    if len(sys.argv) > 1 and sys.argv[1] in ("reffilter", "reffilm"):
        O.build(force=False)
        if not O.ref_full_available():
            sys.exit("oracle/_ref/ref_filter_harness and ref_film_harness missing: build them from the reference sources "
                     "first (oracle/Makefile, target ref_full)")
        sys.path.insert(0, os.path.dirname(HERE))
        return ref_filter_fixture() if sys.argv[1] == "reffilter" else ref_film_fixture()
    if len(sys.argv) > 1 and sys.argv[1] == "refchecks":
        O.build(force=False)
        if not O.ref_available():
            sys.exit("oracle/_ref/libref_mi.so missing: build it from the reference sources first (oracle/Makefile)")
        return ref_checks_fixture()
    O.build(force=False)
    if not O.ref_available():
        sys.exit("oracle/_ref/libref_mi.so missing: this script must run where /root/reference exists")
    rng = np.random.default_rng(20250103)

    # ---- ref_mi.npz ---------------------------------------------------------------------------------
    xs, ys, lens, mis = [], [], [], []
    for x, y in mi_cases(rng):
        xs.append(x); ys.append(y); lens.append(len(x)); mis.append(O.ref_mi(x, y))
    np.savez_compressed(os.path.join(HERE, "ref_mi.npz"), x=np.concatenate(xs), y=np.concatenate(ys),
                        n=np.array(lens, np.int32), mi=np.array(mis),
                        source="MutualInformation() of /root/reference/src/custom/mi.cpp, g++ 11.4 -O3 -std=gnu++11")

    # ---- ref_ops.npz --------------------------------------------------------------------------------
    rows12 = [rng.normal(size=(8, 12)), np.float32(rng.normal(size=(16, 12)) * 0.05 + 1000.0).astype(float),
              np.tile(np.float32(rng.normal(size=(1, 12))).astype(float), (8, 1)),          # constant features
              np.float32(rng.random((64, 12))).astype(float)]
    rows19 = [np.float32(rng.normal(size=(n, 19)) * s + o).astype(float)
              for n, s, o in ((8, 1.0, 0.0), (49, 0.01, 300.0), (392, 1.0, 0.0), (200, 1e-3, -1000.0))]
    out = {}
    for i, r in enumerate(rows12):
        m, s = O.ref_mean_std(r)
        out["r12_%d" % i], out["m12_%d" % i], out["s12_%d" % i] = r, m, s
    for i, r in enumerate(rows19):
        m, s = O.ref_mean_std(r)
        out["r19_%d" % i], out["m19_%d" % i], out["s19_%d" % i] = r, m, s
        out["z19_%d" % i] = np.stack([O.ref_normalize(row, m, s) for row in r[:16]])
    # 3-sigma test: samples around the acceptance boundary, std == 0, std NaN
    f = rng.normal(size=(200, 12))
    mean = np.zeros(12)
    sd = np.full(12, 0.6)
    f[:20, 0] = 1.8            # exactly 3*0.6 -> a >= b fails (strict <)
    f[20:40, 0] = np.nextafter(1.8, 0)
    sds = np.tile(sd, (200, 1))
    sds[40:60, 3] = 0.0        # std 0 rejects everything
    sds[60:80, 5] = np.nan     # NaN std never rejects (a >= NaN is false)
    out["w3_f"], out["w3_mean"], out["w3_sd"] = f, mean, sds
    out["w3_pass"] = np.array([O.ref_within_3std(f[i], mean, sds[i]) for i in range(200)])
    np.savez_compressed(os.path.join(HERE, "ref_ops.npz"), **out,
                        source="templates of /root/reference/src/custom/ops.h, g++ 11.4 -O3 -std=gnu++11")

    # ---- e2e_*.npz ----------------------------------------------------------------------------------
    specs = [("e2e_clustered_12x10x8_box7", dict(W=12, H=10, S=8, mode="clustered", sigma_f=1e-3, sigma_c=0.01), 7, 0),
             ("e2e_smooth_10x8x8_box7", dict(W=10, H=8, S=8, mode="smooth", sigma_f=0.05, sigma_c=1e-4), 7, 0),
             ("e2e_clustered_8x6x16_box5", dict(W=8, H=6, S=16, mode="clustered", sigma_f=1e-3, sigma_c=0.01), 5, 1),
             ("e2e_constnormal_8x6x8_box7_eps", dict(W=8, H=6, S=8, mode="smooth", sigma_f=0.05, sigma_c=1e-4), 7, 1)]
    for name, gen, box, policy in specs:
        planes = fb.synth_planes(seed=7, **gen)
        if "constnormal" in name:
            planes[7:10] = np.float32([0.0, 0.0, 1.0])[:, None, None, None]
        r = O.filter_pass(planes, O.make_desc(gen["W"], gen["H"], gen["S"], box=box, policy=policy, n_threads=1))
        cin = planes[2:5].astype(np.float64)
        act = float(np.linalg.norm(r["colour"] - cin) / np.linalg.norm(cin))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), planes=planes, box=box, policy=policy,
                            colour=r["colour"], nbhd_size=r["nbhd_size"], member_hash=r["member_hash"],
                            bin_hash=r["bin_hash"], alpha=r["alpha"], beta=r["beta"], wrc=r["wrc"], mi=r["mi"],
                            mean=r["mean"], stddev=r["stddev"], status=r["status"],
                            nonfinite_pixels=r["nonfinite_pixels"], activity=act,
                            source="oracle/rpf_oracle.c (beta map REF_GCC11_O3); inputs stored verbatim")
        print("%-36s mean N %.1f activity %.3e status %d" % (name, r["sum_nbhd"] / (gen["W"] * gen["H"]), act, r["status"]))
    rpfb_fixture()
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            print("%-40s %7.1f KB" % (f, os.path.getsize(os.path.join(HERE, f)) / 1024))


if __name__ == "__main__":
    main()
