#!/usr/bin/env python3
"""Generates tests/golden/wide_classes.npz, the fixture of the route-7 tests (tests/wide_classes_frames.py).

    python tests/golden/make_wide_classes_golden.py          (about ten minutes)

The oracle (oracle/rpf_oracle.c) filters the row of the targets (row 28, box 57, 21 spp, sigma seed 0.5) under both degenerate
policies, as make_wide_golden.py does for its frames.  The fixture holds, never the planes (the tests rebuild those and compare
`crc`):

    nbhd_size, member_hash                                the whole row (the same under both policies: checked)
    pix                                                   the columns the stage outputs are kept for (fixture_pixels())
    mean, stddev, bin_hash                                those pixels (the same under both policies: checked)
    mi_<p>, alpha_<p>, beta_<p>, wrc_<p>, colour_<p>      those pixels, per policy p = ref_abort | eps
    status_<p>, nonfinite_<p>, first_bad_<p>              the run's status
    crc, targets

From N = 48586 on the oracle's own fixed-point table saturates under EPS: it is a valid reference
there only for tables far from the zero band, so every fixture pixel of that size must have min |mi| > 1e-9 -- asserted here
and in tests/test_wide_classes_cpu.py.  Fixtures are data only: expected outputs.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import rpf_pkg  # noqa: E402

rpf_pkg.load()
import pyoracle as O  # noqa: E402
import wide_classes_frames as F  # noqa: E402

MAX_BYTES = 512 * 1024
POLICIES = (("ref_abort", O.DEGEN_REF_ABORT), ("eps", O.DEGEN_EPS))


def make():
    planes, pixels = F.frame()
    pix = F.fixture_pixels()
    out = dict(crc=np.uint32(F.checksum()), targets=np.array(F.TARGETS, np.int32), pix=pix)
    first = None
    for name, policy in POLICIES:
        r = O.filter_pass(planes, O.make_desc(F.W, F.H, F.S, box=F.BOX, row_begin=F.ROW, row_end=F.ROW + 1, policy=policy,
                                              sigma_seed=F.SIGMA_SEED))
        row = {k: r[k][F.ROW].copy() for k in ("nbhd_size", "member_hash", "mean", "stddev", "bin_hash", "mi", "alpha", "beta", "wrc")}
        for (y, x), n in zip(pixels, F.TARGETS):
            assert y == F.ROW and row["nbhd_size"][x] == n, (x, n, int(row["nbhd_size"][x]))
        big = row["nbhd_size"][pix] >= 48586
        assert np.abs(row["mi"][pix][big]).min() > 1e-9, float(np.abs(row["mi"][pix][big]).min())
        if first is None:
            first = row
            out.update(nbhd_size=row["nbhd_size"], member_hash=row["member_hash"])
            out.update({k: row[k][pix] for k in ("mean", "stddev", "bin_hash")})
        else:
            for k in ("nbhd_size", "member_hash", "mean", "stddev", "bin_hash"):
                assert np.array_equal(row[k], first[k], equal_nan=True), (k, "differs between the policies")
        for k in ("mi", "alpha", "beta", "wrc"):
            out["%s_%s" % (k, name)] = row[k][pix]
        out["colour_" + name] = r["colour"][:, F.ROW][:, pix].copy()
        out["status_" + name] = np.int32(r["status"])
        out["nonfinite_" + name] = np.int64(r["nonfinite_pixels"])
        out["first_bad_" + name] = np.int64(r["first_bad_pixel"])
        print("%s: N %d .. %d, status %d, %d non-finite pixels" % (name, row["nbhd_size"].min(), row["nbhd_size"].max(), r["status"],
                                                                   r["nonfinite_pixels"]), flush=True)
    path = os.path.join(HERE, "wide_classes.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (path, size)
    print("%s: %d bytes, %d fixture pixels" % (path, size, len(pix)), flush=True)


if __name__ == "__main__":
    O.build()
    make()
