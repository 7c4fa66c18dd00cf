#!/usr/bin/env python3
"""Generates the fixtures of the wide-neighbourhood tests: tests/golden/wide_<frame>.npz for the frames of tests/wide_frames.py.

    python tests/golden/make_wide_golden.py [frame ...]          (default: every frame; about a minute each per policy)

The oracle (oracle/rpf_oracle.c) filters the row of the targets of each frame (rows [28, 29), box 57, 21 spp, sigma seed 0.5)
under both degenerate policies -- a third of a second per pixel at N ~ 66000, far too slow for a test to do live.  A fixture
holds the oracle's outputs for that row only, never the planes (the tests rebuild those and compare `crc`):

    nbhd_size, mean, stddev, mi, bin_hash, member_hash   the row's debug planes (checked equal under both policies)
    alpha_<p>, beta_<p>, wrc_<p>, colour_<p>, status_<p>, nonfinite_<p>   per policy p = ref_abort | eps
    crc, targets                                          CRC-32 of the stored planes; the planted sizes

What the EPS comparison needs: from N = 48586 on the oracle's fixed-point table saturates, so its
zero-band test is not to be trusted there; the fixtures therefore hold no table anywhere near the band.  Checked here and
again in tests/test_wide_nbhd_cpu.py: min |mi| > 1e-9, and the MI of the two policies are the same bits.

The heavy frame is stored under REF_ABORT only.  Its cells of N - 1 and N - 2 counts index the oracle's table above 48585,
where every entry is the same saturated value: under EPS the oracle's fixed-point sum of the tables (2, 5) ... (3, 6) cancels
to zero and it reports MI = 0 where the reference's own expression (REF_ABORT) gives 2e-4.  There is no valid EPS oracle for
that frame; the GPU test compares its EPS run with the REF_ABORT fixture's discrete outputs and MI.

Fixtures are data only: expected outputs.
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
import wide_frames as F  # noqa: E402

MAX_BYTES = 746699   # the largest file tests/golden held before these
SHARED = ("nbhd_size", "mean", "stddev", "mi", "bin_hash", "member_hash")
PER_POLICY = ("alpha", "beta", "wrc")
POLICIES = (("ref_abort", O.DEGEN_REF_ABORT), ("eps", O.DEGEN_EPS))


def heavy_counts():
    """the joint cells of the heavy frame's four tables, counted with numpy over the target's members"""
    _, p32, _, (n,) = F.frame("heavy")
    mem = F.members("heavy")
    assert int(mem.sum()) == n, (int(mem.sum()), n)
    common = {c: (p32[c] == F.HEAVY_COMMON)[mem] for c in F.HEAVY_COLUMNS}
    out = {}
    for a, b in ((2, 5), (2, 6), (3, 5), (3, 6)):
        out[a, b] = int((common[a] & common[b]).sum())
    return n, out


def make(fid):
    (nr, nf, _), targets = F.FRAMES[fid]
    _, p32, pixels, _ = F.frame(fid)
    W, H = F.geometry(fid)
    if fid == "heavy":
        n, cells = heavy_counts()
        assert cells[2, 5] == n - 1 and cells[2, 6] == n - 1 and cells[3, 5] == n - 2 and cells[3, 6] == n - 2, cells
        assert n - 2 > 65535
    lay = dict(n_random=nr, n_feat=nf) if (nr, nf) != (2, 12) else {}
    out = dict(crc=np.uint32(F.checksum(fid)), targets=np.array(targets, np.int32))
    first = None
    for name, policy in (POLICIES[:1] if fid == "heavy" else POLICIES):
        r = O.filter_pass(p32, O.make_desc(W, H, F.S, box=F.BOX, row_begin=F.ROW, row_end=F.ROW + 1, policy=policy,
                                           sigma_seed=F.SIGMA_SEED, **lay))
        row = {k: r[k][F.ROW].copy() for k in SHARED + PER_POLICY}
        for (y, x), n in zip(pixels, targets):
            assert y == F.ROW and row["nbhd_size"][x] == n, (fid, x, n, int(row["nbhd_size"][x]))
        assert np.abs(row["mi"]).min() > 1e-9, (fid, name, float(np.abs(row["mi"]).min()))
        if first is None:
            first = row
            out.update({k: row[k] for k in SHARED})
        else:
            for k in SHARED:
                assert np.array_equal(row[k], first[k]), (fid, k, "differs between the policies")
        for k in PER_POLICY:
            out["%s_%s" % (k, name)] = row[k]
        out["colour_" + name] = r["colour"][:, F.ROW].copy()
        out["status_" + name] = np.int32(r["status"])
        out["nonfinite_" + name] = np.int64(r["nonfinite_pixels"])
        cin = p32[2:5, F.ROW].astype(np.float64)
        print("%s %s: N %d .. %d, |mi| %.3e .. %.3e, status %d, colours moved %.3f rel-L2" % (
            fid, name, row["nbhd_size"].min(), row["nbhd_size"].max(), np.abs(row["mi"]).min(), np.abs(row["mi"]).max(),
            r["status"], np.linalg.norm(out["colour_" + name] - cin) / np.linalg.norm(cin)), flush=True)
    path = os.path.join(HERE, "wide_%s.npz" % fid)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (path, size)
    print("%s: %d bytes" % (path, size), flush=True)


if __name__ == "__main__":
    O.build()
    for fid in (sys.argv[1:] or list(F.FRAMES)):
        make(fid)
