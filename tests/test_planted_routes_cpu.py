"""CPU tests of the planted frames for routes 10, 11 and 12 and the scheduled kernels (tests/planted_nbhd.py): the restatements
alone, no GPU.  What tests/test_class_edges_routes_gpu.py takes for granted about its inputs is settled here: the sampled
restatement sees exactly the planted size at every target of every SAMPLED_FRAMES entry, the nmax frames have a target at
N = S + D; the membership restatement sees the planted sizes of the full-box frames under the reference's test and under one
test that is not the reference's; the gains of the scheduled cases put SHARE of the target row's entries on either arm of the
clamp; and the sampled restatement moves the colours of every target row at the active seed.

The tables below are the GPU file's too."""
import numpy as np
import pytest

import fast_weights_ref as R
import member_test_ref as MR
import planted_nbhd as P
import sampled_ref as SR
import schedule_ref as SRf
from test_gpu_parity import rel_l2
from test_schedule_fused_cpu import SHARE

EPS = 1
SIGMA = P.ACTIVE_SIGMA_SEED
CAPS = P.CAPACITIES
ROUTE10_FRAMES, GAINS, SAMPLED_GAINS, nonref, class_of = P.ROUTE10_FRAMES, P.GAINS, P.SAMPLED_GAINS, P.nonref, P.class_of


def layout(fid, table=None):
    nr, nf, _ = (table or P.FRAMES)[fid][0]
    return nr, nf


def sampled_geometry(fid):
    """W, H, S, box, D, sampling seed of a sampled frame"""
    _, S, box, D, sseed, targets, _ = P.SAMPLED_FRAMES[fid]
    return box * len(targets), box, S, box, D, sseed


_sampled = {}


def sampled_row(oracle, fid):
    """sampled_ref.sampled_pass of a sampled frame, the target row alone (the Python loop is per pixel): computed once, shared,
    never modified.  sampled_pass has no weight planes on the 27-dim layout (rpf_oracle_cf_weights is 19-dim): there they are
    row_weights below"""
    if fid not in _sampled:
        W, H, S, box, D, sseed = sampled_geometry(fid)
        nr, nf = layout(fid, P.SAMPLED_FRAMES)
        want = SR.sampled_pass(oracle, P.sampled_frame(fid)[1], (sseed, 0, D), 0, box, SIGMA, EPS, n_random=nr, n_feat=nf,
                               weights=(nr, nf) == (2, 12), rows=[(box - 1) // 2])
        if (nr, nf) != (2, 12):
            want.update(row_weights(oracle, fid))
        _sampled[fid] = want
    return _sampled[fid]


def row_weights(oracle, fid):
    """mi, alpha, beta, wrc and colour of a sampled frame's target row for ANY layout, composed from leaves that take one:
    oracle.mi over oracle.pair_table, schedule_ref.alpha_beta at gains (1, 1) -- the unscheduled statements -- and
    fast_weights_ref.pixel_colours; full-frame arrays, the other rows zero.  Held to sampled_pass (rpf_oracle_cf_weights) on a
    19-dim frame by test_row_weights_are_the_oracle_s_on_the_19_dim_layout"""
    (nr, nf, _), S, box, D, sseed, targets, _ = P.SAMPLED_FRAMES[fid]
    p32, b = P.sampled_frame(fid)[1], (box - 1) // 2
    H, W = box, box * len(targets)
    pmean, pstd = MR.stats_of(oracle, p32, EPS, nr, nf)
    pa, pb = oracle.pair_table(nr, nf)
    out = dict(mi=np.zeros((H, W, len(pa))), alpha=np.zeros((H, W, 3)), beta=np.zeros((H, W, nf)), wrc=np.zeros((H, W)),
               colour=np.zeros((3, H, W, S)))
    for x in range(W):
        nb, _, _ = SR.members(p32, pmean, pstd, (sseed, 0, D), 0, b, x, box, nr, nf)
        M, SD = oracle.mean_std(nb)
        SD = np.where(np.isnan(SD), 0.0, SD)
        with np.errstate(invalid="ignore", divide="ignore"):
            z = np.where(SD == 0, 0.0, (nb - M) / SD)
        mi = np.array([oracle.mi(z[:, i], z[:, j]) for i, j in zip(pa, pb)])
        with np.errstate(invalid="ignore"):
            mi = np.where(np.isnan(mi), 0.0, mi)                         # the EPS policy, as rpf_oracle_cf_weights applies it
        a, bt, w = SRf.alpha_beta(mi, 1.0, 1.0, 0, 1e-10, nr, nf)
        out["mi"][b, x], out["alpha"][b, x], out["beta"][b, x], out["wrc"][b, x] = mi, a, bt, w
        out["colour"][:, b, x, :] = R.pixel_colours(nb, S, M, SD, a, bt, w, box, SIGMA, EPS, np.float64, nr, nf, form="direct")
    return out


_members = {}


def member_row(oracle, fid, which, weights=False):
    """member_test_ref.member_pass of a full-box planted frame under MR.reference() ("ref") or nonref() ("nonref"), the target row
    alone: computed once, shared, never modified"""
    if (fid, which, weights) not in _members:
        _, S, box, targets, _, _ = P.FRAMES[fid]
        nr, nf = layout(fid)
        mt = MR.reference(nf) if which == "ref" else nonref(nf)
        _members[fid, which, weights] = MR.member_pass(oracle, P.frame(fid)[1], mt, box, SIGMA, EPS, n_random=nr, n_feat=nf,
                                                       weights=weights, rows=[(box - 1) // 2])
    return _members[fid, which, weights]


# ---- the sampled frames ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", list(P.SAMPLED_FRAMES))
def test_sampled_restatement_sees_the_planted_sizes(oracle, fid):
    (nr, nf, dt), S, box, D, sseed, targets, _ = P.SAMPLED_FRAMES[fid]
    stored, p32, pixels, planted = P.sampled_frame(fid)
    W, H = box * len(targets), box
    assert planted == targets and p32.shape == (5 + nr + nf, H, W, S) and not p32.flags.writeable and not stored.flags.writeable
    pmean, pstd = MR.stats_of(oracle, p32, EPS, nr, nf)
    f0 = 5 + nr
    base = np.sort(np.linspace(0.4, 0.6, S).astype(np.float32).astype(np.float16 if dt == "f16" else np.float32).astype(np.float32))
    interleaved = 0
    for (y, x), n in zip(pixels, targets):
        nb, codes, kept = SR.members(p32, pmean, pstd, (sseed, 0, D), 0, y, x, box, nr, nf)
        qq = SR.draws(sseed, 0, 0, D, box, W, H, S, x, y)
        print("%s target (%d, %d): planted N %d, class %d, %d distinct draws of %d, %d kept" % (fid, y, x, n, class_of(n), len(qq), D, len(kept)))
        assert nb.shape[0] == len(codes) == n and len(kept) == n - S and S <= n <= S + len(qq) <= S + D
        # its own samples were never touched: every feature column is the unpushed permutation, its statistics an unpushed pixel's
        assert np.array_equal(np.sort(p32[f0:, y, x, :], axis=-1), np.broadcast_to(base, (nf, S)))
        np.testing.assert_allclose(pmean[y, x], pmean[pixels[0]], rtol=1e-6)
        np.testing.assert_allclose(pstd[y, x], pstd[pixels[0]], rtol=1e-6)
        assert 1.4 < (np.abs(base - base.mean()).max() / pstd[y, x]).max() < 1.7
        # the accepted draws interleave with rejected ones in visiting order
        rejected = np.setdiff1d(qq, kept)
        if len(kept) >= 8 and len(rejected) >= 8:
            assert ((rejected > kept.min()) & (rejected < kept.max())).any() and ((kept > rejected.min()) & (kept < rejected.max())).any()
            interleaved += 1
    assert interleaved >= 3 or fid in P.NMAX_FRAMES                     # (an nmax frame pushes next to nothing)
    # the row restatement the GPU file compares with agrees
    want = sampled_row(oracle, fid)
    assert [int(want["nbhd_size"][y, x]) for y, x in pixels] == list(targets)


def test_every_class_edge_a_sampled_pass_reaches_is_planted():
    planted = set(n for v in P.SAMPLED_FRAMES.values() for n in v[5])
    for cap in CAPS[:-1]:                      # N = 3136 cannot be reached on a sampled pass: the module docstring of planted_nbhd
        assert cap in planted and cap + 1 in planted, cap
    d27 = set(n for v in P.SAMPLED_FRAMES.values() if v[0][:2] == (4, 18) for n in v[5])
    assert {16, 17, 64, 65, 128, 129} <= d27 and {833, 1600, 1601} <= d27
    _, S, box, D, _, _, _ = P.SAMPLED_FRAMES["SP32"]
    assert S + D == CAPS[-1] and (box * box - 1) * S > 4096


# the translation units of the compiled kernels: per layout and build, part 1's packed kernels (N <= 64) and its K <= 7 kernels
# (N <= 448), part 2 (K 13 / 25: N <= 1600) and part 3 (K 49: N <= 3136)
PART_BANDS = ((1, 64), (65, 448), (449, 1600), (1601, 3136))


@pytest.mark.parametrize("build", ["plain", "scheduled", "listed", "listed_scheduled"])
@pytest.mark.parametrize("lay", [(2, 12, "f32"), (4, 18, "f16")], ids=["d19", "d27"])
def test_every_part_of_every_compiled_build_has_a_planted_size(lay, build):
    """a property of the frame tables: the parametrised GPU tests iterate them, so each layout x build x part -- each entry of the
    dispatch table in csrc/rpf_kernels.hip -- runs at a planted N only if the tables hold one in its band"""
    table = P.SAMPLED_FRAMES if build.startswith("listed") else P.FRAMES
    fids = {"plain": P.FRAMES, "scheduled": GAINS, "listed": P.SAMPLED_FRAMES, "listed_scheduled": SAMPLED_GAINS}[build]
    assert set(fids) <= set(table)
    planted = sorted(set(n for fid in fids if table[fid][0] == lay for n in table[fid][5 if table is P.SAMPLED_FRAMES else 3]))
    for lo, hi in PART_BANDS:
        assert any(lo <= n <= hi for n in planted), (lay, build, (lo, hi), planted)


@pytest.mark.parametrize("fid", P.NMAX_FRAMES)
def test_nmax_frames_have_a_target_at_s_plus_d(oracle, fid):
    _, S, box, D, sseed, targets, _ = P.SAMPLED_FRAMES[fid]
    _, p32, pixels, _ = P.sampled_frame(fid)
    W, H = box * len(targets), box
    full = [(y, x) for (y, x), n in zip(pixels, targets) if n == S + D]
    assert full and S + D - 1 in targets and max(targets) == S + D
    want = sampled_row(oracle, fid)
    for y, x in full:
        qq = SR.draws(sseed, 0, 0, D, box, W, H, S, x, y)
        assert len(qq) == D and want["nbhd_size"][y, x] == S + D           # every draw distinct, in the frame, and a member
    nmax = min(box * box * S, S + D)
    assert nmax == S + D
    if fid == "NM100":
        assert class_of(nmax) == 128 and nmax not in CAPS                  # the pass's bound strictly inside a class
    else:
        assert nmax in CAPS                                                # ... and on a class capacity
    print("%s: nmax %d in class %d, targets at nmax %s" % (fid, nmax, class_of(nmax), full))


def test_plant_sampled_refuses_what_it_cannot_plant():
    with pytest.raises(ValueError):
        P.plant_sampled(1, 7, (1,), 8, 1)
    with pytest.raises(ValueError):
        P.plant_sampled(8, 7, (7,), 8, P.SAMPLING_SEED)            # below S
    with pytest.raises(ValueError):
        P.plant_sampled(8, 7, (17,), 8, P.SAMPLING_SEED)           # above S + D
    with pytest.raises(ValueError):
        P.plant_sampled(8, 7, (16,) * 7, 8, P.SAMPLING_SEED)       # the seventh target has 5 distinct draws
    planes, pixels = P.plant_sampled(4, 3, (4, 6), 6, 3, n_random=3, n_feat=7, seed=5)
    assert planes.shape == (15, 3, 6, 4) and planes.dtype == np.float32 and pixels == [(1, 1), (1, 4)]
    again, _ = P.plant_sampled(4, 3, (4, 6), 6, 3, n_random=3, n_feat=7, seed=5)
    other, _ = P.plant_sampled(4, 3, (4, 6), 6, 3, n_random=3, n_feat=7, seed=6)
    assert np.array_equal(planes, again) and not np.array_equal(planes, other)


@pytest.mark.parametrize("fid", ["NM16", "SP8"])
def test_row_weights_are_the_oracle_s_on_the_19_dim_layout(oracle, fid):
    """row_weights, which carries the 27-dim frame, against sampled_pass on frames both can take: bit for bit"""
    b = (P.SAMPLED_FRAMES[fid][2] - 1) // 2
    want, got = sampled_row(oracle, fid), row_weights(oracle, fid)
    for k in ("mi", "alpha", "beta", "wrc"):
        assert np.array_equal(got[k][b], want[k][b]), k
    assert np.array_equal(got["colour"][:, b], want["colour"][:, b])


@pytest.mark.parametrize("fid", list(P.SAMPLED_FRAMES))
def test_sampled_restatement_moves_the_colours_of_the_target_row(oracle, fid):
    """the `moved` condition of tests/test_class_boundaries_gpu.py, on the restatement alone"""
    b = (P.SAMPLED_FRAMES[fid][2] - 1) // 2
    cin = P.sampled_frame(fid)[1][2:5].astype(np.float64)
    moved = rel_l2(sampled_row(oracle, fid)["colour"][:, b], cin[:, b])
    print("%s: the restatement moves the target row by %.3f" % (fid, moved))
    assert moved > 0.05


# ---- route 10 on the full-box frames ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ref", "nonref"])
@pytest.mark.parametrize("fid", ROUTE10_FRAMES)
def test_membership_restatement_sees_the_planted_sizes(oracle, fid, which):
    _, S, box, targets, _, _ = P.FRAMES[fid]
    nr, nf = layout(fid)
    _, p32, pixels, _ = P.frame(fid)
    b = (box - 1) // 2
    mt = MR.reference(nf) if which == "ref" else nonref(nf)
    if which == "nonref":
        assert len(set(mt[0])) == nf and mt[0].min() >= 2 and mt[0].max() <= 50 and (mt[1] < 0).all()
    n, codes = MR.counts(oracle, p32, mt, box, nr, nf, rows=[b])
    assert [int(n[y, x]) for y, x in pixels] == list(targets) and all(y == b for y, _ in pixels)
    assert all(len(codes[p]) == t for p, t in zip(pixels, targets))
    want = member_row(oracle, fid, which)
    assert np.array_equal(want["nbhd_size"][b], n[b])


# ---- the scheduled cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", ROUTE10_FRAMES)
def test_gains_reach_both_arms_of_the_clamp_on_the_target_rows(oracle, fid):
    box = P.FRAMES[fid][2]
    nr, nf = layout(fid)
    mi = P.oracle_pass(oracle, fid, EPS, SIGMA)["mi"][(box - 1) // 2]
    gc, gf = GAINS[fid]
    ac, ao = SRf.shares(mi, gc, "c", 1e-10, nr, nf)
    bc, bo = SRf.shares(mi, gf, "f", 1e-10, nr, nf)
    print("%s target row, gains (%g, %g): alpha clamped / open %.3f / %.3f, beta factor %.3f / %.3f" % (fid, gc, gf, ac, ao, bc, bo))
    assert min(ac, ao) >= SHARE and min(bc, bo) >= SHARE, (ac, ao, bc, bo)


@pytest.mark.parametrize("fid", list(P.SAMPLED_FRAMES))
def test_sampled_gains_reach_both_arms_of_the_clamp_on_the_target_rows(oracle, fid):
    b = (P.SAMPLED_FRAMES[fid][2] - 1) // 2
    nr, nf = layout(fid, P.SAMPLED_FRAMES)
    mi = sampled_row(oracle, fid)["mi"][b]
    gc, gf = SAMPLED_GAINS[fid]
    ac, ao = SRf.shares(mi, gc, "c", 1e-10, nr, nf)
    bc, bo = SRf.shares(mi, gf, "f", 1e-10, nr, nf)
    print("%s target row, gains (%g, %g): alpha clamped / open %.3f / %.3f, beta factor %.3f / %.3f" % (fid, gc, gf, ac, ao, bc, bo))
    assert min(ac, ao) >= SHARE and min(bc, bo) >= SHARE, (ac, ao, bc, bo)
