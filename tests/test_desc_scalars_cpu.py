"""CPU tests of tests/desc_scalars.py: what tests/test_desc_scalars_gpu.py takes for granted, settled on the oracle and the
restatement alone.

1. The oracle equals the restatement.  For every full-box frame of the table and every combo, oracle.filter_pass(..., beta_map,
   eps) gives alpha, beta and W_r_c bit-equal to schedule_ref.alpha_beta on the oracle's own MI, and MI, statistics and discrete
   planes with the bits of the default pass.  (The sampled frames have no oracle pass; on the 19-dim ones the same is held, under
   every combo, through rpf_oracle_cf_weights -- the stage 3c of sampled_ref.sampled_pass -- on the members of the target row;
   rpf_oracle_cf_weights is 19-dim, so the 27-dim sampled frames rest on the full-box H frames.)  This licenses the GPU file to build the
   oracle's alpha and beta of a combo from the cached default pass.
2. The combos are not vacuous on any frame: alpha or beta change bits, eps 0.0123 moves alpha by >= 1e-4 relative L2, presets 1
   and 2 move beta by >= 0.05, every finite alpha and beta is <= 1 (the premise weight_k <= 1 of tests/stage4_bars.py), and
   under the frame's gains both arms of the clamp hold SHARE at the combo's eps.
   Two layouts have exceptions that follow from the rule, asserted as such: with n_feat = 3 there is no gap and no D_r_fk term, so
   presets 0 and 1 are the same statement; with n_feat = 5 the two differ in beta[4] alone.
3. check_stage3c raises on six planted faults, (a) to (f).
4. eps = 0 under EPS is IEEE: on the frames of section f the oracle's alpha[..., 0] and W_r_c are NaN on every pixel, beta is
   finite, every colour falls back to the input, the status is OK and every pixel is counted."""
import numpy as np
import pytest

import desc_scalars as D
import member_test_ref as MR
import planted_nbhd as P
import sampled_ref as SR
import schedule_ref as SRf
from desc_scalars import COMBOS, DEFAULT, EPS, SIGMA, check_stage3c, same, same_or_nan
from test_gpu_parity import rel_l2
from test_planted_routes_cpu import SHARE, member_row, sampled_row

FULL_BOX = [f for f in D.FRAME_IDS if f not in P.SAMPLED_FRAMES]
SAMPLED = [f for f in D.FRAME_IDS if f in P.SAMPLED_FRAMES]
SAMPLED_19 = [f for f in SAMPLED if P.SAMPLED_FRAMES[f][0][:2] == (2, 12)]
NAN_FRAMES = ("U8", "H8", "B32")
FRONT = ("nbhd_size", "member_hash", "bin_hash", "mean", "stddev", "mi")


def mi_of(oracle, fid):
    """the MI the non-vacuity checks run on: the oracle's default pass (whole frame), or the sampled restatement's target row"""
    f = D.frame(fid)
    if f.sampling is None:
        return D.oracle_pass(oracle, f)["mi"]
    return sampled_row(oracle, fid)["mi"][(f.box - 1) // 2]


# ---- 1. the oracle equals the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FULL_BOX)
def test_oracle_equals_the_restatement(oracle, fid):
    f = D.frame(fid)
    nr, nf, _ = f.lay
    base = D.oracle_pass(oracle, f)
    assert [int(base["nbhd_size"][y, x]) for y, x in f.pixels] == list(f.targets)
    for beta_map, eps in [DEFAULT] + COMBOS:
        want = D.oracle_pass(oracle, f, beta_map, eps)
        a, b, w = SRf.alpha_beta(want["mi"], 1.0, 1.0, beta_map, eps, nr, nf)
        assert same_or_nan(want["alpha"], a) and same_or_nan(want["beta"], b) and same_or_nan(want["wrc"], w), (beta_map, eps)
        check_stage3c(want, beta_map, eps, None, nr, nf)
        for k in FRONT:
            assert same(want[k], base[k]), (k, beta_map, eps)
        assert want["status"] == 0 and np.isfinite(want["colour"]).all()


@pytest.mark.parametrize("fid", SAMPLED_19)
def test_sampled_restatement_equals_the_restatement(oracle, fid):
    """rpf_oracle_cf_weights on the members of a sampled pass, target row: the same statement"""
    f = D.frame(fid)
    b = (f.box - 1) // 2
    sseed, draws = f.sampling
    base = sampled_row(oracle, fid)
    pmean, pstd = MR.stats_of(oracle, f.p32, EPS)
    for x in range(f.W):                                # the statements of sampled_ref.sampled_pass, the members gathered once
        nb, _, _ = SR.members(f.p32, pmean, pstd, (sseed, 0, draws), 0, b, x, f.box)
        M, SD = oracle.mean_std(nb)
        SD = np.where(np.isnan(SD), 0.0, SD)
        with np.errstate(invalid="ignore", divide="ignore"):
            z = np.where(SD == 0, 0.0, (nb - M) / SD)
        assert nb.shape[0] == base["nbhd_size"][b, x]
        for beta_map, eps in [DEFAULT] + COMBOS:
            a, bt, w, mi = oracle.cf_weights(z, beta_map, EPS, eps)
            assert np.array_equal(mi, base["mi"][b, x])
            a2, b2, w2 = SRf.alpha_beta(mi, 1.0, 1.0, beta_map, eps)
            assert same_or_nan(a, a2) and same_or_nan(bt, b2) and same_or_nan(w, w2), (x, beta_map, eps)


# ---- 2. the combos are not vacuous ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", D.FRAME_IDS)
def test_combos_move_alpha_and_beta(oracle, fid):
    f = D.frame(fid)
    nr, nf, _ = f.lay
    mi = mi_of(oracle, fid)
    gains = D.gains_of(fid)
    a0, b0, w0 = SRf.alpha_beta(mi, 1.0, 1.0, *DEFAULT, nr, nf)
    for beta_map, eps in COMBOS:
        a, b, w = SRf.alpha_beta(mi, 1.0, 1.0, beta_map, eps, nr, nf)
        da, db = rel_l2(a, a0), rel_l2(b, b0)
        print("%s (%d, %g): alpha moves %.3e, beta %.3e; largest alpha %.3f, beta %.3f" % (fid, beta_map, eps, da, db, a.max(), b.max()))
        assert np.isfinite(a).all() and np.isfinite(b).all() and a.max() <= 1 and b.max() <= 1
        if nf == 3 and (beta_map, eps) == (1, 1e-10):
            assert same(a, a0) and same(b, b0)          # no gap, no D_r_fk term: presets 0 and 1 are one statement
            continue
        assert not same(a, a0) or not same(b, b0)
        if eps != 1e-10:
            assert da >= 1e-4, da
        if beta_map == 2 or (beta_map == 1 and nf > 5):
            assert db >= 0.05, db
        elif beta_map == 1 and nf == 5 and eps == 1e-10:
            assert same(b[..., :4], b0[..., :4]) and not same(b[..., 4], b0[..., 4]) and (b[..., 4] == 0).all()
        if gains is not None:
            ag, bg, _ = SRf.alpha_beta(mi, gains[0], gains[1], beta_map, eps, nr, nf)
            assert ag.max() <= 1 and bg.max() <= 1 and ag.min() >= 0 and bg.min() >= 0
    if gains is not None:
        for eps in (1e-10, 0.0123):                     # the shares of the target row, as tests/test_planted_routes_cpu.py takes them
            row = mi[(f.box - 1) // 2] if f.sampling is None else mi
            ac, ao = SRf.shares(row, gains[0], "c", eps, nr, nf)
            bc, bo = SRf.shares(row, gains[1], "f", eps, nr, nf)
            print("%s gains (%g, %g) eps %g: alpha clamped / open %.3f / %.3f, beta factor %.3f / %.3f" % (fid, *gains, eps, ac, ao, bc, bo))
            assert min(ac, ao) >= SHARE and min(bc, bo) >= SHARE, (eps, ac, ao, bc, bo)


def test_route_9_row_has_the_planted_sizes_and_an_mi(oracle):
    want = member_row(oracle, "B16", "nonref", weights=True)
    f = D.frame("B16")
    assert [int(want["nbhd_size"][y, x]) for y, x in f.pixels] == list(f.targets)
    assert np.isfinite(want["mi"][(f.box - 1) // 2]).all()


def test_the_table_reaches_every_body_and_build():
    rows = D.ROWS
    for body in "ABCDEF":
        assert any(body in r.bodies and r.gains is None and r.fast is None for r in rows), body
        assert any(body in r.bodies and r.gains is not None for r in rows), body
    for lay in ((2, 12, "f32"), (4, 18, "f16")):        # plain, scheduled, listed and listed-scheduled builds, both compiled layouts
        for mode in ("compiled", "r12"):
            for scheduled in (False, True):
                assert any(r.mode == mode and D.frame(r.fid).lay == lay and (r.gains is not None) == scheduled for r in rows), (lay, mode, scheduled)
    assert {r.fast for r in rows} == {None, "FAST_WEIGHTS", "GENERIC_FAST", "STREAM_FAST"}
    # gains as the flag allows: a scheduled pass is refused with FAST_WEIGHTS, the generic flags run their `sched` branch in fp32
    assert {(r.fast, r.mode) for r in rows if r.fast and r.gains is not None} == {("GENERIC_FAST", "g5"), ("STREAM_FAST", "g3"), ("STREAM_FAST", "w6")}
    assert {x for r in rows for x in r.routes} == set(range(14))
    assert all(r.gains is None or len(r.gains) == 2 for r in rows)


# ---- 3. planted faults ---------------------------------------------------------------------------------------------------------------
def wrong_beta(mi, eps, gap, shift, nR=2, nF=12):
    """stage 3c at gains (1, 1) with the reference's stack rule restated wrongly: zeros up to `gap`, then D_r_fk[k - gap + shift]"""
    r = SRf.ratios(mi, eps, nR, nF)
    cols = [r["D_f_ck"][..., k] if k < 3 else (np.zeros_like(r["den"]) if k < gap else r["D_r_fk"][..., k - gap + shift]) for k in range(nF)]
    return (1 - r["W_r_f"]) * (np.stack(cols, -1) / r["den"][..., None])


def planted(want, **planes):
    got = {k: want[k] for k in ("mi", "alpha", "beta", "wrc")}
    got.update(planes)
    return got


def test_check_stage3c_raises_on_planted_faults(oracle):
    f = D.frame("U8")
    mi = D.oracle_pass(oracle, f)["mi"]
    gains = P.GAINS["U8"]

    def stated(beta_map, eps, g=(1.0, 1.0)):
        a, b, w = SRf.alpha_beta(mi, g[0], g[1], beta_map, eps)
        return dict(mi=mi, alpha=a, beta=b, wrc=w)

    def raises(got, beta_map, eps, g=None):
        with pytest.raises(AssertionError):
            check_stage3c(got, beta_map, eps, g, 2, 12)
    for beta_map, eps in [DEFAULT] + COMBOS:                                         # the control: the right statement passes
        check_stage3c(stated(beta_map, eps), beta_map, eps, None, 2, 12)
        check_stage3c(stated(beta_map, eps, gains), beta_map, eps, gains, 2, 12)
    raises(stated(0, 1e-10), 0, 0.0123)                                              # (a) eps 1e-10 where the call said 0.0123
    raises(stated(0, 1e-10), 1, 1e-10)                                               # (b) preset 0 where the call said 1
    right = stated(1, 1e-10)
    assert same(wrong_beta(mi, 1e-10, 8, 0), right["beta"])                          # (wrong_beta with the right arguments is right)
    raises(planted(right, beta=wrong_beta(mi, 1e-10, 4, 0)), 1, 1e-10)               # (c) the gap 4 where preset 1 wants 8
    raises(planted(right, beta=wrong_beta(mi, 1e-10, 8, 1)), 1, 1e-10)               # (d) D_r_fk[k - gap + 1]
    nan = D.oracle_pass(oracle, D.nan_frame("U8"), 0, 0.0)                           # (e) 0.0 where the contract gives NaN
    check_stage3c(nan, 0, 0.0, None, 2, 12)
    assert np.isnan(nan["alpha"]).any()
    raises(planted(nan, alpha=np.nan_to_num(nan["alpha"], nan=0.0)), 0, 0.0)
    raises(planted(nan, wrc=np.nan_to_num(nan["wrc"], nan=0.0)), 0, 0.0)
    raises(stated(2, 0.0123), 2, 0.0123, gains)                                      # (f) gains (1, 1) where the call had gains
    raises(planted(stated(2, 0.0123, gains), beta=stated(2, 0.0123)["beta"]), 2, 0.0123, gains)


# ---- 4. eps = 0 under EPS ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", NAN_FRAMES)
def test_eps_zero_is_ieee_in_the_oracle(oracle, fid):
    f = D.nan_frame(fid)
    nr, nf, _ = f.lay
    got = D.oracle_pass(oracle, f, 0, 0.0)
    assert [int(got["nbhd_size"][y, x]) for y, x in f.pixels] == list(f.targets)     # colour is not in the membership test
    assert np.isnan(got["alpha"][..., 0]).all() and np.isnan(got["wrc"]).all() and np.isfinite(got["beta"]).all()
    assert np.isfinite(got["alpha"][..., 1:]).all()
    assert np.array_equal(got["colour"], f.p32[2:5].astype(np.float64))
    assert got["status"] == 0 and got["nonfinite_pixels"] == f.W * f.H
    check_stage3c(got, 0, 0.0, None, nr, nf)
    for eps in (1e-10, 0.0123):
        fin = D.oracle_pass(oracle, f, 0, eps)
        assert all(np.isfinite(fin[k]).all() for k in ("alpha", "beta", "wrc", "colour")) and fin["nonfinite_pixels"] == 0
        assert rel_l2(fin["colour"], f.p32[2:5].astype(np.float64)) > 0.05
