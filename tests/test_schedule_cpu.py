"""CPU tests of the per-pass schedule (RPF_FLAG_SCHEDULE): the numpy restatement tests/schedule_ref.py
against the oracle (gains 1 are the oracle's alpha / beta / W_r_c bit for bit), the presets of the library against the
restatement, what needs no device of the bindings, and the branch-coverage condition of every GPU parity case of
tests/test_schedule_gpu.py, asserted here from the oracle so that those cases are known to exercise both arms of the clamp.

rpf_set_schedule needs a context, and a context needs a device: its validation cases are in the GPU file."""
import ctypes as C
import functools

import numpy as np
import pytest

import schedule_ref as SRf
from raytracer_rpf_amd import feature_buffer as fb
from raytracer_rpf_amd import slabs

EPS, REF_ABORT = 1, 0
SIGMA = 0.5
CLUSTERED = dict(mode="clustered", sigma_f=1e-3, sigma_c=0.01)
SHARE = 0.05   # the least share of clamped, and of open, entries a parity case must have (alpha, and beta's factor)

# name: W, H, S, box, generator arguments, (gain_c, gain_f), the size classes the frame must reach (833: the rest list N > 832)
CASES = {
    "packed": (6, 5, 6, 3, dict(), (1.15, 1.6), (16, 32, 64)),
    "packed-c": (6, 5, 6, 3, CLUSTERED, (1.3, 1.15), (16, 32, 64)),
    "wave": (12, 10, 8, 7, dict(), (1.15, 1.6), (64, 128, 256, 448)),
    "wave-c": (12, 10, 8, 7, CLUSTERED, (1.3, 1.15), (64, 128, 256, 448)),
    "rest": (16, 13, 8, 11, dict(), (1.15, 1.6), (128, 256, 448, 832, 833)),
    # entry 1 of preset 1 (gains 2.2, 1.1): its beta factor is clamped on 12.7 % and open on 62.8 % of the entries, so the
    # fallback to entry 3 is not needed
    "preset": (12, 10, 8, 7, dict(flat_frac=0.94), None, (8, 128, 256, 448)),
}
PRESET_ENTRY = 1
# The two composition cases of the GPU file.  Under the published membership test the "preset" frame's neighbourhoods grow to
# N = 117 .. 391 and every W_r^{c,k} lies above 1 / 2.2 while every W_r^{f,k} lies below 1 / 1.1 (the oracle-side restatement: alpha
# clamped / open 1.0 / 0.0, beta factor 0.0 / 1.0 at the preset's gains), so that case takes gains chosen from the quantiles of the
# two ratios there (medians 0.91 and 0.58): (1.1, 2.0) gives 0.62 / 0.38 and 0.58 / 0.42.
MEMBER_GAINS = (1.1, 2.0)
SAMPLED = dict(W=12, H=10, S=8, box=11, draws=100, seed=0x5EED5EED, gains=(1.15, 1.6))    # 0.36 / 0.64 and 0.45 / 0.55
CAPS = (8, 16, 32, 64, 128, 256, 448, 832)


def gains_of(name):
    g = CASES[name][5]
    if g is None:
        _, gc, gf = SRf.preset(1, CASES[name][2])
        return float(gc[PRESET_ENTRY]), float(gf[PRESET_ENTRY])
    return g


@functools.lru_cache(maxsize=None)
def frame(W, H, S, seed=11, **kw):
    p = fb.synth_planes(W, H, S, seed=seed, **kw)
    p.setflags(write=False)
    return p


def planes_of(name):
    W, H, S, _, kw, _, _ = CASES[name]
    return frame(W, H, S, **kw)


_oracle_pass = {}


def oracle_pass(oracle, name):
    """the unscheduled pass of the case by the oracle (EPS, seed 0.5): computed once, shared, never modified"""
    if name not in _oracle_pass:
        W, H, S, box, _, _, _ = CASES[name]
        _oracle_pass[name] = oracle.filter_pass(planes_of(name), oracle.make_desc(W, H, S, box=box, policy=EPS, sigma_seed=SIGMA))
    return _oracle_pass[name]


def class_of(n):
    return next((c for c in CAPS if n <= c), 833)


def same_bits_or_nan(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


# ---- the restatement against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [EPS, REF_ABORT], ids=["eps", "ref_abort"])
@pytest.mark.parametrize("beta_map", [0, 1, 2], ids=["o3", "o2", "paper"])
@pytest.mark.parametrize("kw", [dict(), CLUSTERED, dict(flat_frac=0.94)], ids=["smooth", "clustered", "flat94"])
def test_gains_one_are_the_oracles_weights_bit_for_bit(oracle, kw, beta_map, policy):
    W, H, S, box = 12, 10, 8, 7
    want = oracle.filter_pass(frame(W, H, S, **kw), oracle.make_desc(W, H, S, box=box, policy=policy, beta_map=beta_map, sigma_seed=SIGMA))
    a, b, w = SRf.alpha_beta(want["mi"], 1.0, 1.0, beta_map, 1e-10 if policy == EPS else 0.0)
    assert same_bits_or_nan(a, want["alpha"]) and same_bits_or_nan(b, want["beta"]) and same_bits_or_nan(w, want["wrc"])
    if policy == EPS:
        assert not np.isnan(a).any() and not np.isnan(b).any()
    # gains that are NOT 1 take the other arm and change something, and the clamp leaves nothing negative
    a2, b2, w2 = SRf.alpha_beta(want["mi"], 1.15, 1.6, beta_map, 1e-10 if policy == EPS else 0.0)
    assert same_bits_or_nan(w2, want["wrc"]) and not same_bits_or_nan(a2, want["alpha"])
    with np.errstate(invalid="ignore"):
        assert not (a2 < 0).any() and (a2[~np.isnan(a2)] <= 1).all()


def test_factor_is_two_roundings_and_keeps_nan():
    w = np.array([0.0, 0.25, 1 / 3, 0.9, 1.0, np.nan, np.inf, -0.0])
    got = SRf.factor(1.15, w)
    for i, x in enumerate(w):
        t = np.float64(1.15) * np.float64(x)
        v = np.float64(1.0) - t
        want = v if not (v < 0) else 0.0
        assert (np.isnan(want) and np.isnan(got[i])) or want == got[i], (x, want, got[i])
    assert np.isnan(got[5]) and got[6] == 0.0 and got[4] == 0.0


# ---- the presets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 8, 21, 32])
@pytest.mark.parametrize("kind", [0, 1])
def test_presets_equal_the_restatement_bit_for_bit(hipmod, kind, S):
    sc = hipmod.schedule_preset(kind, S)
    seed, gc, gf = SRf.preset(kind, S)
    assert (sc.pass0, sc.reserved) == (0, 0)
    for field, want in (("seed", seed), ("gain_c", gc), ("gain_f", gf)):
        got = np.array(list(getattr(sc, field)), np.float64)
        assert got.tobytes() == want.tobytes(), (field, got, want)
    if kind == 0:
        assert set(sc.seed) == {0.002} and set(sc.gain_c) == {1.0} and set(sc.gain_f) == {1.0}
    else:
        assert sc.seed[0] == np.sqrt(0.16 / S) and sc.gain_c[0] == 2.0 and sc.gain_f[0] == 1.0 and sc.gain_c[3] == 2.0 * (1.0 + 0.1 * 3)


def test_preset_refusals(hipmod):
    L = hipmod.load()
    sc = hipmod.Schedule()
    for kind, S in [(2, 8), (-1, 8), (0, 0), (1, 0), (1, -3)]:
        assert L.rpf_schedule_preset(kind, S, C.byref(sc)) == hipmod.E_BADARG, (kind, S)
        with pytest.raises(hipmod.RpfError) as e:
            hipmod.schedule_preset(kind, S)
        assert e.value.status == hipmod.E_BADARG
    assert L.rpf_schedule_preset(0, 8, None) == hipmod.E_BADARG
    assert L.rpf_set_schedule(None, C.byref(hipmod.schedule_preset(0, 8))) == hipmod.E_BADARG        # no context
    assert L.rpf_multi_set_schedule(None, C.byref(hipmod.schedule_preset(0, 8))) == hipmod.E_BADARG


# ---- the bindings -------------------------------------------------------------------------------------------------------------
def test_flag_struct_and_helpers(hipmod):
    assert hipmod.SCHEDULE_FLAG == 8192
    assert not any(getattr(hipmod, n) == 8192 for n in dir(hipmod) if n.startswith("FLAG_"))
    assert C.sizeof(hipmod.Schedule) == 8 + 3 * 8 * hipmod.MAX_BOXES and hipmod.Schedule.seed.offset == 8
    assert hipmod.Schedule.gain_c.offset == 8 + 8 * hipmod.MAX_BOXES and hipmod.Schedule.gain_f.offset == 8 + 16 * hipmod.MAX_BOXES
    for sym in ("rpf_set_schedule", "rpf_multi_set_schedule", "rpf_schedule_preset"):
        assert sym in hipmod.EXPORTS and hasattr(hipmod.load(), sym)
    sc = hipmod.make_schedule([0.5, 0.25], [1.15, 1.3], [1.6, 1.15], pass0=2)
    assert sc.pass0 == 2 and list(sc.seed)[:3] == [0.5, 0.25, 0.002] and list(sc.gain_c)[:3] == [1.15, 1.3, 1.0]
    assert list(sc.gain_f)[:3] == [1.6, 1.15, 1.0]
    sc = hipmod.make_schedule(0.5, 1.0, 2.0)
    assert set(sc.seed) == {0.5} and set(sc.gain_c) == {1.0} and set(sc.gain_f) == {2.0}


def test_the_flag_changes_no_answer_that_needs_no_device(hipmod):
    """rpf_layout_kernels and rpf_max_nbhd ignore the flag: the same answer with and without it on every word of the other bits
    that matter to them"""
    F = hipmod.SCHEDULE_FLAG
    words = [0, hipmod.FLAG_GENERIC, hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED, hipmod.FLAG_WIDE_NBHD, hipmod.FLAG_FAST_WEIGHTS,
             hipmod.FLAG_GENERIC_PACKED, hipmod.FLAG_GENERIC | hipmod.FLAG_STREAM_FAST, hipmod.MEMBER_TEST_FLAG, hipmod.SAMPLED_NBHD_FLAG,
             hipmod.FLAG_GENERIC | hipmod.FLAG_FAST_WEIGHTS]
    for w in words:
        for lay in (dict(), dict(n_random=3, n_feat=7)):
            a, b = hipmod.make_desc(12, 10, 8, flags=w, **lay), hipmod.make_desc(12, 10, 8, flags=w | F, **lay)
            assert hipmod.layout_kernels(a) == hipmod.layout_kernels(b), (w, lay)
            assert hipmod.max_nbhd(a) == hipmod.max_nbhd(b), (w, lay)


def test_slabs_refuse_the_flag(hipmod):
    with pytest.raises(NotImplementedError) as e:
        slabs.check_desc(hipmod.make_desc(12, 10, 8, flags=hipmod.SCHEDULE_FLAG | hipmod.FLAG_GENERIC))
    assert "SCHEDULE_FLAG" in str(e.value) and "pass0" in str(e.value)
    assert slabs.check_desc(hipmod.make_desc(12, 10, 8, flags=hipmod.FLAG_GENERIC)) is not None


# ---- the branch-coverage condition of the GPU parity cases --------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_cases_exercise_both_arms_of_the_clamp(oracle, name):
    want = oracle_pass(oracle, name)
    gc, gf = gains_of(name)
    ac, ao = SRf.shares(want["mi"], gc, "c", 1e-10)
    bc, bo = SRf.shares(want["mi"], gf, "f", 1e-10)
    n = want["nbhd_size"]
    print("SCHEDULE %s: N %d .. %d, gains (%g, %g): alpha clamped / open %.3f / %.3f, beta factor %.3f / %.3f" % (
        name, n.min(), n.max(), gc, gf, ac, ao, bc, bo))
    assert min(ac, ao) >= SHARE and min(bc, bo) >= SHARE, (ac, ao, bc, bo)
    classes = {class_of(int(v)) for v in n.ravel()}
    assert set(CASES[name][6]) <= classes, (CASES[name][6], sorted(classes))        # the frame reaches the kernels it is here for
    # the scheduled values really differ from the unscheduled ones, and W_r_c does not move
    a, b, w = SRf.alpha_beta(want["mi"], gc, gf, 0, 1e-10)
    assert w.tobytes() == want["wrc"].tobytes() and a.tobytes() != want["alpha"].tobytes() and b.tobytes() != want["beta"].tobytes()
    assert (a == 0).mean() >= SHARE and ((a > 0) & (a < 1)).mean() >= SHARE


def test_composition_cases_exercise_both_arms_of_the_clamp(oracle):
    import member_test_ref as MR
    q = SAMPLED
    runs = {"member test": (planes_of("preset"), MEMBER_GAINS, 7, dict(mt=MR.published19())),
            "sampled": (frame(q["W"], q["H"], q["S"]), q["gains"], q["box"], dict(cfg=(q["seed"], 0, q["draws"])))}
    for label, (planes, (gc, gf), box, kw) in runs.items():
        want = SRf.scheduled_pass(oracle, planes, (SIGMA, gc, gf), box, **kw)
        ac, ao = SRf.shares(want["mi"], gc, "c", 1e-10)
        bc, bo = SRf.shares(want["mi"], gf, "f", 1e-10)
        print("SCHEDULE %s: N %d .. %d, alpha %.3f / %.3f, beta factor %.3f / %.3f" % (
            label, want["nbhd_size"].min(), want["nbhd_size"].max(), ac, ao, bc, bo))
        assert min(ac, ao, bc, bo) >= SHARE, (label, ac, ao, bc, bo)


def test_preset_case_uses_entry_one_of_the_published_preset():
    assert gains_of("preset") == (2.0 * (1.0 + 0.1 * 1), 1.0 + 0.1 * 1)
