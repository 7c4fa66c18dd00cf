"""CPU tests of the per-pass activity report (RPF_FLAG_PASS_REPORT): the flag and the ctypes mirror against
include/rpf_hip.h (sizes and offsets from a program compiled against the header), the fold against the numpy restatement
tests/pass_report_ref.py bit for bit, and the restatement on oracle outputs -- the coverage conditions of the frames the GPU file
uses, asserted here so that its cases are known not to be vacuous.

The frames (12x10x8, box 7, EPS policy, generator seed 11):
  identity   the smooth generator with sigma_c = 0.1 at sigma_seed 0.002: the oracle returns its input bit for bit
  active     the clustered generator.  At sigma_seed 0.5 the oracle moves EVERY sample (unchanged_samples = 0 of 960, at each of
             the generator seeds 1 .. 12), so that seed gives moved2 > 0 alone; 0 < unchanged_samples < samples wants another
             seed: 0.02, the largest of 0.5, 0.1, 0.05, 0.02 at which the oracle leaves some samples alone (22 of 960)
  scheduled  the flat_frac = 0.94 frame under gains (2.2, 1.1) as in test_schedule_*: alpha is clamped on its 113 flat pixels
  own-only   the same frame: 113 of 120 pixels have N = S"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import pass_report_ref as PR
import schedule_ref as SRf
from raytracer_rpf_amd import feature_buffer as fb
from raytracer_rpf_amd import slabs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1
W, H, S, BOX = 12, 10, 8, 7
CLUSTERED = dict(mode="clustered", sigma_f=1e-3, sigma_c=0.01)
IDENTITY = (dict(sigma_c=0.1), 0.002)
ACTIVE = (CLUSTERED, 0.02)
FLAT = dict(flat_frac=0.94)
SCHED_GAINS = (2.2, 1.1)


@functools.lru_cache(maxsize=None)
def frame(w=W, h=H, s=S, seed=11, **kw):
    p = fb.synth_planes(w, h, s, seed=seed, **kw)
    p.setflags(write=False)
    return p


def colours_of(planes):
    return np.ascontiguousarray(planes[2:5], np.float64)


_oracle_pass = {}


def oracle_report(oracle, key, kw, sigma_seed, gains=None):
    """(row records, their fold) of the restatement on the oracle's pass over frame(**kw): computed once, shared, never modified"""
    if key not in _oracle_pass:
        planes = frame(**kw)
        if gains is None:
            want = oracle.filter_pass(planes, oracle.make_desc(W, H, S, box=BOX, policy=EPS, sigma_seed=sigma_seed))
        else:
            want = SRf.scheduled_pass(oracle, planes, (sigma_seed,) + gains, BOX)
        rr = PR.rows(colours_of(planes), want["colour"], want["nbhd_size"], want["alpha"], want["beta"], want["wrc"])
        _oracle_pass[key] = (rr, PR.fold(rr))
    return _oracle_pass[key]


# ---- the flag and the bindings ------------------------------------------------------------------------------------------------
def header_text():
    with open(os.path.join(ROOT, "include", "rpf_hip.h")) as f:
        return f.read()


def test_flag_value_and_family(hipmod):
    m = re.search(r"RPF_FLAG_PASS_REPORT\s*=\s*(\d+)", header_text())
    assert m and int(m.group(1)) == hipmod.PASS_REPORT_FLAG == 32768
    bits = {n: getattr(hipmod, n) for n in dir(hipmod) if (n.startswith("FLAG_") or n.endswith("_FLAG")) and n != "PASS_REPORT_FLAG"}
    assert all(v & hipmod.PASS_REPORT_FLAG == 0 for v in bits.values()), bits          # a bit of its own
    assert not any(n.startswith("FLAG_") and v == 32768 for n, v in bits.items())
    others = [int(v) for v in re.findall(r"RPF_FLAG_[A-Z_]+\s*=\s*(\d+)", header_text())]
    assert others.count(32768) == 1 and sum(others) == sum(set(others))                # ... in the header as well
    assert int(re.search(r"#define RPF_REPORT_NCLASS (\d+)", header_text()).group(1)) == hipmod.REPORT_NCLASS == len(PR.CAPS) + 1


def test_struct_sizes_and_offsets_match_the_header(hipmod, tmp_path):
    row = [n for n, _ in hipmod.ReportRow._fields_]
    rep = [n for n, _ in hipmod.PassReport._fields_]
    src = ["#include <cstdio>", "#include <cstddef>", '#include "rpf_hip.h"', "int main() {",
           '  std::printf("%zu %zu\\n", sizeof(rpf_report_row), sizeof(rpf_pass_report));']
    src += ['  std::printf("row.%s %%zu %%zu\\n", offsetof(rpf_report_row, %s), sizeof(((rpf_report_row *)0)->%s));' % (n, n, n) for n in row]
    src += ['  std::printf("rep.%s %%zu %%zu\\n", offsetof(rpf_pass_report, %s), sizeof(((rpf_pass_report *)0)->%s));' % (n, n, n) for n in rep]
    src += ["  return 0;", "}"]
    cpp, exe = tmp_path / "offsets.cpp", tmp_path / "offsets"
    cpp.write_text("\n".join(src))
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(cpp)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    assert [int(v) for v in lines[0].split()] == [C.sizeof(hipmod.ReportRow), C.sizeof(hipmod.PassReport)] == [920, 960]
    seen = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in lines[1:] if ln}
    for n in row:
        f = getattr(hipmod.ReportRow, n)
        assert seen["row." + n] == (f.offset, f.size), n
    for n in rep:
        f = getattr(hipmod.PassReport, n)
        assert seen["rep." + n] == (f.offset, f.size), n
    assert len(seen) == len(row) + len(rep)
    assert hipmod.ReportRow.sum_nbhd.offset == 448 and hipmod.ReportRow.min_nbhd.offset == 912 and hipmod.PassReport.total.offset == 40


def test_exports_and_methods(hipmod):
    for sym in ("rpf_query_pass_report", "rpf_query_pass_report_rows", "rpf_multi_query_pass_report", "rpf_pass_report_rows_device",
                "rpf_pass_report_fold"):
        assert sym in hipmod.EXPORTS and hasattr(hipmod.load(), sym), sym
    for name in ("pass_report", "pass_report_rows", "pass_report_rows_device"):
        assert callable(getattr(hipmod.Context, name)), name
    assert callable(hipmod.MultiContext.pass_report) and callable(hipmod.pass_report_fold)


def test_the_flag_changes_no_answer_that_needs_no_device(hipmod):
    F = hipmod.PASS_REPORT_FLAG
    words = [0, hipmod.FLAG_GENERIC, hipmod.FLAG_GENERIC | hipmod.FLAG_GENERIC_PACKED, hipmod.FLAG_WIDE_NBHD, hipmod.FLAG_FAST_WEIGHTS,
             hipmod.FLAG_GENERIC_PACKED, hipmod.FLAG_GENERIC | hipmod.FLAG_STREAM_FAST, hipmod.MEMBER_TEST_FLAG, hipmod.SAMPLED_NBHD_FLAG,
             hipmod.SAMPLED_NBHD_FLAG | hipmod.SAMPLED_REST_FLAG, hipmod.SAMPLED_REST_FLAG, hipmod.FLAG_GENERIC | hipmod.FLAG_FAST_WEIGHTS]
    for w in words:
        for lay in (dict(), dict(n_random=3, n_feat=7)):
            a, b = hipmod.make_desc(12, 10, 8, flags=w, **lay), hipmod.make_desc(12, 10, 8, flags=w | F, **lay)
            assert hipmod.layout_kernels(a) == hipmod.layout_kernels(b), (w, lay)
            assert hipmod.max_nbhd(a) == hipmod.max_nbhd(b) and hipmod.max_draws(a) == hipmod.max_draws(b), (w, lay)


def test_slabs_refuse_the_flag(hipmod):
    with pytest.raises(NotImplementedError) as e:
        slabs.check_desc(hipmod.make_desc(12, 10, 8, flags=hipmod.PASS_REPORT_FLAG))
    assert "PASS_REPORT_FLAG" in str(e.value) and "pass_report_fold" in str(e.value)
    assert slabs.check_desc(hipmod.make_desc(12, 10, 8)) is not None


def test_queries_refuse_a_null_context(hipmod):
    L = hipmod.load()
    r, row = hipmod.PassReport(), hipmod.ReportRow()
    assert L.rpf_query_pass_report(None, 0, C.byref(r)) == hipmod.E_BADARG
    assert L.rpf_query_pass_report_rows(None, 0, C.byref(row), 1) == hipmod.E_BADARG
    assert L.rpf_multi_query_pass_report(None, 0, C.byref(r)) == hipmod.E_BADARG


# ---- the fold -------------------------------------------------------------------------------------------------------------------
def random_records(n, seed):
    rng = np.random.default_rng(seed)
    recs = []
    for _ in range(n):
        r = {}
        for k in PR.DOUBLES:
            shape = () if k == "wrc_sum" else (PR.MAX_NDIM if k == "beta_sum" else 3)
            r[k] = np.asarray(rng.standard_normal(shape) * 10.0 ** rng.integers(-8, 9, shape))
        for k in PR.COUNTS:
            shape = {"class_pixels": 9, "alpha_zero": 3, "beta_zero": PR.MAX_NDIM}.get(k, ())
            r[k] = np.asarray(rng.integers(0, 1 << 40, shape), np.int64)
        r["min_nbhd"], r["max_nbhd"] = np.int64(rng.integers(1, 500)), np.int64(rng.integers(500, 70000))
        recs.append(r)
    return recs


@pytest.mark.parametrize("n", [1, 2, 7, 24])
def test_fold_equals_the_restatement_bit_for_bit(hipmod, n):
    recs = random_records(n, 100 + n)
    got = PR.of_ctypes(hipmod.pass_report_fold([PR.to_ctypes(hipmod, r) for r in recs]))
    assert PR.differing(got, PR.fold(recs)) == []
    if n == 1:
        assert PR.differing(got, recs[0]) == []
    if n > 2:   # a chain, not a tree and not a reversed chain
        assert PR.differing(got, PR.fold(recs[::-1])) != []


def test_fold_keeps_negative_zero_sums(hipmod):
    recs = random_records(3, 5)
    for r in recs:
        r["alpha_sum"] = np.array([-0.0, -0.0, 0.0])
    recs[1]["alpha_sum"] = np.array([-0.0, 0.0, 0.0])
    got = PR.of_ctypes(hipmod.pass_report_fold([PR.to_ctypes(hipmod, r) for r in recs]))
    assert PR.differing(got, PR.fold(recs)) == []
    assert np.signbit(got["alpha_sum"]).tolist() == [True, False, False]               # -0 + -0 = -0; -0 + +0 = +0
    one = PR.of_ctypes(hipmod.pass_report_fold([PR.to_ctypes(hipmod, recs[0])]))
    assert np.signbit(one["alpha_sum"]).tolist() == [True, True, False]


def test_fold_refusals(hipmod):
    L = hipmod.load()
    rows, out = (hipmod.ReportRow * 2)(), hipmod.ReportRow()
    assert L.rpf_pass_report_fold(None, 2, C.byref(out)) == hipmod.E_BADARG
    assert L.rpf_pass_report_fold(rows, 2, None) == hipmod.E_BADARG
    assert L.rpf_pass_report_fold(rows, 0, C.byref(out)) == hipmod.E_BADARG
    assert L.rpf_pass_report_fold(rows, -1, C.byref(out)) == hipmod.E_BADARG
    assert L.rpf_pass_report_fold(rows, 2, C.byref(out)) == hipmod.OK
    for bad in (None, []):
        with pytest.raises(hipmod.RpfError) as e:
            hipmod.pass_report_fold(bad)
        assert e.value.status == hipmod.E_BADARG


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------
def test_restatement_on_a_hand_made_frame():
    a = np.zeros((3, 1, 2, 2))
    b = np.zeros((3, 1, 2, 2))
    a[:, 0, 0] = [[1.0, 2.0], [0.5, 0.25], [3.0, -1.0]]
    b[:, 0, 0] = [[1.0, 4.0], [0.5, 0.25], [3.0, -1.0]]                                 # sample 1 moves on channel 0 by 2
    a[:, 0, 1] = 1.0
    b[:, 0, 1] = 1.0
    b[1, 0, 1, 0] = np.inf                                                             # pixel 1 is bad: one bad sample
    alpha = np.array([[[0.0, 0.5, np.nan], [-0.0, 0.25, 1.0]]])
    rr = PR.rows(a, b, np.array([[2, 9]]), alpha, None, np.array([[0.5, np.inf]]))
    assert len(rr) == 1
    r = rr[0]
    assert r["moved2"].tolist() == [4.0, 0.0, 0.0] and r["in2"].tolist() == [5.0, 0.3125, 10.0]
    assert r["pix_moved2"].tolist() == [4.0, 0.0, 0.0] and r["pix_in2"].tolist() == [9.0, 0.5625, 4.0]
    assert (r["unchanged_samples"], r["nonfinite_samples"], r["nonfinite_pixels"]) == (2, 1, 1)
    assert r["alpha_sum"].tolist() == [0.0, 0.75, 1.0] and r["alpha_zero"].tolist() == [2, 0, 0] and r["weights_nonfinite"] == 2
    assert r["wrc_sum"] == 0.5 and not r["beta_sum"].any() and not r["beta_zero"].any()
    assert (r["sum_nbhd"], r["min_nbhd"], r["max_nbhd"], r["own_only_pixels"]) == (11, 2, 9, 1)
    assert r["class_pixels"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert PR.differing(PR.fold(rr), r) == []


def test_class_bounds():
    n = np.array([[1, 8, 9, 16, 17, 64, 65, 448, 449, 832, 833, 70000]])
    z = np.zeros((3, 1, n.size, 1))
    r = PR.rows(z, z, n, None, None, None)[0]
    assert r["class_pixels"].tolist() == [2, 2, 1, 1, 1, 0, 1, 2, 2] and r["own_only_pixels"] == 1


# ---- the coverage of the frames the GPU file uses -----------------------------------------------------------------------------------
def test_identity_frame(oracle):
    rr, t = oracle_report(oracle, "identity", IDENTITY[0], IDENTITY[1])
    assert t["unchanged_samples"] == W * H * S and not t["moved2"].any() and not t["pix_moved2"].any()
    assert (t["in2"] > 0).all() and t["nonfinite_samples"] == 0 and t["weights_nonfinite"] == 0


def test_active_frame(oracle):
    rr, t = oracle_report(oracle, "active", ACTIVE[0], ACTIVE[1])
    print("PASS REPORT active frame: unchanged %d of %d, relative L2 moved %.3e" % (t["unchanged_samples"], W * H * S, PR.moved_rel_l2(t)))
    assert 0 < t["unchanged_samples"] < W * H * S and (t["moved2"] > 0).all() and (t["pix_moved2"] > 0).all()
    rr5, t5 = oracle_report(oracle, "active .5", CLUSTERED, 0.5)                        # the seed of the other suites: everything moves
    assert t5["unchanged_samples"] == 0 and (t5["moved2"] > t["moved2"]).all()
    assert len({r["moved2"].tobytes() for r in rr}) == H                                # the rows differ: the fold's order matters


def test_scheduled_frame_clamps_some_alpha(oracle):
    rr, t = oracle_report(oracle, "scheduled", FLAT, 0.5, SCHED_GAINS)
    share = t["alpha_zero"] / (W * H)
    print("PASS REPORT scheduled frame: clamped alpha share", share)
    assert ((share > 0) & (share < 1)).all()
    _, plain = oracle_report(oracle, "flat", FLAT, 0.5)
    assert plain["alpha_zero"].tolist() != t["alpha_zero"].tolist()


def test_own_only_frame(oracle):
    _, t = oracle_report(oracle, "flat", FLAT, 0.5)
    assert 0 < t["own_only_pixels"] < W * H and t["class_pixels"][0] == t["own_only_pixels"] and t["class_pixels"].sum() == W * H
    assert t["min_nbhd"] == S and t["max_nbhd"] > 64
