"""GPU tests of the state one listed-member pass leaves in a context for the next (routes 7, 8 and 9 share one count-and-deal step:
the member pool and its capacity, the cursor and its NaN-flag slot, the class lists, the redo list, the membership table and the
sampled pass in progress).  One context runs route 7, 8, 9, 7 under REF_ABORT, 8 under the membership test, 9 and 7 again on the
planted frame of tests/test_listed_routes_cpu.py; every pass must return what the same pass returns on a fresh context, bit for
bit, and the same once more with option "wide_pool" = 1, which sends every pass through the repeat at the pool's exact size."""
import numpy as np
import pytest

import test_listed_routes_cpu as F

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = F.EPS, F.REF_ABORT
# (what the pass is, policy) in the order one context runs them; "8m": a sampled pass whose draws meet the membership test
SEQUENCE = (("7", EPS), ("8", EPS), ("9", EPS), ("7", REF_ABORT), ("8m", EPS), ("9", EPS), ("7", EPS))
ROUTE = {"7": 7, "8": 8, "9": 9, "8m": 8}
ARRAYS = ("colour", "nbhd_size", "member_hash", "bin_hash", "mean", "stddev", "mi", "alpha", "beta", "wrc")
SCALARS = ("status", "route", "launches", "redo_pixels", "sum_nbhd", "max_nbhd")


def new_context(hipmod, wide_pool=None):
    """a context with option wide = 1 and both configurations set once, up front: the flags of a pass pick what it reads"""
    c = hipmod.Context(0)
    c.set_option("wide", 1)
    if wide_pool is not None:
        c.set_option("wide_pool", wide_pool)
    c.set_sampling(hipmod.make_sampling(F.SAMPLING[0], [F.SAMPLING[2]], row_origin=F.SAMPLING[1]))
    c.set_membership(hipmod.membership_preset(hipmod.MEMBERSHIP_REFERENCE))      # multiples 3, floors -1
    return c


def run(c, hipmod, kind, policy):
    planes, _ = F.frame()
    _, H, W, S = planes.shape
    flags = {"7": hipmod.FLAG_WIDE_NBHD | hipmod.FLAG_WIDE_CLASSES, "8": hipmod.SAMPLED_NBHD_FLAG, "9": hipmod.MEMBER_TEST_FLAG,
             "8m": hipmod.SAMPLED_NBHD_FLAG | hipmod.MEMBER_TEST_FLAG}[kind]
    desc = hipmod.make_desc(W, H, S, policy=policy, sigma_seed=F.P.ACTIVE_SIGMA_SEED, flags=flags)
    got = c.filter_pass_debug(planes, desc, box=F.BOX, allow_nonfinite=policy == REF_ABORT)
    cn = c.counters()
    got.update(route=c.route(), launches=cn.filter_kernel_launches, redo_pixels=cn.redo_pixels)
    return got


def run_sequence(hipmod, wide_pool=None):
    c = new_context(hipmod, wide_pool)
    try:
        out = [run(c, hipmod, kind, policy) for kind, policy in SEQUENCE]
        assert c.counters().options_active == 1
    finally:
        c.close()
    return out


@pytest.fixture(scope="module")
def fresh(hipmod):
    """every distinct pass of the sequence on a context of its own: computed once, shared, never modified"""
    out = {}
    for step in dict.fromkeys(SEQUENCE):
        c = new_context(hipmod)
        try:
            out[step] = run(c, hipmod, *step)
        finally:
            c.close()
    return out


@pytest.fixture(scope="module")
def sequence(hipmod):
    return run_sequence(hipmod)


def assert_same_pass(got, want, what):
    for k in SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ARRAYS:   # bytes: no tolerance, and a NaN equals a NaN of the same bits only
        assert got[k].shape == want[k].shape and np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)


def test_every_pass_of_the_sequence_equals_a_fresh_context(sequence, fresh):
    for i, step in enumerate(SEQUENCE):
        assert_same_pass(sequence[i], fresh[step], (i, step))


def test_wide_pool_1_repeats_every_count_and_gives_the_same_bits(hipmod, sequence):
    pooled = run_sequence(hipmod, wide_pool=1)
    for i, step in enumerate(SEQUENCE):
        assert_same_pass(pooled[i], sequence[i], (i, step))


def test_planted_sizes_routes_and_launch_counts(hipmod, oracle, fresh):
    _, pixels = F.frame()
    full, sampled = F.full_box(oracle, EPS)["nbhd_size"], F.sampled(oracle)["nbhd_size"]
    for (kind, policy), got in fresh.items():
        n = got["nbhd_size"]
        at_targets = [int(n[y, x]) for y, x in pixels]
        print("LISTED %s policy %d: route %d, %d launches, redo %d, status %d" % (kind, policy, got["route"], got["launches"],
                                                                                   got["redo_pixels"], got["status"]))
        assert got["route"] == ROUTE[kind]
        if kind in ("7", "9"):
            assert at_targets == list(F.TARGETS) and np.array_equal(n, full)
            # eight classes and the rest list (F: every one is filled); REF_ABORT: the wide kernel's redo launch on top
            assert got["launches"] == (10 if policy == REF_ABORT else 9)
            assert (got["sum_nbhd"], got["max_nbhd"]) == (int(full.sum()), int(full.max()))
        else:
            assert (n <= full).all() and at_targets == [int(sampled[y, x]) for y, x in pixels]
            assert np.array_equal(n, sampled) and got["launches"] == 8      # eight classes, no rest list, no redo
        if policy == EPS:
            assert got["status"] == hipmod.OK and got["redo_pixels"] == 0
