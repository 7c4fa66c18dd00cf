"""GPU tests of the row-band host pipeline: rpf_filter from page-locked buffers cuts the first and the last pass of a call into
row bands, one route_pass per band, while the next band uploads and the previous one downloads.  include/rpf_hip.h promises that
such a call equals the serial one (RPF_FLAG_NO_OVERLAP, or any pageable buffer) bit for bit.  Every case of tests/host_bands.py --
at least three bands each, on every route, both plane types, both policies, non-finite inputs and every per-pass table -- runs
both ways on contexts of their own and is held to that promise, to the documented launch rule applied per band, and to the
independent reference of the case (the oracle's chain, or the numpy restatement of the flag) at the bar of tests/test_gpu_parity.py.
tests/test_host_bands_cpu.py holds the conditions that make each case able to fail."""
import numpy as np
import pytest

import host_bands as HB
from host_bands import CASES, REF_ABORT
from test_gpu_parity import REL_L2_BAR, rel_l2

pytestmark = pytest.mark.gpu

COUNTERS = ("samples_filtered", "sum_nbhd", "nonfinite_pixels", "max_nbhd", "first_bad_pixel", "filter_kernel_launches",
            "options_active", "redo_pixels")     # every field of rpf_counters that is not a time
COMPILED = (0, 1, 2)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def configure(c, hipmod, name):
    """the options and tables of a case on a context; the two options a case may set go back to their defaults first"""
    case = CASES[name]
    for k, v in (("wide", -1), ("wide_pool", -1)) + case.options:
        c.set_option(k, v)
    if case.draws is not None:
        c.set_sampling(hipmod.make_sampling(HB.SAMPLING_SEED, case.draws))
    if case.membership is not None:
        c.set_membership(hipmod.membership_preset(hipmod.MEMBERSHIP_PUBLISHED_19))
    if case.schedule is not None:
        c.set_schedule(hipmod.make_schedule(**case.schedule))


def desc_of(hipmod, name, banded):
    case = CASES[name]
    W, H, S = case.shape
    nr, nf, dt = case.lay
    r0, r1 = case.rows if case.rows else (0, H)
    return hipmod.make_desc(W, H, S, boxes=case.boxes, row_begin=r0, row_end=r1, policy=case.policy, sigma_seed=case.sigma_seed,
                            flags=case.flags | (0 if banded else hipmod.FLAG_NO_OVERLAP), n_random=nr, n_feat=nf,
                            plane_dtype=hipmod.PLANES_F16 if dt == "f16" else hipmod.PLANES_F32)


def run(c, hipmod, name, banded):
    """one rpf_filter call of a case on c.  banded: planes, ray weights and both outputs page-locked (one pageable pointer selects
    the serial path); else pageable arrays under RPF_FLAG_NO_OVERLAP"""
    case = CASES[name]
    W, H, S = case.shape
    planes, rw = HB.planes_of(name), HB.ray_weight_of(name)
    desc = desc_of(hipmod, name, banded)
    if banded:
        pin, pin_rw = c.host_empty(planes.shape, planes.dtype), c.host_empty(rw.shape)
        pin[...], pin_rw[...] = planes, rw
        out_s, out_p = c.host_empty((3, H, W, S)), c.host_empty((H, W, 3))
        out_s[...], out_p[...] = -1.0, -1.0
        _, _, st = c.filter(pin, desc, ray_weight=pin_rw, out_samples=out_s, out_pixels=out_p, allow_nonfinite=True)
        srgb, prgb = np.array(out_s), np.array(out_p)
    else:
        srgb, prgb, st = c.filter(planes, desc, ray_weight=rw, allow_nonfinite=True)
    cn = c.counters()
    got = dict(sample_rgb=srgb, pixel_rgb=prgb, status=st, nbhd=c.nbhd(W, H), route=c.route())
    got.update((k, getattr(cn, k)) for k in COUNTERS)
    for k in ("sample_rgb", "pixel_rgb", "nbhd"):
        got[k].setflags(write=False)
    return got


@pytest.fixture(scope="module")
def fresh(hipmod):
    """(serial, banded) of a case, each on a context that has run nothing else: computed once, shared, never modified"""
    done = {}

    def get(name):
        if name not in done:
            pair = []
            for banded in (False, True):
                with hipmod.Context(0) as c:
                    configure(c, hipmod, name)
                    pair.append(run(c, hipmod, name, banded))
            done[name] = tuple(pair)
        return done[name]
    return get


def assert_same_call(got, want, rows, tag, route=True):
    """bit for bit: the colours and the N map of the slab; equal: the status, the route and every counter that is not a time (the
    launches: the callers)"""
    for k in ("sample_rgb", "pixel_rgb"):
        assert same(got[k], want[k]), (tag, k, int((got[k] != want[k]).sum()))
    assert same(got["nbhd"][rows[0]:rows[1]], want["nbhd"][rows[0]:rows[1]]), (tag, "nbhd")
    for k in ("status",) + (("route",) if route else ()) + COUNTERS:
        if k != "filter_kernel_launches":
            assert got[k] == want[k], (tag, k, got[k], want[k])


@pytest.mark.parametrize("name", list(CASES))
def test_banded_call(hipmod, oracle, fresh, name):
    """One case, serial and banded, against each other and against the reference.

    The route of fused19-nan: with option "count_first" at -1 a probe picks between routes 0 (fused) and 1 (count first).  A band
    that probed its own rows alone chose 0 in the last band where the serial call chooses 1 (same colours, other route); the band
    pipeline now has every band probe the rows of the slab that are resident, the last band of a pass the whole slab, so
    rpf_query_route answers as after the serial call."""
    case = CASES[name]
    W, H, S = case.shape
    r0, r1 = case.rows if case.rows else (0, H)
    serial, banded = fresh(name)
    ref, cut = HB.reference(oracle, name), HB.cut_of(name)
    want_launches = HB.expected_launches(case.routes, ref["nbhd"], cut, case.policy, case.rows)
    want_serial = HB.expected_launches(case.routes, ref["nbhd"], [(0, H)], case.policy, case.rows)
    fin = np.isfinite(ref["colour"])
    rel = rel_l2(banded["sample_rgb"].astype(np.float64)[fin], ref["colour"][fin])
    print("BANDS %s: routes %s (last pass as run: %d), %d bands, launches %d banded / %d serial (rule: %s / %s), redo %d / %d, "
          "rel-L2 %.3e (bar %.1e)" % (name, list(case.routes), banded["route"], len(cut), banded["filter_kernel_launches"],
                                      serial["filter_kernel_launches"], want_launches, want_serial, banded["redo_pixels"],
                                      serial["redo_pixels"], rel, REL_L2_BAR))
    # the routes: as the case says, on both calls
    for got in (serial, banded):
        assert got["route"] in COMPILED if case.routes[-1] == 0 else got["route"] == case.routes[-1]
        assert got["options_active"] == int(bool(case.options))
    # the bands ran
    if want_launches is not None:
        assert serial["filter_kernel_launches"] == want_serial          # the documented rule, once per pass
        assert banded["filter_kernel_launches"] == want_launches        # ... and once per band of the first and the last pass
        assert want_launches > want_serial
    else:
        assert banded["filter_kernel_launches"] > serial["filter_kernel_launches"]
    # the banded call is the serial call
    assert_same_call(banded, serial, (r0, r1), name, route=False)     # (the route: below, last)
    assert (banded["sample_rgb"] != -1.0).all() and (banded["pixel_rgb"] != -1.0).all()          # every band came back
    # ... and the reference's
    assert np.array_equal(banded["nbhd"][r0:r1], ref["nbhd"][-1][r0:r1])
    assert (banded["status"] == hipmod.E_NONFINITE) == (ref["status"] == 1) and banded["status"] in (hipmod.OK, hipmod.E_NONFINITE)
    assert np.array_equal(np.isnan(banded["sample_rgb"]), np.isnan(ref["colour"]))
    assert fin.any() and rel <= REL_L2_BAR
    assert banded["samples_filtered"] == (r1 - r0) * W * S * len(case.boxes)
    assert banded["sum_nbhd"] == int(ref["nbhd"][-1][r0:r1].sum()) and banded["max_nbhd"] == int(ref["nbhd"][-1][r0:r1].max())
    assert banded["redo_pixels"] == ref["redo_pixels"]
    assert banded["nonfinite_pixels"] == ref["nonfinite_pixels"] and banded["first_bad_pixel"] == ref["first_bad_pixel"]
    if fin.all():
        want_pix = oracle.pixel_mean(ref["colour"], oracle.make_desc(W, H, S), HB.ray_weight_of(name))
        assert rel_l2(banded["pixel_rgb"].astype(np.float64), want_pix) <= REL_L2_BAR
    if case.rows:   # rows outside the slab come back as the input colours
        cin = HB.p32_of(name)[2:5]
        assert np.array_equal(banded["sample_rgb"][:, :r0], cin[:, :r0]) and np.array_equal(banded["sample_rgb"][:, r1:], cin[:, r1:])
    # the route of the last pass, as rpf_query_route names it
    assert banded["route"] == serial["route"], (name, "route", banded["route"], serial["route"])


def test_banded_then_serial_then_banded_on_one_context(hipmod, fresh):
    """the grow-only buffers, the band events and the member pool of one context through calls of other shapes, routes and
    policies: every call returns what a context of its own returns"""
    with hipmod.Context(0) as c:
        for i, (name, banded) in enumerate((("g5", True), ("fused19-ra", False), ("wide7-hook", True), ("g5", True))):
            configure(c, hipmod, name)
            got = run(c, hipmod, name, banded)
            want = fresh(name)[1 if banded else 0]
            assert_same_call(got, want, (0, CASES[name].shape[1]), (i, name))
            assert got["filter_kernel_launches"] == want["filter_kernel_launches"], (i, name)


def test_multi_counters_after_the_fix(hipmod, oracle, fresh):
    """rpf_multi_query_counters adds up what the slabs report: with every slab's count that of its own last pass, the sum is the
    one-context call's"""
    name = "g5-ra"
    serial = fresh(name)[0]
    with hipmod.MultiContext([0, 0]) as mc:
        srgb, prgb, st = mc.filter(HB.planes_of(name), desc_of(hipmod, name, True), ray_weight=HB.ray_weight_of(name), allow_nonfinite=True)
        cn = mc.counters()
    assert st == serial["status"] and same(srgb, serial["sample_rgb"]) and same(prgb, serial["pixel_rgb"])
    assert cn.redo_pixels == serial["redo_pixels"] == HB.reference(oracle, name)["redo_pixels"] > 0
    assert CASES[name].policy == REF_ABORT
