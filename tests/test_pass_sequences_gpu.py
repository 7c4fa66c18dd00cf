"""GPU tests of box lists that return to an earlier box (tests/test_pass_sequences_cpu.py holds the table, the frames and the
conditions that make each sequence able to fail).  A context keeps state for a whole call -- the size-binned route's membership
cache, the class lists, masks and counts, the member pool and its cursor, the redo list, the uploaded tables -- and a later pass
of a call must not meet what an earlier pass of another route left in it.

The yardstick is the chain: pass p of the list alone, boxes = (box_p,), on a context of its own that has run nothing else, fed the
fp64 colours the previous link returned; the sampling table enters at pass_id0 = p, the schedule at pass0 = p, the spike flag on
the last link only.  One call with the whole list must return the last link's colours byte for byte (a NaN equals a NaN of the
same bits only), its status, its route, and counters that add up.  The unflagged sequences are also held to the chain of oracle
passes at the bar of tests/test_gpu_parity.py; the flagged passes are held to their restatements one pass at a time elsewhere.

Counters: samples_filtered and filter_kernel_launches accumulate over the passes of a call, so the call's are the sums over the
chain.  sum_nbhd, max_nbhd and redo_pixels are those of the LAST pass of a call (include/rpf_hip.h, rpf_counters: "sum over
filtered pixels of N, last pass"; "RPF_DEGEN_REF_ABORT, last pass"): the call's equal the last link's, not a sum over the chain."""
import numpy as np
import pytest

import test_pass_sequences_cpu as T
from test_gpu_parity import REL_L2_BAR, rel_l2

pytestmark = pytest.mark.gpu

EPS, REF_ABORT = T.EPS, T.REF_ABORT
SPIKE_FIELDS = ("spike_samples", "spike_pixels", "skipped_pixels", "applied")
# the route of every pass of every sequence, as rpf_query_route names them (0 / 1: the unbinned route, fused or count first)
UNBINNED = (0, 1)
ROUTES = {"aba16": (2, UNBINNED, 2), "aba8": (2, UNBINNED, 2), "aabab16": (2, 2, UNBINNED, 2, 2), "bab8": (UNBINNED, 2, UNBINNED),
          "s-bin": (8, 2, 8, 2), "s-gpw": (5, 8, 5), "s-mem": (8, 9, 8), "w-back": (7, 7, 7), "pipeline": (8, 8, 9, 9)}


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def configure(c, hipmod, name, options=(), p=None):
    """the options and tables of a sequence on a Context or MultiContext: for the whole list (p None) or for pass p alone"""
    s = T.SEQUENCES[name]
    for k, v in options:
        c.set_option(k, v)
    if s.draws is not None:
        c.set_sampling(hipmod.make_sampling(T.SAMPLING_SEED, s.draws if p is None else [s.draws[p]], pass_id0=0 if p is None else p))
    if s.membership is not None:
        c.set_membership(hipmod.membership_preset(hipmod.MEMBERSHIP_PUBLISHED_19))
    if s.schedule is not None:
        c.set_schedule(hipmod.make_schedule(pass0=0 if p is None else p, **s.schedule))
    if s.spike:
        c.set_spike(1.0, True)


def desc_of(hipmod, name, policy, p=None):
    s = T.SEQUENCES[name]
    W, H, S = s.shape
    flags = s.flags
    if p is not None and p != len(s.boxes) - 1:
        flags &= ~hipmod.FLAG_SPIKE_CLAMP          # a caller who makes one call per pass sets it on the last call only
    return hipmod.make_desc(W, H, S, boxes=s.boxes if p is None else (s.boxes[p],), policy=policy, sigma_seed=s.sigma_seed, flags=flags)


def run(c, hipmod, name, policy, p=None, colour64_in=None):
    """one rpf_filter_ex call on c: the whole list, or pass p alone"""
    srgb, prgb, st, c64 = c.filter(T.planes_of(name), desc_of(hipmod, name, policy, p), colour64_in=colour64_in, want_colour64=True,
                                   allow_nonfinite=policy == REF_ABORT)
    cn, sp = c.counters(), c.spike_stats()
    return dict(colour64=c64, sample_rgb=srgb, pixel_rgb=prgb, status=st, route=c.route(), samples_filtered=cn.samples_filtered,
                sum_nbhd=cn.sum_nbhd, max_nbhd=cn.max_nbhd, launches=cn.filter_kernel_launches, redo_pixels=cn.redo_pixels,
                nonfinite_pixels=cn.nonfinite_pixels, options_active=cn.options_active,
                spike=tuple(getattr(sp, k) for k in SPIKE_FIELDS) + (tuple(sp.energy), tuple(sp.delta)))


@pytest.fixture(scope="module")
def cases(hipmod):
    """(the call, the chain) of a sequence under a variant, each on contexts of their own, one alive at a time: computed once per
    (name, variant), shared, never modified"""
    done = {}

    def get(name, label):
        if (name, label) not in done:
            policy, options = T.variant_of(name, label)
            with hipmod.Context(0) as c:
                configure(c, hipmod, name, options)
                call = run(c, hipmod, name, policy)
            chain, colour = [], None
            for p in range(len(T.SEQUENCES[name].boxes)):
                with hipmod.Context(0) as c:
                    configure(c, hipmod, name, options, p)
                    chain.append(run(c, hipmod, name, policy, p, colour))
                colour = chain[-1]["colour64"]
            for r in [call] + chain:
                for k in ("colour64", "sample_rgb", "pixel_rgb"):
                    r[k].setflags(write=False)
            done[name, label] = (call, chain)
        return done[name, label]
    return get


_oracle_chain = {}


def oracle_chain(oracle, name, policy):
    """the oracle's passes through the boxes, each fed the colours of the one before: computed once, shared"""
    if (name, policy) not in _oracle_chain:
        s = T.SEQUENCES[name]
        W, H, S = s.shape
        c, status = None, 0
        for box in s.boxes:
            r = oracle.filter_pass(T.planes_of(name), oracle.make_desc(W, H, S, box=box, policy=policy, sigma_seed=s.sigma_seed),
                                   colour_in=c, debug=False)
            c, status = r["colour"], max(status, int(r["status"]))
        _oracle_chain[name, policy] = (c, status)
    return _oracle_chain[name, policy]


# ---- one call against the chain --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,label", T.CASES)
def test_call_equals_the_chain_bit_for_bit(hipmod, cases, name, label):
    call, chain = cases(name, label)
    last = chain[-1]
    assert call["status"] == last["status"] and (call["status"] == hipmod.OK or T.variant_of(name, label)[0] == REF_ABORT)
    for k in ("colour64", "sample_rgb", "pixel_rgb"):
        assert same(call[k], last[k]), (k, int((call[k] != last[k]).sum()))
    assert not same(call["colour64"], chain[0]["colour64"])             # the later passes did something


@pytest.mark.parametrize("name,label", T.CASES)
def test_call_counters_and_routes_are_the_chains(hipmod, cases, name, label):
    call, chain = cases(name, label)
    s = T.SEQUENCES[name]
    W, H, S = s.shape
    options = T.variant_of(name, label)[1]
    routes = [r["route"] for r in chain]
    print("SEQUENCE %s/%s: routes %s, launches %s, sum N %s, max N %s, redo %s, status %d" % (
        name, label, routes, [r["launches"] for r in chain], [r["sum_nbhd"] for r in chain], [r["max_nbhd"] for r in chain],
        [r["redo_pixels"] for r in chain], call["status"]))
    for got, want in zip(routes, ROUTES[name]):
        assert got in want if isinstance(want, tuple) else got == want, (routes, ROUTES[name])
    if ("count_first", 0) in options or ("count_first", 1) in options:
        assert routes[1] == dict(options)["count_first"]
    assert len(routes) == len(ROUTES[name]) and call["route"] == chain[-1]["route"]
    assert call["samples_filtered"] == sum(r["samples_filtered"] for r in chain) == W * H * S * len(s.boxes)
    assert call["launches"] == sum(r["launches"] for r in chain)
    # the last pass's (include/rpf_hip.h, rpf_counters), not the chain's sums: see the module docstring
    assert call["sum_nbhd"] == chain[-1]["sum_nbhd"] and call["max_nbhd"] == chain[-1]["max_nbhd"]
    assert call["redo_pixels"] == chain[-1]["redo_pixels"]
    assert call["nonfinite_pixels"] >= chain[-1]["nonfinite_pixels"]    # (all passes of the call against the last link alone)
    assert call["options_active"] == chain[-1]["options_active"] == int(bool(options))
    assert call["spike"] == chain[-1]["spike"]
    if s.spike:
        assert call["spike"][3] == 1 and call["spike"][0] > 0 and all(r["spike"][3] == 0 for r in chain[:-1])
    else:
        assert call["spike"][3] == 0


@pytest.mark.parametrize("name,label", [(n, v) for n, v in T.CASES if n in T.COMPILED])
def test_unflagged_call_against_the_oracles_chain(hipmod, oracle, cases, name, label):
    call, _ = cases(name, label)
    policy = T.variant_of(name, label)[0]
    want, status = oracle_chain(oracle, name, policy)
    got, cin = call["sample_rgb"].astype(np.float64), T.planes_of(name)[2:5].astype(np.float64)
    assert (call["status"] == hipmod.E_NONFINITE) == (status == 1)
    fin = np.isfinite(want)
    if policy == REF_ABORT:
        assert np.array_equal(np.isnan(call["colour64"]), np.isnan(want))
    else:
        assert fin.all() and np.isfinite(call["colour64"]).all()
    r, r64, moved = rel_l2(got[fin], want[fin]), rel_l2(call["colour64"][fin], want[fin]), rel_l2(got[fin], cin[fin])
    print("SEQUENCE %s/%s: rel-L2 against the oracle's chain %.3e (fp64 colours %.3e; bar %.1e), moved %.3e, finite on %.3f" % (
        name, label, r, r64, REL_L2_BAR, moved, fin.mean()))
    assert r <= REL_L2_BAR and moved > 1e-3


# ---- one context, call after call ------------------------------------------------------------------------------------------------
def test_same_context_again_and_again(hipmod, cases):
    first = {n: cases(n, "eps")[0] for n in ("aba16", "aabab16")}
    with hipmod.Context(0) as c:
        for i, name in enumerate(("aba16", "aba16", "aabab16", "aba16")):
            configure(c, hipmod, name)
            got = run(c, hipmod, name, EPS)
            for k in ("colour64", "sample_rgb", "pixel_rgb"):
                assert same(got[k], first[name][k]), (i, name, k)
            for k in ("status", "route", "samples_filtered", "sum_nbhd", "max_nbhd", "launches", "redo_pixels"):
                assert got[k] == first[name][k], (i, name, k)


# ---- row slabs ---------------------------------------------------------------------------------------------------------------------
def need_devices(devices):
    import torch
    if max(devices) >= torch.cuda.device_count():
        pytest.skip("needs %d visible GPUs" % (max(devices) + 1))


@pytest.mark.parametrize("name,devices", [("aba16", (0, 0)), ("aba16", (0, 0, 0)), ("aba8", (0, 0)), ("pipeline", (0, 0)),
                                          ("aba16", (0, 1)), ("aba8", (0, 1)), ("pipeline", (0, 1))])
def test_multi_equals_one_context(hipmod, cases, name, devices):
    from raytracer_rpf_amd import slabs
    need_devices(devices)
    s = T.SEQUENCES[name]
    H, halo = s.shape[1], (max(s.boxes) - 1) // 2
    rows = [slabs.slab_for(H, len(devices), g, halo) for g in range(len(devices))]      # every slab owns at least the halo
    assert min(r.row1 - r.row0 for r in rows) >= halo
    want = cases(name, "eps")[0]
    with hipmod.MultiContext(list(devices)) as mc:
        configure(mc, hipmod, name)
        srgb, prgb, st = mc.filter(T.planes_of(name), desc_of(hipmod, name, EPS))
        cn, sp = mc.counters(), mc.spike_stats()
    assert st == want["status"] == hipmod.OK
    assert same(srgb, want["sample_rgb"]) and same(prgb, want["pixel_rgb"])
    for k in ("samples_filtered", "sum_nbhd", "max_nbhd", "redo_pixels", "nonfinite_pixels"):
        assert getattr(cn, k) == want[k], k
    assert cn.filter_kernel_launches >= want["launches"]                 # (per slab and class: no fewer than one context's)
    assert tuple(getattr(sp, k) for k in SPIKE_FIELDS) + (tuple(sp.energy), tuple(sp.delta)) == want["spike"]


@pytest.mark.parametrize("devices", [(0, 0), (0, 1)])
def test_film_step_behind_the_sequence(ctx, hipmod, cases, devices):
    need_devices(devices)
    name = "aba16"
    W, H, _ = T.SEQUENCES[name].shape
    film = hipmod.make_film(((0, 0), (W, H)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX, 0.5), sample_origin=(0, 0))
    desc = desc_of(hipmod, name, EPS)
    want = ctx.filter_film(T.planes_of(name), desc, film)
    with hipmod.MultiContext(list(devices)) as mc:
        got = mc.filter_film(T.planes_of(name), desc, film)
    assert same(want[0], cases(name, "eps")[0]["sample_rgb"])
    for g, w, what in zip(got, want, ("sample_rgb", "contribSum", "filterWeightSum", "image")):
        assert same(g, w), what
    assert (want[2] != 0).all() and np.isfinite(want[3]).all()
