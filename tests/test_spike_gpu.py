"""GPU tests of the spike pass (RPF_FLAG_SPIKE_CLAMP), bit for bit against the restatement
tests/spike_ref.py: the two device halves on every shape at which the kernels take another path, the flag end to end through
rpf_filter / _ex / _device / _film and rpf_multi_*, the refusals and the stats."""
import functools
import os

import numpy as np
import pytest

import spike_ref as R
from raytracer_rpf_amd import feature_buffer as fb

pytestmark = pytest.mark.gpu

F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def same_bits(a, b):
    """fp64 arrays equal bit for bit (-0.0 is not 0.0), a NaN matching a NaN"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a.view(np.uint64)[ok], b.view(np.uint64)[ok])


def counts(s):
    return dict(spike_samples=s.spike_samples, spike_pixels=s.spike_pixels, skipped_pixels=s.skipped_pixels)


def stats_tuple(s):
    return (s.applied, s.spike_samples, s.spike_pixels, s.skipped_pixels, tuple(np.array(s.energy).view(np.uint64)),
            tuple(np.array(s.delta).view(np.uint64)))


@functools.lru_cache(maxsize=None)
def halves_case(index, t, slab):
    W, H, S = R.SHAPES[index]
    c = R.make_frame(W, H, S, seed=index)
    rb, re = (1, H - 1) if slab else (0, H)
    return c, R.apply(c, t, True, rb, re), (rb, re)


HALVES = [(i, t, False) for i in range(len(R.SHAPES)) for t in R.THRESHOLDS] + \
         [(R.SHAPES.index(s), t, True) for s in R.SLAB_SHAPES for t in R.THRESHOLDS]


@pytest.mark.parametrize("index,t,slab", HALVES, ids=["%dx%dx%d-t%g%s" % (R.SHAPES[i] + (t, "-slab" if sl else "")) for i, t, sl in HALVES])
def test_the_two_halves_against_the_restatement(ctx, hipmod, index, t, slab):
    import torch
    W, H, S = R.SHAPES[index]
    c, ref, (rb, re) = halves_case(index, t, slab)
    dc = torch.from_numpy(c).to(torch.device("cuda", 0))
    stream = torch.cuda.current_stream().cuda_stream
    desc = hipmod.make_desc(W, H, S, row_begin=rb, row_end=re)
    rows, st = ctx.spike_clamp_device(desc, dc.data_ptr(), t, stream)
    torch.cuda.synchronize()
    got = dc.cpu().numpy()
    assert same_bits(got, ref["clamped"]), np.argwhere(got != ref["clamped"])[:5]
    assert same_bits(rows, ref["row_sums"])
    assert counts(st) == {k: ref[k] for k in ("spike_samples", "spike_pixels", "skipped_pixels")} and st.applied == 1
    E, delta = hipmod.spike_delta(rows, (re - rb) * W * S)
    assert same_bits(E, ref["energy"]) and same_bits(delta, ref["delta"])
    assert same_bits(np.array(st.energy), ref["energy"]) and same_bits(np.array(st.delta), ref["delta"])
    ctx.colour_add_device(desc, dc.data_ptr(), delta, stream)
    torch.cuda.synchronize()
    got = dc.cpu().numpy()
    assert same_bits(got, ref["colour"]), np.argwhere(got != ref["colour"])[:5]
    if slab:  # the rows outside keep their bits
        assert same_bits(got[:, :rb], c[:, :rb]) and same_bits(got[:, re:], c[:, re:])


def test_add_half_skips_an_all_zero_delta_and_keeps_minus_zero(ctx, hipmod):
    import torch
    c = np.full((3, 2, 3, 5), -0.0)
    dc = torch.from_numpy(c).to(torch.device("cuda", 0))
    desc = hipmod.make_desc(3, 2, 5)
    ctx.colour_add_device(desc, dc.data_ptr(), [0.0, -0.0, 0.0])
    torch.cuda.synchronize()
    assert same_bits(dc.cpu().numpy(), c)
    ctx.colour_add_device(desc, dc.data_ptr(), [0.0, 0.0, 2.0])  # one non-zero: all three channels are added
    torch.cuda.synchronize()
    assert same_bits(dc.cpu().numpy(), R.add(c, [0.0, 0.0, 2.0]))


def plant(planes, seed, frac=0.04):
    """fireflies in the input colours: a share of the samples multiplied by 1e3 on all three channels"""
    planes = np.array(planes)
    rng = np.random.default_rng(seed)
    hit = rng.random(planes.shape[1:]) < frac
    planes[2:5, hit] *= F(1e3)
    return planes


@functools.lru_cache(maxsize=None)
def golden_planes():
    planes, _ = fb.load_rpfb(os.path.join(GOLD, "clustered_10x8x8.rpfb"))
    return plant(planes, 7)


def device_reduce(ctx, hipmod, desc, c64):
    import torch
    dev = torch.device("cuda", 0)
    dc = torch.from_numpy(np.ascontiguousarray(c64)).to(dev)
    s = torch.empty((3, desc.H, desc.W, desc.S), dtype=torch.float32, device=dev)
    p = torch.empty((desc.H, desc.W, 3), dtype=torch.float32, device=dev)
    ctx.reduce_device(desc, dc.data_ptr(), None, s.data_ptr(), p.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return s.cpu().numpy(), p.cpu().numpy()


def end_to_end(ctx, hipmod, planes, boxes, flags=0, nonfinite=False, **lay):
    """nonfinite: the passes leave NaN colours (RPF_E_NONFINITE with and without the flag; the spike pass still runs, and
    flags nothing in a NaN pixel)"""
    import torch
    _, H, W, S = planes.shape
    off = hipmod.make_desc(W, H, S, boxes=boxes, flags=flags, **lay)
    on = hipmod.make_desc(W, H, S, boxes=boxes, flags=flags | hipmod.FLAG_SPIKE_CLAMP, **lay)
    want_status = hipmod.E_NONFINITE if nonfinite else hipmod.OK
    _, _, st0, raw = ctx.filter(planes, off, want_colour64=True, allow_nonfinite=nonfinite)
    assert st0 == want_status and ctx.spike_stats().applied == 0
    route, launches = ctx.route(), ctx.counters().filter_kernel_launches
    ref = R.apply(raw, 1.0)
    srgb, prgb, st1, c64 = ctx.filter(planes, on, want_colour64=True, allow_nonfinite=nonfinite)
    assert st1 == want_status
    st = ctx.spike_stats()
    assert same_bits(c64, ref["colour"]), np.argwhere(c64 != ref["colour"])[:5]
    if not nonfinite:
        assert ref["spike_samples"] > 0 and (ref["delta"] != 0).any()  # the frame has what the pass is for
        assert not same_bits(c64, raw)
    assert counts(st) == {k: ref[k] for k in ("spike_samples", "spike_pixels", "skipped_pixels")} and st.applied == 1
    assert same_bits(np.array(st.energy), ref["energy"]) and same_bits(np.array(st.delta), ref["delta"])
    assert (ctx.route(), ctx.counters().filter_kernel_launches) == (route, launches)  # the route answers as without the flag
    assert np.array_equal(srgb, c64.astype(F), equal_nan=True)
    s2, p2 = device_reduce(ctx, hipmod, on, c64)
    assert np.array_equal(srgb, s2, equal_nan=True) and np.array_equal(prgb, p2, equal_nan=True)
    # rpf_filter (no fp64 colours across the boundary): the same samples and pixel means
    s3, p3, _ = ctx.filter(planes, on, allow_nonfinite=nonfinite)
    assert np.array_equal(s3, srgb, equal_nan=True) and np.array_equal(p3, prgb, equal_nan=True)
    # ... and from page-locked buffers: the flag takes the serial path there (no band may leave before delta is known), so no
    # band pipeline runs in this test -- and these frames, below 32 rows, would be one band of it anyway
    pp, ps_, ppx = ctx.host_empty(planes.shape), ctx.host_empty(srgb.shape), ctx.host_empty(prgb.shape)
    pp[...] = planes
    ps_[...] = 0
    ppx[...] = 0
    ctx.filter(pp, on, out_samples=ps_, out_pixels=ppx, allow_nonfinite=nonfinite)
    assert np.array_equal(ps_, srgb, equal_nan=True) and np.array_equal(ppx, prgb, equal_nan=True)
    # rpf_filter_device: the same planes
    dev = torch.device("cuda", 0)
    dp = torch.from_numpy(np.ascontiguousarray(planes)).to(dev)
    dc = torch.empty((3, H, W, S), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    ctx.colour_from_planes_device(on, dp.data_ptr(), dc.data_ptr(), stream)
    assert ctx.filter_device(on, dp.data_ptr(), dc.data_ptr(), stream, allow_nonfinite=nonfinite) == want_status
    torch.cuda.synchronize()
    assert same_bits(dc.cpu().numpy(), c64)
    assert stats_tuple(ctx.spike_stats()) == stats_tuple(st)
    return raw, c64


@pytest.mark.parametrize("boxes", [(7,), (5, 3), (7, 5)])
def test_flag_end_to_end(ctx, hipmod, boxes):
    """colour64_out with the flag = the restatement applied to colour64_out without it: for two boxes that also says the pass
    ran once, at the end.  A box-3 pass has sigma_p = box / 4 = 0 (rpf.cpp:531, integer division) and leaves every colour NaN,
    as in the reference: (5, 3) is the case where RPF_E_NONFINITE comes back as before and the spike pass still runs; (7, 5) is
    the two-pass case with finite colours"""
    end_to_end(ctx, hipmod, golden_planes(), boxes, nonfinite=boxes[-1] == 3)


def test_flag_end_to_end_generic_layout(ctx, hipmod):
    planes = plant(fb.synth_planes(10, 8, 8, seed=61, mode="clustered", n_random=3, n_feat=5), 8)
    end_to_end(ctx, hipmod, planes, (7,), flags=hipmod.FLAG_GENERIC, n_random=3, n_feat=5)


def test_parameters_timing_and_one_call_per_pass(ctx, hipmod):
    planes = golden_planes()
    _, H, W, S = planes.shape
    off = hipmod.make_desc(W, H, S, boxes=(7, 5))
    _, _, _, raw = ctx.filter(planes, off, want_colour64=True)
    try:
        ctx.set_spike(2.5, False)
        on = hipmod.make_desc(W, H, S, boxes=(7, 5), flags=hipmod.FLAG_SPIKE_CLAMP | hipmod.FLAG_TIMING)
        _, _, _, c64 = ctx.filter(planes, on, want_colour64=True)
        ref = R.apply(raw, 2.5, preserve_energy=False)
        assert ref["spike_samples"] > 0
        assert same_bits(c64, ref["colour"])
        st = ctx.spike_stats()
        assert same_bits(np.array(st.delta), ref["delta"]) and st.spike_ms > 0
    finally:
        ctx.set_spike(1.0, True)
    # a caller who makes one call per pass sets the flag on the last call only
    _, _, _, c1 = ctx.filter(planes, hipmod.make_desc(W, H, S, boxes=(7,)), want_colour64=True)
    _, _, _, c2 = ctx.filter(planes, hipmod.make_desc(W, H, S, boxes=(5,), flags=hipmod.FLAG_SPIKE_CLAMP), colour64_in=c1, want_colour64=True)
    assert same_bits(c2, R.apply(raw, 1.0)["colour"])


def test_filter_film_with_the_flag(ctx, hipmod):
    """rpf_filter_film with the flag = film_splat_device on the restated colours, all three film outputs"""
    import torch
    W, H, S = 12, 9, 8
    planes = plant(fb.synth_planes(W, H, S, seed=50, mode="clustered"), 9)
    film = hipmod.make_film(((0, 0), (W, H)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX), sample_origin=(0, 0))
    rw = (0.5 + np.random.default_rng(4).random((H, W, S))).astype(F)
    _, _, _, raw = ctx.filter(planes, hipmod.make_desc(W, H, S), want_colour64=True)
    ref = R.apply(raw, 1.0)
    assert ref["spike_samples"] > 0 and (ref["delta"] != 0).any()
    on = hipmod.make_desc(W, H, S, flags=hipmod.FLAG_SPIKE_CLAMP)
    srgb, t, w, img = ctx.filter_film(planes, on, film, ray_weight=rw)
    assert np.array_equal(srgb, ref["colour"].astype(F))
    assert ctx.spike_stats().applied == 1 and ctx.spike_stats().spike_samples == ref["spike_samples"]
    dev = torch.device("cuda", 0)
    dp = torch.from_numpy(np.ascontiguousarray(planes)).to(dev)
    dc = torch.from_numpy(np.ascontiguousarray(ref["colour"])).to(dev)
    drw = torch.from_numpy(rw).to(dev)
    ny, nx = film.py1 - film.py0, film.px1 - film.px0
    outs = [torch.full(sh, float("nan"), dtype=torch.float32, device=dev) for sh in ((ny, nx, 3), (ny, nx), (ny, nx, 3))]
    ctx.film_splat_device(hipmod.make_desc(W, H, S), film, dp.data_ptr(), dc.data_ptr(), drw.data_ptr(), outs[0].data_ptr(),
                          outs[1].data_ptr(), outs[2].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for got, want in zip((t, w, img), outs):
        assert np.array_equal(got, want.cpu().numpy())
    # ... and not what the film step makes of the unclamped colours
    _, t0, _, _ = ctx.filter_film(planes, hipmod.make_desc(W, H, S), film, ray_weight=rw)
    assert not np.array_equal(t0, t) and ctx.spike_stats().applied == 0


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_multi_equals_one_context(ctx, hipmod, devices):
    """rpf_multi_filter and rpf_multi_filter_film on row slabs: samples, pixel means, film outputs and stats are those of one
    context, bit for bit (10 x 12 x 8, box 7: every slab owns at least 3 rows)"""
    W, H, S = 10, 12, 8
    planes = plant(fb.synth_planes(W, H, S, seed=70, mode="clustered"), 10)
    on = hipmod.make_desc(W, H, S, boxes=(7,), flags=hipmod.FLAG_SPIKE_CLAMP)
    film = hipmod.make_film(((0, 0), (W, H)), 0.5, hipmod.film_table(hipmod.PIXFILTER_BOX), sample_origin=(0, 0))
    srgb, prgb, _ = ctx.filter(planes, on)
    one = ctx.spike_stats()
    assert one.applied == 1 and one.spike_samples > 0 and any(d != 0 for d in one.delta)
    f1 = ctx.filter_film(planes, on, film)
    with hipmod.MultiContext(devices) as m:
        s2, p2, _ = m.filter(planes, on)
        assert np.array_equal(s2, srgb) and np.array_equal(p2, prgb)
        assert stats_tuple(m.spike_stats()) == stats_tuple(one)
        f2 = m.filter_film(planes, on, film)
        for a, b in zip(f1, f2):
            assert np.array_equal(a, b)
        assert stats_tuple(m.spike_stats()) == stats_tuple(one)
        m.filter(planes, hipmod.make_desc(W, H, S, boxes=(7,)))
        assert m.spike_stats().applied == 0
        with pytest.raises(hipmod.RpfError) as e:
            m.set_spike(-1.0, True)
        assert e.value.status == hipmod.E_BADARG
        m.set_spike(2.5, False)
        s3, _, _ = m.filter(planes, on)
    try:
        ctx.set_spike(2.5, False)
        s4, _, _ = ctx.filter(planes, on)
    finally:
        ctx.set_spike(1.0, True)
    assert np.array_equal(s3, s4) and not np.array_equal(s3, srgb)


def test_refusals_and_stats(ctx, hipmod):
    for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(hipmod.RpfError) as e:
            ctx.set_spike(bad, True)
        assert e.value.status == hipmod.E_BADARG
    for bad in (2, -1):
        with pytest.raises(hipmod.RpfError) as e:
            ctx.set_spike(1.0, bad)
        assert e.value.status == hipmod.E_BADARG
    planes = golden_planes()
    _, H, W, S = planes.shape
    with pytest.raises(hipmod.RpfError) as e:
        ctx.filter_pass_debug(planes, hipmod.make_desc(W, H, S, flags=hipmod.FLAG_SPIKE_CLAMP), box=7, debug=False)
    assert e.value.status == hipmod.E_UNSUPPORTED and "rpf_filter_pass_debug" in str(e.value)
    import torch
    dc = torch.zeros((3, H, W, S), dtype=torch.float64, device=torch.device("cuda", 0))
    with pytest.raises(hipmod.RpfError) as e:
        ctx.spike_clamp_device(hipmod.make_desc(W, H, S), dc.data_ptr(), 0.0)
    assert e.value.status == hipmod.E_BADARG
    # the parameters survived the refusals: the defaults still apply
    off, on = hipmod.make_desc(W, H, S), hipmod.make_desc(W, H, S, flags=hipmod.FLAG_SPIKE_CLAMP)
    assert hipmod.layout_kernels(off) == hipmod.layout_kernels(on) and hipmod.max_nbhd(off) == hipmod.max_nbhd(on)
    _, _, _, raw = ctx.filter(planes, off, want_colour64=True)
    st = ctx.spike_stats()
    assert stats_tuple(st) == (0, 0, 0, 0, (0, 0, 0), (0, 0, 0)) and st.spike_ms == 0
    c0 = ctx.counters()
    _, _, _, c64 = ctx.filter(planes, on, want_colour64=True)
    c1 = ctx.counters()
    assert ctx.spike_stats().applied == 1 and same_bits(c64, R.apply(raw, 1.0)["colour"])
    for f in ("samples_filtered", "sum_nbhd", "nonfinite_pixels", "max_nbhd", "first_bad_pixel", "filter_kernel_launches",
              "options_active", "redo_pixels"):
        assert getattr(c0, f) == getattr(c1, f), f


def test_host_mirror_passes_the_spike_keys_on(ctx, hipmod):
    """RPFFilter with spikeclamp: one FilterAndReduce call with the box list, and the reference's call shape -- one
    ApplyRPFFilter per box size, the flag on the last call only -- both give rpf_filter_ex's colours with the flag"""
    import ctypes as C
    lib = C.CDLL(os.path.join(os.path.dirname(hipmod.LIB_PATH), "librpf_host.so"))
    planes = golden_planes()
    _, H, W, S = planes.shape
    _, _, _, want = ctx.filter(planes, hipmod.make_desc(W, H, S, boxes=(7, 5), flags=hipmod.FLAG_SPIKE_CLAMP), want_colour64=True)
    assert ctx.spike_stats().spike_samples > 0
    boxes = (C.c_int32 * 2)(7, 5)
    for mode in (0x200, 0x200 | 0x100):
        aos = np.ascontiguousarray(fb.planes_to_aos(planes), np.float64)
        err = C.create_string_buffer(256)
        st = lib.rpf_host_apply_filter_aos(aos.ctypes.data_as(C.c_void_p), None, W, H, S, boxes, 2, mode, 0, 0, None, err, 256)
        assert st == 0, err.value
        got = np.transpose(aos[..., 2:5], (3, 1, 0, 2))  # [x][y][s][c] -> [c][y][x][s]
        assert same_bits(got, want), mode
