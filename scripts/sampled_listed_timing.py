#!/usr/bin/env python3
"""Time sampled passes under RPF_FLAG_SAMPLED_LISTED (route 12) against what runs the same pass without the
bit: route 11 (RPF_FLAG_SAMPLED_FUSED) where that applies, route 8 everywhere.  RPF_FLAG_TIMING kernel times
(rpf_counters.filter_kernel_ms: count + classify + the class launches of a pass), the minimum and the values of --steps calls after
one warm-up call of every leg; the legs of one pass ALTERNATE call by call inside one session, so that a drift of the device is in
every leg alike.  One JSON line per leg, with mean N and ns per member beside it, and one verdict line per pair by section 13f's
rule: a difference counts when it is larger than the spread of either side's calls.

  box_smooth / box_flat   480x270x8, smooth and flat_frac = 0.94 (the captured-like regime): the schedule {55, 35, 17, 7} with the
                          paper's fractions 0.02, 0.04, 0.3, 0.5 of box * box * S as draws (484, 392, 693, 196: section 13f's two
                          tables), one call per pass (pass_id0 = the pass, colours carried on the device): routes 8, 11 and 12.
  spp32                   480x270x32 smooth with the paper's draws 1904, 1536, 2742, 752 (section 13e's table) under
                          RPF_FLAG_SAMPLED_REST | RPF_FLAG_WIDE_NBHD: route 12 against what the call runs without the bit -- route 8
                          at box 55 (wide), route 11 below it.
  spp32_flat              the same on the captured-like 32-spp frame (flat_frac = 0.94).
  waves                   box 17 x 32 spp of that frame on route 12 with option "waves_per_pixel" 1 and 4: the classes N <= 1600 and
                          N <= 3136 on the one-wave and on the four-wave (split-route) listed kernels, at a window above 4096
                          candidates.
  share                   one box-17 pass of the flat 8-spp frame on routes 8, 11 and 12, for a rocprofv3 --kernel-trace --stats run
                          of its own (the three count kernels and the class kernels behind each).
The mask and pool bytes per box are printed with every route-12 leg (mask: ceil((box*box - 1) * S / 64) * 8 bytes per pixel; pool:
4 * (sum N - pixels * S) bytes, what the cursor ends at).

RPF_HIP_LIB picks another build of the library for the whole run (the parent's, built with build(tag=...), gives routes 8 and 11 alone:
--legs 8 11).  Without --step every step runs as a child process under its own time limit, and the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"box_smooth": 300, "box_flat": 240, "spp32": 420, "spp32_flat": 240, "waves": 180, "share": 120}  # seconds each
CLASS_CAPS = (8, 16, 32, 64, 128, 256, 448, 832, 1600, 3136)
SCHEDULE = ((55, 0.02), (35, 0.04), (17, 0.3), (7, 0.5))
SPP32 = ((55, 1904), (35, 1536), (17, 2742), (7, 752))
GEN = dict(seed=20261017, sigma_f=0.05, sigma_c=1e-4, mode="smooth")
DEFAULTS = dict(waves_per_pixel=0)   # every other option: -1


def census(n):
    lo = (0,) + CLASS_CAPS[:-1]
    return [int(((n > a) & (n <= b)).sum()) for a, b in zip(lo, CLASS_CAPS)] + [int((n > CLASS_CAPS[-1]).sum())]


def make(torch, fb, flat, S=8):
    dev = torch.device("cuda", 0)
    W, H = 480, 270
    planes = fb.synth_planes_chunked(W, H, S, xp=fb.torch_backend(dev), flat_frac=flat, **GEN)
    return planes, torch.empty((3, H, W, S), dtype=torch.float64, device=dev)


def alternate(ctx, hip, torch, planes, colour, box, legs, steps, pass_id0=0):
    """legs: (label, flags, draws, options).  Every leg is called once (warm-up), then the legs take turns, `steps` rounds; the
    colours are restored from a copy before each call, and the LAST leg's result stays in `colour` for the next pass"""
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    keep = colour.clone()
    ms = {label: [] for label, _, _, _ in legs}
    info = {}
    for it in range(steps + 1):
        for label, flags, draws, opts in legs:
            for k, v in opts.items():
                ctx.set_option(k, v)
            ctx.set_sampling(hip.make_sampling(1, [draws], pass_id0=pass_id0))
            desc = hip.make_desc(W, H, S, boxes=(box,), policy=hip.DEGEN_EPS, flags=flags | hip.FLAG_TIMING)
            colour.copy_(keep)
            ctx.filter_device(desc, planes.data_ptr(), colour.data_ptr(), stream)
            c = ctx.counters()
            if it:
                ms[label].append(c.filter_kernel_ms)
            info[label] = dict(route=ctx.route(), launches=c.filter_kernel_launches, sum_nbhd=c.sum_nbhd, max_nbhd=c.max_nbhd,
                               census=census(ctx.nbhd(W, H).ravel()))
            for k in opts:
                ctx.set_option(k, DEFAULTS.get(k, -1))
    out = {}
    for label, _, draws, _ in legs:
        i, v = info[label], ms[label]
        out[label] = dict(leg=label, shape="%dx%dx%d box %d" % (W, H, S, box), draws=draws, route=i["route"], launches=i["launches"],
                          mean_nbhd=round(i["sum_nbhd"] / (W * H), 1), max_nbhd=i["max_nbhd"], filter_ms=[round(x, 3) for x in v],
                          filter_ms_min=round(min(v), 3), ns_per_member=round(1e6 * min(v) / max(i["sum_nbhd"], 1), 3), census=i["census"])
        if i["route"] == 12:
            out[label].update(mask_bytes_per_pixel=8 * max(1, ((box * box - 1) * S + 63) // 64),
                              pool_bytes_per_pixel=round(4.0 * (i["sum_nbhd"] - W * H * S) / (W * H), 1))
        print(json.dumps(out[label]), flush=True)
    return out


def verdict(name, box, old, new):
    """the decision rule of section 13f: a difference counts when it is larger than the spread of either side's calls"""
    spread = max(max(old["filter_ms"]) - min(old["filter_ms"]), max(new["filter_ms"]) - min(new["filter_ms"]))
    diff = new["filter_ms_min"] - old["filter_ms_min"]
    print(json.dumps(dict(leg="%s box %d" % (name, box), routes="%d over %d" % (new["route"], old["route"]),
                          ratio=round(new["filter_ms_min"] / old["filter_ms_min"], 4), minus_ms=round(diff, 3), spread_ms=round(spread, 3),
                          verdict="slower" if diff > spread else ("faster" if -diff > spread else "within the spread"))), flush=True)


def bits_of(hip, legs):
    N = hip.SAMPLED_NBHD_FLAG
    have = {8: N, 11: N | hip.SAMPLED_FUSED_FLAG}
    if 12 in legs:
        have[12] = N | hip.SAMPLED_LISTED_FLAG
    return {r: have[r] for r in legs}


def step_box(name, steps, want):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, colour = make(torch, fb, 0.94 if name.endswith("flat") else 0.0)
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    flags = bits_of(hip, want)
    with hip.Context(0) as ctx:
        ctx.colour_from_planes_device(hip.make_desc(W, H, S), planes.data_ptr(), colour.data_ptr(), stream)
        tot = {r: 0.0 for r in want}
        for p, (box, frac) in enumerate(SCHEDULE):
            D = int(frac * box * box * S)
            legs = [("%s pass %d route %d" % (name, p, r), flags[r], D, {}) for r in want]
            res = alternate(ctx, hip, torch, planes, colour, box, legs, steps, pass_id0=p)
            for r, leg in zip(want, legs):
                tot[r] += res[leg[0]]["filter_ms_min"]
                if r == 12:
                    for o, oleg in zip(want, legs):
                        if o != 12:
                            verdict(name, box, res[oleg[0]], res[leg[0]])
        print(json.dumps(dict(leg=name + " total", filter_ms_min_sum={"route %d" % r: round(v, 3) for r, v in tot.items()})), flush=True)


def step_spp32(name, steps, want):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, colour = make(torch, fb, 0.94 if name.endswith("flat") else 0.0, S=32)
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    more = hip.SAMPLED_REST_FLAG | hip.FLAG_WIDE_NBHD
    old = hip.SAMPLED_NBHD_FLAG | hip.SAMPLED_FUSED_FLAG | more     # route 8 at box 55 (wide), route 11 below it: what the parent runs
    with hip.Context(0) as ctx:
        ctx.colour_from_planes_device(hip.make_desc(W, H, S), planes.data_ptr(), colour.data_ptr(), stream)
        tot = [0.0, 0.0]
        for p, (box, D) in enumerate(SPP32):
            legs = [("%s pass %d without the bit" % (name, p), old, D, {})]
            if 12 in want:
                legs.append(("%s pass %d route 12" % (name, p), hip.SAMPLED_NBHD_FLAG | hip.SAMPLED_LISTED_FLAG | more, D, {}))
            res = alternate(ctx, hip, torch, planes, colour, box, legs, steps, pass_id0=p)
            for i, leg in enumerate(legs):
                tot[i] += res[leg[0]]["filter_ms_min"]
            if len(legs) == 2:
                verdict(name, box, res[legs[0][0]], res[legs[1][0]])
        print(json.dumps(dict(leg=name + " total", without_the_bit_ms=round(tot[0], 3), route12_ms=round(tot[1], 3))), flush=True)


def step_waves(steps):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, colour = make(torch, fb, 0.0, S=32)
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    L = hip.SAMPLED_NBHD_FLAG | hip.SAMPLED_LISTED_FLAG | hip.SAMPLED_REST_FLAG
    with hip.Context(0) as ctx:
        ctx.colour_from_planes_device(hip.make_desc(W, H, S), planes.data_ptr(), colour.data_ptr(), stream)
        for D in (1536, 2742):      # N <= 1600 on (nearly) every pixel; N <= 3136
            legs = [("waves box 17 D %d waves_per_pixel %d" % (D, w), L, D, dict(waves_per_pixel=w)) for w in (1, 4)]
            res = alternate(ctx, hip, torch, planes, colour, 17, legs, steps, pass_id0=2)
            verdict("waves 4 over 1, D %d" % D, 17, res[legs[0][0]], res[legs[1][0]])


def step_share(want):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, colour = make(torch, fb, 0.94)
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    flags = bits_of(hip, want)
    with hip.Context(0) as ctx:
        ctx.colour_from_planes_device(hip.make_desc(W, H, S), planes.data_ptr(), colour.data_ptr(), stream)
        alternate(ctx, hip, torch, planes, colour, 17, [("share route %d" % r, flags[r], 693, {}) for r in want], 1, pass_id0=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--step", choices=list(STEPS))
    ap.add_argument("--only", nargs="*", default=list(STEPS)[:-1])
    ap.add_argument("--legs", nargs="*", type=int, default=[8, 11, 12], choices=[8, 11, 12])
    a = ap.parse_args()
    if a.step is None:
        for name in a.only:
            cmd = ["timeout", "-k", "10", str(STEPS[name]), sys.executable, os.path.abspath(__file__), "--step", name, "--steps", str(a.steps),
                   "--legs"] + [str(r) for r in a.legs]
            rc = subprocess.call(cmd)
            if rc != 0:
                print(json.dumps(dict(step=name, exit=rc, note="stopped: nothing more runs on the GPU after a failed step")), flush=True)
                sys.exit(rc)
        return
    import rpf_pkg
    rpf_pkg.load()
    from raytracer_rpf_amd import hip
    print(json.dumps({"step": a.step, "library": os.path.relpath(hip.LIB_PATH, ROOT), "version": hip.load().rpf_version().decode()}), flush=True)
    if a.step in ("box_smooth", "box_flat"):
        step_box(a.step, a.steps, a.legs)
    elif a.step in ("spp32", "spp32_flat"):
        step_spp32(a.step, a.steps, a.legs)
    elif a.step == "waves":
        if 12 in a.legs:
            step_waves(a.steps)
    else:
        step_share(a.legs)


if __name__ == "__main__":
    main()
