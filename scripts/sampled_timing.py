#!/usr/bin/env python3
"""Time sampled passes (RPF_FLAG_SAMPLED_NBHD, route 8) against the unsampled routes, RPF_FLAG_TIMING
kernel times (rpf_counters.filter_kernel_ms: count + classify + class launches of a pass), minimum over --steps calls after
one warm-up call.  One JSON line per leg.

  wide57 / flat57   the 256x57x21 buffers of DESIGN.md 11d / 11f (smooth; flat_frac = 0.94, the captured-like regime), ONE
                    box-57 pass (57 * 57 * 21 = 68229: routes 6 and 7 need a pass above 65535) on route 6, route 7 and route 8,
                    and one box-55 pass on route 8 alone.  Draws: the paper's 0.02 * box * box * S - S is 1343 (box 57) and 1249
                    (box 55), above what a class holds: both legs run at the cap, D = 832 - 21 = 811.
  sched8            480x270x8, smooth and flat_frac = 0.94: the schedule {55, 35, 17, 7} with the paper's fractions 0.02, 0.04,
                    0.3, 0.5 of box * box * S as draws (484, 392, 693, 196), per pass (one call per pass, pass_id0 = the pass,
                    colours carried on the device) and in total; against the unsampled call on the fused routes, per pass.
  The count kernel's share of a sampled pass: rocprofv3 --kernel-trace --stats over `--step share` (sampled_count_kernel
  against the class kernels).

Without --step every step runs as a child process under its own time limit, and the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"wide57": 420, "flat57": 300, "sched8_smooth": 420, "sched8_flat": 300, "share": 120}  # seconds each
CLASS_CAPS = (8, 16, 32, 64, 128, 256, 448, 832)
SCHEDULE = ((55, 0.02), (35, 0.04), (17, 0.3), (7, 0.5))


def census(n):
    lo = (0,) + CLASS_CAPS[:-1]
    return [int(((n > a) & (n <= b)).sum()) for a, b in zip(lo, CLASS_CAPS)] + [int((n > CLASS_CAPS[-1]).sum())]


def one_pass(ctx, hip, torch, planes, colour, box, flags, steps, label, draws=None, pass_id0=0, seed=1, reseed=True, **extra):
    """`steps` timed calls of one pass after a warm-up call; colour is re-seeded from the planes before each unless reseed is off
    (then the caller's colours are restored from a copy)"""
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    if draws is not None:
        ctx.set_sampling(hip.make_sampling(seed, [draws], pass_id0=pass_id0))
    desc = hip.make_desc(W, H, S, boxes=(box,), policy=hip.DEGEN_EPS, flags=flags | hip.FLAG_TIMING)
    keep = None if reseed else colour.clone()
    ms = []
    for it in range(steps + 1):
        if reseed:
            ctx.colour_from_planes_device(desc, planes.data_ptr(), colour.data_ptr(), stream)
        else:
            colour.copy_(keep)
        ctx.filter_device(desc, planes.data_ptr(), colour.data_ptr(), stream)
        if it:
            ms.append(ctx.counters().filter_kernel_ms)
    c = ctx.counters()
    rec = dict(leg=label, shape="%dx%dx%d box %d" % (W, H, S, box), draws=draws, route=ctx.route(), launches=c.filter_kernel_launches,
               mean_nbhd=round(c.sum_nbhd / (W * H), 1), max_nbhd=c.max_nbhd, filter_ms_min=round(min(ms), 3),
               filter_ms_max=round(max(ms), 3), census=census(ctx.nbhd(W, H).ravel()), **extra)
    print(json.dumps(rec), flush=True)
    return rec


def step_57(name, steps):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    dev = torch.device("cuda", 0)
    W, H, S, flat = 256, 57, 21, (0.94 if name == "flat57" else 0.0)
    planes = fb.synth_planes_chunked(W, H, S, xp=fb.torch_backend(dev), seed=20261017, sigma_f=0.05, sigma_c=1e-4, mode="smooth", flat_frac=flat)
    colour = torch.empty((3, H, W, S), dtype=torch.float64, device=dev)
    D = 832 - S
    with hip.Context(0) as ctx:
        r6 = one_pass(ctx, hip, torch, planes, colour, 57, hip.FLAG_WIDE_NBHD, steps, name + " route 6")
        r7 = one_pass(ctx, hip, torch, planes, colour, 57, hip.FLAG_WIDE_NBHD | hip.FLAG_WIDE_CLASSES, steps, name + " route 7")
        r8 = one_pass(ctx, hip, torch, planes, colour, 57, hip.FLAG_WIDE_NBHD | hip.SAMPLED_NBHD_FLAG, steps, name + " route 8", draws=D)
        print(json.dumps(dict(leg=name + " box 57", route8_over_route7=round(r8["filter_ms_min"] / r7["filter_ms_min"], 4),
                              route8_over_route6=round(r8["filter_ms_min"] / r6["filter_ms_min"], 4))), flush=True)
        one_pass(ctx, hip, torch, planes, colour, 55, hip.SAMPLED_NBHD_FLAG, steps, name + " route 8 box 55", draws=D)


def step_sched(name, steps, only_sampled=False):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    dev = torch.device("cuda", 0)
    W, H, S, flat = 480, 270, 8, (0.94 if name.endswith("flat") else 0.0)
    planes = fb.synth_planes_chunked(W, H, S, xp=fb.torch_backend(dev), seed=20261017, sigma_f=0.05, sigma_c=1e-4, mode="smooth", flat_frac=flat)
    stream = torch.cuda.current_stream().cuda_stream
    with hip.Context(0) as ctx:
        for label, sampled in (("sampled", True),) + (() if only_sampled else (("unsampled", False),)):
            colour = torch.empty((3, H, W, S), dtype=torch.float64, device=dev)
            ctx.colour_from_planes_device(hip.make_desc(W, H, S), planes.data_ptr(), colour.data_ptr(), stream)
            total = 0.0
            for p, (box, frac) in enumerate(SCHEDULE):
                D = int(frac * box * box * S)  # the paper's fraction of box * box * S; S + D <= 832 at 8 spp
                rec = one_pass(ctx, hip, torch, planes, colour, box, hip.SAMPLED_NBHD_FLAG if sampled else 0, steps,
                               "%s %s pass %d" % (name, label, p), draws=D if sampled else None, pass_id0=p, reseed=False)
                total += rec["filter_ms_min"]
            print(json.dumps(dict(leg="%s %s total" % (name, label), filter_ms_min_sum=round(total, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--step", choices=list(STEPS))
    ap.add_argument("--only", nargs="*", default=list(STEPS)[:-1])
    a = ap.parse_args()
    if a.step is None:
        for name in a.only:
            cmd = ["timeout", "-k", "10", str(STEPS[name]), sys.executable, os.path.abspath(__file__), "--step", name, "--steps", str(a.steps)]
            rc = subprocess.call(cmd)
            if rc != 0:
                print(json.dumps(dict(step=name, exit=rc, note="stopped: nothing more runs on the GPU after a failed step")), flush=True)
                sys.exit(rc)
        return
    import rpf_pkg
    rpf_pkg.load()
    from raytracer_rpf_amd import hip
    print(json.dumps({"step": a.step, "library": os.path.relpath(hip.LIB_PATH, ROOT), "version": hip.load().rpf_version().decode()}), flush=True)
    if a.step in ("wide57", "flat57"):
        step_57(a.step, a.steps)
    elif a.step == "share":
        step_sched("sched8_smooth", 1, only_sampled=True)
    else:
        step_sched(a.step, a.steps)


if __name__ == "__main__":
    main()
