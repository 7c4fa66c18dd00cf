#!/usr/bin/env python3
"""Time sampled passes beyond S + draws = 832 (RPF_FLAG_SAMPLED_NBHD | RPF_FLAG_SAMPLED_REST, route 8) against
the unsampled routes, RPF_FLAG_TIMING kernel times (rpf_counters.filter_kernel_ms: count + classify + class launches + the rest
launch of a pass), minimum over --steps calls after one warm-up call.  One JSON line per leg.

  sched32_smooth / sched32_flat   480x270x32, smooth and flat_frac = 0.94 (the captured-like regime): the schedule {55, 35, 17, 7}
                    with the paper's fractions 0.02, 0.04, 0.3, 0.5 of box * box * S less the S own samples as draws (1904, 1536,
                    2742, 752), one call per pass (pass_id0 = the pass, colours carried on the device), under SAMPLED_NBHD |
                    SAMPLED_REST | WIDE_NBHD.
  unsampled32_smooth / unsampled32_flat   the same four passes unsampled on the fastest accepted routes: WIDE_NBHD | WIDE_CLASSES for
                    box 55 (55 * 55 * 32 = 96800 > 65535), the fused routes below it.  They run on any build of the ABI: RPF_HIP_LIB
                    names the parent's for the comparison.
  share2742 / share8160 / count800_block / count800_wave   one sampled box-17 pass each on the smooth buffer for rocprofv3
                    --kernel-trace --stats (a run of its own): the count kernel's share at D = 2742 and D = 8160, and
                    sampled_count_block_kernel at D = 800 (S = 33 puts S + D at 833) next to sampled_count_kernel at D = 800 (S = 32).

Without --step the steps of --only run as child processes, each under its own time limit, and the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"sched32_smooth": 300, "sched32_flat": 300, "unsampled32_smooth": 540, "unsampled32_flat": 420,
         "share2742": 120, "share8160": 120, "count800_block": 120, "count800_wave": 120}  # seconds each
CLASS_CAPS = (8, 16, 32, 64, 128, 256, 448, 832)
SCHEDULE = ((55, 0.02), (35, 0.04), (17, 0.3), (7, 0.5))
W, H = 480, 270


def census(n):
    lo = (0,) + CLASS_CAPS[:-1]
    return [int(((n > a) & (n <= b)).sum()) for a, b in zip(lo, CLASS_CAPS)] + [int((n > CLASS_CAPS[-1]).sum())]


def buffer_of(torch, fb, S, flat):
    dev = torch.device("cuda", 0)
    planes = fb.synth_planes_chunked(W, H, S, xp=fb.torch_backend(dev), seed=20261017, sigma_f=0.05, sigma_c=1e-4, mode="smooth",
                                     flat_frac=0.94 if flat else 0.0)
    return planes, torch.empty((3, H, W, S), dtype=torch.float64, device=dev)


def one_pass(ctx, hip, torch, planes, colour, box, flags, steps, label, draws=None, pass_id0=0, seed=1):
    """`steps` timed calls of one pass after a warm-up call, each on the caller's colours (restored from a copy)"""
    S = planes.shape[3]
    stream = torch.cuda.current_stream().cuda_stream
    if draws is not None:
        ctx.set_sampling(hip.make_sampling(seed, [draws], pass_id0=pass_id0))
    desc = hip.make_desc(W, H, S, boxes=(box,), policy=hip.DEGEN_EPS, flags=flags | hip.FLAG_TIMING)
    keep = colour.clone()
    ms = []
    for it in range(steps + 1):
        colour.copy_(keep)
        ctx.filter_device(desc, planes.data_ptr(), colour.data_ptr(), stream)
        if it:
            ms.append(ctx.counters().filter_kernel_ms)
    c = ctx.counters()
    rec = dict(leg=label, shape="%dx%dx%d box %d" % (W, H, S, box), draws=draws, route=ctx.route(), launches=c.filter_kernel_launches,
               mean_nbhd=round(c.sum_nbhd / (W * H), 1), max_nbhd=c.max_nbhd, filter_ms_min=round(min(ms), 3),
               filter_ms_max=round(max(ms), 3), census=census(ctx.nbhd(W, H).ravel()))
    print(json.dumps(rec), flush=True)
    return rec


def step_schedule(name, steps):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    S, sampled = 32, name.startswith("sched32")
    planes, colour = buffer_of(torch, fb, S, name.endswith("flat"))
    stream = torch.cuda.current_stream().cuda_stream
    with hip.Context(0) as ctx:
        ctx.colour_from_planes_device(hip.make_desc(W, H, S), planes.data_ptr(), colour.data_ptr(), stream)
        total = 0.0
        for p, (box, frac) in enumerate(SCHEDULE):
            if sampled:
                D = int(round(frac * box * box * S)) - S   # the paper's neighbourhood size less the own samples
                flags = hip.SAMPLED_NBHD_FLAG | hip.SAMPLED_REST_FLAG | hip.FLAG_WIDE_NBHD
            else:
                D = None
                flags = (hip.FLAG_WIDE_NBHD | hip.FLAG_WIDE_CLASSES) if box * box * S > 65535 else 0
            rec = one_pass(ctx, hip, torch, planes, colour, box, flags, steps, "%s pass %d" % (name, p), draws=D, pass_id0=p)
            total += rec["filter_ms_min"]
        print(json.dumps(dict(leg="%s total" % name, filter_ms_min_sum=round(total, 3))), flush=True)


def step_one(name):
    """one sampled box-17 pass, no repeat: what the profiler's kernel statistics are taken over"""
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    S, D = {"share2742": (32, 2742), "share8160": (32, 8160), "count800_block": (33, 800), "count800_wave": (32, 800)}[name]
    planes, colour = buffer_of(torch, fb, S, False)
    stream = torch.cuda.current_stream().cuda_stream
    with hip.Context(0) as ctx:
        ctx.colour_from_planes_device(hip.make_desc(W, H, S), planes.data_ptr(), colour.data_ptr(), stream)
        one_pass(ctx, hip, torch, planes, colour, 17, hip.SAMPLED_NBHD_FLAG | hip.SAMPLED_REST_FLAG, 1, name, draws=D)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--step", choices=list(STEPS))
    ap.add_argument("--only", nargs="*", default=["sched32_smooth", "sched32_flat", "unsampled32_smooth", "unsampled32_flat"])
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
    if a.step.startswith(("sched32", "unsampled32")):
        step_schedule(a.step, a.steps)
    else:
        step_one(a.step)


if __name__ == "__main__":
    main()
