#!/usr/bin/env python3
"""Time passes under the membership test (RPF_FLAG_MEMBER_TEST, route 9) against the unflagged routes,
RPF_FLAG_TIMING kernel times (rpf_counters.filter_kernel_ms: count + classify + class and rest launches of a pass), minimum over
--steps calls after one warm-up call.  One JSON line per leg, with mean N and sum S * N (pair evaluations of stage 4) beside it.

  slab_smooth / slab_flat   1920x270x8, smooth and flat_frac = 0.94 (the captured-like regime), ONE box-7 pass: without the flag,
                            with it under multiples 3 / floors -1 (the reference's test on route 9) and under preset 1.  The
                            preset-1 pass of the flat frame does more work by design: its yardstick is the unflagged pass of
                            the SMOOTH frame, whose mean N is similar, not its own unflagged time.
  sched8                    480x270x8 flat_frac = 0.94: the schedule {55, 35, 17, 7} with the draws of DESIGN.md section 13d
                            (484, 392, 693, 196) under SAMPLED_NBHD_FLAG alone and with MEMBER_TEST_FLAG (preset 1) as well, per
                            pass (one call per pass, pass_id0 = the pass, colours carried on the device) and in total.
  activity                  480x270x8 flat_frac = 0.94, one box-7 pass at sigma_seed 0.002 and 0.5: rel-L2 of the per-pixel mean
                            colour against the input's, without the flag and under preset 1.
  The count kernel's share of a pass: rocprofv3 --kernel-trace --stats over `--step share` (the preset-1 pass of slab_flat).

Without --step every step runs as a child process under its own time limit, and the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"slab_smooth": 300, "slab_flat": 300, "sched8": 300, "activity": 180, "share": 180}  # seconds each
CLASS_CAPS = (8, 16, 32, 64, 128, 256, 448, 832)
SCHEDULE = ((55, 484), (35, 392), (17, 693), (7, 196))
GEN = dict(seed=20261017, sigma_f=0.05, sigma_c=1e-4, mode="smooth")


def census(n):
    lo = (0,) + CLASS_CAPS[:-1]
    return [int(((n > a) & (n <= b)).sum()) for a, b in zip(lo, CLASS_CAPS)] + [int((n > CLASS_CAPS[-1]).sum())]


def one_pass(ctx, hip, torch, planes, colour, box, flags, steps, label, draws=None, pass_id0=0, reseed=True, sigma_seed=0.002):
    """`steps` timed calls of one pass after a warm-up call; colour is re-seeded from the planes before each unless reseed is off
    (then the caller's colours are restored from a copy, and the last call's result stays in `colour`)"""
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    if draws is not None:
        ctx.set_sampling(hip.make_sampling(1, [draws], pass_id0=pass_id0))
    desc = hip.make_desc(W, H, S, boxes=(box,), policy=hip.DEGEN_EPS, flags=flags | hip.FLAG_TIMING, sigma_seed=sigma_seed)
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
               mean_nbhd=round(c.sum_nbhd / (W * H), 1), max_nbhd=c.max_nbhd, sum_S_N=int(S * c.sum_nbhd),
               filter_ms_min=round(min(ms), 3), filter_ms_max=round(max(ms), 3), census=census(ctx.nbhd(W, H).ravel()))
    print(json.dumps(rec), flush=True)
    return rec


def make(torch, fb, W, H, S, flat):
    dev = torch.device("cuda", 0)
    planes = fb.synth_planes_chunked(W, H, S, xp=fb.torch_backend(dev), flat_frac=flat, **GEN)
    return planes, torch.empty((3, H, W, S), dtype=torch.float64, device=dev)


def step_slab(name, steps, only_preset=False):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, colour = make(torch, fb, 1920, 270, 8, 0.94 if name == "slab_flat" else 0.0)
    F = hip.MEMBER_TEST_FLAG
    with hip.Context(0) as ctx:
        if not only_preset:
            one_pass(ctx, hip, torch, planes, colour, 7, 0, steps, name + " unflagged")
            ctx.set_membership(hip.membership_preset(hip.MEMBERSHIP_REFERENCE))
            one_pass(ctx, hip, torch, planes, colour, 7, F, steps, name + " multiples 3, floors -1")
        ctx.set_membership(hip.membership_preset(hip.MEMBERSHIP_PUBLISHED_19))
        one_pass(ctx, hip, torch, planes, colour, 7, F, steps, name + " preset 1")


def step_sched(steps):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, _ = make(torch, fb, 480, 270, 8, 0.94)
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    with hip.Context(0) as ctx:
        ctx.set_membership(hip.membership_preset(hip.MEMBERSHIP_PUBLISHED_19))
        for label, flags in (("sampled", hip.SAMPLED_NBHD_FLAG), ("sampled + member test", hip.SAMPLED_NBHD_FLAG | hip.MEMBER_TEST_FLAG)):
            colour = torch.empty((3, H, W, S), dtype=torch.float64, device=planes.device)
            ctx.colour_from_planes_device(hip.make_desc(W, H, S), planes.data_ptr(), colour.data_ptr(), stream)
            total = 0.0
            for p, (box, D) in enumerate(SCHEDULE):
                rec = one_pass(ctx, hip, torch, planes, colour, box, flags, steps, "sched8 %s pass %d" % (label, p), draws=D, pass_id0=p,
                               reseed=False)
                total += rec["filter_ms_min"]
            print(json.dumps(dict(leg="sched8 %s total" % label, filter_ms_min_sum=round(total, 3))), flush=True)


def step_activity():
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, colour = make(torch, fb, 480, 270, 8, 0.94)
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    with hip.Context(0) as ctx:
        ctx.set_membership(hip.membership_preset(hip.MEMBERSHIP_PUBLISHED_19))
        for sigma in (0.002, 0.5):
            for label, flags in (("unflagged", 0), ("preset 1", hip.MEMBER_TEST_FLAG)):
                desc = hip.make_desc(W, H, S, boxes=(7,), policy=hip.DEGEN_EPS, flags=flags, sigma_seed=sigma)
                ctx.colour_from_planes_device(desc, planes.data_ptr(), colour.data_ptr(), stream)
                before = colour.mean(dim=3)
                sample_in = colour.clone()
                ctx.filter_device(desc, planes.data_ptr(), colour.data_ptr(), stream)
                torch.cuda.synchronize()
                after = colour.mean(dim=3)
                c = ctx.counters()
                print(json.dumps(dict(leg="activity %s" % label, shape="%dx%dx%d box 7" % (W, H, S), sigma_seed=sigma, route=ctx.route(),
                                      mean_nbhd=round(c.sum_nbhd / (W * H), 1),
                                      rel_l2_pixel_means=float((after - before).norm() / before.norm()),
                                      rel_l2_samples=float((colour - sample_in).norm() / sample_in.norm()),
                                      pixels_changed=float(((after - before).abs().amax(dim=0) > 0).double().mean()))), flush=True)


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
    if a.step in ("slab_smooth", "slab_flat"):
        step_slab(a.step, a.steps)
    elif a.step == "share":
        step_slab("slab_flat", 1, only_preset=True)
    elif a.step == "sched8":
        step_sched(a.steps)
    else:
        step_activity()


if __name__ == "__main__":
    main()
