#!/usr/bin/env python3
"""Time passes under RPF_FLAG_MEMBER_TEST | RPF_FLAG_MEMBER_FUSED (route 10) against their yardsticks,
RPF_FLAG_TIMING kernel times (rpf_counters.filter_kernel_ms: count + classify + the class launches of a pass), minimum over --steps
calls after one warm-up call.  One JSON line per leg, with mean N and sum S * N (pair evaluations of stage 4) beside it.

  slab_smooth / slab_flat   1920x270x8, smooth and flat_frac = 0.94 (the captured-like regime of section 14d), ONE box-7 pass:
                            (a) unflagged, default route; (b) unflagged with option "binning" = 1 (route 2: route 10's structure and
                            kernels except the count kernel); (c) route 9 and (d) route 10 under multiples 3 / floors -1; (e) route 9
                            and (f) route 10 under preset 1.  Yardsticks: (b) for (d); (c) and (e) for (d) and (f); (a) of the
                            SMOOTH frame, by time per member, for (f) of the flat frame.
  box17                     480x270x8 flat_frac = 0.94, one box-17 pass: unflagged, route 9 and route 10 under preset 1.
  sched8                    480x270x8 flat_frac = 0.94: the schedule {55, 35, 17, 7} of section 14d with SAMPLED_NBHD_FLAG and the draws
                            of section 13d (484, 392, 693, 196) under preset 1, without and with the new bit (every pass has draws: every
                            pass stays route 8), and with the draws of boxes 17 and 7 set to 0 (those two passes: route 9 -> route 10).
  The count kernel's share of a pass: rocprofv3 --kernel-trace --stats over `--step share` (pass (f) of slab_flat, once).

Without --step every step runs as a child process under its own time limit, and the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"slab_smooth": 300, "slab_flat": 300, "box17": 300, "sched8": 420, "share": 180}  # seconds each
CLASS_CAPS = (8, 16, 32, 64, 128, 256, 448, 832, 1600, 3136)
SCHEDULE = ((55, 484), (35, 392), (17, 693), (7, 196))
GEN = dict(seed=20261017, sigma_f=0.05, sigma_c=1e-4, mode="smooth")


def census(n):
    lo = (0,) + CLASS_CAPS[:-1]
    return [int(((n > a) & (n <= b)).sum()) for a, b in zip(lo, CLASS_CAPS)] + [int((n > CLASS_CAPS[-1]).sum())]


def one_pass(ctx, hip, torch, planes, colour, box, flags, steps, label, draws=None, pass_id0=0, reseed=True):
    """`steps` timed calls of one pass after a warm-up call; colour is re-seeded from the planes before each unless reseed is off
    (then the caller's colours are restored from a copy, and the last call's result stays in `colour`)"""
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    if draws is not None:
        ctx.set_sampling(hip.make_sampling(1, [draws], pass_id0=pass_id0))
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
               mean_nbhd=round(c.sum_nbhd / (W * H), 1), max_nbhd=c.max_nbhd, sum_S_N=int(S * c.sum_nbhd),
               filter_ms_min=round(min(ms), 3), filter_ms_max=round(max(ms), 3),
               ns_per_member=round(1e6 * min(ms) / max(c.sum_nbhd, 1), 3), census=census(ctx.nbhd(W, H).ravel()))
    print(json.dumps(rec), flush=True)
    return rec


def make(torch, fb, W, H, S, flat):
    dev = torch.device("cuda", 0)
    planes = fb.synth_planes_chunked(W, H, S, xp=fb.torch_backend(dev), flat_frac=flat, **GEN)
    return planes, torch.empty((3, H, W, S), dtype=torch.float64, device=dev)


def step_slab(name, steps, only_f=False):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, colour = make(torch, fb, 1920, 270, 8, 0.94 if name == "slab_flat" else 0.0)
    M, X = hip.MEMBER_TEST_FLAG, hip.MEMBER_TEST_FLAG | hip.MEMBER_FUSED_FLAG
    with hip.Context(0) as ctx:
        if not only_f:
            one_pass(ctx, hip, torch, planes, colour, 7, 0, steps, name + " (a) unflagged")
            ctx.set_option("binning", 1)
            one_pass(ctx, hip, torch, planes, colour, 7, 0, steps, name + " (b) unflagged, binning 1")
            ctx.set_option("binning", -1)
            ctx.set_membership(hip.membership_preset(hip.MEMBERSHIP_REFERENCE))
            one_pass(ctx, hip, torch, planes, colour, 7, M, steps, name + " (c) route 9, multiples 3, floors -1")
            one_pass(ctx, hip, torch, planes, colour, 7, X, steps, name + " (d) route 10, multiples 3, floors -1")
        ctx.set_membership(hip.membership_preset(hip.MEMBERSHIP_PUBLISHED_19))
        if not only_f:
            one_pass(ctx, hip, torch, planes, colour, 7, M, steps, name + " (e) route 9, preset 1")
        one_pass(ctx, hip, torch, planes, colour, 7, X, steps, name + " (f) route 10, preset 1")


def step_box17(steps):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, colour = make(torch, fb, 480, 270, 8, 0.94)
    M, X = hip.MEMBER_TEST_FLAG, hip.MEMBER_TEST_FLAG | hip.MEMBER_FUSED_FLAG
    with hip.Context(0) as ctx:
        ctx.set_membership(hip.membership_preset(hip.MEMBERSHIP_PUBLISHED_19))
        one_pass(ctx, hip, torch, planes, colour, 17, 0, steps, "box17 unflagged")
        one_pass(ctx, hip, torch, planes, colour, 17, M, steps, "box17 route 9, preset 1")
        one_pass(ctx, hip, torch, planes, colour, 17, X, steps, "box17 route 10, preset 1")


def step_sched(steps):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, _ = make(torch, fb, 480, 270, 8, 0.94)
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    SM = hip.SAMPLED_NBHD_FLAG | hip.MEMBER_TEST_FLAG
    legs = (("sampled + member test", SM, SCHEDULE), ("sampled + member test + fused", SM | hip.MEMBER_FUSED_FLAG, SCHEDULE),
            ("boxes 17, 7 full: member test", SM, SCHEDULE[:2] + ((17, 0), (7, 0))),
            ("boxes 17, 7 full: member test + fused", SM | hip.MEMBER_FUSED_FLAG, SCHEDULE[:2] + ((17, 0), (7, 0))))
    with hip.Context(0) as ctx:
        ctx.set_membership(hip.membership_preset(hip.MEMBERSHIP_PUBLISHED_19))
        for label, flags, schedule in legs:
            colour = torch.empty((3, H, W, S), dtype=torch.float64, device=planes.device)
            ctx.colour_from_planes_device(hip.make_desc(W, H, S), planes.data_ptr(), colour.data_ptr(), stream)
            total, routes = 0.0, []
            for p, (box, D) in enumerate(schedule):
                rec = one_pass(ctx, hip, torch, planes, colour, box, flags, steps, "sched8 %s pass %d" % (label, p), draws=D, pass_id0=p,
                               reseed=False)
                total += rec["filter_ms_min"]
                routes.append(rec["route"])
            print(json.dumps(dict(leg="sched8 %s total" % label, routes=routes, filter_ms_min_sum=round(total, 3))), flush=True)


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
        step_slab("slab_flat", 1, only_f=True)
    elif a.step == "box17":
        step_box17(a.steps)
    else:
        step_sched(a.steps)


if __name__ == "__main__":
    main()
