#!/usr/bin/env python3
"""Time passes whose schedule entry has a gain other than 1 under RPF_FLAG_SCHEDULE_FUSED against the route
the same pass takes without the bit, and against their unscheduled twins (the same pass with gains (1, 1) on the unscheduled
kernels).  RPF_FLAG_TIMING kernel times (rpf_counters.filter_kernel_ms: count + classify + the class launches of a pass), minimum
over --steps calls after one warm-up call.  One JSON line per leg, with mean N and ns per member beside it.

  slab_smooth / slab_flat   1920x270x8, smooth and flat_frac = 0.94 (the captured-like regime of section 14d), ONE box-7 pass under
                            entry 1 of the published preset (gains 2.2, 1.1):
                            (a) RPF_FLAG_GENERIC | PACKED | WAVE | SCHEDULE, route 5: the way without the bit; (b) the new bit, route
                            0 / 1 / 2; (b1) its twin, gains (1, 1); under preset-1 membership (c) route 9, (d) route 10 with the new
                            bit, (d1) its twin.
  box17                     480x270x8 flat_frac = 0.94, one box-17 pass under preset-1 membership and the same entry: (c), (d), (d1).
  sched8                    480x270x8 flat_frac = 0.94: the schedule {55, 35, 17, 7} of section 14e's last paragraph -- draws 484, 392
                            for boxes 55 and 35, 0 for boxes 17 and 7 -- under preset-1 membership, RPF_FLAG_MEMBER_FUSED and the
                            published preset's entries 0 .. 3, without and with the new bit (passes 2 and 3: route 9 -> route 10).

Without --step every step runs as a child process under its own time limit, and the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"slab_smooth": 300, "slab_flat": 300, "box17": 300, "sched8": 420}  # seconds each
CLASS_CAPS = (8, 16, 32, 64, 128, 256, 448, 832, 1600, 3136)
SCHEDULE = ((55, 484), (35, 392), (17, 0), (7, 0))
GEN = dict(seed=20261017, sigma_f=0.05, sigma_c=1e-4, mode="smooth")
ENTRY = 1  # of the published preset: gains (2.2, 1.1)


def census(n):
    lo = (0,) + CLASS_CAPS[:-1]
    return [int(((n > a) & (n <= b)).sum()) for a, b in zip(lo, CLASS_CAPS)] + [int((n > CLASS_CAPS[-1]).sum())]


def entry_schedule(hip, S, entry, ones=False):
    """the published preset read from `entry` on by pass 0 of a call; ones: that entry's seed with gains (1, 1), the unscheduled twin"""
    sc = hip.schedule_preset(hip.SCHEDULE_PUBLISHED, S)
    if ones:
        sc.gain_c[entry], sc.gain_f[entry] = 1.0, 1.0
    sc.pass0 = entry
    return sc


def one_pass(ctx, hip, torch, planes, colour, box, flags, steps, label, sched, draws=None, pass_id0=0, reseed=True):
    """`steps` timed calls of one pass after a warm-up call; colour is re-seeded from the planes before each unless reseed is off
    (then the caller's colours are restored from a copy, and the last call's result stays in `colour`)"""
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    ctx.set_schedule(sched)
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
    e = sched.pass0
    rec = dict(leg=label, shape="%dx%dx%d box %d" % (W, H, S, box), draws=draws, gains=[sched.gain_c[e], sched.gain_f[e]], route=ctx.route(),
               launches=c.filter_kernel_launches, mean_nbhd=round(c.sum_nbhd / (W * H), 1), max_nbhd=c.max_nbhd,
               filter_ms=[round(v, 3) for v in ms], filter_ms_min=round(min(ms), 3),
               ns_per_member=round(1e6 * min(ms) / max(c.sum_nbhd, 1), 3), census=census(ctx.nbhd(W, H).ravel()))
    print(json.dumps(rec), flush=True)
    return rec


def make(torch, fb, W, H, S, flat):
    dev = torch.device("cuda", 0)
    planes = fb.synth_planes_chunked(W, H, S, xp=fb.torch_backend(dev), flat_frac=flat, **GEN)
    return planes, torch.empty((3, H, W, S), dtype=torch.float64, device=dev)


def member_legs(ctx, hip, torch, planes, colour, box, steps, name):
    S = planes.shape[3]
    F, X = hip.SCHEDULE_FLAG, hip.SCHEDULE_FLAG | hip.SCHEDULE_FUSED_FLAG
    M = hip.MEMBER_TEST_FLAG | hip.MEMBER_FUSED_FLAG
    ctx.set_membership(hip.membership_preset(hip.MEMBERSHIP_PUBLISHED_19))
    one_pass(ctx, hip, torch, planes, colour, box, M | F, steps, name + " (c) member test, gains: route 9", entry_schedule(hip, S, ENTRY))
    one_pass(ctx, hip, torch, planes, colour, box, M | X, steps, name + " (d) member test, gains, new bit: route 10", entry_schedule(hip, S, ENTRY))
    one_pass(ctx, hip, torch, planes, colour, box, M | X, steps, name + " (d1) member test, gains (1, 1): route 10, unscheduled kernels",
             entry_schedule(hip, S, ENTRY, ones=True))


def step_slab(name, steps):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, colour = make(torch, fb, 1920, 270, 8, 0.94 if name == "slab_flat" else 0.0)
    S = planes.shape[3]
    F, X = hip.SCHEDULE_FLAG, hip.SCHEDULE_FLAG | hip.SCHEDULE_FUSED_FLAG
    G = hip.FLAG_GENERIC | hip.FLAG_GENERIC_PACKED | hip.FLAG_GENERIC_WAVE
    with hip.Context(0) as ctx:
        one_pass(ctx, hip, torch, planes, colour, 7, G | F, steps, name + " (a) generic | packed | wave, gains: route 5", entry_schedule(hip, S, ENTRY))
        one_pass(ctx, hip, torch, planes, colour, 7, X, steps, name + " (b) gains, new bit: compiled kernels", entry_schedule(hip, S, ENTRY))
        one_pass(ctx, hip, torch, planes, colour, 7, X, steps, name + " (b1) gains (1, 1): unscheduled kernels", entry_schedule(hip, S, ENTRY, ones=True))
        member_legs(ctx, hip, torch, planes, colour, 7, steps, name)


def step_box17(steps):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, colour = make(torch, fb, 480, 270, 8, 0.94)
    with hip.Context(0) as ctx:
        member_legs(ctx, hip, torch, planes, colour, 17, steps, "box17")


def step_sched(steps):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, _ = make(torch, fb, 480, 270, 8, 0.94)
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    SM = hip.SAMPLED_NBHD_FLAG | hip.MEMBER_TEST_FLAG | hip.MEMBER_FUSED_FLAG | hip.SCHEDULE_FLAG
    with hip.Context(0) as ctx:
        ctx.set_membership(hip.membership_preset(hip.MEMBERSHIP_PUBLISHED_19))
        for label, flags in (("without the new bit", SM), ("with the new bit", SM | hip.SCHEDULE_FUSED_FLAG)):
            colour = torch.empty((3, H, W, S), dtype=torch.float64, device=planes.device)
            ctx.colour_from_planes_device(hip.make_desc(W, H, S), planes.data_ptr(), colour.data_ptr(), stream)
            total, routes = 0.0, []
            for p, (box, D) in enumerate(SCHEDULE):
                rec = one_pass(ctx, hip, torch, planes, colour, box, flags, steps, "sched8 %s pass %d" % (label, p), entry_schedule(hip, S, p),
                               draws=D, pass_id0=p, reseed=False)
                total += rec["filter_ms_min"]
                routes.append(rec["route"])
            print(json.dumps(dict(leg="sched8 %s total" % label, routes=routes, filter_ms_min_sum=round(total, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--step", choices=list(STEPS))
    ap.add_argument("--only", nargs="*", default=list(STEPS))
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
    elif a.step == "box17":
        step_box17(a.steps)
    else:
        step_sched(a.steps)


if __name__ == "__main__":
    main()
