#!/usr/bin/env python3
"""Time and characterise passes under the per-pass schedule (RPF_FLAG_SCHEDULE).  RPF_FLAG_TIMING kernel
times (rpf_counters.filter_kernel_ms), minimum and maximum over --steps calls after one warm-up call; one JSON line per leg.

  off        the flag off, on the three layout-generic configurations whose kernels gained the branch: route 5 (G | P | W) on the
             smooth and the captured-like (flat_frac = 0.94) 1920x270x8 slab at box 7, route 7 (WIDE_NBHD | WIDE_CLASSES) on the
             captured-like 256x57x21 buffer at box 57.  With --parent-lib PATH (a build of the parent commit) the step runs
             --runs times on each library, alternating parent / new, each run a process of its own: the spread of the parent's
             runs is the yardstick for the difference.
  on         the same three under the flag with gains 1 (no bit: the unscheduled statements) and with gains (1.15, 1.6).
  activity   captured-like 480x270x8, the schedule {55, 35, 17, 7} with the draws of DESIGN.md section 13d (484, 392, 693, 196)
             under SAMPLED_NBHD_FLAG | MEMBER_TEST_FLAG (membership preset 1) | SCHEDULE_FLAG, one pass per call through
             rpf_filter_pass_debug (pass0 and pass_id0 = the pass, colours carried): schedule preset 0 against preset 1 -- rel-L2
             of pixel means and of samples against the input, and per pass the mean alpha, the mean beta and the share of
             clamped (zero) alpha entries.

Without --step every step runs as a child process under its own time limit, and the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"off": 240, "on": 240, "activity": 400}  # seconds each
PASSES = ((55, 484), (35, 392), (17, 693), (7, 196))
GEN = dict(seed=20261017, sigma_f=0.05, sigma_c=1e-4, mode="smooth")
GAINS = (1.15, 1.6)


def configs(hip):
    gpw = hip.FLAG_GENERIC | hip.FLAG_GENERIC_PACKED | hip.FLAG_GENERIC_WAVE
    return (("route 5 smooth", 1920, 270, 8, 7, 0.0, gpw), ("route 5 captured-like", 1920, 270, 8, 7, 0.94, gpw),
            ("route 7 captured-like", 256, 57, 21, 57, 0.94, hip.FLAG_WIDE_NBHD | hip.FLAG_WIDE_CLASSES))


def make(torch, fb, W, H, S, flat):
    dev = torch.device("cuda", 0)
    planes = fb.synth_planes_chunked(W, H, S, xp=fb.torch_backend(dev), flat_frac=flat, **GEN)
    return planes, torch.empty((3, H, W, S), dtype=torch.float64, device=dev)


def one_pass(ctx, hip, torch, planes, colour, box, flags, steps, label, sigma_seed=0.5):
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    desc = hip.make_desc(W, H, S, boxes=(box,), policy=hip.DEGEN_EPS, flags=flags | hip.FLAG_TIMING, sigma_seed=sigma_seed)
    ms = []
    for it in range(steps + 1):
        ctx.colour_from_planes_device(desc, planes.data_ptr(), colour.data_ptr(), stream)
        ctx.filter_device(desc, planes.data_ptr(), colour.data_ptr(), stream)
        if it:
            ms.append(ctx.counters().filter_kernel_ms)
    c = ctx.counters()
    rec = dict(leg=label, shape="%dx%dx%d box %d" % (W, H, S, box), route=ctx.route(), launches=c.filter_kernel_launches,
               mean_nbhd=round(c.sum_nbhd / (W * H), 1), max_nbhd=c.max_nbhd, filter_ms_min=round(min(ms), 3), filter_ms_max=round(max(ms), 3))
    print(json.dumps(rec), flush=True)
    return rec


def step_off_on(steps, on):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    for name, W, H, S, box, flat, flags in configs(hip):
        planes, colour = make(torch, fb, W, H, S, flat)
        with hip.Context(0) as ctx:
            if not on:
                one_pass(ctx, hip, torch, planes, colour, box, flags, steps, name + ", flag off")
                continue
            ctx.set_schedule(hip.make_schedule(0.5, 1.0, 1.0))
            one_pass(ctx, hip, torch, planes, colour, box, flags | hip.SCHEDULE_FLAG, steps, name + ", gains (1, 1)", sigma_seed=0.002)
            ctx.set_schedule(hip.make_schedule(0.5, *GAINS))
            one_pass(ctx, hip, torch, planes, colour, box, flags | hip.SCHEDULE_FLAG, steps, name + ", gains (%g, %g)" % GAINS, sigma_seed=0.002)
        del planes, colour


def step_activity():
    import numpy as np
    from raytracer_rpf_amd import feature_buffer as fb, hip
    W, H, S = 480, 270, 8
    planes = fb.synth_planes_chunked(W, H, S, flat_frac=0.94, **GEN)
    cin = planes[2:5].astype(np.float64)
    flags = hip.SAMPLED_NBHD_FLAG | hip.MEMBER_TEST_FLAG | hip.SCHEDULE_FLAG
    desc = hip.make_desc(W, H, S, policy=hip.DEGEN_EPS, flags=flags)

    def rel(a, b):
        return float(np.linalg.norm(a - b) / np.linalg.norm(b))
    with hip.Context(0) as ctx:
        ctx.set_membership(hip.membership_preset(hip.MEMBERSHIP_PUBLISHED_19))
        for kind in (hip.SCHEDULE_REFERENCE, hip.SCHEDULE_PUBLISHED):
            sched = hip.schedule_preset(kind, S)
            colour = cin
            for p, (box, D) in enumerate(PASSES):
                sched.pass0 = p
                ctx.set_schedule(sched)
                ctx.set_sampling(hip.make_sampling(1, [D], pass_id0=p))
                got = ctx.filter_pass_debug(planes, desc, box=box, colour_in=colour)
                colour = got["colour"]
                print(json.dumps(dict(leg="activity preset %d pass %d" % (kind, p), box=box, draws=D, route=ctx.route(), seed=sched.seed[p],
                                      gain_c=sched.gain_c[p], gain_f=sched.gain_f[p], mean_nbhd=round(got["sum_nbhd"] / (W * H), 1),
                                      mean_alpha=float(got["alpha"].mean()), mean_beta=float(got["beta"].mean()),
                                      alpha_clamped=float((got["alpha"] == 0).mean()), beta_zero=float((got["beta"] == 0).mean()),
                                      rel_l2_samples_so_far=rel(colour, cin))), flush=True)
                del got
            print(json.dumps(dict(leg="activity preset %d after 4 passes" % kind, shape="%dx%dx%d" % (W, H, S),
                                  rel_l2_pixel_means=rel(colour.mean(axis=3), cin.mean(axis=3)), rel_l2_samples=rel(colour, cin))), flush=True)


def child(name, steps, lib=None):
    env = dict(os.environ)
    if lib:
        env["RPF_HIP_LIB"] = os.path.abspath(lib)
    cmd = ["timeout", "-k", "10", str(STEPS[name]), sys.executable, os.path.abspath(__file__), "--step", name, "--steps", str(steps)]
    rc = subprocess.call(cmd, env=env)
    if rc != 0:
        print(json.dumps(dict(step=name, exit=rc, note="stopped: nothing more runs on the GPU after a failed step")), flush=True)
        sys.exit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--step", choices=list(STEPS))
    ap.add_argument("--only", nargs="*", default=list(STEPS))
    ap.add_argument("--parent-lib", help="a build of the parent commit: step `off` alternates it with the in-tree library")
    a = ap.parse_args()
    if a.step is None:
        for name in a.only:
            if name == "off" and a.parent_lib:
                for _ in range(a.runs):
                    child(name, a.steps, a.parent_lib)
                    child(name, a.steps)
            else:
                child(name, a.steps)
        return
    import rpf_pkg
    rpf_pkg.load()
    from raytracer_rpf_amd import hip
    print(json.dumps({"step": a.step, "library": os.path.relpath(hip.LIB_PATH, ROOT), "version": hip.load().rpf_version().decode()}), flush=True)
    if a.step == "activity":
        step_activity()
    else:
        step_off_on(a.steps, a.step == "on")


if __name__ == "__main__":
    main()
