#!/usr/bin/env python3
"""Time sampled passes under RPF_FLAG_SAMPLED_FUSED (route 11) against route 8, the same pass without the
bit, and against the unsampled pass on the compiled kernels.  RPF_FLAG_TIMING kernel times (rpf_counters.filter_kernel_ms: count
+ classify + the class launches of a pass), the minimum and the three values of --steps calls after one warm-up call of every leg;
the legs of one pass ALTERNATE call by call inside one session (route 8, route 11, unsampled, route 8, ...), so that a drift of the
device is in every leg alike.  One JSON line per leg, with mean N and ns per member beside it.

  box_smooth / box_flat   480x270x8, smooth and flat_frac = 0.94 (the captured-like regime): the schedule {55, 35, 17, 7} with the
                          paper's fractions 0.02, 0.04, 0.3, 0.5 of box * box * S as draws (484, 392, 693, 196; the frames and draws
                          of sections 13d and 15e), one call per pass (pass_id0 = the pass, colours carried on the device): route 8,
                          route 11 and the unsampled pass, per box.
  sched8                  480x270x8 flat_frac = 0.94: the table of section 15e -- draws 484, 392 for boxes 55 and 35, 0 for boxes 17
                          and 7, under preset-1 membership, RPF_FLAG_MEMBER_FUSED, RPF_FLAG_SCHEDULE_FUSED and the published preset's
                          entries 0 .. 3 -- without and with RPF_FLAG_SAMPLED_FUSED (passes 0 and 1: route 8 -> route 11).
  stride                  box_flat's boxes 55 and 35 on route 11 and -- option "sampled_fused_stride" below the pass's stride -- on
                          route 8 through the same flagged call: the option's way out, timed.
  share                   one box-17 pass of the flat frame on route 8 and on route 11, for a rocprofv3 --kernel-trace --stats run of
                          its own (sampled_count_kernel against sampled_count_mask_kernel and the class kernels behind each).

Without --step every step runs as a child process under its own time limit, and the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"box_smooth": 420, "box_flat": 300, "sched8": 300, "stride": 300, "share": 120}  # seconds each
CLASS_CAPS = (8, 16, 32, 64, 128, 256, 448, 832, 1600, 3136)
SCHEDULE = ((55, 0.02), (35, 0.04), (17, 0.3), (7, 0.5))
SCHED8 = ((55, 484), (35, 392), (17, 0), (7, 0))
GEN = dict(seed=20261017, sigma_f=0.05, sigma_c=1e-4, mode="smooth")


def census(n):
    lo = (0,) + CLASS_CAPS[:-1]
    return [int(((n > a) & (n <= b)).sum()) for a, b in zip(lo, CLASS_CAPS)] + [int((n > CLASS_CAPS[-1]).sum())]


def make(torch, fb, flat):
    dev = torch.device("cuda", 0)
    W, H, S = 480, 270, 8
    planes = fb.synth_planes_chunked(W, H, S, xp=fb.torch_backend(dev), flat_frac=flat, **GEN)
    return planes, torch.empty((3, H, W, S), dtype=torch.float64, device=dev)


def alternate(ctx, hip, torch, planes, colour, box, legs, steps, pass_id0=0, sched=None):
    """legs: (label, flags, draws, options).  Every leg is called once (warm-up), then the legs take turns, `steps` rounds; the
    colours are restored from a copy before each call, and the LAST leg's result stays in `colour` for the next pass"""
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    keep = colour.clone()
    ms = {label: [] for label, _, _, _ in legs}
    info = {}
    if sched is not None:
        ctx.set_schedule(sched)
    for it in range(steps + 1):
        for label, flags, draws, opts in legs:
            for k, v in opts.items():
                ctx.set_option(k, v)
            if draws is not None:
                ctx.set_sampling(hip.make_sampling(1, [draws], pass_id0=pass_id0))
            desc = hip.make_desc(W, H, S, boxes=(box,), policy=hip.DEGEN_EPS, flags=flags | hip.FLAG_TIMING)
            colour.copy_(keep)
            ctx.filter_device(desc, planes.data_ptr(), colour.data_ptr(), stream)
            c = ctx.counters()
            if it:
                ms[label].append(c.filter_kernel_ms)
            info[label] = dict(route=ctx.route(), launches=c.filter_kernel_launches, sum_nbhd=c.sum_nbhd, max_nbhd=c.max_nbhd, draws=draws,
                               census=census(ctx.nbhd(W, H).ravel()))
            for k in opts:
                ctx.set_option(k, -1)
    out = {}
    for label, _, _, _ in legs:
        i, v = info[label], ms[label]
        out[label] = dict(leg=label, shape="%dx%dx%d box %d" % (W, H, S, box), draws=i["draws"], route=i["route"], launches=i["launches"],
                          mean_nbhd=round(i["sum_nbhd"] / (W * H), 1), max_nbhd=i["max_nbhd"], filter_ms=[round(x, 3) for x in v],
                          filter_ms_min=round(min(v), 3), ns_per_member=round(1e6 * min(v) / max(i["sum_nbhd"], 1), 3), census=i["census"])
        print(json.dumps(out[label]), flush=True)
    return out


def verdict(name, box, old, new):
    """the decision rule of section 13f: a loss counts when it is larger than the spread of either side's calls"""
    spread = max(max(old["filter_ms"]) - min(old["filter_ms"]), max(new["filter_ms"]) - min(new["filter_ms"]))
    diff = new["filter_ms_min"] - old["filter_ms_min"]
    print(json.dumps(dict(leg="%s box %d" % (name, box), route11_over_route8=round(new["filter_ms_min"] / old["filter_ms_min"], 4),
                          route11_minus_route8_ms=round(diff, 3), spread_ms=round(spread, 3),
                          verdict="slower" if diff > spread else ("faster" if -diff > spread else "within the spread"))), flush=True)


def step_box(name, steps):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, colour = make(torch, fb, 0.94 if name.endswith("flat") else 0.0)
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    N, X = hip.SAMPLED_NBHD_FLAG, hip.SAMPLED_NBHD_FLAG | hip.SAMPLED_FUSED_FLAG
    with hip.Context(0) as ctx:
        ctx.colour_from_planes_device(hip.make_desc(W, H, S), planes.data_ptr(), colour.data_ptr(), stream)
        tot = dict(r8=0.0, r11=0.0, full=0.0)
        for p, (box, frac) in enumerate(SCHEDULE):
            D = int(frac * box * box * S)
            legs = (("%s pass %d unsampled" % (name, p), 0, None, {}), ("%s pass %d route 8" % (name, p), N, D, {}),
                    ("%s pass %d route 11" % (name, p), X, D, {}))
            r = alternate(ctx, hip, torch, planes, colour, box, legs, steps, pass_id0=p)
            verdict(name, box, r[legs[1][0]], r[legs[2][0]])
            for k, leg in zip(("full", "r8", "r11"), legs):
                tot[k] += r[leg[0]]["filter_ms_min"]
        print(json.dumps(dict(leg=name + " total", unsampled_ms=round(tot["full"], 3), route8_ms=round(tot["r8"], 3), route11_ms=round(tot["r11"], 3))), flush=True)


def step_sched8(steps):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, colour = make(torch, fb, 0.94)
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    SM = hip.SAMPLED_NBHD_FLAG | hip.MEMBER_TEST_FLAG | hip.MEMBER_FUSED_FLAG | hip.SCHEDULE_FLAG | hip.SCHEDULE_FUSED_FLAG
    with hip.Context(0) as ctx:
        ctx.set_membership(hip.membership_preset(hip.MEMBERSHIP_PUBLISHED_19))
        ctx.colour_from_planes_device(hip.make_desc(W, H, S), planes.data_ptr(), colour.data_ptr(), stream)
        tot, routes = [0.0, 0.0], [[], []]
        for p, (box, D) in enumerate(SCHED8):
            sc = hip.schedule_preset(hip.SCHEDULE_PUBLISHED, S)
            sc.pass0 = p
            legs = (("sched8 without the new bit pass %d" % p, SM, D, {}), ("sched8 with the new bit pass %d" % p, SM | hip.SAMPLED_FUSED_FLAG, D, {}))
            r = alternate(ctx, hip, torch, planes, colour, box, legs, steps, pass_id0=p, sched=sc)
            for i, leg in enumerate(legs):
                tot[i] += r[leg[0]]["filter_ms_min"]
                routes[i].append(r[leg[0]]["route"])
        for i, label in enumerate(("without the new bit", "with the new bit")):
            print(json.dumps(dict(leg="sched8 %s total" % label, routes=routes[i], filter_ms_min_sum=round(tot[i], 3))), flush=True)


def step_stride(steps):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, colour = make(torch, fb, 0.94)
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    X = hip.SAMPLED_NBHD_FLAG | hip.SAMPLED_FUSED_FLAG
    with hip.Context(0) as ctx:
        ctx.colour_from_planes_device(hip.make_desc(W, H, S), planes.data_ptr(), colour.data_ptr(), stream)
        for p, (box, frac) in enumerate(SCHEDULE[:2]):
            D, stride = int(frac * box * box * S), ((box * box - 1) * S + 63) // 64
            legs = (("stride box %d, option %d: route 8" % (box, stride - 1), X, D, dict(sampled_fused_stride=stride - 1)),
                    ("stride box %d, option %d: route 11" % (box, stride), X, D, dict(sampled_fused_stride=stride)))
            alternate(ctx, hip, torch, planes, colour, box, legs, steps, pass_id0=p)


def step_share():
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    planes, colour = make(torch, fb, 0.94)
    _, H, W, S = planes.shape
    stream = torch.cuda.current_stream().cuda_stream
    N, X = hip.SAMPLED_NBHD_FLAG, hip.SAMPLED_NBHD_FLAG | hip.SAMPLED_FUSED_FLAG
    with hip.Context(0) as ctx:
        ctx.colour_from_planes_device(hip.make_desc(W, H, S), planes.data_ptr(), colour.data_ptr(), stream)
        alternate(ctx, hip, torch, planes, colour, 17, (("share route 8", N, 693, {}), ("share route 11", X, 693, {})), 1, pass_id0=2)


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
    if a.step in ("box_smooth", "box_flat"):
        step_box(a.step, a.steps)
    elif a.step == "sched8":
        step_sched8(a.steps)
    elif a.step == "stride":
        step_stride(a.steps)
    else:
        step_share()


if __name__ == "__main__":
    main()
