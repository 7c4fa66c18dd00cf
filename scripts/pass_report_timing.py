#!/usr/bin/env python3
"""Time the per-pass activity report (RPF_FLAG_PASS_REPORT).  One JSON line per leg.

  kernels    1920x1080x8 device planes (two fp64 colour buffers, N, alpha, beta, W_r_c): rpf_pass_report_rows_device between
             two device events -- the clearing of the row records, the two report kernels and the read-back of the 1080 row
             records (0.99 MB) -- minimum and maximum over --steps calls after one warm-up call, next to a device-to-device copy
             of the same two colour buffers (2 x 3 planes, 796 MB read and as much written) between the same kind of events.
             Both numbers are stated as measured; no bound is fixed in advance.
  flag       a route-5 pass (G | P | W, smooth 1920x270x8, box 7): rpf_filter_device with and without the flag, host clock around
             the call (it ends in a synchronise), minimum and maximum over --steps calls after one warm-up call of each.
  bench      bench.py --gpus 1 --steps 5 --warmup 1, --runs times on each of --parent-lib (a build of the parent commit) and the
             in-tree library, alternating, each run a process of its own: the two sets of step times must overlap.

Without --step every step runs as a child process under its own time limit, and the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"kernels": 240, "flag": 240, "bench": 300}  # seconds each (bench: each run)
GEN = dict(seed=20261020, sigma_f=0.05, sigma_c=1e-4, mode="smooth")


def step_kernels(steps):
    import torch
    from raytracer_rpf_amd import hip
    W, H, S, nF = 1920, 1080, 8, 12
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    a = torch.rand((3, H, W, S), dtype=torch.float64, device=dev, generator=g)
    b = a + (torch.rand((3, H, W, S), dtype=torch.float64, device=dev, generator=g) < 0.5) * 1e-3
    nbhd = torch.randint(8, 393, (H, W), dtype=torch.int32, device=dev, generator=g)
    alpha, beta, wrc = (torch.rand(sh, dtype=torch.float64, device=dev, generator=g) for sh in ((H, W, 3), (H, W, nF), (H, W)))
    a2, b2 = torch.empty_like(a), torch.empty_like(b)
    desc = hip.make_desc(W, H, S)
    stream = torch.cuda.current_stream().cuda_stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ms = []
        for it in range(steps + 1):
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if it:
                ms.append(ev[0].elapsed_time(ev[1]))
        return round(min(ms), 3), round(max(ms), 3)
    with hip.Context(0) as ctx:
        rep = timed(lambda: ctx.pass_report_rows_device(desc, a.data_ptr(), b.data_ptr(), nbhd.data_ptr(), alpha.data_ptr(), beta.data_ptr(),
                                                        wrc.data_ptr(), stream=stream))
        nul = timed(lambda: ctx.pass_report_rows_device(desc, a.data_ptr(), b.data_ptr(), nbhd.data_ptr(), stream=stream))

    def copy():
        a2.copy_(a)
        b2.copy_(b)
    cp = timed(copy)
    colour_mb = 2 * 3 * H * W * S * 8 / 1e6
    read_mb = colour_mb + H * W * (4 + 8 * (3 + nF + 1)) / 1e6
    print(json.dumps(dict(leg="report, all planes", shape="%dx%dx%d" % (W, H, S), ms_min=rep[0], ms_max=rep[1], bytes_read_mb=round(read_mb, 1),
                          what="row records cleared + pixel kernel + row kernel + 0.99 MB read-back, device events")), flush=True)
    print(json.dumps(dict(leg="report, NULL weight planes", ms_min=nul[0], ms_max=nul[1])), flush=True)
    print(json.dumps(dict(leg="device copy of the two colour buffers", ms_min=cp[0], ms_max=cp[1], bytes_read_mb=round(colour_mb, 1),
                          bytes_written_mb=round(colour_mb, 1), what="two torch copy_ calls, device events")), flush=True)


def step_flag(steps):
    import torch
    from raytracer_rpf_amd import feature_buffer as fb, hip
    W, H, S, box = 1920, 270, 8, 7
    dev = torch.device("cuda", 0)
    planes = fb.synth_planes_chunked(W, H, S, xp=fb.torch_backend(dev), **GEN)
    colour = torch.empty((3, H, W, S), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    gpw = hip.FLAG_GENERIC | hip.FLAG_GENERIC_PACKED | hip.FLAG_GENERIC_WAVE
    with hip.Context(0) as ctx:
        for label, flags in (("flag off", gpw), ("flag on", gpw | hip.PASS_REPORT_FLAG), ("flag off again", gpw)):
            desc = hip.make_desc(W, H, S, boxes=(box,), policy=hip.DEGEN_EPS, flags=flags, sigma_seed=0.5)
            ms = []
            for it in range(steps + 1):
                ctx.colour_from_planes_device(desc, planes.data_ptr(), colour.data_ptr(), stream)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctx.filter_device(desc, planes.data_ptr(), colour.data_ptr(), stream)
                torch.cuda.synchronize()
                if it:
                    ms.append((time.perf_counter() - t0) * 1e3)
            c, r = ctx.counters(), ctx.pass_report(0)
            rec = dict(leg="route-5 pass, " + label, shape="%dx%dx%d box %d" % (W, H, S, box), route=ctx.route(), launches=c.filter_kernel_launches,
                       call_ms_min=round(min(ms), 3), call_ms_max=round(max(ms), 3), report_applied=r.applied)
            if r.applied:
                t = r.total
                rec.update(rel_l2_moved=(sum(t.moved2) / sum(t.in2)) ** 0.5, unchanged_share=t.unchanged_samples / r.samples,
                           mean_alpha=[v / r.pixels for v in t.alpha_sum], own_only_share=t.own_only_pixels / r.pixels,
                           class_pixels=list(t.class_pixels))
            print(json.dumps(rec), flush=True)


def child(name, steps, lib=None):
    env = dict(os.environ)
    if lib:
        env["RPF_HIP_LIB"] = os.path.abspath(lib)
    if name == "bench":
        cmd = ["timeout", "-k", "10", str(STEPS[name]), sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1"]
    else:
        cmd = ["timeout", "-k", "10", str(STEPS[name]), sys.executable, os.path.abspath(__file__), "--step", name, "--steps", str(steps)]
    rc = subprocess.call(cmd, env=env)
    if rc != 0:
        print(json.dumps(dict(step=name, exit=rc, note="stopped: nothing more runs on the GPU after a failed step")), flush=True)
        sys.exit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--step", choices=["kernels", "flag"])
    ap.add_argument("--only", nargs="*", default=list(STEPS))
    ap.add_argument("--parent-lib", help="a build of the parent commit: step `bench` alternates it with the in-tree library")
    a = ap.parse_args()
    if a.step is None:
        for name in a.only:
            if name == "bench":
                for _ in range(a.runs):
                    if a.parent_lib:
                        child(name, a.steps, a.parent_lib)
                    child(name, a.steps)
            else:
                child(name, a.steps)
        return
    import rpf_pkg
    rpf_pkg.load()
    from raytracer_rpf_amd import hip
    print(json.dumps({"step": a.step, "library": os.path.relpath(hip.LIB_PATH, ROOT), "version": hip.load().rpf_version().decode()}), flush=True)
    if a.step == "kernels":
        step_kernels(a.steps)
    else:
        step_flag(a.steps)


if __name__ == "__main__":
    main()
