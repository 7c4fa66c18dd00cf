#!/usr/bin/env python3
"""Time the spike pass (RPF_FLAG_SPIKE_CLAMP) on the 1920x1080x8 colour planes.

Default mode: the two device halves (rpf_spike_clamp_device, rpf_colour_add_device) on lognormal colours with 5 % of the
samples multiplied by 1e3, generated on the device.  Every step first restores the colours with a device-to-device copy of the
three planes: that copy is the yardstick of section 12 (it reads and writes exactly the bytes the add kernel does).  One JSON
line with the event-timed milliseconds of the copy, of the clamp half (clamp + row sums + read-back) and of the add half.  Kernel
times: run it under `rocprofv3 --kernel-trace --memory-copy-trace --stats`.

--host: the wall clock of rpf_filter from page-locked buffers with and without the flag on the clustered 1920x1080x8 frame, box 7:
the difference is the price of giving up the banded download (the flag implies RPF_FLAG_NO_OVERLAP) plus the pass itself; a
third figure, RPF_FLAG_NO_OVERLAP alone, separates the two."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import rpf_pkg  # noqa: E402

rpf_pkg.load()
from raytracer_rpf_amd import hip  # noqa: E402


def run_kernels(W, H, S, steps, warmup, threshold):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    col0 = torch.exp(torch.randn((3, H, W, S), generator=g, device=dev, dtype=torch.float64) - 1.0)
    hit = torch.rand((H, W, S), generator=g, device=dev) < 0.05
    col0[:, hit] *= 1e3
    col = torch.empty_like(col0)
    desc = hip.make_desc(W, H, S)
    stream = torch.cuda.current_stream().cuda_stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ms = {"copy": [], "clamp_half": [], "add_half": []}
    with hip.Context(0) as ctx:
        for i in range(warmup + steps):
            ev[0].record()
            col.copy_(col0)
            ev[1].record()
            rows, st = ctx.spike_clamp_device(desc, col.data_ptr(), threshold, stream)
            ev[2].record()
            _, delta = hip.spike_delta(rows, W * H * S)
            ctx.colour_add_device(desc, col.data_ptr(), delta, stream)
            ev[3].record()
            torch.cuda.synchronize()
            if i >= warmup:
                for k, (a, b) in zip(ms, ((0, 1), (1, 2), (2, 3))):
                    ms[k].append(ev[a].elapsed_time(ev[b]))
    print(json.dumps({"frame": [W, H, S], "threshold": threshold, "steps": steps, "bytes_three_planes": 3 * W * H * S * 8,
                      "spike_samples": st.spike_samples, "spike_pixels": st.spike_pixels, "skipped_pixels": st.skipped_pixels,
                      "delta": list(delta), **{k + "_ms_median": round(float(np.median(v)), 4) for k, v in ms.items()},
                      **{k + "_ms_min": round(min(v), 4) for k, v in ms.items()}}), flush=True)


def run_host(W, H, S, steps, warmup):
    from raytracer_rpf_amd import feature_buffer as fb
    dev = torch.device("cuda", 0)
    with hip.Context(0) as ctx:
        planes = ctx.host_empty((19, H, W, S))
        planes[...] = fb.synth_planes(W, H, S, xp=fb.torch_backend(dev), mode="clustered", sigma_f=1e-3, sigma_c=0.01).cpu().numpy()
        torch.cuda.empty_cache()
        srgb, prgb = ctx.host_empty((3, H, W, S)), ctx.host_empty((H, W, 3))
        for name, flags in (("rpf_filter", 0), ("rpf_filter, RPF_FLAG_NO_OVERLAP", hip.FLAG_NO_OVERLAP),
                            ("rpf_filter, RPF_FLAG_SPIKE_CLAMP", hip.FLAG_SPIKE_CLAMP)):
            desc = hip.make_desc(W, H, S, boxes=(7,), policy=hip.DEGEN_EPS, flags=flags)
            ms = []
            for i in range(warmup + steps):
                t0 = time.perf_counter()
                ctx.filter(planes, desc, out_samples=srgb, out_pixels=prgb)
                if i >= warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            s = ctx.spike_stats()
            print(json.dumps({"entry": name, "frame": [W, H, S], "calls": steps, "ms_min": round(min(ms), 2),
                              "ms_median": round(float(np.median(ms)), 2), "ms_max": round(max(ms), 2), "spike_applied": s.applied,
                              "spike_samples": s.spike_samples}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frame", default="1920x1080x8")
    ap.add_argument("--threshold", type=float, default=1.0)
    ap.add_argument("--host", action="store_true", help="time rpf_filter with and without the flag instead of the device halves")
    a = ap.parse_args()
    W, H, S = (int(v) for v in a.frame.split("x"))
    if a.host:
        run_host(W, H, S, a.steps, a.warmup)
    else:
        run_kernels(W, H, S, a.steps, a.warmup, a.threshold)


if __name__ == "__main__":
    main()
