#!/usr/bin/env python3
"""Time the film step alone (rpf_film_splat_device) on a full frame: pbrt's sample film for the image (border included),
pFilm uniform inside each pixel, random colours and ray weights, all generated on the device.  One JSON line per case with
the wall time per call (pFilm check + read-back, stage, gather, stream drained).  Kernel times: run it under
`rocprofv3 --kernel-trace --stats`.  Usage: film_timing.py [--steps K] [--case WxHxS:filter ...], filter = box, triangle,
gaussian, mitchell, sinc at pbrt's default radius."""
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

KINDS = {"box": hip.PIXFILTER_BOX, "triangle": hip.PIXFILTER_TRIANGLE, "gaussian": hip.PIXFILTER_GAUSSIAN,
         "mitchell": hip.PIXFILTER_MITCHELL, "sinc": hip.PIXFILTER_SINC}


def run(ctx, w_img, h_img, S, name, steps, warmup):
    kind = KINDS[name]
    r = hip.DEFAULT_RADIUS[kind]
    film = hip.make_film(((0, 0), (w_img, h_img)), r, hip.film_table(kind))
    f32 = np.float32
    x1 = int(np.ceil(f32(w_img) - f32(0.5) + f32(r)))  # Film::GetSampleBounds().pMax
    y1 = int(np.ceil(f32(h_img) - f32(0.5) + f32(r)))
    W, H = x1 - film.sample_x0, y1 - film.sample_y0
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    pf = torch.empty((2, H, W, S), dtype=torch.float32, device=dev)
    pf[0] = (torch.arange(W, device=dev, dtype=torch.float32) + film.sample_x0)[None, :, None]
    pf[1] = (torch.arange(H, device=dev, dtype=torch.float32) + film.sample_y0)[:, None, None]
    pf += torch.rand((2, H, W, S), generator=g, device=dev)
    col = torch.rand((3, H, W, S), generator=g, device=dev, dtype=torch.float64)
    rw = torch.rand((H, W, S), generator=g, device=dev) + 0.5
    tile = torch.empty((h_img, w_img, 3), dtype=torch.float32, device=dev)
    wt = torch.empty((h_img, w_img), dtype=torch.float32, device=dev)
    img = torch.empty((h_img, w_img, 3), dtype=torch.float32, device=dev)
    desc = hip.make_desc(W, H, S)
    stream = torch.cuda.current_stream().cuda_stream
    args = (desc, film, pf.data_ptr(), col.data_ptr(), rw.data_ptr(), tile.data_ptr(), wt.data_ptr(), img.data_ptr(), stream)
    for _ in range(warmup):
        ctx.film_splat_device(*args)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ctx.film_splat_device(*args)  # returns after the stream has drained
    ms = (time.perf_counter() - t0) * 1e3 / steps
    samples = W * H * S
    print(json.dumps({"case": "%dx%dx%d:%s" % (w_img, h_img, S, name), "radius": r, "window": [film.sample_x0, film.sample_y0, W, H],
                      "samples": samples, "ms_per_call": round(ms, 4), "image_mean": float(img.mean())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", action="append", default=None)
    a = ap.parse_args()
    cases = a.case or ["1920x1080x8:gaussian", "3840x2160x32:sinc"]
    with hip.Context(0) as ctx:
        for c in cases:
            dims, name = c.split(":")
            w, h, s = (int(v) for v in dims.split("x"))
            run(ctx, w, h, s, name, a.steps, a.warmup)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
