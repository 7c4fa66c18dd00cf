#!/usr/bin/env python3
"""Time the film step alone (rpf_film_splat_device) on a full frame: pbrt's sample film for the image (border included),
pFilm uniform inside each pixel, random colours and ray weights, all generated on the device.  One JSON line per case with
the wall time per call (pFilm check + read-back, stage, gather, stream drained).  Kernel times: run it under
`rocprofv3 --kernel-trace --stats`.  Usage: film_timing.py [--steps K] [--case WxHxS:filter ...], filter = box, triangle,
gaussian, mitchell, sinc at pbrt's default radius.

--slabs N [N ...] times the HOST entries instead, on the sample film of a 1920x1080x8 image (gaussian r = 2: 1924 x 1084)
from the clustered generator (small neighbourhoods: the passes do not drown the film step), box 7 (--boxes 7,5 for two
passes, so that the colour halo refresh between passes is inside the timed call): rpf_filter and
rpf_filter_film on one context, then rpf_multi_filter and rpf_multi_filter_film with N slab contexts on device 0.  One
JSON line per entry with the range over the calls.  A library from before rpf_multi_filter_film (RPF_HIP_LIB) is measured
by the same script: the entry is left out when the export is missing.  Slab contexts that share a device serialise, so
N > 1 on one GPU shows what the deeper halo, the extra refresh and the per-slab read-backs cost, not what several GPUs
gain."""
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


def run_slabs(slab_counts, steps, warmup, boxes):
    import ctypes as C
    from raytracer_rpf_amd import feature_buffer as fb
    L = hip.load()
    w_img, h_img, S = 1920, 1080, 8
    kind = hip.PIXFILTER_GAUSSIAN
    film = hip.make_film(((0, 0), (w_img, h_img)), 2.0, hip.film_table(kind))
    W, H = w_img - 2 * film.sample_x0, h_img - 2 * film.sample_y0  # pbrt's sample bounds for r = 2: two pixels each way
    dev = torch.device("cuda", 0)
    planes = fb.synth_planes(W, H, S, xp=fb.torch_backend(dev), mode="clustered", sigma_f=1e-3, sigma_c=0.01).cpu().numpy()
    planes[0] += np.float32(film.sample_x0)
    planes[1] += np.float32(film.sample_y0)
    torch.cuda.empty_cache()
    desc = hip.make_desc(W, H, S, boxes=boxes, policy=hip.DEGEN_EPS)
    srgb, prgb = np.empty((3, H, W, S), np.float32), np.empty((H, W, 3), np.float32)
    tile, wt, img = (np.empty(s, np.float32) for s in ((h_img, w_img, 3), (h_img, w_img), (h_img, w_img, 3)))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    has_film = hasattr(L, "rpf_multi_filter_film")

    def timed(name, slabs, call, last_error):
        ms = []
        for i in range(warmup + steps):
            t0 = time.perf_counter()
            st = call()
            dt = (time.perf_counter() - t0) * 1e3
            if st != hip.OK:
                raise hip.RpfError(st, last_error())
            if i >= warmup:
                ms.append(dt)
        print(json.dumps({"entry": name, "slabs": slabs, "frame": [W, H, S], "boxes": list(boxes), "calls": steps,
                          "ms_min": round(min(ms), 2), "ms_median": round(float(np.median(ms)), 2), "ms_max": round(max(ms), 2),
                          "library": os.path.basename(hip.LIB_PATH)}), flush=True)

    with hip.Context(0) as ctx:
        err = lambda: L.rpf_last_error(ctx._h).decode()
        timed("rpf_filter", 1, lambda: L.rpf_filter(ctx._h, C.byref(desc), vp(planes), None, vp(srgb), vp(prgb)), err)
        timed("rpf_filter_film", 1, lambda: L.rpf_filter_film(ctx._h, C.byref(desc), C.byref(film), vp(planes), None, vp(srgb),
                                                              vp(tile), vp(wt), vp(img)), err)
        want = (srgb.copy(), tile.copy(), wt.copy(), img.copy())
    for n in slab_counts:
        with hip.MultiContext([0] * n) as mc:
            err = lambda: L.rpf_multi_last_error(mc._h).decode()
            timed("rpf_multi_filter", n, lambda: L.rpf_multi_filter(mc._h, C.byref(desc), vp(planes), None, vp(srgb), vp(prgb)), err)
            if has_film:
                timed("rpf_multi_filter_film", n, lambda: L.rpf_multi_filter_film(mc._h, C.byref(desc), C.byref(film), vp(planes),
                                                                                 None, vp(srgb), vp(tile), vp(wt), vp(img)), err)
                same = all(np.array_equal(a, b) for a, b in zip((srgb, tile, wt, img), want))
                print(json.dumps({"entry": "rpf_multi_filter_film", "slabs": n, "equals_rpf_filter_film": bool(same)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", action="append", default=None)
    ap.add_argument("--slabs", type=int, nargs="+", default=None, help="time the host entries with N slab contexts on device 0")
    ap.add_argument("--boxes", default="7", help="--slabs: box list, e.g. 7,5 (two passes: the colour halo refresh runs between them)")
    a = ap.parse_args()
    if a.slabs:
        run_slabs(a.slabs, a.steps, a.warmup, tuple(int(b) for b in a.boxes.split(",")))
        return
    cases = a.case or ["1920x1080x8:gaussian", "3840x2160x32:sinc"]
    with hip.Context(0) as ctx:
        for c in cases:
            dims, name = c.split(":")
            w, h, s = (int(v) for v in dims.split("x"))
            run(ctx, w, h, s, name, a.steps, a.warmup)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
