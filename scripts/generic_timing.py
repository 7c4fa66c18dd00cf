#!/usr/bin/env python3
"""Time the filter pass of the layout-generic routes (RPF_FLAG_GENERIC alone: route 3; with RPF_FLAG_GENERIC_PACKED: route
4, `generic` = 2; with RPF_FLAG_GENERIC_WAVE as well: route 5, `generic` = 3) next to the fused routes: seeded buffers generated on
the device, rpf_filter_device with RPF_FLAG_TIMING (filter_kernel_ms: events around the pass's filter launches, stage 1a
excluded), one warm-up call, then --steps calls; one JSON line per case with the min and max over the calls, the route,
the launches and the mean neighbourhood size.  Cases (--case to pick by name):
  smooth8      1920x270x8 smooth sigma_f = 0.05, box 7 (mean N ~ 296): 19-dim layout without and with the flag
  flat8        the same slab with flat_frac = 0.94 under EPS (the captured-like small-N regime): without and with the flag
  lay3_12      the smooth slab as (3, 12, fp32) with the flag
  lay4_18      the smooth slab as (4, 18, fp32) with the flag
  box17        256x64x16 smooth, box 17 (N > 3136 for most pixels): 19-dim layout without the flag (the streaming kernel)
               and with it
  wide57       256x57 smooth, box 57, one generated 21-spp buffer: its first 14 samples per pixel under RPF_FLAG_GENERIC
               (box*box*S = 45486: route 3, the streaming kernel) and all 21 under RPF_FLAG_GENERIC | RPF_FLAG_WIDE_NBHD
               (68229: route 6, the wide kernel, `generic` = 6) and | RPF_FLAG_WIDE_CLASSES (route 7, `generic` = 7: nearly
               every pixel still goes to the wide kernel, so the difference is what the count pass costs when it buys
               nothing); ns_per_pixel_sample = filter time / (pixels x mean N)
  flat57       the same geometry with flat_frac = 0.94 (the captured-like small-N regime) under route 6 and under route 7
  flat55       a 1920x64 slab at 32 spp, box 55 (96800: the reference's first box), flat_frac = 0.94, routes 6 and 7: many
               rounds of the wide kernel's slots (seconds per step; not in the default case list's spirit: pick it by name)
  lay4_18_f16  the smooth slab as (4, 18) stored as fp16 halves: routes 3, 4, 5 and the fp32-weight legs of 4 and 5
  smooth32     1920x68x32 smooth, box 7 (N up to 1568), layouts (2, 12) and (3, 12): route 3, route 5 and route 13
               (RPF_FLAG_GENERIC_QUAD on top of route 5's flags, `generic` = 4: 832 < N <= 3136 on the four-wave kernels)
  smooth64     960x34x64 smooth, box 7 (N up to 3136): routes 3, 5 and 13
  box17_8      256x64x8 smooth, box 17 (N up to 2312): routes 3, 5 and 13
  smooth8_quad, flat8_quad   the slabs of smooth8 and flat8 (no pixel above 832) under route 5 and route 13: what the flag
               costs where it has nothing to do
A record of these five cases carries census4, the pixels with N <= 832, <= 1600, <= 3136 and above; a route-13 record carries
ratio_to_route5 and below_route5 (its slowest call against route 5's fastest).
smooth8, flat8, lay3_12, lay4_18 and lay4_18_f16 end with the legs of RPF_FLAG_GENERIC_FAST (`generic` = 12: route 4 with the
flag, 13: route 5 with it; skipped on a library from before the flag): such a record carries ratio_to_fp64, its time over the
same route's without the flag.
smooth8 and flat8 (routes 3 and 5), wide57 (routes 3, 6 and 7) and flat57 (routes 6 and 7) then run the legs of
RPF_FLAG_STREAM_FAST (`generic` + 20: 21 route 3, 23 route 5, 33 route 5 with RPF_FLAG_GENERIC_FAST as well, 26 route 6, 27 route
7; skipped on a library from before the flag), with ratio_to_fp64 and "stream_fast": 1 in the record.
A record of a wide pass carries the class census of its N plane (pixels with N <= 8, 16, ... 832, and the rest).
Each case's variants run in one process on one context and on the same generated buffer; a route-4 or route-5 record
carries ratio_to_route3 next to ratio_to_fused, a route-5 record ratio_to_route4 as well.
A library loaded through RPF_HIP_LIB (a build variant) is measured by the same script."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import rpf_pkg  # noqa: E402

rpf_pkg.load()
from raytracer_rpf_amd import feature_buffer as fb  # noqa: E402
from raytracer_rpf_amd import hip  # noqa: E402

# name: (W, H, S, box, flat_frac, [(n_random, n_feat, generic[, S of this variant: the first samples of the buffer]), ...])
CASES = {
    "smooth8": (1920, 270, 8, 7, 0.0, [(2, 12, 0), (2, 12, 1), (2, 12, 2), (2, 12, 3), (2, 12, 12), (2, 12, 13), (2, 12, 21), (2, 12, 23),
                                       (2, 12, 33)]),
    "flat8": (1920, 270, 8, 7, 0.94, [(2, 12, 0), (2, 12, 1), (2, 12, 2), (2, 12, 3), (2, 12, 12), (2, 12, 13), (2, 12, 21), (2, 12, 23),
                                      (2, 12, 33)]),
    "lay3_12": (1920, 270, 8, 7, 0.0, [(3, 12, 1), (3, 12, 2), (3, 12, 3), (3, 12, 12), (3, 12, 13)]),
    "lay4_18": (1920, 270, 8, 7, 0.0, [(4, 18, 1), (4, 18, 2), (4, 18, 3), (4, 18, 12), (4, 18, 13)]),
    "lay4_18_f16": (1920, 270, 8, 7, 0.0, [(4, 18, 1), (4, 18, 2), (4, 18, 3), (4, 18, 12), (4, 18, 13)]),
    "box17": (256, 64, 16, 17, 0.0, [(2, 12, 0), (2, 12, 1), (2, 12, 2), (2, 12, 3)]),
    "wide57": (256, 57, 21, 57, 0.0, [(2, 12, 1, 14), (2, 12, 6, 21), (2, 12, 7, 21), (2, 12, 21, 14), (2, 12, 26, 21), (2, 12, 27, 21)]),
    "flat57": (256, 57, 21, 57, 0.94, [(2, 12, 6, 21), (2, 12, 7, 21), (2, 12, 26, 21), (2, 12, 27, 21)]),
    "flat55": (1920, 64, 32, 55, 0.94, [(2, 12, 6, 32), (2, 12, 7, 32)]),
    "smooth32": (1920, 68, 32, 7, 0.0, [(2, 12, 1), (2, 12, 3), (2, 12, 4), (3, 12, 1), (3, 12, 3), (3, 12, 4)]),
    "smooth64": (960, 34, 64, 7, 0.0, [(2, 12, 1), (2, 12, 3), (2, 12, 4)]),
    "box17_8": (256, 64, 8, 17, 0.0, [(2, 12, 1), (2, 12, 3), (2, 12, 4)]),
    "smooth8_quad": (1920, 270, 8, 7, 0.0, [(2, 12, 3), (2, 12, 4)]),
    "flat8_quad": (1920, 270, 8, 7, 0.94, [(2, 12, 3), (2, 12, 4)]),
}
QUAD_CASES = ("smooth32", "smooth64", "box17_8", "smooth8_quad", "flat8_quad")  # the cases of RPF_FLAG_GENERIC_QUAD (`generic` = 4)
F16_CASES = ("lay4_18_f16",)  # planes stored as fp16 halves
CLASS_CAPS = (8, 16, 32, 64, 128, 256, 448, 832)


def has_generic_fast():
    """the flag alone is refused by a library that knows it; one from before it ignores the bit"""
    return hasattr(hip, "FLAG_GENERIC_FAST") and hip.layout_kernels(hip.make_desc(8, 8, 4, flags=hip.FLAG_GENERIC_FAST))[0] == hip.E_UNSUPPORTED


def has_stream_fast():
    return hasattr(hip, "FLAG_STREAM_FAST") and hip.layout_kernels(hip.make_desc(8, 8, 4, flags=hip.FLAG_STREAM_FAST))[0] == hip.E_UNSUPPORTED


def run(ctx, name, steps):
    W, H, S_buf, box, flat, legs = CASES[name]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    whole, planes, made = None, None, None
    f16 = name in F16_CASES
    for leg in legs:
        nr, nf, generic = leg[:3]
        stream_fast = generic >= 20  # RPF_FLAG_STREAM_FAST
        if stream_fast and not has_stream_fast():
            continue
        generic = generic - 20 if stream_fast else generic
        fast = generic in (12, 13)   # RPF_FLAG_GENERIC_FAST on route 4 / 5
        if fast and not has_generic_fast():
            continue
        generic = generic - 10 if fast else generic
        S = leg[3] if len(leg) > 3 else S_buf
        if made != (nr, nf):  # one buffer for the variants of a layout
            whole = fb.synth_planes_chunked(W, H, S_buf, xp=fb.torch_backend(dev), seed=20261017, sigma_f=0.05, sigma_c=1e-4,
                                            mode="smooth", flat_frac=flat, n_random=nr, n_feat=nf, **({"dtype": "f16"} if f16 else {}))
            made = (nr, nf)
        planes = whole if S == S_buf else whole[..., :S].contiguous()
        colour = torch.empty((3, H, W, S), dtype=torch.float64, device=dev)
        flags = hip.FLAG_TIMING | (hip.FLAG_GENERIC if generic else 0) | (hip.FLAG_GENERIC_PACKED if generic in (2, 3, 4) else 0)
        flags |= hip.FLAG_GENERIC_WAVE if generic in (3, 4) else 0
        flags |= hip.GENERIC_QUAD_FLAG if generic == 4 else 0
        flags |= hip.FLAG_WIDE_NBHD if generic in (6, 7) else 0
        flags |= hip.FLAG_WIDE_CLASSES if generic == 7 else 0
        flags |= hip.FLAG_GENERIC_FAST if fast else 0
        flags |= hip.FLAG_STREAM_FAST if stream_fast else 0
        desc = hip.make_desc(W, H, S, boxes=(box,), policy=hip.DEGEN_EPS, flags=flags, n_random=nr, n_feat=nf,
                             **({"plane_dtype": hip.PLANES_F16} if f16 else {}))
        ms = []
        for it in range(steps + 1):
            ctx.colour_from_planes_device(desc, planes.data_ptr(), colour.data_ptr(), stream)
            ctx.filter_device(desc, planes.data_ptr(), colour.data_ptr(), stream)
            if it:  # the first call warms up (allocations, tables)
                ms.append(ctx.counters().filter_kernel_ms)
        c = ctx.counters()
        rec = {"case": name, "shape": "%dx%dx%d box %d" % (W, H, S, box), "flat_frac": flat, "layout": [nr, nf, "f16" if f16 else "f32"],
               "generic": generic, "fp32_weights": int(fast), "stream_fast": int(stream_fast), "route": ctx.route(), "launches": c.filter_kernel_launches,
               "mean_nbhd": round(c.sum_nbhd / (W * H), 1), "max_nbhd": c.max_nbhd,
               "filter_ms_min": round(min(ms), 3), "filter_ms_max": round(max(ms), 3), "stats_ms": round(c.stats_kernel_ms, 3),
               "colour_mean": float(colour.mean())}
        if generic in (6, 7):
            n = ctx.nbhd(W, H).ravel()
            lo = (0,) + CLASS_CAPS[:-1]
            rec["census"] = [int(((n > a) & (n <= b)).sum()) for a, b in zip(lo, CLASS_CAPS)] + [int((n > CLASS_CAPS[-1]).sum())]
        if name in QUAD_CASES:
            n = ctx.nbhd(W, H).ravel()
            rec["census4"] = [int((n <= 832).sum()), int(((n > 832) & (n <= 1600)).sum()), int(((n > 1600) & (n <= 3136)).sum()), int((n > 3136).sum())]
        r5 = out.get((nr, nf, 3))
        if generic == 4 and r5:
            rec["ratio_to_route5"] = round(rec["filter_ms_min"] / r5["filter_ms_min"], 3)
            rec["below_route5"] = bool(rec["filter_ms_max"] < r5["filter_ms_min"])
        r6 = out.get((nr, nf, 6))
        if generic == 7 and r6:
            rec["ratio_to_route6"] = round(rec["filter_ms_min"] / r6["filter_ms_min"], 4)
        if len(leg) > 3:
            rec["ns_per_pixel_sample"] = round(rec["filter_ms_min"] * 1e6 / max(c.sum_nbhd, 1), 4)
        if fast or stream_fast:  # the same route without the flag, measured a moment ago on the same buffer
            rec["ratio_to_fp64"] = round(rec["filter_ms_min"] / out[(nr, nf, generic)]["filter_ms_min"], 3)
            print(json.dumps(rec), flush=True)
            del colour
            continue
        out[(nr, nf, generic)] = rec
        base = out.get((nr, nf, 0))
        if generic and base:
            rec["ratio_to_fused"] = round(rec["filter_ms_min"] / base["filter_ms_min"], 2)
        r3 = out.get((nr, nf, 1))
        if generic in (2, 3, 4) and r3:
            rec["ratio_to_route3"] = round(rec["filter_ms_min"] / r3["filter_ms_min"], 3)
        r4 = out.get((nr, nf, 2))
        if generic == 3 and r4:
            rec["ratio_to_route4"] = round(rec["filter_ms_min"] / r4["filter_ms_min"], 3)
        print(json.dumps(rec), flush=True)
        del colour


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--case", nargs="*", default=[c for c in CASES if c != "flat55" and c not in QUAD_CASES])
    a = ap.parse_args()
    print(json.dumps({"library": hip.LIB_PATH, "version": hip.load().rpf_version().decode()}), flush=True)
    with hip.Context(0) as ctx:
        for name in a.case:
            run(ctx, name, a.steps)


if __name__ == "__main__":
    main()
