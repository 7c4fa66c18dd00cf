"""NumPy restatement of pbrt-v3's film step as the rpf integrator drives it (test infrastructure, not a test module).

RPFIntegrator::Render feeds every sample through FilmTile::AddSample (film.h:121-161) in the order buffer column x, row y,
sample s (rpf.cpp:783-786), then MergeFilmTile and WriteImage (film.cpp:117-130, 169-203).  Here every operation takes
np.float32 operands, so each rounds to single precision and nothing is fused.  The loop runs over output pixels at once
(vectorised) and over the candidate window in the reference's order (qx, qy, s ascending), which is the order in which the
serial loop adds to any one pixel.  The window is deliberately two pixels wider than floor(r + 0.5): the candidate test is
pbrt's own, so extra candidates change nothing, and a kernel whose window missed a sample would disagree with this.
"""
import math

import numpy as np

F = np.float32
BOX, TRIANGLE, GAUSSIAN, MITCHELL, SINC = range(5)
TW = 16  # Film::filterTableWidth
DEFAULT_RADIUS = {BOX: 0.5, TRIANGLE: 2.0, GAUSSIAN: 2.0, MITCHELL: 2.0, SINC: 4.0}


def _max0(v):
    """std::max((Float)0, v) = (0 < v) ? v : 0"""
    return np.where(F(0) < v, v, F(0)).astype(F)


# ---- filters (filters/*.cpp Evaluate) and the table of film.cpp:66-76 --------------------------------------------------
def _mitchell1d(x, B, C):
    x = F(abs(F(2) * x))
    if x > F(1):
        return ((-B - F(6) * C) * x * x * x + (F(6) * B + F(30) * C) * x * x + (F(-12) * B - F(48) * C) * x
                + (F(8) * B + F(24) * C)) * (F(1) / F(6))
    return ((F(12) - F(9) * B - F(6) * C) * x * x * x + (F(-18) + F(12) * B + F(6) * C) * x * x + (F(6) - F(2) * B)) * (F(1) / F(6))


def _sinc(x):
    x = F(abs(x))
    if float(x) < 1e-5:
        return F(1)
    pi = F(math.pi)
    return F(np.sin(pi * x)) / (pi * x)


def _windowed_sinc(x, radius, tau):
    x = F(abs(x))
    if x > radius:
        return F(0)
    lanczos = _sinc(x / tau)
    return _sinc(x) * lanczos


def evaluate(kind, px, py, rx, ry, p0=None, p1=None):
    px, py, rx, ry = F(px), F(py), F(rx), F(ry)
    if kind == BOX:
        return F(1)
    if kind == TRIANGLE:
        return F(_max0(rx - F(abs(px))) * _max0(ry - F(abs(py))))
    if kind == GAUSSIAN:
        a = F(2) if p0 is None else F(p0)
        ex, ey = F(np.exp(-a * rx * rx)), F(np.exp(-a * ry * ry))
        return F(_max0(F(np.exp(-a * px * px)) - ex) * _max0(F(np.exp(-a * py * py)) - ey))
    if kind == MITCHELL:
        B = F(1) / F(3) if p0 is None else F(p0)
        C = F(1) / F(3) if p1 is None else F(p1)
        return F(_mitchell1d(px * (F(1) / rx), B, C) * _mitchell1d(py * (F(1) / ry), B, C))
    if kind == SINC:
        tau = F(3) if p0 is None else F(p0)
        return F(_windowed_sinc(px, rx, tau) * _windowed_sinc(py, ry, tau))
    raise ValueError(kind)


def filter_table(kind, rx=None, ry=None, p0=None, p1=None):
    rx = F(DEFAULT_RADIUS[kind] if rx is None else rx)
    ry = rx if ry is None else F(ry)
    t = np.empty((TW, TW), F)
    for y in range(TW):
        for x in range(TW):
            t[y, x] = evaluate(kind, (F(x) + F(0.5)) * rx / F(TW), (F(y) + F(0.5)) * ry / F(TW), rx, ry, p0, p1)
    return t


def sample_bounds(pixel_bounds, rx, ry):
    """Film::GetSampleBounds (film.cpp:80-86): ((x0, y0), (x1, y1))"""
    (px0, py0), (px1, py1) = pixel_bounds
    return ((int(np.floor(F(px0) + F(0.5) - F(rx))), int(np.floor(F(py0) + F(0.5) - F(ry)))),
            (int(np.ceil(F(px1) - F(0.5) + F(rx))), int(np.ceil(F(py1) - F(0.5) + F(ry)))))


# ---- FilmTile::AddSample over the whole sample film, gathered per output pixel ------------------------------------------
def prepare(colour, ray_weight=None, max_sample_luminance=np.inf):
    """per sample: L = (Float) colour, the luminance clamp, then L * sampleWeight.  colour [3,H,W,S] -> float32 [3,H,W,S];
    also returns how many samples the clamp changed"""
    L = np.asarray(colour).astype(F)
    m = F(max_sample_luminance)
    lum = F(0.212671) * L[0] + F(0.715160) * L[1] + F(0.072169) * L[2]
    hit = lum > m
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        k = (m / lum).astype(F)
        L = np.where(hit[None], L * k[None], L).astype(F)
    sw = F(1) if ray_weight is None else np.asarray(ray_weight, F)[None]
    return (L * sw).astype(F), int(hit.sum())


def splat(pfilm, lw, origin, pixel_bounds, rx, ry, table, extra=2):
    """pfilm float32 [2,H,W,S] (raster coordinates), lw from prepare(); returns contribSum [ny,nx,3], filterWeightSum [ny,nx].
    The window reaches floor(r + 0.5) + extra pixels each way (tests narrow it to show that a case needs the width)."""
    (sx0, sy0), ((px0, py0), (px1, py1)) = origin, pixel_bounds
    _, H, W, S = pfilm.shape
    rx, ry = F(rx), F(ry)
    irx, iry = F(1) / rx, F(1) / ry
    d = (np.asarray(pfilm, F) - F(0.5)).astype(F)
    X = np.arange(px0, px1)[None, :]
    Y = np.arange(py0, py1)[:, None]
    Xf, Yf = X.astype(F), Y.astype(F)
    bx, by = X - sx0, Y - sy0
    ny, nx = py1 - py0, px1 - px0
    acc = np.zeros((3, ny, nx), F)
    wsum = np.zeros((ny, nx), F)
    hx, hy = int(np.floor(float(rx) + 0.5)) + extra, int(np.floor(float(ry) + 0.5)) + extra
    with np.errstate(invalid="ignore", over="ignore"):
        for ox in range(-hx, hx + 1):
            qx = bx + ox
            okx = (qx >= 0) & (qx < W)
            qxc = np.clip(qx, 0, W - 1)
            for oy in range(-hy, hy + 1):
                qy = by + oy
                oky = (qy >= 0) & (qy < H)
                if not oky.any() or not okx.any():
                    continue
                qyc = np.clip(qy, 0, H - 1)
                for s in range(S):
                    dx = d[0][qyc, qxc, s]
                    dy = d[1][qyc, qxc, s]
                    p0x = np.ceil(dx - rx).astype(np.int64)
                    p1x = np.floor(dx + rx).astype(np.int64) + 1
                    p0y = np.ceil(dy - ry).astype(np.int64)
                    p1y = np.floor(dy + ry).astype(np.int64) + 1
                    hit = okx & oky & (p0x <= X) & (X < p1x) & (p0y <= Y) & (Y < p1y)
                    if not hit.any():
                        continue
                    fx = np.abs((Xf - dx) * irx * F(TW))
                    fy = np.abs((Yf - dy) * iry * F(TW))
                    ifx = np.minimum(np.floor(np.where(hit, fx, F(0))).astype(np.int64), TW - 1)
                    ify = np.minimum(np.floor(np.where(hit, fy, F(0))).astype(np.int64), TW - 1)
                    fw = table[ify, ifx]
                    for c in range(3):
                        acc[c] = np.where(hit, acc[c] + lw[c][qyc, qxc, s] * fw, acc[c])
                    wsum = np.where(hit, wsum + fw, wsum)
    return np.moveaxis(acc, 0, -1).copy(), wsum


def write_image(tile_rgb, tile_w, scale=1.0):
    """MergeFilmTile into a zeroed Film::Pixel, then WriteImage with no splats (film.cpp:117-130, 169-203)"""
    a0, a1, a2 = (tile_rgb[..., c].astype(F) for c in range(3))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x0 = F(0) + (F(0.412453) * a0 + F(0.357580) * a1 + F(0.180423) * a2)
        x1 = F(0) + (F(0.212671) * a0 + F(0.715160) * a1 + F(0.072169) * a2)
        x2 = F(0) + (F(0.019334) * a0 + F(0.119193) * a1 + F(0.950227) * a2)
        w = F(0) + tile_w.astype(F)
        r = [F(3.240479) * x0 - F(1.537150) * x1 - F(0.498535) * x2,
             F(-0.969256) * x0 + F(1.875991) * x1 + F(0.041556) * x2,
             F(0.055648) * x0 - F(0.204043) * x1 + F(1.057311) * x2]
        nz = w != F(0)
        inv = F(1) / np.where(nz, w, F(1))
        out = []
        for v in r:
            v = np.where(nz, _max0(v * inv), v).astype(F)
            out.append(((v + F(0)) * F(scale)).astype(F))
    return np.stack(out, axis=-1)


def film(pfilm, colour, origin, pixel_bounds, rx, ry, table, ray_weight=None, max_sample_luminance=np.inf, scale=1.0):
    """the whole step: (contribSum, filterWeightSum, image, clamped-sample count)"""
    lw, n_clamped = prepare(colour, ray_weight, max_sample_luminance)
    t, w = splat(pfilm, lw, origin, pixel_bounds, rx, ry, table)
    return t, w, write_image(t, w, scale), n_clamped
