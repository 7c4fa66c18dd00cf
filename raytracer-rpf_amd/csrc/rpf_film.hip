// rpf_film.hip -- the film step: pbrt's FilmTile::AddSample (film.h:121-161) for every filtered sample, in the reference's
// order (rpf.cpp:783-786: buffer column x outer, row y inner, then s), followed by MergeFilmTile + WriteImage
// (film.cpp:117-130, 169-203).  Compiled with -ffp-contract=off and IEEE fp32 (denormals kept, correctly rounded division):
// every output is bit-identical to a serial fp32 evaluation of pbrt's expressions in that order.
//
// Kernels:
//   film_check_kernel  every sample's pFilm lies in [q, q+1] (q = its pixel's raster coordinate); the lowest offender in the
//                      reference's order goes to one 64-bit atomicMin
//   film_stage_kernel  per sample d = pFilm - 0.5 and L * sampleWeight after the luminance clamp (20 B), transposed to
//                      [y][s][x] so that 64 lanes at 64 consecutive output pixels read one contiguous run per candidate
//   film_splat_kernel  a GATHER: one lane per output pixel walks the sample pixels that can reach it, qx ascending, qy
//                      ascending, s ascending -- the order in which pbrt's serial loop adds to that pixel -- runs pbrt's own
//                      p0 <= x < p1 test and table lookup, and accumulates in fp32 registers.  No float atomics, so the bits
//                      do not depend on scheduling.  The window half-width (hx, hy) is proven on the host (rpf_api_film.hip
//                      film_window); the candidate test itself is pbrt's, so a wider window changes
//                      nothing but time.
#include "rpf_internal.h"

namespace rpf {

namespace {

constexpr int kTableW = RPF_FILTER_TABLE_WIDTH;
constexpr int kTileX = 64, kTileY = 4; // film_splat_kernel: one wave per output row segment of 64 pixels, four rows per workgroup

__global__ __launch_bounds__(256) void film_check_kernel(FilmParams f, const float *planes, unsigned long long *first_bad) {
    const uint32_t WS = (uint32_t)f.W * (uint32_t)f.S;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long key = ~0ull;
    if (i < f.plane_stride) {
        const uint32_t y = (uint32_t)(i / WS), r = (uint32_t)(i - (uint64_t)y * WS), x = r / (uint32_t)f.S, s = r - x * (uint32_t)f.S;
        const float qx = (float)(f.sx0 + (int)x), qy = (float)(f.sy0 + (int)y); // exact: |q| <= 2^22
        const float px = planes[i], py = planes[f.plane_stride + i];
        // NaN fails every comparison, so it is refused with the out-of-pixel samples
        const bool ok = px >= qx && px <= qx + 1.f && py >= qy && py <= qy + 1.f;
        if (!ok) key = ((uint64_t)x * (uint64_t)f.H + y) * (uint64_t)f.S + s;
    }
    if (__ballot(key != ~0ull) == 0) return;
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(key, m, 64);
        key = o < key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) atomicMin(first_bad, key);
}

__global__ __launch_bounds__(256) void film_stage_kernel(FilmParams f, const float *planes, const double *colour,
                                                         const float *ray_weight, float2 *d_stage, float *lw_stage) {
    const uint32_t WS = (uint32_t)f.W * (uint32_t)f.S;
    const uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x; // output order [y][s][x]: coalesced stores
    if (o >= f.plane_stride) return;
    const uint32_t y = (uint32_t)(o / WS), r = (uint32_t)(o - (uint64_t)y * WS), s = r / (uint32_t)f.W, x = r - s * (uint32_t)f.W;
    const uint64_t i = ((uint64_t)y * f.W + x) * f.S + s; // the planes' order [y][x][s]
    const uint64_t ps = f.plane_stride;
    // Point2f pFilmDiscrete = pFilm - Vector2f(0.5f, 0.5f)
    d_stage[o] = make_float2(planes[i] - 0.5f, planes[ps + i] - 0.5f);
    // SampleData::getL (sd.h:102-110): the fp64 colour rounded to Float
    float L0 = (float)colour[i], L1 = (float)colour[ps + i], L2 = (float)colour[2 * ps + i];
    // if (L.y() > maxSampleLuminance) L *= maxSampleLuminance / L.y();   y() = spectrum.h:463-464
    const float lum = 0.212671f * L0 + 0.715160f * L1 + 0.072169f * L2;
    if (lum > f.max_lum) {
        const float k = f.max_lum / lum;
        L0 = L0 * k; L1 = L1 * k; L2 = L2 * k;
    }
    // L * sampleWeight * filterWeight evaluates left to right: the first product is per sample
    const float sw = ray_weight ? ray_weight[i] : 1.f;
    lw_stage[o] = L0 * sw;
    lw_stage[ps + o] = L1 * sw;
    lw_stage[2 * ps + o] = L2 * sw;
}

// pbrt's std::max((Float)0, v): (0 < v) ? v : 0 -- a NaN becomes 0, unlike fmaxf's
__device__ inline float max0(float v) { return (0.f < v) ? v : 0.f; }

__global__ __launch_bounds__(256) void film_splat_kernel(FilmParams f, const float *table, const float2 *d_stage,
                                                         const float *lw_stage, float *tile_rgb, float *tile_w,
                                                         float *image_rgb) {
    __shared__ float tab[kTableW * kTableW];
    tab[threadIdx.x] = table[threadIdx.x]; // 256 threads, 256 entries
    __syncthreads();
    const int nx = f.px1 - f.px0, ny = f.py1 - f.py0;
    const int tiles_x = (nx + kTileX - 1) / kTileX;
    const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)(blockIdx.x / (unsigned)tiles_x);
    const int X = f.px0 + tx * kTileX + (int)(threadIdx.x & 63);
    const int Y = f.py0 + ty * kTileY + (int)(threadIdx.x >> 6); // one wave = one output row: qy loops are wave-uniform
    if (X >= f.px1 || Y >= f.py1) return;
    const float Xf = (float)X, Yf = (float)Y;
    const int bx = X - f.sx0, by = Y - f.sy0; // buffer coordinates of the output pixel (may lie outside the buffer)
    const uint64_t ps = f.plane_stride, W = (uint64_t)f.W;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, wsum = 0.f; // FilmTilePixel: contribSum, filterWeightSum
    for (int qx = bx - f.hx; qx <= bx + f.hx; ++qx) {
        if (qx < 0 || qx >= f.W) continue;
        for (int qy = by - f.hy; qy <= by + f.hy; ++qy) {
            if (qy < 0 || qy >= f.H) continue;
            uint64_t o = (uint64_t)qy * f.S * W + (uint64_t)qx;
            for (int s = 0; s < f.S; ++s, o += W) {
                const float2 d = d_stage[o];
                // p0 = Ceil(pFilmDiscrete - filterRadius), p1 = Floor(pFilmDiscrete + filterRadius) + 1; X in [p0, p1)
                // (the clip of p0 / p1 to the pixel bounds cannot change the answer for an X inside them)
                const int p0x = (int)ceilf(d.x - f.rx), p1x = (int)floorf(d.x + f.rx) + 1;
                const int p0y = (int)ceilf(d.y - f.ry), p1y = (int)floorf(d.y + f.ry) + 1;
                if (p0x <= X && X < p1x && p0y <= Y && Y < p1y) {
                    const float fx = fabsf((Xf - d.x) * f.inv_rx * (float)kTableW);
                    const float fy = fabsf((Yf - d.y) * f.inv_ry * (float)kTableW);
                    const int ifx = min((int)floorf(fx), kTableW - 1), ify = min((int)floorf(fy), kTableW - 1);
                    const float fw = tab[ify * kTableW + ifx];
                    a0 = a0 + lw_stage[o] * fw;
                    a1 = a1 + lw_stage[ps + o] * fw;
                    a2 = a2 + lw_stage[2 * ps + o] * fw;
                    wsum = wsum + fw;
                }
            }
        }
    }
    const uint64_t t = (uint64_t)(Y - f.py0) * (uint64_t)nx + (uint64_t)(X - f.px0);
    if (tile_rgb) {
        tile_rgb[t * 3 + 0] = a0;
        tile_rgb[t * 3 + 1] = a1;
        tile_rgb[t * 3 + 2] = a2;
    }
    if (tile_w) tile_w[t] = wsum;
    if (image_rgb) {
        // MergeFilmTile: contribSum.ToXYZ (RGBToXYZ, spectrum.h:62-66) added to a zeroed Film::Pixel
        const float x0 = 0.f + (0.412453f * a0 + 0.357580f * a1 + 0.180423f * a2);
        const float x1 = 0.f + (0.212671f * a0 + 0.715160f * a1 + 0.072169f * a2);
        const float x2 = 0.f + (0.019334f * a0 + 0.119193f * a1 + 0.950227f * a2);
        const float w = 0.f + wsum;
        // WriteImage: XYZToRGB (spectrum.h:56-60), normalise by the weight sum, add the (empty) splat, scale
        float r0 = 3.240479f * x0 - 1.537150f * x1 - 0.498535f * x2;
        float r1 = -0.969256f * x0 + 1.875991f * x1 + 0.041556f * x2;
        float r2 = 0.055648f * x0 - 0.204043f * x1 + 1.057311f * x2;
        if (w != 0.f) {
            const float inv = 1.f / w;
            r0 = max0(r0 * inv); r1 = max0(r1 * inv); r2 = max0(r2 * inv);
        }
        // rgb += splatScale * XYZToRGB(splatXYZ): 1 * (+0) with no splats -- it still turns a -0 into +0
        r0 = r0 + 0.f; r1 = r1 + 0.f; r2 = r2 + 0.f;
        image_rgb[t * 3 + 0] = r0 * f.scale;
        image_rgb[t * 3 + 1] = r1 * f.scale;
        image_rgb[t * 3 + 2] = r2 * f.scale;
    }
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + 255) / 256); }

} // namespace

hipError_t launch_film_check(const FilmParams &f, const float *planes, unsigned long long *first_bad, hipStream_t s) {
    hipLaunchKernelGGL(film_check_kernel, dim3(blocks_for(f.plane_stride)), dim3(256), 0, s, f, planes, first_bad);
    return hipGetLastError();
}

hipError_t launch_film_stage(const FilmParams &f, const float *planes, const double *colour, const float *ray_weight,
                             float2 *d_stage, float *lw_stage, hipStream_t s) {
    hipLaunchKernelGGL(film_stage_kernel, dim3(blocks_for(f.plane_stride)), dim3(256), 0, s, f, planes, colour, ray_weight,
                       d_stage, lw_stage);
    return hipGetLastError();
}

hipError_t launch_film_splat(const FilmParams &f, const float *table, const float2 *d_stage, const float *lw_stage,
                             float *tile_rgb, float *tile_w, float *image_rgb, hipStream_t s) {
    const uint64_t tiles = (uint64_t)((f.px1 - f.px0 + kTileX - 1) / kTileX) * (uint64_t)((f.py1 - f.py0 + kTileY - 1) / kTileY);
    hipLaunchKernelGGL(film_splat_kernel, dim3((unsigned)tiles), dim3(kTileX * kTileY), 0, s, f, table, d_stage, lw_stage,
                       tile_rgb, tile_w, image_rgb);
    return hipGetLastError();
}

} // namespace rpf
