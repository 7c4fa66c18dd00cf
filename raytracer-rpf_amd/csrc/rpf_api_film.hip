// rpf_api_film.hip -- the host half of the film step (kernels: rpf_film.hip): the gather window, set-up and refusals,
// pbrt's filter tables (pure fp32 host arithmetic), and the entry points rpf_film_filter_table, rpf_film_window,
// rpf_filter_film, rpf_film_splat_device.  rpf_api_multi.hip runs the same step slab by slab (rpf_multi_filter_film) through
// the helpers rpf_api.h declares.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "rpf_api.h"

using namespace rpf;

namespace {

// Window of the gather.  A sample of buffer pixel q (raster) has pFilm in [q, q+1], so d = fl(pFilm - 0.5) lies in
// [q - 0.5, q + 0.5] (both ends are floats for |q| <= 2^22, and rounding is monotone).  It touches output pixel x iff
// fl(d - r) <= x (Ceil(d - r) <= x) and fl(d + r) >= x (Floor(d + r) >= x).  fl is monotone, so a q can touch x only if
// fl(q - 0.5 - r) <= x and fl(q + 0.5 + r) >= x.  In exact arithmetic that is |q - x| <= k = floor(r + 0.5).  For
// |q - x| = k + 1 the exact value misses x by g = (k + 1) - (r + 0.5) > 0 (computed exactly in double), and rounding can
// close that gap only when g is within half an ulp of the result, whose magnitude is at most M: half an ulp(M) <= M 2^-24.
// So the half-width is k, or k + 1 when g <= M 2^-23 (margin 2x); |q - x| >= k + 2 misses by g + 1 > 1.  DESIGN.md
// section 10 walks through it; box r = 1.5 - 2^-23 with pixels from 2 on is a case that needs the k + 1.
int film_window(float r, double M) {
    const double k = std::floor((double)r + 0.5);
    const double g = (k + 1.0) - ((double)r + 0.5);
    return (int)k + (g <= std::ldexp(M, -23) ? 1 : 0);
}

constexpr int32_t kFilmCoordMax = 1 << 22; // raster coordinates and radii: fp32 resolves half pixels (and q + 1) exactly

} // namespace

namespace rpf {

// The geometry of the film step for the buffer of d as the sample film: the refusals and the gather window, pure host
// arithmetic (no context, no device).  A refusal's text goes to `why`.
int32_t film_geometry(const rpf_desc *d, const rpf_film *film, FilmParams &f, std::string &why) {
    auto refuse = [&](int32_t st, const char *msg) { why = msg; return st; };
    if (!film) return refuse(RPF_E_BADARG, "film is NULL");
    if (d->row_begin != 0 || d->row_end != d->H)
        return refuse(RPF_E_BADARG, "the film step needs the whole buffer (row_begin == 0, row_end == H): a sample reaches "
                                    "pixels of the rows around it");
    if (layout_of(d).f16)
        return refuse(RPF_E_UNSUPPORTED, "the film step needs fp32 planes: an fp16 pFilm cannot place a sample inside its "
                                         "pixel beyond 2048");
    for (float r : {film->radius_x, film->radius_y})
        if (!(r > 0.f) || !std::isfinite(r) || r > (float)kFilmCoordMax)
            return refuse(RPF_E_BADARG, "filter radius must be finite, > 0 and <= 2^22");
    if (film->px1 <= film->px0 || film->py1 <= film->py0) return refuse(RPF_E_BADARG, "empty pixel bounds");
    const int64_t coords[] = {film->sample_x0, (int64_t)film->sample_x0 + d->W, film->sample_y0, (int64_t)film->sample_y0 + d->H,
                              film->px0, film->px1, film->py0, film->py1};
    int64_t m = 0;
    for (int64_t c : coords) m = std::max<int64_t>(m, c < 0 ? -c : c);
    if (m > kFilmCoordMax) return refuse(RPF_E_BADARG, "raster coordinates (sample film, pixel bounds) must lie within +-2^22");
    if ((int64_t)(film->px1 - film->px0) * (film->py1 - film->py0) >= (1ll << 31))
        return refuse(RPF_E_BADARG, "more than 2^31 output pixels");
    std::memset(&f, 0, sizeof(f));
    f.W = d->W; f.H = d->H; f.S = d->S;
    f.sx0 = film->sample_x0; f.sy0 = film->sample_y0;
    f.px0 = film->px0; f.py0 = film->py0; f.px1 = film->px1; f.py1 = film->py1;
    f.rx = film->radius_x; f.ry = film->radius_y;
    f.inv_rx = 1.f / film->radius_x; f.inv_ry = 1.f / film->radius_y; // FilmTile::invFilterRadius
    f.hx = film_window(f.rx, (double)m + f.rx + 2.0);
    f.hy = film_window(f.ry, (double)m + f.ry + 2.0);
    f.max_lum = film->max_sample_luminance;
    f.scale = film->scale;
    f.plane_stride = (uint64_t)d->W * d->H * d->S;
    return RPF_OK;
}

// the context's workspace of the film step for a buffer of f.plane_stride samples
int32_t film_ensure(rpf_ctx *ctx, const FilmParams &f) {
    int32_t st;
    if ((st = ctx->d_film_d.ensure(ctx, f.plane_stride * sizeof(float2)))) return st;
    if ((st = ctx->d_film_lw.ensure(ctx, 3 * f.plane_stride * sizeof(float)))) return st;
    if ((st = ctx->d_film_table.ensure(ctx, sizeof(rpf_film::table)))) return st;
    return ctx->d_film_bad.ensure(ctx, sizeof(unsigned long long));
}

// pFilm inside its pixel, for every sample of the buffer: *key = the first offender in the reference's order,
// (x * f.H + y) * f.S + s in buffer coordinates, or kFilmNoOffender.  Synchronises s.
int32_t film_first_offender(rpf_ctx *ctx, const FilmParams &f, const float *d_planes, hipStream_t s, unsigned long long *key) {
    HIP_TRY(hipMemsetAsync(ctx->d_film_bad, 0xff, sizeof(*key), s)); // = kFilmNoOffender
    HIP_TRY(launch_film_check(f, d_planes, ctx->d_film_bad, s));
    HIP_TRY(hipMemcpyAsync(key, ctx->d_film_bad, sizeof(*key), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return RPF_OK;
}

// the refusal's text: sample smp of buffer pixel (x, y) of the sample film of f, with its pFilm
std::string film_offender_message(const FilmParams &f, int x, int y, int smp, float pfilm_x, float pfilm_y) {
    char buf[256];
    std::snprintf(buf, sizeof(buf), "pFilm (%.9g, %.9g) of sample %d of buffer pixel (x=%d, y=%d) lies outside its raster pixel "
                  "[%d, %d] x [%d, %d] (pPixel + Get2D() stays inside it)", pfilm_x, pfilm_y, smp, x, y, f.sx0 + x, f.sx0 + x + 1,
                  f.sy0 + y, f.sy0 + y + 1);
    return buf;
}

// stage + gather; the caller has run the pFilm check on the same planes
int32_t film_splat(rpf_ctx *ctx, const FilmParams &f, const rpf_film *film, const float *d_planes, const double *d_colour,
                   const float *d_ray_weight, float *d_tile_rgb, float *d_tile_w, float *d_image, hipStream_t s) {
    Range rg("rpf:film step");
    HIP_TRY(hipMemcpyAsync(ctx->d_film_table, film->table, sizeof(film->table), hipMemcpyHostToDevice, s));
    HIP_TRY(launch_film_stage(f, d_planes, d_colour, d_ray_weight, ctx->d_film_d, ctx->d_film_lw, s));
    HIP_TRY(launch_film_splat(f, ctx->d_film_table, ctx->d_film_d, ctx->d_film_lw, d_tile_rgb, d_tile_w, d_image, s));
    return RPF_OK;
}

} // namespace rpf

namespace {

int32_t film_setup(rpf_ctx *ctx, const rpf_desc *d, const rpf_film *film, FilmParams &f) {
    std::string why;
    const int32_t st = film_geometry(d, film, f, why);
    if (st) return fail(ctx, st, why);
    return film_ensure(ctx, f);
}

// pFilm inside its pixel, for every sample (read back: the refusal names the first offender in the reference's order)
int32_t film_check(rpf_ctx *ctx, const FilmParams &f, const float *d_planes, hipStream_t s) {
    unsigned long long bad = kFilmNoOffender;
    int32_t st;
    if ((st = film_first_offender(ctx, f, d_planes, s, &bad))) return st;
    if (bad == kFilmNoOffender) return RPF_OK;
    const int smp = (int)(bad % (uint64_t)f.S), y = (int)(bad / f.S % (uint64_t)f.H), x = (int)(bad / f.S / f.H);
    const uint64_t i = ((uint64_t)y * f.W + x) * f.S + smp;
    float p[2] = {0.f, 0.f};
    HIP_TRY(hipMemcpy(&p[0], d_planes + i, sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&p[1], d_planes + f.plane_stride + i, sizeof(float), hipMemcpyDeviceToHost));
    return fail(ctx, RPF_E_BADARG, film_offender_message(f, x, y, smp, p[0], p[1]));
}

// ---- pbrt's filter table (film.cpp:66-76 and the five Evaluate()s), host fp32 -----------------------------------------
// Restated from the semantics of pbrt-v3's filters; every expression keeps pbrt's operand order and types (Float = float,
// integer literals converted to float, std::max((Float)0, v) = (0 < v) ? v : 0, std::exp / std::sin of a float = expf /
// sinf).  This TU is compiled with -ffp-contract=off, so nothing is fused.
float fmax0(float v) { return (0.f < v) ? v : 0.f; }

float mitchell_1d(float x, float B, float C) {
    x = std::fabs(2 * x);
    if (x > 1)
        return ((-B - 6 * C) * x * x * x + (6 * B + 30 * C) * x * x + (-12 * B - 48 * C) * x + (8 * B + 24 * C)) * (1.f / 6.f);
    return ((12 - 9 * B - 6 * C) * x * x * x + (-18 + 12 * B + 6 * C) * x * x + (6 - 2 * B)) * (1.f / 6.f);
}

float sinc_1d(float x) {
    const float kPi = 3.14159265358979323846f;
    x = std::fabs(x);
    if ((double)x < 1e-5) return 1;
    return std::sin(kPi * x) / (kPi * x);
}

float windowed_sinc(float x, float radius, float tau) {
    x = std::fabs(x);
    if (x > radius) return 0;
    const float lanczos = sinc_1d(x / tau);
    return sinc_1d(x) * lanczos;
}

} // namespace

extern "C" {

int32_t rpf_film_filter_table(int32_t kind, float radius_x, float radius_y, float p0, float p1, float *table_out) {
    if (!table_out) return RPF_E_BADARG;
    for (float r : {radius_x, radius_y})
        if (!(r > 0.f) || !std::isfinite(r)) return RPF_E_BADARG;
    if (kind < RPF_PIXFILTER_BOX || kind > RPF_PIXFILTER_SINC) return RPF_E_BADARG;
    // pbrt's parameter defaults: gaussian.cpp:45 alpha 2, mitchell.cpp:59-60 B = C = 1/3, sinc.cpp:56 tau 3
    const float alpha = std::isnan(p0) ? 2.f : p0;
    const float B = std::isnan(p0) ? 1.f / 3.f : p0, C = std::isnan(p1) ? 1.f / 3.f : p1;
    const float tau = std::isnan(p0) ? 3.f : p0;
    const float expX = std::exp(-alpha * radius_x * radius_x), expY = std::exp(-alpha * radius_y * radius_y);
    const float inv_rx = 1 / radius_x, inv_ry = 1 / radius_y; // Filter::invRadius
    int offset = 0;
    for (int y = 0; y < RPF_FILTER_TABLE_WIDTH; ++y) {
        for (int x = 0; x < RPF_FILTER_TABLE_WIDTH; ++x, ++offset) {
            const float px = (x + 0.5f) * radius_x / RPF_FILTER_TABLE_WIDTH;
            const float py = (y + 0.5f) * radius_y / RPF_FILTER_TABLE_WIDTH;
            float v = 1.f; // box: Evaluate() = 1
            if (kind == RPF_PIXFILTER_TRIANGLE)
                v = fmax0(radius_x - std::fabs(px)) * fmax0(radius_y - std::fabs(py));
            else if (kind == RPF_PIXFILTER_GAUSSIAN)
                v = fmax0(float(std::exp(-alpha * px * px) - expX)) * fmax0(float(std::exp(-alpha * py * py) - expY));
            else if (kind == RPF_PIXFILTER_MITCHELL)
                v = mitchell_1d(px * inv_rx, B, C) * mitchell_1d(py * inv_ry, B, C);
            else if (kind == RPF_PIXFILTER_SINC)
                v = windowed_sinc(px, radius_x, tau) * windowed_sinc(py, radius_y, tau);
            table_out[offset] = v;
        }
    }
    return RPF_OK;
}

int32_t rpf_film_window(const rpf_desc *d, const rpf_film *film, int32_t *half_x, int32_t *half_y) {
    if (!d || d->W <= 0 || d->H <= 0 || d->S <= 0) return RPF_E_BADARG;
    FilmParams f;
    std::string why;
    const int32_t st = film_geometry(d, film, f, why);
    if (st) return st;
    if (half_x) *half_x = f.hx;
    if (half_y) *half_y = f.hy;
    return RPF_OK;
}

int32_t rpf_filter_film(rpf_ctx *ctx, const rpf_desc *d, const rpf_film *film, const void *planes, const float *ray_weight,
                        float *sample_rgb_out, float *tile_rgb_out, float *tile_weight_out, float *image_rgb_out) {
    int32_t st = enter(ctx, d, true);
    if (st) return st;
    if (!planes) return fail(ctx, RPF_E_BADARG, "planes is NULL");
    FilmParams f;
    if ((st = film_setup(ctx, d, film, f))) return st;
    hipStream_t s = ctx->stream;
    const size_t ps = f.plane_stride, npix = (size_t)(f.px1 - f.px0) * (f.py1 - f.py0);
    if ((st = ensure_outputs(ctx, d, sample_rgb_out != nullptr, false))) return st;
    const bool film_out = tile_rgb_out || tile_weight_out || image_rgb_out;
    if (film_out && (st = ctx->d_film_out.ensure(ctx, 7 * npix * sizeof(float)))) return st;
    float *d_tile = ctx->d_film_out, *d_w = d_tile + 3 * npix, *d_img = d_w + npix;
    {
        Range rg("rpf:upload");
        if ((st = upload_frame(ctx, d, planes, ray_weight, true, nullptr, s))) return st;
    }
    const float *d_planes = reinterpret_cast<const float *>(ctx->d_planes.ptr);
    if ((st = film_check(ctx, f, d_planes, s))) return st; // refused before any pass runs
    const int32_t fst = run_passes(ctx, d, ctx->d_planes, ctx->d_colA, s);
    if (fst != RPF_OK && fst != RPF_E_NONFINITE) return fst;
    if ((st = download_rows(ctx, d, ctx->d_colA, nullptr, 0, d->H, sample_rgb_out, nullptr, ps, 0, s, s, nullptr))) return st;
    if (film_out) {
        if ((st = film_splat(ctx, f, film, d_planes, ctx->d_colA, ray_weight ? ctx->d_rayw.ptr : nullptr, tile_rgb_out ? d_tile : nullptr,
                             tile_weight_out ? d_w : nullptr, image_rgb_out ? d_img : nullptr, s)))
            return st;
        if (tile_rgb_out) HIP_TRY(hipMemcpyAsync(tile_rgb_out, d_tile, 3 * npix * sizeof(float), hipMemcpyDeviceToHost, s));
        if (tile_weight_out) HIP_TRY(hipMemcpyAsync(tile_weight_out, d_w, npix * sizeof(float), hipMemcpyDeviceToHost, s));
        if (image_rgb_out) HIP_TRY(hipMemcpyAsync(image_rgb_out, d_img, 3 * npix * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return fst;
}

int32_t rpf_film_splat_device(rpf_ctx *ctx, const rpf_desc *d, const rpf_film *film, const void *d_planes,
                              const double *d_colour, const float *d_ray_weight, float *d_tile_rgb, float *d_tile_weight,
                              float *d_image_rgb, void *stream) {
    int32_t st = enter(ctx, d, false);
    if (st) return st;
    if (!d_planes || !d_colour) return fail(ctx, RPF_E_BADARG, "NULL device pointer");
    FilmParams f;
    if ((st = film_setup(ctx, d, film, f))) return st;
    hipStream_t s = (hipStream_t)stream; // NULL = the legacy default stream: ordered after the caller's own work
    const float *planes = static_cast<const float *>(d_planes);
    if ((st = film_check(ctx, f, planes, s))) return st;
    if ((st = film_splat(ctx, f, film, planes, d_colour, d_ray_weight, d_tile_rgb, d_tile_weight, d_image_rgb, s))) return st;
    HIP_TRY(hipStreamSynchronize(s));
    return RPF_OK;
}

} // extern "C"
