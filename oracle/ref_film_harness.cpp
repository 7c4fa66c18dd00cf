/*
 * ref_film_harness.cpp -- drives the REAL pbrt Film of the reference (film.h / film.cpp and filters/*.cpp) the way
 * RPFIntegrator::Render does: one FilmTile over the film's sample bounds, FilmTile::AddSample for every sample in the
 * order buffer column x, row y, sample s, then Film::MergeFilmTile and Film::WriteImage.  Built by oracle/Makefile (target
 * `ref_full`) into oracle/_ref/ref_film_harness from the reference's sources where they lie; this file reaches them only
 * by #include path and builds only where the reference tree exists.  pbrt::WriteImage is defined here (the reference's
 * image writers are not linked) and keeps the RGB array Film::WriteImage hands it.
 *
 * TEST INFRASTRUCTURE ONLY: used to pin tests/pbrt_film_ref.py and the library's filter tables, and to generate
 * tests/golden/ref_film.npz.
 *
 *   usage: ref_film_harness film IN OUT
 *   IN :  int32 kind (0 box, 1 triangle, 2 gaussian, 3 mitchell, 4 windowed sinc), W, H, S, xres, yres
 *         float32 rx, ry, p0, p1 (gaussian alpha | mitchell B, C | sinc tau), crop x0, x1, y0, y1 (fractions, as the
 *         scene file gives them), maxSampleLuminance, scale
 *         float32 pFilm[2][H][W][S];  float64 colour[3][H][W][S];  float32 rayWeight[H][W][S]
 *   OUT:  int32 croppedPixelBounds x0 y0 x1 y1, sample bounds x0 y0 x1 y1, tile pixel bounds x0 y0 x1 y1
 *         float32 filterTable[16][16]
 *         float32 contribSum[ny][nx][3], filterWeightSum[ny][nx]   (the tile's pixels, before the merge)
 *         float32 image[ny'][nx'][3]                               (what Film::WriteImage passes to the image writer)
 *
 *   usage: ref_film_harness tables IN OUT
 *   IN :  int32 n;  n x { int32 kind; float32 rx, ry, p0, p1 }
 *   OUT:  n x float32 filterTable[16][16]
 */
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <iterator>
#include <limits>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <sstream>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#define private public /* Film::filterTable and FilmTile::pixels are private */
#include "film.h"
#include "filters/box.h"
#include "filters/gaussian.h"
#include "filters/mitchell.h"
#include "filters/sinc.h"
#include "filters/triangle.h"
#include "custom/sd.h"
#undef private

static std::vector<float> g_image;
static int g_image_bounds[4];

namespace pbrt {
Options PbrtOptions;
void WriteImage(const std::string &, const Float *rgb, const Bounds2i &outputBounds, const Point2i &) {
    g_image.assign(rgb, rgb + 3 * (size_t)outputBounds.Area());
    g_image_bounds[0] = outputBounds.pMin.x;
    g_image_bounds[1] = outputBounds.pMin.y;
    g_image_bounds[2] = outputBounds.pMax.x;
    g_image_bounds[3] = outputBounds.pMax.y;
}
}  // namespace pbrt

namespace {

bool read_all(FILE *f, void *p, size_t n) { return std::fread(p, 1, n, f) == n; }
bool write_all(FILE *f, const void *p, size_t n) { return std::fwrite(p, 1, n, f) == n; }

std::unique_ptr<pbrt::Filter> make_filter(int kind, float rx, float ry, float p0, float p1) {
    const pbrt::Vector2f r(rx, ry);
    switch (kind) {
    case 0: return std::unique_ptr<pbrt::Filter>(new pbrt::BoxFilter(r));
    case 1: return std::unique_ptr<pbrt::Filter>(new pbrt::TriangleFilter(r));
    case 2: return std::unique_ptr<pbrt::Filter>(new pbrt::GaussianFilter(r, p0));
    case 3: return std::unique_ptr<pbrt::Filter>(new pbrt::MitchellFilter(r, p0, p1));
    case 4: return std::unique_ptr<pbrt::Filter>(new pbrt::LanczosSincFilter(r, p0));
    }
    return nullptr;
}

void put_bounds(int32_t *d, const pbrt::Bounds2i &b) {
    d[0] = b.pMin.x; d[1] = b.pMin.y; d[2] = b.pMax.x; d[3] = b.pMax.y;
}

int tables(FILE *in, FILE *out) {
    int32_t n;
    if (!read_all(in, &n, sizeof n) || n < 0) return 2;
    for (int i = 0; i < n; ++i) {
        int32_t kind;
        float v[4];
        if (!read_all(in, &kind, sizeof kind) || !read_all(in, v, sizeof v)) return 2;
        std::unique_ptr<pbrt::Filter> f = make_filter(kind, v[0], v[1], v[2], v[3]);
        if (!f) return 2;
        pbrt::Film film(pbrt::Point2i(4, 4), pbrt::Bounds2f(pbrt::Point2f(0, 0), pbrt::Point2f(1, 1)), std::move(f), 35.f,
                        "unused.pfm", 1.f);
        if (!write_all(out, film.filterTable, sizeof film.filterTable)) return 2;
    }
    return 0;
}

int film_step(FILE *in, FILE *out) {
    int32_t hi[6];
    float hf[10];
    if (!read_all(in, hi, sizeof hi) || !read_all(in, hf, sizeof hf)) return 2;
    const int kind = hi[0], W = hi[1], H = hi[2], S = hi[3], xres = hi[4], yres = hi[5];
    if (W < 1 || H < 1 || S < 1 || xres < 1 || yres < 1) return 2;
    const size_t plane = (size_t)H * W * S;
    std::vector<float> pfilm(2 * plane), rw(plane);
    std::vector<double> colour(3 * plane);
    if (!read_all(in, pfilm.data(), sizeof(float) * pfilm.size()) ||
        !read_all(in, colour.data(), sizeof(double) * colour.size()) || !read_all(in, rw.data(), sizeof(float) * rw.size()))
        return 2;
    std::unique_ptr<pbrt::Filter> f = make_filter(kind, hf[0], hf[1], hf[2], hf[3]);
    if (!f) return 2;
    pbrt::Film film(pbrt::Point2i(xres, yres), pbrt::Bounds2f(pbrt::Point2f(hf[4], hf[6]), pbrt::Point2f(hf[5], hf[7])),
                    std::move(f), 35.f, "unused.pfm", hf[9], hf[8]);
    const pbrt::Bounds2i sb = film.GetSampleBounds();
    std::unique_ptr<pbrt::FilmTile> tile = film.GetFilmTile(sb);
    for (int x = 0; x < W; ++x)
        for (int y = 0; y < H; ++y)
            for (int s = 0; s < S; ++s) {
                const size_t i = ((size_t)y * W + x) * S + s;
                pbrt::SampleData sd; /* carries the sample as the reference's sample film does: doubles, and a Float weight */
                sd.data[0] = pfilm[i];
                sd.data[1] = pfilm[plane + i];
                for (int c = 0; c < 3; ++c) sd.data[2 + c] = colour[c * plane + i];
                sd.rayWeight = rw[i];
                tile->AddSample(sd.getPFilm(), sd.getL(), sd.rayWeight);
            }
    int32_t b[12];
    put_bounds(b, film.croppedPixelBounds);
    put_bounds(b + 4, sb);
    const pbrt::Bounds2i tb = tile->GetPixelBounds();
    put_bounds(b + 8, tb);
    std::vector<float> sums, weights;
    for (pbrt::Point2i p : tb) { /* row-major: y outer, x inner */
        const pbrt::FilmTilePixel &tp = tile->GetPixel(p);
        pbrt::Float rgb[3];
        tp.contribSum.ToRGB(rgb);
        sums.insert(sums.end(), rgb, rgb + 3);
        weights.push_back(tp.filterWeightSum);
    }
    film.MergeFilmTile(std::move(tile));
    film.WriteImage();
    if (std::memcmp(g_image_bounds, b, sizeof g_image_bounds) != 0) return 2;
    if (!write_all(out, b, sizeof b) || !write_all(out, film.filterTable, sizeof film.filterTable) ||
        !write_all(out, sums.data(), sizeof(float) * sums.size()) ||
        !write_all(out, weights.data(), sizeof(float) * weights.size()) ||
        !write_all(out, g_image.data(), sizeof(float) * g_image.size()))
        return 2;
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s film|tables IN OUT\n", argv[0]);
        return 2;
    }
    FILE *in = std::fopen(argv[2], "rb");
    FILE *out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    int rc = 2;
    if (!std::strcmp(argv[1], "film")) rc = film_step(in, out);
    if (!std::strcmp(argv[1], "tables")) rc = tables(in, out);
    std::fclose(in);
    if (std::fclose(out) != 0) rc = 2;
    return rc;
}
