/*
 * ref_filter_harness.cpp -- runs the REAL RPFIntegrator::ApplyRPFFilter of the reference on a feature buffer read from a
 * file, once per box size, and writes the filtered sample colours.  Built by oracle/Makefile (target `ref_full`) into
 * oracle/_ref/ref_filter_harness from the reference's sources where they lie: like ref_harness.cpp this file reaches them
 * only by #include path, so it builds only where the reference tree exists, and nothing of it is copied into this
 * repository.  glog and OpenEXR are replaced by the stand-ins under oracle/ref_stub/.
 *
 * TEST INFRASTRUCTURE ONLY: used to pin oracle/rpf_oracle.c and to generate tests/golden/ref_filter.npz.
 *
 *   usage: ref_filter_harness IN OUT
 *   IN :  int32 W, H, S, n_threads, n_boxes, box[n_boxes];  float32 planes[19][H][W][S]
 *   OUT:  float64 colour[3][H][W][S]
 *
 * The film is W x H with a box pixel filter of radius 0.5 and no crop window, so Film::GetSampleBounds() is (0,0)-(W,H)
 * and buffer pixel (x, y) is the reference's samples[x][y].  The process ends with the reference's own status: the
 * reference calls exit(1) where a filtered colour is NaN ("PRIME ERROR"), which is why this is a program and not a
 * library.  Exit status 2 is this harness's own (bad arguments or files).
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

/* ApplyRPFFilter is a private member; every standard header the reference pulls in is already included above or is
 * indifferent to this */
#define private public
#define protected public
#include "custom/rpf.h"
#include "custom/sample_film.h"
#include "camera.h"
#include "film.h"
#include "filters/box.h"
#include "parallel.h"
#undef private
#undef protected

namespace pbrt {
Options PbrtOptions; /* the reference defines it in its scene-description front end, which is not linked */
}

namespace {

struct NoCamera : pbrt::Camera {
    NoCamera(pbrt::Film *film)
        : pbrt::Camera(pbrt::AnimatedTransform(&identity, 0, &identity, 1), 0, 1, film, nullptr) {}
    pbrt::Float GenerateRay(const pbrt::CameraSample &, pbrt::Ray *) const override { return 0; }
    static pbrt::Transform identity;
};
pbrt::Transform NoCamera::identity;

bool read_all(FILE *f, void *p, size_t n) { return std::fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE *in = std::fopen(argv[1], "rb");
    int32_t head[5];
    if (!in || !read_all(in, head, sizeof head)) return 2;
    const int W = head[0], H = head[1], S = head[2], n_threads = head[3], n_boxes = head[4];
    if (W < 1 || H < 1 || S < 1 || n_threads < 1 || n_boxes < 0 || n_boxes > 64) return 2;
    std::vector<int32_t> boxes(n_boxes);
    if (n_boxes && !read_all(in, boxes.data(), sizeof(int32_t) * n_boxes)) return 2;
    const size_t plane = (size_t)H * W * S;
    std::vector<float> planes(19 * plane);
    if (!read_all(in, planes.data(), sizeof(float) * planes.size())) return 2;
    std::fclose(in);

    pbrt::PbrtOptions.nThreads = n_threads;
    pbrt::PbrtOptions.quiet = true;
    pbrt::ParallelInit();
    {
        pbrt::Film *film = new pbrt::Film(pbrt::Point2i(W, H), pbrt::Bounds2f(pbrt::Point2f(0, 0), pbrt::Point2f(1, 1)),
                                          std::unique_ptr<pbrt::Filter>(new pbrt::BoxFilter(pbrt::Vector2f(0.5f, 0.5f))),
                                          35.f, "unused.pfm", 1.f);
        std::shared_ptr<const pbrt::Camera> camera(new NoCamera(film)); /* the camera owns and deletes the film */
        const pbrt::Bounds2i sb = film->GetSampleBounds();
        if (sb.pMin.x != 0 || sb.pMin.y != 0 || sb.pMax.x != W || sb.pMax.y != H) return 2;
        pbrt::RPFIntegrator integrator(5, camera, std::shared_ptr<pbrt::Sampler>(), sb);

        pbrt::SamplingFilm sf(sb);
        for (int x = 0; x < W; ++x)
            for (int y = 0; y < H; ++y)
                for (int s = 0; s < S; ++s) {
                    pbrt::SampleData sd;
                    for (int c = 0; c < 19; ++c) sd.data[c] = planes[c * plane + ((size_t)y * W + x) * S + s];
                    sd.rayWeight = 1;
                    sf.AddSample(pbrt::Point2i(x, y), sd);
                }
        for (int b = 0; b < n_boxes; ++b) integrator.ApplyRPFFilter(sf, 16, boxes[b]);

        std::vector<double> out(3 * plane);
        for (int x = 0; x < W; ++x)
            for (int y = 0; y < H; ++y) {
                const pbrt::SampleDataSet &px = sf.samples[x][y];
                if ((int)px.size() != S) return 2;
                for (int s = 0; s < S; ++s)
                    for (int c = 0; c < 3; ++c) out[c * plane + ((size_t)y * W + x) * S + s] = px[s].getColorI(c);
            }
        FILE *o = std::fopen(argv[2], "wb");
        if (!o || std::fwrite(out.data(), sizeof(double), out.size(), o) != out.size()) return 2;
        std::fclose(o);
    }
    pbrt::ParallelCleanup();
    return 0;
}
