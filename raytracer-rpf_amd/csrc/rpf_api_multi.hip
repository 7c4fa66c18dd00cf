// rpf_api_multi.hip -- one process, several GPUs: row slabs behind the ABI (rpf_multi_*).
// The reference's caller is one process (RPFIntegrator::Render, rpf.cpp:737-805); rpf_multi lets that one caller use
// every GPU of the node.  The image is cut into contiguous row slabs, one per entry of `devices` (an entry may repeat:
// two slabs on one GPU rehearse the multi-GPU path on a one-GPU box); slab g holds its rows plus `halo` rows of each
// neighbour, halo = max over the box list of (box-1)/2 (rpf.cpp:561).  Features never change, so their halo travels
// with the upload; colours change every pass, so before pass i >= 1 every slab's halo rows are refreshed from the
// neighbour's OWNED boundary rows with hipMemcpyPeerAsync (xGMI when peer access is available, staged otherwise; a
// plain device copy when both slabs share a GPU).  Passes run concurrently, one host thread per slab.
// rpf_multi_filter_film adds pbrt's film step (rpf_api_film.hip) on every slab: the halo deepens to the film's row half-width
// for the whole image where that is larger, the pFilm check of every slab is merged on the host before any pass, and after
// the last pass one more colour refresh feeds the unchanged film kernels, each slab's buffer described as a sample film of
// its own.  One planner (plan_halo = rpf_multi_halo_plan) gives the slabs and every halo copy.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "rpf_api.h"

using namespace rpf;

struct rpf_multi {
    std::vector<rpf_ctx *> ctx;
    std::vector<int> dev;
    std::string err;
    rpf_counters counters{};
    double spike_threshold = 1.0; // rpf_multi_set_spike
    int32_t spike_energy = 1;
    rpf_spike_stats spike{};      // the spike pass of the most recent call, merged over the slabs
    rpf_pass_report report[RPF_MAX_BOXES] = {}; // RPF_FLAG_PASS_REPORT: the passes of the most recent call, merged over the slabs
    rpf_sampling sampling{};      // rpf_multi_set_sampling: the caller's configuration (every slab adds its first image row to row_origin)
    bool sampling_set = false;
};

namespace {

struct MSlab { int a, b, ht, hb; int rows() const { return ht + (b - a) + hb; } }; // owned image rows [a,b), halo rows held
struct MCopy { int src, src_row, dst, dst_row, rows; };                            // buffer rows of slab src -> slab dst

int32_t mfail(rpf_multi *m, int32_t st, const std::string &msg) {
    if (m) m->err = msg;
    return st;
}

// The one slab / halo planner (rpf_multi_halo_plan): slab g owns image rows [g*H/G, (g+1)*H/G) and holds `depth` rows of each
// neighbour (fewer at the image's edges); `copies` refreshes every halo row from the neighbour's OWNED boundary rows, which
// is why a slab must own at least `depth` rows (it would otherwise have to forward rows it does not own).
int32_t plan_halo(int H, int G, int depth, std::vector<MSlab> &sl, std::vector<MCopy> &copies) {
    if (H <= 0 || G <= 0 || depth < 0) return RPF_E_BADARG;
    sl.resize(G);
    copies.clear();
    for (int g = 0; g < G; ++g) {
        sl[g].a = (int)((int64_t)g * H / G);
        sl[g].b = (int)((int64_t)(g + 1) * H / G);
        sl[g].ht = std::min(depth, sl[g].a);
        sl[g].hb = std::min(depth, H - sl[g].b);
        if (G > 1 && sl[g].b - sl[g].a < depth) return RPF_E_BADARG;
    }
    for (int g = 0; g + 1 < G; ++g) {
        const MSlab &up = sl[g], &dn = sl[g + 1];
        const int own_end = up.ht + (up.b - up.a); // first buffer row of slab g's bottom halo
        if (up.hb > 0) copies.push_back({g + 1, dn.ht, g, own_end, up.hb});      // bottom halo of g <- first owned rows of g+1
        if (dn.ht > 0) copies.push_back({g, own_end - dn.ht, g + 1, 0, dn.ht});  // top halo of g+1 <- last owned rows of g
    }
    return RPF_OK;
}

// the film step of rpf_multi_filter_film (null for rpf_multi_filter): the whole image's film and the caller's arrays
struct MFilm {
    const rpf_film *film;
    float *tile_rgb, *tile_w, *image_rgb;
};

// rpf_multi_filter and rpf_multi_filter_film: upload, [pFilm check], passes with the colour halo refreshed in between,
// [one more refresh and the film step on every slab], download, merged status and counters
int32_t multi_run(rpf_multi *m, const rpf_desc *d, const void *planes_v, const float *ray_weight, float *sample_rgb_out,
                  float *pixel_rgb_out, const MFilm *mf) {
    if (!m || m->ctx.empty()) return RPF_E_BADARG;
    m->spike = rpf_spike_stats{};
    for (rpf_pass_report &r : m->report) r = rpf_pass_report{};
    {
        const int32_t st = validate(m->ctx[0], d, true);
        if (st != RPF_OK) return mfail(m, st, m->ctx[0]->err);
    }
    if (!planes_v) return mfail(m, RPF_E_BADARG, "planes is NULL");
    if (d->row_begin != 0 || d->row_end != d->H)
        return mfail(m, RPF_E_BADARG, std::string(mf ? "rpf_multi_filter_film" : "rpf_multi_filter") +
                                          " filters the whole image (row_begin = 0, row_end = H): the slabs are its own");
    FilmParams fimg{}; // the film step of the whole image: its refusals, and the row half-width every slab's halo must cover
    if (mf) {
        std::string why;
        const int32_t st = film_geometry(d, mf->film, fimg, why);
        if (st != RPF_OK) return mfail(m, st, why);
    }
    const bool film_out = mf && (mf->tile_rgb || mf->tile_w || mf->image_rgb);
    const int G = (int)m->ctx.size(), W = d->W, H = d->H, S = d->S;
    int halo = 0;
    for (int i = 0; i < d->n_box; ++i) halo = std::max(halo, (d->box_sizes[i] - 1) / 2);
    const int depth = std::max(halo, mf ? fimg.hy : 0);
    std::vector<MSlab> sl;
    std::vector<MCopy> copies;
    if (plan_halo(H, G, depth, sl, copies) != RPF_OK) {
        if (!mf)
            return mfail(m, RPF_E_BADARG, "a row slab is thinner than the halo its neighbours need (H / devices < (box-1)/2): use fewer devices");
        return mfail(m, RPF_E_BADARG, "a row slab is thinner than the halo its neighbours need (H / devices < max((box-1)/2, film "
                                      "row half-width) = max(" + std::to_string(halo) + ", " + std::to_string(fimg.hy) +
                                      ")): use fewer devices");
    }
    const SampleLayout lay = layout_of(d);
    const int ND = lay.ndim();
    const size_t pb = lay.plane_bytes(), row = (size_t)W * S, ps_img = row * H;
    const char *planes = static_cast<const char *>(planes_v);
    std::vector<double *> cin(G), cout(G);
    std::vector<int32_t> status(G, RPF_OK);
    std::vector<rpf_desc> sd(G, *d);
    // Each slab's buffer as a sample film of its own: the origin moved down to the buffer's first image row, the output rows
    // clipped to the rows the slab owns (the first / last slab also takes the output rows above / below the sample film).
    // With `depth` >= fimg.hy halo rows every output pixel gathers the same samples in the same order as in the whole frame.
    // The window (hx, hy) stays the image's: pbrt's own test decides what a sample reaches, the window only bounds the walk.
    std::vector<FilmParams> fs(G, fimg);
    std::vector<unsigned long long> offender(G, kFilmNoOffender);
    if (mf)
        for (int g = 0; g < G; ++g) {
            FilmParams &f = fs[g];
            f.H = sl[g].rows();
            f.sy0 = fimg.sy0 + sl[g].a - sl[g].ht;
            f.plane_stride = row * sl[g].rows();
            f.py0 = g == 0 ? fimg.py0 : std::max(fimg.py0, fimg.sy0 + sl[g].a);
            f.py1 = g == G - 1 ? fimg.py1 : std::min(fimg.py1, fimg.sy0 + sl[g].b);
        }
    auto film_rows = [&](int g) { return film_out && fs[g].py1 > fs[g].py0; }; // a crop window elsewhere: no film work

    // ---- upload: every slab's rows (+ halo rows) of every plane; colours seeded on the device ------------------------
    auto per_slab = [&](auto &&fn) {
        std::vector<std::thread> th;
        for (int g = 0; g < G; ++g) th.emplace_back([&, g] { status[g] = fn(g); });
        for (auto &t : th) t.join();
        for (int g = 0; g < G; ++g)
            if (status[g] != RPF_OK && status[g] != RPF_E_NONFINITE) return mfail(m, status[g], "slab " + std::to_string(g) + ": " + m->ctx[g]->err);
        return (int32_t)RPF_OK;
    };
    int32_t st = per_slab([&](int g) -> int32_t {
        rpf_ctx *ctx = m->ctx[g];
        HIP_TRY(hipSetDevice(ctx->device));
        const MSlab &q = sl[g];
        const size_t ps = row * q.rows();
        rpf_desc &ds = sd[g];
        ds.H = q.rows(); ds.row_begin = q.ht; ds.row_end = q.ht + (q.b - q.a); ds.n_box = 1;
        if (m->sampling_set) { // buffer row 0 of the slab is image row a - ht: the slab draws what the whole image draws
            ctx->sampling = m->sampling;
            ctx->sampling.row_origin = m->sampling.row_origin + (q.a - q.ht);
        }
        int32_t e;
        if ((e = ensure_frame(ctx, &ds, ray_weight != nullptr, true))) return e;
        if ((e = ctx->d_colB.ensure(ctx, 3 * ps * sizeof(double)))) return e;
        if ((e = ensure_outputs(ctx, &ds, sample_rgb_out != nullptr, pixel_rgb_out != nullptr))) return e;
        if (mf && (e = film_ensure(ctx, fs[g]))) return e;
        if (film_rows(g) && (e = ctx->d_film_out.ensure(ctx, 7 * (size_t)(fs[g].px1 - fs[g].px0) * (fs[g].py1 - fs[g].py0) * sizeof(float))))
            return e;
        hipStream_t s = ctx->stream;
        const size_t o = (size_t)(q.a - q.ht) * row;
        for (int k = 0; k < ND; ++k)
            HIP_TRY(hipMemcpyAsync(ctx->d_planes + (size_t)k * ps * pb, planes + ((size_t)k * ps_img + o) * pb, ps * pb,
                                   hipMemcpyHostToDevice, s));
        if (ray_weight) HIP_TRY(hipMemcpyAsync(ctx->d_rayw, ray_weight + o, ps * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(launch_colour_from_planes(ctx->d_planes, lay.f16 != 0, ctx->d_colA, ps, s));
        if ((e = begin_call(ctx, s))) return e;
        // the pFilm check of the slab's buffer, before any pass (it synchronises s); merged below
        if (mf) { if ((e = film_first_offender(ctx, fs[g], reinterpret_cast<const float *>(ctx->d_planes.ptr), s, &offender[g]))) return e; }
        else HIP_TRY(hipStreamSynchronize(s));
        cin[g] = ctx->d_colA; cout[g] = ctx->d_colB;
        return RPF_OK;
    });
    if (st != RPF_OK) return st;

    // ---- the merged pFilm check: the first offender of the WHOLE image in the reference's order, (x * H + y) * S + s.
    // A slab's key orders its buffer by (x, local y, s); local y grows with the image's y, so each slab reports the first
    // offender among the rows it holds, and the minimum over the slabs of the re-keyed reports is the image's first.  A halo
    // row is the neighbour's sample under the same image key, so it is neither reported twice nor out of order.
    if (mf) {
        unsigned long long first = kFilmNoOffender;
        for (int g = 0; g < G; ++g) {
            if (offender[g] == kFilmNoOffender) continue;
            const uint64_t k = offender[g], rows = (uint64_t)sl[g].rows();
            const uint64_t smp = k % (uint64_t)S, yl = k / S % rows, x = k / S / rows, y = (uint64_t)(sl[g].a - sl[g].ht) + yl;
            first = std::min<unsigned long long>(first, (x * (uint64_t)H + y) * S + smp);
        }
        if (first != kFilmNoOffender) {
            const int smp = (int)(first % (uint64_t)S), y = (int)(first / S % (uint64_t)H), x = (int)(first / S / H);
            const float *pf = static_cast<const float *>(planes_v); // fp32 planes: film_geometry refused fp16
            const size_t i = ((size_t)y * W + x) * S + smp;
            return mfail(m, RPF_E_BADARG, film_offender_message(fimg, x, y, smp, pf[i], pf[ps_img + i]));
        }
    }

    // ---- colour halo refresh: every slab's halo rows from the neighbours' owned rows, one loop over the planner's copies;
    // queued on the destination slab's stream with its device current, a plain device copy when both slabs share a GPU
    auto refresh = [&]() -> int32_t {
        Range rg("rpf:colour halo refresh (peer copies)");
        for (const MCopy &k : copies) {
            rpf_ctx *src = m->ctx[k.src], *dst = m->ctx[k.dst];
            const size_t ps_s = row * sl[k.src].rows(), ps_d = row * sl[k.dst].rows(), bytes = (size_t)k.rows * row * sizeof(double);
            (void)hipSetDevice(dst->device);
            for (int c = 0; c < 3; ++c) {
                const double *from = cin[k.src] + c * ps_s + (size_t)k.src_row * row;
                double *to = cin[k.dst] + c * ps_d + (size_t)k.dst_row * row;
                const hipError_t e = src->device == dst->device
                                         ? hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToDevice, dst->stream)
                                         : hipMemcpyPeerAsync(to, dst->device, from, src->device, bytes, dst->stream);
                if (e != hipSuccess) return mfail(m, RPF_E_HIP, std::string("halo copy: ") + hipGetErrorString(e));
            }
        }
        for (int g = 0; g < G; ++g) { // every copy has landed before any slab goes on
            (void)hipSetDevice(m->ctx[g]->device);
            if (hipStreamSynchronize(m->ctx[g]->stream) != hipSuccess) return mfail(m, RPF_E_HIP, "halo copy synchronise");
        }
        return RPF_OK;
    };

    float ms_filter = 0.f;
    int launches = 0;
    const bool report = (d->flags & RPF_FLAG_PASS_REPORT) != 0;
    for (int i = 0; i < d->n_box; ++i) {
        const int box = d->box_sizes[i];
        if (i > 0 && G > 1 && (st = refresh()) != RPF_OK) return st; // pass 0: the upload already carried the halo
        // ---- the pass, all slabs concurrently ------------------------------------------------------------------------
        std::vector<float> ms(G, 0.f);
        std::vector<int> nl(G, 0);
        st = per_slab([&](int g) -> int32_t {
            rpf_ctx *ctx = m->ctx[g];
            HIP_TRY(hipSetDevice(ctx->device));
            hipStream_t s = ctx->stream;
            PassSetup pp;
            int32_t e;
            rpf_debug rep{}; // RPF_FLAG_PASS_REPORT: the pass writes alpha, beta and W_r_c into the slab context's scratch planes
            if (report && (e = report_planes(ctx, &sd[g], rep, s))) return e;
            if ((e = setup_pass(ctx, &sd[g], box, i, ctx->d_planes, cin[g], cout[g], report ? &rep : nullptr, pp))) return e;
            // halo rows pass through (they are refreshed from the neighbour before the next pass)
            if ((e = pass_through(ctx, &sd[g], cin[g], cout[g], 0, sd[g].H, s))) return e;
            if (i == 0) HIP_TRY(launch_pixel_stats(pp.p, s)); // stage 1a depends on the features only
            HIP_TRY(hipEventRecord(ctx->ev[0], s));
            if ((e = route_pass(ctx, pp.p, s, &nl[g]))) return e;
            HIP_TRY(hipEventRecord(ctx->ev[1], s));
            HIP_TRY(hipEventSynchronize(ctx->ev[1]));
            HIP_TRY(hipEventElapsedTime(&ms[g], ctx->ev[0], ctx->ev[1]));
            if (report && (e = report_pass(ctx, &sd[g], i, box, cin[g], cout[g], rep, s))) return e; // the rows the slab owns
            return RPF_OK;
        });
        if (st != RPF_OK) return st;
        if (report) { // the row records of every slab in image-row order, folded by the one-context path's function: the same bits
            std::vector<rpf_report_row> rows;
            rows.reserve((size_t)H);
            for (int g = 0; g < G; ++g) rows.insert(rows.end(), m->ctx[g]->report_rows[i].begin(), m->ctx[g]->report_rows[i].end());
            rpf_pass_report r = m->ctx[0]->report[i]; // applied, box, draws and route: the first slab's
            r.rows = (int32_t)rows.size();
            r.pixels = (int64_t)rows.size() * W;
            r.samples = r.pixels * S;
            r.total = rpf_report_row{};
            if (!rows.empty()) (void)rpf_pass_report_fold(rows.data(), (int64_t)rows.size(), &r.total);
            m->report[i] = r;
        }
        float mx = 0.f;
        for (int g = 0; g < G; ++g) { mx = std::max(mx, ms[g]); launches += nl[g]; std::swap(cin[g], cout[g]); }
        ms_filter += mx;
    }
    // ---- the spike pass (RPF_FLAG_SPIKE_CLAMP): every slab clamps the rows it owns, the host concatenates the row sums in
    // image-row order and folds them with the one-context path's function, every slab adds delta to its owned rows; the same
    // chains in the same order as one context, so the same bits.  Only then the film step's halo refresh below.
    m->spike = rpf_spike_stats{};
    if (d->flags & RPF_FLAG_SPIKE_CLAMP) {
        const bool timing = (d->flags & RPF_FLAG_TIMING) != 0;
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<double> row_sums((size_t)H * 3);
        std::vector<rpf_spike_stats> ss(G);
        st = per_slab([&](int g) -> int32_t {
            rpf_ctx *ctx = m->ctx[g];
            HIP_TRY(hipSetDevice(ctx->device));
            return spike_clamp(ctx, &sd[g], cin[g], m->spike_threshold, row_sums.data() + (size_t)sl[g].a * 3, &ss[g], ctx->stream);
        });
        if (st != RPF_OK) return st;
        rpf_spike_stats tot_s{};
        tot_s.applied = 1;
        for (int g = 0; g < G; ++g) {
            tot_s.spike_samples += ss[g].spike_samples;
            tot_s.spike_pixels += ss[g].spike_pixels;
            tot_s.skipped_pixels += ss[g].skipped_pixels;
        }
        (void)rpf_spike_delta(row_sums.data(), H, (int64_t)H * W * S, tot_s.energy, tot_s.delta);
        if (m->spike_energy) {
            st = per_slab([&](int g) -> int32_t {
                rpf_ctx *ctx = m->ctx[g];
                HIP_TRY(hipSetDevice(ctx->device));
                int32_t e;
                if ((e = spike_add(ctx, &sd[g], cin[g], tot_s.delta, ctx->stream))) return e;
                HIP_TRY(hipStreamSynchronize(ctx->stream)); // the film step's refresh reads these rows from another slab's stream
                return RPF_OK;
            });
            if (st != RPF_OK) return st;
        }
        if (timing) tot_s.spike_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        m->spike = tot_s;
    }
    // the film step reads the neighbours' FILTERED colours in its halo rows (the refresh moves `depth` >= fimg.hy rows)
    if (film_out && G > 1 && (st = refresh()) != RPF_OK) return st;

    // ---- reduce + download the owned rows, [the film step of the slab's output rows]; merge status and counters --------
    rpf_counters tot{};
    tot.first_bad_pixel = -1;
    std::vector<rpf_counters> cs(G);
    st = per_slab([&](int g) -> int32_t {
        rpf_ctx *ctx = m->ctx[g];
        HIP_TRY(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        const MSlab &q = sl[g];
        const float *d_rayw = ray_weight ? ctx->d_rayw.ptr : nullptr;
        int32_t e;
        if ((e = download_rows(ctx, &sd[g], cin[g], d_rayw, sd[g].row_begin, sd[g].row_end, sample_rgb_out, pixel_rgb_out, ps_img,
                               q.a, s, s, nullptr)))
            return e;
        if (film_rows(g)) { // the slab's rows of the caller's [py1-py0][px1-px0] arrays, straight from its own outputs
            const FilmParams &f = fs[g];
            const size_t nx = (size_t)(f.px1 - f.px0), npix = nx * (size_t)(f.py1 - f.py0), o = (size_t)(f.py0 - fimg.py0) * nx;
            float *d_tile = ctx->d_film_out, *d_w = d_tile + 3 * npix, *d_img = d_w + npix;
            if ((e = film_splat(ctx, f, mf->film, reinterpret_cast<const float *>(ctx->d_planes.ptr), cin[g], d_rayw,
                                mf->tile_rgb ? d_tile : nullptr, mf->tile_w ? d_w : nullptr, mf->image_rgb ? d_img : nullptr, s)))
                return e;
            if (mf->tile_rgb) HIP_TRY(hipMemcpyAsync(mf->tile_rgb + 3 * o, d_tile, 3 * npix * sizeof(float), hipMemcpyDeviceToHost, s));
            if (mf->tile_w) HIP_TRY(hipMemcpyAsync(mf->tile_w + o, d_w, npix * sizeof(float), hipMemcpyDeviceToHost, s));
            if (mf->image_rgb) HIP_TRY(hipMemcpyAsync(mf->image_rgb + 3 * o, d_img, 3 * npix * sizeof(float), hipMemcpyDeviceToHost, s));
        }
        const int32_t fst = finish_counters(ctx, &sd[g], d->n_box, s); // samples_filtered counts every pass; synchronises
        cs[g] = ctx->counters;
        return fst;
    });
    if (st != RPF_OK) return st;
    bool bad = false;
    for (int g = 0; g < G; ++g) {
        const rpf_counters &c = cs[g];
        tot.samples_filtered += c.samples_filtered;
        tot.sum_nbhd += c.sum_nbhd;
        tot.nonfinite_pixels += c.nonfinite_pixels;
        tot.max_nbhd = std::max(tot.max_nbhd, c.max_nbhd);
        tot.options_active |= c.options_active;
        tot.redo_pixels += c.redo_pixels;
        if (c.first_bad_pixel >= 0) { // slab-local y*W+x -> image index
            const int yl = c.first_bad_pixel / W, x = c.first_bad_pixel % W;
            const int gi = (sl[g].a - sl[g].ht + yl) * W + x;
            if (tot.first_bad_pixel < 0 || gi < tot.first_bad_pixel) tot.first_bad_pixel = gi;
        }
        bad = bad || status[g] == RPF_E_NONFINITE;
    }
    tot.filter_kernel_ms = ms_filter; // per pass: the slowest slab
    tot.filter_kernel_launches = launches;
    m->counters = tot;
    if (bad) {
        return mfail(m, RPF_E_NONFINITE, nonfinite_message(tot.first_bad_pixel % W, tot.first_bad_pixel / W, tot.nonfinite_pixels));
    }
    return RPF_OK;
}

} // namespace

extern "C" {

int32_t rpf_multi_create(rpf_multi **out, const int32_t *devices, int32_t n_devices) {
    if (!out) return RPF_E_BADARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RPF_E_NODEVICE;
    rpf_multi *m = new rpf_multi();
    *out = m; // returned even on failure so that rpf_multi_last_error() can be read
    std::vector<int> devs;
    if (devices && n_devices > 0) devs.assign(devices, devices + n_devices);
    else for (int i = 0; i < n; ++i) devs.push_back(i); // NULL / 0: every visible device
    for (int d : devs) {
        rpf_ctx *c = nullptr;
        const int32_t st = rpf_create(&c, d);
        if (st != RPF_OK) {
            const std::string e = c ? c->err : std::string("no such device");
            if (c) rpf_destroy(c);
            return mfail(m, st, "rpf_create(device " + std::to_string(d) + "): " + e);
        }
        m->ctx.push_back(c);
        m->dev.push_back(d);
    }
    // direct peer copies between neighbouring slabs where the hardware offers them (failure = staged copies: still correct)
    for (size_t g = 0; g + 1 < devs.size(); ++g) {
        const int a = devs[g], b = devs[g + 1];
        if (a == b) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, a, b) == hipSuccess && can) { (void)hipSetDevice(a); (void)hipDeviceEnablePeerAccess(b, 0); }
        if (hipDeviceCanAccessPeer(&can, b, a) == hipSuccess && can) { (void)hipSetDevice(b); (void)hipDeviceEnablePeerAccess(a, 0); }
        (void)hipGetLastError(); // "already enabled" is not an error here
    }
    return RPF_OK;
}

void rpf_multi_destroy(rpf_multi *m) {
    if (!m) return;
    for (rpf_ctx *c : m->ctx) rpf_destroy(c);
    delete m;
}

const char *rpf_multi_last_error(const rpf_multi *m) { return m ? m->err.c_str() : "multi context is NULL"; }
int32_t rpf_multi_device_count(const rpf_multi *m) { return m ? (int32_t)m->ctx.size() : 0; }

int32_t rpf_multi_set_option(rpf_multi *m, const char *name, int64_t value) {
    if (!m) return RPF_E_BADARG;
    for (rpf_ctx *c : m->ctx) {
        const int32_t st = rpf_set_option(c, name, value);
        if (st != RPF_OK) return mfail(m, st, c->err);
    }
    return RPF_OK;
}

int32_t rpf_multi_query_counters(rpf_multi *m, rpf_counters *out) {
    if (!m || !out) return RPF_E_BADARG;
    *out = m->counters;
    return RPF_OK;
}

int32_t rpf_multi_set_spike(rpf_multi *m, double threshold, int32_t preserve_energy) {
    if (!m) return RPF_E_BADARG;
    std::string why;
    const int32_t st = spike_check_params(threshold, preserve_energy, why);
    if (st) return mfail(m, st, why);
    m->spike_threshold = threshold;
    m->spike_energy = preserve_energy;
    return RPF_OK;
}

int32_t rpf_multi_set_sampling(rpf_multi *m, const rpf_sampling *cfg) {
    if (!m) return RPF_E_BADARG;
    std::string why;
    const int32_t st = check_sampling(cfg, why);
    if (st) return mfail(m, st, why);
    m->sampling = *cfg;
    m->sampling_set = true;
    for (rpf_ctx *c : m->ctx) (void)rpf_set_sampling(c, cfg); // multi_run moves each slab's row_origin
    return RPF_OK;
}

int32_t rpf_multi_set_membership(rpf_multi *m, const rpf_membership *cfg) {
    if (!m) return RPF_E_BADARG;
    std::string why;
    const int32_t st = check_membership(cfg, why);
    if (st) return mfail(m, st, why);
    for (rpf_ctx *c : m->ctx) (void)rpf_set_membership(c, cfg); // a function of the pixel alone: every slab takes it as it is
    return RPF_OK;
}

int32_t rpf_multi_set_schedule(rpf_multi *m, const rpf_schedule *cfg) {
    if (!m) return RPF_E_BADARG;
    std::string why;
    const int32_t st = check_schedule_table(cfg, why);
    if (st) return mfail(m, st, why);
    for (rpf_ctx *c : m->ctx) (void)rpf_set_schedule(c, cfg); // indexed by the pass of the call, which every slab runs: the same table
    return RPF_OK;
}

int32_t rpf_multi_query_spike(rpf_multi *m, rpf_spike_stats *out) {
    if (!m || !out) return RPF_E_BADARG;
    *out = m->spike;
    return RPF_OK;
}

int32_t rpf_multi_query_pass_report(rpf_multi *m, int32_t pass, rpf_pass_report *out) {
    if (!m) return RPF_E_BADARG;
    if (!out || pass < 0 || pass >= RPF_MAX_BOXES) return mfail(m, RPF_E_BADARG, "rpf_multi_query_pass_report: out is NULL or pass outside [0, RPF_MAX_BOXES)");
    *out = m->report[pass];
    return RPF_OK;
}

int32_t rpf_multi_filter(rpf_multi *m, const rpf_desc *d, const void *planes_v, const float *ray_weight,
                         float *sample_rgb_out, float *pixel_rgb_out) {
    return multi_run(m, d, planes_v, ray_weight, sample_rgb_out, pixel_rgb_out, nullptr);
}

int32_t rpf_multi_filter_film(rpf_multi *m, const rpf_desc *d, const rpf_film *film, const void *planes_v, const float *ray_weight,
                              float *sample_rgb_out, float *tile_rgb_out, float *tile_weight_out, float *image_rgb_out) {
    const MFilm mf{film, tile_rgb_out, tile_weight_out, image_rgb_out};
    return multi_run(m, d, planes_v, ray_weight, sample_rgb_out, nullptr, &mf);
}

int32_t rpf_multi_halo_plan(int32_t H, int32_t n_slabs, int32_t depth, int32_t *slabs_out, int32_t *copies_out,
                            int32_t *n_copies_out) {
    std::vector<MSlab> sl;
    std::vector<MCopy> copies;
    const int32_t st = plan_halo(H, n_slabs, depth, sl, copies);
    if (st != RPF_OK) return st;
    if (slabs_out)
        for (const MSlab &q : sl) { *slabs_out++ = q.a; *slabs_out++ = q.b; *slabs_out++ = q.ht; *slabs_out++ = q.hb; }
    if (copies_out)
        for (const MCopy &k : copies) {
            *copies_out++ = k.src; *copies_out++ = k.src_row; *copies_out++ = k.dst; *copies_out++ = k.dst_row; *copies_out++ = k.rows;
        }
    if (n_copies_out) *n_copies_out = (int32_t)copies.size();
    return RPF_OK;
}

} // extern "C"
