// rpf_api_multi.hip -- one process, several GPUs: row slabs behind the ABI (rpf_multi_*).
// The reference's caller is one process (RPFIntegrator::Render, rpf.cpp:737-805); rpf_multi lets that one caller use
// every GPU of the node.  The image is cut into contiguous row slabs, one per entry of `devices` (an entry may repeat:
// two slabs on one GPU rehearse the multi-GPU path on a one-GPU box); slab g holds its rows plus `halo` rows of each
// neighbour, halo = max over the box list of (box-1)/2 (rpf.cpp:561).  Features never change, so their halo travels
// with the upload; colours change every pass, so before pass i >= 1 every slab's halo rows are refreshed from the
// neighbour's OWNED boundary rows with hipMemcpyPeerAsync (xGMI when peer access is available, staged otherwise; a
// plain device copy when both slabs share a GPU).  Passes run concurrently, one host thread per slab.
#include <hip/hip_runtime.h>

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
};

namespace {

struct MSlab { int a, b, ht, hb; int rows() const { return ht + (b - a) + hb; } }; // owned image rows [a,b), halo rows held

int32_t mfail(rpf_multi *m, int32_t st, const std::string &msg) {
    if (m) m->err = msg;
    return st;
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

int32_t rpf_multi_filter(rpf_multi *m, const rpf_desc *d, const void *planes_v, const float *ray_weight,
                         float *sample_rgb_out, float *pixel_rgb_out) {
    if (!m || m->ctx.empty()) return RPF_E_BADARG;
    {
        const int32_t st = validate(m->ctx[0], d, true);
        if (st != RPF_OK) return mfail(m, st, m->ctx[0]->err);
    }
    if (!planes_v) return mfail(m, RPF_E_BADARG, "planes is NULL");
    if (d->row_begin != 0 || d->row_end != d->H)
        return mfail(m, RPF_E_BADARG, "rpf_multi_filter filters the whole image (row_begin = 0, row_end = H): the slabs are its own");
    const int G = (int)m->ctx.size(), W = d->W, H = d->H, S = d->S;
    int halo = 0;
    for (int i = 0; i < d->n_box; ++i) halo = std::max(halo, (d->box_sizes[i] - 1) / 2);
    std::vector<MSlab> sl(G);
    for (int g = 0; g < G; ++g) {
        sl[g].a = (int)((int64_t)g * H / G);
        sl[g].b = (int)((int64_t)(g + 1) * H / G);
        sl[g].ht = std::min(halo, sl[g].a);
        sl[g].hb = std::min(halo, H - sl[g].b);
        if (G > 1 && sl[g].b - sl[g].a < halo)
            return mfail(m, RPF_E_BADARG, "a row slab is thinner than the halo its neighbours need (H / devices < (box-1)/2): use fewer devices");
    }
    const SampleLayout lay = layout_of(d);
    const int ND = lay.ndim();
    const size_t pb = lay.plane_bytes(), row = (size_t)W * S, ps_img = row * H;
    const char *planes = static_cast<const char *>(planes_v);
    std::vector<double *> cin(G), cout(G);
    std::vector<int32_t> status(G, RPF_OK);
    std::vector<rpf_desc> sd(G, *d);

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
        int32_t e;
        if ((e = ensure_frame(ctx, &ds, ray_weight != nullptr, true))) return e;
        if ((e = ctx->d_colB.ensure(ctx, 3 * ps * sizeof(double)))) return e;
        if ((e = ensure_outputs(ctx, &ds, sample_rgb_out != nullptr, pixel_rgb_out != nullptr))) return e;
        hipStream_t s = ctx->stream;
        const size_t o = (size_t)(q.a - q.ht) * row;
        for (int k = 0; k < ND; ++k)
            HIP_TRY(hipMemcpyAsync(ctx->d_planes + (size_t)k * ps * pb, planes + ((size_t)k * ps_img + o) * pb, ps * pb,
                                   hipMemcpyHostToDevice, s));
        if (ray_weight) HIP_TRY(hipMemcpyAsync(ctx->d_rayw, ray_weight + o, ps * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(launch_colour_from_planes(ctx->d_planes, lay.f16 != 0, ctx->d_colA, ps, s));
        if ((e = begin_call(ctx, s))) return e;
        HIP_TRY(hipStreamSynchronize(s));
        cin[g] = ctx->d_colA; cout[g] = ctx->d_colB;
        return RPF_OK;
    });
    if (st != RPF_OK) return st;

    float ms_filter = 0.f;
    int launches = 0;
    for (int i = 0; i < d->n_box; ++i) {
        const int box = d->box_sizes[i];
        // ---- colour halo refresh from the neighbours' owned rows (pass 0: the upload already carried it) ----------
        if (i > 0 && G > 1) {
            Range rg("rpf:colour halo refresh (peer copies)");
            for (int g = 0; g + 1 < G; ++g) {
                rpf_ctx *up = m->ctx[g], *dn = m->ctx[g + 1];
                const size_t ps_u = row * sl[g].rows(), ps_d = row * sl[g + 1].rows();
                const size_t hb = (size_t)sl[g].hb * row, ht = (size_t)sl[g + 1].ht * row; // == halo rows on both sides
                for (int c = 0; c < 3; ++c) {
                    // bottom halo of slab g <- first owned rows of slab g+1
                    const double *src1 = cin[g + 1] + c * ps_d + (size_t)sl[g + 1].ht * row;
                    double *dst1 = cin[g] + c * ps_u + (size_t)(sl[g].ht + sl[g].b - sl[g].a) * row;
                    // top halo of slab g+1 <- last owned rows of slab g
                    const double *src2 = cin[g] + c * ps_u + (size_t)(sl[g].ht + sl[g].b - sl[g].a) * row - ht;
                    double *dst2 = cin[g + 1] + c * ps_d;
                    hipError_t e1, e2;
                    if (up->device == dn->device) {
                        (void)hipSetDevice(up->device);
                        e1 = hipMemcpyAsync(dst1, src1, hb * sizeof(double), hipMemcpyDeviceToDevice, up->stream);
                        e2 = hipMemcpyAsync(dst2, src2, ht * sizeof(double), hipMemcpyDeviceToDevice, up->stream);
                    } else {
                        (void)hipSetDevice(up->device); // each copy is queued with its stream's device current
                        e1 = hipMemcpyPeerAsync(dst1, up->device, src1, dn->device, hb * sizeof(double), up->stream);
                        (void)hipSetDevice(dn->device);
                        e2 = hipMemcpyPeerAsync(dst2, dn->device, src2, up->device, ht * sizeof(double), dn->stream);
                    }
                    if (e1 != hipSuccess || e2 != hipSuccess)
                        return mfail(m, RPF_E_HIP, std::string("halo copy: ") + hipGetErrorString(e1 != hipSuccess ? e1 : e2));
                }
            }
            for (int g = 0; g < G; ++g) { // every copy has landed before any slab starts the pass
                (void)hipSetDevice(m->ctx[g]->device);
                if (hipStreamSynchronize(m->ctx[g]->stream) != hipSuccess) return mfail(m, RPF_E_HIP, "halo copy synchronise");
            }
        }
        // ---- the pass, all slabs concurrently ------------------------------------------------------------------------
        std::vector<float> ms(G, 0.f);
        std::vector<int> nl(G, 0);
        st = per_slab([&](int g) -> int32_t {
            rpf_ctx *ctx = m->ctx[g];
            HIP_TRY(hipSetDevice(ctx->device));
            hipStream_t s = ctx->stream;
            PassSetup pp;
            int32_t e;
            if ((e = setup_pass(ctx, &sd[g], box, ctx->d_planes, cin[g], cout[g], nullptr, pp))) return e;
            // halo rows pass through (they are refreshed from the neighbour before the next pass)
            if ((e = pass_through(ctx, &sd[g], cin[g], cout[g], 0, sd[g].H, s))) return e;
            if (i == 0) HIP_TRY(launch_pixel_stats(pp.p, s)); // stage 1a depends on the features only
            HIP_TRY(hipEventRecord(ctx->ev[0], s));
            if ((e = launch_filter_binned(ctx, pp.p, s, &nl[g]))) return e;
            HIP_TRY(hipEventRecord(ctx->ev[1], s));
            HIP_TRY(hipEventSynchronize(ctx->ev[1]));
            HIP_TRY(hipEventElapsedTime(&ms[g], ctx->ev[0], ctx->ev[1]));
            return RPF_OK;
        });
        if (st != RPF_OK) return st;
        float mx = 0.f;
        for (int g = 0; g < G; ++g) { mx = std::max(mx, ms[g]); launches += nl[g]; std::swap(cin[g], cout[g]); }
        ms_filter += mx;
    }

    // ---- reduce + download the owned rows; merge status and counters -----------------------------------------------
    rpf_counters tot{};
    tot.first_bad_pixel = -1;
    std::vector<rpf_counters> cs(G);
    st = per_slab([&](int g) -> int32_t {
        rpf_ctx *ctx = m->ctx[g];
        HIP_TRY(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        const MSlab &q = sl[g];
        int32_t e;
        if ((e = download_rows(ctx, &sd[g], cin[g], ray_weight ? ctx->d_rayw.ptr : nullptr, sd[g].row_begin, sd[g].row_end,
                               sample_rgb_out, pixel_rgb_out, ps_img, q.a, s, s, nullptr)))
            return e;
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

} // extern "C"
