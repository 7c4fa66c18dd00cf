// rpf_api_report.hip -- the host half of the per-pass activity report (kernels: rpf_report.hip; definition: DESIGN.md section
// 16): the scratch planes a pass with RPF_FLAG_PASS_REPORT writes alpha, beta and W_r_c into, the row records of one pass
// (report_rows: launch, one read-back), the fold of the rows (rpf_pass_report_fold, the one function the one-context path,
// rpf_api_multi.hip and a caller who owns the slabs all use), and the entry a pass loop files after route_pass (report_pass).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "rpf_api.h"

using namespace rpf;

static_assert(sizeof(rpf_report_row) == 920 && offsetof(rpf_report_row, sum_nbhd) == 448 && offsetof(rpf_report_row, unchanged_samples) == 536 &&
                  offsetof(rpf_report_row, alpha_zero) == 568 && offsetof(rpf_report_row, beta_zero) == 592 && offsetof(rpf_report_row, min_nbhd) == 912,
              "rpf_report_row is ABI");
static_assert(sizeof(rpf_pass_report) == 960 && offsetof(rpf_pass_report, pixels) == 24 && offsetof(rpf_pass_report, total) == 40, "rpf_pass_report is ABI");

namespace rpf {

// A call begins: no pass has reported yet
void report_clear(rpf_ctx *ctx) {
    for (int i = 0; i < RPF_MAX_BOXES; ++i) {
        ctx->report[i] = rpf_pass_report{};
        ctx->report_rows[i].clear();
    }
}

// The planes a reporting pass hands to setup_pass as its debug planes: the caller's (dev names them already) or the context's
// scratch, each [H*W] pixels and cleared on s, so that a pixel no kernel writes reads as zeros, as in rpf_filter_pass_debug
int32_t report_planes(rpf_ctx *ctx, const rpf_desc *d, rpf_debug &dev, hipStream_t s) {
    const size_t HW = (size_t)d->W * d->H, nF = (size_t)layout_of(d).nF;
    int32_t st;
    if (!dev.alpha) {
        if ((st = ctx->d_rep_alpha.ensure(ctx, HW * 3 * sizeof(double)))) return st;
        HIP_TRY(hipMemsetAsync(ctx->d_rep_alpha, 0, HW * 3 * sizeof(double), s));
        dev.alpha = ctx->d_rep_alpha;
    }
    if (!dev.beta) {
        if ((st = ctx->d_rep_beta.ensure(ctx, HW * nF * sizeof(double)))) return st;
        HIP_TRY(hipMemsetAsync(ctx->d_rep_beta, 0, HW * nF * sizeof(double), s));
        dev.beta = ctx->d_rep_beta;
    }
    if (!dev.wrc) {
        if ((st = ctx->d_rep_wrc.ensure(ctx, HW * sizeof(double)))) return st;
        HIP_TRY(hipMemsetAsync(ctx->d_rep_wrc, 0, HW * sizeof(double), s));
        dev.wrc = ctx->d_rep_wrc;
    }
    return RPF_OK;
}

// The row records of rows [row_begin, row_end) of d into rows_out (host).  One read-back; synchronises s.
int32_t report_rows(rpf_ctx *ctx, const rpf_desc *d, const double *col_in, const double *col_out, const int32_t *nbhd,
                    const double *alpha, const double *beta, const double *wrc, rpf_report_row *rows_out, hipStream_t s) {
    const int rows = d->row_end - d->row_begin;
    if (rows <= 0) return RPF_OK;
    Range rg("rpf:pass report");
    const SampleLayout lay = layout_of(d);
    if (lay.nF < 1 || lay.nF > RPF_MAX_NDIM) return fail(ctx, RPF_E_BADARG, "pass report: n_feat outside [1, RPF_MAX_NDIM]");
    int32_t st;
    if ((st = ctx->d_rep_pix.ensure(ctx, (size_t)rows * d->W * kReportPixelValues * sizeof(double)))) return st;
    if ((st = ctx->d_rep_rows.ensure(ctx, (size_t)rows * sizeof(rpf_report_row)))) return st;
    int32_t cap[RPF_REPORT_NCLASS - 1];
    for (int c = 0; c < RPF_REPORT_NCLASS - 1; ++c) cap[c] = class_capacity(c); // the bounds of the routes' size classes
    const ReportPlanes in{col_in, col_out, nbhd, alpha, beta, wrc, lay.nF};
    HIP_TRY(launch_pass_report(in, d->W, d->H, d->S, d->row_begin, d->row_end, cap, ctx->d_rep_pix, ctx->d_rep_rows, s));
    HIP_TRY(hipMemcpyAsync(rows_out, ctx->d_rep_rows, (size_t)rows * sizeof(rpf_report_row), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return RPF_OK;
}

// Pass `pass` of the call in progress has run (route_pass, its redo launch included) at `box` from col_in to col_out with the
// planes of `dev`: its row records and their fold become entry `pass` of the context.  Synchronises s.
int32_t report_pass(rpf_ctx *ctx, const rpf_desc *d, int pass, int box, const double *col_in, const double *col_out,
                    const rpf_debug &dev, hipStream_t s) {
    if (pass < 0 || pass >= RPF_MAX_BOXES) return RPF_OK;
    const int rows = std::max(d->row_end - d->row_begin, 0);
    std::vector<rpf_report_row> &rr = ctx->report_rows[pass];
    rr.assign((size_t)rows, rpf_report_row{});
    int32_t st;
    if ((st = report_rows(ctx, d, col_in, col_out, ctx->d_nbhd, dev.alpha, dev.beta, dev.wrc, rr.data(), s))) return st;
    rpf_pass_report r{};
    r.applied = 1;
    r.box = box;
    r.draws = ctx->samp_now.draws;
    r.route = ctx->last_route;
    r.rows = rows;
    r.pixels = (int64_t)rows * d->W;
    r.samples = r.pixels * d->S;
    if (rows > 0) (void)rpf_pass_report_fold(rr.data(), rows, &r.total);
    ctx->report[pass] = r;
    return RPF_OK;
}

} // namespace rpf

extern "C" {

int32_t rpf_pass_report_fold(const rpf_report_row *rows, int64_t n_rows, rpf_report_row *total_out) {
    if (!rows || !total_out || n_rows <= 0) return RPF_E_BADARG;
    rpf_report_row t = rows[0];
    constexpr int kDoubles = (int)(offsetof(rpf_report_row, sum_nbhd) / sizeof(double));
    constexpr int kCounts = (int)((offsetof(rpf_report_row, min_nbhd) - offsetof(rpf_report_row, sum_nbhd)) / sizeof(int64_t));
    double *td = reinterpret_cast<double *>(&t);
    int64_t *tc = &t.sum_nbhd;
    for (int64_t y = 1; y < n_rows; ++y) {
        const rpf_report_row &r = rows[y];
        const double *rd = reinterpret_cast<const double *>(&r);
        const int64_t *rc = &r.sum_nbhd;
        for (int i = 0; i < kDoubles; ++i) td[i] = td[i] + rd[i];
        for (int i = 0; i < kCounts; ++i) tc[i] += rc[i];
        t.min_nbhd = std::min(t.min_nbhd, r.min_nbhd);
        t.max_nbhd = std::max(t.max_nbhd, r.max_nbhd);
    }
    *total_out = t;
    return RPF_OK;
}

int32_t rpf_query_pass_report(rpf_ctx *ctx, int32_t pass, rpf_pass_report *out) {
    if (!ctx) return RPF_E_BADARG;
    if (!out || pass < 0 || pass >= RPF_MAX_BOXES) return fail(ctx, RPF_E_BADARG, "rpf_query_pass_report: out is NULL or pass outside [0, RPF_MAX_BOXES)");
    *out = ctx->report[pass];
    return RPF_OK;
}

int32_t rpf_query_pass_report_rows(rpf_ctx *ctx, int32_t pass, rpf_report_row *rows_out, int64_t n_rows) {
    if (!ctx) return RPF_E_BADARG;
    if (!rows_out || pass < 0 || pass >= RPF_MAX_BOXES)
        return fail(ctx, RPF_E_BADARG, "rpf_query_pass_report_rows: rows_out is NULL or pass outside [0, RPF_MAX_BOXES)");
    const std::vector<rpf_report_row> &rr = ctx->report_rows[pass];
    if (n_rows != (int64_t)rr.size()) return fail(ctx, RPF_E_BADARG, "rpf_query_pass_report_rows: n_rows is not the row count of that pass's report");
    if (!rr.empty()) std::memcpy(rows_out, rr.data(), rr.size() * sizeof(rpf_report_row));
    return RPF_OK;
}

int32_t rpf_pass_report_rows_device(rpf_ctx *ctx, const rpf_desc *d, const double *d_col_in, const double *d_col_out,
                                    const int32_t *d_nbhd, const double *d_alpha, const double *d_beta, const double *d_wrc,
                                    rpf_report_row *rows_out, void *stream) {
    int32_t st = enter(ctx, d, false);
    if (st) return st;
    if (!d_col_in || !d_col_out || !d_nbhd || !rows_out) return fail(ctx, RPF_E_BADARG, "NULL pointer");
    hipStream_t s = (hipStream_t)stream; // NULL = the legacy default stream: ordered after the caller's own work
    return report_rows(ctx, d, d_col_in, d_col_out, d_nbhd, d_alpha, d_beta, d_wrc, rows_out, s);
}

} // extern "C"
