// rpf_api_spike.hip -- the host half of the spike pass (kernels: rpf_spike.hip; definition: DESIGN.md section 12): the
// parameters, the two halves (clamp with its row sums; add), the fold of the row sums into E and delta (rpf_spike_delta, the one
// function both the one-context path and rpf_api_multi.hip use), and the pass run_passes appends to a call with
// RPF_FLAG_SPIKE_CLAMP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "rpf_api.h"

using namespace rpf;

namespace rpf {

int32_t spike_check_params(double threshold, int32_t preserve_energy, std::string &why) {
    if (!std::isfinite(threshold) || !(threshold > 0.0)) {
        why = "spike threshold must be finite and > 0";
        return RPF_E_BADARG;
    }
    if (preserve_energy != 0 && preserve_energy != 1) {
        why = "preserve_energy must be 0 or 1";
        return RPF_E_BADARG;
    }
    return RPF_OK;
}

// The clamp half on rows [row_begin, row_end) of d: spikes replaced in d_colour, the per-row sums of the removed energy in
// row_sums (host, [rows][3]), the three counts in *stats (its other fields are left alone).  One read-back; synchronises s.
int32_t spike_clamp(rpf_ctx *ctx, const rpf_desc *d, double *d_colour, double threshold, double *row_sums, rpf_spike_stats *stats,
                    hipStream_t s) {
    const int rows = d->row_end - d->row_begin;
    if (stats) stats->spike_samples = stats->spike_pixels = stats->skipped_pixels = 0;
    if (rows <= 0) return RPF_OK;
    Range rg("rpf:spike clamp + row sums");
    int32_t st;
    if ((st = ctx->d_spike_e.ensure(ctx, (size_t)rows * d->W * 3 * sizeof(double)))) return st;
    if ((st = ctx->d_spike_rows.ensure(ctx, (size_t)rows * 3 * sizeof(double)))) return st;
    if ((st = ctx->d_spike_cnt.ensure(ctx, 3 * sizeof(unsigned long long)))) return st;
    unsigned long long cnt[3] = {0, 0, 0};
    HIP_TRY(hipMemsetAsync(ctx->d_spike_cnt, 0, sizeof(cnt), s));
    HIP_TRY(launch_spike_clamp(d_colour, d->W, d->H, d->S, d->row_begin, d->row_end, threshold, ctx->d_spike_e, ctx->d_spike_cnt, s));
    HIP_TRY(launch_spike_row_sums(ctx->d_spike_e, rows, d->W, ctx->d_spike_rows, s));
    HIP_TRY(hipMemcpyAsync(row_sums, ctx->d_spike_rows, (size_t)rows * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(cnt, ctx->d_spike_cnt, sizeof(cnt), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (stats) {
        stats->spike_samples = (int64_t)cnt[0];
        stats->spike_pixels = (int64_t)cnt[1];
        stats->skipped_pixels = (int64_t)cnt[2];
    }
    return RPF_OK;
}

// The add half: c += delta[k] on rows [row_begin, row_end) of d; all three channels or, when every delta is 0, none.  Queued on s.
int32_t spike_add(rpf_ctx *ctx, const rpf_desc *d, double *d_colour, const double delta[3], hipStream_t s) {
    if (delta[0] == 0.0 && delta[1] == 0.0 && delta[2] == 0.0) return RPF_OK;
    Range rg("rpf:spike energy add");
    HIP_TRY(launch_spike_add(d_colour, d->W, d->H, d->S, d->row_begin, d->row_end, delta, s));
    return RPF_OK;
}

// The pass of a call with RPF_FLAG_SPIKE_CLAMP on one context: clamp, fold, add; the context's stats.  The fold costs one small
// read-back and a synchronisation of s inside a call that drains its stream before it returns anyway.
int32_t spike_pass(rpf_ctx *ctx, const rpf_desc *d, double *d_colour, hipStream_t s) {
    const bool timing = (d->flags & RPF_FLAG_TIMING) != 0;
    const int rows = d->row_end - d->row_begin;
    rpf_spike_stats st_{};
    st_.applied = 1;
    int32_t st;
    if (timing) HIP_TRY(hipEventRecord(ctx->ev[1], s));
    std::vector<double> row_sums((size_t)std::max(rows, 0) * 3);
    if ((st = spike_clamp(ctx, d, d_colour, ctx->spike_threshold, row_sums.data(), &st_, s))) return st;
    if (rows > 0) {
        (void)rpf_spike_delta(row_sums.data(), rows, (int64_t)rows * d->W * d->S, st_.energy, st_.delta);
        if (ctx->spike_energy && (st = spike_add(ctx, d, d_colour, st_.delta, s))) return st;
    }
    if (timing) {
        HIP_TRY(hipEventRecord(ctx->ev[2], s));
        HIP_TRY(hipEventSynchronize(ctx->ev[2]));
        HIP_TRY(hipEventElapsedTime(&st_.spike_ms, ctx->ev[1], ctx->ev[2]));
    }
    ctx->spike = st_;
    return RPF_OK;
}

} // namespace rpf

extern "C" {

int32_t rpf_spike_delta(const double *row_sums, int64_t n_rows, int64_t n_samples, double *energy_out, double *delta_out) {
    if (!row_sums || !energy_out || !delta_out || n_rows <= 0 || n_samples <= 0) return RPF_E_BADARG;
    for (int k = 0; k < 3; ++k) {
        double e = row_sums[k];
        for (int64_t y = 1; y < n_rows; ++y) e = e + row_sums[y * 3 + k];
        energy_out[k] = e;
        delta_out[k] = e / (double)n_samples;
    }
    return RPF_OK;
}

int32_t rpf_set_spike(rpf_ctx *ctx, double threshold, int32_t preserve_energy) {
    if (!ctx) return RPF_E_BADARG;
    std::string why;
    const int32_t st = spike_check_params(threshold, preserve_energy, why);
    if (st) return fail(ctx, st, why);
    ctx->spike_threshold = threshold;
    ctx->spike_energy = preserve_energy;
    return RPF_OK;
}

int32_t rpf_query_spike(rpf_ctx *ctx, rpf_spike_stats *out) {
    if (!ctx || !out) return RPF_E_BADARG;
    *out = ctx->spike;
    return RPF_OK;
}

int32_t rpf_spike_clamp_device(rpf_ctx *ctx, const rpf_desc *d, double *d_colour, double threshold, double *row_sums_out,
                               rpf_spike_stats *stats_out, void *stream) {
    int32_t st = enter(ctx, d, false);
    if (st) return st;
    if (!d_colour || !row_sums_out) return fail(ctx, RPF_E_BADARG, "NULL pointer");
    std::string why;
    if ((st = spike_check_params(threshold, 1, why))) return fail(ctx, st, why);
    hipStream_t s = (hipStream_t)stream; // NULL = the legacy default stream: ordered after the caller's own work
    rpf_spike_stats ss{};
    ss.applied = 1;
    if ((st = spike_clamp(ctx, d, d_colour, threshold, row_sums_out, &ss, s))) return st;
    const int rows = d->row_end - d->row_begin;
    if (rows > 0) (void)rpf_spike_delta(row_sums_out, rows, (int64_t)rows * d->W * d->S, ss.energy, ss.delta);
    if (stats_out) *stats_out = ss;
    return RPF_OK;
}

int32_t rpf_colour_add_device(rpf_ctx *ctx, const rpf_desc *d, double *d_colour, const double *delta, void *stream) {
    int32_t st = enter(ctx, d, false);
    if (st) return st;
    if (!d_colour || !delta) return fail(ctx, RPF_E_BADARG, "NULL pointer");
    hipStream_t s = (hipStream_t)stream; // NULL = the legacy default stream: ordered after the caller's own work
    if ((st = spike_add(ctx, d, d_colour, delta, s))) return st;
    HIP_TRY(hipStreamSynchronize(s));
    return RPF_OK;
}

} // extern "C"
