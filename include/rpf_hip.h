/*
 * rpf_hip.h -- C ABI of librpf_hip.so: the MI355X (gfx950) Random Parameter Filtering pass.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference (tux550/RayTracer-RPF, a
 * pbrt-v3 fork) has no plugin ABI: its integrator calls the private member
 *     void RPFIntegrator::ApplyRPFFilter(SamplingFilm&, const int tileSize, int box_size)
 *                                                   /root/reference/src/custom/rpf.h:91-95, rpf.cpp:497-733
 * once per box size from RPFIntegrator::Render (rpf.cpp:767-775) and then reduces the filtered samples
 * into the film (rpf.cpp:779-804).  A maintainer replaces the body of ApplyRPFFilter (or the loop in
 * Render) with one call to rpf_filter(); INTEGRATION.md shows the binding.  No pbrt type crosses this
 * boundary: plain pointers, sizes and POD structs only, no exceptions, integer status codes.
 *
 * Data layout on both sides of the ABI: 19 SoA planes of fp32, plane d at base + d*H*W*S, element
 * (y, x, s) at ((y*W)+x)*S + s, dims = SampleData::data (sd.h:62-94):
 *     0,1 pFilm | 2,3,4 L rgb | 5,6 pLens | 7..9 n0 | 10..12 p0 | 13..15 n1 | 16..18 p1
 * (the reference stores the same 19 values as doubles in samples[x][y][s], sample_film.cpp:32-42; they
 * are fp32-valued because pbrt's Float is float.)  Colours travel between passes as fp64 planes on the
 * device, exactly as the reference carries them in SampleData doubles.
 *
 * Threading: one caller thread per rpf_ctx at a time; distinct contexts are independent.
 * Multi-GPU: one context per device; a context filters a ROW SLAB [row_begin,row_end) of a buffer that also holds
 * the halo rows it needs.  A strict sub-slab is filtered ONE pass per call (n_box == 1) with a colour-halo exchange
 * between passes: raytracer-rpf_amd/slabs.py does that across processes (RCCL send/recv).
 */
#ifndef RPF_HIP_H
#define RPF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPF_NDIM 19   /* the reference's sample vector (sd.h:21-49); other layouts: rpf_desc.n_random / n_feat */
#define RPF_NFEAT 12
#define RPF_NPAIR 96
#define RPF_MAX_BOXES 8
#define RPF_MAX_NDIM 40 /* widest sample vector of the layout-generic kernels (RPF_FLAG_GENERIC): 5 + n_random + n_feat */
#define RPF_SAMPLED_MAX 8192 /* the most S + draws of a sampled pass under RPF_FLAG_SAMPLED_REST (832 without it); rpf_max_draws() */
/* general layout: columns [0,2) pFilm | [2,5) colour | [5,5+nR) random parameters | [5+nR,5+nR+nF) features */
#define RPF_NDIM_OF(nR, nF) (5 + (nR) + (nF))
#define RPF_NPAIR_OF(nR, nF) ((nF) * ((nR) + 2) + 3 * ((nR) + 2 + (nF))) /* MI pairs, rpf.cpp:416-442 generalised */
enum { RPF_PLANES_F32 = 0, RPF_PLANES_F16 = 1 };

typedef struct rpf_ctx rpf_ctx;

/* status codes; replaces the reference's exit(1) on NaN (rpf.cpp:702-705) and its silent preconditions */
typedef enum rpf_status {
    RPF_OK = 0,
    RPF_E_BADARG = 1,      /* malformed descriptor / NULL pointer / even box / S<=0 ...            */
    RPF_E_HIP = 2,         /* a HIP runtime call failed; text in rpf_last_error()                  */
    RPF_E_NONFINITE = 3,   /* REF_ABORT policy: a filtered colour came out NaN (reference aborts)  */
    RPF_E_NOMEM = 4,
    RPF_E_UNSUPPORTED = 5, /* neighbourhood too large (box*box*S > 65535, or its LDS working set); a sample layout
                              without compiled kernels and without RPF_FLAG_GENERIC, or outside that flag's bounds */
    RPF_E_NODEVICE = 6
} rpf_status;

/* which D term feeds W_c_fk[k] for k = 0..11.  rpf.cpp:464 indexes the 3-element D_f_ck with k < 12
 * (undefined behaviour); the presets name what each build of the reference reads. */
typedef enum rpf_beta_map {
    RPF_BETA_REF_GCC11_O3 = 0, /* {Dfc[0..2], 0, Drf[0..7]}         g++ 11.4 -O3 (CMake Release)   */
    RPF_BETA_REF_GCC11_O2 = 1, /* {Dfc[0..2], 0,0,0,0,0, Drf[0..3]} g++ 11.4 -O0/-O2               */
    RPF_BETA_PAPER = 2         /* sum_c MI(c_c, f_k): the formula in the comment at rpf.cpp:459    */
} rpf_beta_map;

typedef enum rpf_degenerate_policy {
    RPF_DEGEN_REF_ABORT = 0, /* IEEE propagation exactly as the reference; NaN colour => RPF_E_NONFINITE */
    RPF_DEGEN_EPS = 1        /* documented deviation: +eps in the three denominators of rpf.cpp:464-470,
                                negative variances clamped to 0, NaN colours fall back to the input    */
} rpf_degenerate_policy;

enum {
    RPF_FLAG_NONE = 0,
    RPF_FLAG_TIMING = 1,       /* bracket kernels with hipEvents (rpf_query_counters) */
    RPF_FLAG_FAST_WEIGHTS = 2, /* opt-in: the S x N pair weights of stage 4 (rpf.cpp:637-678) are evaluated in fp32 on
                                  fp64-formed normalised values, with the hardware exp; everything that decides
                                  discrete outcomes (membership, bins, MI) is unchanged.  Colours move by ~1e-6
                                  relative (bar 1e-4).  Default off: fp64 throughout, like the reference.
                                  Two kinds of pixel are filtered in fp64 under the flag as well: a neighbourhood above 3136
                                  samples (the streaming kernel), and, under RPF_DEGEN_REF_ABORT, a pixel on the redo list
                                  (rpf_counters.redo_pixels), which the reference-expression kernel filters whole.
                                  The fp32 kernels exist for the reference's 19-dim layout (n_random = 2, n_feat = 12,
                                  fp32 planes) only: with any other layout the flag is RPF_E_UNSUPPORTED, from every
                                  filter entry point and from rpf_layout_kernels, before any device work. */
    RPF_FLAG_NO_OVERLAP = 4,   /* rpf_filter(): upload, filter and download one after the other instead of the
                                  row-band pipeline (same results; for A/B timing).  RPF_FLAG_TIMING implies it. */
    RPF_FLAG_GENERIC = 8,      /* opt-in: run this call on the layout-generic kernels, which take n_random / n_feat as run-time
                                  values: n_random >= 1, n_feat >= 1, 5 + n_random + n_feat <= RPF_MAX_NDIM, fp32 or fp16
                                  planes, neighbourhoods up to 65535 samples.  REQUIRED for a layout without compiled kernels
                                  (without it such a descriptor stays RPF_E_UNSUPPORTED: the refusal also tells a caller that
                                  a layout was mis-declared, and this route is several times slower than the fused kernels);
                                  ALLOWED for the two compiled layouts, where it selects the generic kernels instead of the
                                  fused routes (A/B timing, parity).  fp64 throughout: together with RPF_FLAG_FAST_WEIGHTS
                                  it is RPF_E_UNSUPPORTED.  One filter launch per pass; rpf_query_route says 3. */
    RPF_FLAG_GENERIC_PACKED = 16, /* opt-in, modifies RPF_FLAG_GENERIC: the pixels whose neighbourhood holds N <= 64 samples
                                  (about 94 % of a path-traced buffer) run on the packed layout-generic kernels -- a pixel gets
                                  8, 16, 32 or 64 lanes of a wavefront instead of a 256-thread workgroup -- behind a count
                                  pass of their own; the other pixels stay on the generic filter kernel.  Same layouts as the
                                  generic flag, the two compiled ones included.  Same membership, bins, statistics, MI, alpha,
                                  beta and W_r_c as under the generic flag alone; the colours agree to rounding.
                                  rpf_query_route says 4 (3 for a pass with S > 64, which no packed class can hold and which
                                  runs exactly as without this flag).  Without RPF_FLAG_GENERIC, or together with
                                  RPF_FLAG_FAST_WEIGHTS, it is RPF_E_UNSUPPORTED, from every filter entry point and from
                                  rpf_layout_kernels, before any device work. */
    RPF_FLAG_GENERIC_WAVE = 32, /* opt-in, modifies RPF_FLAG_GENERIC | RPF_FLAG_GENERIC_PACKED: the pixels whose neighbourhood
                                  holds 64 < N <= 832 samples run on the one-wave layout-generic kernels -- one wavefront per
                                  pixel, no workgroup barrier, size classes N <= 128, 256, 448 and 832 with LDS sized for the
                                  class -- behind the count pass of the packed flag; only N > 832 stays on the generic filter
                                  kernel.  Same layouts as the generic flag.  Same membership, bins, statistics, MI, alpha,
                                  beta and W_r_c as under the generic flag alone; the colours agree to rounding.
                                  rpf_query_route says 5 (3 for a pass with S > 832, which no class can hold and which runs
                                  exactly as under RPF_FLAG_GENERIC alone; a pass with 64 < S <= 832 is route 5 with empty
                                  packed classes).  Without both RPF_FLAG_GENERIC and RPF_FLAG_GENERIC_PACKED, or together
                                  with RPF_FLAG_FAST_WEIGHTS, it is RPF_E_UNSUPPORTED, from every filter entry point and from
                                  rpf_layout_kernels, before any device work. */
    RPF_FLAG_WIDE_NBHD = 64,   /* opt-in: passes with 65535 < box*box*S <= 262144 (the reference's box list {55, 35, 17, 7} at
                                  32 spp: 55*55*32 = 96800) are accepted and run on the wide layout-generic kernel -- 16-bit bin
                                  ids, 32-bit histogram cells built in bands of rows, MI from a table of k ln k in 2^-41 fixed
                                  point.  Every pixel of such a pass runs on that kernel: one launch per pass,
                                  rpf_query_route says 6, redo_pixels is 0 (the reference's MI expression is evaluated in
                                  place).  A pass of the same call with box*box*S <= 65535 runs exactly as without the flag:
                                  same route, same bits.  Above 262144 a pass stays RPF_E_UNSUPPORTED; rpf_max_nbhd() tells the
                                  bound.  The two compiled layouts take the flag without RPF_FLAG_GENERIC, any other layout
                                  needs RPF_FLAG_GENERIC as before; RPF_FLAG_GENERIC_PACKED / RPF_FLAG_GENERIC_WAVE are accepted
                                  alongside and do not affect a wide pass.  fp64 throughout: together with
                                  RPF_FLAG_FAST_WEIGHTS it is RPF_E_UNSUPPORTED, from every filter entry point and from
                                  rpf_layout_kernels, before any device work. */
    RPF_FLAG_WIDE_CLASSES = 128, /* opt-in, modifies RPF_FLAG_WIDE_NBHD: a wide pass (box*box*S > 65535, or option "wide" = 1) is
                                  counted first and dealt by neighbourhood size -- a count kernel of its own lists the members
                                  of every pixel with N <= 832 (no acceptance masks: the extra memory is O(pixels) plus the sum
                                  of the listed N) and proves N = S without a walk for a pixel with a zero-variance feature --
                                  and the packed (N <= 8, 16, 32, 64) and one-wave (N <= 128, 256, 448, 832) layout-generic
                                  kernels take those pixels; only N > 832 stays on the wide kernel.  Same membership, bins,
                                  statistics, N and counters sum_nbhd / max_nbhd as under the wide flag alone; MI, alpha, beta
                                  and W_r_c agree to the rounding of the two k ln k tables, the colours to rounding.
                                  rpf_query_route says 7 (6 for a wide pass with S > 832, which no class can hold and which
                                  runs exactly as without this flag).  Every other pass of the call runs exactly as without
                                  the flag.  It needs neither RPF_FLAG_GENERIC_PACKED nor RPF_FLAG_GENERIC_WAVE, which keep
                                  steering the non-wide passes only.  Without RPF_FLAG_WIDE_NBHD it is RPF_E_UNSUPPORTED, from
                                  every filter entry point and from rpf_layout_kernels, before any device work. */
    RPF_FLAG_GENERIC_FAST = 256, /* opt-in, modifies RPF_FLAG_GENERIC | RPF_FLAG_GENERIC_PACKED (with or without
                                  RPF_FLAG_GENERIC_WAVE): on a pass that takes route 4 or 5 the packed kernels (N <= 64) and,
                                  with the wave flag, the one-wave kernels (64 < N <= 832) evaluate the S x N pair weights of
                                  stage 4 in fp32 -- z = (x - M) / SD and the 5 + n_feat coefficients formed in fp64 and rounded
                                  once, differences, squares and the weighted sum in fp32, ONE hardware exponential of the
                                  summed exponent, the weights widened to fp64, both sums and the quotient in fp64.  Any layout
                                  the generic flag takes, fp32 or fp16 planes.  Membership, bins, statistics, MI, alpha, beta
                                  and W_r_c are the bits of the same flags without this one; the colours move by ~1e-8
                                  relative (bar 1e-4).  Filtered in fp64 under the flag as well, bit for bit as without it: the
                                  rest list (N > 64, or N > 832 with the wave flag) on the generic filter kernel; under
                                  RPF_DEGEN_REF_ABORT a pixel on the redo list (rpf_counters.redo_pixels); a pass that falls
                                  back to route 3 (S > 64, or S > 832 with the wave flag).  rpf_query_route keeps saying 4 / 5,
                                  filter_kernel_launches and redo_pixels count as without the flag.  RPF_FLAG_FAST_WEIGHTS keeps
                                  its meaning and its refusals.  Without both RPF_FLAG_GENERIC and RPF_FLAG_GENERIC_PACKED,
                                  together with RPF_FLAG_FAST_WEIGHTS, or together with RPF_FLAG_WIDE_NBHD (wide passes are fp64
                                  throughout) it is RPF_E_UNSUPPORTED, from every filter entry point and from
                                  rpf_layout_kernels, before any device work. */
    RPF_FLAG_SPIKE_CLAMP = 1024, /* opt-in: after the LAST pass of the call the spike pass runs on the fp64 colours of the filtered
                                  rows -- a sample further than `threshold` standard deviations from its pixel's mean on any
                                  channel is replaced by the mean of the pixel's other samples, and (preserve_energy) the removed
                                  energy is handed back to every sample of the filtered rows as one constant per channel; the
                                  definition is DESIGN.md section 12, the parameters rpf_set_spike below.  It runs before the
                                  reduce, before every download (fp32 samples, colour64_out, pixel means) and before the film
                                  step, from rpf_filter, rpf_filter_ex, rpf_filter_device, rpf_filter_film, rpf_multi_filter and
                                  rpf_multi_filter_film.  A caller who makes one call per pass sets it on the last call only.
                                  Independent of every route flag: rpf_layout_kernels, rpf_max_nbhd, rpf_query_route,
                                  rpf_counters and the launch counts answer as without it.  In rpf_filter it implies the serial
                                  download of RPF_FLAG_NO_OVERLAP (no band may leave before delta is known).
                                  RPF_E_NONFINITE is returned as before, and the spike pass still runs.
                                  rpf_filter_pass_debug refuses the flag (RPF_E_UNSUPPORTED) before any device work. */
    RPF_FLAG_SAMPLED_NBHD = 2048, /* opt-in: the published random-subset gather.  A pass p of the call with draws[p] > 0
                                  (rpf_set_sampling below) does not take every sample of its box as a candidate: it draws
                                  draws[p] samples per pixel, Gaussian-distributed around the pixel, from a counter-based
                                  generator in integer arithmetic, keeps the distinct ones in the
                                  reference's visiting order and runs the unchanged 3-sigma test on them.  The member list
                                  is a subsequence of the full-box list; everything behind it (statistics, bins, MI, alpha,
                                  beta, W_r_c, weights, blend; fp64) is that of the packed and one-wave layout-generic
                                  kernels on that list.  rpf_query_route says 8, redo_pixels is 0, filter_kernel_launches
                                  counts one launch per non-empty size class, sum_nbhd / max_nbhd / rpf_query_nbhd report
                                  the sampled N.  S + draws[p] <= 832 (RPF_E_BADARG otherwise; RPF_FLAG_SAMPLED_REST lifts
                                  the bound to 8192).  A pass with draws[p] == 0
                                  runs exactly as without the flag: same route, same bits.  Every filter entry point takes
                                  the flag (rpf_filter_pass_debug: pass id pass_id0, draws[0]); an entry point that runs no
                                  pass (stage 1a, the colour / reduce / spike / film-window helpers) takes a descriptor with
                                  the flag as one without it and does not look at the configuration.  The two compiled layouts
                                  take it alone, any other layout needs RPF_FLAG_GENERIC as before; rpf_layout_kernels
                                  reports *generic_out as without it; rpf_max_nbhd is unchanged (a pass above 65535 still
                                  needs RPF_FLAG_WIDE_NBHD).  Refused before any device work: the flag without a prior
                                  rpf_set_sampling, a negative draw count, S + draws[p] > 832 (RPF_E_BADARG); a pass with
                                  draws[p] > 0 under RPF_DEGEN_REF_ABORT (the reference has no sampled gather to reproduce and
                                  the redo kernels run their own full-box stage 1b), the flag with RPF_FLAG_FAST_WEIGHTS,
                                  RPF_FLAG_GENERIC_FAST or RPF_FLAG_STREAM_FAST (sampled passes are fp64; rpf_layout_kernels
                                  answers the same way) (RPF_E_UNSUPPORTED). */
    RPF_FLAG_MEMBER_TEST = 4096,  /* opt-in: the published membership test.  Stage 1b's test takes a multiple of sigma and an
                                  absolute floor per feature (rpf_set_membership below): a candidate is
                                  rejected on feature k iff |f_k - m_k| >= sd_k * mult_k AND |f_k - m_k| > fl_k, fl_k = -inf when
                                  sd_k > floor_k, else floor_k -- so a flat pixel (sd_k = 0) accepts its flat neighbours instead
                                  of rejecting everything.  mult 3 and a negative floor on every feature is the reference's test
                                  on every input.  Own samples first, the visiting order and every stage behind the list are
                                  unchanged.  The flag covers every pass of a call.  A full-box pass takes route 9
                                  (rpf_query_route; route 10 under RPF_FLAG_MEMBER_FUSED below): a count kernel lists the members of every pixel with N <= 832, the packed
                                  and one-wave layout-generic kernels filter them by size class, the wide kernel takes the
                                  pixels with N > 832 under the same test; redo_pixels is 0, filter_kernel_launches counts one
                                  launch per non-empty class plus one for a non-empty rest list, sum_nbhd / max_nbhd /
                                  rpf_query_nbhd report the new N.  The member pool grows to the sum of N - S over the listed
                                  pixels (option "wide_pool" sets its first size): about pixels * 384 * 4 bytes, 3 GB, on a
                                  flat 1080p frame of 8 spp at box 7.  A sampled pass (RPF_FLAG_SAMPLED_NBHD, draws > 0) stays
                                  route 8 and applies the test to its draws.  A call without the flag is not affected.  The two
                                  compiled layouts take the flag alone, any other layout needs RPF_FLAG_GENERIC;
                                  rpf_layout_kernels reports *generic_out as without it; rpf_max_nbhd is unchanged.  Every
                                  filter entry point takes the flag; one that runs no pass ignores it.  Refused before any
                                  device work: the flag without a prior rpf_set_membership (RPF_E_BADARG); under
                                  RPF_DEGEN_REF_ABORT (the reference has no such test, and the redo kernels run their own
                                  stage 1b), with RPF_FLAG_FAST_WEIGHTS, RPF_FLAG_GENERIC_FAST or RPF_FLAG_STREAM_FAST (fp64
                                  only; rpf_layout_kernels answers the same way), a full-box pass with S > 832
                                  (RPF_E_UNSUPPORTED). */
    RPF_FLAG_SCHEDULE = 8192,     /* opt-in: the per-pass schedule of the weight stage (rpf_set_schedule below; DESIGN.md section
                                  15).  Pass p of the call reads entry e = pass0 + p of the table: seed[e] replaces
                                  desc.sigma_seed (sigma_c^2 = sigma_f^2 = seed[e]^2 / (1 - W_r_c)^2), and stage 3c forms
                                  alpha_k = clamp0(1 - gain_c[e] * W_r^{c,k}), beta_k = clamp0(1 - gain_f[e] * W_r^{f,k}) *
                                  W_c^{f,k} with clamp0(v) = v < 0 ? 0 : v (a NaN stays a NaN), each product and each difference
                                  rounded once.  W_r_c, sigma_p, stages 1 to 3b and the blend are untouched; the debug planes
                                  alpha / beta report the scheduled values.  A pass whose two gains are exactly 1 runs the
                                  statements of a call without the flag on the route it would take without it (the fused
                                  routes 0 to 2 included, under either degenerate policy) with seed[e] as its seed: gains 1 are
                                  the reference on every input by construction.  A pass with a gain other than 1 runs on the
                                  layout-generic kernels only (routes 3 to 9: RPF_FLAG_GENERIC, a wide pass, a sampled pass or
                                  RPF_FLAG_MEMBER_TEST), fp64 or with RPF_FLAG_GENERIC_FAST / RPF_FLAG_STREAM_FAST (the fp32
                                  coefficients are formed from the scheduled alpha / beta).  The flag selects no route:
                                  rpf_query_route, the counters, rpf_layout_kernels and rpf_max_nbhd answer as without it.  It
                                  composes with RPF_FLAG_SAMPLED_NBHD, RPF_FLAG_MEMBER_TEST and RPF_FLAG_SPIKE_CLAMP.  An entry
                                  point that runs no pass ignores it; rpf_filter_pass_debug is one pass and reads entry pass0.
                                  Refused before any device work: the flag without a prior rpf_set_schedule, pass0 + the
                                  number of passes > RPF_MAX_BOXES (RPF_E_BADARG); a pass with a gain other than 1 under
                                  RPF_DEGEN_REF_ABORT (the reference has no such rule, and the redo launch would have to carry
                                  it) or on the fused kernels (RPF_E_UNSUPPORTED). */
    RPF_FLAG_SAMPLED_REST = 16384, /* opt-in, modifies RPF_FLAG_SAMPLED_NBHD: a sampled pass may have S + draws[p] <= RPF_SAMPLED_MAX
                                  (8192) instead of 832; rpf_max_draws() tells the bound.  The definition
                                  of a sampled neighbourhood is unchanged: the own samples, then the distinct surviving draws
                                  that pass stage 1b's test, in ascending visiting order.  A pass with S + draws[p] <= 832 runs
                                  exactly as without this flag: same count kernel, same launches, same bits.  Above it the draws
                                  are counted by a kernel that sorts them a workgroup per pixel; pixels that end with N <= 832
                                  run on the packed and one-wave class kernels as before, and pixels with N > 832 go to one rest
                                  launch of the generic filter kernel that reads their listed members (fp64, the 2^-44 table,
                                  LDS and scratch sized for S + draws, not for box*box*S).  S itself may exceed 832: every
                                  pixel of such a pass is a rest pixel.  rpf_query_route keeps saying 8, redo_pixels is 0,
                                  filter_kernel_launches counts one launch per non-empty class plus one for a non-empty rest
                                  list, sum_nbhd / max_nbhd / rpf_query_nbhd report the sampled N.  The member pool grows to the
                                  sum of N - S over the pixels, at most pixels * draws entries (option "wide_pool" sets its
                                  first size).  It composes with RPF_FLAG_MEMBER_TEST, RPF_FLAG_SCHEDULE, RPF_FLAG_SPIKE_CLAMP
                                  and RPF_FLAG_WIDE_NBHD (a pass with box*box*S > 65535 still needs that flag) as route 8 does,
                                  from every filter entry point; rpf_layout_kernels reports *generic_out as without it and
                                  rpf_max_nbhd is unchanged.  Refused before any device work: the flag without
                                  RPF_FLAG_SAMPLED_NBHD (RPF_E_UNSUPPORTED; rpf_layout_kernels answers the same way);
                                  S + draws[p] > 8192 on a pass with draws[p] > 0 (RPF_E_BADARG); every other refusal of a
                                  sampled pass stands (RPF_DEGEN_REF_ABORT, the three fp32 flags, a missing rpf_set_sampling,
                                  a negative draw count). */
    RPF_FLAG_PASS_REPORT = 32768, /* opt-in: every pass of the call leaves one rpf_pass_report (below), reduced
                                  on the device from that pass's input colours, its output colours (before the spike pass), N,
                                  alpha, beta and W_r_c over the filtered rows.  Taken by rpf_filter, rpf_filter_ex,
                                  rpf_filter_device, rpf_filter_film, rpf_multi_filter, rpf_multi_filter_film and
                                  rpf_filter_pass_debug (entry 0); an entry point that runs no pass ignores it.  It changes no
                                  result, counter, route or launch count: rpf_layout_kernels, rpf_max_nbhd, rpf_max_draws,
                                  rpf_query_route and rpf_counters answer as without it (filter_kernel_launches counts filter
                                  kernels, not the report's).  Each pass pays three scratch planes (alpha, beta, W_r_c), their
                                  clearing, the report kernels and one small read-back that drains the stream.  In rpf_filter it
                                  implies the serial order of RPF_FLAG_NO_OVERLAP.  RPF_E_NONFINITE is returned as before, and
                                  the report is still filled. */
    RPF_FLAG_MEMBER_FUSED = 65536, /* opt-in, modifies RPF_FLAG_MEMBER_TEST: a full-box pass of the call runs on the compiled, fused
                                  kernels behind a count kernel that applies the configured test (route 10; DESIGN.md section
                                  14e) -- the structure of the size-binned route 2: the count kernel leaves N and the acceptance
                                  masks, the pixels are dealt into the eleven size classes, the packed, one-wave and four-wave
                                  compiled kernels rebuild their member lists from the masks, and the class N > 3136 goes to
                                  the wide kernel under the same test.  A pass takes route 10 when it has no sampled draws, the
                                  layout is one of the two compiled ones and the call is without RPF_FLAG_GENERIC,
                                  box*box*S <= 65535 and option "wide" does not force it, and under RPF_FLAG_SCHEDULE its entry's
                                  gains are both 1 (the entry's seed is honoured).  Every other pass of the call runs exactly as
                                  without this flag (route 8 sampled, route 9 scheduled-gain, wide or layout-generic).
                                  Membership, statistics and bin ids are route 9's bits; MI, alpha, beta, W_r_c and the colours
                                  are those the compiled kernels give for that member list (route 2's kernels: the per-sample
                                  stage-4 bars of the resident classes).  Options "packed", "waves_per_pixel", "split_weights",
                                  "table_in_lds" and "strip_w" act as on route 2; "binning" has no effect.  redo_pixels is 0,
                                  filter_kernel_launches counts one launch per non-empty class of the eleven, sum_nbhd /
                                  max_nbhd / rpf_query_nbhd report the configured test's N.  A later pass of the same call with
                                  the same box re-uses the masks and lists (never across rpf_set_membership, never from or
                                  for a pass of another route).  No member pool is allocated.  rpf_layout_kernels answers as
                                  for the word without the flag; rpf_max_nbhd and rpf_max_draws do not read it.  Refused before
                                  any device work: the flag without RPF_FLAG_MEMBER_TEST (RPF_E_UNSUPPORTED; rpf_layout_kernels
                                  answers the same way); every refusal of RPF_FLAG_MEMBER_TEST stands with it. */
    RPF_FLAG_SCHEDULE_FUSED = 131072, /* opt-in, modifies RPF_FLAG_SCHEDULE: a permission, not a route.  A pass
                                  of the call whose entry has a gain other than 1 and which carries no layout-generic bit (a
                                  compiled layout, no RPF_FLAG_GENERIC, not wide, not sampled, no membership test) is no longer
                                  refused: it runs on the route it would take with gains of 1 -- route 0, 1 or 2, same probe, same
                                  options, same launch counts -- on builds of the compiled kernels that form
                                  alpha_k = clamp0(1 - gain_c * W_r^{c,k}) and beta_k = clamp0(1 - gain_f * W_r^{f,k}) * W_c^{f,k}
                                  in stage 3c (the quotients are the unscheduled kernels' own; each product and difference is
                                  rounded once; a NaN stays a NaN; W_r_c is untouched).  Under RPF_FLAG_MEMBER_TEST |
                                  RPF_FLAG_MEMBER_FUSED such a pass takes route 10 instead of route 9.  The streaming class
                                  N > 3136 of either runs the kernel it runs without the flag, under the same gains.
                                  rpf_query_route, the counters, rpf_query_nbhd, rpf_layout_kernels, rpf_max_nbhd and
                                  rpf_max_draws answer as for the same call with gains of 1.  Every pass that carries
                                  layout-generic bits (RPF_FLAG_GENERIC, wide, sampled, route 9 without RPF_FLAG_MEMBER_FUSED)
                                  runs exactly as without this flag, and a pass with both gains 1 runs the unscheduled kernels.
                                  Taken by every filter entry point (rpf_filter_pass_debug reads entry pass0).  Refused before
                                  any device work: the flag without RPF_FLAG_SCHEDULE (RPF_E_UNSUPPORTED; rpf_layout_kernels
                                  answers the same way); a gain other than 1 on a pass of the compiled kernels together with
                                  RPF_FLAG_FAST_WEIGHTS (RPF_E_UNSUPPORTED: the scheduled builds are fp64 only); every refusal
                                  of RPF_FLAG_SCHEDULE stands (RPF_DEGEN_REF_ABORT with a gain other than 1 included). */
    RPF_FLAG_SAMPLED_FUSED = 262144, /* opt-in, modifies RPF_FLAG_SAMPLED_NBHD: a sampled pass of the call runs on the compiled, fused
                                  kernels behind a count kernel that leaves the draws as acceptance masks (route 11; DESIGN.md
                                  section 13f) -- the second half of the size-binned route 2: the count kernel forms the draws
                                  of route 8 (same key, same table, same discards), applies stage 1b's test (the configured one
                                  under RPF_FLAG_MEMBER_TEST) and leaves N and one bit per accepted candidate of the window; the
                                  pixels are dealt into the ten resident size classes, and the packed, one-wave and four-wave
                                  compiled kernels rebuild their member lists from the masks.  A pass takes route 11 when it has
                                  draws[p] > 0, the layout is one of the two compiled ones and the call is without
                                  RPF_FLAG_GENERIC, box*box*S <= 65535 and option "wide" does not force it, S + draws[p] <= 3136
                                  (the largest resident class; with more draws the pass needs RPF_FLAG_SAMPLED_REST and stays on
                                  route 8), its mask stride is within option "sampled_fused_stride", and under RPF_FLAG_SCHEDULE
                                  its entry's gains are both 1 or the call carries RPF_FLAG_SCHEDULE_FUSED (the pass then runs
                                  the scheduled builds).  Every other pass of the call runs exactly as without this flag.
                                  Membership, statistics and bin ids are route 8's bits; MI, alpha, beta, W_r_c and the colours
                                  are those the compiled kernels give for that member list (route 2's kernels: the per-sample
                                  stage-4 bars of the resident classes).  The kernels are sized from min(box*box*S, S + draws).
                                  Options "packed", "waves_per_pixel", "split_weights", "table_in_lds" and "strip_w" act as on
                                  route 2; "binning" has no effect.  redo_pixels is 0, filter_kernel_launches counts one launch
                                  per non-empty class (the count kernel is not counted), sum_nbhd / max_nbhd / rpf_query_nbhd
                                  report the sampled N.  Masks and lists are never re-used by a later pass (the draws change
                                  with the pass id), and no member pool is allocated: the masks take
                                  ceil((box*box - 1) * S / 64) * 8 bytes per pixel.  rpf_layout_kernels answers as for the word
                                  without the flag; rpf_max_nbhd and rpf_max_draws do not read it.  Refused before any device
                                  work: the flag without RPF_FLAG_SAMPLED_NBHD (RPF_E_UNSUPPORTED; rpf_layout_kernels answers
                                  the same way); every refusal of RPF_FLAG_SAMPLED_NBHD stands with it. */
    RPF_FLAG_SAMPLED_LISTED = 524288, /* opt-in, modifies RPF_FLAG_SAMPLED_NBHD: a sampled pass of the call runs on the listed builds of
                                  the compiled, fused kernels, which take their member lists from route 8's member pool instead of
                                  rebuilding them from acceptance masks (route 12).  The count kernel lists
                                  the accepted draws of route 8 (same key, same table, same discards, stage 1b's test or under
                                  RPF_FLAG_MEMBER_TEST the configured one) as plane offsets behind one cursor reservation per pixel
                                  -- for box*box*S <= 65535 the bitmap kernel of route 11 with a listing tail, above that route
                                  8's own count launch -- the pixels are dealt into the ten resident size classes, and the packed,
                                  one-wave and four-wave compiled kernels copy their lists.  A pass takes route 12 when it has
                                  draws[p] > 0, the layout is one of the two compiled ones and the call is without
                                  RPF_FLAG_GENERIC, S + draws[p] <= 3136, the pass is accepted at all (the window span check;
                                  box*box*S <= 262144 with RPF_FLAG_WIDE_NBHD above 65535), option "wide" does not force it, and
                                  under RPF_FLAG_SCHEDULE its entry's gains are both 1 or the call carries RPF_FLAG_SCHEDULE_FUSED
                                  (the pass then runs the scheduled listed builds).  Every other pass of the call runs exactly as
                                  without this flag.  It does not need RPF_FLAG_SAMPLED_FUSED; with both, a pass that both routes
                                  can take runs on route 12 when its mask stride is at least option "sampled_listed_stride", and
                                  a pass route 11 cannot take (wide, or above "sampled_fused_stride") runs on route 12.  Results
                                  are route 11's bit for bit where both apply: membership, statistics and bin ids are route 8's
                                  bits; MI, alpha, beta, W_r_c and the colours are those the compiled kernels give for that list.
                                  The kernels are sized from min(box*box*S, S + draws), on a wide pass too.  No mask buffer is
                                  allocated: the pool takes 4 * (N - S) bytes per pixel, at most 4 * draws, under route 8's rules
                                  (option "wide_pool": grown once to the cursor's figure, the count repeated).  Options "packed",
                                  "waves_per_pixel", "split_weights", "table_in_lds" and "strip_w" act as on route 2 (the four-wave
                                  kernels are not shut out at windows above 4096 candidates: a list needs no mask array).
                                  rpf_layout_kernels answers as for the word without the flag; rpf_max_nbhd and rpf_max_draws do
                                  not read it: S + draws > 832 still needs RPF_FLAG_SAMPLED_REST, a pass above 65535
                                  RPF_FLAG_WIDE_NBHD.  Refused before any device work: the flag without RPF_FLAG_SAMPLED_NBHD
                                  (RPF_E_UNSUPPORTED; rpf_layout_kernels answers the same way); every refusal of
                                  RPF_FLAG_SAMPLED_NBHD stands with it. */
    RPF_FLAG_GENERIC_QUAD = 1048576, /* opt-in, modifies RPF_FLAG_GENERIC | RPF_FLAG_GENERIC_PACKED | RPF_FLAG_GENERIC_WAVE: the
                                  pixels whose neighbourhood holds 832 < N <= 3136 samples run on the four-wave layout-generic
                                  kernels -- a 256-thread workgroup per pixel with the member list, the bin ids and T[0 .. capacity]
                                  resident in LDS, size classes N <= 1600 and 3136, the member list rebuilt from the count pass's
                                  acceptance masks without a second 3-sigma test -- behind the count pass of the packed flag; only
                                  N > 3136 stays on the generic filter kernel.  A layout whose LDS carve-up
                                  does not fit a class (rpf_generic_quad_carve below tells) is not offered it: those pixels stay
                                  on the generic filter kernel.  Same layouts as the generic flag.  Same membership, bins,
                                  statistics, MI, alpha, beta and W_r_c as under the generic flag alone; the colours agree to
                                  rounding.  rpf_query_route says 13 for a pass with S <= 3136 (a pass with 832 < S <= 3136 has
                                  empty packed and one-wave classes; a pass with S > 3136 is route 3).  A wide, sampled or
                                  member-test pass of the call runs as without the flag.  fp64 only: without all three of
                                  RPF_FLAG_GENERIC, RPF_FLAG_GENERIC_PACKED and RPF_FLAG_GENERIC_WAVE, or together with
                                  RPF_FLAG_FAST_WEIGHTS, RPF_FLAG_GENERIC_FAST or RPF_FLAG_STREAM_FAST, it is RPF_E_UNSUPPORTED,
                                  from every filter entry point and from rpf_layout_kernels, before any device work. */
    RPF_FLAG_STREAM_FAST = 512/* opt-in, modifies RPF_FLAG_GENERIC and / or RPF_FLAG_WIDE_NBHD: the two kernels that walk a
                                  neighbourhood of any size with 256 threads -- the generic filter kernel (route 3, the rest
                                  list N > 64 / N > 832 of routes 4 / 5) and the wide kernel (route 6, the rest list N > 832 of
                                  route 7) -- evaluate the S x N pair weights of stage 4 in the fp32 arithmetic described for
                                  RPF_FLAG_GENERIC_FAST above: z and the 5 + n_feat coefficients formed in fp64 and rounded
                                  once, differences, squares and the weighted sum in fp32, ONE hardware exponential, the
                                  weights widened to fp64, both sums and the quotient in fp64.  On a wide pass dealt by size
                                  class (route 7) the packed and one-wave class kernels run their fp32 instantiations as well:
                                  under this flag every pixel of a wide pass is fp32.  On routes 4 / 5 the packed and one-wave
                                  classes stay steered by RPF_FLAG_GENERIC_FAST alone; with both flags every pixel of the pass
                                  is fp32.  Any layout the kernels take, fp32 or fp16 planes.  Membership, bins, statistics,
                                  MI, alpha, beta and W_r_c are the bits of the same flags without this one; the colours move
                                  by ~1e-8 relative (bar 1e-4).  It pays where neighbourhoods are large -- wide passes, large
                                  boxes -- and is slower than fp64 on a box-7 pass (the fp32 instantiations hold one workgroup per
                                  CU).  Filtered in fp64 under the flag as well, bit for bit as
                                  without it: under RPF_DEGEN_REF_ABORT a pixel on the redo list (routes 4, 5 and 7); every
                                  pass that runs the compiled, fused kernels (routes 0, 1, 2 -- the non-wide passes of a
                                  RPF_FLAG_WIDE_NBHD call without RPF_FLAG_GENERIC), their streaming class N > 3136 included.
                                  rpf_query_route, filter_kernel_launches, redo_pixels, sum_nbhd and max_nbhd are those of the
                                  same flags without this one.  Without both RPF_FLAG_GENERIC and RPF_FLAG_WIDE_NBHD it is
                                  RPF_E_UNSUPPORTED; together with RPF_FLAG_FAST_WEIGHTS one of that flag's refusals fires;
                                  every older refusal stands (RPF_FLAG_GENERIC_FAST with RPF_FLAG_WIDE_NBHD among them) -- from
                                  every filter entry point and from rpf_layout_kernels, before any device work. */
};

typedef struct rpf_desc {
    int32_t W;                         /* pixels per row                                            */
    int32_t H;                         /* rows present in the buffers (owned + halo)                */
    int32_t S;                         /* samples per pixel, identical for every pixel              */
    int32_t row_begin;                 /* first row to filter                                       */
    int32_t row_end;                   /* one past the last row to filter                           */
    int32_t n_box;                     /* number of passes (> 1 only when the slab is the whole buffer) */
    int32_t box_sizes[RPF_MAX_BOXES];  /* odd box sizes, one per pass (reference: {7}, rpf.cpp:767)  */
    int32_t beta_map;                  /* rpf_beta_map                                              */
    int32_t degenerate_policy;         /* rpf_degenerate_policy                                     */
    int32_t flags;
    double eps;                        /* RPF_DEGEN_EPS epsilon (1e-10).  Under RPF_DEGEN_EPS a NaN or negative value is
                                          RPF_E_BADARG before any device work; a zero of either sign (IEEE: 0 / 0 is a NaN and the
                                          colour falls back), +inf and every positive value are accepted.  RPF_DEGEN_REF_ABORT never reads it */
    double sigma_seed;                 /* rpf.cpp:533: 0.002                                        */
    /* Sample-vector layout.  All three 0 = the reference's: 2 random parameters (pLens), 12 features, fp32 planes.
     * Compiled kernels also exist for n_random = 4, n_feat = 18 with RPF_PLANES_F16 (27 dims, fp16 feature storage: BASELINE
     * configs[4]).  Any other layout -- a pbrt fork that records time, or the light-sample coordinates of each bounce, as
     * further random parameters, or more features -- needs RPF_FLAG_GENERIC in `flags` (bounds there; a field of 0 still means
     * the reference's value) and returns RPF_E_UNSUPPORTED without it; rpf_layout_kernels() tells which.  With fp16 planes every `planes` pointer of this header
     * addresses 16-bit IEEE halves instead of floats; colours are still carried as fp64, outputs stay fp32.
     * Per-pixel debug planes are then sized by RPF_NDIM_OF / RPF_NPAIR_OF / n_feat. */
    int32_t n_random;
    int32_t n_feat;
    int32_t plane_dtype;               /* RPF_PLANES_F32 / RPF_PLANES_F16                           */
    int32_t reserved;
} rpf_desc;

/* per-pixel stage outputs for parity tests; every pointer may be NULL; indexed [y*W+x] */
typedef struct rpf_debug {
    int32_t *nbhd_size;    /* [H*W]      N, stage 1b (rpf.cpp:556-586)                              */
    double *mean;          /* [H*W*19]   neighbourhood mean,  stage 2 (rpf.cpp:600)                  */
    double *stddev;        /* [H*W*19]   neighbourhood std,   stage 2 (rpf.cpp:601)                  */
    double *mi;            /* [H*W*96]   MI values in ComputeCFWeights call order (rpf.cpp:416-442)  */
    double *alpha;         /* [H*W*3]    rpf.cpp:474-476                                             */
    double *beta;          /* [H*W*12]   rpf.cpp:478-480                                             */
    double *wrc;           /* [H*W]      rpf.cpp:483-487                                             */
    uint32_t *bin_hash;    /* [H*W*19]   FNV-1a over each column's histogram bin ids (mi.cpp:14-16)  */
    uint32_t *member_hash; /* [H*W]      FNV-1a over the neighbourhood member list, in order         */
} rpf_debug;

typedef struct rpf_counters {
    int64_t samples_filtered;   /* (row_end-row_begin)*W*S*n_box of the last call                    */
    int64_t sum_nbhd;           /* sum over filtered pixels of N, last pass                         */
    int64_t nonfinite_pixels;   /* pixels whose filtered colour was NaN, all passes                 */
    int32_t max_nbhd;
    int32_t first_bad_pixel;    /* y*W+x, -1 if none                                                */
    float filter_kernel_ms;     /* RPF_FLAG_TIMING: sum over passes of the fused filter kernel      */
    float stats_kernel_ms;      /* RPF_FLAG_TIMING: sum over passes of the per-pixel stats kernel   */
    float device_total_ms;      /* RPF_FLAG_TIMING: first launch to last kernel end                 */
    float h2d_ms;               /* rpf_filter(): host->HBM marshalling, wall clock                  */
    float d2h_ms;               /* rpf_filter(): HBM->host                                          */
    int32_t filter_kernel_launches;
    int32_t options_active;     /* 1 when any rpf_set_option override was in force (diagnostic runs)   */
    int32_t redo_pixels;        /* RPF_DEGEN_REF_ABORT, last pass: pixels filtered a second time with the reference's own
                                   floating-point MI expression (an exactly independent histogram pair at a non-power-of-two
                                   N: mi.cpp:79-86 returns rounding residue there, not 0).  The total of the pass: rpf_filter's
                                   row-band pipeline, which filters the last pass band by band, reports the sum over its
                                   bands, the figure of the serial call                                  */
} rpf_counters;

const char *rpf_version(void);
const char *rpf_status_string(int32_t status);

/* lifetime.  device = HIP device ordinal of this process. */
int32_t rpf_create(rpf_ctx **out, int32_t device);
void rpf_destroy(rpf_ctx *ctx);
const char *rpf_last_error(const rpf_ctx *ctx);

/*
 * The drop-in call: replaces the `for (box_size : box_sizes) ApplyRPFFilter(...)` loop of
 * rpf.cpp:767-775 plus the per-pixel reduction of rpf.cpp:779-794 (box reconstruction filter r=0.5).
 *   planes          host, 19 fp32 planes [19][H][W][S]
 *   ray_weight      host, [H][W][S] fp32 (SampleData::rayWeight, sd.h:60) or NULL (= 1)
 *   sample_rgb_out  host, 3 fp32 planes [3][H][W][S] of filtered sample colours, or NULL
 *   pixel_rgb_out   host, [H][W][3] fp32 mean over s of colour*rayWeight (rows outside the slab: unfiltered), or NULL
 */
int32_t rpf_filter(rpf_ctx *ctx, const rpf_desc *desc, const void *planes, const float *ray_weight,
                   float *sample_rgb_out, float *pixel_rgb_out);

/* rpf_filter() with the sample colours carried as doubles across the boundary, as the reference carries them in
 * SampleData (sd.h:205-208 getColorI / setColorI; the film that one ApplyRPFFilter call leaves is the input of the next,
 * rpf.cpp:732, 767-775).  A caller that keeps the reference's call shape -- one ApplyRPFFilter(film, tile, box) per box
 * size -- uses this so that no colour is rounded to fp32 between passes:
 *   colour64_in   host, 3 fp64 planes [3][H][W][S], or NULL (= planes 2..4 of `planes`)
 *   colour64_out  host, 3 fp64 planes of filtered colours, or NULL
 * With either pointer set the call runs upload, passes, download one after the other (no row-band overlap). */
int32_t rpf_filter_ex(rpf_ctx *ctx, const rpf_desc *desc, const void *planes, const double *colour64_in,
                      const float *ray_weight, float *sample_rgb_out, float *pixel_rgb_out, double *colour64_out);

/* Per-context tuning / diagnostic overrides (nothing in the library reads the environment).  Names:
 *   "stage_mask"       -1 = all stages (default); other values SKIP stages for timing ablations: results are WRONG
 *   "binning"          -1 auto (size-binned launches when box*box*S > 512), 0 off, 1 on
 *   "waves_per_pixel"  0 auto, 1, 4 (4 needs box*box*S > 832)
 *   "table_in_lds"     -1 auto, 0, 1
 *   "lds_pad"          extra LDS bytes per workgroup (lowers occupancy)
 *   "split_weights"    32- and 64-spp size classes: three launches (in-order chains; bins + MI; weights) instead of one
 *                      kernel, the light stages at two to three times the occupancy: -1 auto (default: on), 0 off, 1 on;
 *                      same results bit for bit
 *   "strip_w"          pixels per XCD strip of the pixel walk: 0 auto (default), else a multiple of 8; same results
 *   "packed"           neighbourhoods of N <= 64 samples on the packed kernels (8 / 4 / 2 / 1 pixels per wavefront): -1 auto
 *                      (default: on), 0 off (every pixel gets a whole wavefront), 1 on.  Every stage output up to alpha / beta /
 *                      W_r_c is the same bits either way; colours agree to rounding (~1e-16 relative)
 *   "count_first"      passes with box*box*S <= 512: stage 1b as its own launch ahead of the filter kernels (the route of
 *                      small-neighbourhood buffers) or inside filter_pixel_kernel: -1 auto (default: a ~2000-pixel probe
 *                      decides per pass), 0 fused, 1 count first.  Same results bit for bit; rpf_query_route tells.
 *   "screen"           far-pair screen of the weight stage (four-wave kernels): 1 on (default), 0 off.  Both settings
 *                      give the same filtered colours bit for bit.
 *   "wide"             passes of a call with RPF_FLAG_WIDE_NBHD: -1 auto (default: the wide kernel takes the passes with
 *                      box*box*S > 65535), 1 force (it takes every pass of such a call; a test hook: below 48586 samples it
 *                      then reads the 2^-44 table of the other kernels and gives the bits of route 3).  No effect without
 *                      the flag.
 *   "wide_pool"        wide passes of a call with RPF_FLAG_WIDE_CLASSES: entries of the member pool at the first count
 *                      launch: -1 auto (default: 8 per pixel of the slab), else that many (a test hook: a pool the data
 *                      exceeds is grown to the exact size and the count launch repeated; same results bit for bit)
 *   "sampled_fused_stride"  sampled passes of a call with RPF_FLAG_SAMPLED_FUSED: the largest mask stride, in 64-bit words per
 *                      pixel (ceil((box*box - 1) * S / 64)), at which such a pass takes route 11: -1 no bound (default), else 0 ..
 *                      1024; a pass above the bound stays on route 8 and runs exactly as without the flag.  No effect without
 *                      the flag (DESIGN.md section 13f has the measurements behind the default)
 *   "sampled_listed_stride"  sampled passes of a call with RPF_FLAG_SAMPLED_LISTED and RPF_FLAG_SAMPLED_FUSED both: the smallest
 *                      mask stride (the same figure) from which a pass that both routes can take runs on route 12: -1 auto (default:
 *                      the measured value of DESIGN.md section 13g, 144: box 17 x 32 spp and every wider window), else 0 .. 1025 (1025: never where route 11 applies).  A pass
 *                      that route 11 cannot take (wide, or above "sampled_fused_stride") runs on route 12 whatever it says.  No
 *                      effect without both flags
 * These names (but "wide", "wide_pool", "sampled_fused_stride" and "sampled_listed_stride") steer the fused routes only: a call with RPF_FLAG_GENERIC, with or without RPF_FLAG_GENERIC_PACKED, runs
 * the same kernels whatever they say (they are accepted and have no effect there; options_active still reports them).
 * rpf_counters.options_active tells whether a result was produced under any override. */
int32_t rpf_set_option(rpf_ctx *ctx, const char *name, int64_t value);
/* RPF_OK when rpf_set_option would take (name, value), RPF_E_BADARG otherwise.  Needs no context and no device. */
int32_t rpf_check_option(const char *name, int64_t value);

/* Page-locked host memory for the buffers handed to rpf_filter(): a feature producer that writes its samples straight
 * into such planes (instead of the reference's heap SamplingFilm, sample_film.cpp:6-43) gets full-rate DMA and real
 * overlap of the upload with the first filter pass.  Pageable buffers work too, more slowly. */
int32_t rpf_host_alloc(rpf_ctx *ctx, uint64_t bytes, void **out);
int32_t rpf_host_free(rpf_ctx *ctx, void *ptr); /* ctx may be NULL */

/* Same pass structure with every buffer already resident in HBM (device pointers).  d_colour is 3 fp64
 * planes [3][H][W][S], read as the input colours and overwritten with the filtered ones; planes 2..4 of
 * d_planes are ignored.  Runs on `stream`: the hipStream_t on which the caller produced the buffers (NULL = the
 * legacy default stream, e.g. PyTorch's default stream), so the pass is ordered after that work without an explicit
 * synchronisation.  Returns after the stream has drained (the status and the counters are read back). */
int32_t rpf_filter_device(rpf_ctx *ctx, const rpf_desc *desc, const void *d_planes, double *d_colour,
                          void *stream);

/* fp32 colour planes (planes 2..4 of d_planes) -> fp64 colour planes; and back, plus the pixel mean */
int32_t rpf_colour_from_planes_device(rpf_ctx *ctx, const rpf_desc *desc, const void *d_planes,
                                      double *d_colour, void *stream);
int32_t rpf_reduce_device(rpf_ctx *ctx, const rpf_desc *desc, const double *d_colour, const float *d_ray_weight,
                          float *d_sample_rgb_out, float *d_pixel_rgb_out, void *stream);

/* ---- stage-level entry points (host buffers; used by the parity tests) ---------------------------- */

/* stage 1a, FillMeanAndStddev (rpf.cpp:302-353): mean/std [H*W*12] fp64, pixel-major */
int32_t rpf_stage_pixel_stats(rpf_ctx *ctx, const rpf_desc *desc, const void *planes, double *mean, double *stddev);

/* one pass with one box size; colour_in (3 fp64 planes) may be NULL (= planes 2..4); colour_out 3 fp64
 * planes; dbg host pointers, any may be NULL */
int32_t rpf_filter_pass_debug(rpf_ctx *ctx, const rpf_desc *desc, int32_t box, const void *planes,
                              const double *colour_in, double *colour_out, const rpf_debug *dbg);

/* counters of the most recent rpf_filter / rpf_filter_device / rpf_filter_pass_debug call */
/* On the generic route (RPF_FLAG_GENERIC) filter_kernel_launches counts one launch per pass and redo_pixels is 0: that
 * kernel evaluates the reference's floating-point MI expression in place.
 * With RPF_FLAG_GENERIC_PACKED as well (route 4) filter_kernel_launches counts, per pass, one launch per non-empty packed
 * class (N <= 8, 16, 32, 64), one for the generic filter kernel when some pixel has N > 64, and under RPF_DEGEN_REF_ABORT one
 * for the redo launch; redo_pixels counts the pixels the packed kernels put on the redo list (the generic filter kernel then
 * filters them whole, evaluating the reference's expression in place).
 * With RPF_FLAG_GENERIC_WAVE as well (route 5) filter_kernel_launches counts, per pass, one launch per non-empty packed class,
 * one per non-empty one-wave class (N <= 128, 256, 448, 832), one for the generic filter kernel when some pixel has N > 832,
 * and under RPF_DEGEN_REF_ABORT one for the redo launch; redo_pixels counts the pixels the packed and the one-wave kernels put
 * on the redo list.
 * A wide pass (RPF_FLAG_WIDE_NBHD, box*box*S > 65535: route 6) counts one launch and leaves redo_pixels 0, whatever the other
 * flags say: it has no count pass and no size classes.
 * With RPF_FLAG_WIDE_CLASSES as well (route 7) such a pass counts as route 5 does, with the wide kernel in place of the generic
 * filter kernel: one launch per non-empty packed class, one per non-empty one-wave class, one for the wide kernel when some
 * pixel has N > 832, and under RPF_DEGEN_REF_ABORT one for the redo launch (the wide kernel again); redo_pixels counts the
 * pixels the packed and the one-wave kernels put on the redo list.
 * A sampled pass (RPF_FLAG_SAMPLED_NBHD with draws > 0: route 8) counts one launch per non-empty packed or one-wave class and
 * nothing else -- S + draws <= 832 leaves no rest list, and RPF_DEGEN_REF_ABORT is refused -- and leaves redo_pixels 0; under
 * RPF_FLAG_SAMPLED_REST a pass with S + draws > 832 adds one launch for a non-empty rest list (N > 832);
 * sum_nbhd / max_nbhd are those of the sampled neighbourhoods.
 * A full-box pass under RPF_FLAG_MEMBER_TEST (route 9) counts one launch per non-empty packed or one-wave class and one for the
 * wide kernel when some pixel has N > 832; RPF_DEGEN_REF_ABORT is refused, so redo_pixels is 0; sum_nbhd / max_nbhd are those
 * of the neighbourhoods the configured test leaves.
 * With RPF_FLAG_MEMBER_FUSED (route 10) such a pass counts as route 2 does: one launch per non-empty class of the eleven (the
 * class N > 3136 is the wide kernel's); redo_pixels is 0.
 * With RPF_FLAG_SAMPLED_FUSED (route 11) a sampled pass counts one launch per non-empty class of the ten resident ones (its count
 * kernel is not counted, and no pixel reaches the streaming class); redo_pixels is 0; sum_nbhd / max_nbhd are those of the
 * sampled neighbourhoods.
 * With RPF_FLAG_SAMPLED_LISTED (route 12) a sampled pass counts as on route 11: one launch per non-empty class of the ten resident
 * ones (the count kernel -- repeated once when the member pool had to grow -- is not counted, and no pixel reaches the streaming
 * class); redo_pixels is 0; sum_nbhd / max_nbhd are those of the sampled neighbourhoods.
 * With RPF_FLAG_GENERIC_QUAD (route 13) a pass counts as route 5 does, with one launch more per non-empty four-wave class
 * (N <= 1600, 3136): the generic filter kernel's launch is for N > 3136, or N above the last class the layout is offered;
 * redo_pixels includes the pixels the four-wave kernels put on the redo list. */
int32_t rpf_query_counters(rpf_ctx *ctx, rpf_counters *out);

/* neighbourhood size N of every pixel (rpf.cpp:586: the neighbourhood vector's size) as the last pass of the most recent
 * call left it: nbhd_out host, int32 [H*W] (rows outside the filtered slab: whatever an earlier call left there);
 * count must equal desc W*H of that call.  For workload statistics (mean / percentiles of N). */
int32_t rpf_query_nbhd(rpf_ctx *ctx, int32_t *nbhd_out, int64_t count);

/* which kernel route the last pass of the most recent call took (a performance decision, the results are the same bits):
 * 0 = fused (filter_pixel_kernel runs stage 1b itself), 1 = count first (stage 1b as its own launch, then the packed
 * small-neighbourhood kernels take most pixels: the route of path-traced buffers), 2 = size-binned
 * (box*box*S > 512), 3 = the layout-generic kernels (RPF_FLAG_GENERIC; several times slower, same membership, bins and
 * statistics), 4 = the layout-generic kernels with small neighbourhoods packed (RPF_FLAG_GENERIC | RPF_FLAG_GENERIC_PACKED
 * on a pass with S <= 64), 5 = the same with 64 < N <= 832 on the one-wave layout-generic kernels (... | RPF_FLAG_GENERIC_WAVE
 * on a pass with S <= 832), 6 = the wide layout-generic kernel (RPF_FLAG_WIDE_NBHD on a pass with box*box*S > 65535),
 * 7 = such a pass counted first and dealt by size class (... | RPF_FLAG_WIDE_CLASSES, S <= 832),
 * 8 = a sampled pass (RPF_FLAG_SAMPLED_NBHD with draws > 0: its member lists differ, by definition),
 * 9 = a full-box pass under RPF_FLAG_MEMBER_TEST (count kernel with the configured membership test, size classes, the wide
 * kernel for N > 832; its member lists are the reference's only under the reference's multiples and floors),
 * 10 = such a pass under RPF_FLAG_MEMBER_FUSED on a compiled layout (count kernel with the configured test, then the compiled
 * kernels of route 2 by size class; the same member lists as route 9),
 * 11 = a sampled pass under RPF_FLAG_SAMPLED_FUSED on a compiled layout (the draws' count kernel leaves acceptance masks, then
 * the compiled kernels of route 2 by size class; the same member lists as route 8),
 * 12 = a sampled pass under RPF_FLAG_SAMPLED_LISTED on a compiled layout (a count kernel lists the draws into the member pool, then
 * the listed builds of the compiled kernels by size class; the same member lists as route 8, wide windows included),
 * 13 = route 5 with 832 < N <= 3136 on the four-wave layout-generic kernels (... | RPF_FLAG_GENERIC_QUAD on a pass with
 * S <= 3136),
 * -1 = no pass yet.  Option "count_first" (0 / 1) overrides the probe that chooses between 0 and 1.  rpf_filter's row-band
 * pipeline runs that probe once per band, on the rows of the slab that are resident by then -- the last band of a pass on the
 * whole slab -- so the answer after such a call is the serial call's (bands above the last may have taken the other of 0 / 1:
 * same bits). */
int32_t rpf_query_route(rpf_ctx *ctx, int32_t *route_out);

/* visualizeSF (rpf.cpp:37-101, visualization/vis.cpp:34-51): the reference's six debug images, without the EXR
 * writer: per-pixel mean over the S samples of n0, n1, p0, p1, (pFilm.x, pFilm.y, 0), (pLens.x, pLens.y, 0), each
 * channel divided by its maximum over the image.  images_out: host, fp64 [6][H][W][3] in that order. */
int32_t rpf_feature_images(rpf_ctx *ctx, const rpf_desc *desc, const void *planes, double *images_out);

/* device self-test: the kernels divide by wave-uniform divisors with a hoisted reciprocal (3 instructions per
 * quotient); this compares n pseudo-random quotients bit-for-bit with the compiler's IEEE fp64 division.
 * mode 0: operand magnitudes of the filter (2^-40..2^40); mode 1: 2^-600..2^600 (exercises the fallback). */
int32_t rpf_selftest_udiv(rpf_ctx *ctx, uint64_t n, uint64_t seed, int32_t mode, uint64_t *mismatches);

/* ---- one caller, every GPU of the node -------------------------------------------------------------------------
 * The reference's caller is a single process (RPFIntegrator::Render, rpf.cpp:737-805, reached from api.cpp:1620).  A
 * rpf_multi owns one context per entry of `devices` (NULL / 0 = every visible device; an ordinal may repeat: two slabs
 * on one GPU rehearse the path on a one-GPU box) and rpf_multi_filter() is rpf_filter() for the whole image: it cuts
 * the image into contiguous row slabs (rows [g*H/G, (g+1)*H/G) on entry g), uploads each slab with the halo rows of its
 * neighbours ((box-1)/2 rows, rpf.cpp:561-571), runs every pass on all slabs concurrently, and refreshes the colour
 * halo between passes with peer-to-peer copies of the neighbour's owned boundary rows (features never change, so their
 * halo travels with the upload).  Results are bit-identical to rpf_filter() on one device -- VERIFIED with two and three slab
 * contexts on ONE device (plain device copies for the halo); the branch taken between two different ordinals
 * (hipDeviceEnablePeerAccess + hipMemcpyPeerAsync) has not executed on hardware in this repository's development (one-GPU
 * boxes): tests/test_gpu_parity.py::test_multi_context_row_slabs_equal_one_context carries (0, 1) cases that run wherever a
 * second GPU is visible, and bench.py's `multi_inprocess` leg uses every visible device.  desc->row_begin / row_end
 * must name the whole image; a slab must own at least (box-1)/2 rows.  One caller thread per rpf_multi. */
typedef struct rpf_multi rpf_multi;
int32_t rpf_multi_create(rpf_multi **out, const int32_t *devices, int32_t n_devices);
void rpf_multi_destroy(rpf_multi *m);
const char *rpf_multi_last_error(const rpf_multi *m);
int32_t rpf_multi_device_count(const rpf_multi *m);
int32_t rpf_multi_set_option(rpf_multi *m, const char *name, int64_t value);
int32_t rpf_multi_filter(rpf_multi *m, const rpf_desc *desc, const void *planes, const float *ray_weight,
                         float *sample_rgb_out, float *pixel_rgb_out);
/* merged over the slabs: sums, maxima, the lowest offending image pixel; filter_kernel_ms = sum over passes of the
 * slowest slab's kernel time */
int32_t rpf_multi_query_counters(rpf_multi *m, rpf_counters *out);

/* The slab / halo planner every slab path uses (rpf_multi_filter, rpf_multi_filter_film; raytracer-rpf_amd/slabs.py holds the
 * same slabs).  Needs no device.  n_slabs row slabs of an image of H rows, each holding `depth` halo rows of its neighbours:
 *   slabs_out   [n_slabs][4] = {a, b, ht, hb}: owned image rows [a, b) = [g*H/n_slabs, (g+1)*H/n_slabs), halo rows held above
 *               and below (min(depth, rows that exist)); buffer row 0 of slab g is image row a - ht
 *   copies_out  [*n_copies_out][5] = {source slab, source buffer row, destination slab, destination buffer row, rows}: a
 *               refresh of every halo row from the neighbour's OWNED boundary rows; room for 2 * (n_slabs - 1) entries
 * Any output may be NULL.  RPF_E_BADARG for H <= 0, n_slabs <= 0, depth < 0, or when n_slabs > 1 and a slab owns fewer than
 * `depth` rows (it would have to forward rows it does not own). */
int32_t rpf_multi_halo_plan(int32_t H, int32_t n_slabs, int32_t depth, int32_t *slabs_out, int32_t *copies_out,
                            int32_t *n_copies_out);

/* Which kernels the filter entry points will run for the layout and flags of desc, and whether they take it at all: RPF_OK
 * with *generic_out = 0 (the compiled, fused kernels) or 1 (the layout-generic kernels); RPF_E_UNSUPPORTED where every filter
 * entry point refuses the layout / flag combination (same function, so the two cannot drift) -- a layout without kernels,
 * RPF_FLAG_FAST_WEIGHTS on a layout other than the reference's 19 dims, or together with RPF_FLAG_GENERIC;
 * RPF_FLAG_GENERIC_PACKED without RPF_FLAG_GENERIC or with RPF_FLAG_FAST_WEIGHTS; RPF_FLAG_GENERIC_WAVE without both of
 * those flags or with RPF_FLAG_FAST_WEIGHTS; RPF_FLAG_WIDE_NBHD with RPF_FLAG_FAST_WEIGHTS; RPF_FLAG_WIDE_CLASSES without
 * RPF_FLAG_WIDE_NBHD; RPF_FLAG_GENERIC_FAST without both RPF_FLAG_GENERIC and RPF_FLAG_GENERIC_PACKED, with
 * RPF_FLAG_FAST_WEIGHTS or with RPF_FLAG_WIDE_NBHD (where it is accepted, *generic_out is 1 as without it);
 * RPF_FLAG_STREAM_FAST without both RPF_FLAG_GENERIC and RPF_FLAG_WIDE_NBHD (where it is accepted, *generic_out is that of the
 * same flags without it; with RPF_FLAG_FAST_WEIGHTS one of that flag's refusals above fires); RPF_E_BADARG for a NULL desc.
 * Only n_random, n_feat, plane_dtype and flags are read.  Needs no context and no device.  generic_out may be NULL. */
int32_t rpf_layout_kernels(const rpf_desc *desc, int32_t *generic_out);

/* The largest box*box*S a pass may have under the flags of desc: *nmax_out = 65535, or 262144 with RPF_FLAG_WIDE_NBHD; a
 * larger pass is RPF_E_UNSUPPORTED from every filter entry point (the pass set-up calls this function, so the two cannot
 * drift).  Only flags is read.  Needs no context and no device.  RPF_E_BADARG for a NULL pointer. */
int32_t rpf_max_nbhd(const rpf_desc *desc, int32_t *nmax_out);

/* The most draws a sampled pass (RPF_FLAG_SAMPLED_NBHD) may have under S and the flags of desc: *dmax_out = max(0, 832 - S), or
 * max(0, RPF_SAMPLED_MAX - S) with RPF_FLAG_SAMPLED_REST; a pass with more is RPF_E_BADARG from every filter entry point (their
 * check calls this function, so the two cannot drift).  Only S and flags are read.  Needs no context and no device.
 * RPF_E_BADARG for a NULL pointer or S <= 0. */
int32_t rpf_max_draws(const rpf_desc *desc, int32_t *dmax_out);

/* What the layout of desc gets from RPF_FLAG_GENERIC_QUAD at the size class `capacity` (1600 or 3136): RPF_OK when the LDS
 * carve-up of the four-wave kernel fits 160 KiB, with *workgroups_per_cu_out = the workgroups a compute unit holds and
 * *lds_bytes_out = the bytes of one workgroup; RPF_E_UNSUPPORTED when it does not fit (route 13 then leaves the pixels of that
 * class to the generic filter kernel) or the layout is none the layout-generic kernels take; RPF_E_BADARG for any other capacity
 * or a NULL desc.  Only n_random, n_feat and plane_dtype are read.  Needs no context and no device.  Either output may be NULL. */
int32_t rpf_generic_quad_carve(const rpf_desc *desc, int32_t capacity, int32_t *workgroups_per_cu_out, int64_t *lds_bytes_out);

/* The table the wide kernel forms MI from: table_out[k] = round(k ln k * 2^41), k = 0 .. nmax (nmax + 1 entries), computed on
 * the host in long double.  Every entry up to nmax = 262144 is below 2^63 (the 2^-44 table of the other kernels stops being
 * exact at k = 48586).  Host only, for parity checks; RPF_E_BADARG for NULL or nmax outside [0, 262144]. */
int32_t rpf_wide_table(int32_t nmax, uint64_t *table_out);

/* LDS bytes per workgroup the fused kernel needs for (S, box); > device limit => RPF_E_UNSUPPORTED */
int64_t rpf_lds_bytes_required(int32_t S, int32_t box);

/* The fused kernels gather a pixel's window through 32-bit byte offsets from the window's first sample, so the span of
 * box rows of the slab in bytes of an fp64 plane, box*W*S*8, must fit 32 bits.  RPF_OK if it does, RPF_E_UNSUPPORTED if
 * not (every filter entry point refuses such a call the same way), RPF_E_BADARG for non-positive arguments.  Needs no
 * device.  With box*box*S <= 65535 this only binds for slabs hundreds of thousands of pixels wide. */
int32_t rpf_check_window_span(int32_t W, int32_t S, int32_t box);

/* ---- the film step: pbrt's reconstruction filter and crop window on the filtered samples -----------------------------
 * RPFIntegrator::Render ends by feeding every sample through FilmTile::AddSample (rpf.cpp:779-794, film.h:121-161), x outer,
 * y inner, then s, and then MergeFilmTile + WriteImage (film.cpp:117-130, 169-203).  rpf_filter()'s pixel_rgb_out covers
 * only pbrt's default box filter of radius 0.5 with no crop window, and not in pbrt's arithmetic; these entry points
 * compute the film's values for any of pbrt's five PixelFilters and any crop window, bit-identical to a serial fp32
 * evaluation in the reference's order.  The buffer [H][W][S] is the sample film: its pixel (0,0) is raster pixel
 * (sample_x0, sample_y0) = Film::GetSampleBounds().pMin, which lies left of / above the image when the filter is wider
 * than half a pixel (e.g. (-2,-2) for gaussian r = 2 on a full frame).
 * Preconditions (RPF_E_BADARG otherwise, the message names the first offending sample in the reference's order):
 * every sample's pFilm lies in [q, q+1] on each axis, q = the raster coordinate of its pixel (what pbrt's
 * pPixel + Get2D() gives, fp32 rounding up to q+1 included; NaN fails); radii finite, > 0; non-empty pixel bounds; raster
 * coordinates (sample film and pixel bounds) and radii within +-2^22; the whole buffer is one slab (row_begin == 0,
 * row_end == H; row slabs over several contexts: rpf_multi_filter_film below).  fp16 planes (the 27-dim layout) are RPF_E_UNSUPPORTED: fp16 cannot place pFilm in its pixel
 * beyond 2048. */
enum { RPF_PIXFILTER_BOX = 0, RPF_PIXFILTER_TRIANGLE, RPF_PIXFILTER_GAUSSIAN, RPF_PIXFILTER_MITCHELL, RPF_PIXFILTER_SINC };
#define RPF_FILTER_TABLE_WIDTH 16 /* Film::filterTableWidth, film.h:91 */

typedef struct rpf_film {
    int32_t sample_x0, sample_y0;   /* raster coords of buffer pixel (0,0) = Film::GetSampleBounds().pMin              */
    int32_t px0, py0, px1, py1;     /* Film::croppedPixelBounds [p0, p1): the output pixels                            */
    float radius_x, radius_y;       /* Filter::radius                                                                 */
    float max_sample_luminance;     /* Film "maxsampleluminance" (film.cpp:248); INFINITY = off                       */
    float scale;                    /* Film "scale" (film.cpp:246); used by image_rgb_out only                        */
    float table[RPF_FILTER_TABLE_WIDTH * RPF_FILTER_TABLE_WIDTH]; /* Film::filterTable, [y][x], as film.cpp:66-76 fills it */
} rpf_film;

/* pbrt's filter table for the five filters (film.cpp:66-76 with each filter's Evaluate), host only, works without a GPU.
 * p0 / p1: gaussian alpha | mitchell B, C | sinc tau; a NaN parameter takes pbrt's default (gaussian alpha 2, mitchell
 * B = C = 1/3, sinc tau 3).  A pbrt binding passes pbrt's own table instead. */
int32_t rpf_film_filter_table(int32_t kind, float radius_x, float radius_y, float p0, float p1, float *table_out);

/* rpf_filter()'s passes over the W x H x S buffer (the sample film), then the film step.  Any output may be NULL.
 *   sample_rgb_out   [3][H][W][S]           filtered sample colours, as rpf_filter
 *   tile_rgb_out     [py1-py0][px1-px0][3]  FilmTilePixel::contribSum
 *   tile_weight_out  [py1-py0][px1-px0]     FilmTilePixel::filterWeightSum
 *   image_rgb_out    [py1-py0][px1-px0][3]  Film::WriteImage's value of the pixel (no splats), scale applied */
int32_t rpf_filter_film(rpf_ctx *ctx, const rpf_desc *desc, const rpf_film *film, const void *planes, const float *ray_weight,
                        float *sample_rgb_out, float *tile_rgb_out, float *tile_weight_out, float *image_rgb_out);
/* the film step alone on device buffers: d_planes' pFilm planes (0, 1), d_colour 3 fp64 planes [3][H][W][S] (what
 * rpf_filter_device leaves), d_ray_weight [H][W][S] or NULL (= 1); outputs as above, device pointers, any may be NULL.
 * Stream-ordered on `stream` like rpf_reduce_device; returns after the stream has drained (the pFilm check is read back). */
int32_t rpf_film_splat_device(rpf_ctx *ctx, const rpf_desc *desc, const rpf_film *film, const void *d_planes,
                              const double *d_colour, const float *d_ray_weight, float *d_tile_rgb, float *d_tile_weight,
                              float *d_image_rgb, void *stream);

/* The gather half-widths of the film step for the buffer of desc as the sample film: a sample of buffer pixel q can reach
 * output pixel x only if |q - x| <= half (floor(r + 0.5), or one more where fp32 rounding can close the gap; DESIGN.md
 * section 10).  half_y is the number of rows of each neighbour a row slab must hold for the film step.  Needs no context and
 * no device; refuses what rpf_filter_film refuses about desc and film, with the same status (radii, empty bounds,
 * coordinates beyond +-2^22, a sub-slab: RPF_E_BADARG; fp16 planes: RPF_E_UNSUPPORTED).  Either output may be NULL. */
int32_t rpf_film_window(const rpf_desc *desc, const rpf_film *film, int32_t *half_x, int32_t *half_y);

/* rpf_filter_film() for the whole image on every slab context of a rpf_multi: arguments, output shapes and meaning as
 * rpf_filter_film, any output may be NULL; results (samples, contribSum, filterWeightSum, image, status, merged counters)
 * are bit-identical to rpf_filter_film on one device -- VERIFIED with one, two and three slab contexts on ONE device; like
 * rpf_multi_filter, the peer-copy branch (two different ordinals) has still only run between slab contexts on one device.
 *   - refuses what rpf_multi_filter refuses (whole image only, ...) and what rpf_filter_film refuses for the whole frame,
 *     before anything is uploaded;
 *   - every slab holds depth = max(max over boxes of (box-1)/2, half_y of rpf_film_window for the whole image) rows of each
 *     neighbour, planes and ray weights; a slab that owns fewer rows is RPF_E_BADARG;
 *   - the pFilm check runs on every slab before any pass and is merged: the refusal names the first offender of the whole
 *     image in the reference's order, in whole-buffer coordinates, with rpf_filter_film's text;
 *   - after the last pass the colour halo is refreshed once more, then every slab runs the film step on its own buffer
 *     (origin moved to the buffer's first image row, output rows clipped to the rows it owns; the first / last slab also
 *     takes output rows above / below the sample film) and its rows go straight into the caller's arrays.  A slab whose rows
 *     meet no output row (a crop window elsewhere) does no film work;
 *   - RPF_E_NONFINITE as rpf_multi_filter: the film step still runs and every output is written. */
int32_t rpf_multi_filter_film(rpf_multi *m, const rpf_desc *desc, const rpf_film *film, const void *planes,
                              const float *ray_weight, float *sample_rgb_out, float *tile_rgb_out, float *tile_weight_out,
                              float *image_rgb_out);

/* ---- the spike pass: spike clamp and energy preservation after the last filter pass (RPF_FLAG_SPIKE_CLAMP) --------------
 * The reference leaves the HDR clamp and the energy-preservation step of the published algorithm out (commented,
 * rpf.cpp:707-713); a firefly that survives the passes goes straight into FilmTile::AddSample.  This pass is defined in
 * DESIGN.md section 12, in IEEE fp64 with every sum a serial chain in a stated order.  In short, on the filtered rows only:
 *   per pixel and channel k   m_k = mean of the S colours, sd_k = sqrt(sum (c - m_k)^2 / S);
 *   sample s is a spike       when |c_sk - m_k| > threshold * sd_k on ANY channel (strict; false against NaN: a pixel that
 *                             holds a NaN or an infinite colour has a NaN sd_k, flags nothing and is left as it is);
 *   n spikes of S             n == 0: untouched; n == S: untouched, counted as skipped; else every spike's three channels
 *                             become m'_k, the mean of the samples that passed, and e_k = sum over spikes of (c_sk - m'_k);
 *   energy                    E_k = sum over rows of (sum over x of e_k); delta_k = E_k / (rows * W * S); with
 *                             preserve_energy every sample of the filtered rows gets c += delta_k (all three channels, unless
 *                             all three delta_k are 0).  rayWeight plays no part.  Rows outside the slab keep their bits. */
typedef struct rpf_spike_stats {
    int64_t spike_samples;   /* samples replaced                                                      */
    int64_t spike_pixels;    /* pixels with 0 < n < S                                                 */
    int64_t skipped_pixels;  /* pixels with n == S                                                    */
    double energy[3];        /* E_k                                                                   */
    double delta[3];         /* delta_k as folded from E_k, whether or not preserve_energy added it  */
    float spike_ms;          /* RPF_FLAG_TIMING: the spike pass, first launch to the end of the add   */
    int32_t applied;         /* 1 when the most recent call ran the pass; 0 (and zeros above) otherwise */
} rpf_spike_stats;

/* threshold: finite, > 0 (default 1.0); preserve_energy: 0 or 1 (default 1); anything else is RPF_E_BADARG */
int32_t rpf_set_spike(rpf_ctx *ctx, double threshold, int32_t preserve_energy);
int32_t rpf_multi_set_spike(rpf_multi *m, double threshold, int32_t preserve_energy);
/* the spike pass of the most recent rpf_filter / _ex / _device / _film call (rpf_multi_*: merged over the slabs, the same
 * numbers as one context) */
int32_t rpf_query_spike(rpf_ctx *ctx, rpf_spike_stats *out);
int32_t rpf_multi_query_spike(rpf_multi *m, rpf_spike_stats *out);

/* The two halves, for a caller who owns the slabs (one context per process: the row sums of every slab are gathered in
 * image-row order, folded with rpf_spike_delta, and the same delta added on every slab).  d_colour: device, 3 fp64 planes
 * [3][H][W][S]; rows [row_begin, row_end) of desc are worked on.  Stream-ordered on `stream` like rpf_reduce_device; both
 * return after the stream has drained.
 *   rpf_spike_clamp_device   replaces the spikes; row_sums_out: HOST, [(row_end - row_begin)][3] doubles, the per-row sums of the
 *                            removed energy; stats_out (may be NULL): the three counts of these rows, applied = 1, energy and
 *                            delta as rpf_spike_delta folds these rows alone
 *   rpf_colour_add_device    c += delta[k] on every sample of the rows; delta: HOST, three doubles */
int32_t rpf_spike_clamp_device(rpf_ctx *ctx, const rpf_desc *desc, double *d_colour, double threshold, double *row_sums_out,
                               rpf_spike_stats *stats_out, void *stream);
int32_t rpf_colour_add_device(rpf_ctx *ctx, const rpf_desc *desc, double *d_colour, const double *delta, void *stream);

/* The fold every path uses: energy_out[k] = row_sums[0][k] + row_sums[1][k] + ... in row order, delta_out[k] = energy_out[k] /
 * (double)n_samples.  row_sums: [n_rows][3]; n_samples: the number of samples of those rows, rows * W * S.  Needs no context
 * and no device.  RPF_E_BADARG for a NULL pointer or a non-positive count. */
int32_t rpf_spike_delta(const double *row_sums, int64_t n_rows, int64_t n_samples, double *energy_out, double *delta_out);

/* ---- the per-pass activity report (RPF_FLAG_PASS_REPORT) ----------------------------------------------
 * What one pass did to the filtered rows [row_begin, row_end), in IEEE fp64 with every sum a serial chain whose first term is
 * its first element.  a = the pass's input colours, b = its output colours (before the spike pass), k = channel.
 *   per pixel, chains over s   m_k = sum (b-a)*(b-a), i_k = sum a*a, pa_k = sum a, pb_k = sum b, pm_k = (pb_k - pa_k)^2,
 *                              pi_k = pa_k^2.  A pixel with a non-finite value among its 6*S colours is BAD: it gives +0.0 to all
 *                              twelve, counts once in nonfinite_pixels, and its samples that hold a non-finite value count in
 *                              nonfinite_samples.  unchanged_samples: samples whose three b have the 64 bits of their a (bad
 *                              pixels included).
 *   per row, chains over x     the twelve pixel values, alpha_k, beta_k (k < n_feat) and W_r_c of every pixel; a weight that is
 *                              not finite gives +0.0 and counts in weights_nonfinite; alpha_zero / beta_zero count the entries
 *                              == 0.0.  sum / min / max of N, the pixels with N == S, the pixels per size class (N <= 8, 16, 32,
 *                              64, 128, 256, 448, 832, and above: the classes of the routes).
 *   per pass                   the rows folded in ascending image-row order by rpf_pass_report_fold: doubles as a chain, counts
 *                              summed, min_nbhd / max_nbhd the minimum / maximum.
 * Relative L2 moved per pass = sqrt(sum_k moved2[k] / sum_k in2[k]); of the pixel means, the same of pix_moved2 / pix_in2; mean
 * alpha_k = alpha_sum[k] / pixels; share of clamped alpha = alpha_zero[k] / pixels; share of N = S = own_only_pixels / pixels. */
#define RPF_REPORT_NCLASS 9
typedef struct rpf_report_row {
    double moved2[3], in2[3], pix_moved2[3], pix_in2[3];     /* sums over the row's pixels of m_k, i_k, pm_k, pi_k */
    double alpha_sum[3], wrc_sum, beta_sum[RPF_MAX_NDIM];
    int64_t sum_nbhd, own_only_pixels, class_pixels[RPF_REPORT_NCLASS];
    int64_t unchanged_samples, nonfinite_samples, nonfinite_pixels, weights_nonfinite;
    int64_t alpha_zero[3], beta_zero[RPF_MAX_NDIM];
    int32_t min_nbhd, max_nbhd;
} rpf_report_row;
typedef struct rpf_pass_report {
    int32_t applied;          /* 1 when the most recent call filled this entry, else 0 and zeros below */
    int32_t box, draws, route, rows; /* the pass's box, its draws (0: not sampled), its rpf_query_route, row_end - row_begin */
    int64_t pixels, samples;  /* rows*W, rows*W*S */
    rpf_report_row total;     /* the fold of the rows */
} rpf_pass_report;

/* Pass `pass` of the most recent call on ctx: its record | its (row_end - row_begin) row records, in row order (for a caller who
 * owns the slabs and folds them itself; n_rows must be that count, 0 rows and applied == 0 included) | merged over the slabs of a
 * rpf_multi: the rows of every slab gathered in image-row order and folded, the same numbers as one context; `route` and `draws`
 * are the first slab's.  An entry no pass of that call filled has applied = 0 and zeros.  RPF_E_BADARG for a NULL pointer, a
 * pass outside [0, RPF_MAX_BOXES) or a wrong n_rows. */
int32_t rpf_query_pass_report(rpf_ctx *ctx, int32_t pass, rpf_pass_report *out);
int32_t rpf_query_pass_report_rows(rpf_ctx *ctx, int32_t pass, rpf_report_row *rows_out, int64_t n_rows);
int32_t rpf_multi_query_pass_report(rpf_multi *m, int32_t pass, rpf_pass_report *out);

/* The device half, for a caller who owns the passes: the row records of rows [row_begin, row_end) of desc from device buffers --
 * d_col_in / d_col_out: 3 fp64 planes [3][H][W][S]; d_nbhd: int32 [H*W]; d_alpha [H*W][3], d_beta [H*W][n_feat], d_wrc [H*W]
 * fp64, each may be NULL (its fields are then zero).  rows_out: HOST, row_end - row_begin records.  Stream-ordered on `stream`
 * like rpf_spike_clamp_device; returns after the stream has drained. */
int32_t rpf_pass_report_rows_device(rpf_ctx *ctx, const rpf_desc *desc, const double *d_col_in, const double *d_col_out,
                                    const int32_t *d_nbhd, const double *d_alpha, const double *d_beta, const double *d_wrc,
                                    rpf_report_row *rows_out, void *stream);

/* The fold every path uses: *total_out = rows[0] folded with rows[1], rows[2], ... in that order.  Needs no context and no device.
 * RPF_E_BADARG for a NULL pointer or n_rows <= 0. */
int32_t rpf_pass_report_fold(const rpf_report_row *rows, int64_t n_rows, rpf_report_row *total_out);

/* ---- sampled neighbourhoods (RPF_FLAG_SAMPLED_NBHD) ---------------------------------------------
 * Pass p of a call has id pass_id0 + p and draws[p] draws per pixel (0: the pass runs as without the flag).  row_origin is the
 * image row of buffer row 0: the key of a pixel is formed from its IMAGE row, so a row slab draws what the whole image draws.
 * rpf_multi_* adds each slab's first buffer row to the caller's value; a caller who owns the slabs sets it, and sets pass_id0
 * when making one call per pass. */
typedef struct rpf_sampling {
    uint64_t seed;
    int32_t pass_id0;
    int32_t row_origin;
    int32_t draws[RPF_MAX_BOXES];
} rpf_sampling;

/* RPF_E_BADARG for a NULL pointer or a negative draw count; needs no device work.  The configuration stays until replaced. */
int32_t rpf_set_sampling(rpf_ctx *ctx, const rpf_sampling *cfg);
int32_t rpf_multi_set_sampling(rpf_multi *m, const rpf_sampling *cfg);

/* The Gaussian threshold table of a box: table_out[k] = floor(2^32 * C_k / C_(box-1)), k = 0 .. box - 2 (box - 1 entries),
 * C_k = sum_{j <= k} exp(-(j - b)^2 / (2 sigma^2)), b = (box - 1) / 2, sigma = box / 4.0, computed in long double.  A 32-bit
 * word u names the window column (or row) #{k : table[k] <= u}.  Host only; RPF_E_BADARG for NULL, an even box or a box
 * outside [1, 511]. */
int32_t rpf_sampling_table(int32_t box, uint32_t *table_out);

/* The draws of buffer pixel (x, y) of a W x H x S buffer in pass `pass` (index into cfg->draws) with `box`: the distinct
 * surviving visiting-order indices qq in ascending order, BEFORE the 3-sigma test; qq_out has room for cfg->draws[pass]
 * entries, *n_out tells how many were written.  Host only, no device.  RPF_E_BADARG for NULL, pass outside [0, RPF_MAX_BOXES),
 * a negative draw count, an even or out-of-range box, non-positive sizes or a pixel outside the buffer. */
int32_t rpf_sampling_draws(const rpf_sampling *cfg, int32_t pass, int32_t box, int32_t W, int32_t H, int32_t S, int32_t x,
                           int32_t y, int32_t *qq_out, int32_t *n_out);

/* ---- the membership test of stage 1b (RPF_FLAG_MEMBER_TEST) ----------------------------------------
 * Feature k < n_feat of the descriptor has a multiple mult[k] of the pixel's sigma and an absolute floor floor[k]; with
 * a = |(double)f_k - m_k|, lim = sd_k * mult[k] (one rounding) and fl = sd_k > floor[k] ? -inf : floor[k], a candidate is
 * rejected on k iff a >= lim && a > fl, and is a member iff no feature rejects it.  Every comparison with a NaN is false: a
 * NaN never rejects.  mult 3 with a negative floor on every feature is the reference's test on every input. */
typedef struct rpf_membership {
    double mult[RPF_MAX_NDIM];
    double floor[RPF_MAX_NDIM];
} rpf_membership;

/* RPF_E_BADARG for a NULL pointer, a mult that is not finite and > 0, or a floor that is NaN or +inf, in ANY of the
 * RPF_MAX_NDIM entries (so that a later descriptor with any n_feat is covered); needs no device work.  The configuration
 * stays until replaced. */
int32_t rpf_set_membership(rpf_ctx *ctx, const rpf_membership *cfg);
int32_t rpf_multi_set_membership(rpf_multi *m, const rpf_membership *cfg);

/* Fills all RPF_MAX_NDIM entries of *out (those from n_feat on as kind 0 has them).  Host only, no device.
 * kind 0, the reference: every multiple 3, every floor -1 (any 1 <= n_feat <= RPF_MAX_NDIM).
 * kind 1, "published, 19-dim layout": multiples 3, and 30 on features 3..5 and 9..11 (the world positions p0 and p1); floors
 * 0.1; needs n_feat == 12.  These constants are written down FROM MEMORY of the paper's Algorithm 2 (3 sigma generally, 30
 * sigma for world position, floor 0.1): the paper was not at hand, and nothing in the library depends on them.  A floor on a
 * world position is scene-scale dependent (positions span +-10^3): a caller is expected to set those floors for
 * the scene, the preset is a convenience.
 * RPF_E_BADARG for NULL, an unknown kind, n_feat outside [1, RPF_MAX_NDIM], or kind 1 with n_feat != 12. */
int32_t rpf_membership_preset(int32_t kind, int32_t n_feat, rpf_membership *out);

/* ---- the per-pass schedule of the weight stage (RPF_FLAG_SCHEDULE) ----------------------------------
 * Pass p of a call reads entry e = pass0 + p.  With W_r^{c,k} and W_r^{f,k} the ratios stage 3c forms today (same sums, same
 * order, the policy's epsilon in the denominators), in IEEE fp64 without contraction:
 *   alpha_k = clamp0(1 - gain_c[e] * W_r^{c,k}),  beta_k = clamp0(1 - gain_f[e] * W_r^{f,k}) * W_c^{f,k},
 *   clamp0(v) = (v < 0) ? 0.0 : v  (a NaN stays a NaN), the product and the difference rounded once each,
 * and seed[e] stands where desc.sigma_seed stood.  A pass with both gains exactly 1.0 runs the unscheduled statements. */
typedef struct rpf_schedule {
    int32_t pass0;                    /* pass p of a call reads entry pass0 + p (rpf_sampling.pass_id0's part for a caller who makes one call per pass) */
    int32_t reserved;                 /* 0 */
    double  seed[RPF_MAX_BOXES];      /* replaces desc.sigma_seed for that pass: sigma_c^2 = sigma_f^2 = seed^2 / (1 - W_r_c)^2 */
    double  gain_c[RPF_MAX_BOXES];    /* g_c: alpha_k = clamp0(1 - g_c * W_r^{c,k}) */
    double  gain_f[RPF_MAX_BOXES];    /* g_f: beta_k  = clamp0(1 - g_f * W_r^{f,k}) * W_c^{f,k} */
} rpf_schedule;

/* RPF_E_BADARG for a NULL pointer, pass0 outside [0, RPF_MAX_BOXES), a seed that is not finite and > 0, or a gain that is not
 * finite and >= 0, in ANY of the RPF_MAX_BOXES entries; needs no device work.  The configuration stays until replaced. */
int32_t rpf_set_schedule(rpf_ctx *ctx, const rpf_schedule *cfg);
int32_t rpf_multi_set_schedule(rpf_multi *m, const rpf_schedule *cfg);

/* Fills *out (pass0 = 0, reserved = 0, all RPF_MAX_BOXES entries).  Host only, no device.  S: samples per pixel.
 * kind 0, the reference: every seed 0.002, every gain 1.
 * kind 1, "published": seed[t] = sqrt(8.0 * v_t / (double)S) with v_0 = 0.02 and v_t = 0.002 otherwise, gain_c[t] =
 * 2.0 * (1.0 + 0.1 * t), gain_f[t] = 1.0 + 0.1 * t, formed in C doubles in exactly these expressions.  These constants are
 * written down FROM MEMORY of the paper (sigma^2 = 8 sigma_8^2 / spp with sigma_8^2 = 0.02 in the first iteration and 0.002
 * afterwards; alpha = max(1 - 2 (1 + 0.1 t) W_r^c, 0), beta = W_c^f max(1 - (1 + 0.1 t) W_r^f, 0)): the paper was not at hand,
 * and nothing in the library depends on them.
 * RPF_E_BADARG for NULL, an unknown kind, or S <= 0. */
int32_t rpf_schedule_preset(int32_t kind, int32_t S, rpf_schedule *out);

#ifdef __cplusplus
}
#endif
#endif
