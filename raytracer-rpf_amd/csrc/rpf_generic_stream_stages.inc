// rpf_generic_stream_stages.inc -- the stages that generic::filter_pixel_kernel (rpf_generic.hip) and generic::filter_wide_kernel
// (rpf_generic_wide.hip) run with the same statements on the same thread mapping (256 threads, one pixel): one copy, included
// into the pixel loop of both kernels.  RPF_STREAM_PART 1: stages 1b, 2 and 3a and the debug hashes; 2: stage 3c; 3: stage 4 in
// fp64 and the status report; 4: stage 4 in the fp32 arithmetic of RPF_FLAG_STREAM_FAST (DESIGN.md section 11f) and the status
// report -- the kernels' FAST instantiations include part 4 where the others include part 3, and nothing else differs between
// them.  Between parts 1 and 2 each kernel has its own stage 3b (16-bit cells in LDS | 32-bit cells in bands).
//
// Text, not functions, and the statements spelled out rather than calls of rpf_generic_common.h's small functions: both forms
// were built and measured (profiles/generic_refactor_parent_vs_new.txt, sections 3 and 4).  Same bits, same waves per SIMD, no
// scratch either way, but filter_pixel_kernel<float> came out +0.4 to +0.7 % (stage functions) and +0.7 to +1.8 % (small functions
// called from this text, bodies inline: 142.62 -> 143.60 ms, 74.62 -> 75.97 ms, 189.84 -> 192.33 ms) on the route-3 legs of the
// 1920x270x8 slabs, outside the parent's own spread.  filter_wide_kernel passed both of its legs in the second form; it keeps
// this text because it is one text with filter_pixel_kernel's.  As it stands both kernels' assembly is the parent's.
//
// Names the including kernel provides: p, D and ndim, nF, nR, nAnc, npair, nwt, colF; tid, lane, wv; W, H, S, b, HW; pix, x, y;
// e_eps; list, bins and the type Bin of a bin id; sStat, sZ, sMI, sW, sRedD, sChunk, sRed4, sCnt; for part 4 also smem and cv (the
// start of the dynamic LDS and the carve-up, whose off_chunk it rounds up); for part 1 also the compile-time constants kMemberTest
// and kListed and, where kMemberTest is true, mtab (RPF_FLAG_MEMBER_TEST: mult[RPF_MAX_NDIM] | floor[RPF_MAX_NDIM] on the device; DESIGN.md section 14).
// The statements under kMemberTest are discarded where it is false, and so is one side of kListed: such a kernel sees the text it saw.
// Part 1 leaves n, B and dn.
#if RPF_STREAM_PART == 1
        // ---- stage 1b: the 3-sigma test and the member list, reference order (rpf.cpp:556-586) -------------------
        // kListed (the rest launch of a sampled pass; DESIGN.md section 13e): no walk of the box -- N is what the count kernel wrote, the
        // members behind the own samples are those it listed, in its order, and p.nbhd is not rewritten
        for (int s = tid; s < S; s += kThreads) list[s] = (uint32_t)(pix * S + s); // own samples first
        int n = S;
        if constexpr (kListed) {
            n = min(p.nbhd[pix], p.nmax); // (S + draws <= p.nmax by the route's construction: the clamp never bites)
            const uint64_t mb = n > S ? p.member_base[pix] : 0ull; // (a pixel that lists nothing has no base)
            for (int i = tid; i < n - S; i += kThreads) list[S + i] = p.members[mb + i];
        } else {
            const int x0 = max(x - b, 0), x1 = min(x + b, W - 1), y0 = max(y - b, 0), y1 = min(y + b, H - 1);
            const int nyv = y1 - y0 + 1;
            const int centre_rank = (x - x0) * nyv + (y - y0);
            const int ncand = ((x1 - x0 + 1) * nyv - 1) * S;
            double *sMf = sChunk + 8, *sLf = sMf + nF;
            for (int k = tid; k < nF; k += kThreads) {
                sMf[k] = p.pmean[(uint64_t)k * HW + pix];
                if constexpr (kMemberTest) { // lim_k = sd_k * mult_k, fl_k = -inf where sd_k is above the floor (behind sLf)
                    const double sd = p.pstd[(uint64_t)k * HW + pix], fk = mtab[RPF_MAX_NDIM + k];
                    sLf[k] = sd * mtab[k];
                    sLf[nF + k] = sd > fk ? -__builtin_inf() : fk;
                } else {
                    sLf[k] = p.pstd[(uint64_t)k * HW + pix] * 3.0; // multiplyArray(std, 3), rpf.cpp:579
                }
            }
            __syncthreads();
            for (int q0 = 0; q0 < ncand; q0 += kThreads) {
                const int qb = q0 + wv * 64;                       // this wave's 64-candidate block
                unsigned long long mask = 0ull;
                uint32_t off = 0u;
                if (qb < ncand) { // wave-uniform
                    const int qq = qb + lane;
                    bool pass = qq < ncand;
                    if (pass) {
                        int cell = qq / S;
                        const int s = qq - cell * S;
                        if (cell >= centre_rank) ++cell;              // rpf.cpp:565: skip the centre pixel
                        const int ix = cell / nyv, iy = cell - ix * nyv; // xn outer, yn inner ascending (rpf.cpp:562-563)
                        off = (uint32_t)(((uint64_t)(y0 + iy) * W + (x0 + ix)) * S + s);
                        for (int k = 0; k < nF; ++k) {
                            const double a = fabs((double)ldp<T>(p, colF + k, off) - sMf[k]);
                            if constexpr (kMemberTest) {
                                if (a >= sLf[k] && a > sLf[nF + k]) pass = false; // a NaN never rejects here either
                            } else {
                                if (a >= sLf[k]) pass = false;     // allLessThan: fails iff a >= b (ops.h:101-104): a NaN never rejects
                            }
                        }
                    }
                    mask = __ballot(pass);
                }
                if (lane == 0) sCnt[wv] = __popcll(mask);
                __syncthreads();
                int base = n;
                for (int w = 0; w < wv; ++w) base += sCnt[w];
                const int tot = sCnt[0] + sCnt[1] + sCnt[2] + sCnt[3];
                if ((mask >> lane) & 1ull) {
                    const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
                    if (at < p.nmax) list[at] = off;
                }
                n += tot;
                __syncthreads();
            }
            if (tid == 0) p.nbhd[pix] = n;
        }
        __threadfence_block();
        __syncthreads();
        const int B = max(1, (int)sqrt((double)n));                // mi.cpp:54
        const double dn = (double)n;

        // ---- stage 2: in-order sums over the neighbourhood (rpf.cpp:596-601), chunks of 64 staged through LDS ------
        // lane c of wave 0 adds column c's x front to back, lane c of wave 1 its x*x: one thread per chain
        {
            double acc = 0.0;
            const bool chain = wv < 2 && lane < ndim, is_sq = wv == 1;
            for (int j0 = 0; j0 < n; j0 += kChunk) {
                const int cnt = min(kChunk, n - j0);
                for (int t = tid; t < cnt * ndim; t += kThreads) {
                    const int c = t / cnt, q = t - c * cnt;
                    sChunk[c * (kChunk + 1) + q] = load_col<T>(p, c, list[j0 + q]);
                }
                __syncthreads();
                if (chain) {
                    const double *src = sChunk + lane * (kChunk + 1);
                    for (int q = 0; q < cnt; ++q) { const double v = src[q]; acc = acc + (is_sq ? v * v : v); } // ops.h:121, 138
                }
                __syncthreads();
            }
            if (chain && is_sq) sRedD[lane] = acc;
            __syncthreads();
            if (chain && !is_sq) {
                const double sq = sRedD[lane];
                const double mean = acc / dn;                                  // ops.h:123
                double sd = sqrt(sq / dn - mean * mean);                       // ops.h:141
                if (p.policy == RPF_DEGEN_EPS && isnan(sd)) sd = 0.0;
                sStat[lane] = mean; sStat[ndim + lane] = sd;
                if (p.dbg.mean) p.dbg.mean[pix * ndim + lane] = mean;
                if (p.dbg.stddev) p.dbg.stddev[pix * ndim + lane] = sd;
            }
        }
        // column minima / maxima (order-free), then the per-column constants of the binning (sd.h:229-232, mi.cpp:47-50)
        for (int c = wv; c < ndim; c += kThreads / 64) { // a column per wave
            double mn = INFINITY, mx = -INFINITY;
            for (int j = lane; j < n; j += 64) { const double v = load_col<T>(p, c, list[j]); mn = fmin(mn, v); mx = fmax(mx, v); }
            for (int s = 32; s > 0; s >>= 1) { mn = fmin(mn, __shfl_down(mn, s, 64)); mx = fmax(mx, __shfl_down(mx, s, 64)); }
            if (lane == 0) { sStat[2 * ndim + c] = mn; sStat[3 * ndim + c] = mx; }
        }
        __syncthreads();
        if (tid < ndim) {
            const double Mc = sStat[tid], SDc = sStat[ndim + tid];
            const bool sd0 = (SDc == 0.0);
            const double lo = sd0 ? 0.0 : (sStat[2 * ndim + tid] - Mc) / SDc, hi = sd0 ? 0.0 : (sStat[3 * ndim + tid] - Mc) / SDc;
            sZ[tid] = lo; sZ[ndim + tid] = hi - lo;
            sZ[2 * ndim + tid] = (double)((sd0 ? 1 : 0) | (!(hi != lo) ? 2 : 0)); // mi.cpp:7 / 28 / 34
        }
        __syncthreads();

        // ---- stage 3a: normalise, bin ids (one Bin per sample and column) ------------------------------------------
        for (int c = 0; c < ndim; ++c) {
            const double Mc = sStat[c], SDc = sStat[ndim + c], lo = sZ[c], range = sZ[ndim + c];
            const int flags = (int)sZ[2 * ndim + c];
            const bool sd0 = flags & 1, flat = flags & 2;
            Bin *bc = bins + (uint64_t)c * p.nmax;
            for (int j = tid; j < n; j += kThreads) {
                int bin = 0;
                if (!flat) {
                    const double a = load_col<T>(p, c, list[j]) - Mc;       // subtractArrays
                    const double z = sd0 ? 0.0 : a / SDc;                      // divideArrays, ops.h:48
                    const double t = (z - lo) / range * (double)B;             // mi.cpp:14
                    bin = max(min((int)t, B - 1), 0);
                }
                bc[j] = (Bin)bin;
            }
        }
        __threadfence_block();
        __syncthreads();
        if (p.dbg.member_hash != nullptr && tid == 0) {
            uint32_t h = 2166136261u;
            for (int j = 0; j < n; ++j) {
                const uint32_t o = list[j], s = o % (uint32_t)S, q = o / (uint32_t)S;
                const int yn = (int)(q / (uint32_t)W), xn = (int)(q % (uint32_t)W);
                h = fnv1a_u32(h, (uint32_t)(((xn - x + b) * p.box + (yn - y + b)) * S) + s);
            }
            p.dbg.member_hash[pix] = h;
        }
        if (p.dbg.bin_hash != nullptr && tid < ndim) {
            uint32_t h = 2166136261u;
            const Bin *bc = bins + (uint64_t)tid * p.nmax;
            for (int j = 0; j < n; ++j) h = fnv1a_u16(h, bc[j]);
            p.dbg.bin_hash[pix * ndim + tid] = h;
        }
#elif RPF_STREAM_PART == 2
        // ---- stage 3c: alpha, beta, W_r_c (rpf.cpp:444-487) ----------------------------------------------------------
        double *sDrf = sW, *sD9 = sDrf + nF, *sAlpha = sD9 + 12, *sBeta = sAlpha + 4, *sWrc = sBeta + nF;
        {
            const int k = min(tid, nF - 1), c = min(tid, 2);
            double Drf = 0.0, Dpf = 0.0, Dcf = 0.0, Drc = 0.0, Dpc = 0.0, Dfc = 0.0;
            const int base = D.npairF + c * D.npairC;
            for (int l = 0; l < nR; ++l) { Drf += sMI[k * nAnc + l]; Drc += sMI[base + l]; }                 // rpf.cpp:421, 432
            for (int l = 0; l < 2; ++l) { Dpf += sMI[k * nAnc + nR + l]; Dpc += sMI[base + nR + l]; }        // rpf.cpp:425, 436
            for (int cc = 0; cc < 3; ++cc) Dcf += sMI[D.npairF + cc * D.npairC + nAnc + k];
            for (int j = 0; j < nF; ++j) Dfc += sMI[base + nAnc + j];                                        // rpf.cpp:440
            if (tid < nF) sDrf[tid] = Drf;
            if (tid < 3) { sD9[tid] = Drc; sD9[3 + tid] = Dpc; sD9[6 + tid] = Dfc; }
            __syncthreads();
            double D_f_c = 0.0, D_r_c = 0.0, D_p_c = 0.0;                                                    // rpf.cpp:449-456
            for (int i = 0; i < 3; ++i) { D_f_c += sD9[6 + i]; D_r_c += sD9[i]; D_p_c += sD9[3 + i]; }
            const double den = D_f_c + D_r_c + D_p_c + e_eps;
            double wsum = 0.0;
            for (int i = 0; i < 3; ++i) wsum += sD9[i] / (sD9[i] + sD9[3 + i] + e_eps);                      // rpf.cpp:470, 485
            const double wrc = wsum / 3;                                                                     // rpf.cpp:487
            const bool sched = (p.generic & kGenericSchedule) != 0; // RPF_FLAG_SCHEDULE with a gain other than 1: uniform
            double alpha_c;
            if (sched) alpha_c = schedule_factor(p.gain_c, Drc / (Drc + Dpc + e_eps));                       // clamp0(1 - g_c W_r^{c,k})
            else alpha_c = 1 - Drc / (Drc + Dpc + e_eps);                                                    // rpf.cpp:470, 475
            // the beta presets keep the reference's stack rule for any nF: k < 3 reads D_f_ck, a gap of zeros, then D_r_fk
            double num;
            if (p.beta_map == RPF_BETA_PAPER) num = Dcf;
            else if (p.beta_map == RPF_BETA_REF_GCC11_O2) num = k < 3 ? sD9[6 + c] : (k < 8 ? 0.0 : sDrf[max(k - 8, 0)]);
            else num = k < 3 ? sD9[6 + c] : (k < 4 ? 0.0 : sDrf[max(k - 4, 0)]);
            double beta_k;
            if (sched) beta_k = schedule_factor(p.gain_f, Drf / (Drf + Dpf + e_eps)) * (num / den);          // clamp0(1 - g_f W_r^{f,k}) W_c^{f,k}
            else beta_k = (1 - Drf / (Drf + Dpf + e_eps)) * (num / den);                                     // rpf.cpp:464-465, 479
            if (tid < nF) { sBeta[tid] = beta_k; if (p.dbg.beta) p.dbg.beta[pix * nF + tid] = beta_k; }
            if (tid < 3) { sAlpha[tid] = alpha_c; if (p.dbg.alpha) p.dbg.alpha[pix * 3 + tid] = alpha_c; }
            if (tid == 0) { sWrc[0] = wrc; if (p.dbg.wrc) p.dbg.wrc[pix] = wrc; }
            __syncthreads();
        }

#elif RPF_STREAM_PART == 3
        // ---- stage 4: weights and blend, term by term as rpf.cpp:646-717; kOwn own samples per sweep.  The column loop is
        // outermost: a neighbour's value of column k is loaded and normalised once, then the kOwn own samples' sp / sc / sf
        // take its term -- each accumulator still receives its terms in ascending k (the reference's order).
        {
            const double wrc = sWrc[0];
            const double sigma_c2 = p.seed * p.seed / (1 - wrc) / (1 - wrc);                                  // rpf.cpp:662
            const double sigma_p2 = p.sigma_p * p.sigma_p;
            auto znorm = [&](int c, double xv) { const double sd = sStat[ndim + c]; return sd == 0.0 ? 0.0 : (xv - sStat[c]) / sd; };
            double *sOwnZ = sChunk; // [nwt][kOwn] normalised own samples of the sweep (the staging chunk is dead)
            bool bad = false;
            for (int i0 = 0; i0 < S; i0 += kOwn) {
                __syncthreads();
                for (int t = tid; t < kOwn * nwt; t += kThreads) {
                    const int k = t / kOwn, ii = t % kOwn, i = min(i0 + ii, S - 1);
                    const int col = k < 5 ? k : k + nR;
                    sOwnZ[t] = znorm(col, load_col<T>(p, col, (uint32_t)(pix * S + i)));
                }
                __syncthreads();
                double sw[kOwn], s0[kOwn], s1[kOwn], s2[kOwn];
#pragma unroll
                for (int ii = 0; ii < kOwn; ++ii) { sw[ii] = 0.0; s0[ii] = 0.0; s1[ii] = 0.0; s2[ii] = 0.0; }
                for (int j = tid; j < n; j += kThreads) {
                    const uint32_t off = list[j];
                    double sp[kOwn], sc[kOwn], sf[kOwn], cj[3];
#pragma unroll
                    for (int ii = 0; ii < kOwn; ++ii) { sp[ii] = 0.0; sc[ii] = 0.0; sf[ii] = 0.0; }
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const double zj = znorm(k, (double)ldp<T>(p, k, off));
#pragma unroll
                        for (int ii = 0; ii < kOwn; ++ii) { const double t = sOwnZ[k * kOwn + ii] - zj; sp[ii] += t * t; }
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        cj[k] = p.col_in[(uint64_t)k * p.plane_stride + off];
                        const double zj = znorm(2 + k, cj[k]), ak = sAlpha[k];
#pragma unroll
                        for (int ii = 0; ii < kOwn; ++ii) { const double t = sOwnZ[(2 + k) * kOwn + ii] - zj; sc[ii] += (t * t) * ak; }
                    }
                    for (int k = 0; k < nF; ++k) {
                        const double zj = znorm(colF + k, (double)ldp<T>(p, colF + k, off)), bk = sBeta[k];
#pragma unroll
                        for (int ii = 0; ii < kOwn; ++ii) { const double t = sOwnZ[(5 + k) * kOwn + ii] - zj; sf[ii] += (t * t) * bk; }
                    }
#pragma unroll
                    for (int ii = 0; ii < kOwn; ++ii) {
                        double w = exp(-sp[ii] / (2 * sigma_p2)) * exp(-sc[ii] / (2 * sigma_c2)) * exp(-sf[ii] / (2 * sigma_c2)); // rpf.cpp:667-670
                        w = (i0 + ii < S) ? w : 0.0;
                        sw[ii] += w; s0[ii] += w * cj[0]; s1[ii] += w * cj[1]; s2[ii] += w * cj[2];   // rpf.cpp:691-692
                    }
                }
                // the four sums of an own sample are reduced in the pairing of a halving tree over the 256 threads:
                // v[t] + v[t + 128], + 64 across the waves, then 32 ... 1 inside wave 0
#pragma unroll
                for (int ii = 0; ii < kOwn; ++ii) {
                    __syncthreads();
                    sRed4[tid] = sw[ii]; sRed4[kThreads + tid] = s0[ii];
                    sRed4[2 * kThreads + tid] = s1[ii]; sRed4[3 * kThreads + tid] = s2[ii];
                    __syncthreads();
                    if (wv == 0) {
                        double v[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const double *r = sRed4 + q * kThreads + lane;
                            double a = (r[0] + r[128]) + (r[64] + r[192]);
                            for (int s = 32; s > 0; s >>= 1) a = a + __shfl_down(a, s, 64);
                            v[q] = __shfl(a, 0, 64);
                        }
                        const int i = i0 + ii;
                        if (lane < 3 && i < S) {
                            double prime = (lane == 0 ? v[1] : (lane == 1 ? v[2] : v[3])) / v[0];                 // rpf.cpp:700
                            if (isnan(prime)) {                                                                    // rpf.cpp:702
                                bad = true;
                                if (p.policy == RPF_DEGEN_EPS) prime = p.col_in[(uint64_t)lane * p.plane_stride + pix * S + i];
                            }
                            p.col_out[(uint64_t)lane * p.plane_stride + pix * S + i] = prime;
                        }
                    }
                }
            }
            const int anybad = __syncthreads_or(bad ? 1 : 0);
            if (tid == 0 && anybad) {
                atomicAdd(&p.status[0], 1);
                atomicMin(&p.status[1], (int)pix);
            }
        }
#elif RPF_STREAM_PART == 4
        // ---- stage 4 under RPF_FLAG_STREAM_FAST: the pair arithmetic in fp32 (DESIGN.md section 11f), kStreamFastOwn own samples
        // per sweep.  Once per pixel: 1 / SD per column (fp64; the slots of the column minima and maxima are dead), which columns
        // have SD == 0 (z = 0 there) as one wave-uniform mask, and the coefficients of the summed exponent with log2 e folded in,
        // formed in fp64 and rounded once (the sums of stage 3c they overwrite are dead).  A member's z = (x - M) * (1 / SD) is
        // formed in fp64 and rounded once; d = z_i - z_j, d * d and E += (d * d) * coef are fp32 with one accumulator per own
        // sample, two own samples to a packed instruction; one hardware exponential; the weight widened to fp64.  The four sums,
        // the halving tree, the quotient, the padding rule and the status report are part 3's statements.
        {
            constexpr int kFO = kStreamFastOwn;
            const double wrc = sWrc[0];
            const double sigma_c2 = p.seed * p.seed / (1 - wrc) / (1 - wrc);                                  // rpf.cpp:662
            const double sigma_p2 = p.sigma_p * p.sigma_p;
            const double kLog2e = 1.4426950408889634;
            double *sInv = sStat + 2 * ndim;
            float *sCoef = reinterpret_cast<float *>(sDrf);
            const double sdl = sStat[ndim + min(lane, ndim - 1)];
            const unsigned long long sd0mask = __ballot(lane < ndim && sdl == 0.0); // (every wave forms the same mask)
            if (tid < ndim) sInv[tid] = 1.0 / sdl;
            if (tid < nwt)
                sCoef[tid] = (float)((tid < 2 ? 1.0 / (2 * sigma_p2) : (tid < 5 ? sAlpha[tid - 2] : sBeta[tid - 5]) / (2 * sigma_c2)) * kLog2e);
            auto zfast = [&](int c, double xv) { return ((sd0mask >> c) & 1ull) ? 0.f : (float)((xv - sStat[c]) * sInv[c]); };
            // [nwt][kFO] normalised own samples of the sweep, in the dead staging chunk from its first 16-byte boundary on (the
            // carve-ups leave the room): term() reads them as 16-byte vectors
            float *sOwnZ = reinterpret_cast<float *>(smem + up16(cv.off_chunk));
            bool bad = false;
            for (int i0 = 0; i0 < S; i0 += kFO) {
                __syncthreads();
                for (int t = tid; t < kFO * nwt; t += kThreads) {
                    const int k = t / kFO, ii = t % kFO, i = min(i0 + ii, S - 1);
                    const int col = k < 5 ? k : k + nR;
                    sOwnZ[t] = zfast(col, load_col<T>(p, col, (uint32_t)(pix * S + i)));
                }
                __syncthreads();
                double sw[kFO], s0[kFO], s1[kFO], s2[kFO];
#pragma unroll
                for (int ii = 0; ii < kFO; ++ii) { sw[ii] = 0.0; s0[ii] = 0.0; s1[ii] = 0.0; s2[ii] = 0.0; }
                for (int j = tid; j < n; j += kThreads) {
                    const uint32_t off = list[j];
                    f32x2 E[kFO / 2];
#pragma unroll
                    for (int q = 0; q < kFO / 2; ++q) E[q] = f32x2{0.f, 0.f};
                    double cj[3];
                    // one accumulator per own sample takes the column's term, two own samples to a packed instruction
                    auto term = [&](int k, float zj) {
                        const float ck = sCoef[k];
                        const f32x2 zj2 = f32x2{zj, zj}, ck2 = f32x2{ck, ck};
#pragma unroll
                        for (int q4 = 0; q4 < kFO / 4; ++q4) {
                            const f32x4a zo = *reinterpret_cast<const f32x4a *>(sOwnZ + k * kFO + 4 * q4);
                            const f32x2 da = f32x2{zo[0], zo[1]} - zj2, db = f32x2{zo[2], zo[3]} - zj2;
                            E[2 * q4] = __builtin_elementwise_fma(da * da, ck2, E[2 * q4]);
                            E[2 * q4 + 1] = __builtin_elementwise_fma(db * db, ck2, E[2 * q4 + 1]);
                        }
                    };
                    // every gather of the member that needs no loop is issued here, the features kStreamGather at a time with
                    // the next group in flight while this one is weighed
                    const float pf0 = ldp<T>(p, 0, off), pf1 = ldp<T>(p, 1, off);
#pragma unroll
                    for (int k = 0; k < 3; ++k) cj[k] = p.col_in[(uint64_t)k * p.plane_stride + off];
                    float fv[kStreamGather];
#pragma unroll
                    for (int u = 0; u < kStreamGather; ++u) fv[u] = ldp<T>(p, colF + min(u, nF - 1), off);
                    term(0, zfast(0, (double)pf0));
                    term(1, zfast(1, (double)pf1));
#pragma unroll
                    for (int k = 0; k < 3; ++k) term(2 + k, zfast(2 + k, cj[k]));
                    for (int k0 = 0; k0 < nF; k0 += kStreamGather) {
                        float cur[kStreamGather];
#pragma unroll
                        for (int u = 0; u < kStreamGather; ++u) cur[u] = fv[u];
                        if (k0 + kStreamGather < nF) {
#pragma unroll
                            for (int u = 0; u < kStreamGather; ++u) fv[u] = ldp<T>(p, colF + min(k0 + kStreamGather + u, nF - 1), off);
                        }
#pragma unroll
                        for (int u = 0; u < kStreamGather; ++u) {
                            const int k = k0 + u;
                            if (k >= nF) break;
                            term(5 + k, zfast(colF + k, (double)cur[u]));
                        }
                    }
#pragma unroll
                    for (int ii = 0; ii < kFO; ++ii) {
                        double w = (double)__builtin_amdgcn_exp2f(-E[ii >> 1][ii & 1]);
                        w = (i0 + ii < S) ? w : 0.0;
                        sw[ii] += w; s0[ii] += w * cj[0]; s1[ii] += w * cj[1]; s2[ii] += w * cj[2];   // rpf.cpp:691-692
                    }
                }
                // the four sums of an own sample are reduced in the pairing of a halving tree over the 256 threads:
                // v[t] + v[t + 128], + 64 across the waves, then 32 ... 1 inside wave 0
#pragma unroll
                for (int ii = 0; ii < kFO; ++ii) {
                    if (i0 + ii >= S) break; // workgroup-uniform: a padding sample stores nothing
                    __syncthreads();
                    sRed4[tid] = sw[ii]; sRed4[kThreads + tid] = s0[ii];
                    sRed4[2 * kThreads + tid] = s1[ii]; sRed4[3 * kThreads + tid] = s2[ii];
                    __syncthreads();
                    if (wv == 0) {
                        double v[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const double *r = sRed4 + q * kThreads + lane;
                            double a = (r[0] + r[128]) + (r[64] + r[192]);
                            for (int s = 32; s > 0; s >>= 1) a = a + __shfl_down(a, s, 64);
                            v[q] = __shfl(a, 0, 64);
                        }
                        const int i = i0 + ii;
                        if (lane < 3 && i < S) {
                            double prime = (lane == 0 ? v[1] : (lane == 1 ? v[2] : v[3])) / v[0];                 // rpf.cpp:700
                            if (isnan(prime)) {                                                                    // rpf.cpp:702
                                bad = true;
                                if (p.policy == RPF_DEGEN_EPS) prime = p.col_in[(uint64_t)lane * p.plane_stride + pix * S + i];
                            }
                            p.col_out[(uint64_t)lane * p.plane_stride + pix * S + i] = prime;
                        }
                    }
                }
            }
            const int anybad = __syncthreads_or(bad ? 1 : 0);
            if (tid == 0 && anybad) {
                atomicAdd(&p.status[0], 1);
                atomicMin(&p.status[1], (int)pix);
            }
        }
#else
#error "RPF_STREAM_PART must be 1, 2, 3 or 4"
#endif
#undef RPF_STREAM_PART
