// rpf_generic_sampled_bitmap.inc -- steps 1 to 4 of the bitmap count kernels of a sampled pass (rpf_generic_sampled_mask.hip:
// sampled_count_mask_kernel of route 11 and sampled_count_list_kernel of route 12; DESIGN.md sections 13f and 13g), the statements
// the two kernels share.  Included inside the kernel's body, after `extern __shared__ ... sm_lds[]`, with T, MEMBER, p and o of the
// kernel in scope; o has table, seed, pass_id, row_origin, draws, queue_bytes and member, and p.mask_stride holds the u64 words of a
// wave's bitmap (ncand <= 64 * p.mask_stride).  A wave without a pixel returns from the kernel here.  Leaves, for the kernel's last
// step: bits (the accepted candidates of the window), win, pix, lane, nw (the words the window uses), S, W and acc.
// These are the statements sampled_count_mask_kernel had in its body: that kernel's device assembly is what it was
// (profiles/sampled_listed_parent_vs_new.txt).
    uint32_t *sT = reinterpret_cast<uint32_t *>(sm_lds); // [kScTable]
    const int nT = p.box - 1;
    for (int k = threadIdx.x; k < nT; k += 256) sT[k] = o.table[k];
    __syncthreads(); // the only barrier: before any wave leaves
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t npix = (uint32_t)(p.row_end - p.row_begin) * (uint32_t)p.W;
    const uint32_t e = blockIdx.x * 4u + (uint32_t)wv;
    if (e >= npix) return; // wave-uniform
    const uint32_t wave_bytes = p.mask_stride * 8u + o.queue_bytes;
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(sm_lds + kScTable * 4u + (uint32_t)wv * wave_bytes); // [mask_stride]
    uint16_t *queue = reinterpret_cast<uint16_t *>(bits + p.mask_stride);                                            // [draws]
    const int W = p.W, H = p.H, S = p.S, b = p.b;
    const uint64_t HW = (uint64_t)H * W;
    const uint64_t pix = (uint64_t)p.row_begin * W + e;
    const int y = (int)(pix / (uint32_t)W), x = (int)(pix - (uint64_t)y * W);
    const int nF = p.lay.nF, colF = 5 + p.lay.nR;
    const int D = o.draws; // 1 .. kMaxResident - S (the route's condition)

    const uint64_t h = sc_pixel_key(o, x, y);
    const Window win = make_window(x, y, b, W, H, S);
    const int nw = (win.ncand + 63) >> 6; // <= p.mask_stride (the launch checks the stride against the box)

    // ---- 1, 2: the bitmap of the pixel's D draws (DESIGN.md section 13a) ------------------------------------------------------
    for (int w = lane; w < nw; w += 64) bits[w] = 0ull;
    wsync();
    for (int q = lane; q < D; q += 64) {
        const uint32_t qq = sc_draw(h, q, sT, nT, win, x, y, b, W, H, S); // < ncand, or kScNone
        if (qq != kScNone) atomicOr(&bits[qq >> 6], 1ull << (qq & 63u));
    }
    wsync();
    // ---- 3: the set bits in ascending qq, at most min(D, ncand) of them ------------------------------------------------------
    int qn = 0;
    for (int w0 = 0; w0 < nw; w0 += 64) {
        const int w = w0 + lane;
        unsigned long long m = w < nw ? bits[w] : 0ull;
        const int cnt = __popcll(m);
        int incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        int at = qn + incl - cnt;
        while (m != 0ull) {
            queue[at++] = (uint16_t)(w * 64 + (__ffsll((long long)m) - 1));
            m &= m - 1ull;
        }
        qn += __shfl(incl, 63, 64);
    }
    wsync();
    // ---- 4: stage 1b's test on the distinct draws, 64 at a time (rpf.cpp:576-586) ----------------------------------------------
    int acc = 0;
    for (int kb = 0; kb < qn; kb += 64) {
        const int k = kb + lane;
        const bool live = k < qn;
        const uint32_t qq = live ? (uint32_t)queue[k] : 0u;
        const uint32_t off = live ? candidate_offset(win, W, S, (int)qq) : 0u;
        const bool pass = passes_stage1b_wave<T, MEMBER>(p, o.member, colF, nF, off, HW, pix, live);
        if (live && !pass) atomicAnd(&bits[qq >> 6], ~(1ull << (qq & 63u)));
        acc += __popcll(__ballot(pass));
    }
    wsync();
