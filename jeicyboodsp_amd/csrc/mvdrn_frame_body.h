// mvdrn_frame_body.h -- the beamformed frame of one block, the one text of it: a FRAGMENT of a kernel's body, included
// once in mvdrn_apply_pairs_kernel (mvdrn_kernels.hip), once in mvnb_apply_kernel (mvdrn_batch_kernels.hip) and once in
// mvnl_apply_kernel (mvdrn_live_kernels.hip), not a
// header; text and not a function for mvdrn_walk_body.h's reason (as a function the batch kernel's products conj(w) X
// and their sums came out with src0 and src1 exchanged, which shows where the weights are NaN).
//
// One wave, pair-owned bins (frame_io.h): lane l works on the bins m, m + 512 of m = l + 64 d, d < 5.  Y[k] =
// sum_m conj(w_k[m]) X_m[k] with w_k = conj(w_{1024-k}) above 512 is Hermitian when the X_m are, so the 513 bins the
// five items cover are all of it: ten weights and ten products per lane and microphone (sixteen with every bin a lane's
// own), and the inverse transform's mirrored inputs come from presplit_inv_pair.
//
// The includer has in scope:
//   int lane, n_mics; const float2 *table
//   const float2 *W     the block's row of the weight table, [microphone][bin]
//   src                 an object with  load(m, lane, prev, cur): the two blocks of microphone m's frame as 16-byte-per-
//                       lane images (asked for in the order m = 0, 1, ...), and  done(m, lane): microphone m is in the sum
// and gets  float2 y[8]: the frame, sample pair 2 lane + 128 d in y[d], unscaled (mvn_emit_block takes it from there).
    __shared__ __attribute__((aligned(16))) float2 lds[kWaveLdsComplex];
    __shared__ __attribute__((aligned(16))) unsigned int stage32[528];
    WaveTwiddles tw;
    load_wave_twiddles(tw, table, lane);
    PairTwiddles pw;
    load_pair_twiddles(pw, table, lane);
    const float nyq = lane == 0 ? -1.f : 1.f;                      // k = 512 (lane 0, d = 0) is its own mirror: conj(w) there

    float2 ylo[5], yhi[5];
#pragma unroll
    for (int d = 0; d < 5; d++) { ylo[d] = make_float2(0.f, 0.f); yhi[d] = make_float2(0.f, 0.f); }
    // a microphone's two blocks are requested while the one before it is transformed (the LDS fences would hold the loads back)
    u32x4 nxt_prev, nxt_cur;
    src.load(0, lane, nxt_prev, nxt_cur);
    for (int m = 0; m < n_mics; m++) {
        const float2 *Wm = W + (size_t)m * kMvnBins;
        float2 wl[5], wh[5];
#pragma unroll
        for (int d = 0; d < 5; d++) { wl[d] = Wm[lane + 64 * d]; wh[d] = Wm[512 - lane - 64 * d]; }
        const u32x4 img_prev = nxt_prev, img_cur = nxt_cur;
        if (m + 1 < n_mics) src.load(m + 1, lane, nxt_prev, nxt_cur);
        float2 v[8], zr[5];
        mvdr_frame_pairs(stage32, lane, img_prev, img_cur, v, 0.5f);
        wave_fft512<false>(v, lds, lane, tw);
        wave_lds_fence();
        pair_fetch_lds(v, lds, lane, zr);
#pragma unroll
        for (int d = 0; d < 5; d++) {
            const float2 e = cadd_conj(v[d], zr[d]), o = csub_conj_mj(v[d], zr[d]);
            const float2 t = cmul(pw.w[d], o);
            const float2 lo = cadd(e, t), hi = csub(e, t);         // X[m], X[m + 512]
            ylo[d].x += wl[d].x * lo.x + wl[d].y * lo.y;           // conj(w_m) X[m]
            ylo[d].y += wl[d].x * lo.y - wl[d].y * lo.x;
            const float why = d == 0 ? nyq * wh[d].y : wh[d].y;
            yhi[d].x += wh[d].x * hi.x - why * hi.y;               // w_{512-m} X[m + 512]
            yhi[d].y += wh[d].x * hi.y + why * hi.x;
        }
        src.done(m, lane);
    }
    // Y[512] = w_512^H X[512] is its own mirror, and real only when c_512 is: with a fractional delay it is not, and the
    // pre-split below would fold its imaginary part into the frame.  y is the real part of the IDFT (include/jdsp.h), to
    // which Im Y[512] adds nothing: it goes in as zero, like the 512-point path's bin 256.
    yhi[0].y = lane == 0 ? 0.f : yhi[0].y;
    float2 y[8], ret[4];
#pragma unroll
    for (int d = 0; d < 5; d++) {
        if (d < 4) presplit_inv_pair(ylo[d], yhi[d], pw.w[d], y[d], ret[d]);
        else y[d] = presplit_inv_reg(ylo[d], yhi[d], pw.w[d]);
    }
    pair_return_lds(ret, lds, lane, y);
    wave_fft512<true>(y, lds, lane, tw);
