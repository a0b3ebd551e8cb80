// mvdrn_walk_body.h -- the covariance walk and its solve, the one text of it: a FRAGMENT of a kernel's body, included
// once in mvdrn_update_kernel (mvdrn_kernels.hip), once in mvnb_update_kernel (mvdrn_batch_kernels.hip) and once in
// mvnl_update_kernel (mvdrn_live_kernels.hip), not a header.
//
// Why not a function.  As `__device__ __forceinline__ mvn_update_walk(...)` both kernels kept their resources and every
// opcode count, and every finite output bit; but the compiler simplifies a function on its own before it inlines it, the
// kernel then sees the elimination already unrolled, and its reassociate pass orders the operands of the commutative
// products f * row[c] by another rank than over the rolled loops (96 v_mul_f64 / v_fma_f64 per kernel with src0 and src1
// exchanged).  Where both operands are NaN -- the zero matrix of a fresh stream, a singular lead at loading 0 -- the
// NaN that comes out follows the operand's position, and six digests of tools/ab_bits.py moved.  With the bound handed
// over so that the function stays rolled until it is inlined, the kernels had 144 bytes of scratch.  Included as text
// the kernels compile as they did (profiles/r25_mvdrn_one_walk.txt).
//
// The includer has in scope:
//   cd R[8]             this lane's row of the matrix entering the walk (changed: the row after event e1 - 1)
//   int grp, r          lane >> 3, lane & 7: the bin in the wave and the row
//   int kb, k           this group's bin and min(kb, n_bins - 1): a group past the last bin repeats it and stores nothing
//   int e0, e1          the walk's events [e0, e1)
//   bool lead           solve R as it came in too (version e0)
//   n_mics, n_bins, inv_n, spec, steer, loading, weights    as the kernels' arguments of those names
// Versions v = (lead ? e0 : e0 + 1) .. e1.  Version v adds event v - 1 when v > e0, then Gaussian elimination of
// [R' | c] to a diagonal (R' = R + loading * tr(R) / n * I, Hermitian positive definite once loaded, so no pivoting; pivot
// rows are left unnormalised and each unknown is divided by its pivot at the end), then w = x / (c^H x), stored as row v.
// Step p: the lane holding row p puts its entries right of the diagonal and its right-hand side in LDS, the group's
// other rows subtract their multiple of it.
    __shared__ __attribute__((aligned(16))) float2 sx[8][8];       // the event's spectra, [bin in wave][microphone]
    __shared__ __attribute__((aligned(16))) double2 srow[8][9];    // the pivot row and its right-hand side
    __shared__ __attribute__((aligned(16))) double2 sc[8][8];      // steering vectors
    __shared__ __attribute__((aligned(16))) double2 sv[8][8];      // diagonals, then the unknowns
    const bool row_live = r < n_mics;
    const double2 sr = steer[(size_t)k * 8 + r];
    const cd cr = {row_live ? sr.x : 0.0, row_live ? sr.y : 0.0};
    sc[grp][r] = d2_of(cr);
    float2 xr = make_float2(0.f, 0.f);
    if (row_live && e0 < e1) xr = spec[((size_t)e0 * n_mics + r) * n_bins + k];     // event e0 is the first the walk adds
    for (int v = lead ? e0 : e0 + 1; v <= e1; v++) {
        if (v > e0) mvn_row_add(R, xr, sx[grp], r, inv_n);
        if (row_live && v < e1) xr = spec[((size_t)v * n_mics + r) * n_bins + k];   // event v is the one version v + 1 adds
        double dgx = R[0].x;                                   // the diagonal entry (real) of this lane's row
#pragma unroll
        for (int c = 1; c < 8; c++) dgx = r == c ? R[c].x : dgx;
        wave_lds_fence();
        sv[grp][r] = make_double2(dgx, 0.0);
        wave_lds_fence();
        double tr = 0.0;
        for (int d = 0; d < n_mics; d++) tr += sv[grp][d].x;
        const double load = loading * tr / n_mics;
        cd A[8];
#pragma unroll
        for (int c = 0; c < 8; c++) {
            A[c].x = r == c ? (row_live ? R[c].x + load : 1.0) : R[c].x;
            A[c].y = r == c && !row_live ? 0.0 : R[c].y;
        }
        cd b = cr, my_inv = {1.0, 0.0};
#pragma unroll
        for (int p = 0; p < 8; p++) {
            if (p < n_mics) {
                wave_lds_fence();
                if (r == p) {
#pragma unroll
                    for (int c = p; c < 8; c++) srow[grp][c] = d2_of(A[c]);
                    srow[grp][8] = d2_of(b);
                }
                wave_lds_fence();
                const cd inv = cd_inv_fast(cd_of(srow[grp][p]));
                cd f = cd_mul(A[p], inv);                       // this row's multiple of the pivot row
                my_inv.x = r == p ? inv.x : my_inv.x;
                my_inv.y = r == p ? inv.y : my_inv.y;
                f.x = r == p ? 0.0 : f.x;
                f.y = r == p ? 0.0 : f.y;
#pragma unroll
                for (int c = p + 1; c < 8; c++) A[c] = cd_sub(A[c], cd_mul(f, cd_of(srow[grp][c])));
                b = cd_sub(b, cd_mul(f, cd_of(srow[grp][8])));
            }
        }
        const cd x = cd_mul(b, my_inv);
        wave_lds_fence();
        sv[grp][r] = d2_of(x);
        wave_lds_fence();
        cd den = {0.0, 0.0};                                   // c^H x
        for (int d = 0; d < n_mics; d++) {
            const cd xd = cd_of(sv[grp][d]);
            const cd cdv = cd_of(sc[grp][d]);
            den.x += cdv.x * xd.x + cdv.y * xd.y;
            den.y += cdv.x * xd.y - cdv.y * xd.x;
        }
        const cd w = cd_mul(x, cd_inv_fast(den));
        // [version][microphone][bin]: the apply kernel reads one microphone's weights for consecutive bins
        if (row_live && kb < n_bins) weights[((size_t)v * 8 + r) * n_bins + k] = make_float2((float)w.x, (float)w.y);
    }
