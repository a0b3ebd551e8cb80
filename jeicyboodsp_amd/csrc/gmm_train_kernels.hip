// gmm_train_kernels.hip -- GMM training (GMMAlgorithm_Train_Auto_ver2.cpp) on device-resident MFCC vectors (gfx950).
//
//   gmm_train_kernel         main()'s per-class file loop (Train:87-146): KmeansAlogorithm (Train:342-438) on a
//                            class's first file, EmAlgorithmBasedGmmParameter (Train:255-340) on every file
//   gmm_train_params_kernel  PCADiagonalizeCovarianceMatrix (Train:456-518) of a copy of the state
//
// One workgroup per class, persistent over that class's files of the call: the files of a class are a strict serial
// chain (k-means, then 3 x (eigen -> E -> M) per file), so the parallelism is across classes and across the frames
// of a file.  The figure of merit is the latency of that chain, not HBM bandwidth.
//
// Determinism: every sum over frames is formed as fixed 64-frame tiles (frame index relative to the file start),
// each summed in ascending frame order by one thread, and the tile sums added in ascending tile order.  Nothing
// depends on the workgroup size or on which wave held a frame, so results are bit-identical across
// "threads_per_class" and across call cuts.  No FMA contraction anywhere in this file: products and sums round one
// by one, as the reference's do.
//
// Eigen-decomposition: the four 12x12 covariances of a class, one wave each, by parallel cyclic Jacobi (round-robin
// pairing: 6 disjoint rotations per step, 11 steps per sweep), ping-pong buffers in LDS, at most kJacobiSweeps
// sweeps.  Every device loop has a fixed upper bound: Jacobi sweeps, k-means passes (the "kmeans_max_passes" option),
// rounds of a file.
#include "jdsp_internal.h"

#pragma clang fp contract(off)

namespace jdsp {
namespace {

constexpr int kTile = 64;             // frames per tile of every reduction
constexpr int kRound = 256;           // frames staged in LDS at a time (4 tiles)
constexpr int kTilesPerRound = kRound / kTile;
constexpr int kQMax = 316;            // most quantities one reduction forms: 4 x 78 covariance entries + 4 counts
constexpr int kJacobiSweeps = 32;
constexpr double kPI = 3.141592;      // Train:21

struct Smem {
    double st[kTrDoubles];            // the class's state: alpa, mean, covariance, k-means cost
    int sti[kTrInts];
    // staged frames; while no frames are staged, the Jacobi ping-pong buffers A[2][4][144], V[2][4][144] live here
    double x[kRound * 12];
    double w[kRound * 4];             // per staged frame: weights (EM), selection bits (k-means) or the frame's cost
    double part[kTilesPerRound * kQMax];
    double acc[kQMax];
    double rc[4 * 12 * 2];            // per matrix and index j: (c, s_j) of this Jacobi step
    int pt[4 * 12];                   // ... and the partner index of j
    int any[kJacobiSweeps];           // rotations done in sweep s (any matrix)
    int bad[4];                       // matrix k had a non-finite entry
    double E[4 * 96];                 // [k][i][j]: the 8 kept eigenvectors, sorted, sign-canonical
    double lam[4 * 8];
    double pm[4 * 8];                 // projected means
    double coef[4 * 8];               // (1/sqrt(2 PI)) (1/sqrt(lam))
    int files[kRound];
    int wave_cnt[4];
    int n_files;
    int flags;
};

__device__ __forceinline__ long clampl(long long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : (long)v); }

// ---- eigen-decomposition ----------------------------------------------------------------------------------------
// Input: the four matrices in A[0][k] (row-major 12x12).  Output: E, lam of Smem (and the converged A / V left in
// the buffer `*cur`).  Wave k < 4 owns matrix k; every thread of the block takes part in the barriers.
__device__ void jacobi4(Smem &s, int *cur_out)
{
    double *A = s.x, *V = s.x + 2 * 576;              // [buf][k][144]
    const int tid = threadIdx.x, lane = tid & 63, k = tid >> 6;
    for (int e = tid; e < 4 * 144; e += blockDim.x) V[e] = ((e % 144) / 12 == (e % 12)) ? 1.0 : 0.0;
    if (tid < kJacobiSweeps) s.any[tid] = 0;
    if (tid < 4) s.bad[tid] = 0;
    __syncthreads();
    if (k < 4) {
        bool bad = false;
        for (int e = lane; e < 144; e += 64) bad |= !isfinite(A[k * 144 + e]);
        if (bad) s.bad[k] = 1;
    }
    int cur = 0;
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
        for (int step = 0; step < 11; step++) {
            if (k < 4 && lane < 6) {
                const int p = lane == 0 ? 11 : (step + lane) % 11, q = lane == 0 ? step : (step - lane + 11) % 11;
                const double *a = A + cur * 576 + k * 144;
                const double app = a[p * 12 + p], aqq = a[q * 12 + q], apq = a[p * 12 + q];
                double c = 1.0, sn = 0.0;
                if (fabs(apq) > 2.220446049250313e-16 * sqrt(fabs(app * aqq))) {
                    const double th = (aqq - app) / (2.0 * apq);
                    const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                    c = 1.0 / sqrt(t * t + 1.0);
                    sn = t * c;
                    s.any[sweep] = 1;
                }
                // a'_rp = c a_rp - s a_rq,  a'_rq = c a_rq + s a_rp
                s.rc[(k * 12 + p) * 2] = c; s.rc[(k * 12 + p) * 2 + 1] = -sn; s.pt[k * 12 + p] = q;
                s.rc[(k * 12 + q) * 2] = c; s.rc[(k * 12 + q) * 2 + 1] = sn;  s.pt[k * 12 + q] = p;
            }
            __syncthreads();
            if (k < 4) {
                const double *a = A + cur * 576 + k * 144, *v = V + cur * 576 + k * 144;
                double *an = A + (cur ^ 1) * 576 + k * 144, *vn = V + (cur ^ 1) * 576 + k * 144;
                for (int e = lane; e < 144; e += 64) {
                    const int i = e / 12, j = e % 12;
                    const int pi = s.pt[k * 12 + i], pj = s.pt[k * 12 + j];
                    const double ci = s.rc[(k * 12 + i) * 2], si = s.rc[(k * 12 + i) * 2 + 1];
                    const double cj = s.rc[(k * 12 + j) * 2], sj = s.rc[(k * 12 + j) * 2 + 1];
                    // J^T A J for the six disjoint rotations: columns, then rows
                    const double bij = cj * a[i * 12 + j] + sj * a[i * 12 + pj];
                    const double bpj = cj * a[pi * 12 + j] + sj * a[pi * 12 + pj];
                    // the rotated pair's own off-diagonal entry is zero by construction: stored as such, so that
                    // its rounding residue does not keep the sweeps going
                    an[e] = (j == pi && sj != 0.0) ? 0.0 : ci * bij + si * bpj;
                    vn[e] = cj * v[i * 12 + j] + sj * v[i * 12 + pj];
                }
            }
            cur ^= 1;
            __syncthreads();
        }
        if (!s.any[sweep]) break;                     // uniform: read after the barrier that ends the step
    }
    *cur_out = cur;
}

// Train:218-238: rank = number of strictly larger eigenvalues; slot j takes the first index of rank j, else keeps the
// previous pick.  Then the canonical sign: the largest-magnitude component of each kept column (first index on
// ties) is made positive.  One thread per matrix.
__device__ void select_eigen(Smem &s, int cur, int k)
{
    const double *a = s.x + cur * 576 + k * 144, *v = s.x + 2 * 576 + cur * 576 + k * 144;
    const bool bad = s.bad[k] != 0;
    int arg = 0;
    for (int j = 0; j < 8; j++) {
        for (int m = 0; m < 12; m++) {
            int rank = 0;
            for (int o = 0; o < 12; o++)
                if (a[m * 13] < a[o * 13]) rank++;
            if (rank == j) { arg = m; break; }
        }
        int big = 0;
        for (int i = 1; i < 12; i++)
            if (fabs(v[i * 12 + arg]) > fabs(v[big * 12 + arg])) big = i;
        const double sg = v[big * 12 + arg] < 0.0 ? -1.0 : 1.0;
        for (int i = 0; i < 12; i++) s.E[k * 96 + i * 8 + j] = bad ? NAN : sg * v[i * 12 + arg];
        s.lam[k * 8 + j] = bad ? NAN : a[arg * 13];
    }
}

// Eigenpairs of the four covariances of the state, then the x-independent parts of probability() (Train:240-249):
// projected means and the normalisation (1/sqrt(2 PI)) (1/sqrt(lam_i)).
__device__ void prepare_density(Smem &s)
{
    for (int e = threadIdx.x; e < 576; e += blockDim.x) s.x[e] = s.st[kTrCov + e];
    __syncthreads();
    int cur;
    jacobi4(s, &cur);
    if (threadIdx.x < 4) select_eigen(s, cur, threadIdx.x);
    __syncthreads();
    if (threadIdx.x < 32) {
        const int k = threadIdx.x >> 3, j = threadIdx.x & 7;
        double m = 0.0;
        for (int i = 0; i < 12; i++) m += s.st[kTrMean + 12 * k + i] * s.E[k * 96 + i * 8 + j];
        s.pm[k * 8 + j] = m;
        s.coef[k * 8 + j] = (1.0 / sqrt(2.0 * kPI)) * (1.0 / sqrt(s.lam[k * 8 + j]));
    }
    __syncthreads();
}

// ---- reductions over the frames of a file -------------------------------------------------------------------------
enum { kStageAssign = 0, kStageSel = 1, kStageEstep = 2, kStageWbuf = 3 };
enum { kSumCost = 0, kSumWx = 1, kSumCov = 2 };

__device__ __forceinline__ int n_quantities(int sum) { return sum == kSumCost ? 1 : (sum == kSumWx ? 52 : kQMax); }

// covariance quantity q < 312 -> mixture k and the pair a <= b
__device__ __forceinline__ void cov_index(int q, int &k, int &a, int &b)
{
    k = q / 78;
    int r = q % 78;
    a = 0;
    while (r >= 12 - a) { r -= 12 - a; a++; }
    b = a + r;
}

__device__ __forceinline__ double dist2(const double *x, const double *m)   // DistanceToCenter, Train:440-447
{
    double d = 0.0;
    for (int i = 0; i < 12; i++) {
        const double t = x[i] - m[i];
        d += t * t;
    }
    return d;
}

// Stages the file's frames round by round and sums the quantities of `sum` over them into s.acc[0..Q).
//   kStageAssign  k-means step 2) + 3) (Train:357-376): arg-min with `>=` from j = 0 (last index wins ties),
//                 Selection |= bit, and the frame's cost sum_j sel_j dist_j
//   kStageSel     w = the selection bits (0 / 1)
//   kStageEstep   E-step (Train:270-284): w_k = probability_k(x) alpa_k / sum; stored to wbuf for kStageWbuf
//   kStageWbuf    w = what kStageEstep stored (the same thread staged that frame)
__device__ void reduce_file(Smem &s, int stage, int sum, const double *__restrict__ feats, long first, long n,
                            unsigned char *__restrict__ sel, double *__restrict__ wbuf)
{
    const int tid = threadIdx.x, Q = n_quantities(sum);
    for (int q = tid; q < Q; q += blockDim.x) s.acc[q] = 0.0;
    for (long r0 = 0; r0 < n; r0 += kRound) {
        const int cnt = (int)(n - r0 < kRound ? n - r0 : kRound);
        if (tid < cnt) {
            const long f = first + r0 + tid;
            double x[12];
            const double2 *p = reinterpret_cast<const double2 *>(feats + 12 * f);
            for (int i = 0; i < 6; i++) {
                const double2 v = p[i];
                x[2 * i] = v.x;
                x[2 * i + 1] = v.y;
            }
            for (int i = 0; i < 12; i++) s.x[tid * 12 + i] = x[i];
            double w[4];
            if (stage == kStageAssign) {
                double d[4];
                for (int j = 0; j < 4; j++) d[j] = dist2(x, s.st + kTrMean + 12 * j);
                double best = d[0];
                int arg = 0;
                for (int j = 0; j < 4; j++)
                    if (best >= d[j]) { arg = j; best = d[j]; }
                const unsigned bits = sel[f] | (1u << arg);
                sel[f] = (unsigned char)bits;
                double c = 0.0;
                for (int j = 0; j < 4; j++)
                    if (bits & (1u << j)) c += d[j];
                w[0] = c; w[1] = w[2] = w[3] = 0.0;
            } else if (stage == kStageSel) {
                const unsigned bits = sel[f];
                for (int j = 0; j < 4; j++) w[j] = (bits >> j) & 1u ? 1.0 : 0.0;
            } else if (stage == kStageEstep) {
                double t = 0.0;
#pragma unroll 1
                for (int k = 0; k < 4; k++) {
                    double pr = 1.0;
#pragma unroll 1
                    for (int j = 0; j < 8; j++) {                                   // Train:245-250
                        double y = 0.0;
                        for (int i = 0; i < 12; i++) y += x[i] * s.E[k * 96 + i * 8 + j];
                        const double dd = y - s.pm[k * 8 + j];
                        pr *= s.coef[k * 8 + j] * exp(((-1 / 2.0) * (dd * dd)) / s.lam[k * 8 + j]);
                    }
                    w[k] = pr * s.st[kTrAlpa + k];
                    t += w[k];
                }
                for (int k = 0; k < 4; k++) {
                    w[k] = w[k] / t;
                    wbuf[4 * f + k] = w[k];
                }
            } else {
                for (int k = 0; k < 4; k++) w[k] = wbuf[4 * f + k];
            }
            for (int k = 0; k < 4; k++) s.w[tid * 4 + k] = w[k];
        }
        __syncthreads();
        const int nt = (cnt + kTile - 1) / kTile;
        for (int it = tid; it < Q * nt; it += blockDim.x) {
            const int q = it % Q, t = it / Q;
            const int i0 = t * kTile, i1 = min(i0 + kTile, cnt);
            double a = 0.0;
            if (sum == kSumCost) {
                for (int i = i0; i < i1; i++) a += s.w[i * 4];
            } else if (sum == kSumWx) {
                if (q < 48) {
                    const int k = q / 12, d = q % 12;
                    for (int i = i0; i < i1; i++) a += s.w[i * 4 + k] * s.x[i * 12 + d];      // Train:300
                } else {
                    for (int i = i0; i < i1; i++) a += s.w[i * 4 + q - 48];                  // Train:291
                }
            } else {
                if (q < 312) {
                    int k, ia, ib;
                    cov_index(q, k, ia, ib);
                    const double ma = s.st[kTrMean + 12 * k + ia], mb = s.st[kTrMean + 12 * k + ib];
                    for (int i = i0; i < i1; i++)                                            // Train:313, :396
                        a += ((s.x[i * 12 + ia] - ma) * (s.x[i * 12 + ib] - mb)) * s.w[i * 4 + k];
                } else {
                    for (int i = i0; i < i1; i++) a += s.w[i * 4 + q - 312];
                }
            }
            s.part[t * kQMax + q] = a;
        }
        __syncthreads();
        for (int q = tid; q < Q; q += blockDim.x)
            for (int t = 0; t < nt; t++) s.acc[q] += s.part[t * kQMax + q];
        __syncthreads();
    }
}

// covariance[k] = acc / div[k], both triangles (Train:315-322, :399-407)
__device__ void store_cov(Smem &s, const double *div)
{
    for (int q = threadIdx.x; q < 312; q += blockDim.x) {
        int k, a, b;
        cov_index(q, k, a, b);
        const double v = s.acc[q] / div[k];
        s.st[kTrCov + 144 * k + 12 * a + b] = v;
        s.st[kTrCov + 144 * k + 12 * b + a] = v;
    }
}

// KmeansAlogorithm (Train:342-438) on the class's first file, means already initialised (Train:120-124).
__device__ void kmeans(Smem &s, const double *feats, long first, long n, unsigned char *sel, int max_passes)
{
    if (threadIdx.x < kRound)                          // the thread that stages frame i in reduce_file clears it
        for (long i = threadIdx.x; i < n; i += kRound) sel[first + i] = 0;
    __syncthreads();
    double cost_before = 0.0, cost = 0.0;
    int count = 0;
    bool capped = false;
    double cnt[4];
    while (true) {
        count++;
        reduce_file(s, kStageAssign, kSumCost, feats, first, n, sel, nullptr);
        cost = s.acc[0];
        __syncthreads();
        const bool go_on = count == 1 || fabs(cost - cost_before) >= 1.0;                  // Train:379
        if (go_on && count < max_passes) {
            cost_before = cost;
            reduce_file(s, kStageSel, kSumWx, feats, first, n, sel, nullptr);             // Train:414-434
            for (int q = threadIdx.x; q < 48; q += blockDim.x) {
                const double c = s.acc[48 + q / 12];
                s.st[kTrMean + q] = c == 0.0 ? 0.0 : s.acc[q] / c;
            }
            __syncthreads();
            continue;
        }
        capped = go_on;
        reduce_file(s, kStageSel, kSumCov, feats, first, n, sel, nullptr);                // Train:385-410
        for (int k = 0; k < 4; k++) cnt[k] = s.acc[312 + k];
        store_cov(s, cnt);
        break;
    }
    if (threadIdx.x == 0) {
        s.sti[kTrPasses] = count;
        s.sti[kTrCapped] = capped ? 1 : 0;
        for (int k = 0; k < 4; k++) s.sti[kTrSelected + k] = (int)cnt[k];
        s.st[kTrCost] = cost;
    }
    if (threadIdx.x < 4) s.st[kTrAlpa + threadIdx.x] = 1.0 / 4;                              // Train:129-131
    __syncthreads();
}

// EmAlgorithmBasedGmmParameter (Train:255-340): three iterations; the log-likelihood pass (:326-332) only prints and
// is not computed.
__device__ void em(Smem &s, const double *feats, long first, long n, double *wbuf)
{
    for (int iter = 0; iter < 3; iter++) {
        prepare_density(s);
        reduce_file(s, kStageEstep, kSumWx, feats, first, n, nullptr, wbuf);
        double nkey[4];
        for (int k = 0; k < 4; k++) nkey[k] = s.st[kTrAlpa + k] + s.acc[48 + k];                // Train:291-293
        __syncthreads();
        for (int q = threadIdx.x; q < 48; q += blockDim.x) {                                   // Train:297-304
            const int k = q / 12;
            s.st[kTrMean + q] = (s.st[kTrMean + q] + s.acc[q]) / nkey[k];
        }
        if (threadIdx.x < 4) s.st[kTrAlpa + threadIdx.x] = nkey[threadIdx.x] / (double)n;        // Train:294
        __syncthreads();
        reduce_file(s, kStageWbuf, kSumCov, feats, first, n, nullptr, wbuf);
        store_cov(s, nkey);
        __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void gmm_train_kernel(const double *__restrict__ feats, long n_frames,
                                                         const long long *__restrict__ file_first,
                                                         const int *__restrict__ file_class, long n_files,
                                                         int n_classes, int max_passes, GmmTrainState *__restrict__ state,
                                                         unsigned char *__restrict__ sel, double *__restrict__ wbuf)
{
    __shared__ Smem s;
    const int c = blockIdx.x, tid = threadIdx.x;
    GmmTrainState *g = state + c;
    for (int e = tid; e < kTrDoubles; e += blockDim.x) s.st[e] = g->d[e];
    if (tid < kTrInts) s.sti[tid] = g->i[tid];
    if (tid == 0) s.flags = 0;
    __syncthreads();
    for (long base = 0; base < n_files; base += kRound) {
        // this class's files among [base, base + 256), in ascending order (ballot compaction over the first 4 waves)
        bool match = false;
        if (tid < kRound && base + tid < n_files) {
            const int fc = file_class[base + tid];
            match = fc == c;
            if (c == 0 && (fc < 0 || fc >= n_classes)) atomicOr(&s.flags, (int)JDSP_GMM_TRAIN_BAD_CLASS);
            // decreasing offsets can make two files (of two classes) share vectors, and with them the per-vector
            // workspace: flagged, the overlapping classes' results are then unspecified (nothing is read outside feats)
            if (c == 0 && file_first[base + tid + 1] < file_first[base + tid])
                atomicOr(&s.flags, (int)JDSP_GMM_TRAIN_UNORDERED);
        }
        const unsigned long long m = __ballot(match);
        const int lane = tid & 63, wv = tid >> 6;
        if (tid < kRound && lane == 0) s.wave_cnt[wv] = __popcll(m);
        __syncthreads();
        if (tid < kRound && match) {
            int pos = __popcll(m & ((1ull << lane) - 1ull));
            for (int v = 0; v < wv; v++) pos += s.wave_cnt[v];
            s.files[pos] = (int)(base + tid);
        }
        if (tid == 0) s.n_files = s.wave_cnt[0] + s.wave_cnt[1] + s.wave_cnt[2] + s.wave_cnt[3];
        __syncthreads();
        const int nf = s.n_files;
        for (int fi = 0; fi < nf; fi++) {
            const long f = s.files[fi];
            // offsets outside [0, n_frames] are the caller's error; clamped so that nothing outside feats is read
            const long lo = clampl(file_first[f], 0, n_frames), hi = clampl(file_first[f + 1], lo, n_frames);
            const bool clamped = file_first[f] != lo || file_first[f + 1] != hi;
            const long n = hi - lo;
            const bool seen = s.sti[kTrSeen] != 0;
            __syncthreads();
            if (tid == 0 && clamped) atomicOr(&s.flags, (int)JDSP_GMM_TRAIN_CLAMPED);
            if (n == 0) {
                if (tid == 0) atomicOr(&s.flags, (int)JDSP_GMM_TRAIN_EMPTY_FILE);
                continue;
            }
            if (!seen && n < 13) {
                if (tid == 0) atomicOr(&s.flags, (int)JDSP_GMM_TRAIN_SHORT_FIRST);
                continue;
            }
            if (!seen) {
                for (int q = tid; q < 48; q += blockDim.x)                                    // Train:120-124
                    s.st[kTrMean + q] = feats[12 * (lo + 4 * (q / 12)) + q % 12];
                kmeans(s, feats, lo, n, sel, max_passes);
            }
            em(s, feats, lo, n, wbuf);
            if (tid == 0) {
                s.sti[kTrSeen] = 1;
                s.sti[kTrFiles]++;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid == 0) s.sti[kTrStatus] |= s.flags;
    __syncthreads();
    for (int e = tid; e < kTrDoubles; e += blockDim.x) g->d[e] = s.st[e];
    if (tid < kTrInts) g->i[tid] = s.sti[tid];
}

// PCADiagonalizeCovarianceMatrix (Train:456-518) of each class's state; one 256-thread workgroup per class.
__global__ __launch_bounds__(256) void gmm_train_params_kernel(const GmmTrainState *__restrict__ state,
                                                               jdsp_gmm_train_param *__restrict__ out)
{
    __shared__ Smem s;
    const int c = blockIdx.x, tid = threadIdx.x;
    for (int e = tid; e < kTrDoubles; e += blockDim.x) s.st[e] = state[c].d[e];
    __syncthreads();
    prepare_density(s);
    double *o = reinterpret_cast<double *>(out + c);
    // record layout (doubles): alpa 0..3, mean 4..51, covariance 52..627, eigenVector 628..1011
    for (int e = tid; e < 1012; e += blockDim.x) {
        double v;
        if (e < 4) {
            v = s.st[kTrAlpa + e];
        } else if (e < 52) {
            const int k = (e - 4) / 12, i = (e - 4) % 12;
            v = i < 8 ? s.pm[k * 8 + i] : 0.0;                                               // Train:508-511
        } else if (e < 628) {
            const int k = (e - 52) / 144, r = (e - 52) % 144, i = r / 12, j = r % 12;
            v = i < 8 ? (i == j ? s.lam[k * 8 + i] : 0.0) : s.st[kTrCov + 144 * k + r];      // Train:512-513
        } else {
            v = s.E[e - 628];                                                                 // Train:514-516
        }
        o[e] = v;
    }
}

}  // namespace

int launch_gmm_train(hipStream_t st, int threads, int n_classes, const double *feats, long n_frames,
                     const long long *file_first, const int *file_class, long n_files, int kmeans_max_passes,
                     GmmTrainState *state, unsigned char *sel, double *wbuf)
{
    hipLaunchKernelGGL(gmm_train_kernel, dim3(n_classes), dim3(threads), 0, st, feats, n_frames, file_first, file_class,
                       n_files, n_classes, kmeans_max_passes, state, sel, wbuf);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_gmm_train_params(hipStream_t st, int n_classes, const GmmTrainState *state, jdsp_gmm_train_param *out)
{
    hipLaunchKernelGGL(gmm_train_params_kernel, dim3(n_classes), dim3(256), 0, st, state, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace jdsp
