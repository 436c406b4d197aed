// EKF pose augmentation and covariance housekeeping for a batch of independent filters (the family map is in ekf.hip): augment, undo,
// symmetrise, normalise, transform and map-point kernels, with the hv_ekf_* entries that launch them.
//   * pose augmentation: the Joseph form (I-KH) P (I-KH)' + K R K' is expanded around the 7-row
//     +-1 matrix visAugH into a rank-14 correction (4 MFMA k-steps per 16 x 16 tile) of the shifted
//     matrix A P A' + Q, which is a gather of P and never materialised; mirrored tile pairs meet
//     through an in-wave LDS transpose for the fused (P+P')/2, and the result goes to the second of
//     two ping-pong buffers: one read and one write of P per augmentation. The 14 rows and columns
//     visAugH touches are then rewritten from the Joseph form itself (W = T P1 times the rows of T,
//     formed first): the expansion cancels the slot's 1e8 prior against itself there and loses seven
//     to eight digits of entries of size 1e-6, which a whole-matrix norm never sees.
#include <utility>

#include "ekf_device.hpp"
#include "ekf_host.hpp"

// The library is built with -ffp-contract=off for the tracker's bit-exact binary32 sequence; the
// EKF is judged against a relative tolerance, and a fused multiply-add is one rounding fewer and
// half the f64 instructions of its dependency chains.
#pragma clang fp contract(fast)

namespace hv {

namespace {

// ---------------------------------------------------------------------------------------------
// pose augmentation / undo (ekf.cpp:848-903) and housekeeping
// ---------------------------------------------------------------------------------------------
struct AugmentArgs {
    int n, cam_poses, map_dim;
    double *m, *P, *P1, *m1;          // P1/m1: per-filter scratch (n*n, n)
    const int *dropped;               // per filter (or null -> dropped0), -1 = last
    int dropped0;
    double q_pos, q_ori, rd;          // visAugQ diagonal (scaled), augmentR * noiseScale
    const unsigned char *active;
};

__device__ __forceinline__ int aug_src(int i, int dropped, int n)   // visAugA[dropped] as a gather (ekf.cpp:230-248)
{
    if (i < CAM) return i;
    if (i < CAM + POSE) return -1;                                    // slot 0 is re-created by the update
    if (i < CAM + (dropped + 1) * POSE) return i - POSE;
    return i;
}
__device__ __forceinline__ int augh_plus(int i) { return i < 3 ? POS + i : ORI + (i - 3); }   // visAugH (ekf.cpp:267-278)
__device__ __forceinline__ int augh_minus(int i) { return CAM + i; }
// the 14 state indices visAugH touches (POS, ORI, trail slot 0) in the order [plus(0..6); minus(0..6)], and the inverse (-1: none)
constexpr int AUGJ = 2 * POSE;
__device__ __forceinline__ int augj_index(int jj) { return jj < POSE ? augh_plus(jj) : augh_minus(jj - POSE); }
__device__ __forceinline__ int augj_slot(int i)
{
    if (i < POS + 3) return i - POS;
    if (i >= ORI && i < ORI + 4) return 3 + (i - ORI);
    if (i >= CAM && i < CAM + POSE) return POSE + (i - CAM);
    return -1;
}

constexpr int AUG_THREADS = 1024;

// In-wave transpose of a 16 x 16 f64 tile held in the MFMA C layout (lane (rq, c) holds rows rq + 4 q of
// column c) through a 16 x 17 LDS scratch private to the wavefront: DS operations of one wave execute
// in order, so no barrier is involved.
__device__ __forceinline__ void tile_transpose(double (&v)[4], double *scr, int rq, int c)
{
#pragma unroll
    for (int q = 0; q < 4; q++) scr[(rq + 4 * q) * 17 + c] = v[q];
#pragma unroll
    for (int q = 0; q < 4; q++) v[q] = scr[c * 17 + rq + 4 * q];
}

// triangular pair index p -> (I <= J)
__device__ __forceinline__ void tri_decode(int p, int &I, int &J)
{
    J = 0;
    while (p > J) { p -= J + 1; J++; }
    I = p;
}

// The kernel reads the covariance from P and writes the result to P1 (the host swaps the two
// afterwards): the shifted matrix A P A' + Q is a gather of P and is never materialised, so the
// covariance crosses HBM once in each direction instead of three + one times.
// SYM (hv_ekf_symmetrize_augment_dev, r04): the covariance is read as (P + P') / 2 -- maintainPositiveSemiDefinite (ekf.cpp:1059-1067),
// which the backend calls at the end of the visual updates (backend.cpp:1267), folded into the augmentation that follows it: the
// mirrored element of every gathered value belongs to the tile pair the same wavefront reads anyway (L2 hits), and a separate
// symmetrise launch is one more read and write of every covariance. Same values as the two calls in sequence, bit for bit.
template <bool SYM>
__global__ __launch_bounds__(AUG_THREADS) void ekf_augment_kernel(AugmentArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = blockIdx.x, t = threadIdx.x, n = a.n;
    double *m = a.m + (size_t)b * n;
    const double *P = a.P + (size_t)b * n * n;
    double *Pout = a.P1 + (size_t)b * n * n, *m1 = a.m1 + (size_t)b * n;
    if (a.active && !a.active[b]) {                                  // untouched filter: carry P over to the new buffer
        for (int e = t; e < n * n; e += AUG_THREADS) {
            if (SYM) { const int i = e % n, j = e / n; Pout[e] = 0.5 * (P[e] + P[(size_t)i * n + j]); }
            else Pout[e] = P[e];
        }
        return;
    }
    int dropped = a.dropped ? a.dropped[b] : a.dropped0;
    if (dropped < 0) dropped = a.cam_poses - 1;
    // [HP | K | G]: 7 x n each, row-major [k * n + j] and contiguous: rows 0..13 are the MFMA A operand
    // (HP; K), rows 7..20 the B operand (K; G) of step 4
    static_assert(AUG_POSE == POSE && AUG_J == AUGJ, "AugmentLds is written for the pose block of this state layout");
    const AugmentLds L = augment_lds(n, AUG_THREADS / 64);
    double *HP = smem + L.HP, *K = smem + L.K, *G = smem + L.G;
    double *S0 = smem + L.S0, *Lc = smem + L.Lc, *vres = smem + L.vres;
    double *scr_all = smem + L.scratch;                               // 16 waves x 16 x 17 transpose scratch

    // P1 = A P A' + Q as a function (ekf.cpp:230-248, 848-871)
    auto p1 = [&](int i, int j) -> double {
        const int si = aug_src(i, dropped, n), sj = aug_src(j, dropped, n);
        double v = 0.0;
        if (si >= 0 && sj >= 0) {
            v = P[(size_t)sj * n + si];
            if (SYM) v = 0.5 * (v + P[(size_t)si * n + sj]);
        }
        if (i == j && i >= CAM && i < CAM + POSE) v += (i < CAM + 3) ? a.q_pos : a.q_ori;
        return v;
    };

    // 1. m1 = A m
    for (int i = t; i < n; i += AUG_THREADS) { const int s = aug_src(i, dropped, n); m1[i] = s >= 0 ? m[s] : 0.0; }
    // 2. HP = H P1 (7 x n), S0 = HP H'
    for (int e = t; e < POSE * n; e += AUG_THREADS) {
        const int k = e / n, j = e % n;
        HP[e] = p1(augh_plus(k), j) - p1(augh_minus(k), j);
    }
    __syncthreads();
    if (t < POSE * POSE) { const int i = t / POSE, c = t % POSE; S0[t] = HP[i * n + augh_plus(c)] - HP[i * n + augh_minus(c)]; }
    if (t >= 64 && t < 64 + POSE) { const int i = t - 64; vres[i] = -(m1[augh_plus(i)] - m1[augh_minus(i)]); }
    __syncthreads();
    if (t == 0) {                                                   // Cholesky of S = S0 + rd I (7 x 7)
        for (int i = 0; i < POSE; i++) for (int c = 0; c < POSE; c++) Lc[i * POSE + c] = 0.0;
        for (int c = 0; c < POSE; c++) {
            double d = S0[c * POSE + c] + a.rd;
            for (int p = 0; p < c; p++) d -= Lc[c * POSE + p] * Lc[c * POSE + p];
            d = sqrt(d);
            Lc[c * POSE + c] = d;
            for (int i = c + 1; i < POSE; i++) {
                double s = 0.5 * (S0[i * POSE + c] + S0[c * POSE + i]);
                for (int p = 0; p < c; p++) s -= Lc[i * POSE + p] * Lc[c * POSE + p];
                Lc[i * POSE + c] = s / d;
            }
        }
    }
    __syncthreads();
    // K(j, :) = S^-1 HP(:, j)   (K = (S^-1 HP)')
    for (int j = t; j < n; j += AUG_THREADS) {
        double x[POSE];
        for (int i = 0; i < POSE; i++) { double s = HP[i * n + j]; for (int p = 0; p < i; p++) s -= Lc[i * POSE + p] * x[p]; x[i] = s / Lc[i * POSE + i]; }
        for (int i = POSE - 1; i >= 0; i--) { double s = x[i]; for (int p = i + 1; p < POSE; p++) s -= Lc[p * POSE + i] * x[p]; x[i] = s / Lc[i * POSE + i]; }
        double dm = 0;
        for (int i = 0; i < POSE; i++) { K[i * n + j] = x[i]; dm += x[i] * vres[i]; }
        m[j] = m1[j] + dm;                                          // m = A m + K (-H A m)
    }
    __syncthreads();
    // 3. G = P1 H' - K S0 - rd K   (n x 7): then P = P1 - K HP - G K' reproduces the Joseph form
    for (int e = t; e < POSE * n; e += AUG_THREADS) {
        const int c = e / n, i = e % n;
        double g = p1(i, augh_plus(c)) - p1(i, augh_minus(c));
        for (int k = 0; k < POSE; k++) g -= K[k * n + i] * S0[k * POSE + c];
        G[e] = g - a.rd * K[c * n + i];
    }
    __syncthreads();
    // 4. Pout = sym(P1 - K HP - G K')   (maintainPositiveSemiDefinite fused, ekf.cpp:872). A wavefront
    // owns a pair of mirrored 16 x 16 tiles; the rank-14 correction of a tile is 4 f64 MFMA steps,
    //   X(j, i) = P1(i, j) - sum_kk Aop(kk, j) Bop(kk, i),   Aop = [HP; K],  Bop = [K; G],
    // accumulated onto the gathered tile, and the two tiles meet through an in-wave LDS transpose, so
    // every global access is a 128-byte row segment.
    {
        const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63, rq = lane >> 4, c = lane & 15;
        double *scr = scr_all + wave * (16 * 17);
        const int tb = (n + 15) >> 4, npairs = tb * (tb + 1) / 2;
        auto corrected_tile = [&](int i0, int j0, double (&x)[4]) {          // x[q] = X(j0 + rq + 4 q, i0 + c)
            double4v acc;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int i = i0 + c, j = j0 + rq + 4 * q;
                acc[q] = (i < n && j < n) ? p1(i, j) : 0.0;
            }
#pragma unroll
            for (int sx = 0; sx < 4; sx++) {
                const int kk = 4 * sx + rq;
                const double av = HP[(size_t)min(kk, 13) * n + min(j0 + c, n - 1)];          // Aop(kk, j0 + c)
                const double bv = K[(size_t)min(kk, 13) * n + min(i0 + c, n - 1)];           // Bop(kk, i0 + c)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(kk < 14 ? -av : 0.0, kk < 14 ? bv : 0.0, acc, 0, 0, 0);
            }
#pragma unroll
            for (int q = 0; q < 4; q++) x[q] = acc[q];
        };
        for (int p = wave; p < npairs; p += AUG_THREADS / 64) {
            int I, J;
            tri_decode(p, I, J);
            const int i0 = 16 * I, j0 = 16 * J;
            double x[4], y[4];
            corrected_tile(i0, j0, x);                                        // element (i0 + c, j0 + r)
            if (I != J) corrected_tile(j0, i0, y);                            // element (j0 + c, i0 + r)
            else {
#pragma unroll
                for (int q = 0; q < 4; q++) y[q] = x[q];
            }
            tile_transpose(y, scr, rq, c);                                    // now the mirror of x[q]
#pragma unroll
            for (int q = 0; q < 4; q++) {
                x[q] = 0.5 * (x[q] + y[q]);
                const int i = i0 + c, j = j0 + rq + 4 * q;
                if (i < n && j < n) Pout[(size_t)j * n + i] = x[q];
            }
            if (I != J) {
                tile_transpose(x, scr, rq, c);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int i = j0 + c, j = i0 + rq + 4 * q;
                    if (i < n && j < n) Pout[(size_t)j * n + i] = x[q];
                }
            }
        }
    }
    __syncthreads();
    // 5. The 14 columns visAugH touches (POS, ORI, trail slot 0) and, by symmetry, the same 14 rows, in the Joseph form itself.
    // There step 4's expansion subtracts numbers the size of the slot's prior (1e8) to leave a variance of 1e-6: exact algebra,
    // seven to eight digits lost in every entry of those rows on its own scale (profiles/ekf_accuracy). With W = P1 - K HP = T P1 and
    // the rows of T = I - K H formed FIRST on their support (those same 14 columns), 1 + K(cam, .) is a small number with a small
    // absolute error, and P(:, j) = W T(j, :)' + rd K K(j, :)' carries W's cancellation error times that small number only.
    // Wc (n x 14) and T14 borrow the transpose scratch, which step 4 is done with.
    {
        double *Wc = scr_all, *T14 = smem + L.T14;
        for (int e = t; e < AUGJ * n; e += AUG_THREADS) {
            const int cc = e / n, i = e % n, jc = augj_index(cc);
            double w = p1(i, jc);
            for (int k = 0; k < POSE; k++) w -= K[k * n + i] * HP[k * n + jc];
            Wc[e] = w;
        }
        if (t < AUGJ * AUGJ) {
            const int jj = t / AUGJ, cc = t % AUGJ;
            const double kv = K[(cc < POSE ? cc : cc - POSE) * n + augj_index(jj)];      // H(k, J[cc]) = +1 (k = cc) / -1 (k = cc - 7)
            T14[t] = (jj == cc ? 1.0 : 0.0) + (cc < POSE ? -kv : kv);
        }
        __syncthreads();
        auto column = [&](int i, int jj) -> double {                     // (W T' + rd K K')(i, J[jj])
            const int j = augj_index(jj);
            double s = 0.0, kk = 0.0;
            for (int cc = 0; cc < AUGJ; cc++) s += Wc[cc * n + i] * T14[jj * AUGJ + cc];
            for (int k = 0; k < POSE; k++) kk += K[k * n + i] * K[k * n + j];
            return s + a.rd * kk;
        };
        for (int e = t; e < AUGJ * n; e += AUG_THREADS) {
            const int jj = e / n, i = e % n, j = augj_index(jj), ii = augj_slot(i);
            if (ii > jj) continue;                                       // inside the 14 x 14 block one thread writes both mirrors
            double v = column(i, jj);
            if (ii >= 0) v = 0.5 * (v + column(j, ii));
            Pout[(size_t)j * n + i] = v;
            Pout[(size_t)i * n + j] = v;
        }
    }
    const int nq = 1 + (n - a.map_dim - CAM) / POSE;
    if (t < nq) normalize4(m + (t == 0 ? ORI : CAM + POSE * (t - 1) + 3));
}

struct ShiftArgs { int n, map_dim; double *m, *P, *P1, *m1; const unsigned char *active; };

// updateUndoAugmentation (ekf.cpp:888-903): m = U m, P = U P U' with the shift visUnaugmentA (251-265)
__device__ __forceinline__ int unaug_src(int i, int n, int map_dim)
{
    const int trail = n - map_dim;
    if (i < CAM || i >= trail) return i;
    return (i + POSE < trail) ? i + POSE : -1;
}

// writes the shifted covariance to P1 (the host swaps P and P1 afterwards) and the shifted mean in place
__global__ __launch_bounds__(1024) void ekf_unaugment_kernel(ShiftArgs a)
{
    const int b = blockIdx.x, t = threadIdx.x, n = a.n;
    double *m = a.m + (size_t)b * n;
    const double *P = a.P + (size_t)b * n * n;
    double *P1 = a.P1 + (size_t)b * n * n, *m1 = a.m1 + (size_t)b * n;
    if (a.active && !a.active[b]) {
        for (int e = t; e < n * n; e += 1024) P1[e] = P[e];
        return;
    }
    for (int i = t; i < n; i += 1024) { const int s = unaug_src(i, n, a.map_dim); m1[i] = s >= 0 ? m[s] : 0.0; }
    for (int e = t; e < n * n; e += 1024) {
        const int si = unaug_src(e % n, n, a.map_dim), sj = unaug_src(e / n, n, a.map_dim);
        P1[e] = (si >= 0 && sj >= 0) ? P[(size_t)sj * n + si] : 0.0;
    }
    __syncthreads();
    for (int i = t; i < n; i += 1024) m[i] = m1[i];
}

// maintainPositiveSemiDefinite (ekf.cpp:1059-1067): P = (P + P') / 2, one wavefront per pair of mirrored
// 16 x 16 tiles (in-wave LDS transpose: both tiles are read and written as 128-byte row segments)
__global__ __launch_bounds__(1024) void ekf_symmetrize_kernel(int n, double *Pall)
{
    __shared__ double scr_all[16 * 16 * 17];
    double *P = Pall + (size_t)blockIdx.x * n * n;
    const int t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63, rq = lane >> 4, c = lane & 15;
    double *scr = scr_all + wave * (16 * 17);
    const int tb = (n + 15) >> 4, npairs = tb * (tb + 1) / 2;
    for (int p = wave; p < npairs; p += 16) {
        int I, J;
        tri_decode(p, I, J);
        const int i0 = 16 * I, j0 = 16 * J;
        double x[4], y[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int r = rq + 4 * q;
            x[q] = (i0 + c < n && j0 + r < n) ? P[(size_t)(j0 + r) * n + i0 + c] : 0.0;
            y[q] = (j0 + c < n && i0 + r < n) ? P[(size_t)(i0 + r) * n + j0 + c] : 0.0;
        }
        tile_transpose(y, scr, rq, c);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            x[q] = 0.5 * (x[q] + y[q]);
            const int r = rq + 4 * q;
            if (i0 + c < n && j0 + r < n) P[(size_t)(j0 + r) * n + i0 + c] = x[q];
        }
        if (I != J) {
            tile_transpose(x, scr, rq, c);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int r = rq + 4 * q;
                if (j0 + c < n && i0 + r < n) P[(size_t)(i0 + r) * n + j0 + c] = x[q];
            }
        }
    }
}

__global__ void ekf_normalize_kernel(int n, int map_dim, double *mall, int only_current)
{
    double *m = mall + (size_t)blockIdx.x * n;
    const int nq = only_current ? 1 : 1 + (n - map_dim - CAM) / POSE;
    const int t = threadIdx.x;
    if (t < nq) normalize4(m + (t == 0 ? ORI : CAM + POSE * (t - 1) + 3));
}

// transformTo (ekf.cpp:704-758): m = A m (+ translation of every position), P = A P A' with the
// block-diagonal A = diag(pC, pC, qC, I_10, {pC, qC} x poses [, I]); one thread per block pair.
struct TransformArgs { int n, cam_poses; double *m, *P; double pC[9], qC[16], tr[3]; };   // row-major blocks

// (blk_of, the blocks of A: ekf_device.hpp)
__global__ __launch_bounds__(256) void ekf_transform_kernel(TransformArgs a)
{
    const int n = a.n, nblk = 13 + 2 * a.cam_poses + (n - CAM - POSE * a.cam_poses);
    double *P = a.P, *m = a.m;
    for (int e = threadIdx.x + blockIdx.x * 256; e < nblk * nblk; e += 256 * gridDim.x) {
        int si, ni, ki, sj, nj, kj;
        blk_of(e % nblk, a.cam_poses, si, ni, ki);
        blk_of(e / nblk, a.cam_poses, sj, nj, kj);
        if (ki == 0 && kj == 0) continue;
        double X[16], Y[16];
        for (int i = 0; i < ni; i++) for (int j = 0; j < nj; j++) X[i * 4 + j] = P[(size_t)(sj + j) * n + si + i];
        const double *Ai = ki == 1 ? a.pC : a.qC, *Aj = kj == 1 ? a.pC : a.qC;
        for (int i = 0; i < ni; i++) for (int j = 0; j < nj; j++) {      // Y = Ai X
            double s = 0;
            if (ki == 0) s = X[i * 4 + j]; else for (int k = 0; k < ni; k++) s += Ai[i * ni + k] * X[k * 4 + j];
            Y[i * 4 + j] = s;
        }
        for (int i = 0; i < ni; i++) for (int j = 0; j < nj; j++) {      // P = Y Aj'
            double s = 0;
            if (kj == 0) s = Y[i * 4 + j]; else for (int k = 0; k < nj; k++) s += Y[i * 4 + k] * Aj[j * nj + k];
            P[(size_t)(sj + j) * n + si + i] = s;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < nblk) {
        int s, sz, kind;
        blk_of(threadIdx.x, a.cam_poses, s, sz, kind);
        if (kind) {
            double x[4], y[4];
            for (int i = 0; i < sz; i++) x[i] = m[s + i];
            const double *A = kind == 1 ? a.pC : a.qC;
            for (int i = 0; i < sz; i++) { double t2 = 0; for (int k = 0; k < sz; k++) t2 += A[i * sz + k] * x[k]; y[i] = t2; }
            const bool is_pos = kind == 1 && s != VEL;
            for (int i = 0; i < sz; i++) m[s + i] = y[i] + (is_pos ? a.tr[i] : 0.0);
        }
    }
}

// insertMapPoint (ekf.cpp:911-921) on the resident state of one filter: nothing but the three coordinates crosses the bus
// (C linkage: it was defined between the C entries, and its unmangled name is in the library's symbol list)
extern "C" __global__ __launch_bounds__(256) void ekf_insert_map_point_kernel(int n, int off, double *m, double *P, double x, double y, double z)
{
    const int t = threadIdx.x;
    for (int i = t; i < 3 * n; i += 256) {
        const int k = i / n, j = i - k * n;
        P[(size_t)(off + k) * n + j] = 0.0;
        P[(size_t)j * n + off + k] = 0.0;
    }
    __syncthreads();
    if (t < 3) { P[(size_t)(off + t) * n + off + t] = 1e6; m[off + t] = t == 0 ? x : t == 1 ? y : z; }
}

}  // namespace

// the kernels' dynamic-LDS limits (ekf_kernels_init)
int ekf_augment_init(Ctx *c)
{
    HV_HIP(c, set_lds_limit(ekf_augment_kernel<false>, LDS_AUGMENT_LIMIT));      // (<true>, the device-pointer entries' folded form, stays at LDS_DEFAULT_LIMIT)
    return HV_OK;
}

}  // namespace hv

using hv::Ctx;
using hv::Ekf;

extern "C" {

// the arguments of an augmentation that do not depend on the entry (dropped0 = -1, no `dropped` / `active` arrays) and its dynamic LDS
static size_t augment_fill(const Ekf *e, hv::AugmentArgs &a)
{
    a = hv::AugmentArgs{};
    a.n = e->n; a.cam_poses = e->cam; a.map_dim = e->map_dim;
    a.m = e->fixed.m; a.P = e->fixed.P; a.P1 = e->fixed.P1; a.m1 = e->fixed.m1;
    a.dropped0 = -1;
    a.q_pos = e->par.noiseInitialPosTrail * e->par.noiseInitialPosTrail * e->noise_scale;
    a.q_ori = e->par.noiseInitialOriTrail * e->par.noiseInitialOriTrail * e->noise_scale;
    a.rd = e->par.augmentR * e->noise_scale;
    return hv::lds_bytes(hv::augment_lds(e->n, hv::AUG_THREADS / 64));
}

int hv_ekf_augment(hv_ekf *h, const int *discarded, const unsigned char *active)
{
    if (!h) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    hv::AugmentArgs a;
    const size_t shmem = augment_fill(e, a);
    if (discarded && e->batch == 1) { a.dropped0 = discarded[0]; discarded = nullptr; }      // an immediate, no copy
    hv::Stage s(c);
    const auto o_drop = s.in(discarded, (size_t)e->batch);
    const auto o_act = s.in(active, (size_t)e->batch);
    if (const int rc = s.upload()) return rc;
    a.dropped = s.at_or_null(o_drop); a.active = s.at_or_null(o_act);
    if (shmem > hv::LDS_AUGMENT_LIMIT) return HV_ERR_UNSUPPORTED;      // (state vectors with map points, n > ~190, need more than the default limit)
    hv::ScopedKernelTime tm(c, HV_K_EKF_AUGMENT);
    hipLaunchKernelGGL(hv::ekf_augment_kernel<false>, dim3(e->batch), dim3(hv::AUG_THREADS), shmem, c->stream, a);
    HV_HIP(c, hipGetLastError());
    std::swap(e->fixed.P, e->fixed.P1);                 // the kernel wrote the new covariance to the other buffer
    return HV_OK;
}

static int augment_dev_impl(hv_ekf *h, const int *discarded_dev, const unsigned char *active_dev, bool sym_input)
{
    if (!h) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    hv::AugmentArgs a;
    const size_t shmem = augment_fill(e, a);
    a.dropped = discarded_dev; a.active = active_dev;
    if (shmem > hv::LDS_DEFAULT_LIMIT) return HV_ERR_UNSUPPORTED;     // map-point states: use hv_ekf_augment (only ekf_augment_kernel<false> has a raised LDS limit)
    hv::ScopedKernelTime tm(c, HV_K_EKF_AUGMENT);
    if (sym_input) hipLaunchKernelGGL(hv::ekf_augment_kernel<true>, dim3(e->batch), dim3(hv::AUG_THREADS), shmem, c->stream, a);
    else           hipLaunchKernelGGL(hv::ekf_augment_kernel<false>, dim3(e->batch), dim3(hv::AUG_THREADS), shmem, c->stream, a);
    HV_HIP(c, hipGetLastError());
    std::swap(e->fixed.P, e->fixed.P1);
    return HV_OK;
}

// host-pointer form of hv_ekf_symmetrize_augment_dev (ABI 4)
int hv_ekf_symmetrize_augment(hv_ekf *h, const int *discarded, const unsigned char *active)
{
    if (!h) return HV_ERR_INVALID;
    Ekf *e = &h->e;
    hv::Stage s(e->c);
    const auto o_drop = s.in(discarded, (size_t)e->batch);
    const auto o_act = s.in(active, (size_t)e->batch);
    if (const int rc = s.upload()) return rc;
    const int rc = augment_dev_impl(h, s.at_or_null(o_drop), s.at_or_null(o_act), true);
    if (rc != HV_ERR_UNSUPPORTED) return rc;
    // (map-point states: the folded kernel's LDS limit; the two calls it stands for)
    const int rc2 = hv_ekf_symmetrize(h);
    return rc2 != HV_OK ? rc2 : hv_ekf_augment(h, discarded, active);
}

int hv_ekf_augment_dev(hv_ekf *h, const int *discarded_dev, const unsigned char *active_dev) { return augment_dev_impl(h, discarded_dev, active_dev, false); }
int hv_ekf_symmetrize_augment_dev(hv_ekf *h, const int *discarded_dev, const unsigned char *active_dev) { return augment_dev_impl(h, discarded_dev, active_dev, true); }

int hv_ekf_undo_augment(hv_ekf *h, const unsigned char *active)
{
    if (!h) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    hv::Stage s(c);
    const auto o_act = s.in(active, (size_t)e->batch);
    if (const int rc = s.upload()) return rc;
    hv::ShiftArgs a{e->n, e->map_dim, e->fixed.m, e->fixed.P, e->fixed.P1, e->fixed.m1, s.at_or_null(o_act)};
    hv::ScopedKernelTime tm(c, HV_K_EKF_AUGMENT);
    hipLaunchKernelGGL(hv::ekf_unaugment_kernel, dim3(e->batch), dim3(1024), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    std::swap(e->fixed.P, e->fixed.P1);
    return HV_OK;
}

// hv_ekf_undo_augment with the mask already on the device (added within ABI 4): no host copy, capturable
int hv_ekf_undo_augment_dev(hv_ekf *h, const unsigned char *active_dev)
{
    if (!h) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    hv::ShiftArgs a{e->n, e->map_dim, e->fixed.m, e->fixed.P, e->fixed.P1, e->fixed.m1, active_dev};
    hv::ScopedKernelTime tm(c, HV_K_EKF_AUGMENT);
    hipLaunchKernelGGL(hv::ekf_unaugment_kernel, dim3(e->batch), dim3(1024), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    std::swap(e->fixed.P, e->fixed.P1);
    return HV_OK;
}

int hv_ekf_symmetrize(hv_ekf *h)
{
    if (!h) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    hipLaunchKernelGGL(hv::ekf_symmetrize_kernel, dim3(e->batch), dim3(1024), 0, c->stream, e->n, e->fixed.P);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_ekf_normalize_quaternions(hv_ekf *h, int only_current)
{
    if (!h) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    hipLaunchKernelGGL(hv::ekf_normalize_kernel, dim3(e->batch), dim3(64), 0, c->stream, e->n, e->map_dim, e->fixed.m, only_current);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_ekf_transform(hv_ekf *h, int b, const double *pC3x3, const double *qC4x4, const double *translation3)
{
    if (!h || !pC3x3 || !qC4x4 || !translation3 || b < 0 || b >= h->e.batch) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    hv::TransformArgs a{};
    a.n = e->n; a.cam_poses = e->cam;
    a.m = e->fixed.m + (size_t)b * e->n; a.P = e->fixed.P + (size_t)b * e->n * e->n;
    for (int i = 0; i < 9; i++) a.pC[i] = pC3x3[i];
    for (int i = 0; i < 16; i++) a.qC[i] = qC4x4[i];
    for (int i = 0; i < 3; i++) a.tr[i] = translation3[i];
    hipLaunchKernelGGL(hv::ekf_transform_kernel, dim3(8), dim3(256), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_ekf_insert_map_point(hv_ekf *h, int b, int map_index, const double *pf)
{
    if (!h || !pf || b < 0 || b >= h->e.batch) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    if (map_index < 0 || 3 * (map_index + 1) > e->map_dim) return HV_ERR_INVALID;
    const int off = e->n - e->map_dim + 3 * map_index;
    hipLaunchKernelGGL(hv::ekf_insert_map_point_kernel, dim3(1), dim3(256), 0, c->stream, e->n, off, e->fixed.m + (size_t)b * e->n,
                       e->fixed.P + (size_t)b * e->n * e->n, pf[0], pf[1], pf[2]);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_ekf_get_map_point(hv_ekf *h, int b, int map_index, double *pf)
{
    if (!h || !pf || b < 0 || b >= h->e.batch) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    if (map_index < 0 || 3 * (map_index + 1) > e->map_dim) return HV_ERR_INVALID;
    HV_HIP(c, hipMemcpyAsync(pf, e->fixed.m + (size_t)b * e->n + e->n - e->map_dim + 3 * map_index, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    return HV_OK;
}

}  // extern "C"
