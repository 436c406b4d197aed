// EKF covariance algebra for a batch of independent filters, one workgroup per filter.
//
// Replaces the dense parts of odometry::EKF (reference: src/odometry/ekf.cpp; oracle:
// oracle/ekf_oracle.c). State m (n) and covariance P (n x n, f64, column-major as Eigen) live in
// HBM; the mean-side scalar bookkeeping (sample times, augment counters, rate limits) stays in the
// host adapter. Design for CDNA4 (numbers: scripts/f64_ubench.hip, scripts/ekf_microbench.py):
//   * f64 vector and f64 matrix peak are the same 128 flop/clk/CU on gfx950; the matrix cores are
//     used because one v_mfma_f64_16x16x4_f64 retires 1024 MACs for two operand loads (one f64 per
//     lane each) where a v_fma_f64 needs two operands per MAC, and because a lone wavefront issues a
//     dependent v_fma_f64 only every ~7 cycles;
//   * visual update / chi2 gate (ekf_update_kernel): S = H P H' + R is factored and both triangular
//     solves are done in ONE blocked Cholesky pass over the tall matrix T = [S ; v' ; (HP)'] in LDS
//     (16-column blocks: MFMA panel / trailing updates, the 16 x 16 diagonal factor and its inverse
//     in the registers of one wavefront), after which chi2 = ns z'z, m += Y'z, P -= Y'Y with
//     Y = L^-1 HP. K is never formed; the reference forms K = (S^-1 HP)' with a pivoted LDLT and
//     P -= K HP, algebraically identical (parity 1e-9 relative per call, measured ~1e-13). At the
//     reference's sizes (n = 160, <= 47 rows) H is staged in LDS too and every wavefront owns whole
//     16-column blocks of P: the tiles it streams from HBM as MFMA operands of H P are already in the
//     accumulator layout of P -= Y'Y and stay in registers until then, so P is read once per update;
//   * predict: thread 0 evaluates the mean and the 20 x 20 Jacobians while the other wavefronts
//     already hold the slabs of P10 / P01 they need; the off-diagonal blocks are MFMA items;
//   * pose augmentation: the Joseph form (I-KH) P (I-KH)' + K R K' is expanded around the 7-row
//     +-1 matrix visAugH into a rank-14 correction (4 MFMA k-steps per 16 x 16 tile) of the shifted
//     matrix A P A' + Q, which is a gather of P and never materialised; mirrored tile pairs meet
//     through an in-wave LDS transpose for the fused (P+P')/2, and the result goes to the second of
//     two ping-pong buffers: one read and one write of P per augmentation. The 14 rows and columns
//     visAugH touches are then rewritten from the Joseph form itself (W = T P1 times the rows of T,
//     formed first): the expansion cancels the slot's 1e8 prior against itself there and loses seven
//     to eight digits of entries of size 1e-6, which a whole-matrix norm never sees.
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <utility>

#include <stdlib.h>

#include "ekf_device.hpp"
#include "ekf_host.hpp"

// The library is built with -ffp-contract=off for the tracker's bit-exact binary32 sequence; the
// EKF is judged against a relative tolerance, and a fused multiply-add is one rounding fewer and
// half the f64 instructions of its dependency chains.
#pragma clang fp contract(fast)

namespace hv {

namespace {


// developer aid: s_memtime stamps of the kernels' phases (block 0, thread 0), read back through
// hv_debug_ekf_phase_stamps. Compiled in only with -DHV_EKF_PHASE_STAMPS (HV_EKF_PHASE_STAMPS=1 in the
// environment of hybvio_amd/build.py): every stamp is a scalar memory wait in the middle of a pipeline.
}  // namespace
__device__ long long g_phase_stamp[16];
namespace {
#ifdef HV_EKF_PHASE_STAMPS
#define PHASE_STAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_phase_stamp[i] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define PHASE_STAMP(i) do { } while (0)
#endif


__device__ __forceinline__ void normalize4(double *q)
{
    const double nn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (nn > 0.0) { q[0] /= nn; q[1] /= nn; q[2] /= nn; q[3] /= nn; }
}

// ---------------------------------------------------------------------------------------------
// predict (ekf.cpp:320-514)
// ---------------------------------------------------------------------------------------------
struct PredictArgs {
    int n, batch;
    double *m, *P, *Q, *dydx;            // per filter: n, n*n, 144, 400
    const double *dt, *gyro, *acc;        // device arrays [batch], [batch*3], [batch*3] (or null -> immediates)
    double dt0, g0[3], a0[3];
    int nsteps;                           // IMU samples per launch; device arrays are [nsteps][batch](x3)
    double noise_scale, gravity, baa, baa_rev, bga, bga_rev;
};

__device__ void quat2rmat_d(const double q[4], double R[9], double dR[36])   // util.cpp:10-47, column-major
{
    const double rows[4][9] = {
        { 2*q[0], -2*q[3],  2*q[2],   2*q[3],  2*q[0], -2*q[1],  -2*q[2],  2*q[1],  2*q[0] },
        { 2*q[1],  2*q[2],  2*q[3],   2*q[2], -2*q[1], -2*q[0],   2*q[3],  2*q[0], -2*q[1] },
        {-2*q[2],  2*q[1],  2*q[0],   2*q[1],  2*q[2],  2*q[3],  -2*q[0],  2*q[3], -2*q[2] },
        {-2*q[3], -2*q[0],  2*q[1],   2*q[0], -2*q[3],  2*q[2],   2*q[1],  2*q[2],  2*q[3] } };
    for (int k = 0; k < 4; k++)
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) dR[9 * k + 3 * j + i] = rows[k][3 * i + j];
    const double Rr[9] = {
        q[0]*q[0]+q[1]*q[1]-q[2]*q[2]-q[3]*q[3], 2*q[1]*q[2] - 2*q[0]*q[3], 2*q[1]*q[3] + 2*q[0]*q[2],
        2*q[1]*q[2] + 2*q[0]*q[3], q[0]*q[0]-q[1]*q[1]+q[2]*q[2]-q[3]*q[3], 2*q[2]*q[3] - 2*q[0]*q[1],
        2*q[1]*q[3] - 2*q[0]*q[2], 2*q[2]*q[3] + 2*q[0]*q[1], q[0]*q[0]-q[1]*q[1]-q[2]*q[2]+q[3]*q[3] };
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[3 * j + i] = Rr[3 * i + j];
}

// cos(th) and sin(th) / th of the half rotation angle th = |w| dt / 2 >= 0 of one IMU sample (ekf.cpp:415-425). Below 0.25 rad -- 100 rad/s at
// dt = 5 ms; every sample a camera rig produces -- both are Taylor polynomials in th^2 up to th^16 / th^17 (remainder < 1e-26), two Horner
// chains side by side on the one lane that owns the mean's serial section, instead of the device library's cos() and sin() with their
// argument reduction and a division (~1.1 k of a sample's ~2.9 k cycles, late r06). Within an ulp of the library's values; the
// reference's own branch for th <= 1e-8 is kept as it is.
__device__ __forceinline__ void cos_sinc(double th, double &c, double &sc)
{
    if (th < 0.25) {
        const double x = th * th;
        double pc = 1.0 / 20922789888000.0, ps = -1.0 / 355687428096000.0;     // 1 / 16!, -1 / 17!
        pc = pc * x - 1.0 / 87178291200.0;   ps = ps * x + 1.0 / 1307674368000.0;   // -1 / 14!, 1 / 15!
        pc = pc * x + 1.0 / 479001600.0;     ps = ps * x - 1.0 / 6227020800.0;      //  1 / 12!, -1 / 13!
        pc = pc * x - 1.0 / 3628800.0;       ps = ps * x + 1.0 / 39916800.0;        // -1 / 10!, 1 / 11!
        pc = pc * x + 1.0 / 40320.0;         ps = ps * x - 1.0 / 362880.0;          //  1 / 8!, -1 / 9!
        pc = pc * x - 1.0 / 720.0;           ps = ps * x + 1.0 / 5040.0;            // -1 / 6!, 1 / 7!
        pc = pc * x + 1.0 / 24.0;            ps = ps * x - 1.0 / 120.0;             //  1 / 4!, -1 / 5!
        pc = pc * x - 0.5;                   ps = ps * x + 1.0 / 6.0;               // -1 / 2!, 1 / 3!
        c = pc * x + 1.0;
        sc = th > 1e-8 ? 1.0 - ps * x : 1.0 - th * th / 6.0;
    } else {
        c = cos(th); sc = sin(th) / th;
    }
}

// entry t = 3 i + j of Rr(q) (util.cpp:10-47), for the lane that owns it: two code paths -- the diagonal's four squares, the off-diagonal's
// two products -- with the operands selected per lane (a `switch` over the nine entries ran its cases one after the other: ~890 cycles of a
// sample's mean recursion, late r06). Shared by both predict kernels, so that they contract to the same FMAs.
__device__ __forceinline__ double quat_rotation_entry(int t, const double *sqn)
{
    const double qq[4] = {sqn[0], sqn[1], sqn[2], sqn[3]};
    const int i = t / 3, j = t - 3 * i;
    if (i == j) {                                           // q0^2 + s1 q1^2 + s2 q2^2 + s3 q3^2, signs (+ - -), (- + -), (- - +)
        const double a1 = qq[1] * qq[1], a2 = qq[2] * qq[2], a3 = qq[3] * qq[3];
        double acc = qq[0] * qq[0];
        acc = i == 0 ? acc + a1 : acc - a1;
        acc = i == 1 ? acc + a2 : acc - a2;
        acc = i == 2 ? acc + a3 : acc - a3;
        return acc;
    }
    // Rr: (0,1) 2q1q2 - 2q0q3, (0,2) 2q1q3 + 2q0q2, (1,0) 2q1q2 + 2q0q3, (1,2) 2q2q3 - 2q0q1, (2,0) 2q1q3 - 2q0q2, (2,1) 2q2q3 + 2q0q1
    const int ia = i + 1, ib = j + 1, ic = 6 - ia - ib;
    const int lo = ia < ib ? ia : ib, hi = ia < ib ? ib : ia;
    const double p = 2 * qq[lo] * qq[hi], r = 2 * qq[0] * qq[ic];
    const bool plus = (i == 0 && j == 2) || (i == 1 && j == 0) || (i == 2 && j == 1);
    return plus ? p + r : p - r;
}

#define F_(i, j) F[(j) * INER + (i)]
#define L_(i, j) Lm[(j) * INER + (i)]

// (two workgroups per CU: 256 registers per lane)
__global__ __launch_bounds__(256, 2) void ekf_predict_kernel(PredictArgs a)
{
    __shared__ double F[INER * INER], Lm[INER * QD], Qs[QD * QD], LQ[INER * QD], P00[INER * INER], FP[INER * INER];
    __shared__ double Phi[INER * INER], PhiN[INER * INER];
    __shared__ double ms[INER], sh[112];           // the inertial part of the mean; stage values of the mean / F / L section
    const int b = blockIdx.x, t = threadIdx.x, n = a.n;
    double *m = a.m + (size_t)b * n, *P = a.P + (size_t)b * n * n, *Q = a.Q + (size_t)b * QD * QD;
    // nsteps IMU samples in one launch: the mean / Jacobian chain and the 20 x 20 block recursion
    // P00 <- F P00 F' + L Q L' run per sample in LDS; the off-diagonal blocks only ever see the product
    // Phi = F_n ... F_1 (P10 <- P10 Phi', P01 <- Phi P01), so they are touched once at the end.
    bool any = false;
    for (int s = 0; s < a.nsteps; s++) { const double d = a.dt ? a.dt[(size_t)s * a.batch + b] : a.dt0; any = any || d > 0.0; }
    if (!any) return;                              // ekf.cpp:365-368 (the host adapter keeps the clock)

    PHASE_STAMP(12);
    // Off-diagonal blocks P10 <- P10 F', P01 <- F P01 (ekf.cpp:506-508) as MFMA items: item I < tiles is
    // the 16-row tile I of P10, item tiles + C the 16-column tile C of P01; either one needs a 16 x 20
    // slab of P (5 k-steps, one f64 per lane each) and all of F. The slabs of the first five items of
    // every wave are requested here, before thread 0 starts on the mean / F / L, so that their HBM
    // round trip hides behind that serial section.
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63, kq = lane >> 4, cl = lane & 15;
    const int tiles = (n - INER + 15) >> 4;
    constexpr int NIT = 5;
    auto slab_ptr = [&](int it, int sx) -> double * {
        const int k = min(4 * sx + kq, INER - 1);
        if (it < tiles) return P + (size_t)k * n + min(INER + 16 * it + cl, n - 1);          // P10(i, k): lanes along i
        return P + (size_t)min(INER + 16 * (it - tiles) + cl, n - 1) * n + k;                // P01(k, c): lanes along c
    };
    double slab[NIT][5];
#pragma unroll
    for (int u = 0; u < NIT; u++) {
        const int it = wave + 4 * u;
        if (it < 2 * tiles) {
#pragma unroll
            for (int sx = 0; sx < 5; sx++) slab[u][sx] = *slab_ptr(it, sx);
        }
    }
    for (int i = t; i < INER * INER; i += 256) { Phi[i] = (i % (INER + 1) == 0) ? 1.0 : 0.0; P00[i] = P[(size_t)(i / INER) * n + (i % INER)]; }
    for (int i = t; i < QD * QD; i += 256) Qs[i] = Q[i];
    if (t < INER) ms[t] = m[t];

    double exp_dt = -1.0, e_baa2 = 1.0, e_bga2 = 1.0, e_baa1 = 1.0, e_bga1 = 1.0;     // thread 0 only
    for (int step = 0; step < a.nsteps; step++) {
    const size_t sb = (size_t)step * a.batch + b;
    const double dt = a.dt ? a.dt[sb] : a.dt0;
    if (!(dt > 0.0)) continue;                     // uniform per workgroup
    __syncthreads();
    for (int i = t; i < INER * INER; i += 256) F[i] = (i % (INER + 1) == 0) ? 1.0 : 0.0;
    for (int i = t; i < INER * QD; i += 256) Lm[i] = 0.0;
    __syncthreads();

    // ---- mean, F and L of this sample (ekf.cpp:370-503). r01 ran this section on thread 0 (~1.5 k dependent f64 instructions,
    // half of a sample's time); here every ELEMENT is still evaluated by one lane with the reference's expression and summation
    // order -- results are unchanged -- but the elements of a stage are spread over the lanes of the workgroup, with a barrier
    // where a stage reads what the previous one wrote. Stage scalars and small matrices live in `sh`.
    double *const sA = sh, *const sSrow = sh + 16, *const sqn = sh + 32, *const sprevQ = sh + 36, *const sR = sh + 40,
           *const sdR = sh + 49, *const sTxab = sh + 85, *const sT34 = sh + 88, *const sxa = sh + 100, *const ssc = sh + 103;
    if (t == 0) {
        double xg[3];
        for (int i = 0; i < 3; i++) { xg[i] = a.gyro ? a.gyro[3 * sb + i] : a.g0[i]; sxa[i] = a.acc ? a.acc[3 * sb + i] : a.a0[i]; }
        // the four exponentials of a sample depend on dt only: evaluated when dt changes (IMU samples are equally spaced as a
        // rule, so once per launch), the same values as the per-sample evaluation
        if (dt != exp_dt) {
            exp_dt = dt;
            e_baa2 = a.baa_rev > 0.0 ? (1 - exp(-2 * dt * a.baa_rev)) / (2 * a.baa_rev) : 1.0;
            e_bga2 = a.bga_rev > 0.0 ? (1 - exp(-2 * dt * a.bga_rev)) / (2 * a.bga_rev) : 1.0;
            e_baa1 = exp(-dt * a.baa_rev); e_bga1 = exp(-dt * a.bga_rev);
        }
        ssc[2] = e_baa1; ssc[3] = e_bga1;
        if (a.baa > 0.0) {                          // ekf.cpp:397-404
            double v = a.noise_scale * a.baa * a.baa;
            if (a.baa_rev > 0.0) v *= e_baa2;
            for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Qs[(Q_BAA_DRIFT + j) * QD + Q_BAA_DRIFT + i] = (i == j) ? v : 0.0;
        }
        if (a.bga > 0.0) {                          // ekf.cpp:405-412
            double v = a.noise_scale * a.bga * a.bga;
            if (a.bga_rev > 0.0) v *= e_bga2;
            for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Qs[(Q_BGA_DRIFT + j) * QD + Q_BGA_DRIFT + i] = (i == j) ? v : 0.0;
        }
        // A = exp(-dt/2 Omega(w)) = cos(th) I + sin(th)/th S, th = |w| dt/2   (ekf.cpp:415-425)
        const double w[3] = { xg[0] - ms[BGA], xg[1] - ms[BGA + 1], xg[2] - ms[BGA + 2] };
        const double Srow[16] = { 0, -w[0], -w[1], -w[2],  w[0], 0, -w[2], w[1],  w[1], w[2], 0, -w[0],  w[2], -w[1], w[0], 0 };
#pragma unroll
        for (int i = 0; i < 16; i++) sSrow[i] = Srow[i];
        const double th = sqrt(w[0]*w[0] + w[1]*w[1] + w[2]*w[2]) * dt / 2;
        cos_sinc(th, ssc[0], ssc[1]);
    }
    __syncthreads();
    {   // stage B: A (column-major 4x4), the previous quaternion, T xa - ba, the position
        const double c = ssc[0], sc = ssc[1];
        if (t < 16) { const int i = t & 3, j = t >> 2; sA[4 * j + i] = sc * sSrow[4 * i + j] * (-dt / 2) + (i == j ? c : 0.0); }
        else if (t < 20) sprevQ[t - 16] = ms[ORI + t - 16];
        else if (t >= 32 && t < 35) { const int i = t - 32; sTxab[i] = ms[BAT + i] * sxa[i] - ms[BAA + i]; }
        else if (t >= 40 && t < 43) { const int i = t - 40; ms[POS + i] += ms[VEL + i] * dt; }
    }
    __syncthreads();
    if (t < 4) { double s_ = 0; for (int j = 0; j < 4; j++) s_ += sA[4 * j + t] * sprevQ[j]; sqn[t] = s_; }
    __syncthreads();
    {   // stage D: R(q) and dR/dq (util.cpp:10-47, column-major): one element per lane
        const double q0 = sqn[0], q1 = sqn[1], q2 = sqn[2], q3 = sqn[3];
        if (t < 9) {
            const int i = t / 3, j = t - 3 * i;                 // Rr[3 i + j] -> R[3 j + i]
            const double v = quat_rotation_entry(t, sqn);
            sR[3 * j + i] = v;
        } else if (t >= 64 && t < 100) {
            // rows[k][3 i + j] = sign * 2 q[idx]: two bits of index and one of sign per entry
            const int e = t - 64, k = e / 9, ij = e - 9 * k, i = ij / 3, j = ij - 3 * i;
            constexpr unsigned char IDX[4][9] = { {0,3,2, 3,0,1, 2,1,0}, {1,2,3, 2,1,0, 3,0,1}, {2,1,0, 1,2,3, 0,3,2}, {3,0,1, 0,3,2, 1,2,3} };
            constexpr signed char SGN[4][9] = { {1,-1,1, 1,1,-1, -1,1,1}, {1,1,1, 1,-1,-1, 1,1,-1}, {-1,1,1, 1,1,1, -1,1,-1}, {-1,-1,1, 1,-1,1, 1,1,1} };
            const int id = IDX[k][ij];
            const double qv = id == 0 ? q0 : id == 1 ? q1 : id == 2 ? q2 : q3;
            sdR[9 * k + 3 * j + i] = SGN[k][ij] > 0 ? 2 * qv : -2 * qv;
        }
    }
    __syncthreads();
    {   // stage E: the rest of the mean; the entries of F and L that depend on R, dR, A only
        if (t < 3) {
            const int i = t;
            const double grav = i == 2 ? -a.gravity : 0.0;
            double s_ = 0; for (int j = 0; j < 3; j++) s_ += sR[3 * i + j] * sTxab[j];
            ms[VEL + i] += (s_ + grav) * dt;
            F_(POS + i, VEL + i) = dt;
            L_(BGA + i, Q_BGA_DRIFT + i) = 1.0; L_(BAA + i, Q_BAA_DRIFT + i) = 1.0;
        } else if (t >= 4 && t < 8) ms[ORI + t - 4] = sqn[t - 4];
        else if (t >= 8 && t < 11) { if (a.baa > 0.0) ms[BAA + t - 8] *= ssc[2]; }
        else if (t >= 12 && t < 15) { if (a.bga > 0.0) ms[BGA + t - 12] *= ssc[3]; }
        else if (t >= 16 && t < 28) {
            const int e = t - 16, k = e / 3, i = e - 3 * k;
            double s_ = 0; for (int j = 0; j < 3; j++) s_ += sdR[9 * k + 3 * i + j] * sTxab[j];
            sT34[3 * k + i] = s_ * dt;
        } else if (t >= 32 && t < 44) {
            const int e = t - 32, g = e >> 2, i = e & 3;
            const double h = dt / 2;
            const double dS[3][16] = {
                { 0, h, 0, 0,  -h, 0, 0, 0,  0, 0, 0, h,  0, 0, -h, 0 },
                { 0, 0, h, 0,  0, 0, 0, -h,  -h, 0, 0, 0,  0, h, 0, 0 },
                { 0, 0, 0, h,  0, 0, h, 0,  0, -h, 0, 0,  -h, 0, 0, 0 } };
            double t1[4];
#pragma unroll
            for (int ii = 0; ii < 4; ii++) {
                double s_ = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) { const double d = g == 0 ? dS[0][4 * ii + j] : g == 1 ? dS[1][4 * ii + j] : dS[2][4 * ii + j]; s_ += d * sprevQ[j]; }
                t1[ii] = s_;
            }
            double s_ = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) s_ += sA[4 * j + i] * t1[j];
            L_(ORI + i, Q_GYRO + g) = s_;
        } else if (t >= 48 && t < 57) {
            const int e = t - 48, i = e / 3, j = e - 3 * i;
            L_(VEL + i, Q_ACC + j) = sR[3 * i + j] * dt;
            F_(VEL + i, BAA + j) = -sR[3 * i + j] * dt; F_(VEL + i, BAT + j) = sR[3 * i + j] * sxa[j] * dt;
        } else if (t >= 64 && t < 80) {
            const int e = t - 64, i = e & 3, j = e >> 2;
            F_(ORI + i, ORI + j) = sA[4 * j + i];
        }
    }
    __syncthreads();
    if (t < 12) {
        const int i = t / 4, j = t - 4 * i;
        double s_ = 0; for (int k = 0; k < 4; k++) s_ += sT34[3 * k + i] * sA[4 * j + k];
        F_(VEL + i, ORI + j) = s_;
    }
    __syncthreads();
    if (t < 9) {
        const int i = t / 3, g = t - 3 * i;
        double s_ = 0; for (int k = 0; k < 4; k++) s_ += F_(VEL + i, ORI + k) * L_(ORI + k, Q_GYRO + g);
        L_(VEL + i, Q_GYRO + g) = s_;
        F_(VEL + i, BGA + g) = -s_;
    } else if (t >= 16 && t < 28) {
        const int e = t - 16, i = e / 3, g = e - 3 * i;
        F_(ORI + i, BGA + g) = -L_(ORI + i, Q_GYRO + g);
    }
    __syncthreads();

    PHASE_STAMP(13);
    // P00 = F P00 F' + L Q L' (ekf.cpp:504-505) in LDS; Phi <- F Phi. The 20 x 20 results are four 16 x 16 MFMA tiles, one per
    // wavefront (f64 16x16x4, 5 k-steps): a chain of 5 MFMAs per product where the r01 loops spent 20-32 dependent LDS round trips per
    // element (a sample's products 3 x ~1.3 us -> well under 1 us; the summation order inside a product changes, ~1e-16 relative)
    {
        const int ti = wave & 1, tj = wave >> 1;                 // output rows 16 ti .., columns 16 tj ..
        const int mi = ti ? INER - 16 : 16, nj = tj ? INER - 16 : 16;
        // A(i, k) = F_(16 ti + i, k) = F[k INER + 16 ti + i];  B(k, j) = P00(k, 16 tj + j) = P00[(16 tj + j) INER + k]
        const double4v fp = mfma_tile(F + 16 * ti, 1, INER, mi, P00 + 16 * tj * INER, 1, INER, nj, INER);
        const double4v ph = mfma_tile(F + 16 * ti, 1, INER, mi, Phi + 16 * tj * INER, 1, INER, nj, INER);
        // L Q (20 x 12): row tiles on wavefronts 0 and 1. LQ(i, j) = sum_k L(i, k) Qs(j, k): B(k, j) = Qs[j QD + k]
        double4v lq = {0.0, 0.0, 0.0, 0.0};
        if (wave < 2) lq = mfma_tile(Lm + 16 * wave, 1, INER, wave ? INER - 16 : 16, Qs, 1, QD, QD, QD);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int r = kq + 4 * q;
            if (r < mi && cl < nj) { FP[(16 * tj + cl) * INER + 16 * ti + r] = fp[q]; PhiN[(16 * tj + cl) * INER + 16 * ti + r] = ph[q]; }
            if (wave < 2 && r < (wave ? INER - 16 : 16) && cl < QD) LQ[cl * INER + 16 * wave + r] = lq[q];
        }
        __syncthreads();
        // P00(i, j) = sum_k FP(i, k) F_(j, k) + sum_k LQ(i, k) L_(j, k): B(k, j) = F[k INER + 16 tj + j] resp. Lm[k INER + 16 tj + j]
        const double4v p1 = mfma_tile(FP + 16 * ti, 1, INER, mi, F + 16 * tj, INER, 1, nj, INER);
        const double4v p2 = mfma_tile(LQ + 16 * ti, 1, INER, mi, Lm + 16 * tj, INER, 1, nj, QD);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int r = kq + 4 * q;
            if (r < mi && cl < nj) P00[(16 * tj + cl) * INER + 16 * ti + r] = p1[q] + p2[q];
        }
        for (int e = t; e < INER * INER; e += 256) Phi[e] = PhiN[e];
    }
    }
    __syncthreads();
    for (int i = t; i < INER * INER; i += 256) { P[(size_t)(i / INER) * n + (i % INER)] = P00[i]; a.dydx[(size_t)b * INER * INER + i] = F[i]; }
    for (int i = t; i < QD * QD; i += 256) Q[i] = Qs[i];
    if (t < INER) m[t] = ms[t];
    PHASE_STAMP(14);
    {
        // F operand (the product Phi of the steps' F), shared by every item: lane (kq, cl) holds Phi(cl + 16 tt, 4 s + kq). It is the A operand
        // of (P10 F')' = F P10' (rows c of F, columns i of the tile) and the B operand of (F P01)' =
        // P01' F' (rows c of the tile, columns r of F): both products are formed transposed so that the
        // 16 lanes of an output row group store 16 consecutive doubles.
        double f0[5], f1[5];
#pragma unroll
        for (int sx = 0; sx < 5; sx++) {
            const int k = 4 * sx + kq;                                                        // < 20
            f0[sx] = Phi[k * INER + cl];
            f1[sx] = Phi[k * INER + min(16 + cl, INER - 1)];
        }
        for (int base = 0; base < 2 * tiles; base += 4 * NIT) {
#pragma unroll
            for (int u = 0; u < NIT; u++) {
                const int it = base + wave + 4 * u;
                if (it < 2 * tiles) {
                    if (base > 0) {
#pragma unroll
                        for (int sx = 0; sx < 5; sx++) slab[u][sx] = *slab_ptr(it, sx);
                    }
                    double4v a0 = {0.0, 0.0, 0.0, 0.0}, a1 = a0;
                    const bool p10 = it < tiles;
#pragma unroll
                    for (int sx = 0; sx < 5; sx++) {
                        const double x0 = p10 ? f0[sx] : slab[u][sx], y0 = p10 ? slab[u][sx] : f0[sx];
                        const double x1 = p10 ? f1[sx] : slab[u][sx], y1 = p10 ? slab[u][sx] : f1[sx];
                        a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, y0, a0, 0, 0, 0);
                        a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, y1, a1, 0, 0, 0);
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int rr = kq + 4 * q;                                            // output row within the tile
                        if (p10) {
                            const int i = INER + 16 * it + cl;                                // (c = rr [+16], i)
                            if (i < n) {
                                P[(size_t)rr * n + i] = a0[q];
                                if (16 + rr < INER) P[(size_t)(16 + rr) * n + i] = a1[q];
                            }
                        } else {
                            const int c = INER + 16 * (it - tiles) + rr;                      // (c, r = cl [+16])
                            if (c < n) {
                                P[(size_t)c * n + cl] = a0[q];
                                if (16 + cl < INER) P[(size_t)c * n + 16 + cl] = a1[q];
                            }
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    PHASE_STAMP(15);
}


// ---------------------------------------------------------------------------------------------
// ekf_predict_chain_kernel (late r06): the same arithmetic as ekf_predict_kernel, element by element and in the same
// order -- results are bit-identical --, with the sample-to-sample dependency reduced to what really depends: the MEAN. A sample's F and L
// only read quantities of the mean recursion (A, the old and the new quaternion, R, T xa - ba, dt), so
//   phase 1  ONE wavefront runs the mean recursion of up to PCH samples back to back -- five short stages per sample that talk through LDS
//            inside the wave (DS operations of a wave execute in order: a wave-level fence, no workgroup barrier) -- and leaves every
//            sample's stage values in its own slot;
//   phase 2  all 256 threads form dR, F and L of ALL those samples at once (four workgroup barriers per chunk instead of nine per sample);
//   phase 3  the 20 x 20 recursions P00 <- F P00 F' + L Q L', Phi <- F Phi sample by sample (two barriers each), as before.
// ekf_predict_kernel spent ~5.3 us per sample on nine barrier-separated stages (profiles/r06/predict_pipe_ab.txt); knob ekf_predict_chain 0
// keeps it.
constexpr int PCH = 5;                  // samples per chunk (F and L of a chunk stay in LDS: 5 x (400 + 240) doubles)
__device__ __forceinline__ void wave_sync_lds()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256, 2) void ekf_predict_chain_kernel(PredictArgs a)
{
    constexpr int SHW = 112;                                  // stage values of one sample (the layout of ekf_predict_kernel's `sh`) ...
    constexpr int X_DT = 107, X_LIVE = 108, X_VBAA = 109, X_VBGA = 110;   // ... + its dt, whether it runs, the drift variances of Q
    __shared__ double Fs[PCH * INER * INER], Ls[PCH * INER * QD], Qs[QD * QD], LQ[INER * QD], P00[INER * INER], FP[INER * INER];
    __shared__ double Phi[INER * INER], PhiN[INER * INER];
    __shared__ double ms[INER], shs[PCH * SHW], imu[PCH * 8];    // imu: dt, gyro[3], acc[3] of the chunk's samples
    const int b = blockIdx.x, t = threadIdx.x, n = a.n;
    double *m = a.m + (size_t)b * n, *P = a.P + (size_t)b * n * n, *Q = a.Q + (size_t)b * QD * QD;
    bool any = false;
    for (int s = 0; s < a.nsteps; s++) { const double d = a.dt ? a.dt[(size_t)s * a.batch + b] : a.dt0; any = any || d > 0.0; }
    if (!any) return;                              // ekf.cpp:365-368 (the host adapter keeps the clock)

    PHASE_STAMP(12);
    // off-diagonal items: the slabs of the first five items of every wave are requested here (see ekf_predict_kernel)
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63, kq = lane >> 4, cl = lane & 15;
    const int tiles = (n - INER + 15) >> 4;
    constexpr int NIT = 5;
    auto slab_ptr = [&](int it, int sx) -> double * {
        const int k = min(4 * sx + kq, INER - 1);
        if (it < tiles) return P + (size_t)k * n + min(INER + 16 * it + cl, n - 1);          // P10(i, k): lanes along i
        return P + (size_t)min(INER + 16 * (it - tiles) + cl, n - 1) * n + k;                // P01(k, c): lanes along c
    };
    double slab[NIT][5];
#pragma unroll
    for (int u = 0; u < NIT; u++) {
        const int it = wave + 4 * u;
        if (it < 2 * tiles) {
#pragma unroll
            for (int sx = 0; sx < 5; sx++) slab[u][sx] = *slab_ptr(it, sx);
        }
    }
    for (int i = t; i < INER * INER; i += 256) { Phi[i] = (i % (INER + 1) == 0) ? 1.0 : 0.0; P00[i] = P[(size_t)(i / INER) * n + (i % INER)]; }
    for (int i = t; i < QD * QD; i += 256) Qs[i] = Q[i];
    if (t < INER) ms[t] = m[t];
    __syncthreads();

    double exp_dt = -1.0, e_baa2 = 1.0, e_bga2 = 1.0, e_baa1 = 1.0, e_bga1 = 1.0;     // lane 0 of wave 0 only
    for (int s0 = 0; s0 < a.nsteps; s0 += PCH) {
        const int ns = min(PCH, a.nsteps - s0);
        // the chunk's IMU samples in ONE round trip (requested per sample, every sample's chain started with two dependent global loads)
        if (t < ns * 8) {
            const int sl = t >> 3, e = t & 7;
            const size_t sb = (size_t)(s0 + sl) * a.batch + b;
            double v = 0.0;
            if (e == 0) v = a.dt ? a.dt[sb] : a.dt0;
            else if (e < 4) v = a.gyro ? a.gyro[3 * sb + e - 1] : a.g0[e - 1];
            else if (e < 7) v = a.acc ? a.acc[3 * sb + e - 4] : a.a0[e - 4];
            imu[t] = v;
        }
        __syncthreads();
        // ---- phase 1: the mean recursion of the chunk's samples (ekf.cpp:370-503, the entries of the mean), wave 0 ----
        if (wave == 0) {
            for (int sl = 0; sl < ns; sl++) {
                double *const sh = shs + sl * SHW;
                double *const sA = sh, *const sSrow = sh + 16, *const sqn = sh + 32, *const sprevQ = sh + 36, *const sR = sh + 40,
                       *const sTxab = sh + 85, *const sxa = sh + 100, *const ssc = sh + 103;
                const double dt = imu[8 * sl];
                if (t == 0) { sh[X_DT] = dt; sh[X_LIVE] = dt > 0.0 ? 1.0 : 0.0; }
                if (!(dt > 0.0)) continue;                     // uniform
                if (s0 == 0 && sl == 0) PHASE_STAMP(0);
                if (t == 0) {
                    double xg[3];
                    for (int i = 0; i < 3; i++) { xg[i] = imu[8 * sl + 1 + i]; sxa[i] = imu[8 * sl + 4 + i]; }
                    if (dt != exp_dt) {
                        exp_dt = dt;
                        e_baa2 = a.baa_rev > 0.0 ? (1 - exp(-2 * dt * a.baa_rev)) / (2 * a.baa_rev) : 1.0;
                        e_bga2 = a.bga_rev > 0.0 ? (1 - exp(-2 * dt * a.bga_rev)) / (2 * a.bga_rev) : 1.0;
                        e_baa1 = exp(-dt * a.baa_rev); e_bga1 = exp(-dt * a.bga_rev);
                    }
                    ssc[2] = e_baa1; ssc[3] = e_bga1;
                    if (a.baa > 0.0) { double v = a.noise_scale * a.baa * a.baa; if (a.baa_rev > 0.0) v *= e_baa2; sh[X_VBAA] = v; }   // ekf.cpp:397-404
                    if (a.bga > 0.0) { double v = a.noise_scale * a.bga * a.bga; if (a.bga_rev > 0.0) v *= e_bga2; sh[X_VBGA] = v; }   // ekf.cpp:405-412
                    // A = exp(-dt/2 Omega(w)) = cos(th) I + sin(th)/th S, th = |w| dt/2   (ekf.cpp:415-425)
                    const double w[3] = { xg[0] - ms[BGA], xg[1] - ms[BGA + 1], xg[2] - ms[BGA + 2] };
                    const double Srow[16] = { 0, -w[0], -w[1], -w[2],  w[0], 0, -w[2], w[1],  w[1], w[2], 0, -w[0],  w[2], -w[1], w[0], 0 };
#pragma unroll
                    for (int i = 0; i < 16; i++) sSrow[i] = Srow[i];
                    const double th = sqrt(w[0]*w[0] + w[1]*w[1] + w[2]*w[2]) * dt / 2;
                    cos_sinc(th, ssc[0], ssc[1]);
                }
                wave_sync_lds();
                if (s0 == 0 && sl == 0) PHASE_STAMP(1);
                {   // stage B: A (column-major 4x4), the previous quaternion, T xa - ba, the position
                    const double c = ssc[0], sc = ssc[1];
                    if (t < 16) { const int i = t & 3, j = t >> 2; sA[4 * j + i] = sc * sSrow[4 * i + j] * (-dt / 2) + (i == j ? c : 0.0); }
                    else if (t < 20) sprevQ[t - 16] = ms[ORI + t - 16];
                    else if (t >= 32 && t < 35) { const int i = t - 32; sTxab[i] = ms[BAT + i] * sxa[i] - ms[BAA + i]; }
                    else if (t >= 40 && t < 43) { const int i = t - 40; ms[POS + i] += ms[VEL + i] * dt; }
                }
                wave_sync_lds();
                if (s0 == 0 && sl == 0) PHASE_STAMP(2);
                if (t < 4) { double s_ = 0; for (int j = 0; j < 4; j++) s_ += sA[4 * j + t] * sprevQ[j]; sqn[t] = s_; }
                wave_sync_lds();
                if (s0 == 0 && sl == 0) PHASE_STAMP(3);
                if (t < 9) {   // stage D, the part the mean needs: R(q) (util.cpp:10-47, column-major)
                    const int i = t / 3, j = t - 3 * i;                 // Rr[3 i + j] -> R[3 j + i]
                    sR[3 * j + i] = quat_rotation_entry(t, sqn);
                }
                wave_sync_lds();
                if (s0 == 0 && sl == 0) PHASE_STAMP(4);
                {   // stage E, the entries of the mean
                    if (t < 3) {
                        const int i = t;
                        const double grav = i == 2 ? -a.gravity : 0.0;
                        double s_ = 0; for (int j = 0; j < 3; j++) s_ += sR[3 * i + j] * sTxab[j];
                        ms[VEL + i] += (s_ + grav) * dt;
                    } else if (t >= 4 && t < 8) ms[ORI + t - 4] = sqn[t - 4];
                    else if (t >= 8 && t < 11) { if (a.baa > 0.0) ms[BAA + t - 8] *= ssc[2]; }
                    else if (t >= 12 && t < 15) { if (a.bga > 0.0) ms[BGA + t - 12] *= ssc[3]; }
                }
                wave_sync_lds();
                if (s0 == 0 && sl == 0) PHASE_STAMP(5);
            }
        }
        __syncthreads();
        PHASE_STAMP(13);
        // ---- phase 2: dR, F and L of every live sample of the chunk, one element per lane and pass, the reference's expressions ----
        for (int i = t; i < ns * INER * INER; i += 256) Fs[i] = ((i % (INER * INER)) % (INER + 1) == 0) ? 1.0 : 0.0;
        for (int i = t; i < ns * INER * QD; i += 256) Ls[i] = 0.0;
        for (int w = t; w < ns * 36; w += 256) {                        // stage D: dR / dq
            const int sl = w / 36, e = w - 36 * sl;
            double *const sh = shs + sl * SHW;
            if (sh[X_LIVE] == 0.0) continue;
            const double q0 = sh[32], q1 = sh[33], q2 = sh[34], q3 = sh[35];
            const int k = e / 9, ij = e - 9 * k, i = ij / 3, j = ij - 3 * i;
            constexpr unsigned char IDX[4][9] = { {0,3,2, 3,0,1, 2,1,0}, {1,2,3, 2,1,0, 3,0,1}, {2,1,0, 1,2,3, 0,3,2}, {3,0,1, 0,3,2, 1,2,3} };
            constexpr signed char SGN[4][9] = { {1,-1,1, 1,1,-1, -1,1,1}, {1,1,1, 1,-1,-1, 1,1,-1}, {-1,1,1, 1,1,1, -1,1,-1}, {-1,-1,1, 1,-1,1, 1,1,1} };
            const int id = IDX[k][ij];
            const double qv = id == 0 ? q0 : id == 1 ? q1 : id == 2 ? q2 : q3;
            sh[49 + 9 * k + 3 * j + i] = SGN[k][ij] > 0 ? 2 * qv : -2 * qv;
        }
        __syncthreads();
        for (int w = t; w < ns * 64; w += 256) {                        // stage E: the entries of F and L that depend on R, dR, A only
            const int sl = w >> 6, tt = w & 63;
            double *const sh = shs + sl * SHW;
            if (sh[X_LIVE] == 0.0) continue;
            double *const F = Fs + sl * INER * INER, *const Lm = Ls + sl * INER * QD;
            const double *const sA = sh, *const sprevQ = sh + 36, *const sR = sh + 40, *const sdR = sh + 49, *const sTxab = sh + 85, *const sxa = sh + 100;
            double *const sT34 = sh + 88;
            const double dt = sh[X_DT];
            if (tt < 3) {
                const int i = tt;
                F_(POS + i, VEL + i) = dt;
                L_(BGA + i, Q_BGA_DRIFT + i) = 1.0; L_(BAA + i, Q_BAA_DRIFT + i) = 1.0;
            } else if (tt >= 4 && tt < 16) {
                const int e = tt - 4, k = e / 3, i = e - 3 * k;
                double s_ = 0; for (int j = 0; j < 3; j++) s_ += sdR[9 * k + 3 * i + j] * sTxab[j];
                sT34[3 * k + i] = s_ * dt;
            } else if (tt >= 16 && tt < 28) {
                const int e = tt - 16, g = e >> 2, i = e & 3;
                const double h = dt / 2;
                const double dS[3][16] = {
                    { 0, h, 0, 0,  -h, 0, 0, 0,  0, 0, 0, h,  0, 0, -h, 0 },
                    { 0, 0, h, 0,  0, 0, 0, -h,  -h, 0, 0, 0,  0, h, 0, 0 },
                    { 0, 0, 0, h,  0, 0, h, 0,  0, -h, 0, 0,  -h, 0, 0, 0 } };
                double t1[4];
#pragma unroll
                for (int ii = 0; ii < 4; ii++) {
                    double s_ = 0;
#pragma unroll
                    for (int j = 0; j < 4; j++) { const double d = g == 0 ? dS[0][4 * ii + j] : g == 1 ? dS[1][4 * ii + j] : dS[2][4 * ii + j]; s_ += d * sprevQ[j]; }
                    t1[ii] = s_;
                }
                double s_ = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) s_ += sA[4 * j + i] * t1[j];
                L_(ORI + i, Q_GYRO + g) = s_;
            } else if (tt >= 28 && tt < 37) {
                const int e = tt - 28, i = e / 3, j = e - 3 * i;
                L_(VEL + i, Q_ACC + j) = sR[3 * i + j] * dt;
                F_(VEL + i, BAA + j) = -sR[3 * i + j] * dt; F_(VEL + i, BAT + j) = sR[3 * i + j] * sxa[j] * dt;
            } else if (tt >= 40 && tt < 56) {
                const int e = tt - 40, i = e & 3, j = e >> 2;
                F_(ORI + i, ORI + j) = sA[4 * j + i];
            }
        }
        __syncthreads();
        for (int w = t; w < ns * 12; w += 256) {
            const int sl = w / 12, tt = w - 12 * sl;
            double *const sh = shs + sl * SHW;
            if (sh[X_LIVE] == 0.0) continue;
            double *const F = Fs + sl * INER * INER;
            const double *const sA = sh, *const sT34 = sh + 88;
            const int i = tt / 4, j = tt - 4 * i;
            double s_ = 0; for (int k = 0; k < 4; k++) s_ += sT34[3 * k + i] * sA[4 * j + k];
            F_(VEL + i, ORI + j) = s_;
        }
        __syncthreads();
        for (int w = t; w < ns * 32; w += 256) {
            const int sl = w >> 5, tt = w & 31;
            double *const sh = shs + sl * SHW;
            if (sh[X_LIVE] == 0.0) continue;
            double *const F = Fs + sl * INER * INER, *const Lm = Ls + sl * INER * QD;
            if (tt < 9) {
                const int i = tt / 3, g = tt - 3 * i;
                double s_ = 0; for (int k = 0; k < 4; k++) s_ += F_(VEL + i, ORI + k) * L_(ORI + k, Q_GYRO + g);
                L_(VEL + i, Q_GYRO + g) = s_;
                F_(VEL + i, BGA + g) = -s_;
            } else if (tt >= 16 && tt < 28) {
                const int e = tt - 16, i = e / 3, g = e - 3 * i;
                F_(ORI + i, BGA + g) = -L_(ORI + i, Q_GYRO + g);
            }
        }
        if (s0 == 0) PHASE_STAMP(6);
        // ---- phase 3: P00 = F P00 F' + L Q L' (ekf.cpp:504-505), Phi <- F Phi, sample by sample (see ekf_predict_kernel) ----
        int last_live = -1;
        bool q_set = false;
        // the drift variances of Q (ekf.cpp:397-412) of one sample: Qs is read by the first product phase of a sample only
        auto set_q = [&](const double *sh_q) {
            if (a.baa > 0.0 && t < 9) { const int i = t % 3, j = t / 3; Qs[(Q_BAA_DRIFT + j) * QD + Q_BAA_DRIFT + i] = (i == j) ? sh_q[X_VBAA] : 0.0; }
            if (a.bga > 0.0 && t >= 16 && t < 25) { const int e = t - 16, i = e % 3, j = e / 3; Qs[(Q_BGA_DRIFT + j) * QD + Q_BGA_DRIFT + i] = (i == j) ? sh_q[X_VBGA] : 0.0; }
        };
        for (int sl = 0; sl < ns; sl++) {
            double *const sh = shs + sl * SHW;
            __syncthreads();                                     // (F, L of the chunk; the previous sample's P00 and Phi)
            if (sh[X_LIVE] == 0.0) continue;                     // uniform
            last_live = sl;
            const double *const F = Fs + sl * INER * INER, *const Lm = Ls + sl * INER * QD;
            if (!q_set) { set_q(sh); __syncthreads(); }           // (the chunk's first live sample; the others: behind the previous one's middle barrier)
            q_set = false;
            if (s0 == 0 && sl == 1) PHASE_STAMP(7);
            const int ti = wave & 1, tj = wave >> 1;                 // output rows 16 ti .., columns 16 tj ..
            const int mi = ti ? INER - 16 : 16, nj = tj ? INER - 16 : 16;
            const double4v fp = mfma_tile<5>(F + 16 * ti, 1, INER, mi, P00 + 16 * tj * INER, 1, INER, nj, INER);
            const double4v ph = mfma_tile<5>(F + 16 * ti, 1, INER, mi, Phi + 16 * tj * INER, 1, INER, nj, INER);
            double4v lq = {0.0, 0.0, 0.0, 0.0};
            if (wave < 2) lq = mfma_tile<3>(Lm + 16 * wave, 1, INER, wave ? INER - 16 : 16, Qs, 1, QD, QD, QD);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int r = kq + 4 * q;
                if (r < mi && cl < nj) { FP[(16 * tj + cl) * INER + 16 * ti + r] = fp[q]; PhiN[(16 * tj + cl) * INER + 16 * ti + r] = ph[q]; }
                if (wave < 2 && r < (wave ? INER - 16 : 16) && cl < QD) LQ[cl * INER + 16 * wave + r] = lq[q];
            }
            if (s0 == 0 && sl == 1) PHASE_STAMP(8);
            __syncthreads();
            if (s0 == 0 && sl == 1) PHASE_STAMP(9);
            {   // the next live sample's Q entries (uniform search)
                int nx = sl + 1;
                while (nx < ns && shs[nx * SHW + X_LIVE] == 0.0) nx++;
                if (nx < ns) { set_q(shs + nx * SHW); q_set = true; }
            }
            const double4v p1 = mfma_tile<5>(FP + 16 * ti, 1, INER, mi, F + 16 * tj, INER, 1, nj, INER);
            const double4v p2 = mfma_tile<3>(LQ + 16 * ti, 1, INER, mi, Lm + 16 * tj, INER, 1, nj, QD);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int r = kq + 4 * q;
                if (r < mi && cl < nj) P00[(16 * tj + cl) * INER + 16 * ti + r] = p1[q] + p2[q];
            }
            for (int e = t; e < INER * INER; e += 256) Phi[e] = PhiN[e];
            if (s0 == 0 && sl == 1) PHASE_STAMP(10);
        }
        __syncthreads();
        if (s0 == 0) PHASE_STAMP(11);
        if (last_live >= 0)                                       // der_predict reads the LAST sample's F (ekf_predict_kernel: F after its loop)
            for (int i = t; i < INER * INER; i += 256) a.dydx[(size_t)b * INER * INER + i] = Fs[last_live * INER * INER + i];
        __syncthreads();                                          // (the next chunk overwrites the stage values, F and L)
    }
    for (int i = t; i < INER * INER; i += 256) P[(size_t)(i / INER) * n + (i % INER)] = P00[i];
    for (int i = t; i < QD * QD; i += 256) Q[i] = Qs[i];
    if (t < INER) m[t] = ms[t];
    PHASE_STAMP(14);
    {
        double f0[5], f1[5];
#pragma unroll
        for (int sx = 0; sx < 5; sx++) {
            const int k = 4 * sx + kq;                                                        // < 20
            f0[sx] = Phi[k * INER + cl];
            f1[sx] = Phi[k * INER + min(16 + cl, INER - 1)];
        }
        for (int base = 0; base < 2 * tiles; base += 4 * NIT) {
#pragma unroll
            for (int u = 0; u < NIT; u++) {
                const int it = base + wave + 4 * u;
                if (it < 2 * tiles) {
                    if (base > 0) {
#pragma unroll
                        for (int sx = 0; sx < 5; sx++) slab[u][sx] = *slab_ptr(it, sx);
                    }
                    double4v a0 = {0.0, 0.0, 0.0, 0.0}, a1 = a0;
                    const bool p10 = it < tiles;
#pragma unroll
                    for (int sx = 0; sx < 5; sx++) {
                        const double x0 = p10 ? f0[sx] : slab[u][sx], y0 = p10 ? slab[u][sx] : f0[sx];
                        const double x1 = p10 ? f1[sx] : slab[u][sx], y1 = p10 ? slab[u][sx] : f1[sx];
                        a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, y0, a0, 0, 0, 0);
                        a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, y1, a1, 0, 0, 0);
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int rr = kq + 4 * q;                                            // output row within the tile
                        if (p10) {
                            const int i = INER + 16 * it + cl;                                // (c = rr [+16], i)
                            if (i < n) {
                                P[(size_t)rr * n + i] = a0[q];
                                if (16 + rr < INER) P[(size_t)(16 + rr) * n + i] = a1[q];
                            }
                        } else {
                            const int c = INER + 16 * (it - tiles) + rr;                      // (c, r = cl [+16])
                            if (c < n) {
                                P[(size_t)c * n + cl] = a0[q];
                                if (16 + cl < INER) P[(size_t)c * n + 16 + cl] = a1[q];
                            }
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    PHASE_STAMP(15);
}

// ---------------------------------------------------------------------------------------------
// update / gate (ekf.cpp:57-82, 760-844)
// ---------------------------------------------------------------------------------------------
struct UpdateArgs {
    int n, nr, l, R, Rs;              // R = nr + n + 1 rows of the tall matrix; Rs = its column stride
    int mode;                         // 0 gate only, 1 update, 2 update only if the chi2 gate passes
    int generic;                      // residual = y - H m[0:l] (ekf.cpp:76-79) instead of the given v
    int normalize_all, use_lds, map_dim;
    double *m, *P;
    const double *H, *v;              // per filter: nr*l column-major, nr
    const double *rdiag;              // per filter diagonal of R (already scaled), or null -> rd0
    double rd0, noise_scale;
    double rd1;                       // mode 3 only: R of the update (rd0 is then the R of the gate)
    double *ws;                       // per filter R*nr doubles (used when the tall matrix exceeds LDS)
    double *chi2; int *status;        // optional outputs
    const unsigned char *active;      // optional per-filter enable
    const int *require_inlier;        // optional per-filter gate result of an earlier launch: run only where it is 0 (INLIER)
    int *success_counter;             // optional per-filter count of applied visual updates (updateSuccessCount, backend.cpp:1183)
    // speculative frame loop (small batches, hv_ekf_visual_frame_dev): inputs / outputs are [n_tracks][batch] records
    //   spec 1: grid (batch, n_tracks), chi2 gate of EVERY pending track (index >= cursor[filter]) against the current (m, P)
    //   spec 2: grid (batch): the first pending track whose gate said INLIER is applied (mode 1), cursor moves behind it
    //   spec 3: spec 1 and spec 2 in ONE launch (mode 3, grid (batch, n_tracks)): every pending track is gated; an inlier then waits
    //           for the gate results of the pending tracks in front of it (they belong to workgroups with a smaller linear index:
    //           dispatched earlier, so the wait cannot deadlock) and, if none of them is an inlier, carries on into the update with
    //           the H P it already holds. The workgroup of the last track closes the pass when nobody applied anything.
    int spec, n_tracks, max_successful;
    int *cursor;                      // [batch] first track of the filter that is not final yet
    const int *gate_in;               // spec 2: [n_tracks][batch] gate results of spec 1 (a.status stays free for this launch's own output)
    const int *nr_rec;                // ragged batches: rows of every record (<= nr, which is then the record stride of H and v; 0: none)
    int *cursor_out;                  // spec 3: the cursor after this pass (ping-pong: late workgroups still read the old one)
    int *pub;                         // spec 3: [n_tracks][batch] published gate decisions, pass_id * 4 + {1 not applicable, 2 inlier}
    int pass_id;                      // spec 3: > 0, distinct per pass of a frame (pub is zeroed per frame)
    int *err;                         // spec 3: device error word of the filter batch (bit 0: a hand-shake wait timed out)
    // compact Jacobian written by the fused prepare + gate kernel (VuPrepareArgs::fused): column u of a record is state column
    // acol[u]; the record holds na = 7 * (rows / (2 ncam)) + 1 columns with the record's row count as leading dimension. MODE 2 only.
    const int *acol;                  // [records][na_max] or null (dense H)
    int na_max, ncam;
    size_t h_stride;                  // doubles between the H records
    int v_stride;                     // doubles between the v records (= nr unless the launch serves one length class of a longer-strided batch)
    // Long tracks (49 .. 96 rows: 13 .. 21 stereo poses) as TWO sequential block updates of at most 48 rows each, which is the same
    // posterior (the blocks' measurement noises are independent: R = r^2 I, ekf.cpp:771) and keeps every update on the P-resident MODE 2
    // kernel: half 1 = the first h1 = 2 ceil(rows / 4) rows (the first camera's), half 2 = the rest (the second camera's) with its
    // innovation corrected by the first block's mean step, v2 - H2 dm1. Half 1 leaves dm1 in dm_out and skips the quaternion
    // normalisation; half 2 reads it (dm_in) and normalises. 0 = the whole record in one launch. Compact H, MODE 2 only.
    int half, nr_full;                // nr_full: rows of the whole record when neither nr_rec nor nr says so (uniform long tracks)
    double *dm_out; const double *dm_in;   // [batch][n]
    // half 1 only: the visit's gate statuses. A block 1 that meets a non-positive pivot applies nothing and turns its record's status
    // into CHI2 -- what every other mode reports for a broken factorisation --, so that block 2 (require_inlier) skips the record
    // instead of applying half an update on a stale dm_in (r03 advisor)
    int *gate_rw;
    // speculative frame loop over LONG records (spec 2 with half 1 / 2, r04): the record a filter applies is chosen by the scan of the
    // half-1 launch; `half_auto` makes the block split a per-record decision -- a record of at most 48 rows is applied whole by the
    // half-1 launch (normalisation, success count and cursor included) and skipped by the half-2 launch, a longer one takes both --,
    // and sel_io [batch] carries the chosen track of a long record (-1: none) from the half-1 launch to the half-2 launch, which
    // must not scan again: the first launch may have moved the cursor or turned the record's gate status into CHI2
    int half_auto; int *sel_io;
    // half_auto: the epochs of the frame's records, [n_tracks][batch] (VuPrepareArgs::epoch). A long record whose block 1 was applied and
    // whose block 2 then meets a non-positive pivot leaves (m, P) changed without a counted success: the filter's pending records are
    // marked "never prepared" (-1) so that the next pass prepares them against the state as it is now (r04 advisor)
    int *epoch;
    int batch;
    const int *rec_count, *rec_list;  // compaction list (VuPrepareArgs): workgroup i updates filter rec_list[i], i < *rec_count; the others exit
};

// spec 3 hand-shake between the workgroups of one filter (agent scope: they run on different CUs)
__device__ __forceinline__ void spec_publish(const UpdateArgs &a, int rec, int code)
{
    __hip_atomic_store(a.pub + rec, a.pass_id * 4 + code, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
// decision of record `rec` in this pass; bounded spin (0.2 s): a decision that never arrives is reported as -1
__device__ __forceinline__ int spec_wait(const UpdateArgs &a, int rec)
{
    for (int spin = 0; spin < (1 << 20); ++spin) {
        const int v = __hip_atomic_load(a.pub + rec, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if ((v >> 2) == a.pass_id) return v & 3;
        __builtin_amdgcn_s_sleep(8);
    }
    // never silently: the frame's result is then NOT the sequential loop's (a.err is read by hv_ekf_frame_error / the host-pointer entry points)
    if (a.err) atomicOr(a.err, 1);
    return -1;
}
// thread 0 of the workgroup of the LAST track, when that workgroup applies nothing: if no pending track of the filter was an
// inlier, nobody else moves the cursor -- every pending status is final (or the pass did not run: quota used up)
__device__ __forceinline__ void spec_close(const UpdateArgs &a, int b, int c0, bool pass_ran)
{
    bool any = false;
    for (int jj = c0; jj < a.n_tracks - 1 && !any; ++jj) any = spec_wait(a, jj * (int)gridDim.x + b) == 2;
    if (!any) a.cursor_out[b] = pass_ran ? a.n_tracks : c0;
}

constexpr int UPD_THREADS = 512;   // 8 waves = 2 per SIMD: 256 VGPRs each (whole column blocks of P stay in registers)

// MODE 0: T in the global workspace (tall matrix larger than LDS)
// MODE 1: T in LDS, H streamed from L2
// MODE 2: T and H in LDS (n <= 160, nr <= 48): K-split products, P read from HBM exactly once
// TI (MODE 2 only): 16-row tiles of H, nr <= 16 TI: a compile-time count keeps the MFMA loops free of
// branches (a uniform branch per tile made hipcc wait for each LDS operand right before its MFMA).
// AUTO: the half_auto form of the speculative loop over long records (its own kernel: the other instantiations keep their registers)
template <int MODE, int TI, bool AUTO = false>
__device__ __forceinline__ void ekf_update_body(const UpdateArgs &a, const int b_in /* filter: blockIdx.x, or an entry of a compaction list */)
{
    // (a list entry is a per-lane load: on the scalar unit the filter's base addresses are uniform and its gathers become scalar base +
    //  32-bit lane offset -- one VGPR and one VALU instruction per request instead of a 64-bit multiply-add pair)
    const int b = __builtin_amdgcn_readfirstlane(b_in);
    constexpr bool USE_LDS = MODE >= 1;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    int e = b;                                             // record of this workgroup's H, v, active, chi2, status
    int sel = -1;
    if (a.spec == 1) {
        const int j = blockIdx.y;
        if (j < a.cursor[b] || a.success_counter[b] >= a.max_successful) return;
        e = j * (int)gridDim.x + b;
    } else if (AUTO && a.spec == 2 && a.half == 2) {
        // second block of the long record the half-1 launch chose for this filter (if any)
        sel = a.sel_io[b];
        if (sel < 0) return;
        e = sel * (int)gridDim.x + b;
        if (a.gate_in[e] != 0) {                           // block 1 met a non-positive pivot (status CHI2 now): nothing applied, the track is final
            if (threadIdx.x == 0) a.cursor[b] = sel + 1;
            return;
        }
    } else if (a.spec == 2) {
        // every thread runs the same short scan (uniform): the first pending track that passed its gate
        const int c0 = a.cursor[b];
        if (AUTO && threadIdx.x == 0) a.sel_io[b] = -1;      // (thread 0 also writes the choice below: program order)
        if (c0 >= a.n_tracks || a.success_counter[b] >= a.max_successful) return;
        for (int j = c0; j < a.n_tracks && sel < 0; ++j) {
            const int ee = j * (int)gridDim.x + b;
            if (a.active[ee] && a.gate_in[ee] == 0) sel = j;
        }
        if (sel < 0) {                                     // nothing applicable is left: every pending status is final
            __syncthreads();
            if (threadIdx.x == 0) a.cursor[b] = a.n_tracks;
            return;
        }
        e = sel * (int)gridDim.x + b;
    }
    int c0_spec = 0;
    if (a.spec == 3) {
        const int j = blockIdx.y;
        c0_spec = a.cursor[b];
        e = j * (int)gridDim.x + b;
        const bool pass_runs = c0_spec < a.n_tracks && a.success_counter[b] < a.max_successful;
        if (!pass_runs || j < c0_spec || !a.active[e]) {      // nothing to gate here: still publish, and close the pass if last
            if (threadIdx.x == 0) {
                spec_publish(a, e, 1);
                if (j == a.n_tracks - 1) spec_close(a, b, c0_spec, pass_runs);
            }
            return;
        }
    }
    // The record's flags and its shape are requested TOGETHER: as a sequence of tests each of them was
    // a dependent HBM / L2 round trip of its own -- 15 k cycles went by before the first request for H was issued (r03 phase stamps)
    const int t = threadIdx.x, lane = t & 63;
    const unsigned char act_v = a.active ? a.active[e] : (unsigned char)1;
    const int req_v = a.require_inlier ? a.require_inlier[b] : 0;
    const int nr_rec_v0 = a.nr_rec ? a.nr_rec[e] : a.nr_full;
    int shape_pin = nr_rec_v0;
    asm volatile("" : "+v"(shape_pin));                     // (keeps the three requests in front of the first test)
    const int nr_rec_v = shape_pin;
    if (!act_v) return;
    if (req_v != 0) return;
#ifdef HV_DEBUG_SKIP_UPDATE
    // experiment only (scripts/lanes_probe.py, never in the shipped library): what do the update workgroups cost a step? An applied
    // update counts as a success and leaves (m, P) as they are
    if (a.mode == 1 && a.spec == 0) { if (a.success_counter && t == 0) a.success_counter[b] += 1; return; }
#endif
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);     // wave-uniform: tile indices and their addresses stay on the scalar unit
    constexpr int nwaves = UPD_THREADS / 64;
    const int n = a.n, l = a.l;
    int nr = a.nr, R = a.Rs, Rfull = a.R;                   // R is the column STRIDE of T below; Rfull rows are used
    int roff = 0, ld = a.nr;                               // first row of this launch's block inside the record; leading dimension of H
    int half = a.half;                                     // (half_auto: this record's own split, see UpdateArgs)
    if (a.nr_rec || a.half) {                              // ragged batch / block update: this record's own shape (uniform per workgroup)
        int nr_full = __builtin_amdgcn_readfirstlane(nr_rec_v);
        if (nr_full < 1 || nr_full > a.v_stride) return;    // no track (the prepare launch also cleared `active`)
        nr = nr_full; ld = nr_full;
        if constexpr (AUTO) {
            if (nr_full <= 48) {
                if (half == 2) return;
                half = 0;
            }
            if (half == 1 && t == 0) a.sel_io[b] = sel;
        }
        if (half) {
            if (MODE != 2) return;                         // (the host only asks the LDS-resident kernels for block updates)
            const int h1 = 2 * ((nr_full + 3) >> 2);
            roff = half == 2 ? h1 : 0;
            nr = half == 2 ? nr_full - h1 : h1;
        }
        if (nr < 1 || nr > a.nr) return;
        Rfull = nr + n + 1; R = Rfull;
        if (USE_LDS) R = lds_stride(R);
    }
    double *m = a.m + (size_t)b * n, *P = a.P + (size_t)b * n * n;
    const double *H = a.H + (size_t)e * a.h_stride;        // record stride: the launch's row count x columns; leading dimension: nr
    const double rd = a.rdiag ? a.rdiag[b] : a.rd0;
    // Tall matrix T (a.R rows x nr columns, column-major with stride R >= a.R: T(r, c) = T[c * R + r]; in LDS
    // the stride is padded to lds_stride):
    //   rows 0 .. nr-1   S = H P H' + R            -> L           (S = L L')
    //   row  nr          v'                        -> z' = (L^-1 v)'
    //   rows nr+1 ..     (H P)'  (n rows)          -> Y' = (L^-1 H P)'
    // One blocked Cholesky pass over T does the factorisation and both triangular solves. The gate
    // only needs rows 0 .. nr. All LDS comes from the dynamic region (keeps the base 16-byte aligned), carved as UpdateLds
    // says for this record's shape. USE_LDS is a template parameter so that the common case compiles to
    // ds_read / ds_write (a run-time select would turn every access into a flat load).
    const UpdateLds L = update_lds(R, nr, nwaves, USE_LDS, 0);
    double *T = USE_LDS ? smem + L.T : a.ws + (size_t)b * a.Rs * a.nr;
    double *W = smem + L.chol + CHOL_W, *col = smem + L.chol + CHOL_COL, *red = smem + L.red;
    int *s_stop = reinterpret_cast<int *>(smem + L.flag);
    double *Hs = smem + L.Hs;                     // MODE 2: H zero-padded to (16 TI) x (16 lb), column-major, stride nrp
    constexpr int nrp = 16 * (TI > 0 ? TI : 1);
    const bool gate_only = a.mode == 0;
    const int rv = nr, ry = nr + 1;
    // mode 3 (MODE 2 kernels only): visualTrackOutlierCheck with R = rd0, then -- where it passes -- updateVisualTrack with
    // R = rd1 on the SAME H P: S (without R) and v are parked in the H staging area after phase B, the gate runs the
    // Cholesky on the measurement rows only, and an inlier restores S + rd1 I and v and runs the full factorisation.
    const bool two_r = MODE == 2 && a.mode == 3;
    int Rlim = (gate_only || two_r) ? nr + 1 : Rfull;

    PHASE_STAMP(0);
    const int kq = lane >> 4, cl = lane & 15;      // MFMA lane coordinates: k sub-step / output row group, column
    // MODE 2 ownership: wavefront w owns the 16-column block J = w of P with all of its 16-row K
    // blocks ("item 0"); wavefronts 0..3 also own one K half of block 8 or 9 ("item 1": J = 8 + (w & 1),
    // half w >> 1), which gives every SIMD 2.5 column blocks of matrix work at n = 160. The four B
    // operands of a K block ARE the 16 x 16 tile P(K, J) in the MFMA C layout (lane (kq, c) holds
    // rows kq + 4 s), so the tiles fetched for H P stay in registers and serve as the old values of
    // P -= Y'Y: P crosses HBM once per update. All of a wave's P loads are issued before anything
    // else; K blocks are consumed in arrival order, so the HBM stream (~10 B/clk/CU when every CU
    // pulls at once) overlaps the MFMAs.
    constexpr int NBK = 10, NBH = 5;                // K blocks per column block / per half (n <= 160)
    double pres0[NBK][4], pres1[NBH][4];
    const int tiles_j = (n + 15) >> 4, lb = (l + 15) >> 4;
    const int hs = (tiles_j + 1) >> 1;
    const int J1 = 8 + (wave & 1), kb0_1 = (wave & 2) ? hs : 0, kb1_1 = (wave & 2) ? tiles_j : hs;
    const bool have0 = MODE == 2 && wave < tiles_j, have1 = MODE == 2 && wave < 4 && J1 < tiles_j;
    unsigned kbmask = 0xFFFFFFFFu;                  // K blocks of H P with matrix work (compact H: those that hold a non-zero column)
    if constexpr (MODE == 2) {
        // ---- A: HP = H * P[0:l, :] accumulated into rows ry.. of T (the two K halves of blocks 8, 9
        // meet through ds_add_f64 on the zeroed tile: two addends commute, the sum is reproducible) ----
        auto fetch_blk = [&](auto &pv, int bi, int J, int kb, int kend) {
            if (kb < kend && (kb < lb || !gate_only)) {
                const int jc = min(J * 16 + cl, n - 1);
#pragma unroll
                for (int sx = 0; sx < 4; sx++)
                    pv[bi][sx] = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(P) + (unsigned)(min(kb * 16 + 4 * sx + kq, n - 1) * n + jc) * 8u);
            }
        };
        // request order = arrival order: H first (every MFMA needs it), then the P tiles in the order
        // they are consumed. Only DEPTH K blocks are requested ahead of the MFMAs that use them: a
        // wave that queues its whole column block up front sits in the issue queue until most of it has
        // arrived, and the HBM stream no longer overlaps the matrix work.
        constexpr int HREG = (48 * 160 + UPD_THREADS - 1) / UPD_THREADS, DEPTH = 4;
        if (a.acol) {
            // compact H (fused prepare + gate): Hs is zeroed and the record's na x nr values are gathered BY COMPACT COLUMN and scattered
            // to their state columns -- the addresses of the gather do not depend on the column list, so Hc and the list travel
            // together: one HBM / L2 round trip, 8 values per thread at 11 stereo poses. (r03's first form built the inverse map
            // state column -> compact column in LDS first -- a dependent round trip and two barriers -- and walked all 48 x 160 cells
            // with 15 registers per thread.) kbmask: the 16-row K blocks of H P that hold a non-zero column of H at all.
            int *mask = reinterpret_cast<int *>(col);       // (the col scratch is free until the Cholesky)
            const int na = 7 * (ld / (2 * a.ncam)) + 1;     // (ld = rows of the whole record)
            const int *acol = a.acol + (size_t)e * a.na_max;
            const int total = na * nr;
            const unsigned inv_nr = (unsigned)((0x100000000ull + (unsigned)nr - 1) / (unsigned)nr);      // i / nr = umulhi(i, ceil(2^32 / nr)), i < 2^20
            constexpr int HC = 8;
            double hv[HC]; int hc[HC];
            auto request = [&](int base) {
#pragma unroll
                for (int u = 0; u < HC; u++) {
                    const int i = base + t + u * UPD_THREADS, uc = (int)__umulhi((unsigned)i, inv_nr), r = i - uc * nr;
                    const bool live = i < total;
                    hc[u] = live ? acol[uc] : -1;
                    hv[u] = live ? *reinterpret_cast<const double *>(reinterpret_cast<const char *>(H) + (unsigned)(uc * ld + roff + r) * 8u) : 0.0;
                }
            };
            auto scatter = [&](int base) {
#pragma unroll
                for (int u = 0; u < HC; u++) {
                    const int i = base + t + u * UPD_THREADS, uc = (int)__umulhi((unsigned)i, inv_nr), r = i - uc * nr;
                    if (hc[u] >= 0 && hc[u] < l) {
                        Hs[hc[u] * nrp + r] = hv[u];
                        if (r == 0) atomicOr(mask, 1 << (hc[u] >> 4));
                    }
                }
            };
            request(0);
            // The P tiles are requested BEHIND the gather, the block that is used last FIRST: the kernel sits at 255 VGPRs and the
            // register allocator spills one value of that block right behind its load, i.e. waits for it -- and loads return in order.
            // (r03's first form requested the tiles in front of the staging, block 0 first: the spill waited for all 16 of them,
            // 14 k cycles before the first request for H.)
#pragma unroll
            for (int bi = DEPTH - 1; bi >= 0; bi--) if (have0) fetch_blk(pres0, bi, wave, bi, tiles_j);     // (LAST block first: see below)
            PHASE_STAMP(8);
            for (int i = t; i < nrp * 16 * lb; i += UPD_THREADS) Hs[i] = 0.0;
            for (int i = t; i < R * nr; i += UPD_THREADS) T[i] = 0.0;
            if (t == 0) mask[0] = 0;
            __syncthreads();
            scatter(0);
            for (int base = HC * UPD_THREADS; base < total; base += HC * UPD_THREADS) { request(base); scatter(base); }     // (long mono tracks)
            __syncthreads();
            kbmask = (unsigned)mask[0];
        } else {
            double hreg[HREG];
#pragma unroll
            for (int u = 0; u < HREG; u++) {
                const int i = t + u * UPD_THREADS, k = i / nrp, r = i - k * nrp;
                hreg[u] = (i < nrp * 16 * lb && k < l && r < nr) ? H[(size_t)k * ld + roff + r] : 0.0;
            }
#pragma unroll
            for (int bi = 0; bi < DEPTH; bi++) if (have0) fetch_blk(pres0, bi, wave, bi, tiles_j);
            PHASE_STAMP(8);
            for (int i = t; i < R * nr; i += UPD_THREADS) T[i] = 0.0;
#pragma unroll
            for (int u = 0; u < HREG; u++) {
                const int i = t + u * UPD_THREADS;
                if (i < nrp * 16 * lb) Hs[i] = hreg[u];
            }
        }
        __syncthreads();
        PHASE_STAMP(9);
        const double *hbase = Hs + (size_t)kq * nrp + cl;
        // H operands of a K block: 4 k-steps x TI row tiles, double-buffered across blocks (the reads of
        // block b+1 are issued before the MFMAs of block b: a wavefront that only prefetches one or two
        // ds_reads ahead issues an MFMA every ~100 cycles instead of every 64)
        // (in HALF blocks of two k-steps: 2 x 2 x TI operand registers instead of 2 x 4 x TI -- the kernel sits at 255 VGPRs and the
        //  allocator took its last pair from the P prefetch, spilling a value right behind its load: a full stop in front of the staging)
        auto load_h = [&](int kb, int hf, double (&av)[2][TI]) {
#pragma unroll
            for (int sx = 0; sx < 2; sx++)
#pragma unroll
                for (int mt = 0; mt < TI; mt++) av[sx][mt] = hbase[(size_t)(kb * 16 + 4 * (2 * hf + sx)) * nrp + 16 * mt];
        };
        auto mfma_half = [&](auto &pv, int bi, int hf, const double (&av)[2][TI], double4v (&acc)[TI]) {
#pragma unroll
            for (int sx = 0; sx < 2; sx++)
#pragma unroll
                for (int mt = 0; mt < TI; mt++)
                    acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[sx][mt], pv[bi][2 * hf + sx], acc[mt], 0, 0, 0);
        };
        auto flush = [&](int J, double4v (&acc)[TI]) {
#pragma unroll
            for (int mt = 0; mt < TI; mt++) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int i = 16 * mt + kq + 4 * q, j = J * 16 + cl;
                    if (i < nr && j < n) unsafeAtomicAdd(&T[(size_t)i * R + ry + j], acc[mt][q]);
                }
            }
        };
        {
            double4v acc[TI];
#pragma unroll
            for (int mt = 0; mt < TI; mt++) acc[mt] = double4v{0.0, 0.0, 0.0, 0.0};
            const int nv = have0 ? min(tiles_j, lb) : 0;                   // K blocks with matrix work: 0 .. nv-1
            double av[2][2][TI];
            if (nv > 0) load_h(0, 0, av[0]);
#pragma unroll
            for (int bi = 0; bi < NBK; bi++) {
                if (bi + DEPTH < NBK) { if (have0) fetch_blk(pres0, bi + DEPTH, wave, bi + DEPTH, tiles_j); }
                else if (bi + DEPTH - NBK < NBH) { if (have1) fetch_blk(pres1, bi + DEPTH - NBK, J1, kb0_1 + bi + DEPTH - NBK, kb1_1); }
                if (bi < nv) {
                    const bool work = (kbmask >> bi) & 1;
                    load_h(bi, 1, av[1]);
                    if (work) mfma_half(pres0, bi, 0, av[0], acc);
                    if (bi + 1 < nv) load_h(bi + 1, 0, av[0]);
                    if (work) mfma_half(pres0, bi, 1, av[1], acc);
                }
            }
            if (have0) flush(wave, acc);
        }
        PHASE_STAMP(10);
        {
            double4v acc[TI];
#pragma unroll
            for (int mt = 0; mt < TI; mt++) acc[mt] = double4v{0.0, 0.0, 0.0, 0.0};
            const int nv = have1 ? max(min(kb1_1, lb) - kb0_1, 0) : 0;     // blocks kb0_1 .. kb0_1 + nv - 1
            double av[2][2][TI];
            if (nv > 0) load_h(kb0_1, 0, av[0]);
#pragma unroll
            for (int bi = 0; bi < NBH; bi++) {
                if (bi + DEPTH < NBH) { if (have1) fetch_blk(pres1, bi + DEPTH, J1, kb0_1 + bi + DEPTH, kb1_1); }
                if (bi < nv) {
                    const bool work = (kbmask >> (kb0_1 + bi)) & 1;
                    load_h(kb0_1 + bi, 1, av[1]);
                    if (work) mfma_half(pres1, bi, 0, av[0], acc);
                    if (bi + 1 < nv) load_h(kb0_1 + bi + 1, 0, av[0]);
                    if (work) mfma_half(pres1, bi, 1, av[1], acc);
                }
            }
            if (have1) flush(J1, acc);
        }
        PHASE_STAMP(11);
    } else {
        // ---- A: HP = H * P[0:l, :], stored transposed as rows ry .. ry+n-1 of T; residual row ----
        const int tiles_i = (nr + 15) / 16;
        for (int tile = wave; tile < tiles_i * tiles_j; tile += nwaves) {
            const int i0 = (tile % tiles_i) * 16, j0 = (tile / tiles_i) * 16;
            // A(i, k) = H(i0+i, k) = H[k*nr + i0+i];  B(k, j) = P(k, j0+j), read as P(j0+j, k) = P[k*n + j0+j]:
            // P is symmetric to rounding (predict builds P01/P10 separately, every other step keeps or
            // restores symmetry) and the transposed element is unit-stride across the 16 lanes of a k-row
            const double4v acc = mfma_tile<8>(H + i0, 1, nr, nr - i0, P + j0, n, 1, n - j0, l);
            const int j = j0 + cl;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int i = i0 + kq + 4 * q;
                if (i < nr && j < n) T[(size_t)i * R + ry + j] = acc[q];
            }
        }
    }
    for (int i = t; i < nr; i += UPD_THREADS) {
        double r = a.v[(size_t)e * a.v_stride + roff + i];
        if (a.generic) { double s = 0; for (int k = 0; k < l; k++) s += H[(size_t)k * nr + i] * m[k]; r -= s; }
        if constexpr (MODE == 2) {
            if (a.dm_in) {                                 // second block of a long track: v2 - H2 dm1 (Hs: the staged, zero-padded H of this block)
                const double *dm = a.dm_in + (size_t)b * n;
                double s = 0;
                for (int k = 0; k < l; k++) s += Hs[(size_t)k * nrp + i] * dm[k];
                r -= s;
            }
        }
        T[(size_t)i * R + rv] = r;
    }
    __syncthreads();

    PHASE_STAMP(1);
    // ---- B: S = HP[:, 0:l] * H' + R (lower triangle), rows 0 .. nr-1 of T ----
    {
        const int tb = (nr + 15) / 16;
        if constexpr (MODE == 2) {
            // (tile, K half) items, the halves combined with ds_add_f64 into the zeroed S block
            const int khalf = ((l / 2) + 15) & ~15;
            for (int it = wave; it < tb * (tb + 1); it += nwaves) {             // lower tiles only, two halves each
                const int hh = it & 1;
                int ib = it >> 1, cb = 0;
                while (ib >= tb - cb) { ib -= tb - cb; cb++; }                   // column cb holds tiles ib = cb .. tb-1
                ib += cb;
                const int i0 = ib * 16, c0 = cb * 16;
                const int kbeg = hh ? min(khalf, l) : 0, klen = hh ? l - kbeg : min(khalf, l);
                if (klen <= 0) continue;
                // A(i, k) = HP(i0+i, k) = T[(i0+i)*R + ry + k];  B(k, c) = H(c0+c, k) = Hs[k*nrp + c0+c]
                // (Hs is zero beyond k = l and c = nr; rows i >= nr are clamped and never stored)
                const double *pa = T + (size_t)min(i0 + cl, nr - 1) * R + ry + kbeg + kq;
                const double *pb = Hs + (size_t)(kbeg + kq) * nrp + c0 + cl;
                double4v acc = {0.0, 0.0, 0.0, 0.0};
                for (int k0 = 0; k0 < klen; k0 += 32) {          // 8 k-steps per trip, all 16 operands requested first
                    double av[8], bv[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        const bool live = k0 + 4 * u < klen;             // a partial last step meets the zero padding of Hs
                        const int kk = live ? k0 + 4 * u : 0;
                        av[u] = pa[kk]; bv[u] = pb[(size_t)kk * nrp];
                        if (!live) bv[u] = 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < 8; u++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
                }
                const int c = c0 + cl;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int i = i0 + kq + 4 * q;
                    if (i < nr && c < nr) unsafeAtomicAdd(&T[(size_t)c * R + i], acc[q] + ((i == c && hh == 0) ? rd : 0.0));
                }
            }
        } else {
            for (int tile = wave; tile < tb * tb; tile += nwaves) {
                const int ib = tile % tb, cb = tile / tb;
                if (ib < cb) continue;
                const int i0 = ib * 16, c0 = cb * 16;
                // A(i, k) = HP(i0+i, k) = T[(i0+i)*R + ry + k];  B(k, c) = H(c0+c, k) = H[k*nr + c0+c]
                const double4v acc = mfma_tile<8>(T + (size_t)i0 * R + ry, R, 1, nr - i0, H + c0, nr, 1, nr - c0, l);
                const int c = c0 + cl;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int i = i0 + kq + 4 * q;
                    if (i < nr && c < nr) T[(size_t)c * R + i] = acc[q] + (i == c ? rd : 0.0);
                }
            }
        }
    }
    __syncthreads();
    if constexpr (MODE == 2) {
        if (two_r) {                                          // Hs is dead after phase B: (nr + 1) x nr doubles fit (nrp x 16 lb >= that)
            // (+ 256: slack after the header area)
            for (int e = t; e < (nr + 1) * nr; e += UPD_THREADS) { const int c = e / (nr + 1), i = e - c * (nr + 1); Hs[256 + e] = T[(size_t)c * R + i]; }
            __syncthreads();
        }
    }

    PHASE_STAMP(2);
    for (int pass = 0; pass < (two_r ? 2 : 1); ++pass) {
    // ---- C: blocked left-looking Cholesky of the tall matrix, 16 columns per block, 3 barriers per
    // block (a column-at-a-time version needs one barrier + one LDS round trip + one rsqrt per COLUMN
    // on the critical path of all 16 waves: 1.3-1.7 k cycles per column measured). Per block j:
    //   U  every 16-row tile of block column j -= T(tile, 0:j0) * T(j0:j0+16, 0:j0)'         (MFMA)
    //   D  wave 0 factors the diagonal block in registers and inverts the factor   (factor_diag_block)
    //   P  every tile below the diagonal block *= Linv'                                       (MFMA)
    // Multiplying by the explicit inverse of a 16 x 16 diagonal block instead of substituting is the
    // usual blocked-TRSM trade: the error grows with cond(L_jj), not cond(L).
    for (int j0 = 0; j0 < nr; j0 += 16) {
        const int w = min(16, nr - j0);
        const int ntile = (Rlim - j0 + 15) / 16;
        const int i_l = lane >> 4, c_l = lane & 15;
        if (j0 > 0) {
            for (int tile = wave; tile < ntile; tile += nwaves) {
                const int i0 = j0 + 16 * tile, mi = Rlim - i0;
                // A(i, k) = T(i0+i, k) = T[k*R + i0+i];  B(k, c) = T(j0+c, k) = T[k*R + j0+c]
                const double4v acc = mfma_tile(T + i0, 1, R, mi, T + j0, R, 1, w, j0);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int i = i_l + 4 * q;
                    if (i < mi && c_l < w) T[(size_t)(j0 + c_l) * R + i0 + i] -= acc[q];
                }
            }
            __syncthreads();
        }
        if (j0 == 0) PHASE_STAMP(6);
        if (wave == 0) { if (w <= 8) factor_diag_block<8>(T, W, col, R, j0, w, lane); else factor_diag_block<16>(T, W, col, R, j0, w, lane); }
        __syncthreads();
        if (j0 == 0) PHASE_STAMP(7);
        for (int i0 = j0 + w + 16 * wave; i0 < Rlim; i0 += 16 * nwaves) {        // rows below the w x w diagonal block
            const int mi = Rlim - i0;
            // A(i, k) = T(i0+i, j0+k) = T[(j0+k)*R + i0+i];  B(k, c) = Linv(c, k) = W[k*16 + c]
            const double4v acc = mfma_tile(T + (size_t)j0 * R + i0, 1, R, mi, W, 16, 1, 16, w);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int i = i_l + 4 * q;
                if (i < mi && c_l < w) T[(size_t)(j0 + c_l) * R + i0 + i] = acc[q];
            }
        }
        __syncthreads();
    }

    PHASE_STAMP(3);
    // ---- D: chi2 = noise_scale * z'z ----
    {
        double s = 0;
        for (int c = t; c < nr; c += UPD_THREADS) { const double z = T[(size_t)c * R + rv]; s += z * z; }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        if (t == 0) {
            double tot = 0; for (int w2 = 0; w2 < nwaves; w2++) tot += red[w2];
            tot *= a.noise_scale;
            // A non-positive pivot (S not positive definite: r = 0 with a rank-deficient H) leaves NaN / inf in z: such a filter is
            // reported as CHI2 and left untouched in EVERY mode, where the reference's pivoted LDLT would carry on (r01 advisor)
            const bool broken = !(tot < 1e300);
            const int outlier = broken || ((nr < HV_CHI2INV95_N) ? (tot > d_chi2inv95[nr]) : 0);
            if (pass == 0) {
                if (a.chi2) a.chi2[e] = tot;
                if (a.status) a.status[e] = outlier ? 3 /*CHI2*/ : 0 /*INLIER*/;
            }
            *s_stop = (a.mode == 0) || broken || ((a.mode == 2 || (two_r && pass == 0)) && outlier);
            if (broken && a.gate_rw) a.gate_rw[e] = 3 /*CHI2*/;
            if (AUTO && broken && a.spec == 2 && half != 1) a.cursor[b] = sel + 1;     // (whole short record or block 2: not applied, the track is final)
            if (AUTO && broken && a.spec == 2 && half == 2 && a.epoch)                 // block 1 of this record HAS been applied
                for (int jj = sel + 1; jj < a.n_tracks; ++jj) a.epoch[jj * (int)gridDim.x + b] = -1;
            if (a.spec == 3 && pass == 0) {
                const int j = blockIdx.y;
                spec_publish(a, e, outlier ? 1 : 2);
                if (!outlier) {                               // first inlier in visit order applies; the others are re-examined next pass
                    bool lose = false;
                    for (int jj = c0_spec; jj < j && !lose; ++jj) lose = spec_wait(a, jj * (int)gridDim.x + b) != 1;
                    if (lose) *s_stop = 1;
                }
                if (*s_stop && j == a.n_tracks - 1 && outlier) spec_close(a, b, c0_spec, true);
            }
            // the applying workgroup met a non-positive pivot in the second factorisation: nothing is applied, the track is final
            if (a.spec == 3 && pass == 1 && *s_stop) a.cursor_out[b] = (int)blockIdx.y + 1;
        }
        __syncthreads();
        if (*s_stop) return;
    }
    if constexpr (MODE == 2) {
        if (two_r && pass == 0) {                             // inlier: S + rd1 I and v back, then the full factorisation
            const double shift = a.rd1 - rd;
            for (int e = t; e < (nr + 1) * nr; e += UPD_THREADS) {
                const int c = e / (nr + 1), i = e - c * (nr + 1);
                T[(size_t)c * R + i] = Hs[256 + e] + (i == c ? shift : 0.0);
            }
            Rlim = Rfull;
            __syncthreads();
        }
    }
    }   // pass

    PHASE_STAMP(4);
    // ---- E: m += Y' z ----
    for (int j = t; j < n; j += UPD_THREADS) {
        double s = 0;
        for (int c = 0; c < nr; c++) s += T[(size_t)c * R + ry + j] * T[(size_t)c * R + rv];
        m[j] += s;
        if (a.dm_out && !(AUTO && half == 0)) a.dm_out[(size_t)b * n + j] = s;
    }
    // ---- F: P -= Y' Y ----
    if constexpr (MODE == 2) {
        // tiles P(K, J) of the wave's items; old values are the registers filled in phase A
        auto down_item = [&](auto &pv, int nblk, int J, int kb0, int kb1) {
            const int jc = min(J * 16 + cl, n - 1);
            // B(c, j) = Y(c, J*16 + j) = T[c*R + ry + J*16 + j], c = 4 s + kq: shared by all tiles of the item
            constexpr int KS = 4 * TI;              // k-steps over the nr <= 16 TI rows of Y (zero beyond nr)
            double yj[KS];
#pragma unroll
            for (int sx = 0; sx < KS; sx++) {
                const int c = 4 * sx + kq;
                const double y = T[(size_t)min(c, nr - 1) * R + ry + jc];
                yj[sx] = c < nr ? y : 0.0;
            }
#pragma unroll
            for (int bi = 0; bi < nblk; bi++) {
                const int kb = kb0 + bi;
                if (kb < kb1) {
                    // A(i, c) = Y(c, kb*16 + i) = T[c*R + ry + kb*16 + i]; rows c >= nr meet yj = 0
                    const int ic = min(kb * 16 + cl, n - 1);
                    double av[KS];
#pragma unroll
                    for (int sx = 0; sx < KS; sx++) av[sx] = T[(size_t)min(4 * sx + kq, nr - 1) * R + ry + ic];
                    double4v acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int sx = 0; sx < KS; sx++) {
                        // only the last tile of rows can be (partly) empty: skip whole k-steps beyond nr
                        if (sx < KS - 4 || 4 * sx < nr) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[sx], yj[sx], acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int i = kb * 16 + kq + 4 * q, j = J * 16 + cl;
                        if (i < n && j < n) P[(size_t)i * n + j] = pv[bi][q] - acc[q];
                    }
                }
            }
        };
        if (have0) down_item(pres0, NBK, wave, 0, tiles_j);
        if (have1) down_item(pres1, NBH, J1, kb0_1, kb1_1);
    } else {
        // Y'Y is symmetric: entry (i, j) of a tile is applied to element (j, i), so the 16 lanes of a
        // row group touch 16 consecutive doubles. The old values of the NEXT tile are requested before
        // the MFMA loop of the current one: the ~1 us HBM round trip of P hides behind the matrix work
        // instead of stalling every tile.
        const int tb = (n + 15) / 16, ntiles = tb * tb;
        const int cj = lane & 15, ri = lane >> 4;
        auto p_addr = [&](int tile, int q) -> double * {
            const int i = min((tile % tb) * 16 + ri + 4 * q, n - 1), j = min((tile / tb) * 16 + cj, n - 1);
            return P + (size_t)i * n + j;
        };
        double cur[4], nxt[4] = {0.0, 0.0, 0.0, 0.0};
        if (wave < ntiles) {
#pragma unroll
            for (int q = 0; q < 4; q++) cur[q] = *p_addr(wave, q);
        }
        for (int tile = wave; tile < ntiles; tile += nwaves) {
            const int i0 = (tile % tb) * 16, j0 = (tile / tb) * 16;
            const int tn = min(tile + nwaves, ntiles - 1);
#pragma unroll
            for (int q = 0; q < 4; q++) nxt[q] = *p_addr(tn, q);
            // A(i, c) = Y(c, i0+i) = T[c*R + ry + i0+i];  B(c, j) = Y(c, j0+j) = T[c*R + ry + j0+j]
            const double4v acc = mfma_tile(T + ry + i0, 1, R, n - i0, T + ry + j0, R, 1, n - j0, nr);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int i = i0 + ri + 4 * q, j = j0 + cj;
                if (i < n && j < n) P[(size_t)i * n + j] = cur[q] - acc[q];
                cur[q] = nxt[q];
            }
        }
    }
    __syncthreads();
    PHASE_STAMP(5);
    // ---- G: quaternion normalisation (updateCommon ekf.cpp:29-31 / normalizeQuaternions 1024-1032) ----
    const bool first_block = AUTO ? half == 1 : a.normalize_all < 0;                              // of a long track: no normalisation yet
    const int nq = first_block ? 0 : (a.normalize_all != 0) ? 1 + (n - a.map_dim - CAM) / POSE : 1;      // map points behind the trail are not poses
    if (t < nq) normalize4(m + (t == 0 ? ORI : CAM + POSE * (t - 1) + 3));
    if (a.success_counter && t == 0 && !(AUTO && half == 1)) a.success_counter[b] += 1;
    if (a.spec == 2 && t == 0 && !(AUTO && half == 1)) a.cursor[b] = sel + 1;      // the tracks up to the applied one are final, the rest is re-examined
    if (a.spec == 3 && t == 0) a.cursor_out[b] = (int)blockIdx.y + 1;
}

template <int MODE, int TI>
__global__ __launch_bounds__(UPD_THREADS) void ekf_update_kernel(UpdateArgs a)
{
    // (r03 also tried one workgroup per CU pulling filters from a device queue: inside a loop the body lost its register allocation --
    // ~480 spilled VGPRs, 2.4x the time per filter -- and keeping P in the registers across the two blocks of a long track in ONE launch
    // -- 250 - 450 spilled VGPRs --, so masked launches use the compaction list and long tracks take two launches)
    int b = blockIdx.x;
    if (a.rec_list) { if ((int)blockIdx.x >= *a.rec_count) return; b = a.rec_list[blockIdx.x]; }
    ekf_update_body<MODE, TI>(a, b);
}

// the update launches of the speculative loop over long records (UpdateArgs::half_auto), MODE 2, three row tiles
__global__ __launch_bounds__(UPD_THREADS) void ekf_update_spec_long_kernel(UpdateArgs a)
{
    ekf_update_body<2, 3, true>(a, blockIdx.x);
}

// Two masked update launches in ONE grid (ragged visits: the inliers of the short class and the first block of the long class's
// inliers are different filters, ~200 + ~50 of 1024 at the reference's track mix -- one workgroup each on a CU of its own, so two
// launches were two latency chains back to back on a mostly idle chip): the first workgroups serve a1's list, the next ones a0's.
// The argument block is chosen by a uniform select; the body is instantiated once.
// Every workgroup needs a CU of its own, so a grid of more than num_cus live workgroups takes a second round. The long class follows
// with a second launch anyway (its second block update): `part` 0 = all of a1 + the entries of a0's list that fit beside them on the
// chip (cap = num_cus - *a1.rec_count), `part` 1 = all of a1 + the REST of a0's list -- the visit loop issues (a0 = short class, a1 =
// long block 1, part 0) and then (a0 = short class, a1 = long block 2, part 1); `part` < 0: all of both lists.
struct UpdatePair { UpdateArgs a[2]; };
template <int MODE, int TI>
__global__ __launch_bounds__(UPD_THREADS) void ekf_update_dual_kernel(UpdatePair p, int part, int num_cus)
{
    const int n0 = *p.a[0].rec_count, n1 = *p.a[1].rec_count, i = (int)blockIdx.x;
    const int cap = min(n0, max(num_cus - n1, 0));
    const int lo = part == 1 ? cap : 0, hi = part == 0 ? cap : n0;          // a[0]'s share of this launch
    const bool second = i < n1;
    // (ONE block is read, through a run-time index into the kernel-argument segment: with two by-value blocks and a select per field
    //  both sat in SGPRs -- 250 of them spilled into VGPR lanes, in a kernel that has no VGPR to spare)
    const UpdateArgs &a = p.a[second ? 1 : 0];
    const int j = second ? i : i - n1 + lo;
    if (!second && j >= hi) return;
    ekf_update_body<MODE, TI>(a, a.rec_list[j]);
}

// (r05, measured and dropped: the same grid with a long record's workgroup running block 2 right behind block 1 -- P through L2 in
// between -- and a second launch that only serves the short records that found no CU: one lane 10.04 / 10.00 -> 10.13 / 10.10 ms per
// step, four lanes 29.44 / 29.27 -> 29.40 / 29.23: the visit's length is the long records' block-1 -> block-2 chain either way, and two
// instances of the body cost 12 more spilled VGPRs. profiles/r05/long_blocks_one_launch_ab.txt)

// ---------------------------------------------------------------------------------------------
// chi2 gate for MANY filters at once (throughput launches): S = H P H' + R without ever holding H P.
//
// ekf_update_kernel keeps P in registers (8 waves x 256 VGPRs) and the tall matrix in 134 KB of LDS so that an UPDATE reads P
// once -- one filter per CU at a time, its phases (products, S, a 40-pivot Cholesky) strictly one after the other: a gate launch over
// 1024 filters is 4 rounds of a 33 us latency chain at 32 % MFMA busy. A gate needs none of that state. Here a wavefront
// owns 16-column blocks J of P and chains two MFMA products per block through its accumulators:
//     G_J = P(J, :) H'          (16 x nr; A = tiles of P streamed from HBM, B = H' from LDS)
//     S  += H(:, J) G_J         (nr x nr; A = H from LDS, B = G_J -- the accumulator tile of the first product IS the B operand
//                                layout of the second: lane (kq, c) holds rows 4 v + kq, exactly the k order of a k-step)
// so H P never exists, LDS holds H (61 KB) + S (15 KB) and two workgroups of 4 waves share a CU: one filter's Cholesky runs under
// the other's MFMAs. P(J, k) is read as stored (no symmetry assumption). The factorisation / chi2 part is the blocked Cholesky of
// ekf_update_kernel restricted to the measurement rows.
// ---------------------------------------------------------------------------------------------
struct GateArgs {
    int n, nr, l, Rs;                 // Rs: column stride of the (nr + 1) x nr matrix [S; v'] in LDS
    const double *P;                  // [batch][n][n]
    const double *H, *v;              // [batch] records: nr x l column-major, nr
    double rd, noise_scale;
    double *chi2; int *status;
    const unsigned char *active;
    const int *success_counter; int max_successful;      // optional: filters whose quota is used up are skipped
};

constexpr int GATE_THREADS = 256;

template <int TI>
__global__ __launch_bounds__(GATE_THREADS, 2) void ekf_gate_stream_kernel(GateArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = blockIdx.x;
    if (a.active && !a.active[b]) return;
    if (a.success_counter && a.success_counter[b] >= a.max_successful) return;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    constexpr int nwaves = GATE_THREADS / 64, nrp = 16 * TI;
    const int n = a.n, nr = a.nr, l = a.l, R = a.Rs;
    const double *P = a.P + (size_t)b * n * n, *H = a.H + (size_t)b * nr * l;
    const int lb = (l + 15) >> 4;
    // LDS: Hs [16 lb][nrp] (k-major, zero padded) | T [(nr + 1) x nr, stride R] ; W / col / red live in Hs once the products are done
    const GateStreamLds L = gate_stream_lds(TI, lb, R, nr);
    double *Hs = smem + L.Hs, *T = smem + L.T;
    const int kq = lane >> 4, cl = lane & 15;
    // ---- stage H (zero padded) and zero T ----
    for (int i = t; i < nrp * 16 * lb; i += GATE_THREADS) {
        const int k = i / nrp, r = i - k * nrp;
        Hs[i] = (k < l && r < nr) ? H[(size_t)k * nr + r] : 0.0;
    }
    for (int i = t; i < R * nr; i += GATE_THREADS) T[i] = 0.0;
    __syncthreads();
    // ---- products: this wave's column blocks J = wave, wave + 4, .. ----
    double4v accS[TI * (TI + 1) / 2];
#pragma unroll
    for (int u = 0; u < TI * (TI + 1) / 2; u++) accS[u] = double4v{0.0, 0.0, 0.0, 0.0};
    constexpr int DEPTH = 4;                                    // K blocks of P requested ahead of their MFMAs
    for (int J = wave; J < lb; J += nwaves) {
        const int jrow = min(J * 16 + cl, n - 1);
        auto fetch = [&](double (&pv)[4], int kb) {
#pragma unroll
            for (int sx = 0; sx < 4; sx++) pv[sx] = P[(size_t)min(kb * 16 + 4 * sx + kq, n - 1) * n + jrow];   // A(i = cl, k): P(J16 + cl, k)
        };
        double pv[DEPTH][4];
#pragma unroll
        for (int d = 0; d < DEPTH; d++) if (d < lb) fetch(pv[d], d);
        double4v accG[TI];
#pragma unroll
        for (int ct = 0; ct < TI; ct++) accG[ct] = double4v{0.0, 0.0, 0.0, 0.0};
        for (int kb0 = 0; kb0 < lb; kb0 += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; d++) {
                const int kb = kb0 + d;
                if (kb < lb) {
                    double hb[4][TI];
#pragma unroll
                    for (int sx = 0; sx < 4; sx++)
#pragma unroll
                        for (int ct = 0; ct < TI; ct++) hb[sx][ct] = Hs[(size_t)(kb * 16 + 4 * sx + kq) * nrp + 16 * ct + cl];   // B(k, c) = H(c, k)
#pragma unroll
                    for (int sx = 0; sx < 4; sx++)
#pragma unroll
                        for (int ct = 0; ct < TI; ct++)
                            accG[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(pv[d][sx], hb[sx][ct], accG[ct], 0, 0, 0);
                    if (kb + DEPTH < lb) fetch(pv[d], kb + DEPTH);
                }
            }
        }
        // S(rt, ct) += H(16 rt + i, J16 + k) G_J(k, 16 ct + c), lower tiles; k-step v: A = H(.., J16 + 4 v + kq), B = accG[ct][v]
        if (J * 16 < n) {
#pragma unroll
            for (int v = 0; v < 4; v++) {
                double ha[TI];
#pragma unroll
                for (int rt = 0; rt < TI; rt++) ha[rt] = Hs[(size_t)(J * 16 + 4 * v + kq) * nrp + 16 * rt + cl];                 // A(i = cl, k)
                int u = 0;
#pragma unroll
                for (int ct = 0; ct < TI; ct++)
#pragma unroll
                    for (int rt = ct; rt < TI; rt++, u++)
                        accS[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(ha[rt], accG[ct][v], accS[u], 0, 0, 0);
            }
        }
    }
    // ---- the waves' partial S meet in LDS in WAVE ORDER (r05: one wave per round, a barrier between the rounds -- with ds_add_f64 in
    // arrival order, r01 .. r04, two runs could differ by ~1 ulp of S) ----
    for (int w_turn = 0; w_turn < nwaves; ++w_turn) {
        if (wave == w_turn) {
            int u = 0;
#pragma unroll
            for (int ct = 0; ct < TI; ct++)
#pragma unroll
                for (int rt = ct; rt < TI; rt++, u++)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int i = 16 * rt + kq + 4 * q, c = 16 * ct + cl;
                        if (i < nr && c < nr && i >= c) T[(size_t)c * R + i] += accS[u][q];
                    }
        }
        __syncthreads();
    }
    for (int i = t; i < nr; i += GATE_THREADS) { T[(size_t)i * R + i] += a.rd; T[(size_t)i * R + nr] = a.v[(size_t)b * nr + i]; }
    double *W = Hs + CHOL_W, *col = Hs + CHOL_COL, *red = Hs + CHOL_RED;    // H is dead from here on
    __syncthreads();
    // ---- blocked Cholesky of [S; v'] (see ekf_update_kernel phase C), rows 0 .. nr ----
    const int Rlim = nr + 1;
    for (int j0 = 0; j0 < nr; j0 += 16) {
        const int w = min(16, nr - j0);
        const int ntile = (Rlim - j0 + 15) / 16;
        if (j0 > 0) {
            for (int tile = wave; tile < ntile; tile += nwaves) {
                const int i0 = j0 + 16 * tile, mi = Rlim - i0;
                const double4v acc = mfma_tile(T + i0, 1, R, mi, T + j0, R, 1, w, j0);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int i = kq + 4 * q;
                    if (i < mi && cl < w) T[(size_t)(j0 + cl) * R + i0 + i] -= acc[q];
                }
            }
            __syncthreads();
        }
        if (wave == 0) { if (w <= 8) factor_diag_block<8>(T, W, col, R, j0, w, lane); else factor_diag_block<16>(T, W, col, R, j0, w, lane); }
        __syncthreads();
        for (int i0 = j0 + w + 16 * wave; i0 < Rlim; i0 += 16 * nwaves) {
            const int mi = Rlim - i0;
            const double4v acc = mfma_tile(T + (size_t)j0 * R + i0, 1, R, mi, W, 16, 1, 16, w);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int i = kq + 4 * q;
                if (i < mi && cl < w) T[(size_t)(j0 + cl) * R + i0 + i] = acc[q];
            }
        }
        __syncthreads();
    }
    // ---- chi2 = noise_scale * z'z ----
    double sz = 0;
    for (int c = t; c < nr; c += GATE_THREADS) { const double z = T[(size_t)c * R + nr]; sz += z * z; }
    for (int o = 32; o > 0; o >>= 1) sz += __shfl_down(sz, o);
    if (lane == 0) red[wave] = sz;
    __syncthreads();
    if (t == 0) {
        double tot = 0; for (int w2 = 0; w2 < nwaves; w2++) tot += red[w2];
        tot *= a.noise_scale;
        if (a.chi2) a.chi2[b] = tot;
        // (a non-positive pivot leaves NaN / inf in z: reported as CHI2, as by ekf_update_kernel phase D and the sparse gates -- the bare
        //  comparison is false for a NaN and called such a filter an inlier)
        const bool broken = !(tot < 1e300);
        if (a.status) a.status[b] = (broken || tot > d_chi2inv95[nr]) ? 3 /*CHI2*/ : 0 /*INLIER*/;
    }
}

// ---------------------------------------------------------------------------------------------
// Column-sparse chi2 gate as its own launch (many filters): visualTrackOutlierCheck on the compact Jacobians the prepare launch left
// in HBM (VuPrepareArgs::fused == 2). One 4-wave workgroup per filter -- four waves sit one per SIMD, so the (J, ct) items of
// sparse_gate spread evenly over the matrix pipes --, LDS = Hc (28 KB at 10 stereo poses) + [S; v'] (15 KB): three workgroups per CU,
// whose single-wave Cholesky chains (40 dependent pivots, ~10 us) run under each other's products. The same chain inside the
// prepare kernel (two 80 KB workgroups per CU, both latency chains themselves) cost 60 us per 1024 filters (r03 measurements).
// ---------------------------------------------------------------------------------------------
struct SparseGateArgs {
    int n, nr, ncam, na_max;          // state dimension; rows of the longest record (= record stride of v); cameras; columns per Hc record
    const double *P;                  // [batch][n][n]
    const double *Hc, *v;             // [batch][nr * na_max] compact Jacobians (leading dimension: the record's rows), [batch][nr]
    const int *acol;                  // [batch][na_max]
    const int *nr_rec;                // ragged batches: rows of every record, or null
    const unsigned char *active;      // [batch]: 1 where triangulation and prepareVisualUpdate passed (written by the prepare launch)
    double rd, noise_scale;
    double *chi2; int *status;        // chi2 optional
    int hs_doubles;                   // LDS carve (SparseGateLds::T): doubles reserved for the staged Hc (it is the Cholesky scratch afterwards)
    int lds_doubles;                  // doubles available for Hc + [S; v'] together (BIG build: decides between the padded and the tight layout)
    int batch;
    const int *rec_count, *rec_list;  // this launch's records (compaction list of the long class), or null
    int *inl_count, *inl_list;        // appended: records whose gate said INLIER
};

constexpr int SGATE_THREADS = 256;         // small build: four waves, one per SIMD, three workgroups per CU
constexpr int SGATE_BIG_THREADS = 768;     // big build (one workgroup per CU by its LDS): three waves per SIMD for the 20 (J, group) items of an 84-row track (512 threads: 70.9 us per 256 records of 21 poses, 768: 66.7, 1024: 87 spilled VGPRs)

// BIG = false: up to 48 rows (three 43 KB workgroups per CU at 10 stereo poses); BIG = true: 49 .. 96 rows (tracks of 13 .. 21 stereo
// poses: 13 .. 21 poses x 4 rows), one workgroup per CU with the whole register file, Hc staged with nrp = 16 TI rows per column where that
// fits 160 KB together with [S; v'] and with 84 rows (TIGHT) where it does not (84 rows: 99.5 + 58.5 KB).
template <bool BIG>
__device__ __forceinline__ void sparse_gate_kernel_body(const SparseGateArgs &a, const int b_in)
{
    // (the record index may come out of a compaction list, i.e. a per-lane load: on the scalar unit every base address below is
    //  uniform and the P gather becomes scalar base + 32-bit lane offset)
    const int b = __builtin_amdgcn_readfirstlane(b_in);
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int t = threadIdx.x;
    constexpr int NTH = BIG ? SGATE_BIG_THREADS : SGATE_THREADS;
    PHASE_STAMP(12);
    // (flag, shape, column list and residual requested together: one round trip instead of three dependent ones)
    const unsigned char act_v = a.active[b];
    const int nr_v = a.nr_rec ? a.nr_rec[b] : a.nr;
    int my_acol_raw = a.acol[(size_t)b * a.na_max + min(t, a.na_max - 1)];
    double my_v_raw = a.v[(size_t)b * a.nr + min(t, a.nr - 1)];
    asm volatile("" : "+v"(my_acol_raw), "+v"(my_v_raw));
    if (!act_v) return;                                        // status stays NOT_COMPUTED (preset by the prepare launch)
    const int nr = __builtin_amdgcn_readfirstlane(nr_v);
    if (nr < 2 || nr > a.nr) return;
    const int n = a.n, npose = nr / (2 * a.ncam), na = 7 * npose + 1, na4 = (na + 3) & ~3;
    const int ti = BIG ? max((nr + 15) >> 4, 4) : (nr + 15) >> 4;       // (the BIG build starts at the 4-tile instantiation; chooses the sparse_gate instantiation below)
    const SparseGateShape shape = sparse_gate_shape(BIG, nr, na4, (size_t)a.lds_doubles);    // (uniform) does the padded layout fit?
    const bool tight = shape.tight;
    const int Rs = shape.Rs, nrp = shape.nrp;
    if (tight && nr > HV_GATE_TIGHT_ROWS) return;              // (the launcher sizes LDS for <= 84 rows: never taken)
    double *Hs = smem, *T = smem + a.hs_doubles;
    int *s_acol = reinterpret_cast<int *>(T + (size_t)Rs * nr);
    const double *Hc = a.Hc + (size_t)b * a.nr * a.na_max;
    // stage Hc k-major with zero padding (rows >= nr, columns >= na), [S; v'] zeroed with the residual row in place
    // (8 elements per thread in flight: a load -> LDS store loop without unrolling waits one HBM / L2 round trip per iteration -- 14 of
    // them at 10 stereo poses, which made this staging half of the kernel)
    const int my_acol = t < na ? my_acol_raw : 0;
    const double my_v = t < nr ? my_v_raw : 0.0;
    const int total = na4 * nrp;
    const unsigned inv_nrp = (unsigned)((0x100000000ull + (unsigned)nrp - 1) / (unsigned)nrp);       // i / nrp = umulhi(i, ceil(2^32 / nrp))
    for (int base = 0; base < total; base += 8 * NTH) {
        double hv_[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int i = base + q * NTH + t, u = (int)__umulhi((unsigned)i, inv_nrp), r = i - u * nrp;
            const bool live = i < total && u < na && r < nr;
            hv_[q] = live ? Hc[(size_t)(live ? u : 0) * nr + (live ? r : 0)] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int i = base + q * NTH + t;
            if (i < total) Hs[i] = hv_[q];
        }
    }
    for (int i = t; i < Rs * nr; i += NTH) T[i] = 0.0;             // (row nr of column c is rewritten below by thread c: same thread order
    if (t < na) s_acol[t] = my_acol;                                           //  is not guaranteed, so the barrier comes first)
    __syncthreads();
    if (t < nr) T[(size_t)t * Rs + nr] = my_v;
    __syncthreads();
    PHASE_STAMP(13);
    const double *Pb = a.P + (size_t)b * n * n;
    double chi;
    if constexpr (!BIG) {
        if (ti == 1)      chi = sparse_gate<1, NTH, true>(Pb, n, s_acol, na, Hs, T, Rs, nr, a.rd, a.noise_scale, Hs, BIG ? g_phase_stamp : nullptr);
        else if (ti == 2) chi = sparse_gate<2, NTH, true>(Pb, n, s_acol, na, Hs, T, Rs, nr, a.rd, a.noise_scale, Hs, BIG ? g_phase_stamp : nullptr);
        else              chi = sparse_gate<3, NTH, true>(Pb, n, s_acol, na, Hs, T, Rs, nr, a.rd, a.noise_scale, Hs, BIG ? g_phase_stamp : nullptr);
    } else {
        if (ti <= 4)      chi = sparse_gate<4, NTH, false>(Pb, n, s_acol, na, Hs, T, Rs, nr, a.rd, a.noise_scale, Hs, BIG ? g_phase_stamp : nullptr);
        else if (ti == 5) chi = sparse_gate<5, NTH, false>(Pb, n, s_acol, na, Hs, T, Rs, nr, a.rd, a.noise_scale, Hs, BIG ? g_phase_stamp : nullptr);
        else if (!tight)  chi = sparse_gate<6, NTH, false>(Pb, n, s_acol, na, Hs, T, Rs, nr, a.rd, a.noise_scale, Hs, BIG ? g_phase_stamp : nullptr);
        else              chi = sparse_gate<6, NTH, false, true>(Pb, n, s_acol, na, Hs, T, Rs, nr, a.rd, a.noise_scale, Hs, BIG ? g_phase_stamp : nullptr);
    }
    if (t == 0) {
        const bool broken = !(chi < 1e300);                    // non-positive pivot: reported as CHI2 (ekf_update_kernel phase D)
        const int outlier = broken || ((nr < HV_CHI2INV95_N) ? (chi > d_chi2inv95[nr]) : 0);
        a.status[b] = outlier ? 3 /*CHI2*/ : 0 /*INLIER*/;
        if (!outlier && a.inl_list) a.inl_list[atomicAdd(a.inl_count, 1)] = b;
        if (a.chi2) a.chi2[b] = chi;
    }
}

__global__ __launch_bounds__(SGATE_THREADS, 3) void ekf_sparse_gate_kernel(SparseGateArgs a) { sparse_gate_kernel_body<false>(a, blockIdx.x); }
__global__ __launch_bounds__(SGATE_BIG_THREADS, 1) void ekf_sparse_gate_big_kernel(SparseGateArgs a)
{
    int b = blockIdx.x;
    if (a.rec_list) { if (b >= *a.rec_count) return; b = a.rec_list[b]; }
    sparse_gate_kernel_body<true>(a, b);
}

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

__device__ __forceinline__ void blk_of(int idx, int cam_poses, int &start, int &size, int &kind)
{
    // kind 0: identity 1x1, 1: pC (3x3), 2: qC (4x4)
    if (idx == 0) { start = POS; size = 3; kind = 1; return; }
    if (idx == 1) { start = VEL; size = 3; kind = 1; return; }
    if (idx == 2) { start = ORI; size = 4; kind = 2; return; }
    if (idx < 13) { start = BGA + (idx - 3); size = 1; kind = 0; return; }
    const int p = idx - 13;
    if (p < 2 * cam_poses) { start = CAM + POSE * (p >> 1) + ((p & 1) ? 3 : 0); size = (p & 1) ? 4 : 3; kind = (p & 1) ? 2 : 1; return; }
    start = CAM + POSE * cam_poses + (p - 2 * cam_poses); size = 1; kind = 0;
}

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

}  // namespace

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// an update launch prepared but not issued (UpdateRequest::defer): two of them can share one grid (ekf_launch_update_dual)
struct UpdateLaunch { UpdateArgs a; int kmode = -1, ti = 0, lbk = 0; };

int ekf_launch_update(Ekf *e, const UpdateRequest &rq)
{
    Ctx *c = e->c;
    const int nr = rq.nr, l = rq.l, mode = rq.mode, generic = rq.generic, spec = rq.spec;
    const int nr_stride = rq.nr_stride <= 0 ? nr : rq.nr_stride;
    if (nr < 1 || nr > e->max_rows || l < 1 || l > e->n) return HV_ERR_INVALID;
    // the chi2 gate needs chi2inv95[nr] (the reference asserts n < chi2inv95.size(): ekf.cpp:806); mode 1 with an
    // inlier requirement is the update half of a gate that already ran
    if (!generic && mode != 1 && nr >= HV_CHI2INV95_N) return HV_ERR_INVALID;
    UpdateArgs a{};
    a.n = e->n; a.nr = nr; a.l = l; a.R = nr + e->n + 1;
    const UpdateShape shape = update_shape(e->n, nr, l, UPD_THREADS / 64);
    a.Rs = shape.Rs;                                     // (lds_stride; unpadded where T lives in the global workspace)
    a.mode = mode; a.generic = generic; a.normalize_all = rq.normalize_all; a.map_dim = e->map_dim;
    a.m = e->fixed.m; a.P = e->fixed.P; a.H = rq.H_dev; a.v = rq.v_dev; a.rdiag = rq.rdiag_dev; a.rd0 = rq.rd0; a.rd1 = rq.rd1; a.noise_scale = e->noise_scale;
    a.ws = e->fixed.ws; a.chi2 = rq.chi2_dev; a.status = rq.status_dev; a.active = rq.active_dev; a.require_inlier = rq.require_inlier_dev; a.success_counter = rq.success_counter_dev;
    a.spec = spec; a.n_tracks = rq.n_tracks; a.cursor = rq.cursor_dev; a.max_successful = rq.max_successful; a.gate_in = rq.gate_in_dev;
    a.cursor_out = rq.cursor_out_dev; a.pub = rq.pub_dev; a.pass_id = rq.pass_id; a.nr_rec = rq.nr_rec_dev; a.err = e->fixed.err_dev;
    a.h_stride = (size_t)nr_stride * l; a.v_stride = nr_stride;
    if (rq.compact.acol) {
        const CompactH *compact = &rq.compact;
        a.acol = compact->acol; a.na_max = compact->na_max; a.ncam = compact->ncam; a.h_stride = (size_t)nr_stride * compact->na_max;
        a.half = compact->half; a.nr_full = compact->nr_full;
        if (a.half == 1) { a.dm_out = compact->dm; a.gate_rw = compact->gate_rw; }
        if (a.half == 2) a.dm_in = compact->dm;
        a.rec_count = compact->rec_count; a.rec_list = compact->rec_list;
        a.half_auto = compact->half_auto; a.sel_io = compact->sel_io; a.epoch = compact->epoch;
        if (a.half_auto && (spec != 2 || !a.half || !a.sel_io || !a.dm_out == !a.dm_in)) return HV_ERR_INVALID;
    }
    const int ti = shape.ti, lbk = shape.lbk;
    int kmode = shape.kmode;
    a.use_lds = kmode != 0;
    // HV_EKF_GATE_KMODE (environment, experiments only): kernel variant for gate-only launches (1 = H streamed from L2, 2 WGs / CU)
    if (c->knob.ekf_gate_kmode == 1 && mode == 0 && !spec && kmode == 2) kmode = 1;
    if (a.acol && kmode != 2) return HV_ERR_UNSUPPORTED; // compact H is staged by the LDS-resident kernel only (vu_fused_supported)
    if (mode == 3) {                                     // gate (rd0) + update (rd1) in one launch: MODE 2 kernels only
        const bool can = kmode == 2 && shape.two_r;
        if (rq.two_r_done) *rq.two_r_done = can;
        if (!can) return HV_OK;                          // the caller falls back to two launches
    }
    if (spec && kmode != 2) return HV_ERR_UNSUPPORTED;   // the speculative loop keeps every record in the LDS-resident kernel
    const size_t shmem = lds_bytes(update_lds(shape.Rs, nr, UPD_THREADS / 64, kmode != 0, kmode == 2 ? shape.hs : 0));
    a.batch = e->batch;
    if (UpdateLaunch *defer = rq.defer) {
        if (mode == 3 || spec) return HV_ERR_INVALID;
        defer->a = a; defer->kmode = kmode; defer->ti = ti; defer->lbk = lbk;
        return HV_OK;
    }
    using Kern = void (*)(UpdateArgs);
    if (a.half_auto && (kmode != 2 || ti != 3)) return HV_ERR_INVALID;
    const Kern kern = a.half_auto ? (Kern)ekf_update_spec_long_kernel : kmode == 0 ? (Kern)ekf_update_kernel<0, 0> : kmode == 1 ? (Kern)ekf_update_kernel<1, 0>
                    : ti == 1 ? (Kern)ekf_update_kernel<2, 1> : ti == 2 ? (Kern)ekf_update_kernel<2, 2> : (Kern)ekf_update_kernel<2, 3>;
    ScopedKernelTime tm(c, HV_K_EKF_UPDATE);
    hipLaunchKernelGGL(kern, dim3(e->batch, (spec == 1 || spec == 3) ? rq.n_tracks : 1), dim3(UPD_THREADS), shmem, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

// two deferred masked MODE 2 launches over disjoint filters as one grid; *done = false when their shapes do not allow it (the caller
// then issues them one after the other)
static int ekf_launch_update_dual(Ekf *e, const UpdateLaunch &A, const UpdateLaunch &B, int part, bool *done)
{
    Ctx *c = e->c;
    *done = false;
    if (A.kmode != 2 || B.kmode != 2 || !A.a.rec_list || !B.a.rec_list || !A.a.rec_count || !B.a.rec_count) return HV_OK;
    const int ti = A.ti > B.ti ? A.ti : B.ti;
    if (ti != 3) return HV_OK;                                     // (the only pairing the visit loop produces: 44 + 42 rows)
    const auto bytes = [ti](const UpdateLaunch &u) { return lds_bytes(update_lds(u.a.Rs, u.a.nr, UPD_THREADS / 64, true, (size_t)(16 * ti) * (16 * u.lbk))); };
    const size_t sa = bytes(A), sb = bytes(B), shmem = sa > sb ? sa : sb;
    if (shmem > LDS_UPDATE_LIMIT) return HV_OK;
    ScopedKernelTime tm(c, HV_K_EKF_UPDATE);
    UpdatePair pair;
    pair.a[0] = A.a; pair.a[1] = B.a;
    hipLaunchKernelGGL((ekf_update_dual_kernel<2, 3>), dim3(e->batch), dim3(UPD_THREADS), shmem, c->stream, pair, part, c->num_cus);
    HV_HIP(c, hipGetLastError());
    *done = true;
    return HV_OK;
}

int ekf_launch_update_paired(Ekf *e, const UpdateRequest &us, const UpdateRequest &b1, const UpdateRequest &b2, bool *done)
{
    // (short class beside block 1, what did not fit on the chip beside block 2: see ekf_update_dual_kernel)
    UpdateLaunch s, u1, u2;
    *done = false;
    const auto prepare = [e](UpdateRequest rq, UpdateLaunch *out) { rq.defer = out; return ekf_launch_update(e, rq); };
    int rc = prepare(us, &s);
    if (rc == HV_OK) rc = prepare(b1, &u1);
    if (rc == HV_OK) rc = prepare(b2, &u2);
    if (rc != HV_OK) return rc;
    rc = ekf_launch_update_dual(e, s, u1, 0, done);
    if (rc != HV_OK || !*done) return rc;
    bool again = false;
    return ekf_launch_update_dual(e, s, u2, 1, &again);              // (same shapes: accepted again)
}

int ekf_launch_gate_stream(Ekf *e, const GateStreamRequest &rq)
{
    Ctx *c = e->c;
    const int nr = rq.nr, l = rq.l;
    bool *done = rq.done;
    *done = false;
    if (nr < 1 || nr > 48 || nr >= HV_CHI2INV95_N || l < 1 || l > e->n) return HV_OK;        // the caller keeps its other route
    GateArgs a{};
    a.n = e->n; a.nr = nr; a.l = l;
    a.Rs = lds_stride(nr + 1);
    a.P = e->fixed.P; a.H = rq.H_dev; a.v = rq.v_dev; a.rd = rq.rd; a.noise_scale = e->noise_scale; a.chi2 = rq.chi2_dev; a.status = rq.status_dev;
    a.active = rq.active_dev; a.success_counter = rq.success_counter_dev; a.max_successful = rq.max_successful;
    const int ti = tiles16(nr);
    const GateStreamLds L = gate_stream_lds(ti, tiles16(l), a.Rs, nr);
    if (!gate_stream_admitted(L)) return HV_OK;                               // W / col / red borrow the H area; the gate limit
    using Kern = void (*)(GateArgs);
    const Kern kern = ti == 1 ? (Kern)ekf_gate_stream_kernel<1> : ti == 2 ? (Kern)ekf_gate_stream_kernel<2> : (Kern)ekf_gate_stream_kernel<3>;
    ScopedKernelTime tm(c, HV_K_EKF_UPDATE);
    hipLaunchKernelGGL(kern, dim3(e->batch), dim3(GATE_THREADS), lds_bytes(L), c->stream, a);
    HV_HIP(c, hipGetLastError());
    *done = true;
    return HV_OK;
}

int ekf_launch_sparse_gate(Ekf *e, const SparseGateRequest &rq)
{
    Ctx *c = e->c;
    const int np = rq.np, ncam = rq.ncam;
    const hipStream_t stream = rq.stream ? rq.stream : c->stream;
    const int nr = 2 * np * ncam, na_max = 7 * np + 1;
    if (nr < 2 || nr > 96 || nr >= HV_CHI2INV95_N || !rq.active_dev || !rq.status_dev) return HV_ERR_INVALID;
    const SparseGateLds L = sparse_gate_lds(np, ncam);      // sized for the launch's longest record
    if (!L.supported) return HV_ERR_UNSUPPORTED;
    SparseGateArgs a{};
    a.n = e->n; a.nr = nr; a.ncam = ncam; a.na_max = na_max; a.P = e->fixed.P; a.Hc = rq.Hc_dev; a.v = rq.v_dev; a.acol = rq.acol_dev; a.nr_rec = rq.nr_rec_dev;
    a.active = rq.active_dev; a.rd = rq.rd; a.noise_scale = e->noise_scale; a.chi2 = rq.chi2_dev; a.status = rq.status_dev;
    a.hs_doubles = (int)(L.T - L.Hs); a.lds_doubles = (int)(L.acol - L.Hs);
    ScopedKernelTime tm(c, HV_K_EKF_GATE, stream);
    a.rec_count = rq.rec_count; a.rec_list = rq.rec_list; a.inl_count = rq.inl_count; a.inl_list = rq.inl_list;
    a.batch = e->batch;
    if (L.big) hipLaunchKernelGGL(ekf_sparse_gate_big_kernel, dim3((unsigned)e->batch), dim3(SGATE_BIG_THREADS), L.bytes, stream, a);
    else       hipLaunchKernelGGL(ekf_sparse_gate_kernel, dim3(e->batch), dim3(SGATE_THREADS), L.bytes, stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

// the kernels' dynamic-LDS limits, set once per context (hv_create; never inside a launch that may be under capture)
int ekf_kernels_init(Ctx *c)
{
    HV_HIP(c, set_lds_limit(ekf_update_kernel<1, 0>, LDS_UPDATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_update_kernel<2, 1>, LDS_UPDATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_update_kernel<2, 2>, LDS_UPDATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_update_kernel<2, 3>, LDS_UPDATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_update_spec_long_kernel, LDS_UPDATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_update_dual_kernel<2, 3>, LDS_UPDATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_gate_stream_kernel<1>, LDS_GATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_gate_stream_kernel<2>, LDS_GATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_gate_stream_kernel<3>, LDS_GATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_sparse_gate_kernel, LDS_GATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_sparse_gate_big_kernel, LDS_SGATE_BIG_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_augment_kernel<false>, LDS_AUGMENT_LIMIT));      // (<true>, the device-pointer entries' folded form, stays at LDS_DEFAULT_LIMIT)
    return HV_OK;
}

}  // namespace hv

using hv::Ctx;
using hv::Ekf;

extern "C" {

void hv_ekf_default_params(hv_ekf_params *p)
{
    if (!p) return;
    p->cameraTrailLength = 20; p->hybridMapSize = 0;
    p->noiseScale = 100; p->gravity = 9.819; p->augmentR = 1e-9; p->initZuptR = 1e-4; p->rotationZuptR = 1e-6;
    p->noiseInitialPos = 1e-5; p->noiseInitialOri = 0.0316227766; p->noiseInitialVel = 0.1;
    p->noiseInitialPosTrail = 100; p->noiseInitialOriTrail = 3.16227766;
    p->noiseInitialBGA = 1e-3; p->noiseInitialBAA = 1e-6; p->noiseInitialBAT = 1e-5; p->noiseInitialSFT = 1e-5;
    p->noiseProcessAcc = 0.003; p->noiseProcessGyro = 0.00017; p->noiseProcessBAA = 1e-4; p->noiseProcessBGA = 0;
    p->noiseProcessBAARev = 0.1; p->noiseProcessBGARev = 0.1;
}

void hv_ekf_destroy(hv_ekf *h)
{
    if (!h) return;
    Ekf *e = &h->e;
    if (e->c) for (hipStream_t s : {e->c->stream, e->c->aux_stream}) if (s) (void)hipStreamSynchronize(s);   // both streams, before the first free
    if (e->longc.ev_fork) (void)hipEventDestroy(e->longc.ev_fork);
    if (e->longc.ev_join) (void)hipEventDestroy(e->longc.ev_join);
    delete h;
}

int hv_ekf_create(hv_ctx *ctx, const hv_ekf_params *par, int batch, hv_ekf **out)
{
    if (!ctx || !par || !out || batch < 1 || par->cameraTrailLength < 1 || par->hybridMapSize < 0) return HV_ERR_INVALID;
    *out = nullptr;
    Ctx *c = hv::ctx_of(ctx);
    hv_ekf *h = new (std::nothrow) hv_ekf();
    if (!h) return HV_ERR_NOMEM;
    Ekf *e = &h->e;
    e->c = c; e->par = *par; e->batch = batch;
    e->cam = par->cameraTrailLength; e->map_dim = 3 * par->hybridMapSize;
    const int n = e->n = hv::INER + hv::POSE * e->cam + e->map_dim;
    e->noise_scale = par->noiseScale * par->noiseScale;
    e->max_rows = n;
    const size_t nn = (size_t)n * n;
    bool ok = e->fixed.ensure(*e) == HV_OK;
    if (ok && hipMemset(e->fixed.err_dev, 0, sizeof(int)) != hipSuccess) ok = false;
    if (!ok) { hv_ekf_destroy(h); return HV_ERR_NOMEM; }

    // initial state and covariance: EKFImplementation ctor, ekf.cpp:153-296
    std::vector<double> m0(n, 0.0), P0(nn, 0.0), Q0(144, 0.0);
    auto sq = [](double x) { return x * x; };
    m0[hv::ORI] = 1.0; m0[hv::BAT] = m0[hv::BAT + 1] = m0[hv::BAT + 2] = 1.0;
    for (int i = 0; i < 3; i++) {
        P0[(size_t)(hv::POS + i) * n + hv::POS + i] = sq(par->noiseInitialPos);
        P0[(size_t)(hv::VEL + i) * n + hv::VEL + i] = sq(par->noiseInitialVel);
        P0[(size_t)(hv::BGA + i) * n + hv::BGA + i] = sq(par->noiseInitialBGA);
        P0[(size_t)(hv::BAA + i) * n + hv::BAA + i] = sq(par->noiseInitialBAA);
        P0[(size_t)(hv::BAT + i) * n + hv::BAT + i] = sq(par->noiseInitialBAT);
    }
    for (int i = 0; i < 4; i++) P0[(size_t)(hv::ORI + i) * n + hv::ORI + i] = 1.0;
    P0[(size_t)hv::SFT * n + hv::SFT] = sq(par->noiseInitialSFT);
    for (int cidx = 0; cidx < e->cam; cidx++) {
        const int b0 = hv::CAM + cidx * hv::POSE;
        for (int i = 0; i < 3; i++) P0[(size_t)(b0 + i) * n + b0 + i] = sq(par->noiseInitialPosTrail);
        for (int i = 3; i < 7; i++) P0[(size_t)(b0 + i) * n + b0 + i] = sq(par->noiseInitialOriTrail);
    }
    for (int i = 0; i < 3; i++) { Q0[(hv::Q_ACC + i) * 13] = sq(par->noiseProcessAcc); Q0[(hv::Q_GYRO + i) * 13] = sq(par->noiseProcessGyro); }
    for (auto &x : P0) x *= e->noise_scale;
    for (auto &x : Q0) x *= e->noise_scale;
    int rc = HV_OK;
    for (int b = 0; b < batch && rc == HV_OK; b++) {
        rc = hv_ekf_set_state(h, b, m0.data(), P0.data());
        if (rc == HV_OK) rc = hv_ekf_set_process_noise(h, b, Q0.data());
    }
    if (rc != HV_OK) { hv_ekf_destroy(h); return rc; }
    *out = h;
    return HV_OK;
}

void hv_vu_default_params(hv_vu_params *p)
{
    if (!p) return;
    *p = hv_vu_params{};
    p->triangulationConvergenceThreshold = 1e-2; p->triangulationConvergenceR = 11.0;            // parameter_definitions.c:37-44
    p->triangulationRcondThreshold = 1e-8; p->triangulationGaussNewtonIterations = 10;
    p->triangulationMinDist = 0; p->triangulationMaxDist = 1e300;
    p->estimateImuCameraTimeShift = 1;                                                          // :163
    p->trackRmseThreshold = -1.0; p->trackOutlierThresholdGrowthFactor = 1.0;                   // :21,27
    p->useStereo = 0;
    const double imu[9] = {1, 0, 0, 0, -1, 0, 0, 0, -1};                                         // :178 imuToCameraMatrix (symmetric)
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) {
        const double v = r < 3 && c < 3 ? imu[3 * r + c] : (r == c ? 1.0 : 0.0);
        p->imuToCamera[4 * r + c] = v; p->secondImuToCamera[4 * r + c] = v;
    }
    const double tr[3] = {0.0075, 0.013, -0.0003};                                               // :187 stereoCameraTranslation
    for (int r = 0; r < 3; ++r) p->secondImuToCamera[4 * r + 3] += tr[r];                         // tracker/util.cpp:100-105
}

// insertMapPoint (ekf.cpp:911-921) on the resident state of one filter: nothing but the three coordinates crosses the bus
namespace hv { namespace {
__global__ __launch_bounds__(256) void ekf_insert_map_point_kernel(int n, int off, double *m, double *P, double x, double y, double z)
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
} }

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

int hv_ekf_frame_error(hv_ekf *h, int *flags)
{
    if (!h || !flags) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    HV_HIP(c, hipMemcpyAsync(flags, e->fixed.err_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    if (*flags) HV_HIP(c, hipMemsetAsync(e->fixed.err_dev, 0, sizeof(int), c->stream));
    return HV_OK;
}

/* developer aid (not in the public header): phase time stamps of the last update kernel */
int hv_debug_ekf_phase_stamps(hv_ekf *h, long long *out8)
{
    if (!h || !out8) return HV_ERR_INVALID;
    Ctx *c = h->e.c;
    HV_HIP(c, hipStreamSynchronize(c->stream));
    HV_HIP(c, hipMemcpyFromSymbol(out8, HIP_SYMBOL(hv::g_phase_stamp), sizeof(long long) * 16));
    return HV_OK;
}

int hv_ekf_state_dim(const hv_ekf *h) { return h ? h->e.n : HV_ERR_INVALID; }
int hv_ekf_batch(const hv_ekf *h) { return h ? h->e.batch : HV_ERR_INVALID; }

int hv_ekf_set_state(hv_ekf *h, int b, const double *m, const double *P)
{
    if (!h || b < 0 || b >= h->e.batch) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c; const size_t n = e->n;
    if (m) HV_HIP(c, hipMemcpyAsync(e->fixed.m + b * n, m, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    if (P) HV_HIP(c, hipMemcpyAsync(e->fixed.P + b * n * n, P, sizeof(double) * n * n, hipMemcpyHostToDevice, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    return HV_OK;
}

int hv_ekf_get_state(hv_ekf *h, int b, double *m, double *P)
{
    if (!h || b < 0 || b >= h->e.batch) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c; const size_t n = e->n;
    if (m) HV_HIP(c, hipMemcpyAsync(m, e->fixed.m + b * n, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    if (P) HV_HIP(c, hipMemcpyAsync(P, e->fixed.P + b * n * n, sizeof(double) * n * n, hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    return HV_OK;
}

int hv_ekf_get_means(hv_ekf *h, double *m_all)
{
    if (!h || !m_all) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    HV_HIP(c, hipMemcpyAsync(m_all, e->fixed.m, sizeof(double) * e->n * e->batch, hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    return HV_OK;
}

int hv_ekf_set_process_noise(hv_ekf *h, int b, const double *Q)
{
    if (!h || !Q || b < 0 || b >= h->e.batch) return HV_ERR_INVALID;
    Ctx *c = h->e.c;
    HV_HIP(c, hipMemcpyAsync(h->e.fixed.Q + (size_t)b * 144, Q, sizeof(double) * 144, hipMemcpyHostToDevice, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    return HV_OK;
}

int hv_ekf_get_process_noise(hv_ekf *h, int b, double *Q)
{
    if (!h || !Q || b < 0 || b >= h->e.batch) return HV_ERR_INVALID;
    Ctx *c = h->e.c;
    HV_HIP(c, hipMemcpyAsync(Q, h->e.fixed.Q + (size_t)b * 144, sizeof(double) * 144, hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    return HV_OK;
}

int hv_ekf_get_dydx(hv_ekf *h, int b, double *F)
{
    if (!h || !F || b < 0 || b >= h->e.batch) return HV_ERR_INVALID;
    Ctx *c = h->e.c;
    HV_HIP(c, hipMemcpyAsync(F, h->e.fixed.dydx + (size_t)b * 400, sizeof(double) * 400, hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    return HV_OK;
}

int hv_ekf_device_pointers(hv_ekf *h, double **m_dev, double **P_dev)
{
    if (!h) return HV_ERR_INVALID;
    if (m_dev) *m_dev = h->e.fixed.m;
    if (P_dev) *P_dev = h->e.fixed.P;
    return HV_OK;
}

static int predict_common(Ekf *e, const double *dt_dev, const double *gyro_dev, const double *acc_dev,
                          double dt0, const double *g0, const double *a0, int nsteps = 1)
{
    Ctx *c = e->c;
    hv::PredictArgs a{};
    a.n = e->n; a.batch = e->batch; a.m = e->fixed.m; a.P = e->fixed.P; a.Q = e->fixed.Q; a.dydx = e->fixed.dydx;
    a.dt = dt_dev; a.gyro = gyro_dev; a.acc = acc_dev; a.dt0 = dt0; a.nsteps = nsteps;
    for (int i = 0; i < 3; i++) { a.g0[i] = g0 ? g0[i] : 0.0; a.a0[i] = a0 ? a0[i] : 0.0; }
    a.noise_scale = e->noise_scale; a.gravity = e->par.gravity;
    a.baa = e->par.noiseProcessBAA; a.baa_rev = e->par.noiseProcessBAARev;
    a.bga = e->par.noiseProcessBGA; a.bga_rev = e->par.noiseProcessBGARev;
    hv::ScopedKernelTime tm(c, HV_K_EKF_PREDICT);
    // knob ekf_predict_chain: 1 (late r06) = launches of three or more samples run ekf_predict_chain_kernel (the mean recursion of the samples
    // on one wavefront, F / L of a chunk of samples in one pass); 2 = every launch; 0 = never (ekf_predict_kernel: nine barrier-separated
    // stages per sample). Bit-identical results. Measured (profiles/r06/predict_chain_ab.txt): 10 samples 53.2 -> 50.3 us for one filter,
    // 139 -> 129 us at 1024 filters; ONE sample 13.4 -> 15.0 us, hence the rule
    const int chain = c->knob.ekf_predict_chain;
    if (chain == 2 || (chain == 1 && nsteps >= 3)) hipLaunchKernelGGL(hv::ekf_predict_chain_kernel, dim3(e->batch), dim3(256), 0, c->stream, a);
    else                                hipLaunchKernelGGL(hv::ekf_predict_kernel, dim3(e->batch), dim3(256), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_ekf_predict(hv_ekf *h, const double *dt, const double *gyro, const double *acc)
{
    if (!h || !dt || !gyro || !acc) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    if (e->batch == 1) return predict_common(e, nullptr, nullptr, nullptr, dt[0], gyro, acc);   // immediates, no copy
    const size_t B = e->batch;
    HV_HIP(c, hipMemcpyAsync(e->fixed.simu, dt, sizeof(double) * B, hipMemcpyHostToDevice, c->stream));
    HV_HIP(c, hipMemcpyAsync(e->fixed.simu + B, gyro, sizeof(double) * 3 * B, hipMemcpyHostToDevice, c->stream));
    HV_HIP(c, hipMemcpyAsync(e->fixed.simu + 4 * B, acc, sizeof(double) * 3 * B, hipMemcpyHostToDevice, c->stream));
    return predict_common(e, e->fixed.simu, e->fixed.simu + B, e->fixed.simu + 4 * B, 0.0, nullptr, nullptr);
}

int hv_ekf_predict_dev(hv_ekf *h, const double *dt_dev, const double *gyro_dev, const double *acc_dev)
{
    if (!h || !dt_dev || !gyro_dev || !acc_dev) return HV_ERR_INVALID;
    return predict_common(&h->e, dt_dev, gyro_dev, acc_dev, 0.0, nullptr, nullptr);
}

int hv_ekf_predict_n(hv_ekf *h, int n_samples, const double *dt, const double *gyro, const double *acc)
{
    if (!h || n_samples < 1 || n_samples > HV_EKF_MAX_PREDICT_SAMPLES || !dt || !gyro || !acc) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    if (n_samples == 1 && e->batch == 1) return predict_common(e, nullptr, nullptr, nullptr, dt[0], gyro, acc);
    const size_t nB = (size_t)n_samples * e->batch;
    double *d_dt = e->fixed.simu, *d_g = e->fixed.simu + nB, *d_a = e->fixed.simu + 4 * nB;
    HV_HIP(c, hipMemcpyAsync(d_dt, dt, sizeof(double) * nB, hipMemcpyHostToDevice, c->stream));
    HV_HIP(c, hipMemcpyAsync(d_g, gyro, sizeof(double) * 3 * nB, hipMemcpyHostToDevice, c->stream));
    HV_HIP(c, hipMemcpyAsync(d_a, acc, sizeof(double) * 3 * nB, hipMemcpyHostToDevice, c->stream));
    return predict_common(e, d_dt, d_g, d_a, 0.0, nullptr, nullptr, n_samples);
}

int hv_ekf_predict_n_dev(hv_ekf *h, int n_samples, const double *dt_dev, const double *gyro_dev, const double *acc_dev)
{
    if (!h || n_samples < 1 || !dt_dev || !gyro_dev || !acc_dev) return HV_ERR_INVALID;
    return predict_common(&h->e, dt_dev, gyro_dev, acc_dev, 0.0, nullptr, nullptr, n_samples);
}

static int stage_update_inputs(Ekf *e, int nr, int l, const double *H, const double *v, const double *rdiag,
                               const unsigned char *active)
{
    Ctx *c = e->c; const size_t B = e->batch;
    if ((size_t)nr * l * B > e->fixed.sH_cap) return HV_ERR_INVALID;
    HV_HIP(c, hipMemcpyAsync(e->fixed.sH, H, sizeof(double) * nr * l * B, hipMemcpyHostToDevice, c->stream));
    HV_HIP(c, hipMemcpyAsync(e->fixed.sv, v, sizeof(double) * nr * B, hipMemcpyHostToDevice, c->stream));
    if (rdiag) HV_HIP(c, hipMemcpyAsync(e->fixed.sr, rdiag, sizeof(double) * B, hipMemcpyHostToDevice, c->stream));
    if (active) HV_HIP(c, hipMemcpyAsync(e->fixed.sactive, active, B, hipMemcpyHostToDevice, c->stream));
    return HV_OK;
}

int hv_ekf_update(hv_ekf *h, int nr, int l, const double *H, const double *y, const double *r_diag,
                  const unsigned char *active, int normalize_all)
{
    if (!h || !H || !y || !r_diag) return HV_ERR_INVALID;
    Ekf *e = &h->e;
    if (nr < 1 || nr > e->max_rows || l < 1 || l > e->n) return HV_ERR_INVALID;
    int rc = stage_update_inputs(e, nr, l, H, y, r_diag, active);
    if (rc != HV_OK) return rc;
    hv::UpdateRequest rq;
    rq.nr = nr; rq.l = l; rq.H_dev = e->fixed.sH; rq.v_dev = e->fixed.sv; rq.rdiag_dev = e->fixed.sr; rq.mode = 1; rq.generic = 1; rq.normalize_all = normalize_all;
    if (active) rq.active_dev = e->fixed.sactive;
    return hv::ekf_launch_update(e, rq);
}

int hv_ekf_visual_gate(hv_ekf *h, int nr, int l, const double *H, const double *v, double r, double *chi2, int *status)
{
    if (!h || !H || !v) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    if (nr < 1 || nr > e->max_rows || l < 1 || l > e->n) return HV_ERR_INVALID;
    int rc = stage_update_inputs(e, nr, l, H, v, nullptr, nullptr);
    if (rc != HV_OK) return rc;
    rc = hv::ekf_launch_update(e, hv::gate_request(nr, l, e->fixed.sH, e->fixed.sv, r * r * e->noise_scale, e->fixed.schi2, e->fixed.sstatus));
    if (rc != HV_OK) return rc;
    if (chi2) HV_HIP(c, hipMemcpyAsync(chi2, e->fixed.schi2, sizeof(double) * e->batch, hipMemcpyDeviceToHost, c->stream));
    if (status) HV_HIP(c, hipMemcpyAsync(status, e->fixed.sstatus, sizeof(int) * e->batch, hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    return HV_OK;
}

int hv_ekf_visual_update(hv_ekf *h, int nr, int l, const double *H, const double *v, double r, const unsigned char *active)
{
    if (!h || !H || !v) return HV_ERR_INVALID;
    Ekf *e = &h->e;
    if (nr < 1 || nr > e->max_rows || l < 1 || l > e->n) return HV_ERR_INVALID;
    int rc = stage_update_inputs(e, nr, l, H, v, nullptr, active);
    if (rc != HV_OK) return rc;
    return hv::ekf_launch_update(e, hv::inlier_update_request(nr, l, e->fixed.sH, e->fixed.sv, r * r * e->noise_scale, active ? e->fixed.sactive : nullptr));
}

int hv_ekf_visual_dev(hv_ekf *h, int nr, int l, const double *H_dev, const double *v_dev, double r, int mode,
                      double *chi2_dev, int *status_dev)
{
    if (!h || !H_dev || !v_dev || mode < 0 || mode > 2) return HV_ERR_INVALID;
    Ekf *e = &h->e;
    const int stream_gate = e->c->knob.ekf_stream_gate;
    if (mode == 0 && (stream_gate == 1 || (stream_gate < 0 && e->batch > 256))) {      // gate only, many filters: two per CU
        bool done = false;
        hv::GateStreamRequest g;
        g.nr = nr; g.l = l; g.H_dev = H_dev; g.v_dev = v_dev; g.rd = r * r * e->noise_scale; g.chi2_dev = chi2_dev; g.status_dev = status_dev; g.done = &done;
        const int rc = hv::ekf_launch_gate_stream(e, g);
        if (rc != HV_OK || done) return rc;
    }
    hv::UpdateRequest rq = hv::gate_request(nr, l, H_dev, v_dev, r * r * e->noise_scale, chi2_dev, status_dev);
    rq.mode = mode; rq.normalize_all = 1;
    return hv::ekf_launch_update(e, rq);
}

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
    if (discarded) {
        if (e->batch == 1) a.dropped0 = discarded[0];
        else { HV_HIP(c, hipMemcpyAsync(e->fixed.sdrop, discarded, sizeof(int) * e->batch, hipMemcpyHostToDevice, c->stream)); a.dropped = e->fixed.sdrop; }
    }
    if (active) { HV_HIP(c, hipMemcpyAsync(e->fixed.sactive, active, e->batch, hipMemcpyHostToDevice, c->stream)); a.active = e->fixed.sactive; }
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
    Ekf *e = &h->e; Ctx *c = e->c;
    const int *d_drop = nullptr; const unsigned char *d_act = nullptr;
    if (discarded) { HV_HIP(c, hipMemcpyAsync(e->fixed.sdrop, discarded, sizeof(int) * e->batch, hipMemcpyHostToDevice, c->stream)); d_drop = e->fixed.sdrop; }
    if (active) { HV_HIP(c, hipMemcpyAsync(e->fixed.sactive, active, e->batch, hipMemcpyHostToDevice, c->stream)); d_act = e->fixed.sactive; }
    const int rc = augment_dev_impl(h, d_drop, d_act, true);
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
    hv::ShiftArgs a{e->n, e->map_dim, e->fixed.m, e->fixed.P, e->fixed.P1, e->fixed.m1, nullptr};
    if (active) { HV_HIP(c, hipMemcpyAsync(e->fixed.sactive, active, e->batch, hipMemcpyHostToDevice, c->stream)); a.active = e->fixed.sactive; }
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

}  // extern "C"
