// EKF predict for a batch of independent filters, one workgroup per filter (the family map is in ekf.hip): the kernels, their
// launcher and the hv_ekf_predict* entries.
//   * predict: thread 0 evaluates the mean and the 20 x 20 Jacobians while the other wavefronts
//     already hold the slabs of P10 / P01 they need; the off-diagonal blocks are MFMA items.
#include <math.h>

#include "ekf_device.hpp"
#include "ekf_host.hpp"

// The library is built with -ffp-contract=off for the tracker's bit-exact binary32 sequence; the
// EKF is judged against a relative tolerance, and a fused multiply-add is one rounding fewer and
// half the f64 instructions of its dependency chains.
#pragma clang fp contract(fast)

namespace hv {

namespace {

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

}  // namespace

#ifdef HV_EKF_PHASE_STAMPS
hipError_t ekf_predict_phase_stamps(long long *out16) { return hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_phase_stamp), sizeof(long long) * 16); }
#endif

}  // namespace hv

using hv::Ctx;
using hv::Ekf;

extern "C" {

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

// the samples of every filter staged in the context's arena: dt [n_samples x batch], gyro and acc [n_samples x batch][3]
static int predict_staged(Ekf *e, int n_samples, const double *dt, const double *gyro, const double *acc)
{
    const size_t nB = (size_t)n_samples * e->batch;
    hv::Stage s(e->c);
    const auto o_dt = s.in(dt, nB), o_g = s.in(gyro, 3 * nB), o_a = s.in(acc, 3 * nB);
    if (const int rc = s.upload()) return rc;
    return predict_common(e, s.at(o_dt), s.at(o_g), s.at(o_a), 0.0, nullptr, nullptr, n_samples);
}

int hv_ekf_predict(hv_ekf *h, const double *dt, const double *gyro, const double *acc)
{
    if (!h || !dt || !gyro || !acc) return HV_ERR_INVALID;
    Ekf *e = &h->e;
    if (e->batch == 1) return predict_common(e, nullptr, nullptr, nullptr, dt[0], gyro, acc);   // immediates, no copy
    return predict_staged(e, 1, dt, gyro, acc);
}

int hv_ekf_predict_dev(hv_ekf *h, const double *dt_dev, const double *gyro_dev, const double *acc_dev)
{
    if (!h || !dt_dev || !gyro_dev || !acc_dev) return HV_ERR_INVALID;
    return predict_common(&h->e, dt_dev, gyro_dev, acc_dev, 0.0, nullptr, nullptr);
}

int hv_ekf_predict_n(hv_ekf *h, int n_samples, const double *dt, const double *gyro, const double *acc)
{
    if (!h || n_samples < 1 || n_samples > HV_EKF_MAX_PREDICT_SAMPLES || !dt || !gyro || !acc) return HV_ERR_INVALID;
    Ekf *e = &h->e;
    if (n_samples == 1 && e->batch == 1) return predict_common(e, nullptr, nullptr, nullptr, dt[0], gyro, acc);
    return predict_staged(e, n_samples, dt, gyro, acc);
}

int hv_ekf_predict_n_dev(hv_ekf *h, int n_samples, const double *dt_dev, const double *gyro_dev, const double *acc_dev)
{
    if (!h || n_samples < 1 || !dt_dev || !gyro_dev || !acc_dev) return HV_ERR_INVALID;
    return predict_common(&h->e, dt_dev, gyro_dev, acc_dev, 0.0, nullptr, nullptr, n_samples);
}

}  // extern "C"
