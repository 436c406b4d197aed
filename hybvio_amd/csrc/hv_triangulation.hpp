// The small steps of Triangulator::triangulate (src/odometry/triangulation.cpp) that more than one kernel file uses: the fused
// and the split triangulation fronts (vu_prepare.hip), the optical-flow predictor (flow_predict.hip) and the points-only tail of
// the full point cloud (full_cloud.hip). One statement of each, in the operation order of oracle/triangulation_oracle.c.
//
// No include guard and no namespace of its own, like hv_geometry.hpp, and included behind it (mm3, mmT3, mv3, mTv3, quat2rmat_d,
// pinv32): a translation unit includes it once, inside its anonymous namespace and behind its own contraction pragma, so the
// functions are compiled under the contraction mode of the file that uses them.

__device__ __forceinline__ void pos_ori(int i, int &pos, int &ori)                   // triangulation.cpp:989-998
{
    pos = i == 0 ? 0 : 20 + 7 * (i - 1);
    ori = i == 0 ? 6 : 20 + 7 * (i - 1) + 3;
}

[[maybe_unused]] __device__ __forceinline__ void inverse_depth(const double *p, double *ip, double *dip)   // :1004-1012
{
    const double iz = 1 / p[2];
    ip[0] = p[0] * iz; ip[1] = p[1] * iz; ip[2] = iz;
    dip[0] = iz; dip[1] = 0; dip[2] = -ip[0] * iz; dip[3] = 0; dip[4] = iz; dip[5] = -ip[1] * iz; dip[6] = 0; dip[7] = 0; dip[8] = -ip[2] * iz;
}

// exact solve of the symmetric 3x3 system through the adjugate (ETE.ldlt().solve); returns det
[[maybe_unused]] __device__ __forceinline__ double inv3sym(const double *M, double *inv)
{
    const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
    const double det = M[0] * c00 + M[1] * c01 + M[2] * c02, id = 1.0 / det;
    inv[0] = c00 * id; inv[1] = (M[2] * M[7] - M[1] * M[8]) * id; inv[2] = (M[1] * M[5] - M[2] * M[4]) * id;
    inv[3] = c01 * id; inv[4] = (M[0] * M[8] - M[2] * M[6]) * id; inv[5] = (M[2] * M[3] - M[0] * M[5]) * id;
    inv[6] = c02 * id; inv[7] = (M[1] * M[6] - M[0] * M[7]) * id; inv[8] = (M[0] * M[4] - M[1] * M[3]) * id;
    return det;
}
// the 1-norm of a 3x3: rcond = 1 / (|E'E|_1 |(E'E)^-1|_1) (:313-315)
[[maybe_unused]] __device__ __forceinline__ double norm1_3(const double *M)
{
    double best = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) best = fmax(best, fabs(M[c]) + fabs(M[3 + c]) + fabs(M[6 + c]));
    return best;
}

// One observation of a Gauss-Newton iteration (:216-246): h = C (pfi_x, pfi_y, 1)' + pfi_z t of the pose whose constants are
// C = R_i R_0' and t = R_i (p_0 - p_i), the 2 x 3 block E of the Jacobian and the reprojection error of the measured point y.
// Returns 1 / h_z, which the derivative sums of the visit fronts use again.
[[maybe_unused]] __device__ __forceinline__ double gn_observation(const double *C, const double *t, const double *pfi, const double *y, double *h,
                                                                  double *E, double *err)
{
    const double pfiab[3] = {pfi[0], pfi[1], 1.0};
    mv3(C, pfiab, h);
#pragma unroll
    for (int k = 0; k < 3; ++k) h[k] += pfi[2] * t[k];
    const double ih2 = 1.0 / h[2], ih2sq = ih2 * ih2;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int c = 0; c < 2; ++c) E[3 * r + c] = -ih2 * C[3 * r + c] + h[r] * ih2sq * C[6 + c];
        E[3 * r + 2] = -t[r] * ih2 + h[r] * ih2sq * t[2];
        err[r] = y[r] - h[r] * ih2;
    }
    return ih2;
}

// extractCameraPoseTrail (:65-103) without the derivative matrices: o = p[3] R[9] of the camera T = imuToCamera (4 x 4 row-major) at
// the pose whose position and orientation start at m[ip] and m[io]
[[maybe_unused]] __device__ inline void camera_pose_pR(const double *m, int ip, int io, const double *T, double *o)
{
    const double Ric[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]}, base[3] = {T[3], T[7], T[11]};
    const double q[4] = {m[io], m[io + 1], m[io + 2], m[io + 3]};
    double Rw[9], dRw[36], R[9], t3[3];
    quat2rmat_d(q, Rw, dRw);
    mm3(Ric, Rw, R);
    mTv3(R, base, t3);
    for (int j = 0; j < 3; ++j) o[j] = m[ip + j] - t3[j];
    for (int j = 0; j < 9; ++j) o[3 + j] = R[j];
}

// triangulateWithTwoCameras without derivatives (:610-646) between the poses P0 and P1 (p[3] R[9] each)
[[maybe_unused]] __device__ inline void triangulate_two(const double *P0, const double *P1, const double *ip0, const double *ip1, double *pf)
{
    const double *R0 = P0 + 3, *R1 = P1 + 3;
    double C[9], d01[3], b[3];
    mmT3(R0, R1, C);
    for (int k = 0; k < 3; ++k) d01[k] = P1[k] - P0[k];
    mv3(R0, d01, b);
    const double v0[3] = {ip0[0], ip0[1], 1.0}, v1[3] = {ip1[0], ip1[1], 1.0};
    const double n0 = sqrt(v0[0] * v0[0] + v0[1] * v0[1] + v0[2] * v0[2]), n1 = sqrt(v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2]);
    const double vn0[3] = {v0[0] / n0, v0[1] / n0, v0[2] / n0}, vn1[3] = {v1[0] / n1, v1[1] / n1, v1[2] / n1};
    double Cvn1[3], A[6], iA[6];
    mv3(C, vn1, Cvn1);
    for (int r = 0; r < 3; ++r) { A[2 * r] = vn0[r]; A[2 * r + 1] = -Cvn1[r]; }
    pinv32(A, iA);
    const double s0 = iA[0] * b[0] + iA[1] * b[1] + iA[2] * b[2];
    for (int k = 0; k < 3; ++k) pf[k] = s0 * vn0[k];
}
