// Small binary64 geometry shared by the kernels that read camera poses from the EKF mean (vu_prepare.hip, flow_predict.hip, output.hip,
// upright2p.hip) and by the RANSAC kernels (rot_ransac.hip, ransac5.hip, ransac3.hip, upright2p.hip): 3-vector and 3x3 products, odometry::util::quat2rmat /
// quat2rmat_d (src/odometry/util.cpp:10-47), rmat2quat, the inverse of a general 4x4 and the pseudo-inverse of a full-rank 3x2 matrix
// (src/odometry/triangulation.cpp:1000-1002). 3x3 and 4x4 matrices are row-major double[9] / double[16] (like
// oracle/triangulation_oracle.c).
//
// No include guard and no namespace of its own, on purpose: a translation unit includes it once, inside its anonymous namespace and
// behind its own `#pragma clang fp contract(...)`, so the functions are compiled under the contraction mode of the file that uses
// them (vu_prepare.hip: fast; the others: the build's -ffp-contract=off).

// (a . b) with the first two products added first; a x b
__device__ __forceinline__ double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void mm3(const double *A, const double *B, double *C)
{
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
__device__ __forceinline__ void mmT3(const double *A, const double *B, double *C)   // A B^T
{
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[3 * c] + A[3 * r + 1] * B[3 * c + 1] + A[3 * r + 2] * B[3 * c + 2];
}
__device__ __forceinline__ void mv3(const double *A, const double *x, double *y)
{
#pragma unroll
    for (int r = 0; r < 3; ++r) y[r] = A[3 * r] * x[0] + A[3 * r + 1] * x[1] + A[3 * r + 2] * x[2];
}
__device__ __forceinline__ void mTv3(const double *A, const double *x, double *y)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) y[c] = A[c] * x[0] + A[3 + c] * x[1] + A[6 + c] * x[2];
}

__device__ __forceinline__ void quat2rmat(const double *q, double *R)                // util.cpp:10-26
{
    R[0] = q[0] * q[0] + q[1] * q[1] - q[2] * q[2] - q[3] * q[3]; R[1] = 2 * q[1] * q[2] - 2 * q[0] * q[3]; R[2] = 2 * q[1] * q[3] + 2 * q[0] * q[2];
    R[3] = 2 * q[1] * q[2] + 2 * q[0] * q[3]; R[4] = q[0] * q[0] - q[1] * q[1] + q[2] * q[2] - q[3] * q[3]; R[5] = 2 * q[2] * q[3] - 2 * q[0] * q[1];
    R[6] = 2 * q[1] * q[3] - 2 * q[0] * q[2]; R[7] = 2 * q[2] * q[3] + 2 * q[0] * q[1]; R[8] = q[0] * q[0] - q[1] * q[1] - q[2] * q[2] + q[3] * q[3];
}
// odometry::util::toCameraToWorld (util.cpp:144-158) in its two factors, shared by flow_predict.hip and upright2p.hip: imuToWorld =
// [rot' | position] of the pose at m[ip], m[io] (row-major 4x4), and one entry of the product imuToWorld * cameraToImu with the four
// terms added left to right (the caller supplies cameraToImu: Eigen's inverse is not restated)
[[maybe_unused]] __device__ inline void imu_to_world(const double *m, int ip, int io, double *out)
{
    double R[9];
    quat2rmat(m + io, R);
    const double i2w[16] = {R[0], R[3], R[6], m[ip], R[1], R[4], R[7], m[ip + 1], R[2], R[5], R[8], m[ip + 2], 0.0, 0.0, 0.0, 1.0};
    for (int j = 0; j < 16; ++j) out[j] = i2w[j];
}
[[maybe_unused]] __device__ __forceinline__ double mm4_entry(const double *A, const double *B, int r, int c)
{
    return ((A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]) + A[4 * r + 3] * B[12 + c];
}
[[maybe_unused]] __device__ void quat2rmat_d(const double *q, double *R, double *dR /* [4][9] */)    // util.cpp:10-47: R as above
{
    quat2rmat(q, R);
    const double a = 2 * q[0], b = 2 * q[1], c = 2 * q[2], d = 2 * q[3];
    const double d0[9] = {a, -d, c, d, a, -b, -c, b, a}, d1[9] = {b, c, d, c, -b, -a, d, a, -b};
    const double d2[9] = {-c, b, a, b, c, d, -a, d, -c}, d3[9] = {-d, -a, b, a, -d, c, b, c, d};
#pragma unroll
    for (int k = 0; k < 9; ++k) { dR[k] = d0[k]; dR[9 + k] = d1[k]; dR[18 + k] = d2[k]; dR[27 + k] = d3[k]; }
}

// odometry::util::rmat2quat = Eigen::Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>):
// R row-major, q = (w, x, y, z). The sign of q is the branch's, not the filter's.
[[maybe_unused]] __device__ void rmat2quat(const double *R, double *q)
{
    double t = (R[0] + R[4]) + R[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (R[7] - R[5]) * t; q[2] = (R[2] - R[6]) * t; q[3] = (R[3] - R[1]) * t;
    } else {
        // i = the largest diagonal entry in Eigen's order, j = (i + 1) % 3, k = (j + 1) % 3; written as selections among values
        // read at constant indices, so that no array is indexed by i (a dynamic index puts R and q in scratch)
        const double r00 = R[0], r01 = R[1], r02 = R[2], r10 = R[3], r11 = R[4], r12 = R[5], r20 = R[6], r21 = R[7], r22 = R[8];
        int i = 0;
        if (r11 > r00) i = 1;
        if (r22 > (i ? r11 : r00)) i = 2;
        const double mii = i == 0 ? r00 : i == 1 ? r11 : r22, mjj = i == 0 ? r11 : i == 1 ? r22 : r00, mkk = i == 0 ? r22 : i == 1 ? r00 : r11;
        const double mkj = i == 0 ? r21 : i == 1 ? r02 : r10, mjk = i == 0 ? r12 : i == 1 ? r20 : r01;
        const double mji = i == 0 ? r10 : i == 1 ? r21 : r02, mij = i == 0 ? r01 : i == 1 ? r12 : r20;
        const double mki = i == 0 ? r20 : i == 1 ? r01 : r12, mik = i == 0 ? r02 : i == 1 ? r10 : r21;
        t = sqrt(((mii - mjj) - mkk) + 1.0);
        const double qi = 0.5 * t;
        t = 0.5 / t;
        const double qj = (mji + mij) * t, qk = (mki + mik) * t;
        q[0] = (mkj - mjk) * t;
        q[1] = i == 0 ? qi : i == 1 ? qk : qj;
        q[2] = i == 1 ? qi : i == 2 ? qk : qj;
        q[3] = i == 2 ? qi : i == 0 ? qk : qj;
    }
}

// inverse of a general 4x4 (row-major) through its cofactors, grouped by the 2x2 minors of the upper and the lower row pair; the
// determinant is inverted once (as pinv32 and the 3x3 inverses of the RANSAC kernels do)
[[maybe_unused]] __device__ void inv4(const double *a, double *b)
{
    const double s0 = a[0] * a[5] - a[4] * a[1], s1 = a[0] * a[6] - a[4] * a[2], s2 = a[0] * a[7] - a[4] * a[3];
    const double s3 = a[1] * a[6] - a[5] * a[2], s4 = a[1] * a[7] - a[5] * a[3], s5 = a[2] * a[7] - a[6] * a[3];
    const double c5 = a[10] * a[15] - a[14] * a[11], c4 = a[9] * a[15] - a[13] * a[11], c3 = a[9] * a[14] - a[13] * a[10];
    const double c2 = a[8] * a[15] - a[12] * a[11], c1 = a[8] * a[14] - a[12] * a[10], c0 = a[8] * a[13] - a[12] * a[9];
    const double id = 1.0 / (s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0);
    b[0] = (a[5] * c5 - a[6] * c4 + a[7] * c3) * id;
    b[1] = (-a[1] * c5 + a[2] * c4 - a[3] * c3) * id;
    b[2] = (a[13] * s5 - a[14] * s4 + a[15] * s3) * id;
    b[3] = (-a[9] * s5 + a[10] * s4 - a[11] * s3) * id;
    b[4] = (-a[4] * c5 + a[6] * c2 - a[7] * c1) * id;
    b[5] = (a[0] * c5 - a[2] * c2 + a[3] * c1) * id;
    b[6] = (-a[12] * s5 + a[14] * s2 - a[15] * s1) * id;
    b[7] = (a[8] * s5 - a[10] * s2 + a[11] * s1) * id;
    b[8] = (a[4] * c4 - a[5] * c2 + a[7] * c0) * id;
    b[9] = (-a[0] * c4 + a[1] * c2 - a[3] * c0) * id;
    b[10] = (a[12] * s4 - a[13] * s2 + a[15] * s0) * id;
    b[11] = (-a[8] * s4 + a[9] * s2 - a[11] * s0) * id;
    b[12] = (-a[4] * c3 + a[5] * c1 - a[6] * c0) * id;
    b[13] = (a[0] * c3 - a[1] * c1 + a[2] * c0) * id;
    b[14] = (-a[12] * s3 + a[13] * s1 - a[14] * s0) * id;
    b[15] = (a[8] * s3 - a[9] * s1 + a[10] * s0) * id;
}

// pseudo-inverse of the full-rank 3x2 A (row-major): (A'A)^-1 A', the determinant inverted once
[[maybe_unused]] __device__ void pinv32(const double *A, double *iA)
{
    const double a = A[0] * A[0] + A[2] * A[2] + A[4] * A[4], b = A[0] * A[1] + A[2] * A[3] + A[4] * A[5];
    const double d = A[1] * A[1] + A[3] * A[3] + A[5] * A[5], idet = 1.0 / (a * d - b * b);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        iA[c] = (d * A[2 * c] - b * A[2 * c + 1]) * idet;
        iA[3 + c] = (-b * A[2 * c] + a * A[2 * c + 1]) * idet;
    }
}
