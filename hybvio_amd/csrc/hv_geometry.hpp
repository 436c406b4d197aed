// Small binary64 geometry shared by the kernels that read camera poses from the EKF mean (vu_prepare.hip, flow_predict.hip) and by the
// RANSAC kernels (rot_ransac.hip, ransac5.hip, ransac3.hip): 3-vector and 3x3 products, odometry::util::quat2rmat / quat2rmat_d
// (src/odometry/util.cpp:10-47) and the pseudo-inverse of a full-rank 3x2 matrix (src/odometry/triangulation.cpp:1000-1002). 3x3
// matrices are row-major double[9] (like oracle/triangulation_oracle.c).
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
[[maybe_unused]] __device__ void quat2rmat_d(const double *q, double *R, double *dR /* [4][9] */)    // util.cpp:10-47: R as above
{
    quat2rmat(q, R);
    const double a = 2 * q[0], b = 2 * q[1], c = 2 * q[2], d = 2 * q[3];
    const double d0[9] = {a, -d, c, d, a, -b, -c, b, a}, d1[9] = {b, c, d, c, -b, -a, d, a, -b};
    const double d2[9] = {-c, b, a, b, c, d, -a, d, -c}, d3[9] = {-d, -a, b, a, -d, c, b, c, d};
#pragma unroll
    for (int k = 0; k < 9; ++k) { dR[k] = d0[k]; dR[9 + k] = d1[k]; dR[18 + k] = d2[k]; dR[27 + k] = d3[k]; }
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
