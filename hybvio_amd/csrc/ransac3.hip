// Stereo RANSAC3 track filter: doRansac3 without Theia and the RANSAC3 branch of RansacPipeline::compute.
//
// Reference: src/tracker/ransac_pipeline.cpp:95-151 (compute), :218-272 (doRansac3), src/odometry/triangulation.cpp:711-764
// (triangulateStereoFeatureIdp), src/tracker/camera.cpp:471-476 (normalizePixel). Theia's EstimateCalibratedAbsolutePose is
// not in the tree: the sample-consensus loop follows a recollection of it and the minimal solver is Grunert's P3P with
// Ferrari's quartic, both stated operation by operation in tests/ransac3_restatement.py (divergences: DESIGN.md 3.14).
//
// One 256-thread workgroup per point set:
//   a. the correspondences: TRACKED features in feature order, three normalizePixel calls and the triangulation per lane,
//      survivors compacted with ballots (order kept), world points and image points in LDS
//   then rounds of up to 64 iterations, until the serial loop has ended (the common case ends at minIterations = 50):
//   b. lane 0 replays the sampler's partial shuffle (positions 0..2 in registers, the rest of the index vector in LDS);
//      each sample is handed to the solver in ascending index order
//   c. one P3P per lane (64 lanes), up to four (R, c) per hypothesis into LDS
//   d. one lane per (hypothesis, solution): cost and inlier count over all correspondences, added in order
//   e. lane 0 replays the loop's rule over the stored costs: strict `<`, adaptive limit
//   f. every lane classifies its correspondences with the best model; statuses, pose, summary, the tail of compute
// Arithmetic is binary64 in the operation order of the restatement (the library is built without FMA contraction).
#include "hv_camera.hpp"
#include "hv_internal.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace hv {
namespace {

constexpr int R3_THREADS = 256, R3_WAVES = R3_THREADS / 64;
constexpr int R3_MAX_PTS = 1024;
constexpr int R3_CHUNK = 64;                       // iterations per round; R3_CHUNK * 4 solutions = one lane each in phase d
static_assert(R3_CHUNK * 4 == R3_THREADS, "one lane per (hypothesis, solution)");

struct R3Args {
    int max_points, max_iters, min_iters, use_mle, cap, tail;
    const int *n_points;
    const float *pl, *pr, *cl;            // previous-left, previous-right, current-left corners [sets][max_points][2]
    const uint32_t *draws;                // [sets][3 * max_iters] raw std::mt19937 outputs
    int *status;                          // [sets][max_points] Feature::Status in/out (TRACKED selects)
    const int *r2_summary;                // tail: RANSAC2's {bestInlierCount, visited}
    int *result;                          // tail: [sets][2] {type, inlierCount}
    double *score;                        // tail: [sets]
    double *pose;                         // [sets][12] or NULL
    int *summary;                         // [sets][4] or NULL
    double thr, logp;
    double T[16];                         // secondToFirstCamera, row-major
    hv_camera_model cam0, cam1;
};

__host__ __device__ constexpr size_t lds_bytes(int max_points)
{
    return sizeof(double) * ((size_t)5 * max_points + (size_t)R3_THREADS * 12 + R3_THREADS + 12) +
           sizeof(int) * ((size_t)4 * max_points + (max_points + 63) / 64 + 1 + 3 * R3_CHUNK * 2 + R3_THREADS + 16);
}

// ComputeMaxIterations for a sample of 3 (restatement: compute_max_iterations)
__host__ __device__ inline int max_iterations_for(double ratio, double logp, int min_it, int max_it)
{
    if (ratio <= 0.0) return max_it;
    if (ratio == 1.0) return min_it;
    const double lp = log(1.0 - (ratio * ratio) * ratio) - DBL_EPSILON;
    double v = ceil(logp / lp);
    v = v < (double)min_it ? (double)min_it : v;
    v = v > (double)max_it ? (double)max_it : v;
    return (int)v;
}

__device__ __forceinline__ double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

// triangulateStereoFeatureIdp (triangulation.cpp:711-764) and world_point = (idp.x, idp.y, 1) / idp.z (ransac_pipeline.cpp:244)
__device__ bool triangulate_world(const double *T, double fu, double fv, double su, double sv, double *X)
{
    const double f0[3] = {su, sv, 1.0}, f1[3] = {fu, fv, 1.0};
    const double n0 = sqrt(dot3(f0, f0)), n1 = sqrt(dot3(f1, f1));
    const double f0h[3] = {f0[0] / n0, f0[1] / n0, f0[2] / n0}, f1h[3] = {f1[0] / n1, f1[1] / n1, f1[2] / n1};
    const double t[3] = {T[3], T[7], T[11]};
    double Rf[3], a[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) Rf[i] = (T[4 * i] * f0h[0] + T[4 * i + 1] * f0h[1]) + T[4 * i + 2] * f0h[2];
    double p[3], q[3], r[3];
    cross3(Rf, f1h, p); cross3(Rf, t, q); cross3(f1h, t, r);
    const double pn = sqrt(dot3(p, p)), qn = sqrt(dot3(q, q)), rn = sqrt(dot3(r, r));
    const double l0 = rn / pn, l1 = qn / pn, w = qn / (qn + rn);
    double pf[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) pf[i] = w * (t[i] + l0 * (Rf[i] + f1h[i]));
#pragma unroll
    for (int i = 0; i < 3; ++i) a[i] = ((l0 * T[4 * i]) * f0h[0] + (l0 * T[4 * i + 1]) * f0h[1]) + (l0 * T[4 * i + 2]) * f0h[2];
    const double b[3] = {l1 * f1h[0], l1 * f1h[1], l1 * f1h[2]};
    double v0[3], v1[3], v2[3], v3[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v0[i] = (t[i] + a[i]) - b[i]; v1[i] = (t[i] + a[i]) + b[i]; v2[i] = (t[i] - a[i]) - b[i]; v3[i] = (t[i] - a[i]) + b[i];
    }
    const double c0 = dot3(v0, v0), c1 = dot3(v1, v1), c2 = dot3(v2, v2), c3 = dot3(v3, v3);
    double mn = c2 < c1 ? c2 : c1;
    mn = c3 < mn ? c3 : mn;
    if (c0 > mn) return false;
    const double i0 = pf[0] / pf[2], i1 = pf[1] / pf[2], i2 = 1.0 / pf[2];
    X[0] = i0 / i2; X[1] = i1 / i2; X[2] = 1.0 / i2;
    return true;
}

// real roots of A4 x^4 + ... + A0 (restatement: quartic_real_roots) -> x[4] and ok[4] in LDS
__device__ void quartic_real_roots(double A4, double A3, double A2, double A1, double A0, double *x_out, int *ok_out)
{
    const double a = A3 / A4, b = A2 / A4, c = A1 / A4, d = A0 / A4;
    const double a2 = a * a;
    const double p = b - 0.375 * a2;
    const double q = (c - 0.5 * (a * b)) + 0.125 * (a2 * a);
    const double r = ((d - 0.25 * (a * c)) + 0.0625 * (a2 * b)) - 0.01171875 * (a2 * a2);
    const double k2 = p, k1 = 0.25 * (p * p) - r, k0 = -0.125 * (q * q);
    const double P = k1 - (k2 * k2) / 3.0;
    const double Q = ((2.0 * ((k2 * k2) * k2)) / 27.0 - (k2 * k1) / 3.0) + k0;
    const double D = 0.25 * (Q * Q) + ((P * P) * P) / 27.0;
    double m;
    if (D > 0) {
        const double sD = sqrt(D);
        m = cbrt(-0.5 * Q + sD) + cbrt(-0.5 * Q - sD);
    } else {
        const double Pn = P < 0 ? P : -1.0;
        double arg = ((3.0 * Q) / (2.0 * Pn)) * sqrt(-3.0 / Pn);
        arg = arg < -1.0 ? -1.0 : arg;
        arg = arg > 1.0 ? 1.0 : arg;
        m = (2.0 * sqrt(-Pn / 3.0)) * cos(acos(arg) / 3.0);
    }
    m = m - k2 / 3.0;
#pragma unroll 1
    for (int it = 0; it < 2; ++it) {
        const double fm = ((m + k2) * m + k1) * m + k0, dm = (3.0 * m + 2.0 * k2) * m + k1;
        if (dm != 0) m = m - fm / dm;
    }
    const bool ok = isfinite(m) && m > 0 && A4 != 0;
    const double s = sqrt(2.0 * (ok ? m : 1.0));
    const double h = 0.5 * p + m, g = q / (2.0 * s);
    const double d1 = s * s - 4.0 * (h + g), d2 = s * s - 4.0 * (h - g);
    const double r1 = sqrt(d1 >= 0 ? d1 : 0.0), r2 = sqrt(d2 >= 0 ? d2 : 0.0);
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const double y = k == 0 ? 0.5 * (s + r1) : k == 1 ? 0.5 * (s - r1) : k == 2 ? 0.5 * (-s + r2) : 0.5 * (-s - r2);
        double x = y - 0.25 * a;
#pragma unroll 1
        for (int it = 0; it < 3; ++it) {
            const double fx = (((x + a) * x + b) * x + c) * x + d, dx = ((4.0 * x + 3.0 * a) * x + 2.0 * b) * x + c;
            if (dx != 0) x = x - fx / dx;
        }
        x_out[k] = x;
        ok_out[k] = (ok && (k < 2 ? d1 >= 0 : d2 >= 0)) ? 1 : 0;
    }
}

__device__ __forceinline__ void frame3(const double *A, const double *B, const double *C, double *e1, double *e2, double *e3)
{
    const double d1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, d2[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    const double n1 = sqrt(dot3(d1, d1));
    e1[0] = d1[0] / n1; e1[1] = d1[1] / n1; e1[2] = d1[2] / n1;
    double w[3];
    cross3(e1, d2, w);
    const double n3 = sqrt(dot3(w, w));
    e3[0] = w[0] / n3; e3[1] = w[1] / n3; e3[2] = w[2] / n3;
    cross3(e3, e1, e2);
}

// Grunert's P3P (restatement: p3p): world points Pw[3][3], image points F[3][2] -> mod[4][12] (R row-major, c) and ok[4] in LDS;
// roots[4] is LDS scratch of this lane
__device__ void p3p_lane(const double (*Pw)[3], const double (*F)[2], double *roots, int *ok, double *mod)
{
    double j[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double u = F[k][0], v = F[k][1], n = sqrt((u * u + v * v) + 1.0);
        j[k][0] = u / n; j[k][1] = v / n; j[k][2] = 1.0 / n;
    }
    auto dist2 = [](const double *A, const double *B) {
        const double d[3] = {A[0] - B[0], A[1] - B[1], A[2] - B[2]};
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    };
    const double a2 = dist2(Pw[1], Pw[2]), b2 = dist2(Pw[0], Pw[2]), c2 = dist2(Pw[0], Pw[1]);
    const double ca = dot3(j[1], j[2]), cb = dot3(j[0], j[2]), cg = dot3(j[0], j[1]);
    const double q1 = (a2 - c2) / b2, q2 = (a2 + c2) / b2, q3 = (b2 - c2) / b2, q4 = (b2 - a2) / b2, ra = a2 / b2, rc = c2 / b2;
    const double ca2 = ca * ca, cb2 = cb * cb, cg2 = cg * cg;
    const double A4 = (q1 - 1.0) * (q1 - 1.0) - (4.0 * rc) * ca2;
    const double A3 = 4.0 * (((q1 * (1.0 - q1)) * cb - ((1.0 - q2) * ca) * cg) + ((2.0 * rc) * ca2) * cb);
    const double A2 = 2.0 * ((((((q1 * q1 - 1.0) + ((2.0 * (q1 * q1)) * cb2)) + (2.0 * q3) * ca2) - (((4.0 * q2) * ca) * cb) * cg) +
                             (2.0 * q4) * cg2));
    const double A1 = 4.0 * (((-(q1 * (1.0 + q1))) * cb + ((2.0 * ra) * cg2) * cb) - ((1.0 - q2) * ca) * cg);
    const double A0 = (1.0 + q1) * (1.0 + q1) - (4.0 * ra) * cg2;
    quartic_real_roots(A4, A3, A2, A1, A0, roots, ok);
    double e[3][3];
    frame3(Pw[0], Pw[1], Pw[2], e[0], e[1], e[2]);
#pragma unroll 1
    for (int s = 0; s < 4; ++s) {
        double v = roots[s];
        double u = ((((q1 - 1.0) * (v * v) - ((2.0 * q1) * cb) * v) + 1.0) + q1) / (2.0 * (cg - v * ca));
#pragma unroll 1
        for (int it = 0; it < 2; ++it) {
            const double w = (1.0 + v * v) - (2.0 * v) * cb;
            const double f1 = ((1.0 + u * u) - (2.0 * u) * cg) - w * rc;
            const double f2 = ((u * u + v * v) - ((2.0 * u) * v) * ca) - w * ra;
            const double j11 = 2.0 * (u - cg), j12 = (-2.0 * (v - cb)) * rc;
            const double j21 = 2.0 * (u - v * ca), j22 = 2.0 * (v - u * ca) - (2.0 * (v - cb)) * ra;
            const double det = j11 * j22 - j12 * j21;
            if (isfinite(det) && det != 0) {
                const double un = u - (j22 * f1 - j12 * f2) / det, vn = v - (j11 * f2 - j21 * f1) / det;
                u = un; v = vn;
            }
        }
        const double s1 = sqrt(b2 / ((1.0 + v * v) - (2.0 * v) * cb));
        const double s2 = u * s1, s3 = v * s1;
        const double Y0[3] = {s1 * j[0][0], s1 * j[0][1], s1 * j[0][2]}, Y1[3] = {s2 * j[1][0], s2 * j[1][1], s2 * j[1][2]},
                     Y2[3] = {s3 * j[2][0], s3 * j[2][1], s3 * j[2][2]};
        double g[3][3];
        frame3(Y0, Y1, Y2, g[0], g[1], g[2]);
        double R[3][3];
        bool fin = ok[s] != 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                R[i][k] = (g[0][i] * e[0][k] + g[1][i] * e[1][k]) + g[2][i] * e[2][k];
                fin = fin && isfinite(R[i][k]);
            }
        double *M = mod + 12 * s;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double c = Pw[0][k] - ((R[0][k] * Y0[0] + R[1][k] * Y0[1]) + R[2][k] * Y0[2]);
            fin = fin && isfinite(c);
            M[9 + k] = c;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) M[3 * i + k] = R[i][k];
        ok[s] = fin ? 1 : 0;
    }
}

// |(R (X - c)).hnormalized() - feature|^2 (restatement: residuals)
__device__ __forceinline__ double residual(const double *M, double X0, double X1, double X2, double fu, double fv)
{
    const double d0 = X0 - M[9], d1 = X1 - M[10], d2 = X2 - M[11];
    const double p0 = (M[0] * d0 + M[1] * d1) + M[2] * d2, p1 = (M[3] * d0 + M[4] * d1) + M[5] * d2,
                 p2 = (M[6] * d0 + M[7] * d1) + M[8] * d2;
    const double e0 = p0 / p2 - fu, e1 = p1 / p2 - fv;
    return e0 * e0 + e1 * e1;
}

__global__ __launch_bounds__(R3_THREADS) void ransac3_kernel(R3Args a)
{
    extern __shared__ __attribute__((aligned(16))) double r3_lds[];
    const int set = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int MP = a.max_points;
    double *wx = r3_lds, *wy = wx + MP, *wz = wy + MP, *fu = wz + MP, *fv = fu + MP;
    double *s_mod = fv + MP;                                   // [R3_THREADS][12]
    double *s_cost = s_mod + R3_THREADS * 12;                  // [R3_THREADS] (phase c: the quartic's roots)
    double *s_best = s_cost + R3_THREADS;                      // [12]
    int *s_map = reinterpret_cast<int *>(s_best + 12);         // tracked k -> feature
    int *s_vmap = s_map + MP, *s_st = s_vmap + MP, *s_idx = s_st + MP, *s_chunk = s_idx + MP;
    int *s_tri = s_chunk + (MP + 63) / 64 + 1;                 // [R3_CHUNK][3]
    unsigned *s_draw = reinterpret_cast<unsigned *>(s_tri + 3 * R3_CHUNK);
    int *s_cnt = reinterpret_cast<int *>(s_draw + 3 * R3_CHUNK);   // [R3_THREADS] inlier count, -1 = no model
    int *s_ctl = s_cnt + R3_THREADS;                           // [16]

    __shared__ hv_camera_model s_cam[2];
    __shared__ double s_T[16];
    {
        static_assert(sizeof(hv_camera_model) % 4 == 0, "word copy");
        constexpr int W = (int)(sizeof(hv_camera_model) / 4);
        const int *src0 = reinterpret_cast<const int *>(&a.cam0), *src1 = reinterpret_cast<const int *>(&a.cam1);
        int *dst = reinterpret_cast<int *>(s_cam);
        for (int i = tid; i < 2 * W; i += R3_THREADS) dst[i] = i < W ? src0[i] : src1[i - W];
        if (tid < 16) s_T[tid] = a.T[tid];
        __syncthreads();
    }
    const int n_all = min(max(a.n_points[set], 0), MP);
    const float *pl = a.pl + (size_t)set * MP * 2, *pr = a.pr + (size_t)set * MP * 2, *cl = a.cl + (size_t)set * MP * 2;
    int *ts = a.status + (size_t)set * MP;

    auto compact = [&](auto pred, int *out, int count_in) -> int {
        const int nch = (count_in + 63) / 64;
        for (int ch = wave; ch < nch; ch += R3_WAVES) {
            const int i = ch * 64 + lane;
            const unsigned long long m = __ballot(i < count_in && pred(i));
            if (lane == 0) s_chunk[ch] = __popcll(m);
        }
        __syncthreads();
        if (tid == 0) {
            int acc = 0;
            for (int ch = 0; ch < nch; ++ch) { const int cnt = s_chunk[ch]; s_chunk[ch] = acc; acc += cnt; }
            s_chunk[nch] = acc;
        }
        __syncthreads();
        const int total = s_chunk[nch];
        for (int ch = wave; ch < nch; ch += R3_WAVES) {
            const int i = ch * 64 + lane;
            const bool on = i < count_in && pred(i);
            const unsigned long long m = __ballot(on);
            if (on) out[s_chunk[ch] + __popcll(m & ((1ull << lane) - 1ull))] = i;
        }
        __syncthreads();
        return total;
    };
    // ---- a. the correspondences (ransac_pipeline.cpp:231-251) ----
    const int n = compact([&](int i) { return ts[i] == 0; }, s_map, n_all);
    for (int k = tid; k < n; k += R3_THREADS) {
        const int src = s_map[k];
        double r0[3], r1[3], r2[3], X[3];
        bool ok = pixel_to_ray(s_cam[0], (double)pl[2 * src], (double)pl[2 * src + 1], r0) && r0[2] > 0;
        ok = ok && pixel_to_ray(s_cam[1], (double)pr[2 * src], (double)pr[2 * src + 1], r1) && r1[2] > 0;
        ok = ok && pixel_to_ray(s_cam[0], (double)cl[2 * src], (double)cl[2 * src + 1], r2) && r2[2] > 0;
        ok = ok && triangulate_world(s_T, r0[0] / r0[2], r0[1] / r0[2], r1[0] / r1[2], r1[1] / r1[2], X);
        s_st[k] = ok ? 1 : 0;
        if (ok) { wx[k] = X[0]; wy[k] = X[1]; wz[k] = X[2]; fu[k] = r2[0] / r2[2]; fv[k] = r2[1] / r2[2]; }
    }
    __syncthreads();
    const int m = compact([&](int k) { return s_st[k] != 0; }, s_vmap, n);
    {
        // gather the correspondences to the front (reads all done before the barrier, writes after)
        static_assert(R3_MAX_PTS <= 4 * R3_THREADS, "four points per thread");
        double hv[4][5];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = tid + q * R3_THREADS;
            if (j < m) { const int k = s_vmap[j]; hv[q][0] = wx[k]; hv[q][1] = wy[k]; hv[q][2] = wz[k]; hv[q][3] = fu[k]; hv[q][4] = fv[k]; }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = tid + q * R3_THREADS;
            if (j < m) { wx[j] = hv[q][0]; wy[j] = hv[q][1]; wz[j] = hv[q][2]; fu[j] = hv[q][3]; fv[j] = hv[q][4]; }
        }
    }
    for (int k = tid; k < n; k += R3_THREADS) s_st[k] = 3;                   // :235
    for (int j = tid; j < m; j += R3_THREADS) s_idx[j] = j;
    if (tid == 0) { s_ctl[0] = 0; s_ctl[1] = a.cap; s_ctl[2] = -1; s_ctl[3] = 0; }   // iteration, limit, best iteration, inliers
    __syncthreads();

    const bool run = m >= 3;
    if (run) {
        int i0 = 0, i1 = 1, i2 = 2;                                          // lane 0: positions 0..2 of the index vector
        double best_cost = DBL_MAX;                                          // lane 0
        const uint32_t *draws = a.draws + (size_t)set * 3 * a.max_iters;
        for (;;) {
            const int it0 = s_ctl[0], limit = s_ctl[1];
            if (it0 >= limit) break;
            const int h = min(R3_CHUNK, a.cap - it0);
            if (tid < 3 * h) s_draw[tid] = draws[3 * it0 + tid];
            __syncthreads();
            // ---- b. the sampler: idx[i] <-> idx[i + raw % (m - i)], i = 0, 1, 2 ----
            if (tid == 0) {
                for (int k = 0; k < h; ++k) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const int j = i + (int)(s_draw[3 * k + i] % (unsigned)(m - i));
                        int &mine = i == 0 ? i0 : i == 1 ? i1 : i2;
                        if (j >= 3) { const int o = s_idx[j]; s_idx[j] = mine; mine = o; }
                        else { int &other = j == 0 ? i0 : j == 1 ? i1 : i2; const int o = other; other = mine; mine = o; }
                    }
                    // the solver's canonical order: ascending indices (a repeated triple repeats its models bit for bit)
                    const int lo = min(i0, min(i1, i2)), hi = max(i0, max(i1, i2));
                    s_tri[3 * k] = lo; s_tri[3 * k + 1] = i0 + i1 + i2 - lo - hi; s_tri[3 * k + 2] = hi;
                }
            }
            __syncthreads();
            // ---- c. one P3P per lane ----
            if (tid < h) {
                double Pw[3][3], F[3][2];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int s = s_tri[3 * tid + q];
                    Pw[q][0] = wx[s]; Pw[q][1] = wy[s]; Pw[q][2] = wz[s]; F[q][0] = fu[s]; F[q][1] = fv[s];
                }
                p3p_lane(Pw, F, s_cost + 4 * tid, s_cnt + 4 * tid, s_mod + 48 * tid);
            }
            __syncthreads();
            // ---- d. cost and inlier count of (hypothesis, solution) = lane ----
            {
                const bool have = (tid >> 2) < h && s_cnt[tid] != 0;
                double cost = 0.0;
                int cnt = -1;
                if (have) {
                    double M[12];
#pragma unroll
                    for (int i = 0; i < 12; ++i) M[i] = s_mod[12 * tid + i];
                    cnt = 0;
                    for (int j = 0; j < m; ++j) {
                        const double r = residual(M, wx[j], wy[j], wz[j], fu[j], fv[j]);
                        const bool in = r < a.thr;
                        cnt += in ? 1 : 0;
                        cost = cost + (in ? r : a.thr);
                    }
                    if (!a.use_mle) cost = (double)(m - cnt);
                }
                s_cnt[tid] = cnt; s_cost[tid] = cost;                        // (over the lane's own flag and root)
            }
            __syncthreads();
            // ---- e. the loop's rule over the stored costs ----
            if (tid == 0) {
                int it = it0, lim = limit;
                for (int k = 0; k < h && it < lim; ++k, ++it)
                    for (int s = 0; s < 4; ++s) {
                        const int w = 4 * k + s, cnt = s_cnt[w];
                        if (cnt >= 0 && s_cost[w] < best_cost) {
                            best_cost = s_cost[w];
                            for (int i = 0; i < 12; ++i) s_best[i] = s_mod[12 * w + i];
                            s_ctl[2] = it; s_ctl[3] = cnt;
                            const double ratio = (double)cnt / (double)m;
                            if (!(ratio < 3.0 / (double)m)) lim = min(max_iterations_for(ratio, a.logp, a.min_iters, a.max_iters), lim);
                        }
                    }
                s_ctl[0] = it; s_ctl[1] = lim;
            }
            __syncthreads();
        }
    }
    const int iters = s_ctl[0], best_it = s_ctl[2];
    const bool success = run && best_it >= 0;
    // ---- f. the best model's inliers go back to TRACKED (:265-268) ----
    if (tid == 0) s_ctl[4] = 0;
    __syncthreads();
    if (success) {
        double M[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) M[i] = s_best[i];
        int cnt = 0;
        for (int j = tid; j < m; j += R3_THREADS)
            if (residual(M, wx[j], wy[j], wz[j], fu[j], fv[j]) < a.thr) { s_st[s_vmap[j]] = 0; ++cnt; }
        if (cnt) atomicAdd(&s_ctl[4], cnt);
    }
    __syncthreads();
    const int count = s_ctl[4];
    if (tid == 0) {
        if (a.pose)
            for (int i = 0; i < 12; ++i) a.pose[12 * (size_t)set + i] = success ? s_best[i] : 0.0;
        if (a.summary) {
            int *sm = a.summary + 4 * (size_t)set;
            sm[0] = count; sm[1] = success ? best_it : -1; sm[2] = run ? iters : 0; sm[3] = m;
        }
    }
    if (a.tail && !success) {                                                // SKIPPED: every track is cleared (:139-144)
        for (int i = tid; i < n_all; i += R3_THREADS) ts[i] = 3;
    } else {
        for (int k = tid; k < n; k += R3_THREADS) ts[s_map[k]] = s_st[k];
    }
    if (a.tail && tid == 0) {
        a.result[2 * (size_t)set] = success ? 2 : 0;
        a.result[2 * (size_t)set + 1] = count;
        const int r2count = n >= 2 ? a.r2_summary[2 * set] : 0;              // doRansac2 does not run below two tracks (:210)
        a.score[set] = n ? (double)r2count / (double)n : 0.0;
    }
}

// the host-side checks, made before the context is looked at
int check_params(const hv_ransac3_params *p, int max_points, int n_sets)
{
    if (!p || !(p->ransac3FailureProbability > 0 && p->ransac3FailureProbability < 1) || !(p->ransac3ErrorThresh > 0) ||
        p->ransac3MaxIterations < 1 || p->ransac3MinIterations > p->ransac3MaxIterations ||
        !(p->ransacMinInlierFraction >= 0 && p->ransacMinInlierFraction <= 1) || max_points < 1 || n_sets < 0)
        return HV_ERR_INVALID;
    if (max_points > R3_MAX_PTS || p->ransac3MaxIterations > HV_RANSAC3_MAX_ITERS || n_sets > 65535) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}

void fill_common(R3Args &a, const hv_ransac3_params *p, int max_points, const hv_camera_model *cam0, const hv_camera_model *cam1,
                 const double *second_to_first)
{
    a.max_points = max_points; a.max_iters = p->ransac3MaxIterations; a.min_iters = p->ransac3MinIterations;
    a.use_mle = p->ransac3UseMle ? 1 : 0;
    a.thr = p->ransac3ErrorThresh; a.logp = std::log(p->ransac3FailureProbability);
    a.cap = std::min(a.max_iters, max_iterations_for(p->ransacMinInlierFraction, a.logp, a.min_iters, a.max_iters));
    for (int i = 0; i < 16; ++i) a.T[i] = second_to_first[i];
    a.cam0 = *cam0; a.cam1 = *cam1;
}

int launch(Ctx *c, int n_sets, const R3Args &a)
{
    hipLaunchKernelGGL(ransac3_kernel, dim3((unsigned)n_sets), dim3(R3_THREADS), lds_bytes(a.max_points), c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

}  // namespace

int ransac3_init(Ctx *c)
{
    HV_HIP(c, set_lds_limit(ransac3_kernel, lds_bytes(R3_MAX_PTS)));
    return HV_OK;
}

}  // namespace hv

using hv::Ctx;

extern "C" {

void hv_ransac3_default_params(hv_ransac3_params *p)
{
    if (!p) return;
    p->ransac3ErrorThresh = 1e-4;                 // codegen/parameter_definitions.c:292
    p->ransac3FailureProbability = 1e-4;          // :293
    p->ransac3MaxIterations = 500;                // :294
    p->ransac3MinIterations = 50;                 // :295
    p->ransac3UseMle = 1;                         // :296
    p->ransacMinInlierFraction = 0.3;             // :282
}

int hv_ransac3_batch_dev(hv_ctx *h, const hv_ransac3_params *p, int n_sets, int max_points, const int *n_points_dev,
                         const float *prev_left_dev, const float *prev_right_dev, const float *cur_left_dev,
                         const hv_camera_model *camera0, const hv_camera_model *camera1, const double *second_to_first,
                         const uint32_t *draws_dev, int *status_dev, double *pose_dev, int *summary_dev)
{
    if (const int rc = hv::check_params(p, max_points, n_sets)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c || !camera0 || !camera1 || !second_to_first) return HV_ERR_INVALID;
    if (n_sets > 0 && (!n_points_dev || !prev_left_dev || !prev_right_dev || !cur_left_dev || !draws_dev || !status_dev)) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    hv::R3Args a{};
    hv::fill_common(a, p, max_points, camera0, camera1, second_to_first);
    a.n_points = n_points_dev; a.pl = prev_left_dev; a.pr = prev_right_dev; a.cl = cur_left_dev; a.draws = draws_dev;
    a.status = status_dev; a.pose = pose_dev; a.summary = summary_dev;
    hv::ScopedKernelTime tm(c, HV_K_RANSAC3);
    return hv::launch(c, n_sets, a);
}

int hv_ransac3_lk_batch_dev(hv_ctx *h, const hv_ransac3_params *p, int n_sets, int max_points, const int *n_points_dev,
                            const float *prev_left_dev, const float *prev_right_dev, const float *cur_left_dev,
                            int *track_status_dev, const int *r2_summary_dev, const hv_camera_model *camera0,
                            const hv_camera_model *camera1, const double *second_to_first, const uint32_t *draws_dev,
                            int *result_dev, double *score_dev, double *pose_dev, int *summary_dev)
{
    if (const int rc = hv::check_params(p, max_points, n_sets)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c || !camera0 || !camera1 || !second_to_first) return HV_ERR_INVALID;
    if (n_sets > 0 && (!n_points_dev || !prev_left_dev || !prev_right_dev || !cur_left_dev || !draws_dev || !track_status_dev ||
                       !r2_summary_dev || !result_dev || !score_dev))
        return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    hv::R3Args a{};
    hv::fill_common(a, p, max_points, camera0, camera1, second_to_first);
    a.n_points = n_points_dev; a.pl = prev_left_dev; a.pr = prev_right_dev; a.cl = cur_left_dev; a.draws = draws_dev;
    a.status = track_status_dev; a.r2_summary = r2_summary_dev; a.result = result_dev; a.score = score_dev; a.tail = 1;
    a.pose = pose_dev; a.summary = summary_dev;
    hv::ScopedKernelTime tm(c, HV_K_RANSAC3);
    return hv::launch(c, n_sets, a);
}

int hv_ransac3(hv_ctx *h, const hv_ransac3_params *p, int n, const float *prev_left_xy, const float *prev_right_xy,
               const float *cur_left_xy, const hv_camera_model *camera0, const hv_camera_model *camera1,
               const double *second_to_first, const uint32_t *draws, int *status, double *pose, int *summary)
{
    if (n < 0) return HV_ERR_INVALID;
    if (const int rc = hv::check_params(p, std::max(n, 1), 1)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c || (n > 0 && (!prev_left_xy || !prev_right_xy || !cur_left_xy || !status)) || !camera0 || !camera1 || !second_to_first || !draws)
        return HV_ERR_INVALID;
    const int mp = std::max(n, 1);
    const size_t nd = 3 * (size_t)p->ransac3MaxIterations;
    hv::Stage s(c);
    const auto o_pl = s.take<float>(2 * (size_t)mp), o_pr = s.take<float>(2 * (size_t)mp), o_cl = s.take<float>(2 * (size_t)mp);
    const auto o_n = s.take<int>(1), o_st = s.take<int>(mp), o_sum = s.take<int>(4);
    const auto o_dr = s.take<uint32_t>(nd);
    const auto o_pose = s.take<double>(12);
    int rc = s.reserve();
    if (rc != HV_OK) return rc;
    float *d_pl = s.at(o_pl), *d_pr = s.at(o_pr), *d_cl = s.at(o_cl);
    int *d_n = s.at(o_n), *d_st = s.at(o_st), *d_sum = s.at(o_sum);
    uint32_t *d_dr = s.at(o_dr);
    double *d_pose = s.at(o_pose);
    if (n > 0) {
        HV_HIP(c, hipMemcpyAsync(d_pl, prev_left_xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice, c->stream));
        HV_HIP(c, hipMemcpyAsync(d_pr, prev_right_xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice, c->stream));
        HV_HIP(c, hipMemcpyAsync(d_cl, cur_left_xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice, c->stream));
        HV_HIP(c, hipMemcpyAsync(d_st, status, sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    }
    HV_HIP(c, hipMemcpyAsync(d_dr, draws, sizeof(uint32_t) * nd, hipMemcpyHostToDevice, c->stream));
    HV_HIP(c, hipMemcpyAsync(d_n, &n, sizeof(int), hipMemcpyHostToDevice, c->stream));
    rc = hv_ransac3_batch_dev(h, p, 1, mp, d_n, d_pl, d_pr, d_cl, camera0, camera1, second_to_first, d_dr, d_st, d_pose, d_sum);
    if (rc != HV_OK) return rc;
    int sm[4];
    double ps[12];
    if (n > 0) HV_HIP(c, hipMemcpyAsync(status, d_st, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipMemcpyAsync(ps, d_pose, sizeof(ps), hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipMemcpyAsync(sm, d_sum, sizeof(sm), hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    if (pose) for (int i = 0; i < 12; ++i) pose[i] = ps[i];
    if (summary) for (int i = 0; i < 4; ++i) summary[i] = sm[i];
    return HV_OK;
}

}  // extern "C"
