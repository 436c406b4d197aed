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
// The round loop, b, d, e, f and the compaction of a are hv_sample_consensus.hpp's, shared with upright2p.hip; this file holds the
// problem (R3Problem): the per-lane loop of a, c with the quartic and the P3P, the residual and the entry points.
#include "hv_camera.hpp"
#include "hv_internal.hpp"
#include "ransac_lds.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace hv {
namespace {

#include "hv_geometry.hpp"    // cross3, dot3
#include "hv_stereo_idp.hpp"  // triangulate_world: shared with upright2p.hip
#include "hv_workgroup.hpp"  // block_compact, block_gather_front, stage_cameras

// R3_THREADS, R3_CHUNK (iterations per round): ransac_lds.hpp
#include "hv_sample_consensus.hpp"  // ScArgs, ScView and the phases a (tail), b, d, e, f, the round loop, the host side

struct R3Args : ScArgs {};                // model: the pose, R row-major and c (a type of its own: the kernel's name carries it)

// a workgroup's LDS: the sections of Ransac3Lds as pointers
struct R3View : ScView { double *wx, *wy, *wz, *fu, *fv; };
__device__ __forceinline__ R3View r3_view(unsigned char *base, const Ransac3Lds &L, const hv_camera_model *cam, const double *T)
{
    auto d = [&](size_t off) { return reinterpret_cast<double *>(base + off); };
    return R3View{sc_view(base, L, L.tri, cam, T), d(L.wx), d(L.wy), d(L.wz), d(L.fu), d(L.fv)};
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

// c. One P3P per lane, lanes 0 .. h - 1: up to four (R, c) into s_mod, their flags into s_cnt (s_cost holds the quartic's roots). Ends
// with a barrier, which publishes the models and the flags.
__device__ __forceinline__ void p3p_round(const R3View &v, int h, int tid)
{
    if (tid < h) {
        double Pw[3][3], F[3][2];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int s = v.sample[3 * tid + q];
            Pw[q][0] = v.wx[s]; Pw[q][1] = v.wy[s]; Pw[q][2] = v.wz[s]; F[q][0] = v.fu[s]; F[q][1] = v.fv[s];
        }
        p3p_lane(Pw, F, v.cost + 4 * tid, v.cnt + 4 * tid, v.mod + 48 * tid);
    }
    __syncthreads();
}

// the problem of hv_sample_consensus.hpp: its phases a (the per-lane loop) and c, the residual and the output model
struct R3Problem {
    static constexpr int SAMPLE = 3, SOLUTIONS = 4, MODEL = 12, THREADS = R3_THREADS, CHUNK = R3_CHUNK, TYPE = 2;   // RansacResult::Type::R3
    using View = R3View;

    // a. The correspondences of the n tracked features (ransac_pipeline.cpp:231-251): three normalizePixel calls and the triangulation
    // per lane, then compact_and_init (every status preset to RANSAC_OUTLIER: :235). Begins without a barrier (s_map, s_cam and s_T are
    // published by the caller).
    static __device__ __forceinline__ int correspondences(const R3View &v, const float *pl, const float *pr, const float *cl, int n, int cap, int tid)
    {
        for (int k = tid; k < n; k += R3_THREADS) {
            const int src = v.map[k];
            double h0[2], h1[2], h2[2], X[3];
            bool ok = normalize_pixel_positive(v.cam[0], pl[2 * src], pl[2 * src + 1], h0);
            ok = ok && normalize_pixel_positive(v.cam[1], pr[2 * src], pr[2 * src + 1], h1);
            ok = ok && normalize_pixel_positive(v.cam[0], cl[2 * src], cl[2 * src + 1], h2);
            ok = ok && triangulate_world(v.T, h0[0], h0[1], h1[0], h1[1], X);
            v.st[k] = ok ? 1 : 0;
            if (ok) { v.wx[k] = X[0]; v.wy[k] = X[1]; v.wz[k] = X[2]; v.fu[k] = h2[0]; v.fv[k] = h2[1]; }
        }
        double *const pts[5] = {v.wx, v.wy, v.wz, v.fu, v.fv};
        return compact_and_init<R3Problem>(v, pts, n, cap, tid);
    }

    // c. p3p_round with its barrier, then the model of (hypothesis, solution) = lane from s_mod into M. Returns whether the lane has one.
    static __device__ __forceinline__ bool models(const R3View &v, int h, int tid, double *M)
    {
        p3p_round(v, h, tid);
        const bool have = (tid >> 2) < h && v.cnt[tid] != 0;
        if (have) {
#pragma unroll
            for (int i = 0; i < 12; ++i) M[i] = v.mod[12 * tid + i];
        }
        return have;
    }

    // |(R (X - c)).hnormalized() - feature|^2 of correspondence j (restatement: residuals)
    static __device__ __forceinline__ double residual(const double *M, const R3View &v, int j)
    {
        const double d0 = v.wx[j] - M[9], d1 = v.wy[j] - M[10], d2 = v.wz[j] - M[11];
        const double p0 = (M[0] * d0 + M[1] * d1) + M[2] * d2, p1 = (M[3] * d0 + M[4] * d1) + M[5] * d2,
                     p2 = (M[6] * d0 + M[7] * d1) + M[8] * d2;
        const double e0 = p0 / p2 - v.fu[j], e1 = p1 / p2 - v.fv[j];
        return e0 * e0 + e1 * e1;
    }

    static __device__ __forceinline__ void write_model(double *o, const double *best, bool success)
    {
        for (int i = 0; i < 12; ++i) o[i] = success ? best[i] : 0.0;
    }
};

__global__ __launch_bounds__(R3_THREADS) void ransac3_kernel(R3Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char r3_lds[];
    __shared__ hv_camera_model s_cam[2];
    __shared__ double s_T[16];
    const int tid = threadIdx.x;
    stage_cameras<R3_THREADS>(s_cam, a.cam0, a.cam1);
    if (tid < 16) s_T[tid] = a.T[tid];
    sample_consensus<R3Problem>(r3_view(r3_lds, ransac3_lds(a.max_points), s_cam, s_T), a);   // begins with the barrier for s_cam and s_T
}

ScParams six(const hv_ransac3_params *p)
{
    if (!p) return ScParams{};
    return ScParams{p->ransac3ErrorThresh, p->ransac3FailureProbability, p->ransac3MaxIterations, p->ransac3MinIterations, p->ransac3UseMle,
                    p->ransacMinInlierFraction};
}

int check_params(const hv_ransac3_params *p, int max_points, int n_sets) { return check(six(p), max_points, n_sets, HV_RANSAC3_MAX_ITERS); }

int launch(Ctx *c, int n_sets, const R3Args &a)
{
    return launch(c, ransac3_kernel, R3_THREADS, ransac3_lds(a.max_points).end, n_sets, a);
}

}  // namespace

int ransac3_init(Ctx *c)
{
    HV_HIP(c, set_lds_limit(ransac3_kernel, ransac3_lds(SC_MAX_PTS).end));
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
    hv::fill_common<3>(a, hv::six(p), max_points, camera0, camera1, second_to_first);
    a.n_points = n_points_dev; a.pl = prev_left_dev; a.pr = prev_right_dev; a.cl = cur_left_dev; a.draws = draws_dev;
    a.status = status_dev; a.model = pose_dev; a.summary = summary_dev;
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
    hv::fill_common<3>(a, hv::six(p), max_points, camera0, camera1, second_to_first);
    a.n_points = n_points_dev; a.pl = prev_left_dev; a.pr = prev_right_dev; a.cl = cur_left_dev; a.draws = draws_dev;
    a.status = track_status_dev; a.r2_summary = r2_summary_dev; a.result = result_dev; a.score = score_dev; a.tail = 1;
    a.model = pose_dev; a.summary = summary_dev;
    hv::ScopedKernelTime tm(c, HV_K_RANSAC3);
    return hv::launch(c, n_sets, a);
}

int hv_ransac3(hv_ctx *h, const hv_ransac3_params *p, int n, const float *prev_left_xy, const float *prev_right_xy,
               const float *cur_left_xy, const hv_camera_model *camera0, const hv_camera_model *camera1,
               const double *second_to_first, const uint32_t *draws, int *status, double *pose, int *summary)
{
    return hv::staged_entry<3>(h, hv::six(p), HV_RANSAC3_MAX_ITERS, n, prev_left_xy, prev_right_xy, cur_left_xy,
                               camera0 && camera1 && second_to_first, nullptr, 0, draws, status, pose, summary, [&](const hv::StagedSet &d) {
        return hv_ransac3_batch_dev(h, p, 1, d.max_points, d.n, d.pl, d.pr, d.cl, camera0, camera1, second_to_first, d.draws, d.status, d.model, d.summary);
    });
}

}  // extern "C"
