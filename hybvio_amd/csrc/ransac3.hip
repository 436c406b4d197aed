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
#include "ransac_lds.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace hv {
namespace {

#include "hv_geometry.hpp"    // cross3, dot3
#include "hv_stereo_idp.hpp"  // triangulate_world: shared with upright2p.hip
#include "hv_workgroup.hpp"  // block_compact, block_gather_front, stage_cameras

constexpr int R3_MAX_PTS = 1024;
// R3_THREADS, R3_WAVES, R3_CHUNK (iterations per round): ransac_lds.hpp

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

// a workgroup's LDS: the sections of Ransac3Lds as pointers, the staged cameras and secondToFirstCamera
struct R3View {
    double *wx, *wy, *wz, *fu, *fv, *mod, *cost, *best;
    int *map, *vmap, *st, *idx, *chunk, *tri;
    unsigned *draw;
    int *cnt, *ctl;
    const hv_camera_model *cam;
    const double *T;
};
__device__ __forceinline__ R3View r3_view(unsigned char *base, const Ransac3Lds &L, const hv_camera_model *cam, const double *T)
{
    auto d = [&](size_t off) { return reinterpret_cast<double *>(base + off); };
    auto i = [&](size_t off) { return reinterpret_cast<int *>(base + off); };
    return R3View{d(L.wx), d(L.wy), d(L.wz), d(L.fu), d(L.fv), d(L.mod), d(L.cost), d(L.best),
                  i(L.map), i(L.vmap), i(L.st), i(L.idx), i(L.chunk), i(L.tri), reinterpret_cast<unsigned *>(base + L.draw),
                  i(L.cnt), i(L.ctl), cam, T};
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

// ---- the phases of ransac3_kernel (a .. f of the file header). Every thread of the workgroup calls every phase; each header says which
// barriers the phase holds and what they publish ----

// a. The correspondences of the n tracked features (ransac_pipeline.cpp:231-251): three normalizePixel calls and the triangulation per
// lane, the m survivors compacted to the front (order kept), every status preset to RANSAC_OUTLIER (:235), the sampler's index vector and
// the loop's control words {iteration, limit, best iteration, inliers} initialised. Returns m. Begins without a barrier (s_map, s_cam and
// s_T are published by the caller). Barriers: one after the triangulation (publishes s_st and the points), block_compact's three,
// block_gather_front's one; ends with one, which publishes the gathered points, s_st, s_idx and s_ctl.
__device__ __forceinline__ int correspondences(const R3View &v, const float *pl, const float *pr, const float *cl, int n, int cap, int tid)
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
    __syncthreads();
    const int m = block_compact<R3_WAVES>([&](int k) { return v.st[k] != 0; }, v.vmap, n, v.chunk);
    static_assert(R3_MAX_PTS <= 4 * R3_THREADS, "four points per thread");
    double *const pts[5] = {v.wx, v.wy, v.wz, v.fu, v.fv};
    block_gather_front<R3_THREADS>(pts, v.vmap, m);
    for (int k = tid; k < n; k += R3_THREADS) v.st[k] = 3;
    for (int j = tid; j < m; j += R3_THREADS) v.idx[j] = j;
    if (tid == 0) { v.ctl[0] = 0; v.ctl[1] = cap; v.ctl[2] = -1; v.ctl[3] = 0; }
    __syncthreads();
    return m;
}

// positions 0..2 of the sampler's index vector, kept in registers by lane 0 (the rest is s_idx)
struct R3Head { int i0, i1, i2; };

// b. The sampler for the h iterations from it0: the raw draws go to LDS, a barrier publishes them, then lane 0 replays the partial
// shuffle idx[i] <-> idx[i + raw % (m - i)], i = 0, 1, 2, and hands each sample over in ascending index order. Ends with a barrier,
// which publishes s_tri.
__device__ __forceinline__ void sampler(const R3View &v, const uint32_t *draws, int it0, int h, int m, R3Head &hd, int tid)
{
    if (tid < 3 * h) v.draw[tid] = draws[3 * it0 + tid];
    __syncthreads();
    if (tid == 0) {
        int &i0 = hd.i0, &i1 = hd.i1, &i2 = hd.i2;
        for (int k = 0; k < h; ++k) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int j = i + (int)(v.draw[3 * k + i] % (unsigned)(m - i));
                int &mine = i == 0 ? i0 : i == 1 ? i1 : i2;
                if (j >= 3) { const int o = v.idx[j]; v.idx[j] = mine; mine = o; }
                else { int &other = j == 0 ? i0 : j == 1 ? i1 : i2; const int o = other; other = mine; mine = o; }
            }
            // the solver's canonical order: ascending indices (a repeated triple repeats its models bit for bit)
            const int lo = min(i0, min(i1, i2)), hi = max(i0, max(i1, i2));
            v.tri[3 * k] = lo; v.tri[3 * k + 1] = i0 + i1 + i2 - lo - hi; v.tri[3 * k + 2] = hi;
        }
    }
    __syncthreads();
}

// c. One P3P per lane, lanes 0 .. h - 1: up to four (R, c) into s_mod, their flags into s_cnt (s_cost holds the quartic's roots). Ends
// with a barrier, which publishes the models and the flags.
__device__ __forceinline__ void p3p_round(const R3View &v, int h, int tid)
{
    if (tid < h) {
        double Pw[3][3], F[3][2];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int s = v.tri[3 * tid + q];
            Pw[q][0] = v.wx[s]; Pw[q][1] = v.wy[s]; Pw[q][2] = v.wz[s]; F[q][0] = v.fu[s]; F[q][1] = v.fv[s];
        }
        p3p_lane(Pw, F, v.cost + 4 * tid, v.cnt + 4 * tid, v.mod + 48 * tid);
    }
    __syncthreads();
}

// d. Cost and inlier count of (hypothesis, solution) = lane over all m correspondences, added in order, into s_cost and s_cnt (-1: no
// model) over the lane's own flag and root. Ends with a barrier, which publishes both.
__device__ __forceinline__ void cost_and_count(const R3View &v, int h, int m, double thr, int use_mle, int tid)
{
    const bool have = (tid >> 2) < h && v.cnt[tid] != 0;
    double cost = 0.0;
    int cnt = -1;
    if (have) {
        double M[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) M[i] = v.mod[12 * tid + i];
        cnt = 0;
        for (int j = 0; j < m; ++j) {
            const double r = residual(M, v.wx[j], v.wy[j], v.wz[j], v.fu[j], v.fv[j]);
            const bool in = r < thr;
            cnt += in ? 1 : 0;
            cost = cost + (in ? r : thr);
        }
        if (!use_mle) cost = (double)(m - cnt);
    }
    v.cnt[tid] = cnt; v.cost[tid] = cost;
    __syncthreads();
}

// e. The loop's rule, replayed by lane 0 over the stored costs of the round: strict `<`, adaptive limit; the best model goes to s_best,
// the control words are brought up to date. Ends with a barrier, which publishes s_ctl (the loop's condition reads it) and s_best.
__device__ __forceinline__ void loop_rule(const R3View &v, const R3Args &a, int it0, int limit, int h, int m, double &best_cost, int tid)
{
    if (tid == 0) {
        int it = it0, lim = limit;
        for (int k = 0; k < h && it < lim; ++k, ++it)
            for (int s = 0; s < 4; ++s) {
                const int w = 4 * k + s, cnt = v.cnt[w];
                if (cnt >= 0 && v.cost[w] < best_cost) {
                    best_cost = v.cost[w];
                    for (int i = 0; i < 12; ++i) v.best[i] = v.mod[12 * w + i];
                    v.ctl[2] = it; v.ctl[3] = cnt;
                    const double ratio = (double)cnt / (double)m;
                    if (!(ratio < 3.0 / (double)m)) lim = min(max_iterations_for(ratio, a.logp, a.min_iters, a.max_iters), lim);
                }
            }
        v.ctl[0] = it; v.ctl[1] = lim;
    }
    __syncthreads();
}

// f. The best model's inliers go back to TRACKED (:265-268); statuses, pose, summary and the tail of compute (:139-144). Two barriers:
// one publishes the zeroed counter s_ctl[4], one the inlier count and s_st. Begins and ends without one.
__device__ __forceinline__ void inliers_and_outputs(const R3View &v, const R3Args &a, int set, int *ts, int n_all, int n, int m, bool run,
                                                    int tid)
{
    const int iters = v.ctl[0], best_it = v.ctl[2];
    const bool success = run && best_it >= 0;
    if (tid == 0) v.ctl[4] = 0;
    __syncthreads();
    if (success) {
        double M[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) M[i] = v.best[i];
        int cnt = 0;
        for (int j = tid; j < m; j += R3_THREADS)
            if (residual(M, v.wx[j], v.wy[j], v.wz[j], v.fu[j], v.fv[j]) < a.thr) { v.st[v.vmap[j]] = 0; ++cnt; }
        if (cnt) atomicAdd(&v.ctl[4], cnt);
    }
    __syncthreads();
    const int count = v.ctl[4];
    if (tid == 0) {
        if (a.pose)
            for (int i = 0; i < 12; ++i) a.pose[12 * (size_t)set + i] = success ? v.best[i] : 0.0;
        if (a.summary) {
            int *sm = a.summary + 4 * (size_t)set;
            sm[0] = count; sm[1] = success ? best_it : -1; sm[2] = run ? iters : 0; sm[3] = m;
        }
    }
    if (a.tail && !success) {                                                // SKIPPED: every track is cleared (:139-144)
        for (int i = tid; i < n_all; i += R3_THREADS) ts[i] = 3;
    } else {
        for (int k = tid; k < n; k += R3_THREADS) ts[v.map[k]] = v.st[k];
    }
    if (a.tail && tid == 0) {
        a.result[2 * (size_t)set] = success ? 2 : 0;
        a.result[2 * (size_t)set + 1] = count;
        const int r2count = n >= 2 ? a.r2_summary[2 * set] : 0;              // doRansac2 does not run below two tracks (:210)
        a.score[set] = n ? (double)r2count / (double)n : 0.0;
    }
}

__global__ __launch_bounds__(R3_THREADS) void ransac3_kernel(R3Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char r3_lds[];
    __shared__ hv_camera_model s_cam[2];
    __shared__ double s_T[16];
    const int set = blockIdx.x, tid = threadIdx.x;
    const int MP = a.max_points;
    const R3View v = r3_view(r3_lds, ransac3_lds(MP), s_cam, s_T);
    stage_cameras<R3_THREADS>(s_cam, a.cam0, a.cam1);
    if (tid < 16) s_T[tid] = a.T[tid];
    __syncthreads();                                            // publishes s_cam and s_T
    const int n_all = min(max(a.n_points[set], 0), MP);
    const float *pl = a.pl + (size_t)set * MP * 2, *pr = a.pr + (size_t)set * MP * 2, *cl = a.cl + (size_t)set * MP * 2;
    int *ts = a.status + (size_t)set * MP;

    // the set: TRACKED features in feature order
    const int n = block_compact<R3_WAVES>([&](int i) { return ts[i] == 0; }, v.map, n_all, v.chunk);
    const int m = correspondences(v, pl, pr, cl, n, a.cap, tid);            // a
    // m, and the control words that the loop reads behind a barrier, are the same in every thread: the conditions below are uniform
    // over the workgroup, so the barriers inside the phases are met by every thread or by none
    const bool run = m >= 3;
    if (run) {
        R3Head head{0, 1, 2};                                               // lane 0
        double best_cost = DBL_MAX;                                         // lane 0
        const uint32_t *draws = a.draws + (size_t)set * 3 * a.max_iters;
        for (;;) {                                                          // rounds of up to R3_CHUNK iterations
            const int it0 = v.ctl[0], limit = v.ctl[1];
            if (it0 >= limit) break;
            const int h = min(R3_CHUNK, a.cap - it0);
            sampler(v, draws, it0, h, m, head, tid);                        // b
            p3p_round(v, h, tid);                                           // c
            cost_and_count(v, h, m, a.thr, a.use_mle, tid);                 // d
            loop_rule(v, a, it0, limit, h, m, best_cost, tid);              // e
        }
    }
    inliers_and_outputs(v, a, set, ts, n_all, n, m, run, tid);              // f
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
    hipLaunchKernelGGL(ransac3_kernel, dim3((unsigned)n_sets), dim3(R3_THREADS), ransac3_lds(a.max_points).end, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

}  // namespace

int ransac3_init(Ctx *c)
{
    HV_HIP(c, set_lds_limit(ransac3_kernel, ransac3_lds(R3_MAX_PTS).end));
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
