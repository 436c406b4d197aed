// Stereo upright 2-point track filter: StereoUpright2p::compute without Theia and the UPRIGHT_2P branch of RansacPipeline::compute.
//
// Reference: src/tracker/stereo_upright_2p.cpp:72-81 (the error), :110-183 (compute), src/tracker/ransac_pipeline.cpp:124-127, 137-149
// (the branch and the tail of RansacPipeline::compute), src/odometry/backend.cpp:667-679 (the two poses),
// src/odometry/util.cpp:144-158 (toCameraToWorld), src/odometry/triangulation.cpp:711-764 (triangulateStereoFeatureIdp),
// src/tracker/camera.cpp (pixelToRay, normalizePixel). Theia is not in the tree: the sample-consensus loop follows the recollection
// written down for RANSAC3 and the minimal solver is ours, both stated operation by operation in tests/upright2p_restatement.py
// (divergences: DESIGN.md 3.21).
//
// One 256-thread workgroup per point set:
//   a. the correspondences: R0, R1 from the poses (given, or formed from the filter mean by lane 0), TRACKED features in feature
//      order, two normalizePixel calls, the triangulation and pixelToRay per lane, survivors compacted with ballots (order kept),
//      rotated model points, rotated rays and normalised rays in LDS
//   then rounds of up to 128 iterations, until the serial loop has ended (with the defaults the first limit is 98: one round):
//   b. lane 0 replays the sampler's partial shuffle (positions 0, 1 in registers, the rest of the index vector in LDS); each
//      sample is handed to the solver in ascending index order
//   c. one lane per (hypothesis, root): the quadratic of the pair, this lane's root, (c, s, t) in registers and in LDS
//   d. the same lane: cost and inlier count of its model over all correspondences, added in order
//   e. lane 0 replays the loop's rule over the stored costs: strict `<`, adaptive limit
//   f. every lane classifies its correspondences with the best model; statuses, model, summary, the tail of compute
// The per-hypothesis work is a handful of operations, so c runs on the lane pair of a hypothesis twice over instead of in a phase of
// its own: no barrier between c and d, and the cost phase -- hypotheses x 2 x m residuals, each sum serial in m -- has one lane per
// sum, four wavefronts on the four SIMDs of a compute unit. Arithmetic is binary64 in the operation order of the restatement (the
// library is built without FMA contraction).
#include "ekf_host.hpp"
#include "hv_camera.hpp"
#include "hv_internal.hpp"
#include "ransac_lds.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace hv {
namespace {

#include "hv_geometry.hpp"    // cross3, dot3, imu_to_world, mm4_entry
#include "hv_stereo_idp.hpp"  // triangulate_world
#include "hv_workgroup.hpp"   // block_compact, block_gather_front, stage_cameras

constexpr int U2_MAX_PTS = 1024;
constexpr int U2_STATE_MIN = 27;                   // the current pose and history pose 0 (ekf.hpp: POS 0, ORI 6, CAM 20, 7 per pose)
// U2_THREADS, U2_WAVES, U2_CHUNK (iterations per round), U2_MODEL: ransac_lds.hpp

struct U2Args {
    int max_points, max_iters, min_iters, use_mle, cap, tail, n_state;
    const int *n_points;
    const float *pl, *pr, *cl;            // previous-left, previous-right, current-left corners [sets][max_points][2]
    const uint32_t *draws;                // [sets][2 * max_iters] raw std::mt19937 outputs
    int *status;                          // [sets][max_points] Feature::Status in/out (TRACKED selects)
    const double *poses;                  // [sets][2][16] camera-to-world of the previous and the current frame, or NULL:
    const double *mean;                   // ... [sets][n_state] filter means, the poses are formed from them with cam_to_imu
    const int *r2_summary;                // tail: RANSAC2's {bestInlierCount, visited}
    int *result;                          // tail: [sets][2] {type, inlierCount}
    double *score;                        // tail: [sets]
    double *model;                        // [sets][12] or NULL
    int *summary;                         // [sets][4] or NULL
    double thr, logp;
    double T[16];                         // secondToFirstCamera, row-major
    double cam_to_imu[16];                // the inverse of imuToCamera (chain entry)
    hv_camera_model cam0, cam1;
};

// a workgroup's LDS: the sections of Upright2pLds as pointers, the staged cameras and secondToFirstCamera
struct U2View {
    double *mx, *my, *mz, *rx, *ry, *rz, *nu, *nv, *mod, *cost, *best, *rot;
    int *map, *vmap, *st, *idx, *chunk, *pair;
    unsigned *draw;
    int *cnt, *ctl;
    const hv_camera_model *cam;
    const double *T;
};
__device__ __forceinline__ U2View u2_view(unsigned char *base, const Upright2pLds &L, const hv_camera_model *cam, const double *T)
{
    auto d = [&](size_t off) { return reinterpret_cast<double *>(base + off); };
    auto i = [&](size_t off) { return reinterpret_cast<int *>(base + off); };
    return U2View{d(L.mx), d(L.my), d(L.mz), d(L.rx), d(L.ry), d(L.rz), d(L.nu), d(L.nv), d(L.mod), d(L.cost), d(L.best), d(L.rot),
                  i(L.map), i(L.vmap), i(L.st), i(L.idx), i(L.chunk), i(L.pair), reinterpret_cast<unsigned *>(base + L.draw),
                  i(L.cnt), i(L.ctl), cam, T};
}

// ComputeMaxIterations for a sample of 2 (restatement: compute_max_iterations)
__host__ __device__ inline int max_iterations_for2(double ratio, double logp, int min_it, int max_it)
{
    if (ratio <= 0.0) return max_it;
    if (ratio == 1.0) return min_it;
    const double lp = log(1.0 - ratio * ratio) - DBL_EPSILON;
    double v = ceil(logp / lp);
    v = v < (double)min_it ? (double)min_it : v;
    v = v > (double)max_it ? (double)max_it : v;
    return (int)v;
}

// The minimal solver (restatement: solve) for one root: Rz(theta) X_i + t = lambda_i r_i, i = 0, 1, with root 0 = (-B - sqrt(disc)) / A
// and root 1 = (-B + sqrt(disc)) / A. M = (c, s, tx, ty, tz). false: no solution.
__device__ __forceinline__ bool solve_root(const double *Xa, const double *Xb, const double *ra, const double *rb, int root, double *M)
{
    const bool swap = fabs(ra[2]) > fabs(rb[2]);                       // index 1 has the larger |r.z|
    const double *X0 = swap ? Xb : Xa, *X1 = swap ? Xa : Xb, *r0 = swap ? rb : ra, *r1 = swap ? ra : rb;
    const double D0 = X0[0] - X1[0], D1 = X0[1] - X1[1], D2 = X0[2] - X1[2];
    const double n2 = D0 * D0 + D1 * D1;
    const double k = r0[2] / r1[2];
    const double b0 = r0[0] - k * r1[0], b1 = r0[1] - k * r1[1];
    const double q = D2 / r1[2];
    const double a0 = q * r1[0], a1 = q * r1[1];
    const double A = b0 * b0 + b1 * b1, B = a0 * b0 + a1 * b1, C = (a0 * a0 + a1 * a1) - n2;
    const double disc = B * B - A * C;
    bool ok = n2 != 0 && r1[2] != 0 && A != 0 && disc >= 0;
    const double sq = sqrt(disc >= 0 ? disc : 0.0);
    const double l0 = root == 0 ? (-B - sq) / A : (-B + sq) / A;
    const double d0 = l0 * b0 + a0, d1 = l0 * b1 + a1;
    double c = D0 * d0 + D1 * d1, s = D0 * d1 - D1 * d0;
    const double h = sqrt(c * c + s * s);
    c = c / h; s = s / h;
    M[0] = c; M[1] = s;
    M[2] = l0 * r0[0] - (c * X0[0] - s * X0[1]);
    M[3] = l0 * r0[1] - (s * X0[0] + c * X0[1]);
    M[4] = l0 * r0[2] - X0[2];
#pragma unroll
    for (int i = 0; i < U2_MODEL; ++i) ok = ok && isfinite(M[i]);
    return ok;
}

// |(R1' (R X + t)).hnormalized() - rayNormalized|^2 (restatement: residuals); R1 row-major, read transposed
__device__ __forceinline__ double residual(const double *M, const double *R1, double X0, double X1, double X2, double nu, double nv)
{
    const double w0 = (M[0] * X0 - M[1] * X1) + M[2], w1 = (M[1] * X0 + M[0] * X1) + M[3], w2 = X2 + M[4];
    const double p0 = (R1[0] * w0 + R1[3] * w1) + R1[6] * w2, p1 = (R1[1] * w0 + R1[4] * w1) + R1[7] * w2,
                 p2 = (R1[2] * w0 + R1[5] * w1) + R1[8] * w2;
    const double e0 = p0 / p2 - nu, e1 = p1 / p2 - nv;
    return e0 * e0 + e1 * e1;
}

// ---- the phases of upright2p_kernel (a .. f of the file header). Every thread of the workgroup calls every phase; each header says
// which barriers the phase holds and what they publish ----

// a0. R0 and R1 (the top-left 3x3 of poses[0] and poses[1], stereo_upright_2p.cpp:124-125) into s_rot: read from the given poses, or
// formed from the filter mean as backend.cpp:667-679 does -- toCameraToWorld of history pose 0 and of the current pose -- by lane 0.
// No barrier: the caller's next one publishes s_rot.
__device__ __forceinline__ void rotations(const U2View &v, const U2Args &a, int set, int tid)
{
    if (a.poses) {
        if (tid < 18) v.rot[tid] = a.poses[32 * (size_t)set + 16 * (tid / 9) + 4 * ((tid % 9) / 3) + (tid % 9) % 3];
    } else if (tid == 0) {
        const double *m = a.mean + (size_t)set * a.n_state;
        double i2w[16];
#pragma unroll 1
        for (int w = 0; w < 2; ++w) {
            imu_to_world(m, w ? 0 : 20, w ? 6 : 23, i2w);
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) v.rot[9 * w + 3 * r + c] = mm4_entry(i2w, a.cam_to_imu, r, c);
        }
    }
}

// a. The correspondences of the n tracked features (stereo_upright_2p.cpp:128-160): two normalizePixel calls, the triangulation and
// pixelToRay per lane, the m survivors compacted to the front (order kept), every status preset to RANSAC_OUTLIER (:132), the
// sampler's index vector and the loop's control words {iteration, limit, best iteration, inliers} initialised. Returns m. Begins
// without a barrier (s_map, s_cam, s_T and s_rot are published by the caller). Barriers: one after the triangulation (publishes s_st
// and the points), block_compact's three, block_gather_front's one; ends with one, which publishes the gathered points, s_st, s_idx
// and s_ctl.
__device__ __forceinline__ int correspondences(const U2View &v, const float *pl, const float *pr, const float *cl, int n, int cap, int tid)
{
    for (int k = tid; k < n; k += U2_THREADS) {
        const int src = v.map[k];
        double h0[2], h1[2], ray[3], X[3];
        bool ok = normalize_pixel_positive(v.cam[0], pl[2 * src], pl[2 * src + 1], h0);
        ok = ok && normalize_pixel_positive(v.cam[1], pr[2 * src], pr[2 * src + 1], h1);
        ok = ok && triangulate_world(v.T, h0[0], h0[1], h1[0], h1[1], X);
        ok = ok && pixel_to_ray(v.cam[0], (double)cl[2 * src], (double)cl[2 * src + 1], ray);
        v.st[k] = ok ? 1 : 0;
        if (ok) {
            const double *R0 = v.rot, *R1 = v.rot + 9;
            v.mx[k] = dot3(R0, X); v.my[k] = dot3(R0 + 3, X); v.mz[k] = dot3(R0 + 6, X);
            v.rx[k] = dot3(R1, ray); v.ry[k] = dot3(R1 + 3, ray); v.rz[k] = dot3(R1 + 6, ray);
            v.nu[k] = ray[0] / ray[2]; v.nv[k] = ray[1] / ray[2];
        }
    }
    __syncthreads();
    const int m = block_compact<U2_WAVES>([&](int k) { return v.st[k] != 0; }, v.vmap, n, v.chunk);
    static_assert(U2_MAX_PTS <= 4 * U2_THREADS, "four points per thread");
    double *const pts[8] = {v.mx, v.my, v.mz, v.rx, v.ry, v.rz, v.nu, v.nv};
    block_gather_front<U2_THREADS>(pts, v.vmap, m);
    for (int k = tid; k < n; k += U2_THREADS) v.st[k] = 3;
    for (int j = tid; j < m; j += U2_THREADS) v.idx[j] = j;
    if (tid == 0) { v.ctl[0] = 0; v.ctl[1] = cap; v.ctl[2] = -1; v.ctl[3] = 0; }
    __syncthreads();
    return m;
}

// positions 0, 1 of the sampler's index vector, kept in registers by lane 0 (the rest is s_idx)
struct U2Head { int i0, i1; };

// b. The sampler for the h iterations from it0: the raw draws go to LDS, a barrier publishes them, then lane 0 replays the partial
// shuffle idx[i] <-> idx[i + raw % (m - i)], i = 0, 1, and hands each sample over in ascending index order. Ends with a barrier,
// which publishes s_pair.
__device__ __forceinline__ void sampler(const U2View &v, const uint32_t *draws, int it0, int h, int m, U2Head &hd, int tid)
{
    static_assert(2 * U2_CHUNK <= U2_THREADS, "one draw per thread");
    if (tid < 2 * h) v.draw[tid] = draws[2 * it0 + tid];
    __syncthreads();
    if (tid == 0) {
        int &i0 = hd.i0, &i1 = hd.i1;
        for (int k = 0; k < h; ++k) {
            const int j0 = (int)(v.draw[2 * k] % (unsigned)m);
            if (j0 >= 2) { const int o = v.idx[j0]; v.idx[j0] = i0; i0 = o; }
            else if (j0 == 1) { const int o = i1; i1 = i0; i0 = o; }
            const int j1 = 1 + (int)(v.draw[2 * k + 1] % (unsigned)(m - 1));
            if (j1 >= 2) { const int o = v.idx[j1]; v.idx[j1] = i1; i1 = o; }
            // the solver's canonical order: ascending indices (a repeated pair repeats its models bit for bit)
            v.pair[2 * k] = min(i0, i1); v.pair[2 * k + 1] = max(i0, i1);
        }
    }
    __syncthreads();
}

// c. This lane's root of this lane's hypothesis (lane = 2 * hypothesis + root): the model into M and into s_mod. Returns whether the
// lane has a model. No barrier: d follows in the same lane, and its barrier publishes s_mod.
__device__ __forceinline__ bool solve_lane(const U2View &v, int h, int tid, double *M)
{
    if ((tid >> 1) >= h) return false;
    const int ia = v.pair[tid & ~1], ib = v.pair[tid | 1];
    const double Xa[3] = {v.mx[ia], v.my[ia], v.mz[ia]}, Xb[3] = {v.mx[ib], v.my[ib], v.mz[ib]};
    const double ra[3] = {v.rx[ia], v.ry[ia], v.rz[ia]}, rb[3] = {v.rx[ib], v.ry[ib], v.rz[ib]};
    const bool have = solve_root(Xa, Xb, ra, rb, tid & 1, M);
#pragma unroll
    for (int i = 0; i < U2_MODEL; ++i) v.mod[U2_MODEL * tid + i] = M[i];
    return have;
}

// d. Cost and inlier count of the lane's model over all m correspondences, added in order, into s_cost and s_cnt (-1: no model). Ends
// with a barrier, which publishes both and s_mod.
__device__ __forceinline__ void cost_and_count(const U2View &v, bool have, const double *M, int m, double thr, int use_mle, int tid)
{
    double cost = 0.0;
    int cnt = -1;
    if (have) {
        double R1[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) R1[i] = v.rot[9 + i];
        cnt = 0;
        for (int j = 0; j < m; ++j) {
            const double r = residual(M, R1, v.mx[j], v.my[j], v.mz[j], v.nu[j], v.nv[j]);
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
__device__ __forceinline__ void loop_rule(const U2View &v, const U2Args &a, int it0, int limit, int h, int m, double &best_cost, int tid)
{
    if (tid == 0) {
        int it = it0, lim = limit;
        for (int k = 0; k < h && it < lim; ++k, ++it)
            for (int s = 0; s < 2; ++s) {
                const int w = 2 * k + s, cnt = v.cnt[w];
                if (cnt >= 0 && v.cost[w] < best_cost) {
                    best_cost = v.cost[w];
                    for (int i = 0; i < U2_MODEL; ++i) v.best[i] = v.mod[U2_MODEL * w + i];
                    v.ctl[2] = it; v.ctl[3] = cnt;
                    const double ratio = (double)cnt / (double)m;
                    if (!(ratio < 2.0 / (double)m)) lim = min(max_iterations_for2(ratio, a.logp, a.min_iters, a.max_iters), lim);
                }
            }
        v.ctl[0] = it; v.ctl[1] = lim;
    }
    __syncthreads();
}

// f. The best model's inliers go back to TRACKED (:177-179); statuses, model, summary and the tail of compute
// (ransac_pipeline.cpp:139-144). Two barriers: one publishes the zeroed counter s_ctl[4], one the inlier count and s_st. Begins and
// ends without one.
__device__ __forceinline__ void inliers_and_outputs(const U2View &v, const U2Args &a, int set, int *ts, int n_all, int n, int m, bool run,
                                                    int tid)
{
    const int iters = v.ctl[0], best_it = v.ctl[2];
    const bool success = run && best_it >= 0;
    if (tid == 0) v.ctl[4] = 0;
    __syncthreads();
    if (success) {
        double M[U2_MODEL], R1[9];
#pragma unroll
        for (int i = 0; i < U2_MODEL; ++i) M[i] = v.best[i];
#pragma unroll
        for (int i = 0; i < 9; ++i) R1[i] = v.rot[9 + i];
        int cnt = 0;
        for (int j = tid; j < m; j += U2_THREADS)
            if (residual(M, R1, v.mx[j], v.my[j], v.mz[j], v.nu[j], v.nv[j]) < a.thr) { v.st[v.vmap[j]] = 0; ++cnt; }
        if (cnt) atomicAdd(&v.ctl[4], cnt);
    }
    __syncthreads();
    const int count = v.ctl[4];
    if (tid == 0) {
        if (a.model) {
            double *o = a.model + 12 * (size_t)set;
            const double c = success ? v.best[0] : 0.0, s = success ? v.best[1] : 0.0;
            o[0] = c; o[1] = success ? -s : 0.0; o[2] = 0.0; o[3] = s; o[4] = c; o[5] = 0.0; o[6] = 0.0; o[7] = 0.0; o[8] = success ? 1.0 : 0.0;
            for (int i = 0; i < 3; ++i) o[9 + i] = success ? v.best[2 + i] : 0.0;
        }
        if (a.summary) {
            int *sm = a.summary + 4 * (size_t)set;
            sm[0] = count; sm[1] = success ? best_it : -1; sm[2] = run ? iters : 0; sm[3] = m;
        }
    }
    if (a.tail && !success) {                                                // SKIPPED: every track is cleared (:139-144)
        for (int i = tid; i < n_all; i += U2_THREADS) ts[i] = 3;
    } else {
        for (int k = tid; k < n; k += U2_THREADS) ts[v.map[k]] = v.st[k];
    }
    if (a.tail && tid == 0) {
        a.result[2 * (size_t)set] = success ? 4 : 0;                         // RansacResult::Type::UPRIGHT_2P
        a.result[2 * (size_t)set + 1] = count;
        const int r2count = n >= 2 ? a.r2_summary[2 * set] : 0;              // doRansac2 does not run below two tracks (:210)
        a.score[set] = n ? (double)r2count / (double)n : 0.0;
    }
}

__global__ __launch_bounds__(U2_THREADS) void upright2p_kernel(U2Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char u2_lds[];
    __shared__ hv_camera_model s_cam[2];
    __shared__ double s_T[16];
    const int set = blockIdx.x, tid = threadIdx.x;
    const int MP = a.max_points;
    const U2View v = u2_view(u2_lds, upright2p_lds(MP), s_cam, s_T);
    stage_cameras<U2_THREADS>(s_cam, a.cam0, a.cam1);
    if (tid >= 64 && tid < 80) s_T[tid - 64] = a.T[tid - 64];
    rotations(v, a, set, tid);
    __syncthreads();                                            // publishes s_cam, s_T and s_rot
    const int n_all = min(max(a.n_points[set], 0), MP);
    const float *pl = a.pl + (size_t)set * MP * 2, *pr = a.pr + (size_t)set * MP * 2, *cl = a.cl + (size_t)set * MP * 2;
    int *ts = a.status + (size_t)set * MP;

    // the set: TRACKED features in feature order
    const int n = block_compact<U2_WAVES>([&](int i) { return ts[i] == 0; }, v.map, n_all, v.chunk);
    const int m = correspondences(v, pl, pr, cl, n, a.cap, tid);            // a
    // m, and the control words that the loop reads behind a barrier, are the same in every thread: the conditions below are uniform
    // over the workgroup, so the barriers inside the phases are met by every thread or by none
    const bool run = m >= 2;
    if (run) {
        U2Head head{0, 1};                                                  // lane 0
        double best_cost = DBL_MAX;                                         // lane 0
        const uint32_t *draws = a.draws + (size_t)set * 2 * a.max_iters;
        for (;;) {                                                          // rounds of up to U2_CHUNK iterations
            const int it0 = v.ctl[0], limit = v.ctl[1];
            if (it0 >= limit) break;
            const int h = min(U2_CHUNK, a.cap - it0);
            sampler(v, draws, it0, h, m, head, tid);                        // b
            double M[U2_MODEL];
            const bool have = solve_lane(v, h, tid, M);                     // c
            cost_and_count(v, have, M, m, a.thr, a.use_mle, tid);           // d
            loop_rule(v, a, it0, limit, h, m, best_cost, tid);              // e
        }
    }
    inliers_and_outputs(v, a, set, ts, n_all, n, m, run, tid);              // f
}


// the host-side checks, made before the context is looked at
int check_params(const hv_upright2p_params *p, int max_points, int n_sets)
{
    if (!p || !(p->ransacStereoUpright2pFailureProbability > 0 && p->ransacStereoUpright2pFailureProbability < 1) ||
        !(p->ransacStereoUpright2pErrorThresh > 0) || p->ransacStereoUpright2pMaxIterations < 1 ||
        p->ransacStereoUpright2pMinIterations > p->ransacStereoUpright2pMaxIterations ||
        !(p->ransacMinInlierFraction >= 0 && p->ransacMinInlierFraction <= 1) || max_points < 1 || n_sets < 0)
        return HV_ERR_INVALID;
    if (max_points > U2_MAX_PTS || p->ransacStereoUpright2pMaxIterations > HV_UPRIGHT2P_MAX_ITERS || n_sets > 65535) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}

void fill_common(U2Args &a, const hv_upright2p_params *p, int max_points, const hv_camera_model *cam0, const hv_camera_model *cam1,
                 const double *second_to_first)
{
    a.max_points = max_points; a.max_iters = p->ransacStereoUpright2pMaxIterations; a.min_iters = p->ransacStereoUpright2pMinIterations;
    a.use_mle = p->ransacStereoUpright2pUseMle ? 1 : 0;
    a.thr = p->ransacStereoUpright2pErrorThresh; a.logp = std::log(p->ransacStereoUpright2pFailureProbability);
    a.cap = std::min(a.max_iters, max_iterations_for2(p->ransacMinInlierFraction, a.logp, a.min_iters, a.max_iters));
    for (int i = 0; i < 16; ++i) a.T[i] = second_to_first[i];
    a.cam0 = *cam0; a.cam1 = *cam1;
}

int launch(Ctx *c, int n_sets, const U2Args &a)
{
    hipLaunchKernelGGL(upright2p_kernel, dim3((unsigned)n_sets), dim3(U2_THREADS), upright2p_lds(a.max_points).end, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

}  // namespace

int upright2p_init(Ctx *c)
{
    HV_HIP(c, set_lds_limit(upright2p_kernel, upright2p_lds(U2_MAX_PTS).end));
    return HV_OK;
}

}  // namespace hv

using hv::Ctx;

extern "C" {

void hv_upright2p_default_params(hv_upright2p_params *p)
{
    if (!p) return;
    p->ransacStereoUpright2pErrorThresh = 1e-4;          // codegen/parameter_definitions.c:299
    p->ransacStereoUpright2pFailureProbability = 1e-4;   // :300
    p->ransacStereoUpright2pMaxIterations = 500;         // :301
    p->ransacStereoUpright2pMinIterations = 50;          // :302
    p->ransacStereoUpright2pUseMle = 1;                  // :303
    p->ransacMinInlierFraction = 0.3;                    // :282
}

int hv_upright2p_batch_dev(hv_ctx *h, const hv_upright2p_params *p, int n_sets, int max_points, const int *n_points_dev,
                           const float *prev_left_dev, const float *prev_right_dev, const float *cur_left_dev,
                           const hv_camera_model *camera0, const hv_camera_model *camera1, const double *second_to_first,
                           const double *poses_dev, const uint32_t *draws_dev, int *status_dev, double *model_dev, int *summary_dev)
{
    if (const int rc = hv::check_params(p, max_points, n_sets)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c || !camera0 || !camera1 || !second_to_first) return HV_ERR_INVALID;
    if (n_sets > 0 && (!n_points_dev || !prev_left_dev || !prev_right_dev || !cur_left_dev || !poses_dev || !draws_dev || !status_dev))
        return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    hv::U2Args a{};
    hv::fill_common(a, p, max_points, camera0, camera1, second_to_first);
    a.n_points = n_points_dev; a.pl = prev_left_dev; a.pr = prev_right_dev; a.cl = cur_left_dev; a.poses = poses_dev; a.draws = draws_dev;
    a.status = status_dev; a.model = model_dev; a.summary = summary_dev;
    hv::ScopedKernelTime tm(c, HV_K_RANSAC3);
    return hv::launch(c, n_sets, a);
}

int hv_upright2p_lk_batch_dev(hv_ekf *ekf, const hv_upright2p_params *p, const hv_flow_predict_params *cam_params, int max_points,
                              const int *n_points_dev, const float *prev_left_dev, const float *prev_right_dev,
                              const float *cur_left_dev, int *track_status_dev, const int *r2_summary_dev,
                              const hv_camera_model *camera0, const hv_camera_model *camera1, const double *second_to_first,
                              const uint32_t *draws_dev, int *result_dev, double *score_dev, double *model_dev, int *summary_dev)
{
    if (const int rc = hv::check_params(p, max_points, 0)) return rc;
    if (!cam_params || !camera0 || !camera1 || !second_to_first) return HV_ERR_INVALID;
    if (!n_points_dev || !prev_left_dev || !prev_right_dev || !cur_left_dev || !draws_dev || !track_status_dev || !r2_summary_dev ||
        !result_dev || !score_dev)
        return HV_ERR_INVALID;
    if (!ekf) return HV_ERR_INVALID;
    hv::Ekf *e = &ekf->e;
    Ctx *c = e->c;
    if (e->n < hv::U2_STATE_MIN || e->batch > 65535) return HV_ERR_UNSUPPORTED;
    if (e->batch == 0) return HV_OK;
    hv::U2Args a{};
    hv::fill_common(a, p, max_points, camera0, camera1, second_to_first);
    for (int i = 0; i < 16; ++i) a.cam_to_imu[i] = cam_params->cameraToImu[i];
    a.mean = e->fixed.m; a.n_state = e->n;
    a.n_points = n_points_dev; a.pl = prev_left_dev; a.pr = prev_right_dev; a.cl = cur_left_dev; a.draws = draws_dev;
    a.status = track_status_dev; a.r2_summary = r2_summary_dev; a.result = result_dev; a.score = score_dev; a.tail = 1;
    a.model = model_dev; a.summary = summary_dev;
    hv::ScopedKernelTime tm(c, HV_K_RANSAC3);
    return hv::launch(c, e->batch, a);
}

int hv_upright2p(hv_ctx *h, const hv_upright2p_params *p, int n, const float *prev_left_xy, const float *prev_right_xy,
                 const float *cur_left_xy, const hv_camera_model *camera0, const hv_camera_model *camera1,
                 const double *second_to_first, const double *poses, const uint32_t *draws, int *status, double *model, int *summary)
{
    if (n < 0) return HV_ERR_INVALID;
    if (const int rc = hv::check_params(p, std::max(n, 1), 1)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c || (n > 0 && (!prev_left_xy || !prev_right_xy || !cur_left_xy || !status)) || !camera0 || !camera1 || !second_to_first ||
        !poses || !draws)
        return HV_ERR_INVALID;
    const int mp = std::max(n, 1);
    const size_t nd = 2 * (size_t)p->ransacStereoUpright2pMaxIterations;
    hv::Stage s(c);
    const auto o_pl = s.take<float>(2 * (size_t)mp), o_pr = s.take<float>(2 * (size_t)mp), o_cl = s.take<float>(2 * (size_t)mp);
    const auto o_n = s.take<int>(1), o_st = s.take<int>(mp), o_sum = s.take<int>(4);
    const auto o_dr = s.take<uint32_t>(nd);
    const auto o_model = s.take<double>(12), o_poses = s.take<double>(32);
    int rc = s.reserve();
    if (rc != HV_OK) return rc;
    float *d_pl = s.at(o_pl), *d_pr = s.at(o_pr), *d_cl = s.at(o_cl);
    int *d_n = s.at(o_n), *d_st = s.at(o_st), *d_sum = s.at(o_sum);
    uint32_t *d_dr = s.at(o_dr);
    double *d_model = s.at(o_model), *d_poses = s.at(o_poses);
    if (n > 0) {
        HV_HIP(c, hipMemcpyAsync(d_pl, prev_left_xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice, c->stream));
        HV_HIP(c, hipMemcpyAsync(d_pr, prev_right_xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice, c->stream));
        HV_HIP(c, hipMemcpyAsync(d_cl, cur_left_xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice, c->stream));
        HV_HIP(c, hipMemcpyAsync(d_st, status, sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    }
    HV_HIP(c, hipMemcpyAsync(d_dr, draws, sizeof(uint32_t) * nd, hipMemcpyHostToDevice, c->stream));
    HV_HIP(c, hipMemcpyAsync(d_poses, poses, sizeof(double) * 32, hipMemcpyHostToDevice, c->stream));
    HV_HIP(c, hipMemcpyAsync(d_n, &n, sizeof(int), hipMemcpyHostToDevice, c->stream));
    rc = hv_upright2p_batch_dev(h, p, 1, mp, d_n, d_pl, d_pr, d_cl, camera0, camera1, second_to_first, d_poses, d_dr, d_st, d_model, d_sum);
    if (rc != HV_OK) return rc;
    int sm[4];
    double ps[12];
    if (n > 0) HV_HIP(c, hipMemcpyAsync(status, d_st, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipMemcpyAsync(ps, d_model, sizeof(ps), hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipMemcpyAsync(sm, d_sum, sizeof(sm), hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    if (model) for (int i = 0; i < 12; ++i) model[i] = ps[i];
    if (summary) for (int i = 0; i < 4; ++i) summary[i] = sm[i];
    return HV_OK;
}

}  // extern "C"
