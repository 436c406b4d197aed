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
// The round loop, b, d, e, f and the compaction of a are hv_sample_consensus.hpp's, shared with ransac3.hip; this file holds the
// problem (U2Problem): the rotations and the per-lane loop of a, c with the solver, the residual and the entry points.
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

constexpr int U2_STATE_MIN = 27;                   // the current pose and history pose 0 (ekf.hpp: POS 0, ORI 6, CAM 20, 7 per pose)
// U2_THREADS, U2_CHUNK (iterations per round), U2_MODEL: ransac_lds.hpp
#include "hv_sample_consensus.hpp"  // ScArgs, ScView and the phases a (tail), b, d, e, f, the round loop, the host side

struct U2Args : ScArgs {                  // model: Rz (row-major) and t
    int n_state;
    const double *poses;                  // [sets][2][16] camera-to-world of the previous and the current frame, or NULL:
    const double *mean;                   // ... [sets][n_state] filter means, the poses are formed from them with cam_to_imu
    double cam_to_imu[16];                // the inverse of imuToCamera (chain entry)
};

// a workgroup's LDS: the sections of Upright2pLds as pointers
struct U2View : ScView { double *mx, *my, *mz, *rx, *ry, *rz, *nu, *nv, *rot; };
__device__ __forceinline__ U2View u2_view(unsigned char *base, const Upright2pLds &L, const hv_camera_model *cam, const double *T)
{
    auto d = [&](size_t off) { return reinterpret_cast<double *>(base + off); };
    return U2View{sc_view(base, L, L.pair, cam, T), d(L.mx), d(L.my), d(L.mz), d(L.rx), d(L.ry), d(L.rz), d(L.nu), d(L.nv), d(L.rot)};
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

// the problem of hv_sample_consensus.hpp: its phases a (the per-lane loop) and c, the residual and the output model
struct U2Problem {
    static constexpr int SAMPLE = 2, SOLUTIONS = 2, MODEL = U2_MODEL, THREADS = U2_THREADS, CHUNK = U2_CHUNK, TYPE = 4;   // RansacResult::Type::UPRIGHT_2P
    using View = U2View;

    // a. The correspondences of the n tracked features (stereo_upright_2p.cpp:128-160): two normalizePixel calls, the triangulation and
    // pixelToRay per lane, then compact_and_init (every status preset to RANSAC_OUTLIER: :132). Begins without a barrier (s_map, s_cam,
    // s_T and s_rot are published by the caller).
    static __device__ __forceinline__ int correspondences(const U2View &v, const float *pl, const float *pr, const float *cl, int n, int cap, int tid)
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
        double *const pts[8] = {v.mx, v.my, v.mz, v.rx, v.ry, v.rz, v.nu, v.nv};
        return compact_and_init<U2Problem>(v, pts, n, cap, tid);
    }

    // c. This lane's root of this lane's hypothesis (lane = 2 * hypothesis + root): the model into M and into s_mod. Returns whether
    // the lane has a model. No barrier: d follows in the same lane, and its barrier publishes s_mod.
    static __device__ __forceinline__ bool models(const U2View &v, int h, int tid, double *M)
    {
        if ((tid >> 1) >= h) return false;
        const int ia = v.sample[tid & ~1], ib = v.sample[tid | 1];
        const double Xa[3] = {v.mx[ia], v.my[ia], v.mz[ia]}, Xb[3] = {v.mx[ib], v.my[ib], v.mz[ib]};
        const double ra[3] = {v.rx[ia], v.ry[ia], v.rz[ia]}, rb[3] = {v.rx[ib], v.ry[ib], v.rz[ib]};
        const bool have = solve_root(Xa, Xb, ra, rb, tid & 1, M);
#pragma unroll
        for (int i = 0; i < U2_MODEL; ++i) v.mod[U2_MODEL * tid + i] = M[i];
        return have;
    }

    // |(R1' (R X + t)).hnormalized() - rayNormalized|^2 of correspondence j (restatement: residuals); R1 row-major, read transposed
    // (it does not depend on j: the loops of d and f keep it in registers)
    static __device__ __forceinline__ double residual(const double *M, const U2View &v, int j)
    {
        const double *R1 = v.rot + 9;
        const double X0 = v.mx[j], X1 = v.my[j], X2 = v.mz[j];
        const double w0 = (M[0] * X0 - M[1] * X1) + M[2], w1 = (M[1] * X0 + M[0] * X1) + M[3], w2 = X2 + M[4];
        const double p0 = (R1[0] * w0 + R1[3] * w1) + R1[6] * w2, p1 = (R1[1] * w0 + R1[4] * w1) + R1[7] * w2,
                     p2 = (R1[2] * w0 + R1[5] * w1) + R1[8] * w2;
        const double e0 = p0 / p2 - v.nu[j], e1 = p1 / p2 - v.nv[j];
        return e0 * e0 + e1 * e1;
    }

    static __device__ __forceinline__ void write_model(double *o, const double *best, bool success)
    {
        const double c = success ? best[0] : 0.0, s = success ? best[1] : 0.0;
        o[0] = c; o[1] = success ? -s : 0.0; o[2] = 0.0; o[3] = s; o[4] = c; o[5] = 0.0; o[6] = 0.0; o[7] = 0.0; o[8] = success ? 1.0 : 0.0;
        for (int i = 0; i < 3; ++i) o[9 + i] = success ? best[2 + i] : 0.0;
    }
};

__global__ __launch_bounds__(U2_THREADS) void upright2p_kernel(U2Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char u2_lds[];
    __shared__ hv_camera_model s_cam[2];
    __shared__ double s_T[16];
    const int tid = threadIdx.x;
    const U2View v = u2_view(u2_lds, upright2p_lds(a.max_points), s_cam, s_T);
    stage_cameras<U2_THREADS>(s_cam, a.cam0, a.cam1);
    if (tid >= 64 && tid < 80) s_T[tid - 64] = a.T[tid - 64];
    rotations(v, a, blockIdx.x, tid);
    sample_consensus<U2Problem>(v, a);                          // begins with the barrier for s_cam, s_T and s_rot
}

ScParams six(const hv_upright2p_params *p)
{
    if (!p) return ScParams{};
    return ScParams{p->ransacStereoUpright2pErrorThresh, p->ransacStereoUpright2pFailureProbability, p->ransacStereoUpright2pMaxIterations,
                    p->ransacStereoUpright2pMinIterations, p->ransacStereoUpright2pUseMle, p->ransacMinInlierFraction};
}

int check_params(const hv_upright2p_params *p, int max_points, int n_sets) { return check(six(p), max_points, n_sets, HV_UPRIGHT2P_MAX_ITERS); }

int launch(Ctx *c, int n_sets, const U2Args &a)
{
    return launch(c, upright2p_kernel, U2_THREADS, upright2p_lds(a.max_points).end, n_sets, a);
}

}  // namespace

int upright2p_init(Ctx *c)
{
    HV_HIP(c, set_lds_limit(upright2p_kernel, upright2p_lds(SC_MAX_PTS).end));
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
    hv::fill_common<2>(a, hv::six(p), max_points, camera0, camera1, second_to_first);
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
    hv::fill_common<2>(a, hv::six(p), max_points, camera0, camera1, second_to_first);
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
    return hv::staged_entry<2>(h, hv::six(p), HV_UPRIGHT2P_MAX_ITERS, n, prev_left_xy, prev_right_xy, cur_left_xy,
                               camera0 && camera1 && second_to_first, poses, 32, draws, status, model, summary, [&](const hv::StagedSet &d) {
        return hv_upright2p_batch_dev(h, p, 1, d.max_points, d.n, d.pl, d.pr, d.cl, camera0, camera1, second_to_first, d.extra, d.draws, d.status,
                                      d.model, d.summary);
    });
}

}  // extern "C"
