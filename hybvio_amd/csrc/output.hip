// Device output stage for a batch of resident sequences, one workgroup per set (set s is filter s): what Session::process hands back
// at the end of a frame (backend.cpp:840-860), Control's overwrite of t and trackingStatus (control.cpp:117-128) and the API's pose
// conversion (api.cpp:726-742, 759-808) -- the inertial state and its covariances in the output frame, the pose trail with its
// timestamps, the tracking status and the point cloud of the tracks the visit loop triangulated. Restatement:
// tests/output_restatement.py.
//
// Reference: SlamOdometryCoordinateTransformer (backend.cpp:42-96), EKF::transformTo / translateTo (ekf.cpp:696-758),
// Output::setFromEKF (output.cpp:50-77), computePose (backend.cpp:1368-1386), getPointCloud (:255-280), the point-cloud lines of the
// visit loop (:905, 1066-1070, 1118, 1124, 1191, 1239-1251), util::toOdometryPose / toWorldToCamera (util.cpp:121-142).
//
// One wavefront per set: the work is a few dozen independent scalar chains. Lane 0 takes the current pose and lane i + 1 the trail
// pose i (at most HV_TRAIL_MAX_POSES - 1 = 63 of them) through computePose and, at the end, through the API conversion (one call
// site for each, so that neither is compiled twice); in between, transformTo's three non-identity diagonal blocks of A P A' and the
// 20 mean entries are spread over the lanes (A is block diagonal, so the 20 x 20
// block of A P A' needs no other product: entry (i, j) of a block is sum_k A(i, k) * (sum_l P(k, l) * A(j, l)), every other term of
// the dense products is an exact zero and every identity block a copy); the point cloud is one lane per candidate, the stop rule of
// the visit loop and the append positions from wave ballots. Everything is binary64 and uncontracted (the build's
// -ffp-contract=off), in the operation order of the restatement.
#include <math.h>

#include "ekf_host.hpp"

namespace hv {
namespace {

#include "hv_geometry.hpp"    // quat2rmat, rmat2quat, inv4
#include "hv_workgroup.hpp"   // clampi

constexpr int OUT_THREADS = 64;
constexpr int POS = 0, VEL = 3, ORI = 6, INER = 20, CAM = 20, POSE_DIM = 7;      // the state layout (ekf.hpp)
constexpr int GATE_INLIER = 0;                                                    // VuOutlierStatus::INLIER
constexpr int POINT_POSE_TRAIL = 1, POINT_OUTLIER = 4;                            // PointFeature::Status
static_assert(HV_TRAIL_MAX_POSES <= OUT_THREADS && HV_TRAIL_MAX_VISITS <= OUT_THREADS, "one lane per pose and per candidate");

struct OutputArgs {
    hv_session st;
    hv_trail_index t;
    hv_output_frame in;
    hv_output out;
    int n, K, M, V, ncam, n_sets, max_success, api_passthrough;
    const double *m, *P;                       // [n_sets][n], [n_sets][n][n] column-major: the current buffer of the ping-pong
    double imu_to_camera[16], imu_to_output[16];
};

__device__ inline void mm4(const double *A, const double *B, double *C)
{
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) C[4 * r + c] = ((A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]) + A[4 * r + 3] * B[12 + c];
}

// util::toWorldToCamera (util.cpp:132-142)
__device__ inline void to_world_to_camera(const double *p, const double *q, const double *imu_to_camera, double *out)
{
    double R[9], t[3];
    quat2rmat(q, R);
    for (int r = 0; r < 3; ++r) t[r] = ((-R[3 * r]) * p[0] + (-R[3 * r + 1]) * p[1]) + (-R[3 * r + 2]) * p[2];
    const double w2i[16] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0.0, 0.0, 0.0, 1.0};
    mm4(imu_to_camera, w2i, out);
}

// util::toOdometryPose (util.cpp:121-130): pose[7] = position, orientation
__device__ inline void to_odometry_pose(const double *world_to_camera, const double *imu_to_camera, double *pose)
{
    double inv[16], i2w[16];
    inv4(world_to_camera, inv);
    mm4(inv, imu_to_camera, i2w);
    pose[0] = i2w[3]; pose[1] = i2w[7]; pose[2] = i2w[11];
    const double Rt[9] = {i2w[0], i2w[4], i2w[8], i2w[1], i2w[5], i2w[9], i2w[2], i2w[6], i2w[10]};
    rmat2quat(Rt, pose + 3);
}

// toOdometryPose(toWorldToCamera(p, q, imuToCamera) * slamToOdometry, imuToCamera): transformInertialState (backend.cpp:73-77) and
// the ready branch of computePose (:1374-1375)
__device__ inline void slam_pose(const double *p, const double *q, const double *imu_to_camera, const double *slam_to_odometry, double *pose)
{
    double w2c[16], w2c_slam[16];
    to_world_to_camera(p, q, imu_to_camera, w2c);
    mm4(w2c, slam_to_odometry, w2c_slam);
    to_odometry_pose(w2c_slam, imu_to_camera, pose);
}

// convertOutputPose (api.cpp:726-742) with its inverted test: a non-identity imuToOutput passes the pose through
__device__ inline void api_pose(const OutputArgs &a, const double *identity, const double *pose, double *out)
{
    if (a.api_passthrough) {
        for (int k = 0; k < 7; ++k) out[k] = pose[k];
        return;
    }
    double w2o[16];
    to_world_to_camera(pose, pose + 3, a.imu_to_output, w2o);
    to_odometry_pose(w2o, identity, out);
}

__global__ __launch_bounds__(OUT_THREADS) void output_kernel(OutputArgs a)
{
    __shared__ double s_s2o[16], s_o2s[16], s_id[16];
    __shared__ double s_target[7];             // the (pos, ori) transformTo is called with
    __shared__ double s_pC[9], s_qC[16], s_shift[3];
    __shared__ double s_mean[INER];

    const int set = blockIdx.x, lane = threadIdx.x;
    if (a.in.frozen_dev && a.in.frozen_dev[set]) return;                              // control.cpp:128: output keeps the previous frame's value
    const int n = a.n, K = a.K, M = a.M, V = a.V, T = K - 1;
    const double *m = a.m + (size_t)set * n, *P = a.P + (size_t)set * n * n;
    const bool ready = a.in.ready_dev ? a.in.ready_dev[set] != 0 : true;
    const bool given = ready && a.in.slam_to_odometry_dev != nullptr;             // until setCoordinates both matrices are the identity
    if (lane < 16) {
        const double e = lane % 5 == 0 ? 1.0 : 0.0;
        s_id[lane] = e;
        s_s2o[lane] = given ? a.in.slam_to_odometry_dev[(size_t)set * 16 + lane] : e;
        s_o2s[lane] = given ? a.in.odometry_to_slam_dev[(size_t)set * 16 + lane] : e;
    }
    const int n_trail = clampi(a.t.n_keyframes[set], 1, K) - 1;
    const int32_t *kf_row = a.t.kf_row + (size_t)set * K;
    __syncthreads();

    // ---- control.cpp:118-122, backend.cpp:846, 856-857 ----
    if (lane == 0) {
        a.out.t[set] = a.st.first_sample_t[set] + a.st.time[set];             // getPlatformTime
        a.out.tracking_status[set] = a.in.tracking_status_dev[set];
        a.out.stationary_visual[set] = a.in.stationary_dev ? (a.in.stationary_dev[set] != 0) : 0;
        a.out.n_trail[set] = n_trail;
    }

    // ---- the poses: lane 0 the target of transformTo (backend.cpp:73-77), lane i + 1 computePose(i); one call site for both ----
    double pose[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                     // a trail pose of a set that is not ready: zeros (:1378-1379)
    if (lane <= n_trail && (lane == 0 || ready)) {
        const int ip = lane == 0 ? POS : CAM + POSE_DIM * (lane - 1), io = lane == 0 ? ORI : ip + 3;
        slam_pose(m + ip, m + io, a.imu_to_camera, s_s2o, pose);
    }
    if (lane == 0) {
        for (int k = 0; k < 7; ++k) s_target[k] = pose[k];
    } else if (lane <= n_trail) {
        const int i = lane - 1;
        for (int k = 0; k < 7; ++k) a.out.trail_pose[((size_t)set * T + i) * 7 + k] = pose[k];
        a.out.trail_time[(size_t)set * T + i] = a.t.timestamp[(size_t)set * K + clampi(kf_row[i + 1], 0, K - 1)];
    }
    __syncthreads();

    // ---- transformTo (ekf.cpp:704-757): qChange = conj(q0) * q1, its two matrices, the translation ----
    if (lane == 0) {
        const double c0[4] = {m[ORI], -m[ORI + 1], -m[ORI + 2], -m[ORI + 3]}, *q1 = s_target + 3;
        const double p1 = c0[0] * q1[0] - c0[1] * q1[1] - c0[2] * q1[2] - c0[3] * q1[3];
        const double p2 = c0[0] * q1[1] + c0[1] * q1[0] + c0[2] * q1[3] - c0[3] * q1[2];
        const double p3 = c0[0] * q1[2] - c0[1] * q1[3] + c0[2] * q1[0] + c0[3] * q1[1];
        const double p4 = c0[0] * q1[3] + c0[1] * q1[2] - c0[2] * q1[1] + c0[3] * q1[0];
        const double qC[16] = {p1, -p2, -p3, -p4, p2, p1, p4, -p3, p3, -p4, p1, p2, p4, p3, -p2, p1};      // row-major
        double pC[9];                                                          // row-major: toRotationMatrix() transposed
        const double w = p1, x = p2, y = p3, z = p4;
        const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
                     tyy = ty * y, tyz = tz * y, tzz = tz * z;
        pC[0] = 1 - (tyy + tzz); pC[3] = txy - twz; pC[6] = txz + twy;
        pC[1] = txy + twz; pC[4] = 1 - (txx + tzz); pC[7] = tyz - twx;
        pC[2] = txz - twy; pC[5] = tyz + twx; pC[8] = 1 - (txx + tyy);
        for (int k = 0; k < 16; ++k) s_qC[k] = qC[k];
        for (int k = 0; k < 9; ++k) s_pC[k] = pC[k];
        // translation = pos - pC * refPos; translateTo(position() + translation): deltaX = target - position() (ekf.cpp:696-702)
        for (int i = 0; i < 3; ++i) {
            const double y0 = (pC[3 * i] * m[POS] + pC[3 * i + 1] * m[POS + 1]) + pC[3 * i + 2] * m[POS + 2];
            const double target = y0 + (s_target[i] - y0);
            s_shift[i] = target - y0;
        }
    }
    __syncthreads();

    // ---- setFromEKF (output.cpp:56-62) of the transformed filter: lanes 0 .. 31 the covariance entries, 32 .. 51 the mean ----
    if (lane < 18) {                                                           // positionCov, velocityCov: pC P_bb pC'
        const int s0 = lane < 9 ? POS : VEL, e = lane % 9, i = e / 3, j = e % 3;
        double s = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double *Pk = P + s0 + k;                                     // P(s0 + k, s0 + l) = Pk[(s0 + l) * n]
            const double tmp = (Pk[(size_t)s0 * n] * s_pC[3 * j] + Pk[(size_t)(s0 + 1) * n] * s_pC[3 * j + 1]) + Pk[(size_t)(s0 + 2) * n] * s_pC[3 * j + 2];
            s = k == 0 ? s_pC[3 * i] * tmp : s + s_pC[3 * i + k] * tmp;
        }
        (lane < 9 ? a.out.position_cov : a.out.velocity_cov)[(size_t)set * 9 + e] = s;
        if (i == j) a.out.inertial_cov_diag[(size_t)set * INER + s0 + i] = s;
    } else if (lane < 22) {                                                    // the diagonal of qC P_oo qC'
        const int i = lane - 18;
        double s = 0.0;
        for (int k = 0; k < 4; ++k) {
            const double *Pk = P + ORI + k;
            const double tmp = ((Pk[(size_t)ORI * n] * s_qC[4 * i] + Pk[(size_t)(ORI + 1) * n] * s_qC[4 * i + 1]) + Pk[(size_t)(ORI + 2) * n] * s_qC[4 * i + 2]) +
                               Pk[(size_t)(ORI + 3) * n] * s_qC[4 * i + 3];
            s = k == 0 ? s_qC[4 * i] * tmp : s + s_qC[4 * i + k] * tmp;
        }
        a.out.inertial_cov_diag[(size_t)set * INER + ORI + i] = s;
    } else if (lane < 32) {                                                    // identity blocks: BGA .. SFT
        const int i = ORI + 4 + (lane - 22);
        a.out.inertial_cov_diag[(size_t)set * INER + i] = P[(size_t)i * n + i];
    } else if (lane < 32 + INER) {
        const int i = lane - 32;
        double v;
        if (i < ORI) {
            const int s0 = i < VEL ? POS : VEL, r = i - s0;
            v = (s_pC[3 * r] * m[s0] + s_pC[3 * r + 1] * m[s0 + 1]) + s_pC[3 * r + 2] * m[s0 + 2];
            if (s0 == POS) v = v + s_shift[r];
        } else if (i < ORI + 4) {
            const int r = i - ORI;
            v = ((s_qC[4 * r] * m[ORI] + s_qC[4 * r + 1] * m[ORI + 1]) + s_qC[4 * r + 2] * m[ORI + 2]) + s_qC[4 * r + 3] * m[ORI + 3];
        } else v = m[i];
        s_mean[i] = v;
        a.out.inertial_mean[(size_t)set * INER + i] = v;
    }

    // ---- the point cloud (backend.cpp:1066-1251, 255-280): one lane per candidate ----
    const int n_cand = ready ? clampi(a.in.n_candidates_dev[set], 0, V) : 0;      // getPointCloud returns an empty cloud until ready
    const size_t rec = (size_t)lane * a.n_sets + set;
    int kind = 0, tri = HV_TRI_NOT_VISITED, prep = 0;                           // 0 not visited, 1 success, 2 visited without an inlier
    if (lane < n_cand) {
        tri = a.in.status_dev[2 * rec]; prep = a.in.status_dev[2 * rec + 1];
        if (tri != HV_TRI_NOT_VISITED) kind = a.in.gate_status_dev[rec] == GATE_INLIER ? 1 : 2;
    }
    const unsigned long long below = (1ull << lane) - 1ull, upto = below | (1ull << lane);
    const unsigned long long visited = __ballot(kind != 0), success = __ballot(kind == 1);
    const int attempts = __popcll(visited & upto), successes = __popcll(success & upto);
    // the visit that ends the loop (:1240-1244): the first one that reaches a limit; candidates behind it were not visited
    const unsigned long long stops = __ballot(kind != 0 && ((a.max_success > 0 && successes >= a.max_success) || attempts >= V));
    const int stop = stops ? __ffsll((long long)stops) - 1 : OUT_THREADS;       // its push (:1249-1250) is behind the break
    const bool push = kind != 0 && lane < stop && tri == HV_TRI_OK;
    const unsigned long long pushed = __ballot(push);
    if (push) {
        const size_t o = (size_t)set * V + __popcll(pushed & below);
        a.out.point_id[o] = a.in.cand_id_dev[rec];
        // OUTLIER only behind the gate (:1157-1194): a track whose prepareVisualUpdate failed keeps POSE_TRAIL (:1118)
        a.out.point_status[o] = (prep == HV_PREPARE_VU_OK && kind == 2) ? POINT_OUTLIER : POINT_POSE_TRAIL;
        // track.points[0] (:1069): the first camera's corner select stored in the frame's keyframe, keyframe 1 since finish's push
        const int col = clampi(a.t.cand_col[(size_t)set * V + lane], 0, M - 1), row = clampi(kf_row[1 % K], 0, K - 1);
        const size_t ip = ((((size_t)set * K + row) * M + col) * a.ncam) * 2;
        a.out.point_first_pixel[2 * o] = a.t.image_point[ip]; a.out.point_first_pixel[2 * o + 1] = a.t.image_point[ip + 1];
        const double *pf = a.in.pf_dev + 3 * rec;
        for (int i = 0; i < 3; ++i)                                            // transformVec3ByMat4(odometryToSlam, point)
            a.out.point_xyz[3 * o + i] = ((s_o2s[4 * i] * pf[0] + s_o2s[4 * i + 1] * pf[1]) + s_o2s[4 * i + 2] * pf[2]) + s_o2s[4 * i + 3];
    }
    if (lane == 0) a.out.n_points[set] = __popcll(pushed);

    // ---- convertOutputPose: lane 0 the transformed inertial pose (api.cpp:797), lane i + 1 trail pose i (:775-780) ----
    __syncthreads();
    if (lane == 0) {
        for (int k = 0; k < 3; ++k) pose[k] = s_mean[POS + k];
        for (int k = 0; k < 4; ++k) pose[3 + k] = s_mean[ORI + k];
    }
    if (lane <= n_trail) {
        double api[7];
        api_pose(a, s_id, pose, api);
        double *dst = lane == 0 ? a.out.api_pose + (size_t)set * 7 : a.out.api_trail_pose + ((size_t)set * T + lane - 1) * 7;
        for (int k = 0; k < 7; ++k) dst[k] = api[k];
    }
}

}  // namespace
}  // namespace hv

extern "C" {

void hv_output_default_params(hv_output_params *p)
{
    if (!p) return;
    for (int i = 0; i < 16; ++i) p->imuToCamera[i] = p->imuToOutput[i] = i % 5 == 0 ? 1.0 : 0.0;
    p->maxVisualUpdates = 20;                        // codegen/parameter_definitions.c, as hv_trail_index_default_params
    p->maxSuccessfulVisualUpdates = 5;
    p->cameraTrailLength = 20;
    p->maxTracks = 200;
    p->useStereo = 1;
}

int hv_output_dev(hv_ekf *h, const hv_output_params *p, const hv_session *st, const hv_trail_index *trail, const hv_output_frame *in,
                  const hv_output *out)
{
    if (!p || !st || !st->first_sample_t || !st->time || !in || !out) return HV_ERR_INVALID;
    if (const int rc = hv::trail_check_state(trail)) return rc;
    if (!in->cand_id_dev || !in->n_candidates_dev || !in->status_dev || !in->gate_status_dev || !in->pf_dev || !in->tracking_status_dev)
        return HV_ERR_INVALID;
    if ((in->slam_to_odometry_dev == nullptr) != (in->odometry_to_slam_dev == nullptr)) return HV_ERR_INVALID;
    if (!out->t || !out->tracking_status || !out->stationary_visual || !out->inertial_mean || !out->inertial_cov_diag || !out->position_cov ||
        !out->velocity_cov || !out->n_trail || !out->trail_time || !out->trail_pose || !out->api_pose || !out->api_trail_pose ||
        !out->n_points || !out->point_id || !out->point_status || !out->point_first_pixel || !out->point_xyz)
        return HV_ERR_INVALID;
    if (p->cameraTrailLength < 1 || p->maxTracks < 1 || p->maxVisualUpdates < 1) return HV_ERR_INVALID;
    if (p->maxVisualUpdates > HV_TRAIL_MAX_VISITS || p->cameraTrailLength + 1 > HV_TRAIL_MAX_POSES) return HV_ERR_UNSUPPORTED;
    if (!h) return HV_ERR_INVALID;
    hv::Ekf *e = &h->e;
    hv::Ctx *c = e->c;
    if (e->batch > 65535 || e->n > 1024 || e->n < hv::CAM + hv::POSE_DIM * p->cameraTrailLength) return HV_ERR_UNSUPPORTED;
    if (e->batch == 0) return HV_OK;
    hv::OutputArgs a{};
    a.st = *st; a.t = *trail; a.in = *in; a.out = *out;
    a.n = e->n; a.K = p->cameraTrailLength + 1; a.M = p->maxTracks; a.V = p->maxVisualUpdates; a.ncam = p->useStereo ? 2 : 1;
    a.n_sets = e->batch; a.max_success = p->maxSuccessfulVisualUpdates;
    a.m = e->fixed.m; a.P = e->fixed.P;                                        // P: whichever buffer the ping-pong made current
    bool identity = true;                                                      // api.cpp:730, an exact comparison
    for (int i = 0; i < 16; ++i) {
        a.imu_to_camera[i] = p->imuToCamera[i]; a.imu_to_output[i] = p->imuToOutput[i];
        identity = identity && p->imuToOutput[i] == (i % 5 == 0 ? 1.0 : 0.0);
    }
    a.api_passthrough = !identity;
    hv::ScopedKernelTime tm(c, HV_K_EKF_CONTROL);
    hipLaunchKernelGGL(hv::output_kernel, dim3((unsigned)e->batch), dim3(hv::OUT_THREADS), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

}  // extern "C"
