// Device optical-flow predictor: the OpticalFlowPredictor lambda of Session::applyTracker for many resident sequences at once -- the
// start points of the temporal and the stereo LK call of Tracker::track (use_initial_flow = 1), from the filter mean and the
// pose-trail index.
//
// Reference: src/odometry/backend.cpp:545-664 (the lambda), src/tracker/tracker.cpp:58-62 (its two calls),
// src/odometry/ekf_state_index.cpp:312-339 (widestBaseline), src/odometry/triangulation.cpp:65-103 (extractCameraPoseTrail),
// :610-646 (triangulateWithTwoCameras without derivatives), :1000-1002 (pinv), src/odometry/util.cpp:132-158 (toWorldToCamera,
// toCameraToWorld), src/odometry/util.hpp:77-85 (transformVec3ByMat4), src/tracker/camera.cpp (pixelToRay / rayToPixel, hv_camera.hpp).
//
// One workgroup of 256 threads per set. A few lanes build the first camera's pose of every keyframe and the two 4x4
// transforms of the prediction type from the mean into LDS; the column IDs and lengths are staged in LDS so that a table slot finds
// its column; then a thread loop over the track slots: widestBaseline, the two-camera triangulation, the clamp, un-project, move,
// re-project, round to binary32. Everything is binary64 and uncontracted, in the operation order of
// tests/flow_predict_restatement.py; the one difference is pinv32 (hv_geometry.hpp), which inverts the determinant once where the
// restatement divides six times.
//
// Where the observations are. The entry runs between hv_trail_finish_batch_dev and the next hv_trail_select_batch_dev, where the head
// (keyframe 0) is the new, empty keyframe and the col_len observations of a column sit in the keyframes 1 .. col_len
// (hybvio_hip.h, hv_trail_index): keyframe k holds a track exactly when 1 <= k <= col_len. widestBaseline is written as the
// reference's two searches over that predicate, first keyframe up and last keyframe down.
#include "ekf_host.hpp"
#include "hv_camera.hpp"

namespace hv {
namespace {

#include "hv_geometry.hpp"    // mm3, mmT3, mv3, mTv3, quat2rmat, quat2rmat_d, pinv32, imu_to_world, mm4_entry
#include "hv_triangulation.hpp"   // camera_pose_pR, triangulate_two
#include "hv_workgroup.hpp"   // clampi, stage_cameras

constexpr int FP_THREADS = 256;
constexpr int FP_MAX = HV_TRACKS_MAX_TRACKS;
constexpr int FP_MAX_POSES = HV_TRAIL_MAX_POSES;
constexpr int POSE_WORDS = 12;                                   // p[3] R[9]
constexpr int CAM = 20, POSE_DIM = 7, POS = 0, ORI = 6;         // the state layout (ekf.hpp)
static_assert(FP_MAX_POSES <= FP_THREADS - 64, "the poses are built by the waves behind the first");

struct FlowArgs {
    hv_trail_index t;
    int M, K, ncam, n_state, pose0_history, min_baseline, reuse;
    double min_distance;
    const double *m;                 // [n_sets][n_state] means
    const int32_t *n_tracks, *ids;
    const float *c0;
    float *pred;
    double *distance;
    double tri_imu_to_cam[16];       // imuToCamera: the first camera's pose trail
    double mats[2][16];              // the inverse of the imuToCamera of camToWorld0; the imuToCamera of worldToCam1
};

struct FlowCameras { hv_camera_model cam0, cam1; };

// util::transformVec3ByMat4 (util.hpp:77-85)
__device__ inline void transform_vec3(const double *T, const double *v, double *out)
{
    for (int i = 0; i < 3; ++i) out[i] = ((T[4 * i] * v[0] + T[4 * i + 1] * v[1]) + T[4 * i + 2] * v[2]) + T[4 * i + 3];
}

__global__ __launch_bounds__(FP_THREADS) void flow_predict_kernel(FlowArgs a, FlowCameras cams)
{
    __shared__ hv_camera_model s_cam[2];
    __shared__ double s_pose[FP_MAX_POSES * POSE_WORDS];   // keyframe -> the first camera's p[3] R[9]
    __shared__ double s_c2w[16], s_w2c[16];                // camToWorld0, worldToCam1
    __shared__ double s_mat[4][16];                        // imuToWorld, cameraToImu of camToWorld0; imuToCamera of worldToCam1, worldToImu
    __shared__ int s_cid[FP_MAX];                          // column -> track ID
    __shared__ int s_len[FP_MAX];                          // column -> keyframes holding the track (0: free)
    __shared__ int s_row[FP_MAX_POSES];                    // keyframe -> physical row

    const int set = blockIdx.x, tid = threadIdx.x;
    const int M = a.M, K = a.K;
    const int n = clampi(a.n_tracks[set], 0, M);
    const int n_kf = clampi(a.t.n_keyframes[set], 1, K);
    const double *m = a.m + (size_t)set * a.n_state;
    stage_cameras<FP_THREADS>(s_cam, cams.cam0, cams.cam1);    // published by the barrier that ends phase 2
    // ---- phase 1: the factors of the two transforms (util.cpp:132-158) on one lane, the pose trail (triangulation.cpp:65-103) on the
    // waves behind the first ----
    if (tid == 0) {
        const int ip = a.pose0_history ? CAM : POS, io = a.pose0_history ? CAM + 3 : ORI;
        double R[9], t[3];
        imu_to_world(m, ip, io, s_mat[0]);                     // toCameraToWorld: imuToWorld = [rot' | position]
        quat2rmat(m + ORI, R);                                 // toWorldToCamera: worldToImu = [rot | -rot * position]
        for (int r = 0; r < 3; ++r) t[r] = ((-R[3 * r]) * m[POS] + (-R[3 * r + 1]) * m[POS + 1]) + (-R[3 * r + 2]) * m[POS + 2];
        const double w2i[16] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0.0, 0.0, 0.0, 1.0};
        for (int j = 0; j < 16; ++j) s_mat[3][j] = w2i[j];
    }
    if (tid >= 32 && tid < 64) s_mat[1 + ((tid - 32) >> 4)][tid & 15] = a.mats[(tid - 32) >> 4][tid & 15];
    if (!a.reuse) {
        const int k = tid - 64;
        if (k >= 0 && k < n_kf) {                              // keyframe k is historyPosition(k - 1)
            const int ip = k == 0 ? POS : CAM + POSE_DIM * (k - 1), io = k == 0 ? ORI : CAM + POSE_DIM * (k - 1) + 3;
            camera_pose_pR(m, ip, io, a.tri_imu_to_cam, s_pose + k * POSE_WORDS);
        }
        // ---- phase 2: the columns and the rows ----
        for (int c = tid; c < M; c += FP_THREADS) {
            s_cid[c] = a.t.col_id[(size_t)set * M + c];
            s_len[c] = clampi(a.t.col_len[(size_t)set * M + c], 0, n_kf - 1);
        }
        if (tid < K) s_row[tid] = clampi(a.t.kf_row[(size_t)set * K + tid], 0, K - 1);
    }
    __syncthreads();
    if (tid < 32) {                                            // camToWorld0 = imuToWorld * cameraToImu, worldToCam1 = imuToCamera * worldToImu
        const int w = tid >> 4, r = (tid >> 2) & 3, c = tid & 3;
        const double *A = s_mat[2 * w], *B = s_mat[2 * w + 1];
        (w ? s_w2c : s_c2w)[4 * r + c] = mm4_entry(A, B, r, c);
    }
    __syncthreads();

    // ---- phase 3: the tracks (backend.cpp:613-663) ----
    for (int i = tid; i < n; i += FP_THREADS) {
        const size_t slot = (size_t)set * M + i;
        asm volatile("" ::: "memory");                         // the camera constants stay in LDS: hoisted out of the loop they take the kernel from 126 to 260 registers
        double distance = -1.0;
        if (a.reuse) distance = a.distance[slot];
        else {
            const int id = a.ids[slot];
            int c = -1;
            for (int q = 0; q < M; ++q) c = (s_len[q] > 0 && s_cid[q] == id) ? q : c;   // IDs are unique: at most one column matches
            const int len = c >= 0 ? s_len[c] : 0;
            // widestBaseline (ekf_state_index.cpp:312-339) over "keyframe k holds the track" = 1 <= k <= len
            bool ok = false;
            int k0 = 0, k1 = 0;
            if (n_kf >= 2) {
                for (k0 = 0; k0 < n_kf; ++k0) if (k0 >= 1 && k0 <= len) { ok = true; break; }
                if (ok) {
                    for (k1 = n_kf - 1; ; --k1) { if ((k1 >= 1 && k1 <= len) || k1 == 0) break; }
                    ok = k0 != k1;
                }
            }
            if (ok && k1 - k0 >= a.min_baseline) {
                const size_t o0 = ((((size_t)set * K + s_row[k0]) * M + c) * a.ncam) * 2, o1 = ((((size_t)set * K + s_row[k1]) * M + c) * a.ncam) * 2;
                const double ip0[2] = {a.t.norm_point[o0], a.t.norm_point[o0 + 1]}, ip1[2] = {a.t.norm_point[o1], a.t.norm_point[o1 + 1]};
                double pf[3];
                triangulate_two(s_pose + k0 * POSE_WORDS, s_pose + k1 * POSE_WORDS, ip0, ip1, pf);
                if (pf[2] > 0.0) distance = sqrt(pf[0] * pf[0] + pf[1] * pf[1] + pf[2] * pf[2]);
            }
            if (distance < a.min_distance) distance = a.min_distance;
            if (a.distance) a.distance[slot] = distance;
        }
        const float x0 = a.c0[2 * slot], y0 = a.c0[2 * slot + 1];
        double ray0[3], p[3], ray1[3], pix[2];
        const bool success = pixel_to_ray(s_cam[0], (double)x0, (double)y0, ray0);
        for (int j = 0; j < 3; ++j) ray0[j] *= distance;
        transform_vec3(s_c2w, ray0, p);
        transform_vec3(s_w2c, p, ray1);
        float px = x0, py = y0;
        if (success && ray_to_pixel(s_cam[1], ray1, pix)) { px = (float)pix[0]; py = (float)pix[1]; }
        a.pred[2 * slot] = px;
        a.pred[2 * slot + 1] = py;
    }
}

}  // namespace
}  // namespace hv

extern "C" {

void hv_flow_predict_default_params(hv_flow_predict_params *p)
{
    if (!p) return;
    p->predictOpticalFlowMinTriangulationDistance = 3.0;   // codegen/parameter_definitions.c:213
    p->minBaselinePoses = 10;                              // MIN_TWO_CAMERA_FLOW_TRIANGULATION_BASELINE, backend.cpp:627
    double *mats[4] = {p->imuToCamera, p->secondImuToCamera, p->cameraToImu, p->secondCameraToImu};
    for (double *T : mats)
        for (int i = 0; i < 16; ++i) T[i] = i % 5 == 0 ? 1.0 : 0.0;
}

int hv_flow_predict_batch_dev(hv_ekf *h, const hv_flow_predict_params *p, int type, const hv_trail_index_params *tp,
                              const hv_trail_index *trail, const hv_track_table *table, const float *c0_dev,
                              const hv_camera_model *camera0, const hv_camera_model *camera1, float *pred_xy_dev, double *distance_dev,
                              int reuse_distance)
{
    if (!p) return HV_ERR_INVALID;
    if (const int rc = hv::trail_check_params(tp, 0)) return rc;
    if (const int rc = hv::trail_check_state(trail)) return rc;
    if (!table || !table->n_tracks || !table->ids || !c0_dev || !camera0 || !pred_xy_dev) return HV_ERR_INVALID;
    if (type < HV_FLOW_PREDICT_LEFT || type > HV_FLOW_PREDICT_STEREO || (type != HV_FLOW_PREDICT_LEFT && !camera1)) return HV_ERR_INVALID;
    if ((reuse_distance && !distance_dev) || p->minBaselinePoses < 1) return HV_ERR_INVALID;
    if (tp->maxTracks > hv::FP_MAX || tp->cameraTrailLength + 1 > hv::FP_MAX_POSES) return HV_ERR_UNSUPPORTED;
    if (!h) return HV_ERR_INVALID;
    hv::Ekf *e = &h->e;
    hv::Ctx *c = e->c;
    if (e->n < hv::CAM + hv::POSE_DIM * tp->cameraTrailLength) return HV_ERR_UNSUPPORTED;
    if (e->batch == 0) return HV_OK;
    hv::FlowArgs a{};
    a.t = *trail;
    a.M = tp->maxTracks; a.K = tp->cameraTrailLength + 1; a.ncam = tp->useStereo ? 2 : 1; a.n_state = e->n;
    a.pose0_history = type != HV_FLOW_PREDICT_STEREO;
    a.min_baseline = p->minBaselinePoses; a.reuse = reuse_distance != 0;
    a.min_distance = p->predictOpticalFlowMinTriangulationDistance;
    a.m = e->fixed.m; a.n_tracks = table->n_tracks; a.ids = table->ids; a.c0 = c0_dev; a.pred = pred_xy_dev; a.distance = distance_dev;
    const bool right = type == HV_FLOW_PREDICT_RIGHT;
    for (int i = 0; i < 16; ++i) {
        a.tri_imu_to_cam[i] = p->imuToCamera[i];
        a.mats[0][i] = right ? p->secondCameraToImu[i] : p->cameraToImu[i];
        a.mats[1][i] = type == HV_FLOW_PREDICT_LEFT ? p->imuToCamera[i] : p->secondImuToCamera[i];
    }
    hv::FlowCameras cams{};
    cams.cam0 = right ? *camera1 : *camera0;
    cams.cam1 = type == HV_FLOW_PREDICT_LEFT ? *camera0 : *camera1;
    hv::ScopedKernelTime tm(c, HV_K_TRAIL_INDEX);
    hipLaunchKernelGGL(hv::flow_predict_kernel, dim3((unsigned)e->batch), dim3(hv::FP_THREADS), 0, c->stream, a, cams);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

}  // extern "C"
