// The resident VIO engine: a session of n_sets sequences as one owned object with one call per frame (hv_vio_create: the default
// stereo session; hv_vio_create_session: every session useStereo, useRansac3, useStereoUpright2p, useHybridRansac and featureDetector
// select; hv_vio_frame / hv_vio_view_get / hv_vio_replay_period; include/hybvio_hip.h, INTEGRATION.md "One call per frame").
// Session::process (backend.cpp:716-860) behind Tracker::add, issued as the library's own _dev entries in the reference's order.
//
// No stage is restated here, with one exception: the branch of RansacPipeline::compute that runs no filter behind RANSAC2
// (ransac_pipeline.cpp:134-136) is one division per set, vio_ransac2_score_kernel below. The file owns the buffers the stages pass to
// each other (one block, carved once) and the two kernels that keep what a caller of the long chains keeps on the host:
//   vio_frame_begin_kernel   the frame number's rule fullVisualUpdate = num % visualUpdateForEveryNFrame == 0 || !canPopKeyframe()
//                            (backend.cpp:765, ekf_state_index.hpp:109), the per-frame counters, the "has a previous frame" flag
//                            and the point count of the temporal chain that follows from it;
//   vio_frame_end_kernel     the roles of the pyramid slots (prev_left <- cur_left, the freed slot is the next cur_left), the
//                            frame number, and "has a previous frame" cleared where the frame ended in a reset.
// Both are one thread per set, a few integer loads and stores each: a workgroup of 256 covers 256 sets, and a launch floor is all
// they cost. With them a frame leaves no state on the host, so hv_vio_frame can sit in a HIP graph; the two covariance swaps of a
// frame (undo-augment, symmetrize-augment) cancel, so the graph holds one frame (hv_vio_replay_period() == 1).
#include <math.h>
#include <stdint.h>
#include <new>

#include "ekf_host.hpp"

namespace hv {
namespace {

constexpr int VIO_THREADS = 256;

struct BeginArgs {
    int n_sets, every_n;
    const int32_t *frame_no, *n_keyframes, *n_tracks;
    const uint8_t *has_prev;
    uint8_t *full_update, *prev_seen;
    int32_t *n_lk, *success, *n_candidates, *n_delete;
};
struct EndArgs {
    int n_sets;
    int32_t *slot_prev, *slot_cur, *frame_no;
    uint8_t *has_prev;
    const int32_t *reset_kind;
};

__global__ __launch_bounds__(VIO_THREADS) void vio_frame_begin_kernel(BeginArgs a)
{
    const int s = blockIdx.x * VIO_THREADS + threadIdx.x;
    if (s >= a.n_sets) return;
    const int num = a.frame_no[s];                               // frame->num: 1 on the first frame (sample_sync.cpp:138), never negative
    a.full_update[s] = (num % a.every_n == 0 || a.n_keyframes[s] < 2) ? 1 : 0;
    const uint8_t prev = a.has_prev[s];
    a.prev_seen[s] = prev;
    a.n_lk[s] = prev ? a.n_tracks[s] : 0;                        // no previous image: the temporal chain sees no point
    a.success[s] = 0; a.n_candidates[s] = 0; a.n_delete[s] = 0;
}

__global__ __launch_bounds__(VIO_THREADS) void vio_frame_end_kernel(EndArgs a)
{
    const int s = blockIdx.x * VIO_THREADS + threadIdx.x;
    if (s >= a.n_sets) return;
    const int32_t freed = a.slot_prev[s];
    a.slot_prev[s] = a.slot_cur[s];
    a.slot_cur[s] = freed;
    const int32_t num = a.frame_no[s];
    a.frame_no[s] = num == INT32_MAX ? 1 : num + 1;
    const int32_t kind = a.reset_kind[s];
    a.has_prev[s] = (kind == HV_RESET_FRESH || kind == HV_RESET_KEEP_POSE) ? 0 : 1;   // a reset builds a new tracker
}

// RansacPipeline::compute with useRansac3, useStereoUpright2p and useHybridRansac all off (ransac_pipeline.cpp:134-136): the statuses
// stay as the gate left them and the score is ransac2Result.inlierCount / static_cast<double>(nTrackedFeatures), unguarded: no tracked
// feature gives 0 / 0 = NaN (RANSAC2 is skipped below two points and reports 0 inliers), which hv_tracks_update_batch_dev's
// score * (...) > threshold reads as "not stationary". lastResult() stays the default RansacResult: SKIPPED, 0 inliers.
struct ScoreArgs {
    int n_sets, max_points;
    const int32_t *n_points, *track_status, *r2_summary;
    double *score;
    int32_t *result;
};

__global__ __launch_bounds__(VIO_THREADS) void vio_ransac2_score_kernel(ScoreArgs a)
{
    const int s = blockIdx.x * VIO_THREADS + threadIdx.x;
    if (s >= a.n_sets) return;
    const int n = min(max(a.n_points[s], 0), a.max_points);
    const int32_t *ts = a.track_status + (size_t)s * a.max_points;
    int tracked = 0;
    for (int i = 0; i < n; i++) tracked += ts[i] == 0;           // Feature::Status::TRACKED
    a.score[s] = (double)a.r2_summary[2 * s] / (double)tracked;
    a.result[2 * s] = 0; a.result[2 * s + 1] = 0;
}

inline void mat4_mul(const double *a, const double *b, double *out)        // row-major
{
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double acc = 0.0;
            for (int k = 0; k < 4; k++) acc += a[4 * i + k] * b[4 * k + j];
            out[4 * i + j] = acc;
        }
}

// carves the engine's one block: the same sequence of take() calls runs twice, first without a base to size the block
struct Carver {
    unsigned char *base = nullptr;
    size_t used = 0;
    template <class T> T *take(size_t count)
    {
        used = (used + 255) & ~(size_t)255;
        T *p = base ? reinterpret_cast<T *>(base + used) : nullptr;
        used += count * sizeof(T);
        return p;
    }
    // an array only some sessions have: nothing is taken (and the layout behind it does not move) where it is not wanted
    template <class T> T *take_if(bool wanted, size_t count) { return wanted ? take<T>(count) : nullptr; }
};

enum { FILTER_RANSAC3 = 0, FILTER_UPRIGHT2P = 1, FILTER_HYBRID = 2, FILTER_NONE = 3 };

}  // namespace

struct Vio {
    Ctx *c = nullptr;
    hv_ctx *ctx = nullptr;
    hv_ekf *ekf = nullptr;
    hv_vio_params p{};
    int S = 0, M = 0, K = 0, V = 0, W = 0, nk = 0;
    // what the session is: hv_vio_create leaves the default stereo session, hv_vio_create_session chooses (choose_session)
    bool stereo = true;
    int filter = FILTER_RANSAC3, detector = HV_DETECTOR_GPU_GFTT;
    int n_filter_draws = 0;                                      // raw draws a frame takes from the second tracker generator
    int max_kp = 0;                                              // FAST / legacy GFTT: the key point capacity of an image
    size_t det_work_bytes = 0;
    double r_gate = 0, r_update = 0, second_to_first[16] = {};
    float threshold_pow2 = 0;
    hv_vu_params vu{};
    std::vector<int> slots;                                      // the pool slots the engine holds: 3 per set, 2 for a mono session
    DevBuf<unsigned char> block;

    hv_track_table table{};
    hv_trail_index trail{};
    hv_session ses{};
    hv_ekf_control ctl{};
    hv_rng rng2{}, rng3{}, rng_odo{};
    hv_output rec{};
    // frame state
    int32_t *slot_prev = nullptr, *slot_cur = nullptr, *slot_right = nullptr, *frame_no = nullptr, *n_lk = nullptr;
    uint8_t *has_prev = nullptr, *prev_seen = nullptr, *full_update = nullptr;
    // IMU
    double *dt = nullptr, *time_rows = nullptr;
    // tracker chain
    float *cur_xy = nullptr, *right_xy = nullptr, *r2_R = nullptr, *mask_xy = nullptr, *kp = nullptr, *corners = nullptr, *corners_right = nullptr,
          *new_xy = nullptr, *new_right = nullptr;
    double *distance = nullptr, *score = nullptr;
    uint8_t *lk = nullptr, *lk2 = nullptr, *lk3 = nullptr, *tracked_mask = nullptr;
    int32_t *track_status = nullptr, *stereo_status = nullptr, *r2_status = nullptr, *r2_summary = nullptr, *r3_result = nullptr,
            *r3_summary = nullptr, *r5_summary = nullptr, *n_kp = nullptr, *keyframe = nullptr, *n_mask = nullptr, *src_index = nullptr, *n_corners = nullptr,
            *detection_status = nullptr, *n_new = nullptr, *n_added = nullptr;
    uint32_t *draws2 = nullptr, *draws3 = nullptr, *draws_odo = nullptr;
    // filter chain
    int32_t *keyframe_out = nullptr, *draws_used = nullptr, *n_poses = nullptr, *pose_index = nullptr, *cand_id = nullptr,
            *n_candidates = nullptr, *status = nullptr, *gate_status = nullptr, *success = nullptr, *delete_ids = nullptr,
            *n_delete = nullptr, *n_attempts = nullptr, *n_success = nullptr, *discarded = nullptr, *tracking_out = nullptr,
            *reset_kind = nullptr;
    uint8_t *undo_active = nullptr, *stationary = nullptr, *good_frame = nullptr, *frozen = nullptr;
    double *features = nullptr, *velocities = nullptr, *y = nullptr, *pf = nullptr;
    unsigned char *det_work = nullptr;

    void carve(Carver &a)
    {
        const size_t s = S, m = M, k = K, v = V, w = W, sm = s * m;
        table.n_tracks = a.take<int32_t>(s); table.ids = a.take<int32_t>(sm); table.xy = a.take<float>(sm * 2);
        table.second_xy = a.take_if<float>(stereo, sm * 2); table.status = a.take<int32_t>(sm); table.blacklist = a.take<uint8_t>(sm);
        table.kf_xy = a.take<float>(sm * 2); table.kf_valid = a.take<uint8_t>(sm); table.frame_num = a.take<int32_t>(s);
        table.mask_steps = a.take<int32_t>(s); table.mask_radius = a.take<int32_t>(s); table.frame_flags = a.take<uint8_t>(s);
        trail.n_keyframes = a.take<int32_t>(s); trail.frame_counter = a.take<int32_t>(s); trail.kf_row = a.take<int32_t>(s * k);
        trail.frame_number = a.take<int32_t>(s * k); trail.timestamp = a.take<double>(s * k); trail.col_id = a.take<int32_t>(sm);
        const size_t pt = stereo ? 4 : 2;                        // [cameras][2] per observation
        trail.col_len = a.take<int32_t>(sm); trail.image_point = a.take<float>(s * k * m * pt); trail.norm_point = a.take<double>(s * k * m * pt);
        trail.norm_velocity = a.take<double>(s * k * m * pt); trail.used = a.take<uint8_t>(s * k * m); trail.n_blacklist = a.take<int32_t>(s);
        trail.blacklist_ids = a.take<int32_t>(sm); trail.n_order = a.take<int32_t>(s); trail.n_skipped = a.take<int32_t>(s);
        trail.skipped_pos = a.take<int32_t>(sm); trail.skipped_id = a.take<int32_t>(sm); trail.cand_pos = a.take<int32_t>(s * v);
        trail.cand_col = a.take<int32_t>(s * v);
        ses.good_ring = a.take<float>(s * w); ses.ring_head = a.take<int32_t>(s); ses.ring_entries = a.take<int32_t>(s);
        ses.tracking_status = a.take<int32_t>(s); ses.control_status = a.take<int32_t>(s); ses.last_reset_time = a.take<double>(s);
        ses.first_sample = a.take<uint8_t>(s); ses.first_sample_t = a.take<double>(s); ses.prev_sample_t = a.take<double>(s);
        ses.time = a.take<double>(s); ses.initialized_orientation = a.take<uint8_t>(s);
        ctl.zupt_time = a.take<double>(s); ctl.init_zupt_time = a.take<double>(s); ctl.was_stationary = a.take<int32_t>(s);
        ctl.frames_since_keyframe = a.take<int32_t>(s);
        for (hv_rng *r : {&rng2, &rng3, &rng_odo}) { r->mt = a.take<uint32_t>(s * HV_RNG_STATE_WORDS); r->pos = a.take<int32_t>(s); }
        const size_t t = p.output.cameraTrailLength;
        rec.t = a.take<double>(s); rec.tracking_status = a.take<int32_t>(s); rec.stationary_visual = a.take<uint8_t>(s);
        rec.inertial_mean = a.take<double>(s * 20); rec.inertial_cov_diag = a.take<double>(s * 20); rec.position_cov = a.take<double>(s * 9);
        rec.velocity_cov = a.take<double>(s * 9); rec.n_trail = a.take<int32_t>(s); rec.trail_time = a.take<double>(s * t);
        rec.trail_pose = a.take<double>(s * t * 7); rec.api_pose = a.take<double>(s * 7); rec.api_trail_pose = a.take<double>(s * t * 7);
        rec.n_points = a.take<int32_t>(s); rec.point_id = a.take<int32_t>(s * v); rec.point_status = a.take<int32_t>(s * v);
        rec.point_first_pixel = a.take<float>(s * v * 2); rec.point_xyz = a.take<double>(s * v * 3);

        slot_prev = a.take<int32_t>(s); slot_cur = a.take<int32_t>(s); slot_right = a.take_if<int32_t>(stereo, s); frame_no = a.take<int32_t>(s);
        n_lk = a.take<int32_t>(s); has_prev = a.take<uint8_t>(s); prev_seen = a.take<uint8_t>(s); full_update = a.take<uint8_t>(s);
        dt = a.take<double>((size_t)p.imu_samples_max * s); time_rows = a.take<double>((size_t)p.imu_samples_max * s);

        // (r3_result and r3_summary are the result and the summary of whichever filter runs behind RANSAC2: both sample-consensus
        // filters have the same four summary words, and draws3 holds the draws of the one that is selected)
        const bool consensus = filter == FILTER_RANSAC3 || filter == FILTER_UPRIGHT2P;
        cur_xy = a.take<float>(sm * 2); right_xy = a.take_if<float>(stereo, sm * 2); distance = a.take<double>(sm);
        lk = a.take<uint8_t>(sm); lk2 = a.take_if<uint8_t>(stereo, sm); lk3 = a.take_if<uint8_t>(stereo, sm); tracked_mask = a.take<uint8_t>(sm);
        track_status = a.take<int32_t>(sm); stereo_status = a.take_if<int32_t>(stereo, sm);
        draws2 = a.take<uint32_t>(s * 200); r2_status = a.take<int32_t>(sm); r2_R = a.take<float>(s * 9); r2_summary = a.take<int32_t>(s * 2);
        draws3 = a.take_if<uint32_t>(consensus, s * (size_t)n_filter_draws); r3_result = a.take<int32_t>(s * 2);
        score = a.take<double>(s); r3_summary = a.take_if<int32_t>(consensus, s * 4);
        keyframe = a.take<int32_t>(s); mask_xy = a.take<float>(sm * 2); n_mask = a.take<int32_t>(s); src_index = a.take<int32_t>(sm);
        kp = a.take_if<float>(detector != HV_DETECTOR_GFTT, s * (size_t)(detector == HV_DETECTOR_FAST ? max_kp : nk) * 3);
        corners = a.take<float>(sm * 2); n_corners = a.take<int32_t>(s);
        corners_right = a.take_if<float>(stereo, sm * 2); detection_status = a.take_if<int32_t>(stereo, sm);
        new_xy = a.take<float>(sm * 2); new_right = a.take_if<float>(stereo, sm * 2); n_new = a.take<int32_t>(s); n_added = a.take<int32_t>(s);

        keyframe_out = a.take<int32_t>(s); undo_active = a.take<uint8_t>(s); stationary = a.take<uint8_t>(s);
        draws_odo = a.take<uint32_t>(sm); draws_used = a.take<int32_t>(s);
        n_poses = a.take<int32_t>(v * s); pose_index = a.take<int32_t>(v * s * k);
        features = a.take<double>(v * s * pt * k); velocities = a.take<double>(v * s * pt * k); y = a.take<double>(v * s * pt * k);
        cand_id = a.take<int32_t>(v * s); n_candidates = a.take<int32_t>(s);
        status = a.take<int32_t>(v * s * 2); gate_status = a.take<int32_t>(v * s); pf = a.take<double>(v * s * 3);
        success = a.take<int32_t>(s); delete_ids = a.take<int32_t>(sm); n_delete = a.take<int32_t>(s);
        good_frame = a.take<uint8_t>(s); n_attempts = a.take<int32_t>(s); n_success = a.take<int32_t>(s); discarded = a.take<int32_t>(s);
        tracking_out = a.take<int32_t>(s); frozen = a.take<uint8_t>(s); reset_kind = a.take<int32_t>(s);
        // what only the sessions of hv_vio_create_session have, behind everything the default session carves
        r5_summary = a.take_if<int32_t>(filter == FILTER_HYBRID, s * 4);
        n_kp = a.take_if<int32_t>(detector != HV_DETECTOR_GPU_GFTT, s);          // FAST: n_kp_dev; legacy GFTT: n_cand_dev
        det_work = a.take_if<unsigned char>(det_work_bytes > 0, det_work_bytes);
    }

    // the visit loop of a frame, also run once by create over empty candidate lists: it grows the filter's visit buffers
    int visit_loop()
    {
        return hv_ekf_visual_frame_ragged_dev(ekf, &vu, V, K, n_poses, pose_index, features, velocities, y, r_gate, r_update, status,
                                              gate_status, nullptr, pf, success, p.trail.maxSuccessfulVisualUpdates);
    }
};

}  // namespace hv

struct hv_vio { hv::Vio v; };

using hv::Ctx;
using hv::Vio;

#define VIO_TRY(call)                                  \
    do {                                               \
        const int rc__ = (call);                       \
        if (rc__ != HV_OK) return rc__;                \
    } while (0)

namespace {

// the filter behind RANSAC2, chosen as RansacPipeline::compute chooses it (ransac_pipeline.cpp:121-136): RANSAC3 and the upright
// 2-point filter need two cameras (cameras.size() >= 2), so a mono session falls through them
int choose_filter(const hv_vio_params *p, bool stereo)
{
    if (p->useRansac3 && stereo) return hv::FILTER_RANSAC3;
    if (p->useStereoUpright2p && stereo) return hv::FILTER_UPRIGHT2P;
    return p->useHybridRansac ? hv::FILTER_HYBRID : hv::FILTER_NONE;
}

// the invalid arguments both constructors refuse first
int check_invalid(const hv_vio_params *p, int n_sets, hv_vio **out)
{
    if (!p || !out) return HV_ERR_INVALID;
    if (n_sets < 1 || p->imu_samples_max < 1 || p->imu_samples_max > HV_EKF_MAX_PREDICT_SAMPLES) return HV_ERR_INVALID;
    const int M = p->tracks.maxTracks;
    if (M < 1 || M != p->trail.maxTracks || M != p->gftt.maxTracks || M != p->output.maxTracks) return HV_ERR_INVALID;
    if (p->ekf.cameraTrailLength < 1 || p->ekf.cameraTrailLength != p->trail.cameraTrailLength ||
        p->ekf.cameraTrailLength != p->output.cameraTrailLength) return HV_ERR_INVALID;
    if (p->trail.maxVisualUpdates != p->output.maxVisualUpdates ||
        p->trail.maxSuccessfulVisualUpdates != p->output.maxSuccessfulVisualUpdates) return HV_ERR_INVALID;
    const bool st = p->trail.useStereo != 0;
    if (st != (p->output.useStereo != 0)) return HV_ERR_INVALID;          // (vu.useStereo is not read: the engine's copy takes trail's)
    if (p->session.visualUpdateForEveryNFrame < 1) return HV_ERR_INVALID;
    return HV_OK;
}

// what hv_vio_create decides before it looks at the context
int check_params(const hv_vio_params *p, int n_sets, hv_vio **out)
{
    VIO_TRY(check_invalid(p, n_sets, out));
    const bool st = p->trail.useStereo != 0;
    const int M = p->tracks.maxTracks;
    // outside the default stereo session
    if (!st || p->featureDetector != HV_DETECTOR_GPU_GFTT || !p->useRansac3 || p->gate.independentStereoOpticalFlow ||
        !p->predictOpticalFlow || p->batchVisualUpdate || p->trail.fullPointCloud || p->ekf.hybridMapSize > 0) return HV_ERR_UNSUPPORTED;
    if (n_sets > 65535 || p->ransac3.ransac3MaxIterations < 1 || 3 * (long long)p->ransac3.ransac3MaxIterations > HV_RNG_MAX_DRAWS ||
        M > HV_RNG_MAX_DRAWS) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}

// the raw draws a frame takes from the second tracker generator: 3 per RANSAC3 iteration, 2 per upright 2-point iteration
long long filter_draws(const hv_vio_params *p, int filter)
{
    if (filter == hv::FILTER_RANSAC3) return 3 * (long long)p->ransac3.ransac3MaxIterations;
    if (filter == hv::FILTER_UPRIGHT2P) return 2 * (long long)p->upright2p.ransacStereoUpright2pMaxIterations;
    return 0;
}

// what hv_vio_create_session decides before it looks at the context, in hv_vio_create's order
int check_session_params(const hv_vio_params *p, int n_sets, hv_vio **out)
{
    VIO_TRY(check_invalid(p, n_sets, out));
    const int M = p->tracks.maxTracks;
    switch (p->featureDetector) {
    case HV_DETECTOR_GPU_GFTT: break;                                        // gftt.maxTracks: checked above, whatever the detector
    case HV_DETECTOR_FAST: if (p->fast.maxTracks != M) return HV_ERR_INVALID; break;
    case HV_DETECTOR_GFTT: if (p->gftt_legacy.maxTracks != M) return HV_ERR_INVALID; break;
    default: return HV_ERR_INVALID;
    }
    if (p->gate.independentStereoOpticalFlow || !p->predictOpticalFlow || p->batchVisualUpdate || p->trail.fullPointCloud ||
        p->ekf.hybridMapSize > 0) return HV_ERR_UNSUPPORTED;
    const int filter = choose_filter(p, p->trail.useStereo != 0);
    const long long draws = filter_draws(p, filter);
    const bool consensus = filter == hv::FILTER_RANSAC3 || filter == hv::FILTER_UPRIGHT2P;
    if (n_sets > 65535 || (consensus && draws < 1) || draws > HV_RNG_MAX_DRAWS || M > HV_RNG_MAX_DRAWS) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}

int launch_score(Vio *v)
{
    Ctx *c = v->c;
    hv::ScoreArgs a{v->S, v->M, v->n_lk, v->track_status, v->r2_summary, v->score, v->r3_result};
    hv::ScopedKernelTime tm(c, HV_K_ROT_RANSAC);
    hipLaunchKernelGGL(hv::vio_ransac2_score_kernel, dim3((unsigned)((v->S + hv::VIO_THREADS - 1) / hv::VIO_THREADS)), dim3(hv::VIO_THREADS),
                       0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int launch_begin(Vio *v)
{
    Ctx *c = v->c;
    hv::BeginArgs a{v->S, v->p.session.visualUpdateForEveryNFrame, v->frame_no, v->trail.n_keyframes, v->table.n_tracks, v->has_prev,
                    v->full_update, v->prev_seen, v->n_lk, v->success, v->n_candidates, v->n_delete};
    hv::ScopedKernelTime tm(c, HV_K_EKF_CONTROL);
    hipLaunchKernelGGL(hv::vio_frame_begin_kernel, dim3((unsigned)((v->S + hv::VIO_THREADS - 1) / hv::VIO_THREADS)), dim3(hv::VIO_THREADS), 0,
                       c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int launch_end(Vio *v)
{
    Ctx *c = v->c;
    hv::EndArgs a{v->S, v->slot_prev, v->slot_cur, v->frame_no, v->has_prev, v->reset_kind};
    hv::ScopedKernelTime tm(c, HV_K_EKF_CONTROL);
    hipLaunchKernelGGL(hv::vio_frame_end_kernel, dim3((unsigned)((v->S + hv::VIO_THREADS - 1) / hv::VIO_THREADS)), dim3(hv::VIO_THREADS), 0,
                       c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

// everything of create behind the parameter checks; on failure the caller destroys the half-built engine
int build(Vio *v)
{
    Ctx *c = v->c;
    const hv_vio_params &p = v->p;
    v->M = p.tracks.maxTracks; v->K = p.trail.cameraTrailLength + 1; v->V = p.trail.maxVisualUpdates;
    {   // the ring size, as session.hip forms it (its entries check the range)
        const double w = (double)p.session.targetFps / (double)p.session.visualUpdateForEveryNFrame * p.session.goodFramesTimeWindowSeconds;
        if (!(w >= 1.0)) return HV_ERR_INVALID;
        if (w >= (double)HV_SESSION_MAX_WINDOW + 1.0) return HV_ERR_UNSUPPORTED;
        v->W = (int)(size_t)w;
    }
    if (v->V < 1 || v->V > HV_TRAIL_MAX_VISITS || v->K > HV_TRAIL_MAX_POSES || v->M > HV_TRACKS_MAX_TRACKS) return HV_ERR_UNSUPPORTED;
    v->n_filter_draws = (int)filter_draws(&p, v->filter);
    if (v->detector == HV_DETECTOR_GPU_GFTT) {
        v->nk = hv_gftt_keypoint_count(v->ctx, &p.gftt);
        if (v->nk < 0) return v->nk;
    } else {                                                                 // both bounds cannot overflow, so no image is refused for its count
        const bool fast = v->detector == HV_DETECTOR_FAST;
        v->max_kp = fast ? hv_fast_keypoint_bound(v->ctx) : hv_gftt_legacy_keypoint_bound(v->ctx);
        if (v->max_kp < 0) return v->max_kp;
        v->det_work_bytes = fast ? hv_fast_work_bytes(v->ctx, v->S) : hv_gftt_legacy_work_bytes(v->ctx, v->S, v->max_kp);
        if (v->det_work_bytes == 0) return HV_ERR_INVALID;
    }
    const double focal = (p.camera0.fx + p.camera0.fy) * 0.5;                  // Camera::getFocalLength (camera.cpp:37-39)
    v->r_gate = p.trackChiTestOutlierR / focal; v->r_update = p.visualR / focal;
    v->vu = p.vu;
    v->vu.useStereo = p.trail.useStereo;                                     // hv_vu_default_params leaves it 0: the index decides
    if (v->vu.trackRmseThreshold >= 0.0) v->vu.trackRmseThreshold /= focal;
    const double su = (double)(c->p.width < c->p.height ? c->p.width : c->p.height) / 720.0;      // ransac_pipeline.cpp:87-88
    v->threshold_pow2 = (float)((p.ransac2Threshold * su) * (p.ransac2Threshold * su));
    hv::mat4_mul(p.flow.imuToCamera, p.flow.secondCameraToImu, v->second_to_first);              // ransac_pipeline.cpp:225

    VIO_TRY(hv_ekf_create(v->ctx, &p.ekf, v->S, &v->ekf));
    const int per_set = v->stereo ? 3 : 2;
    for (int i = 0; i < per_set * v->S; i++) {
        int slot = -1;
        VIO_TRY(hv_pyramid_acquire(v->ctx, &slot));
        v->slots.push_back(slot);
    }
    hv::Carver size;
    v->carve(size);
    if (v->block.alloc(size.used + 256)) return HV_ERR_NOMEM;
    hv::Carver place;
    place.base = reinterpret_cast<unsigned char *>(((uintptr_t)v->block.get() + 255) & ~(uintptr_t)255);
    v->carve(place);
    HV_HIP(c, hipMemsetAsync(v->block, 0, v->block.count(), c->stream));
    // the slot roles of frame 0: set s holds slots 3 s (previous left: nothing yet), 3 s + 1 (current left), 3 s + 2 (right); a mono
    // session holds 2 s and 2 s + 1
    std::vector<int32_t> roles((size_t)per_set * v->S);
    for (int s = 0; s < v->S; s++)
        for (int r = 0; r < per_set; r++) roles[(size_t)r * v->S + s] = v->slots[(size_t)per_set * s + r];
    HV_HIP(c, hipMemcpyAsync(v->slot_prev, roles.data(), sizeof(int32_t) * v->S, hipMemcpyHostToDevice, c->stream));
    HV_HIP(c, hipMemcpyAsync(v->slot_cur, roles.data() + v->S, sizeof(int32_t) * v->S, hipMemcpyHostToDevice, c->stream));
    if (v->stereo)
        HV_HIP(c, hipMemcpyAsync(v->slot_right, roles.data() + 2 * (size_t)v->S, sizeof(int32_t) * v->S, hipMemcpyHostToDevice, c->stream));
    const std::vector<int32_t> first_num((size_t)v->S, 1);                  // frame->num = ++frameCount (sample_sync.cpp:138): the first frame is 1
    HV_HIP(c, hipMemcpyAsync(v->frame_no, first_num.data(), sizeof(int32_t) * v->S, hipMemcpyHostToDevice, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));                              // `roles` and `first_num` are pageable host memory

    VIO_TRY(hv_tracks_init_batch_dev(v->ctx, &p.tracks, v->S, &v->table));
    VIO_TRY(hv_trail_init_batch_dev(v->ctx, &p.trail, v->S, &v->trail));
    VIO_TRY(hv_session_init_dev(v->ekf, &p.session, &v->ses));
    VIO_TRY(hv_ekf_control_init_dev(v->ekf, &v->ctl));
    VIO_TRY(hv_rng_seed_batch_dev(v->ctx, v->S, &v->rng2, (uint32_t)p.ransacRngSeed, nullptr, nullptr));
    // (the second tracker generator is RANSAC3's own, ransac_pipeline.cpp:228, or the upright filter's, stereo_upright_2p.cpp:101;
    // a session whose filter draws nothing leaves it as it is seeded here)
    VIO_TRY(hv_rng_seed_batch_dev(v->ctx, v->S, &v->rng3, (uint32_t)p.ransacRngSeed, nullptr, nullptr));
    VIO_TRY(hv_rng_seed_batch_dev(v->ctx, v->S, &v->rng_odo, (uint32_t)p.odometryRngSeed, nullptr, nullptr));
    VIO_TRY(v->visit_loop());                                               // n_poses is all zero: nothing is visited, the buffers grow
    HV_HIP(c, hipStreamSynchronize(c->stream));
    return HV_OK;
}

}  // namespace

extern "C" {

void hv_vio_default_params(hv_vio_params *p)
{
    if (!p) return;
    *p = hv_vio_params{};
    hv_ekf_default_params(&p->ekf);
    hv_gftt_default_params(&p->gftt);
    hv_subpix_default_params(&p->subpix);
    hv_stereo_gate_default_params(&p->gate);
    hv_ransac3_default_params(&p->ransac3);
    hv_track_table_default_params(&p->tracks);
    hv_trail_index_default_params(&p->trail);
    hv_flow_predict_default_params(&p->flow);
    hv_vu_default_params(&p->vu);
    hv_ekf_control_default_params(&p->control);
    hv_session_default_params(&p->session);
    hv_output_default_params(&p->output);
    p->ransac2Threshold = 4.0;               // codegen/parameter_definitions.c: tracker.ransac2Threshold
    p->trackChiTestOutlierR = 1.5;           // odometry.trackChiTestOutlierR
    p->visualR = 0.05;                       // odometry.visualR
    p->ransacRngSeed = 4649;                 // tracker.ransacRngSeed
    p->odometryRngSeed = 0;                  // odometry.rngSeed
    p->imu_samples_max = HV_EKF_MAX_PREDICT_SAMPLES;
    p->featureDetector = HV_DETECTOR_GPU_GFTT;
    p->useRansac3 = 1; p->predictOpticalFlow = 1; p->batchVisualUpdate = 0;
    hv_ransac5_default_params(&p->ransac5);
    hv_upright2p_default_params(&p->upright2p);
    hv_fast_default_params(&p->fast);
    hv_gftt_legacy_default_params(&p->gftt_legacy);
    p->useStereoUpright2p = 0;               // tracker.useStereoUpright2p (parameter_definitions.c:298)
    p->useHybridRansac = 1;                  // tracker.useHybridRansac (:268)
}

}  // extern "C"

namespace {

// the part of both constructors behind the parameter checks: the context checks, then the engine
int create(hv_ctx *ctx, const hv_vio_params *p, int n_sets, bool stereo, int filter, int detector, hv_vio **out)
{
    *out = nullptr;
    Ctx *c = hv::ctx_of(ctx);
    if (!c) return HV_ERR_INVALID;
    if (c->p.max_tracks < p->tracks.maxTracks || c->free_slots.size() < (stereo ? 3 : 2) * (size_t)n_sets) return HV_ERR_INVALID;
    hv_vio *h = new (std::nothrow) hv_vio;
    if (!h) return HV_ERR_NOMEM;
    Vio *v = &h->v;
    v->c = c; v->ctx = ctx; v->p = *p; v->S = n_sets;
    v->stereo = stereo; v->filter = filter; v->detector = detector;
    const int rc = build(v);
    if (rc != HV_OK) { hv_vio_destroy(h); return rc; }
    *out = h;
    return HV_OK;
}

}  // namespace

extern "C" {

int hv_vio_create(hv_ctx *ctx, const hv_vio_params *p, int n_sets, hv_vio **out)
{
    VIO_TRY(check_params(p, n_sets, out));
    return create(ctx, p, n_sets, true, hv::FILTER_RANSAC3, HV_DETECTOR_GPU_GFTT, out);
}

int hv_vio_create_session(hv_ctx *ctx, const hv_vio_params *p, int n_sets, hv_vio **out)
{
    VIO_TRY(check_session_params(p, n_sets, out));
    const bool stereo = p->trail.useStereo != 0;
    return create(ctx, p, n_sets, stereo, choose_filter(p, stereo), p->featureDetector, out);
}

void hv_vio_destroy(hv_vio *h)
{
    if (!h) return;
    Vio *v = &h->v;
    if (v->c && v->c->stream) (void)hipStreamSynchronize(v->c->stream);     // nothing may still read the block or the slots
    if (v->ekf) hv_ekf_destroy(v->ekf);
    for (int slot : v->slots) (void)hv_pyramid_release(v->ctx, slot);
    delete h;
}

int hv_vio_sets(const hv_vio *h) { return h ? h->v.S : HV_ERR_INVALID; }

int hv_vio_replay_period(const hv_vio *h)
{
    // undo-augment and symmetrize-augment swap the covariance buffers once each in every frame, whatever their device masks say, so a
    // frame ends on the buffer it started on; slot roles and frame number are device data (vio_frame_end_kernel)
    return h ? 1 : HV_ERR_INVALID;
}

int hv_vio_view_get(hv_vio *h, hv_vio_view *o)
{
    if (!h || !o) return HV_ERR_INVALID;
    Vio *v = &h->v;
    *o = hv_vio_view{};
    o->ekf = v->ekf; o->table = v->table; o->trail = v->trail; o->session = v->ses; o->control = v->ctl;
    o->rng_pipeline = v->rng2; o->rng_ransac3 = v->rng3; o->rng_odometry = v->rng_odo; o->record = v->rec;
    o->frame_num = v->frame_no; o->has_previous = v->prev_seen; o->full_update = v->full_update; o->keyframe = v->keyframe;
    o->keyframe_out = v->keyframe_out; o->good_frame = v->good_frame; o->reset_kind = v->reset_kind; o->tracking_status = v->tracking_out;
    o->n_candidates = v->n_candidates; o->cand_id = v->cand_id; o->status = v->status; o->gate_status = v->gate_status;
    o->slot_prev_left = v->slot_prev; o->slot_cur_left = v->slot_cur; o->slot_right = v->slot_right;
    o->ransac_result = v->r3_result; o->ransac_score = v->score; o->r5_summary = v->r5_summary;
    return HV_OK;
}

int hv_vio_frame(hv_vio *h, const uint8_t *left_dev, const uint8_t *right_dev, long long image_stride_bytes, int row_stride_bytes,
                 int n_samples, const double *t_dev, const double *gyro_dev, const double *acc_dev)
{
    if (!h || !left_dev || !t_dev || !gyro_dev || !acc_dev) return HV_ERR_INVALID;
    Vio *v = &h->v;
    if ((right_dev != nullptr) != v->stereo) return HV_ERR_INVALID;         // a stereo session takes two images, a mono session one
    if (n_samples < 1 || n_samples > v->p.imu_samples_max) return HV_ERR_INVALID;
    const bool stereo = v->stereo;
    const hv_vio_params &p = v->p;
    hv_ctx *ctx = v->ctx; hv_ekf *ekf = v->ekf;
    const int S = v->S, M = v->M;
    const hv_camera_model *cam0 = &p.camera0, *cam1 = &p.camera1, *cam1s = stereo ? cam1 : nullptr;
    const hv_track_table *tab = &v->table;
    const hv_trail_index *trail = &v->trail;

    VIO_TRY(launch_begin(v));
    // 1. the pyramids, the images copied into the slots
    VIO_TRY(hv_ingest_build_batch_dev(ctx, S, v->slot_cur, left_dev, image_stride_bytes, row_stride_bytes, 1, -1));
    if (stereo) VIO_TRY(hv_ingest_build_batch_dev(ctx, S, v->slot_right, right_dev, image_stride_bytes, row_stride_bytes, 1, -1));
    // 2. the frame's IMU samples
    VIO_TRY(hv_session_imu_dev(ekf, &v->ses, n_samples, t_dev, acc_dev, nullptr, v->dt, v->time_rows));
    VIO_TRY(hv_ekf_predict_n_dev(ekf, n_samples, v->dt, gyro_dev, acc_dev));
    VIO_TRY(hv_ekf_normalize_quaternions(ekf, 1));
    const double *time = v->time_rows + (size_t)(n_samples - 1) * S;
    VIO_TRY(hv_ekf_imu_control_dev(ekf, &p.control, &v->ctl, time, nullptr));
    // 3. temporal LK from the predicted corners
    VIO_TRY(hv_flow_predict_batch_dev(ekf, &p.flow, HV_FLOW_PREDICT_LEFT, &p.trail, trail, tab, tab->xy, cam0, cam1, v->cur_xy, v->distance, 0));
    VIO_TRY(hv_klt_track_batch_ragged_dev(ctx, S, v->slot_prev, v->slot_cur, M, v->n_lk, tab->xy, v->cur_xy, v->lk, nullptr, 1, -1));
    VIO_TRY(hv_flow_status_batch_dev(ctx, S, M, v->n_lk, v->cur_xy, v->lk, v->track_status));
    if (stereo) {
        // 4. stereo LK, the distances reused
        VIO_TRY(hv_flow_predict_batch_dev(ekf, &p.flow, HV_FLOW_PREDICT_STEREO, &p.trail, trail, tab, v->cur_xy, cam0, cam1, v->right_xy, v->distance, 1));
        VIO_TRY(hv_klt_track_batch_ragged_dev(ctx, S, v->slot_cur, v->slot_right, M, v->n_lk, v->cur_xy, v->right_xy, v->lk2, nullptr, 1, -1));
        VIO_TRY(hv_flow_status_batch_dev(ctx, S, M, v->n_lk, v->right_xy, v->lk2, v->stereo_status));
    }
    // 5. gate (mono: right_xy and stereo_status are NULL, tracker.cpp:441-478 without its stereo parts), RANSAC2, the session's filter,
    //    each generator moved by what its filter consumed
    VIO_TRY(hv_track_gate_batch_dev(ctx, &p.gate, S, M, v->n_lk, v->cur_xy, v->right_xy, v->stereo_status, tab->blacklist, cam0, cam1s,
                                    v->track_status, v->tracked_mask));
    VIO_TRY(hv_rng_draw_batch_dev(ctx, S, &v->rng2, 200, v->draws2));
    VIO_TRY(hv_rot_ransac_lk_batch_dev(ctx, S, M, v->n_lk, tab->xy, v->cur_xy, v->tracked_mask, 1, cam0, cam0, v->draws2, v->threshold_pow2,
                                       v->r2_status, v->r2_R, v->r2_summary));
    VIO_TRY(hv_rng_advance_batch_dev(ctx, S, &v->rng2, v->r2_summary + 1, 2, 2, 200));
    const int nd = v->n_filter_draws;
    switch (v->filter) {
    case hv::FILTER_RANSAC3:
        VIO_TRY(hv_rng_draw_batch_dev(ctx, S, &v->rng3, nd, v->draws3));
        VIO_TRY(hv_ransac3_lk_batch_dev(ctx, &p.ransac3, S, M, v->n_lk, tab->xy, tab->second_xy, v->cur_xy, v->track_status, v->r2_summary, cam0,
                                        cam1, v->second_to_first, v->draws3, v->r3_result, v->score, nullptr, v->r3_summary));
        VIO_TRY(hv_rng_advance_batch_dev(ctx, S, &v->rng3, v->r3_summary + 2, 4, 3, nd));
        break;
    case hv::FILTER_UPRIGHT2P:                                               // the frame's predicts are done: the poses of backend.cpp:667-679
        VIO_TRY(hv_rng_draw_batch_dev(ctx, S, &v->rng3, nd, v->draws3));
        VIO_TRY(hv_upright2p_lk_batch_dev(ekf, &p.upright2p, &p.flow, M, v->n_lk, tab->xy, tab->second_xy, v->cur_xy, v->track_status,
                                          v->r2_summary, cam0, cam1, v->second_to_first, v->draws3, v->r3_result, v->score, nullptr,
                                          v->r3_summary));
        VIO_TRY(hv_rng_advance_batch_dev(ctx, S, &v->rng3, v->r3_summary + 2, 4, 2, nd));
        break;
    case hv::FILTER_HYBRID:                                                  // both cameras are camera0 (tracker.cpp:482-487)
        VIO_TRY(hv_hybrid_ransac_lk_batch_dev(ctx, &p.ransac5, S, M, v->n_lk, tab->xy, v->cur_xy, v->track_status, v->r2_status, v->r2_summary,
                                              cam0, cam0, v->r3_result, v->score, nullptr, v->r5_summary));
        break;
    default:
        VIO_TRY(launch_score(v));
        break;
    }
    // 6. the table, the detection of new corners (sub-pixel refinement behind every detector, image.cpp:69-85), the append
    VIO_TRY(hv_tracks_update_batch_dev(ctx, &p.tracks, S, tab, v->cur_xy, v->right_xy, v->track_status, v->score, v->keyframe, v->mask_xy,
                                       v->n_mask, v->src_index, nullptr));
    switch (v->detector) {
    case HV_DETECTOR_GPU_GFTT:
        VIO_TRY(hv_gftt_detect_batch_dev(ctx, &p.gftt, S, v->slot_cur, v->kp, M, v->n_mask, v->mask_xy, tab->mask_radius, M, v->corners, v->n_corners));
        break;
    case HV_DETECTOR_FAST:
        VIO_TRY(hv_fast_detect_batch_dev(ctx, &p.fast, S, v->slot_cur, v->det_work, v->max_kp, v->kp, v->n_kp, M, v->n_mask, v->mask_xy,
                                         tab->mask_radius, M, v->corners, v->n_corners));
        break;
    default:
        VIO_TRY(hv_gftt_legacy_detect_batch_dev(ctx, &p.gftt_legacy, S, v->slot_cur, v->det_work, v->max_kp, v->n_kp, M, v->n_mask, v->mask_xy,
                                                tab->mask_radius, M, v->corners, nullptr, v->n_corners));
        break;
    }
    VIO_TRY(hv_corner_subpix_batch_dev(ctx, &p.subpix, S, v->slot_cur, M, v->n_corners, v->corners, nullptr));
    if (stereo) {
        VIO_TRY(hv_klt_track_batch_ragged_dev(ctx, S, v->slot_cur, v->slot_right, M, v->n_corners, v->corners, v->corners_right, v->lk3, nullptr, 0, -1));
        VIO_TRY(hv_flow_status_batch_dev(ctx, S, M, v->n_corners, v->corners_right, v->lk3, v->detection_status));
    }
    // (mono: no stereo LK of the new corners, every one starts TRACKED, tracker.cpp:291)
    VIO_TRY(hv_detection_filter_batch_dev(ctx, &p.gate, S, M, v->n_corners, v->corners, v->corners_right, v->detection_status, cam0, cam1s, nullptr,
                                          v->new_xy, v->new_right, v->n_new));
    VIO_TRY(hv_tracks_append_batch_dev(ctx, &p.tracks, S, tab, M, v->n_new, v->new_xy, v->new_right, v->n_added));
    // 7. the control part of the frame
    VIO_TRY(hv_ekf_frame_control_dev(ekf, &p.control, &v->ctl, time, v->keyframe, v->full_update, v->keyframe_out, v->undo_active, v->stationary, nullptr));
    VIO_TRY(hv_ekf_undo_augment_dev(ekf, v->undo_active));
    // 8. track selection and the visit loop
    VIO_TRY(hv_rng_draw_batch_dev(ctx, S, &v->rng_odo, M, v->draws_odo));
    VIO_TRY(hv_trail_select_batch_dev(ctx, &p.trail, S, trail, tab, cam0, cam1, v->keyframe_out, v->full_update, v->frame_no, time, v->draws_odo,
                                      v->draws_used, v->n_poses, v->pose_index, v->features, v->velocities, v->y, v->cand_id, v->n_candidates));
    VIO_TRY(v->visit_loop());
    VIO_TRY(hv_rng_advance_batch_dev(ctx, S, &v->rng_odo, v->draws_used, 1, 1, M));
    VIO_TRY(hv_trail_finish_batch_dev(ctx, &p.trail, S, trail, v->cand_id, v->n_candidates, v->status, v->gate_status, v->stationary, v->delete_ids,
                                      v->n_delete, v->good_frame, v->n_attempts, v->n_success, v->discarded));
    // 9. blacklisted tracks leave the table; the augmentation
    VIO_TRY(hv_tracks_delete_batch_dev(ctx, &p.tracks, S, tab, M, v->n_delete, v->delete_ids));
    VIO_TRY(hv_ekf_symmetrize_augment_dev(ekf, v->discarded, nullptr));
    // 10. tracking status, the record, the reset where one was decided (with the tracker generators of the sets that reset)
    VIO_TRY(hv_session_status_dev(ekf, &p.session, &v->ses, v->good_frame, v->full_update, v->tracking_out, v->frozen, v->reset_kind));
    const hv_output_frame of{v->cand_id, v->n_candidates, v->status, v->gate_status, v->pf, v->tracking_out, v->frozen, v->stationary,
                             nullptr, nullptr, nullptr};
    VIO_TRY(hv_output_dev(ekf, &p.output, &v->ses, trail, &of, &v->rec));
    VIO_TRY(hv_session_reset_dev(ekf, &p.session, &v->ses, &v->ctl, &p.tracks, tab, &p.trail, trail, v->reset_kind));
    VIO_TRY(hv_rng_seed_batch_dev(ctx, S, &v->rng2, (uint32_t)p.ransacRngSeed, nullptr, v->reset_kind));
    if (nd > 0) VIO_TRY(hv_rng_seed_batch_dev(ctx, S, &v->rng3, (uint32_t)p.ransacRngSeed, nullptr, v->reset_kind));
    return launch_end(v);
}

}  // extern "C"
