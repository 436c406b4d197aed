// Device full point cloud for a batch of resident sequences (set s is filter s): odometry.fullPointCloud, "triangulate all tracks
// on each frame to get the full point cloud" (codegen/parameter_definitions.c:54-56). With it the visit loop of
// Session::trackerVisualUpdate (backend.cpp:1012-1252) does not break at its limits (:1242-1247): the stopping candidate reaches
// the push at :1249-1251, and every later track of the shuffled order that passes the filter of :1017-1038 (the previous-blacklist
// test of :1039-1046 is conditioned on needMoreVisualUpdates and skips nothing behind the stop) is triangulated from the mean as
// the frame's updates left it (:1048-1099), counted as an update attempt (:1121) and appended when its status is OK (:1126-1132).
// Nothing is gated, applied, marked used, blacklisted or deleted. Restatement: tests/full_cloud_restatement.py.
//
// Reference: backend.cpp:1012-1252, 1269-1274; ekf_state_index.cpp:41-87 (trackScore), :90-147 (createTrackIndex), :192-218
// (buildTrackVectors); triangulation.cpp:65-103 (extractCameraPoseTrail), :120-407 (Triangulator::triangulate, the iterative method
// without calculateDerivatives: the derivative code only accumulates into dpfi / dETE / dEerror and never feeds back into pfi,
// rcond, J or isBehind), :612-646 (triangulateWithTwoCameras), :1004-1012 (inverseDepth), :54-60 (isBehind).
//
// Two kernels:
// - full_cloud_index_kernel, one workgroup per set: derives again from the table and the index as select left it what
//   trail_select_kernel held in LDS (slot -> column, trackScore, nValid, the shuffled order, minTrackScore: the functions of
//   trail_phases.hpp, one statement of each rule), finds the stop from the visit statuses by the rule of trail_finish_kernel and
//   output_kernel, writes the prefix of the cloud (the visited candidates up to and including the stopping one) and the tail list
//   with the pose mask of every track.
// - full_cloud_tri_kernel, one workgroup per set, ONE LANE PER TAIL TRACK: every track of a set reads the same pose trail, and
//   its pose 0 is always keyframe 0 (the head's observation is new, hence never `used`), so the per-pose constants of the
//   Gauss-Newton loop, C_i = R_i R_0' and t_i = R_i (p_0 - p_i), are per SET, not per track: they are built once in LDS and a
//   lane's iteration is ~70 flops per observation on three scalars of state. A lane sums its observations in the oracle's own
//   order (first camera's poses ascending, then the second's), so the result does not depend on the launch shape. The epilogue
//   compacts the OK tracks in tail order behind the prefix.
// Everything is binary64 and uncontracted (the build's -ffp-contract=off).
#include <math.h>

#include "ekf_host.hpp"

namespace hv {
namespace {

#include "hv_geometry.hpp"        // mm3, mmT3, mv3, mTv3, quat2rmat_d, pinv32
#include "hv_triangulation.hpp"   // pos_ori, camera_pose_pR, triangulate_two, gn_observation, inverse_depth, inv3sym, norm1_3
#include "hv_workgroup.hpp"       // clampi, block_compact
#include "trail_phases.hpp"       // trail_track_score, trail_order_phase, trail_filter_skips

constexpr int FC_THREADS = 256, FC_WAVES = FC_THREADS / 64;     // the index kernel
constexpr int FT_THREADS = 128, FT_WAVES = FT_THREADS / 64;     // the triangulation kernel: ~100 tail tracks per set at the defaults
constexpr int FC_MAX = HV_TRACKS_MAX_TRACKS, FC_CHUNKS = FC_MAX / 64;
constexpr int FC_MAX_POSES = HV_TRAIL_MAX_POSES, FC_MAX_VISITS = HV_TRAIL_MAX_VISITS;
constexpr int FAILED_UPDATES_THRESHOLD = 5;                     // backend.cpp:1272
constexpr int GATE_INLIER = 0;                                  // VuOutlierStatus::INLIER
constexpr int POINT_POSE_TRAIL = 1, POINT_OUTLIER = 4;          // PointFeature::Status
constexpr int POSE_REC = 24;                                    // p[3] R[9] C[9] t[3] of a (camera, keyframe)
static_assert(FC_MAX_VISITS <= 64, "one wavefront over the candidates of a set");
static_assert(FC_MAX_POSES <= 64, "tail_pose_mask is one 64-bit word");

struct FullCloudArgs {
    hv_trail_index t;
    hv_full_cloud_frame in;
    hv_full_cloud out;
    int M, K, ncam, V, n_sets, n_state;
    int sampling, min_frames, score_tracks, max_success;
    const int32_t *n_tracks, *ids;
    const double *m;                           // [n_sets][n_state] means
    double imu_to_cam[2][16];
    double conv_threshold, conv_r, rcond_threshold, min_dist, max_dist;
    int gn_iters;
};

// transformVec3ByMat4(odometryToSlam, point), in the order of output_kernel
__device__ inline void to_slam(const double *o2s, const double *pf, double *out)
{
    for (int i = 0; i < 3; ++i) out[i] = ((o2s[4 * i] * pf[0] + o2s[4 * i + 1] * pf[1]) + o2s[4 * i + 2] * pf[2]) + o2s[4 * i + 3];
}

__device__ inline void stage_o2s(const FullCloudArgs &a, int set, double *s_o2s)
{
    if (threadIdx.x < 16)
        s_o2s[threadIdx.x] = a.in.odometry_to_slam_dev ? a.in.odometry_to_slam_dev[(size_t)set * 16 + threadIdx.x] : (threadIdx.x % 5 == 0 ? 1.0 : 0.0);
}

__global__ __launch_bounds__(FC_THREADS) void full_cloud_index_kernel(FullCloudArgs a)
{
    __shared__ int s_cid[FC_MAX];        // column -> track ID
    __shared__ int s_len[FC_MAX];        // column -> keyframes holding the track (0: free)
    __shared__ int s_col[FC_MAX];        // table slot -> column (-1: the track is not in the index)
    __shared__ int s_nvalid[FC_MAX];     // table slot -> nValid (-1: not in the order)
    __shared__ float s_score[FC_MAX];    // table slot -> trackScore
    __shared__ int s_list[FC_MAX];       // trackOrder
    __shared__ int s_draw[FC_MAX];       // the draws; then the tail's positions
    __shared__ int s_trunc[FC_MAX];      // the truncated scores
    __shared__ int s_chunk[FC_CHUNKS + 1];
    __shared__ int s_row[FC_MAX_POSES];
    __shared__ double s_o2s[16];
    __shared__ int s_min;
    __shared__ int s_ctl[4];             // stop position, points of the prefix, attempts, successes

    const int set = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int M = a.M, K = a.K, V = a.V, ncam = a.ncam;
    const int n = clampi(a.n_tracks[set], 0, M);
    const int n_kf = clampi(a.t.n_keyframes[set], 1, K);
    const bool full = a.in.full_update_dev ? a.in.full_update_dev[set] != 0 : true;
    const bool ready = a.in.ready_dev ? a.in.ready_dev[set] != 0 : true;
    const int32_t *ids = a.ids + (size_t)set * M;
    for (int c = tid; c < M; c += FC_THREADS) {
        s_cid[c] = a.t.col_id[(size_t)set * M + c];
        s_len[c] = clampi(a.t.col_len[(size_t)set * M + c], 0, n_kf);
    }
    if (tid < K) s_row[tid] = clampi(a.t.kf_row[(size_t)set * K + tid], 0, K - 1);
    stage_o2s(a, set, s_o2s);
    __syncthreads();

    // ---- slot -> column, trackScore, nValid: a table track that select inserted owns the column with its ID ----
    const int row0 = s_row[0];
    for (int i = tid; i < n; i += FC_THREADS) {
        const int id = ids[i];
        int c = -1;
        for (int q = 0; q < M; ++q) c = (s_len[q] > 0 && s_cid[q] == id) ? q : c;   // IDs are unique: at most one column matches
        s_col[i] = c;
        int n_valid = -1;
        float score = 0.0f;
        if (c >= 0) {
            const float2 head = *reinterpret_cast<const float2 *>(a.t.image_point + trail_obs_at(K, M, ncam, set, row0, c, 0));
            score = trail_track_score(a.t, K, M, ncam, a.sampling, s_row, set, c, s_len[c], head.x, head.y, n_valid);
        }
        s_score[i] = score;
        s_nvalid[i] = n_valid;
    }
    __syncthreads();
    const int n_ord = block_compact<FC_WAVES>([&](int i) { return s_nvalid[i] >= 0; }, s_list, n, s_chunk);
    const float min_score = trail_order_phase<FC_THREADS>(a.score_tracks, a.in.draws_dev + (size_t)set * M, n_ord, s_score, s_list, s_draw, s_trunc, &s_min);

    // ---- the visit loop's counters and its stop (backend.cpp:1121, 1188, 1240-1247), the prefix of the cloud (:1249-1251): one
    // lane per candidate, as output_kernel; here the stopping candidate is pushed too ----
    if (tid < 64) {
        const int n_cand = clampi(a.in.n_candidates_dev[set], 0, V);
        const size_t rec = (size_t)lane * a.n_sets + set;
        int kind = 0, tri = HV_TRI_NOT_VISITED, prep = 0;                      // 0 not visited, 1 success, 2 visited without an inlier
        if (lane < n_cand) {
            tri = a.in.status_dev[2 * rec]; prep = a.in.status_dev[2 * rec + 1];
            if (tri != HV_TRI_NOT_VISITED) kind = a.in.gate_status_dev[rec] == GATE_INLIER ? 1 : 2;
        }
        const unsigned long long below = (1ull << lane) - 1ull, upto = below | (1ull << lane);
        const unsigned long long visited = __ballot(kind != 0), success = __ballot(kind == 1);
        const int attempts = __popcll(visited & upto), successes = __popcll(success & upto);
        const unsigned long long stops = __ballot(kind != 0 && ((a.max_success > 0 && successes >= a.max_success) || attempts >= V));
        const int stop = stops ? __ffsll((long long)stops) - 1 : 64;
        const bool push = ready && kind != 0 && lane <= stop && tri == HV_TRI_OK;
        const unsigned long long pushed = __ballot(push);
        if (push) {
            const size_t o = (size_t)set * M + __popcll(pushed & below);
            a.out.point_id[o] = a.in.cand_id_dev[rec];
            // OUTLIER only behind the gate (:1157-1194): a track whose prepareVisualUpdate failed keeps POSE_TRAIL (:1118)
            a.out.point_status[o] = (prep == HV_PREPARE_VU_OK && kind == 2) ? POINT_OUTLIER : POINT_POSE_TRAIL;
            // track.points[0] (:1069): the first camera's corner select stored in the head
            const int col = clampi(a.t.cand_col[(size_t)set * V + lane], 0, M - 1);
            const size_t ip = trail_obs_at(K, M, ncam, set, row0, col, 0);
            a.out.point_first_pixel[2 * o] = a.t.image_point[ip]; a.out.point_first_pixel[2 * o + 1] = a.t.image_point[ip + 1];
            to_slam(s_o2s, a.in.pf_dev + 3 * rec, a.out.point_xyz + 3 * o);
        }
        if (lane == (stops ? stop : 0)) {
            const unsigned long long counted = stops ? upto : ~0ull;             // a loop that never stopped counted every visit
            s_ctl[0] = stops ? clampi(a.t.cand_pos[(size_t)set * V + stop], 0, M) : n_ord;
            s_ctl[1] = __popcll(pushed);
            s_ctl[2] = __popcll(visited & counted);
            s_ctl[3] = __popcll(success & counted);
        }
    }
    __syncthreads();
    const int stop_pos = s_ctl[0], n_prefix = s_ctl[1], visits = s_ctl[2], successes = s_ctl[3];
    const bool stopped = stop_pos < n_ord;

    // ---- the tail: every later track of the order that the filter lets through (:1017-1038), blacklisted or not ----
    const int n_tail = block_compact<FC_WAVES>([&](int p) {
        if (p <= stop_pos) return false;
        const int slot = s_list[p];
        return !trail_filter_skips(a.score_tracks, s_score[slot], min_score, s_nvalid[slot], a.min_frames, full);
    }, s_draw, n_ord, s_chunk);
    for (int k = tid; k < n_tail; k += FC_THREADS) {
        const int c = s_col[s_list[s_draw[k]]], len = s_len[c];
        unsigned long long mask = 0ull;                                        // createTrackIndex (:90-147), GAP or ALL
        for (int j = 0; j < len; ++j) {
            const bool use = a.sampling == HV_TRACK_SAMPLING_ALL || j == len - 1 || a.t.used[trail_used_at(K, M, set, s_row[j], c)] == 0;
            mask |= use ? 1ull << j : 0ull;
        }
        const size_t o = (size_t)set * M + k;
        a.out.tail_id[o] = s_cid[c];
        a.out.tail_col[o] = c;
        a.out.tail_pose_mask[o] = mask;
    }
    if (tid == 0) {
        a.out.n_tail[set] = n_tail;
        a.out.n_points[set] = n_prefix;                                        // the triangulation kernel adds the tail's
        const int attempts = visits + n_tail;                                  // :1121 counts every triangulated track
        if (a.out.n_attempts) a.out.n_attempts[set] = attempts;
        if (a.out.good_frame) {
            const bool stationary = a.in.stationary_dev ? a.in.stationary_dev[set] != 0 : false;
            a.out.good_frame[set] = ((stationary || stopped) && !(attempts - successes > FAILED_UPDATES_THRESHOLD)) ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(FT_THREADS) void full_cloud_tri_kernel(FullCloudArgs a)
{
    __shared__ double s_pose[2 * FC_MAX_POSES * POSE_REC];   // (camera, keyframe) -> p[3] R[9] C[9] t[3]
    __shared__ double s_o2s[16];
    __shared__ int s_row[FC_MAX_POSES];
    __shared__ int s_wcount[FT_WAVES];

    const int set = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = a.M, K = a.K, ncam = a.ncam;
    const int n_tail = clampi(a.out.n_tail[set], 0, M);
    if (n_tail == 0) return;                                                   // (uniform: nothing behind the stop, n_points is final)
    const int n_kf = clampi(a.t.n_keyframes[set], 1, K);
    const bool ready = a.in.ready_dev ? a.in.ready_dev[set] != 0 : true;
    const double *m = a.m + (size_t)set * a.n_state;

    // ---- extractCameraPoseTrail (triangulation.cpp:65-103) of every keyframe, both cameras; then the constants of the loop ----
    for (int i = tid; i < ncam * n_kf; i += FT_THREADS) {
        const int cam = i / n_kf, k = i - cam * n_kf;
        int ip, io;
        pos_ori(k, ip, io);                                                    // keyframe k is historyPosition(k - 1), keyframe 0 the current pose
        camera_pose_pR(m, ip, io, a.imu_to_cam[cam], s_pose + (cam * K + k) * POSE_REC);
    }
    if (tid < K) s_row[tid] = clampi(a.t.kf_row[(size_t)set * K + tid], 0, K - 1);
    stage_o2s(a, set, s_o2s);
    __syncthreads();
    const double *P0 = s_pose, *R0 = s_pose + 3;                               // trail[0]: the first camera at keyframe 0
    for (int i = tid; i < ncam * n_kf; i += FT_THREADS) {
        const int cam = i / n_kf, k = i - cam * n_kf;
        double *o = s_pose + (cam * K + k) * POSE_REC;
        double C[9], d[3], t[3];
        mmT3(o + 3, R0, C);                                                    // cur.R * R0' (:216)
        for (int j = 0; j < 3; ++j) d[j] = P0[j] - o[j];
        mv3(o + 3, d, t);
        for (int j = 0; j < 9; ++j) o[12 + j] = C[j];
        for (int j = 0; j < 3; ++j) o[21 + j] = t[j];
    }
    __syncthreads();

    const unsigned long long kf_bits = n_kf >= 64 ? ~0ull : (1ull << n_kf) - 1ull;
    const double r_noise = a.conv_r * a.conv_r;
    int base = clampi(a.out.n_points[set], 0, M);                              // the prefix the index kernel wrote
    for (int k0 = 0; k0 < n_tail; k0 += FT_THREADS) {
        const int k = k0 + tid;
        int status = HV_TRI_NOT_VISITED;
        double pf[3] = {0.0, 0.0, 0.0};
        int col = 0;
        if (k < n_tail) {
            const size_t ot = (size_t)set * M + k;
            col = clampi(a.out.tail_col[ot], 0, M - 1);
            const unsigned long long mask = (a.out.tail_pose_mask[ot] & kf_bits) | 1ull;   // pose 0 is keyframe 0
            const int last = 63 - __clzll((long long)mask);                    // ind1: the last pose of the first camera (:154)
            // ---- triangulateWithTwoCameras (:154-173) and inverseDepth ----
            const double *f0 = a.t.norm_point + trail_obs_at(K, M, ncam, set, s_row[0], col, 0);
            const double *f1 = a.t.norm_point + trail_obs_at(K, M, ncam, set, s_row[last], col, 0);
            const double ip0[2] = {f0[0], f0[1]}, ip1[2] = {f1[0], f1[1]};
            triangulate_two(P0, s_pose + last * POSE_REC, ip0, ip1, pf);
            double pfi[3], dip[9];
            inverse_depth(pf, pfi, dip);
            // ---- Gauss-Newton (:206-343), points only ----
            double rcond = 0.0, j_prev = 1e10;
            bool converged = false;
            for (int it = 0; it < a.gn_iters && !converged; ++it) {
                double ETE[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Ee[3] = {0, 0, 0}, error2 = 0.0;
                for (int cam = 0; cam < ncam; ++cam) {
                    unsigned long long rest = mask;
                    while (rest) {
                        const int kf = __ffsll((long long)rest) - 1;
                        rest &= rest - 1ull;
                        const double *o = s_pose + (cam * K + kf) * POSE_REC, *C = o + 12, *t = o + 21;
                        const double *y = a.t.norm_point + trail_obs_at(K, M, ncam, set, s_row[kf], col, cam);
                        double h[3], E[6], err[2];
                        gn_observation(C, t, pfi, y, h, E, err);
                        error2 += err[0] * err[0] + err[1] * err[1];
                        for (int r = 0; r < 3; ++r) {
                            for (int c = r; c < 3; ++c) ETE[3 * r + c] += E[r] * E[c] + E[3 + r] * E[3 + c];   // symmetric: the upper triangle
                            Ee[r] += E[r] * err[0] + E[3 + r] * err[1];
                        }
                    }
                }
                ETE[3] = ETE[1]; ETE[6] = ETE[2]; ETE[7] = ETE[5];
                double X[9], step[3];
                inv3sym(ETE, X);
                mv3(X, Ee, step);
                for (int r = 0; r < 3; ++r) pfi[r] -= step[r];
                rcond = 1.0 / (norm1_3(ETE) * norm1_3(X));                     // :313-315
                const double J = 0.5 * error2 / r_noise, Jd = fabs((J - j_prev) / J);
                j_prev = J;
                converged = Jd < a.conv_threshold;
            }
            // ---- status, back to world coordinates (:345-407) ----
            status = HV_TRI_OK;
            if (!converged) status = HV_TRI_NO_CONVERGENCE;
            else if (rcond < a.rcond_threshold) status = HV_TRI_BAD_COND;
            if (status == HV_TRI_OK) {
                double pf0[3], w[3];
                inverse_depth(pfi, pf0, dip);
                mTv3(R0, pf0, w);                                              // R0' pf0
                for (int r = 0; r < 3; ++r) pf[r] = w[r] + P0[r];
                if (pf[0] == P0[0] && pf[1] == P0[1] && pf[2] == P0[2]) status = HV_TRI_UNKNOWN_PROBLEM;
                else {
                    bool behind = false;                                       // isBehind (:54-60): any pose decides, so no order
                    for (int cam = 0; cam < ncam; ++cam) {
                        unsigned long long rest = mask;
                        while (rest) {
                            const int kf = __ffsll((long long)rest) - 1;
                            rest &= rest - 1ull;
                            const double *o = s_pose + (cam * K + kf) * POSE_REC;
                            const double dd[3] = {pf[0] - o[0], pf[1] - o[1], pf[2] - o[2]};
                            behind = behind || (o[9] * dd[0] + o[10] * dd[1] + o[11] * dd[2] < 0);
                        }
                    }
                    if (behind) status = HV_TRI_BEHIND;
                }
            }
            {   // backend.cpp:1096-1099: the depth window on whatever point the triangulation left behind
                const double dx = pf[0] - P0[0], dy = pf[1] - P0[1], dz = pf[2] - P0[2], depth = sqrt(dx * dx + dy * dy + dz * dz);
                if (depth < a.min_dist || depth > a.max_dist) status = HV_TRI_BAD_DEPTH;
            }
            a.out.tail_status[ot] = status;
        }
        // ---- the OK tracks behind the prefix, in tail order (:1126-1129) ----
        const bool push = ready && status == HV_TRI_OK;
        const unsigned long long pushed = __ballot(push);
        if (lane == 0) s_wcount[wave] = __popcll(pushed);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < FT_WAVES; ++w) { before += w < wave ? s_wcount[w] : 0; total += s_wcount[w]; }
        if (push) {
            const int pos = base + before + __popcll(pushed & ((1ull << lane) - 1ull));
            if (pos < M) {                                                     // (always: prefix and tail are distinct tracks of the order)
                const size_t o = (size_t)set * M + pos;
                a.out.point_id[o] = a.out.tail_id[(size_t)set * M + k];
                a.out.point_status[o] = POINT_POSE_TRAIL;
                const size_t ip = trail_obs_at(K, M, ncam, set, s_row[0], col, 0);
                a.out.point_first_pixel[2 * o] = a.t.image_point[ip]; a.out.point_first_pixel[2 * o + 1] = a.t.image_point[ip + 1];
                to_slam(s_o2s, pf, a.out.point_xyz + 3 * o);
            }
        }
        base = min(base + total, M);
        __syncthreads();                                                       // s_wcount is rewritten by the next chunk
    }
    if (tid == 0) a.out.n_points[set] = base;
}

}  // namespace
}  // namespace hv

extern "C" {

int hv_full_point_cloud_dev(hv_ekf *h, const hv_trail_index_params *tp, const hv_vu_params *vp, const hv_trail_index *trail,
                            const hv_track_table *table, const hv_full_cloud_frame *in, const hv_full_cloud *out)
{
    if (const int rc = hv::trail_check_params(tp, 0)) return rc;
    if (const int rc = hv::trail_check_state(trail)) return rc;
    if (!vp || !table || !table->n_tracks || !table->ids || !in || !out) return HV_ERR_INVALID;
    if (!in->draws_dev || !in->cand_id_dev || !in->n_candidates_dev || !in->status_dev || !in->gate_status_dev || !in->pf_dev)
        return HV_ERR_INVALID;
    if (!out->n_points || !out->point_id || !out->point_status || !out->point_first_pixel || !out->point_xyz || !out->n_tail ||
        !out->tail_id || !out->tail_status || !out->tail_col || !out->tail_pose_mask)
        return HV_ERR_INVALID;
    if ((tp->useStereo != 0) != (vp->useStereo != 0)) return HV_ERR_INVALID;   // one index, one camera rig
    if (const int rc = hv::trail_check_limits(tp, 0)) return rc;
    if (vp->useLinearTriangulation) return HV_ERR_UNSUPPORTED;                 // the tail states the iterative method only
    if (!h) return HV_ERR_INVALID;
    hv::Ekf *e = &h->e;
    hv::Ctx *c = e->c;
    if (e->batch > 65535 || e->n < 20 + 7 * tp->cameraTrailLength) return HV_ERR_UNSUPPORTED;
    if (e->batch == 0) return HV_OK;
    hv::FullCloudArgs a{};
    a.t = *trail; a.in = *in; a.out = *out;
    a.M = tp->maxTracks; a.K = tp->cameraTrailLength + 1; a.ncam = tp->useStereo ? 2 : 1; a.V = tp->maxVisualUpdates;
    a.n_sets = e->batch; a.n_state = e->n;
    a.sampling = tp->trackSampling; a.min_frames = tp->trackMinFrames; a.score_tracks = tp->scoreVisualUpdateTracks;
    a.max_success = tp->maxSuccessfulVisualUpdates;
    a.n_tracks = table->n_tracks; a.ids = table->ids;
    a.m = e->fixed.m;
    for (int i = 0; i < 16; ++i) { a.imu_to_cam[0][i] = vp->imuToCamera[i]; a.imu_to_cam[1][i] = vp->secondImuToCamera[i]; }
    a.conv_threshold = vp->triangulationConvergenceThreshold; a.conv_r = vp->triangulationConvergenceR;
    a.rcond_threshold = vp->triangulationRcondThreshold; a.min_dist = vp->triangulationMinDist; a.max_dist = vp->triangulationMaxDist;
    a.gn_iters = (int)vp->triangulationGaussNewtonIterations;
    {
        hv::ScopedKernelTime tm(c, HV_K_TRAIL_INDEX);
        hipLaunchKernelGGL(hv::full_cloud_index_kernel, dim3((unsigned)e->batch), dim3(hv::FC_THREADS), 0, c->stream, a);
        HV_HIP(c, hipGetLastError());
    }
    {
        hv::ScopedKernelTime tm(c, HV_K_VU_TRI);
        hipLaunchKernelGGL(hv::full_cloud_tri_kernel, dim3((unsigned)e->batch), dim3(hv::FT_THREADS), 0, c->stream, a);
        HV_HIP(c, hipGetLastError());
    }
    return HV_OK;
}

}  // extern "C"
