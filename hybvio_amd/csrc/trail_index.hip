// Device pose-trail index: odometry::EKFStateIndex and the part of Session::trackerVisualUpdate around the visit loop, for many
// resident sequences at once.
//
// Reference: src/odometry/ekf_state_index.{hpp,cpp} (pushHeadKeyframe :23-31, popHeadKeyframe :33-39, trackScore :41-87,
// createTrackIndex :90-147, markTrackUsed :156-181, buildTrackVectors :192-218, prune :220-242, removeKeyframe :244-281,
// updateVelocities :361-384), src/odometry/backend.cpp:793-805, 909-1052, 1189-1213, 1240-1243, 1269-1274 and
// util::shuffleDeterministic (src/util/util.hpp:39-44).
//
// Representation. The reference keeps a vector of keyframes, each with a map from track ID to Feature. Here a
// keyframe is a row and a live track a column of the observation arrays; kf_row maps a keyframe (0 = head) to its physical row, so
// push, pop and remove rotate kf_row and move no observation. After prune() a track sits in the keyframes 0 .. len - 1 and nowhere
// else ("tracks have no gaps", ekf_state_index.cpp:52,105: an observation only ever enters the head, and a track that misses the
// head is erased everywhere), so col_len is the whole membership relation: keyframe i is empty exactly when no column is longer
// than i, prune() is "columns that were not inserted this frame are free", and removing keyframe r shortens the columns longer
// than r by one.
//
// One workgroup of 256 threads per set, a thread loop over the track slots. IDs are matched on lists staged in LDS; lists are
// compacted in order with a wave64 ballot, the lane prefix count and per-chunk offsets; the median of the truncated scores is a
// rank count (no sort, no atomics); the shuffle is the one sequential chain and runs on one lane over the order in LDS; the
// gather runs one wavefront per candidate. Arithmetic that the restatement rounds once is written with the _rn intrinsics.
#include "fresh_state.hpp"
#include "hv_camera.hpp"

namespace hv {
namespace {

constexpr int TI_THREADS = 256, TI_WAVES = TI_THREADS / 64;
constexpr int TI_MAX = HV_TRACKS_MAX_TRACKS, TI_CHUNKS = TI_MAX / 64;
constexpr int TI_MAX_POSES = HV_TRAIL_MAX_POSES, TI_MAX_VISITS = HV_TRAIL_MAX_VISITS;
constexpr int FAILED_UPDATES_THRESHOLD = 5;                     // backend.cpp:1272
constexpr int GATE_INLIER = 0;                                  // VuOutlierStatus::INLIER
static_assert(TI_MAX_POSES <= 64 && TI_MAX_VISITS <= 64, "one wavefront over the poses of a track / the candidates of a set");

struct TrailArgs {
    hv_trail_index t;
    int M, K, ncam, V, n_sets;
    int hanoi, strided_len, strided_stride, fixed_scheme, sampling, min_frames, score_tracks, blacklist, max_success, est_shift;
    // select
    const int32_t *n_tracks, *ids;
    const float *xy, *second_xy;
    const int32_t *keyframe;
    const uint8_t *full;
    const int32_t *frame_num;
    const double *time;
    const uint32_t *draws;
    int32_t *draws_used, *n_poses, *pose_index;
    double *features, *velocities, *y;
    int32_t *cand_id, *n_cand;
    // finish
    const int32_t *status, *gate;
    const uint8_t *stationary;
    int32_t *delete_ids, *n_delete;
    uint8_t *good_frame;
    int32_t *n_attempts, *n_success, *discarded;
};

struct TrailCameras { hv_camera_model cam0, cam1; };

#include "hv_workgroup.hpp"   // clampi, block_compact, stage_cameras
#include "trail_phases.hpp"   // trail_track_score, trail_order_phase, trail_filter_skips: shared with full_cloud.hip

// index of the [2] record of (row, column, camera) in the observation arrays, and of the `used` byte
__device__ inline size_t obs_at(const TrailArgs &a, int set, int row, int col, int cam)
{
    return trail_obs_at(a.K, a.M, a.ncam, set, row, col, cam);
}
__device__ inline size_t used_at(const TrailArgs &a, int set, int row, int col) { return trail_used_at(a.K, a.M, set, row, col); }

__global__ __launch_bounds__(TI_THREADS) void trail_init_kernel(TrailArgs a)
{
    trail_fresh_set(a.t, blockIdx.x, a.M, a.K);
}

__global__ __launch_bounds__(TI_THREADS) void trail_select_kernel(TrailArgs a, TrailCameras cams)
{
    __shared__ hv_camera_model s_cam[2];
    __shared__ int s_cid[TI_MAX];        // column -> track ID
    __shared__ int s_len[TI_MAX];        // column -> keyframes holding the track (0: free)
    __shared__ int s_hit[TI_MAX];        // column -> the table slot with its ID, -1: none; later the skipped positions
    __shared__ int s_col[TI_MAX];        // table slot -> column
    __shared__ int s_old[TI_MAX];        // table slot -> length before the frame (0: new track); then nValid (-1: not inserted)
    __shared__ float s_score[TI_MAX];    // table slot -> trackScore
    __shared__ int s_list[TI_MAX];       // the new slots; then trackOrder
    __shared__ int s_free[TI_MAX];       // the free columns; then the draws; then the candidates' positions
    __shared__ int s_prev[TI_MAX];       // blacklistedPrev
    __shared__ int s_state[TI_MAX];      // position in the order -> 0 skipped, 1 skipped for the blacklist, 2 candidate
    __shared__ int s_chunk[TI_CHUNKS + 1];
    __shared__ int s_row[TI_MAX_POSES];
    __shared__ int s_min;

    const int set = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = a.M, K = a.K, ncam = a.ncam;
    stage_cameras<TI_THREADS>(s_cam, cams.cam0, cams.cam1);     // published by the barrier behind the s_row fill below
    const int n = clampi(a.n_tracks[set], 0, M);
    const int n_kf_in = clampi(a.t.n_keyframes[set], 1, K);
    const int n_prev = a.blacklist ? clampi(a.t.n_blacklist[set], 0, M) : 0;
    const bool full = a.full ? a.full[set] != 0 : true;
    const bool pop = a.keyframe[set] == 0 && n_kf_in >= 2;      // popHeadKeyframe (:33-39); the reference asserts size >= 2
    const int n_kf = pop ? n_kf_in - 1 : n_kf_in;
    const int32_t *ids = a.ids + (size_t)set * M;
    for (int c = tid; c < M; c += TI_THREADS) {
        s_cid[c] = a.t.col_id[(size_t)set * M + c];
        s_len[c] = clampi(a.t.col_len[(size_t)set * M + c], 0, n_kf_in - 1);
        s_hit[c] = -1;
        if (c < n_prev) s_prev[c] = a.t.blacklist_ids[(size_t)set * M + c];
    }
    int my_row = 0;
    if (tid < K) {                                              // the rows after the pop: the empty head's row leaves the list
        const int32_t *row = a.t.kf_row + (size_t)set * K;
        my_row = !pop ? row[tid] : tid < n_kf_in - 1 ? row[tid + 1] : tid == n_kf_in - 1 ? row[0] : row[tid];
        my_row = clampi(my_row, 0, K - 1);
        s_row[tid] = my_row;
    }
    __syncthreads();
    if (pop && tid < K) a.t.kf_row[(size_t)set * K + tid] = my_row;
    // head.frameNumber / head.timestamp (backend.cpp:798-800); the older timestamps are in other rows
    const double t0 = a.time[set];
    const double t1 = n_kf >= 2 ? a.t.timestamp[(size_t)set * K + s_row[1]] : 0.0;
    const double t2 = n_kf >= 3 ? a.t.timestamp[(size_t)set * K + s_row[2]] : 0.0;
    if (tid == 0) {
        a.t.n_keyframes[set] = n_kf;
        a.t.frame_number[(size_t)set * K + s_row[0]] = a.frame_num[set];
        a.t.timestamp[(size_t)set * K + s_row[0]] = t0;
    }

    // ---- the column of every table track: its own, or a free one ----
    for (int i = tid; i < n; i += TI_THREADS) {
        const int id = ids[i];
        int c = -1;
        for (int q = 0; q < M; ++q) c = (s_len[q] > 0 && s_cid[q] == id) ? q : c;   // IDs are unique: at most one column matches
        s_col[i] = c;
        s_old[i] = c >= 0 ? s_len[c] : 0;
        if (c >= 0) s_hit[c] = i;
    }
    __syncthreads();
    const int n_free = block_compact<TI_WAVES>([&](int c) { return s_hit[c] < 0; }, s_free, M, s_chunk);
    const int n_new = block_compact<TI_WAVES>([&](int i) { return s_col[i] < 0; }, s_list, n, s_chunk);
    for (int k = tid; k < n_new && k < n_free; k += TI_THREADS) s_col[s_list[k]] = s_free[k];   // n_new <= n_free: a slot has one column
    for (int c = tid; c < M; c += TI_THREADS) s_len[c] = 0;     // prune (:220-242): a column that is not inserted below is free
    __syncthreads();

    // ---- insert (backend.cpp:909-951), updateVelocities (:361-384), trackScore (:41-87), nValid of createTrackIndex (:90-147) ----
    const int row0 = s_row[0], row1 = s_row[1 % K], row2 = s_row[2 % K];
    for (int i = tid; i < n; i += TI_THREADS) {
        const int c = s_col[i], id = ids[i];
        const size_t k = (size_t)set * M + i;
        float px[2][2] = {{a.xy[2 * k], a.xy[2 * k + 1]}, {-1.0f, -1.0f}};
        double nrm[2][2] = {{-1.0, -1.0}, {-1.0, -1.0}};
        bool ok = c >= 0 && normalize_pixel(s_cam[0], px[0][0], px[0][1], nrm[0]);
        if (ok && ncam == 2) {
            px[1][0] = a.second_xy[2 * k]; px[1][1] = a.second_xy[2 * k + 1];
            ok = normalize_pixel(s_cam[1], px[1][0], px[1][1], nrm[1]);
        }
        if (!ok) { s_old[i] = -1; continue; }
        const int len = s_old[i] > 0 ? (pop ? s_old[i] : s_old[i] + 1) : 1;
        s_cid[c] = id;
        s_len[c] = len;
        double vel0[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
        if (a.est_shift && n_kf >= 2 && !(t0 <= t1) && len >= 2) {
            for (int cam = 0; cam < ncam; ++cam) {
                const size_t o1 = obs_at(a, set, row1, c, cam);
                const double dt = __dsub_rn(t0, t1);
                const double vx = __ddiv_rn(__dsub_rn(nrm[cam][0], a.t.norm_point[o1]), dt);
                const double vy = __ddiv_rn(__dsub_rn(nrm[cam][1], a.t.norm_point[o1 + 1]), dt);
                vel0[cam][0] = vx; vel0[cam][1] = vy;
                if (n_kf == 2 || len < 3) {
                    a.t.norm_velocity[o1] = vx; a.t.norm_velocity[o1 + 1] = vy;
                } else {
                    if (t0 <= t2) break;                        // :378, a return: the second camera keeps what it had
                    const size_t o2 = obs_at(a, set, row2, c, cam);
                    const double dt2 = __dsub_rn(t0, t2);
                    a.t.norm_velocity[o1] = __ddiv_rn(__dsub_rn(nrm[cam][0], a.t.norm_point[o2]), dt2);
                    a.t.norm_velocity[o1 + 1] = __ddiv_rn(__dsub_rn(nrm[cam][1], a.t.norm_point[o2 + 1]), dt2);
                }
            }
        }
        for (int cam = 0; cam < ncam; ++cam) {
            const size_t o = obs_at(a, set, row0, c, cam);
            a.t.image_point[o] = px[cam][0]; a.t.image_point[o + 1] = px[cam][1];
            a.t.norm_point[o] = nrm[cam][0]; a.t.norm_point[o + 1] = nrm[cam][1];
            a.t.norm_velocity[o] = vel0[cam][0]; a.t.norm_velocity[o + 1] = vel0[cam][1];
        }
        a.t.used[used_at(a, set, row0, c)] = 0;
        int n_valid;                                            // the head's observation is new, hence not used
        const float score = trail_track_score(a.t, K, M, ncam, a.sampling, s_row, set, c, len, px[0][0], px[0][1], n_valid);
        s_score[i] = score;
        s_old[i] = n_valid;
    }
    __syncthreads();
    for (int c = tid; c < M; c += TI_THREADS) {
        a.t.col_len[(size_t)set * M + c] = s_len[c];
        a.t.col_id[(size_t)set * M + c] = s_len[c] > 0 ? s_cid[c] : -1;
    }

    // ---- trackOrder, the draws, minTrackScore (backend.cpp:976-992) ----
    const int n_ord = block_compact<TI_WAVES>([&](int i) { return s_old[i] >= 0; }, s_list, n, s_chunk);
    const float min_score = trail_order_phase<TI_THREADS>(a.score_tracks, a.draws + (size_t)set * M, n_ord, s_score, s_list, s_free, s_state, &s_min);
    if (tid == 0) {
        a.draws_used[set] = max(n_ord - 1, 0);
        a.t.n_order[set] = n_ord;
    }

    // ---- the filter of the visit loop (backend.cpp:1017-1046) ----
    for (int p = tid; p < n_ord; p += TI_THREADS) {
        const int slot = s_list[p];
        int st = 2;
        if (trail_filter_skips(a.score_tracks, s_score[slot], min_score, s_old[slot], a.min_frames, full)) st = 0;
        else {
            const int id = s_cid[s_col[slot]];
            for (int q = 0; q < n_prev; ++q) if (s_prev[q] == id) { st = 1; break; }
        }
        s_state[p] = st;
    }
    __syncthreads();
    const int n_skip = block_compact<TI_WAVES>([&](int p) { return s_state[p] == 1; }, s_hit, n_ord, s_chunk);
    const int n_pass = block_compact<TI_WAVES>([&](int p) { return s_state[p] == 2; }, s_free, n_ord, s_chunk);
    const int n_cand = min(n_pass, a.V);
    for (int k = tid; k < n_skip; k += TI_THREADS) {
        a.t.skipped_pos[(size_t)set * M + k] = s_hit[k];
        a.t.skipped_id[(size_t)set * M + k] = s_cid[s_col[s_list[s_hit[k]]]];
    }
    if (tid == 0) { a.t.n_skipped[set] = n_skip; a.n_cand[set] = n_cand; }

    // ---- buildTrackVectors (:192-218), one wavefront per candidate; the barriers above made this frame's head row visible ----
    for (int v = wave; v < a.V; v += TI_WAVES) {
        const size_t rec = (size_t)v * a.n_sets + set;
        if (v >= n_cand) {
            if (lane == 0) { a.n_poses[rec] = 0; a.cand_id[rec] = -1; }
            continue;
        }
        const int p = s_free[v], c = s_col[s_list[p]], len = s_len[c];
        const int row = s_row[lane < len ? lane : 0];
        const bool use = lane < len && (a.sampling == HV_TRACK_SAMPLING_ALL || lane == len - 1 || a.t.used[used_at(a, set, row, c)] == 0);
        const unsigned long long m = __ballot(use);
        const int nv = __popcll(m), k = __popcll(m & ((1ull << lane) - 1ull));
        if (use) {
            a.pose_index[rec * K + k] = lane;
            for (int cam = 0; cam < ncam; ++cam) {
                const size_t o = obs_at(a, set, row, c, cam), d = (rec * ncam * K + (size_t)cam * nv + k) * 2;
                const double fx = a.t.norm_point[o], fy = a.t.norm_point[o + 1];
                a.features[d] = fx; a.features[d + 1] = fy;
                a.y[d] = fx; a.y[d + 1] = fy;
                a.velocities[d] = a.t.norm_velocity[o]; a.velocities[d + 1] = a.t.norm_velocity[o + 1];
            }
        }
        if (lane == 0) {
            a.n_poses[rec] = nv;
            a.cand_id[rec] = s_cid[c];
            a.t.cand_pos[(size_t)set * a.V + v] = p;
            a.t.cand_col[(size_t)set * a.V + v] = c;
        }
    }
}

__global__ __launch_bounds__(TI_THREADS) void trail_finish_kernel(TrailArgs a)
{
    __shared__ int s_kind[TI_MAX_VISITS];   // candidate -> 0 not counted, 1 success, 2 visited, no inlier
    __shared__ int s_pos[TI_MAX_VISITS], s_col[TI_MAX_VISITS], s_id[TI_MAX_VISITS];
    __shared__ int s_row[TI_MAX_POSES];
    __shared__ int s_wmax[TI_WAVES];
    __shared__ int s_ctl[8];                // attempts, successes, stopped, stop position, fails, removed index, rotate end

    const int set = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = a.M, K = a.K, V = a.V;
    const int n_cand = clampi(a.n_cand[set], 0, V);
    const int n_kf = clampi(a.t.n_keyframes[set], 1, K);
    const int n_ord = clampi(a.t.n_order[set], 0, M);
    const int n_skip = a.blacklist ? clampi(a.t.n_skipped[set], 0, M) : 0;
    if (tid < V) {
        int kind = 0;
        if (tid < n_cand) {
            const size_t rec = (size_t)tid * a.n_sets + set;
            if (a.status[2 * rec] != HV_TRI_NOT_VISITED) kind = a.gate[rec] == GATE_INLIER ? 1 : 2;
            s_pos[tid] = a.t.cand_pos[(size_t)set * V + tid];
            s_col[tid] = clampi(a.t.cand_col[(size_t)set * V + tid], 0, M - 1);
            s_id[tid] = a.cand_id[rec];
        }
        s_kind[tid] = kind;
    }
    if (tid < K) s_row[tid] = clampi(a.t.kf_row[(size_t)set * K + tid], 0, K - 1);
    // the longest column: keyframe i is empty exactly when no column is longer than i
    int longest = 0;
    for (int c = tid; c < M; c += TI_THREADS) longest = max(longest, clampi(a.t.col_len[(size_t)set * M + c], 0, n_kf));
    for (int o = 32; o > 0; o >>= 1) longest = max(longest, __shfl_xor(longest, o));
    if (lane == 0) s_wmax[wave] = longest;
    __syncthreads();
    longest = 0;
    for (int w = 0; w < TI_WAVES; ++w) longest = max(longest, s_wmax[w]);

    // ---- the counters and the stop position of the visit loop (backend.cpp:1121, 1188, 1240-1244), pushHeadKeyframe (:23-31) ----
    if (tid == 0) {
        int attempts = 0, successes = 0, stopped = 0, stop_pos = n_ord, fails = 0;
        for (int v = 0; v < n_cand; ++v) {
            const int kind = s_kind[v];
            if (stopped) { s_kind[v] = 0; continue; }
            if (kind == 0) continue;
            ++attempts;
            if (kind == 1) ++successes;
            else if (a.blacklist) a.delete_ids[(size_t)set * M + fails++] = s_id[v];
            const bool limit_successful = a.max_success > 0 && successes >= a.max_success;
            const bool limit_total = attempts >= V;
            if (limit_successful || limit_total) { stopped = 1; stop_pos = s_pos[v]; }
        }
        a.n_delete[set] = fails;
        if (a.n_attempts) a.n_attempts[set] = attempts;
        if (a.n_success) a.n_success[set] = successes;
        if (a.good_frame) {
            const bool stationary = a.stationary ? a.stationary[set] != 0 : false;
            a.good_frame[set] = ((stationary || stopped) && !(attempts - successes > FAILED_UPDATES_THRESHOLD)) ? 1 : 0;
        }
        // removeKeyframe (:244-281), only with a full trail; otherwise the new head takes the first row of no keyframe
        int removed = K - 1, rotate_end = n_kf;
        if (n_kf > K - 1) {
            int r = -1;
            if (!a.fixed_scheme && longest < n_kf) r = K - 1;   // some keyframe behind the head is empty, hence the last one is
            if (r < 0) {
                const int fc = a.t.frame_counter[set] + 1;
                a.t.frame_counter[set] = fc;
                const int stride = a.strided_len > 0 ? a.strided_stride : 1;
                if (fc % stride != 0) r = K - 1 - a.strided_len - a.hanoi - 1;
                else {
                    const int hc = fc / stride;
                    r = K - 1;
                    for (int i = 0; i < a.hanoi; ++i)
                        if (i < 31 && ((hc >> i) & 1)) { r = K - 1 - a.hanoi + i; break; }
                }
            }
            removed = r;
            rotate_end = clampi(r, 0, K - 1);
        }
        if (a.discarded) a.discarded[set] = removed - 1;
        s_ctl[0] = stop_pos; s_ctl[1] = fails; s_ctl[2] = rotate_end; s_ctl[3] = n_kf > K - 1;
    }
    __syncthreads();
    const int stop_pos = s_ctl[0], n_fail = a.blacklist ? s_ctl[1] : 0, rotate_end = s_ctl[2];
    const bool remove = s_ctl[3] != 0;

    // ---- markTrackUsed (:156-181), GAP: every observation of a successful track ----
    if (a.sampling == HV_TRACK_SAMPLING_GAP) {
        for (int v = wave; v < n_cand; v += TI_WAVES) {
            if (s_kind[v] != 1) continue;
            const int c = s_col[v], len = clampi(a.t.col_len[(size_t)set * M + c], 0, n_kf);
            if (lane < len) a.t.used[used_at(a, set, s_row[lane], c)] = 1;
        }
    }

    // ---- blacklistedPrev.swap(tmp.blacklisted) (:1269): the carried skips (:1039-1046) and the failed visits (:1204-1213), by position ----
    int carried = 0;
    for (int k = 0; k < n_skip; ++k) carried += a.t.skipped_pos[(size_t)set * M + k] < stop_pos;   // a prefix: the positions ascend
    for (int k = tid; k < carried; k += TI_THREADS) {
        const int pos = a.t.skipped_pos[(size_t)set * M + k];
        int before = 0;
        for (int v = 0; v < n_cand; ++v) before += s_kind[v] == 2 && s_pos[v] < pos;
        a.t.blacklist_ids[(size_t)set * M + k + before] = a.t.skipped_id[(size_t)set * M + k];
    }
    if (a.blacklist && tid < n_cand && s_kind[tid] == 2) {
        int before = 0;
        for (int v = 0; v < tid; ++v) before += s_kind[v] == 2;
        for (int k = 0; k < carried; ++k) before += a.t.skipped_pos[(size_t)set * M + k] < s_pos[tid];
        a.t.blacklist_ids[(size_t)set * M + before] = s_id[tid];
    }
    if (tid == 0) a.t.n_blacklist[set] = carried + n_fail;

    // ---- the push as a rotation of kf_row: the removed keyframe's row, or the first row of no keyframe, becomes the head's ----
    __syncthreads();                                            // markTrackUsed has read kf_row's copy
    if (remove) {
        for (int c = tid; c < M; c += TI_THREADS) {
            const int len = clampi(a.t.col_len[(size_t)set * M + c], 0, n_kf);
            if (len > rotate_end) {
                a.t.col_len[(size_t)set * M + c] = len - 1;
                if (len == 1) a.t.col_id[(size_t)set * M + c] = -1;
            }
        }
    }
    if (tid <= rotate_end && tid < K) {
        const int from = tid == 0 ? rotate_end : tid - 1;
        a.t.kf_row[(size_t)set * K + tid] = s_row[from];
    }
    if (tid == 0) {
        const int old_head = s_row[0], new_head = s_row[rotate_end];
        if (new_head != old_head) {
            a.t.frame_number[(size_t)set * K + new_head] = a.t.frame_number[(size_t)set * K + old_head];
            a.t.timestamp[(size_t)set * K + new_head] = a.t.timestamp[(size_t)set * K + old_head];
        }
        a.t.n_keyframes[set] = remove ? n_kf : n_kf + 1;
    }
}

// the host-side checks, made before the context is looked at
int check_params(const hv_trail_index_params *p, int n_sets)
{
    if (!p || n_sets < 0 || p->maxTracks < 1 || p->cameraTrailLength < 1) return HV_ERR_INVALID;
    if (p->cameraTrailHanoiLength < 0 || p->cameraTrailStridedLength < 0) return HV_ERR_INVALID;
    if ((long long)p->cameraTrailHanoiLength + p->cameraTrailStridedLength + 1 >= (long long)p->cameraTrailLength + 1) return HV_ERR_INVALID;
    if (p->cameraTrailStridedLength > 0 && p->cameraTrailStridedStride < 1) return HV_ERR_INVALID;
    if (p->trackSampling < HV_TRACK_SAMPLING_GAP || p->trackSampling > HV_TRACK_SAMPLING_RANDOM) return HV_ERR_INVALID;
    return HV_OK;
}

int check_trail(const hv_trail_index *t)
{
    if (!t) return HV_ERR_INVALID;
    if (!t->n_keyframes || !t->frame_counter || !t->kf_row || !t->frame_number || !t->timestamp || !t->col_id || !t->col_len ||
        !t->image_point || !t->norm_point || !t->norm_velocity || !t->used || !t->n_blacklist || !t->blacklist_ids || !t->n_order ||
        !t->n_skipped || !t->skipped_pos || !t->skipped_id || !t->cand_pos || !t->cand_col)
        return HV_ERR_INVALID;
    return HV_OK;
}

// after every HV_ERR_INVALID check of the entry: a call that is both invalid and unsupported is reported as invalid
int check_limits(const hv_trail_index_params *p, int n_sets, bool full_cloud_entry = false)
{
    if (n_sets > 65535 || p->maxTracks > TI_MAX || p->cameraTrailLength + 1 > TI_MAX_POSES) return HV_ERR_UNSUPPORTED;
    if (p->maxVisualUpdates < 1 || p->maxVisualUpdates > TI_MAX_VISITS) return HV_ERR_UNSUPPORTED;
    if (p->trackSampling == HV_TRACK_SAMPLING_RANDOM || p->hybridMapSize > 0 || p->useIndependentStereoTriangulation) return HV_ERR_UNSUPPORTED;
    // the three entries of this file state the loop that breaks at its stop; the tail behind it is hv_full_point_cloud_dev's
    if (p->fullPointCloud && !full_cloud_entry) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}

void fill_common(TrailArgs &a, const hv_trail_index_params *p, int n_sets, const hv_trail_index *t)
{
    a.t = *t;
    a.M = p->maxTracks; a.K = p->cameraTrailLength + 1; a.ncam = p->useStereo ? 2 : 1; a.V = p->maxVisualUpdates; a.n_sets = n_sets;
    a.hanoi = p->cameraTrailHanoiLength; a.strided_len = p->cameraTrailStridedLength; a.strided_stride = p->cameraTrailStridedStride;
    a.fixed_scheme = p->cameraTrailFixedScheme; a.sampling = p->trackSampling; a.min_frames = p->trackMinFrames;
    a.score_tracks = p->scoreVisualUpdateTracks; a.blacklist = p->blacklistTracks; a.max_success = p->maxSuccessfulVisualUpdates;
    a.est_shift = p->estimateImuCameraTimeShift;
}

}  // namespace

// the HV_ERR_INVALID checks of the parameters and of the state, for flow_predict.hip, output.hip and full_cloud.hip, which read the
// same state (hv_internal.hpp)
int trail_check_params(const hv_trail_index_params *p, int n_sets) { return check_params(p, n_sets); }
int trail_check_state(const hv_trail_index *t) { return check_trail(t); }
// the HV_ERR_UNSUPPORTED limits of the index for full_cloud.hip, which does not read fullPointCloud: calling it is the switch
int trail_check_limits(const hv_trail_index_params *p, int n_sets) { return check_limits(p, n_sets, true); }

}  // namespace hv

using hv::Ctx;

extern "C" {

void hv_trail_index_default_params(hv_trail_index_params *p)
{
    if (!p) return;
    p->cameraTrailLength = 20;                       // codegen/parameter_definitions.c
    p->cameraTrailHanoiLength = 3;
    p->cameraTrailStridedLength = 0;
    p->cameraTrailStridedStride = 2;
    p->cameraTrailFixedScheme = 0;
    p->trackSampling = HV_TRACK_SAMPLING_GAP;
    p->trackMinFrames = 4;
    p->scoreVisualUpdateTracks = 1;
    p->blacklistTracks = 1;
    p->maxVisualUpdates = 20;
    p->maxSuccessfulVisualUpdates = 5;
    p->estimateImuCameraTimeShift = 1;
    p->useStereo = 1;
    p->maxTracks = 200;
    p->hybridMapSize = 0;
    p->useIndependentStereoTriangulation = 0;
    p->fullPointCloud = 0;
}

int hv_trail_init_batch_dev(hv_ctx *h, const hv_trail_index_params *p, int n_sets, const hv_trail_index *trail)
{
    if (const int rc = hv::check_params(p, n_sets)) return rc;
    if (const int rc = hv::check_trail(trail)) return rc;
    if (const int rc = hv::check_limits(p, n_sets)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    hv::TrailArgs a{};
    hv::fill_common(a, p, n_sets, trail);
    hv::ScopedKernelTime tm(c, HV_K_TRAIL_INDEX);
    hipLaunchKernelGGL(hv::trail_init_kernel, dim3((unsigned)n_sets), dim3(hv::TI_THREADS), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_trail_select_batch_dev(hv_ctx *h, const hv_trail_index_params *p, int n_sets, const hv_trail_index *trail,
                              const hv_track_table *table, const hv_camera_model *camera0, const hv_camera_model *camera1,
                              const int32_t *keyframe_dev, const uint8_t *full_update_dev, const int32_t *frame_num_dev,
                              const double *time_dev, const uint32_t *draws_dev, int32_t *draws_used_dev, int32_t *n_poses_dev,
                              int32_t *pose_index_dev, double *features_dev, double *velocities_dev, double *y_dev,
                              int32_t *cand_id_dev, int32_t *n_candidates_dev)
{
    if (const int rc = hv::check_params(p, n_sets)) return rc;
    if (const int rc = hv::check_trail(trail)) return rc;
    if (!table || !table->n_tracks || !table->ids || !table->xy || (p->useStereo && (!table->second_xy || !camera1)) || !camera0)
        return HV_ERR_INVALID;
    if (!keyframe_dev || !frame_num_dev || !time_dev || !draws_dev || !draws_used_dev || !n_poses_dev || !pose_index_dev ||
        !features_dev || !velocities_dev || !y_dev || !cand_id_dev || !n_candidates_dev)
        return HV_ERR_INVALID;
    if (const int rc = hv::check_limits(p, n_sets)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    hv::TrailArgs a{};
    hv::fill_common(a, p, n_sets, trail);
    a.n_tracks = table->n_tracks; a.ids = table->ids; a.xy = table->xy; a.second_xy = table->second_xy;
    a.keyframe = keyframe_dev; a.full = full_update_dev; a.frame_num = frame_num_dev; a.time = time_dev; a.draws = draws_dev;
    a.draws_used = draws_used_dev; a.n_poses = n_poses_dev; a.pose_index = pose_index_dev; a.features = features_dev;
    a.velocities = velocities_dev; a.y = y_dev; a.cand_id = cand_id_dev; a.n_cand = n_candidates_dev;
    hv::TrailCameras cams{};
    cams.cam0 = *camera0;
    cams.cam1 = camera1 ? *camera1 : *camera0;
    hv::ScopedKernelTime tm(c, HV_K_TRAIL_INDEX);
    hipLaunchKernelGGL(hv::trail_select_kernel, dim3((unsigned)n_sets), dim3(hv::TI_THREADS), 0, c->stream, a, cams);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_trail_finish_batch_dev(hv_ctx *h, const hv_trail_index_params *p, int n_sets, const hv_trail_index *trail,
                              const int32_t *cand_id_dev, const int32_t *n_candidates_dev, const int32_t *status_dev,
                              const int32_t *gate_status_dev, const uint8_t *stationary_dev, int32_t *delete_ids_dev,
                              int32_t *n_delete_dev, uint8_t *good_frame_dev, int32_t *n_attempts_dev, int32_t *n_success_dev,
                              int32_t *discarded_dev)
{
    if (const int rc = hv::check_params(p, n_sets)) return rc;
    if (const int rc = hv::check_trail(trail)) return rc;
    if (!cand_id_dev || !n_candidates_dev || !status_dev || !gate_status_dev || !delete_ids_dev || !n_delete_dev || !discarded_dev)
        return HV_ERR_INVALID;
    if (const int rc = hv::check_limits(p, n_sets)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    hv::TrailArgs a{};
    hv::fill_common(a, p, n_sets, trail);
    a.cand_id = const_cast<int32_t *>(cand_id_dev); a.n_cand = const_cast<int32_t *>(n_candidates_dev);
    a.status = status_dev; a.gate = gate_status_dev; a.stationary = stationary_dev; a.delete_ids = delete_ids_dev;
    a.n_delete = n_delete_dev; a.good_frame = good_frame_dev; a.n_attempts = n_attempts_dev; a.n_success = n_success_dev;
    a.discarded = discarded_dev;
    hv::ScopedKernelTime tm(c, HV_K_TRAIL_INDEX);
    hipLaunchKernelGGL(hv::trail_finish_kernel, dim3((unsigned)n_sets), dim3(hv::TI_THREADS), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

}  // extern "C"
