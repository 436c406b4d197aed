// The phases of Session::trackerVisualUpdate in front of the visit loop that more than one kernel states: trail_select_kernel
// (trail_index.hip) makes them once per frame, full_cloud_index_kernel (full_cloud.hip) derives them again from the index select
// left behind. One statement of each rule: trackScore and nValid (ekf_state_index.cpp:41-87, 90-147), the draws, minTrackScore and
// shuffleDeterministic (backend.cpp:976-992, util.hpp:39-44) and the part of the visit loop's filter that does not depend on
// needMoreVisualUpdates (backend.cpp:1017-1038).
//
// No include guard and no namespace of its own, like hv_workgroup.hpp, and included behind it; one-dimensional workgroups.
// Arithmetic that the restatement rounds once is written with the _rn intrinsics.

constexpr int TRAIL_SCORE_BATCH = 4;                            // older observations loaded together in trackScore

// index of the [2] record of (row, column, camera) in the observation arrays, and of the `used` byte
__device__ inline size_t trail_obs_at(int K, int M, int ncam, int set, int row, int col, int cam)
{
    return ((((size_t)set * K + row) * M + col) * ncam + cam) * 2;
}
__device__ inline size_t trail_used_at(int K, int M, int set, int row, int col) { return ((size_t)set * K + row) * M + col; }

// trackScore (:41-87) and the nValid of createTrackIndex (:90-147) of the track in column c, which keyframes 0 .. len - 1 hold;
// (head_x, head_y) = the first camera's corner in the head, whose observation is new and hence not used. s_row: keyframe -> row
__device__ inline float trail_track_score(const hv_trail_index &t, int K, int M, int ncam, int sampling, const int *s_row, int set, int c,
                                          int len, float head_x, float head_y, int &n_valid_out)
{
    float score = 0.0f, prev_x = head_x, prev_y = head_y;
    int n_valid = 1;
    for (int j0 = 1; j0 < len; j0 += TRAIL_SCORE_BATCH) {       // the loads of a batch first: only the sum is a dependent chain
        float2 pt[TRAIL_SCORE_BATCH];
        uint8_t us[TRAIL_SCORE_BATCH];
#pragma unroll
        for (int q = 0; q < TRAIL_SCORE_BATCH; ++q) {
            const int row = s_row[min(j0 + q, len - 1)];
            pt[q] = *reinterpret_cast<const float2 *>(t.image_point + trail_obs_at(K, M, ncam, set, row, c, 0));
            us[q] = t.used[trail_used_at(K, M, set, row, c)];
        }
#pragma unroll
        for (int q = 0; q < TRAIL_SCORE_BATCH; ++q) {
            const int j = j0 + q;
            if (j < len) {
                const bool use = sampling == HV_TRACK_SAMPLING_ALL || us[q] == 0 || j == len - 1;
                if (use) {
                    ++n_valid;
                    const double d = __dadd_rn(fabs(__dsub_rn((double)pt[q].x, (double)prev_x)), fabs(__dsub_rn((double)pt[q].y, (double)prev_y)));
                    score = __double2float_rn(__dadd_rn((double)score, d));
                }
                prev_x = pt[q].x; prev_y = pt[q].y;
            }
        }
    }
    n_valid_out = n_valid;
    return score;
}

// trackOrder, the draws, minTrackScore (backend.cpp:976-992) and shuffleDeterministic (util.hpp:39-44). s_list: the n_ord table
// slots of the order, ascending, on entry; shuffled on return. s_score: slot -> trackScore. s_draw, s_trunc: n_ord ints of scratch
// each; s_min: one int. draws: the set's raw std::mt19937 outputs. Every thread of the workgroup calls it; what it reads must be
// visible already; ends with a barrier. Returns minTrackScore (0 without scoreVisualUpdateTracks).
template <int THREADS>
__device__ inline float trail_order_phase(int score_tracks, const uint32_t *draws, int n_ord, const float *s_score, int *s_list, int *s_draw,
                                          int *s_trunc, int *s_min)
{
    const int tid = threadIdx.x;
    // step k of the shuffle is i = n - 1 - k, so every draw % (i + 1) is known before the chain starts
    for (int k = tid; k < n_ord - 1; k += THREADS) s_draw[k] = (int)(draws[k] % (unsigned)(n_ord - k));
    for (int p = tid; p < n_ord; p += THREADS) s_trunc[p] = (int)s_score[s_list[p]];   // static_cast<int> (backend.cpp:988)
    if (tid == 0) *s_min = -1;
    __syncthreads();
    if (score_tracks) {                                         // the element size / 2 of the sorted scores, as a rank count
        const int mid = n_ord / 2;
        for (int p = tid; p < n_ord; p += THREADS) {
            const int v = s_trunc[p];
            int less = 0, le = 0;
            for (int q = 0; q < n_ord; ++q) {
                const int w = s_trunc[q];
                less += w < v; le += w <= v;
            }
            if (less <= mid && mid < le) *s_min = v;            // every thread that gets here holds the same value
        }
    }
    __syncthreads();
    if (tid == 0) {                                             // the one sequential chain
        int k = 0;
        for (int i = n_ord - 1; i > 0; --i) {
            const int j = s_draw[k++];
            const int tmp = s_list[i]; s_list[i] = s_list[j]; s_list[j] = tmp;
        }
    }
    __syncthreads();
    return score_tracks ? (float)*s_min : 0.0f;
}

// the tests of the visit loop's filter that every track meets, stopped loop or not (backend.cpp:1017-1038): true = skipped
__device__ inline bool trail_filter_skips(int score_tracks, float score, float min_score, int n_valid, int min_frames, bool full)
{
    if (score_tracks && score < min_score) return true;
    if (n_valid < min_frames) return true;
    return !full;
}
