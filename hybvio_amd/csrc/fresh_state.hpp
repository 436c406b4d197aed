// What a freshly constructed tracker, pose-trail index and control block hold, written for ONE set by the whole workgroup: shared by
// the init kernels (track_table.hip, trail_index.hip, ekf_control.hip), which write every set, and the session reset (session.hip),
// which writes the sets that reset. Thread loops run over blockDim.x, so any workgroup size serves. (The filter's constructor values
// are EkfFresh in ekf_device.hpp: they need the state layout.)
#pragma once
#include <algorithm>
#include <cmath>

#include "hv_internal.hpp"

namespace hv {

// maskRadius() (tracker.cpp:569-576) at maskScale = steps / 2; w, h = the context's level-0 size
inline int track_mask_radius(const Ctx *c, const hv_track_table_params *p, int steps)
{
    const int min_dim = std::min(c->L.w[0], c->L.h[0]);
    const double scale = std::pow(1.3, steps / 2.0);
    const int r = (int)std::round(scale * min_dim * p->relativeMaskRadius);
    return r < 2 ? 2 : r;
}

// a fresh TrackerImplementation (tracker.cpp:165-174); radius0 = the mask radius of step 0
__device__ inline void tracks_fresh_set(const hv_track_table &t, int set, int max_tracks, int radius0)
{
    for (int i = threadIdx.x; i < max_tracks; i += blockDim.x) {
        const size_t k = (size_t)set * max_tracks + i;
        t.kf_valid[k] = 0;
        t.blacklist[k] = 0;
    }
    if (threadIdx.x == 0) {
        t.n_tracks[set] = 0;
        t.frame_num[set] = 0;
        t.mask_steps[set] = 0;
        t.mask_radius[set] = radius0;
        t.frame_flags[set] = 0;
    }
}

// a fresh EKFStateIndex (ekf_state_index.hpp:100-107); M = maxTracks, K = maxSize
__device__ inline void trail_fresh_set(const hv_trail_index &t, int set, int M, int K)
{
    for (int c = threadIdx.x; c < M; c += blockDim.x) {
        t.col_id[(size_t)set * M + c] = -1;
        t.col_len[(size_t)set * M + c] = 0;
    }
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        t.kf_row[(size_t)set * K + k] = k;
        t.frame_number[(size_t)set * K + k] = 0;
        t.timestamp[(size_t)set * K + k] = 0.0;
    }
    if (threadIdx.x == 0) {
        t.n_keyframes[set] = 1;                                 // pushHeadKeyframe(0, 0) of the constructor
        t.frame_counter[set] = 0;
        t.n_blacklist[set] = 0;
        t.n_order[set] = 0;
        t.n_skipped[set] = 0;
    }
}

// the values of a fresh odometry::EKF (ekf.hpp: ZUPTtime = initZUPTtime = -1, wasStationary false) and of Session (framesSinceKeyframe 0);
// one thread
__device__ inline void ekf_control_fresh(const hv_ekf_control &ctl, int b)
{
    ctl.zupt_time[b] = -1.0; ctl.init_zupt_time[b] = -1.0;
    ctl.was_stationary[b] = 0; ctl.frames_since_keyframe[b] = 0;
}

}  // namespace hv
