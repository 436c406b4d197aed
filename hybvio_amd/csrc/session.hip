// Device session lifecycle for a batch of resident sequences, one workgroup per set (set s is filter s): the filter's sample clock
// and initializeOrientation on the first IMU sample (ekf.cpp:299-317, 357-366; backend.cpp:728-731), the good-frame ring that decides
// Session::trackingStatus (backend.cpp:195-198, 807-819; CircularBuffer, odometry/util.hpp:111-149), Control's status, freeze flag and
// reset rules (control.cpp:117-149) and the reset itself (control.cpp:49-65, backend.cpp:224-229): a new filter, tracker, trail index
// and control block written in place for the sets that reset. Restatement: tests/session_restatement.py. Oracle of the filter part:
// oracle/ekf_oracle.c:178-225, 285-311, 545-587.
//
// None of this is arithmetic work: the kernels are a few scalar rules per set on one lane, plus -- for a reset -- one streaming write
// of the set's n x n covariance (8 n^2 bytes) and of its table and index slices. What they buy is that a lost or diverged sequence no
// longer costs a read-back, a host rebuild and synchronous hv_ekf_set_state calls that drain the lane.
//
// The reset writes the constructor's P, which is diagonal, and transformTo's A is block diagonal, so the A P A' of a keep-pose reset is
// formed per diagonal block of A (blk_of, ekf_device.hpp): entry (i, j) of a block is sum_k A(i, k) * (d_k * A(j, k)), the grouping of
// the dense products A * (P * A') the oracle forms, whose other terms are exact zeros.
#include <math.h>

#include "ekf_device.hpp"
#include "ekf_host.hpp"
#include "fresh_state.hpp"

// (as the EKF family files: the library's default is -ffp-contract=off, the EKF selects fused multiply-adds; the clocks and the status
// rules below are single additions, subtractions, divisions and comparisons, which contraction does not touch)
#pragma clang fp contract(fast)

namespace hv {
namespace {

constexpr int SES_THREADS = 64;               // init, imu, status: one wavefront per set
constexpr int RESET_THREADS = 256;

struct InitArgs { hv_session st; int W; };
struct ImuArgs {
    hv_session st;
    int n, batch, n_samples;
    double *m, *P;                             // [batch][n], [batch][n][n]
    const double *t, *acc;                     // [n_samples][batch], [n_samples][batch][3]
    const unsigned char *active;               // [batch] or null
    double *dt_out, *time_out;                 // [n_samples][batch]
    double gravity, ori_var;                   // odometry.gravity; noiseInitialOri^2 * noiseScale^2
};
struct StatusArgs {
    hv_session st;
    int W;
    double to_tracking, to_failed, reset_after;
    int reset_until_init, reset_on_failed, freeze;
    const unsigned char *good, *full;          // [batch]; [batch] or null (every frame is full)
    int32_t *status;                           // [batch] or null
    unsigned char *frozen;                     // [batch] or null
    int32_t *reset_kind;                       // [batch]
};
struct ResetArgs {
    hv_session st;
    int W, n;
    double *m, *P, *Q, *dydx;                  // the filter arrays, P the current buffer of the ping-pong
    EkfFresh fresh;
    double gravity;
    hv_ekf_control ctl;
    hv_track_table table;
    int max_tracks, radius0;
    hv_trail_index trail;
    int K;
    const int32_t *kind;                       // [batch]
};

// the Session part of the state as its constructor leaves it: the ring empty, trackingStatus INIT, the filter's clock members
__device__ inline void session_fresh_set(const hv_session &st, int b, int W)
{
    for (int i = threadIdx.x; i < W; i += blockDim.x) st.good_ring[(size_t)b * W + i] = 0.0f;
    if (threadIdx.x == 0) {
        st.ring_head[b] = 0; st.ring_entries[b] = 0;
        st.tracking_status[b] = HV_TRACKING_INIT;
        st.first_sample[b] = 1; st.first_sample_t[b] = -1.0; st.prev_sample_t[b] = -1.0; st.time[b] = 0.0;
    }
}

// Eigen::Quaterniond::FromTwoVectors(-gravity, xa) as oracle/ekf_oracle.c:285-306 restates it, gravity = (0, 0, -g), plus the
// zero-vector rule: normalized() leaves a zero vector zero, which ends in q = (sqrt(2) / 2, 0, 0, 0)
__device__ inline void initial_orientation(double g, const double *xa, double *q)
{
    double a[3] = {-0.0, -0.0, g}, b[3] = {xa[0], xa[1], xa[2]};
    const double na = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), nb = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    for (int i = 0; i < 3; i++) { a[i] /= na; if (nb > 0.0) b[i] /= nb; }
    const double c = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    if (c < -1.0 + 1e-12) {                    // antiparallel: a half-turn about an axis orthogonal to a
        double ax[3] = {1.0, 0.0, 0.0};
        if (fabs(a[0]) > 0.9) { ax[0] = 0.0; ax[1] = 1.0; }
        const double d = ax[0] * a[0] + ax[1] * a[1] + ax[2] * a[2];
        for (int i = 0; i < 3; i++) ax[i] -= d * a[i];
        const double nn = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
        q[0] = 0.0; q[1] = ax[0] / nn; q[2] = ax[1] / nn; q[3] = ax[2] / nn;
    } else {
        const double ax[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const double s = sqrt((1.0 + c) * 2.0), invs = 1.0 / s;
        q[0] = s * 0.5; q[1] = ax[0] * invs; q[2] = ax[1] * invs; q[3] = ax[2] * invs;
    }
}

__global__ __launch_bounds__(SES_THREADS) void session_init_kernel(InitArgs a)
{
    const int b = blockIdx.x;
    session_fresh_set(a.st, b, a.W);
    if (threadIdx.x == 0) {
        a.st.control_status[b] = HV_TRACKING_INIT;
        a.st.last_reset_time[b] = 0.0;
        a.st.initialized_orientation[b] = 0;
    }
}

__global__ __launch_bounds__(SES_THREADS) void session_imu_kernel(ImuArgs a)
{
    const int b = blockIdx.x, t = threadIdx.x, n = a.n, B = a.batch;
    if (a.active && !a.active[b]) {            // masked: dt 0 and the stored clock; no state is written
        const double time = a.st.time[b];
        for (int s = t; s < a.n_samples; s += SES_THREADS) { a.dt_out[(size_t)s * B + b] = 0.0; a.time_out[(size_t)s * B + b] = time; }
        return;
    }
    // backend.cpp:728-731: the first sample the session sees sets the orientation and the ORI block of P, nothing else of the filter
    if (!a.st.initialized_orientation[b]) {
        double q[4];
        initial_orientation(a.gravity, a.acc + (size_t)b * 3, q);
        double *m = a.m + (size_t)b * n, *P = a.P + (size_t)b * n * n;
        if (t < 4) m[ORI + t] = q[t];
        if (t < 16) {
            const int i = t & 3, j = t >> 2;
            P[(size_t)(ORI + j) * n + ORI + i] = (i == j && i < 3) ? a.ori_var : 0.0;      // the last component is fixed (ekf.cpp:307-316)
        }
    }
    __syncthreads();                           // every thread has read the flag lane 0 sets now
    if (t != 0) return;
    a.st.initialized_orientation[b] = 1;
    // ekf.cpp:357-366, sample by sample
    bool first = a.st.first_sample[b] != 0;
    double first_t = a.st.first_sample_t[b], prev_t = a.st.prev_sample_t[b], time = a.st.time[b];
    for (int s = 0; s < a.n_samples; s++) {
        const double ts = a.t[(size_t)s * B + b];
        double dt = 0.0;
        if (!first) { dt = ts - prev_t; time = ts - first_t; }
        else { first_t = ts; first = false; }
        prev_t = ts;
        a.dt_out[(size_t)s * B + b] = dt;
        a.time_out[(size_t)s * B + b] = time;
    }
    a.st.first_sample[b] = 0; a.st.first_sample_t[b] = first_t; a.st.prev_sample_t[b] = prev_t; a.st.time[b] = time;
}

__global__ __launch_bounds__(SES_THREADS) void session_status_kernel(StatusArgs a)
{
    __shared__ float s_ring[HV_SESSION_MAX_WINDOW];
    const int b = blockIdx.x, t = threadIdx.x, W = a.W;
    float *ring = a.st.good_ring + (size_t)b * W;
    for (int i = t; i < W; i += SES_THREADS) s_ring[i] = ring[i];
    __syncthreads();
    if (t != 0) return;
    // backend.cpp:807-819
    int ts = a.st.tracking_status[b];
    if (!a.full || a.full[b]) {
        int head = min(max(a.st.ring_head[b], 0), W - 1), entries = min(max(a.st.ring_entries[b], 0), W);
        const float v = a.good[b] ? 1.0f : 0.0f;
        s_ring[head] = v; ring[head] = v;                                 // CircularBuffer::put
        head = (head + 1) % W;
        if (entries != W) entries++;
        a.st.ring_head[b] = head; a.st.ring_entries[b] = entries;
        if (entries > W / 2) {
            float total = 0.0f;                                           // CircularBuffer::mean: mBuffer[0 .. entries) in order
            for (int i = 0; i < entries; i++) total += s_ring[i];
            const double mean = (double)(total / (float)entries);
            if (ts != HV_TRACKING_TRACKING && mean > a.to_tracking) ts = HV_TRACKING_TRACKING;
            else if (ts == HV_TRACKING_TRACKING && mean < a.to_failed) ts = HV_TRACKING_LOST;
        }
        a.st.tracking_status[b] = ts;
    }
    // control.cpp:121-149
    const double now = a.st.first_sample_t[b] + a.st.time[b];             // getPlatformTime
    int cs = a.st.control_status[b];
    if (a.status) a.status[b] = cs;
    if (a.frozen) a.frozen[b] = a.freeze && cs != HV_TRACKING_INIT && ts != HV_TRACKING_TRACKING;
    if (cs == HV_TRACKING_INIT || ts != HV_TRACKING_INIT) cs = ts;        // never back to INIT
    a.st.control_status[b] = cs;
    const bool expired = a.st.last_reset_time[b] + a.reset_after < now;
    int kind = HV_RESET_NONE;
    if (cs == HV_TRACKING_INIT && expired && a.reset_until_init) kind = HV_RESET_FRESH;
    else if (a.reset_on_failed && ts == HV_TRACKING_LOST) kind = HV_RESET_KEEP_POSE;
    else if (cs != HV_TRACKING_INIT && ts == HV_TRACKING_INIT && expired) kind = HV_RESET_KEEP_POSE;
    a.reset_kind[b] = kind;
}

// One diagonal block of transformTo on the fresh filter: A (SZ x SZ, row-major: pC or qC) applied to the block's mean and to its
// diagonal covariance. Every index is a compile-time constant, so A, x and d stay in registers.
template <int SZ>
__device__ __forceinline__ void keep_pose_block(const EkfFresh &fresh, const double (&A)[SZ * SZ], const double (&q0)[4], const double (&shift)[3],
                                                int s0, double *m, double *P, int n)
{
    const bool ori = s0 == ORI;                                            // initializeOrientation: q0, diag(v, v, v, 0)
    double x[SZ], d[SZ];
#pragma unroll
    for (int k = 0; k < SZ; k++) {
        x[k] = ori ? q0[k] : fresh.mean(s0 + k);
        d[k] = ori ? (k < 3 ? fresh.ori_init : 0.0) : fresh.p_diag(s0 + k);
    }
#pragma unroll
    for (int j = 0; j < SZ; j++)
#pragma unroll
        for (int i = 0; i < SZ; i++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < SZ; k++) s += A[i * SZ + k] * (d[k] * A[j * SZ + k]);
            P[(size_t)(s0 + j) * n + s0 + i] = s;
        }
    const bool is_pos = SZ == 3 && s0 != VEL;
#pragma unroll
    for (int i = 0; i < SZ; i++) {
        double y = 0.0;
#pragma unroll
        for (int k = 0; k < SZ; k++) y += A[i * SZ + k] * x[k];
        m[s0 + i] = is_pos ? y + shift[i < 3 ? i : 0] : y;
    }
}

__global__ __launch_bounds__(RESET_THREADS) void session_reset_kernel(ResetArgs a)
{
    const int b = blockIdx.x, t = threadIdx.x, n = a.n;
    const int kind = a.kind[b];
    if (kind != HV_RESET_FRESH && kind != HV_RESET_KEEP_POSE) return;     // (uniform) not reset: nothing of the set is touched
    double *m = a.m + (size_t)b * n, *P = a.P + (size_t)b * n * n;
    // control.cpp:50-57: the old clock and the old pose, read by every thread before anything is written
    const double now = a.st.first_sample_t[b] + a.st.time[b];
    const double pos[3] = {m[POS], m[POS + 1], m[POS + 2]}, q1[4] = {m[ORI], m[ORI + 1], m[ORI + 2], m[ORI + 3]};
    __syncthreads();

    // ---- Control, Session, tracker, trail index ----
    session_fresh_set(a.st, b, a.W);
    if (t == 0) {
        a.st.last_reset_time[b] = now;
        a.st.initialized_orientation[b] = kind == HV_RESET_KEEP_POSE;      // initializeAtPose sets it (backend.cpp:227)
        ekf_control_fresh(a.ctl, b);
    }
    tracks_fresh_set(a.table, b, a.max_tracks, a.radius0);
    trail_fresh_set(a.trail, b, a.max_tracks, a.K);

    // ---- the filter as EKF::build leaves it ----
    for (int i = t; i < n; i += RESET_THREADS) m[i] = a.fresh.mean(i);
    {
        int i = t % n, j = t / n;                                          // element e = j * n + i, walked without a division per element
        const int si = RESET_THREADS % n, sj = RESET_THREADS / n;
        for (int e = t; e < n * n; e += RESET_THREADS) {
            P[e] = i == j ? a.fresh.p_diag(i) : 0.0;
            i += si; j += sj;
            if (i >= n) { i -= n; j++; }
        }
    }
    for (int i = t; i < QD * QD; i += RESET_THREADS) a.Q[(size_t)b * QD * QD + i] = (i % (QD + 1) == 0) ? a.fresh.q_diag(i / (QD + 1)) : 0.0;
    for (int i = t; i < INER * INER; i += RESET_THREADS) a.dydx[(size_t)b * INER * INER + i] = 0.0;
    if (kind != HV_RESET_KEEP_POSE) return;

    // ---- initializeAtPose (backend.cpp:224-229): initializeOrientation(0), then transformTo(pos, q) on the fresh filter ----
    __syncthreads();                                                       // the blocks below overwrite what other threads wrote above
    const double zero[3] = {0.0, 0.0, 0.0};
    double q0[4];
    initial_orientation(a.gravity, zero, q0);                             // (sqrt(2) / 2, 0, 0, 0): not a unit quaternion, kept (header)
    // qChange = conj(q0) * q1 and its two matrices, as oracle/ekf_oracle.c:549-566
    const double c0[4] = {q0[0], -q0[1], -q0[2], -q0[3]};
    const double p1 = c0[0] * q1[0] - c0[1] * q1[1] - c0[2] * q1[2] - c0[3] * q1[3];
    const double p2 = c0[0] * q1[1] + c0[1] * q1[0] + c0[2] * q1[3] - c0[3] * q1[2];
    const double p3 = c0[0] * q1[2] - c0[1] * q1[3] + c0[2] * q1[0] + c0[3] * q1[1];
    const double p4 = c0[0] * q1[3] + c0[1] * q1[2] - c0[2] * q1[1] + c0[3] * q1[0];
    const double qC[16] = {p1, -p2, -p3, -p4, p2, p1, p4, -p3, p3, -p4, p1, p2, p4, p3, -p2, p1};      // row-major
    double pC[9];                                                          // row-major: toRotationMatrix() transposed
    {
        const double w = p1, x = p2, y = p3, z = p4;
        const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
                     tyy = ty * y, tyz = tz * y, tzz = tz * z;
        pC[0] = 1 - (tyy + tzz); pC[3] = txy - twz; pC[6] = txz + twy;
        pC[1] = txy + twz; pC[4] = 1 - (txx + tzz); pC[7] = tyz - twx;
        pC[2] = txz - twy; pC[5] = tyz + twx; pC[8] = 1 - (txx + tyy);
    }
    // translation = pos - pC * refPos and translateTo(m[POS] + translation) (ekf.cpp:696-702, 750-757), refPos the fresh position
    double shift[3];
    for (int i = 0; i < 3; i++) {
        double s = 0.0, y = 0.0;
        for (int k = 0; k < 3; k++) { s += pC[3 * i + k] * a.fresh.mean(POS + k); y += pC[3 * i + k] * a.fresh.mean(POS + k); }
        const double target = y + (pos[i] - s);
        shift[i] = target - y;
    }
    const int nblk = 13 + 2 * a.fresh.cam_poses + (n - CAM - POSE * a.fresh.cam_poses);
    for (int idx = t; idx < nblk; idx += RESET_THREADS) {
        int s0, sz, bk;
        blk_of(idx, a.fresh.cam_poses, s0, sz, bk);
        if (bk == 1) keep_pose_block<3>(a.fresh, pC, q0, shift, s0, m, P, n);
        else if (bk == 2) keep_pose_block<4>(a.fresh, qC, q0, shift, s0, m, P, n);      // (identity blocks keep the constructor's values)
    }
}

}  // namespace
}  // namespace hv

using hv::Ctx;
using hv::Ekf;

namespace {

bool session_complete(const hv_session *st)
{
    return st && st->good_ring && st->ring_head && st->ring_entries && st->tracking_status && st->control_status && st->last_reset_time &&
           st->first_sample && st->first_sample_t && st->prev_sample_t && st->time && st->initialized_orientation;
}

// the ring size (backend.cpp:195-197); HV_ERR_INVALID / HV_ERR_UNSUPPORTED as the header states
int ring_size(const hv_session_params *p, int *W)
{
    if (!p || p->visualUpdateForEveryNFrame < 1) return HV_ERR_INVALID;
    const double w = (double)p->targetFps / (double)p->visualUpdateForEveryNFrame * p->goodFramesTimeWindowSeconds;
    if (!(w >= 1.0)) return HV_ERR_INVALID;                                // (NaN included)
    if (w >= (double)HV_SESSION_MAX_WINDOW + 1.0) return HV_ERR_UNSUPPORTED;
    *W = (int)(size_t)w;
    return HV_OK;
}

// the checks that need the handle, after every other one
int check_filter(const hv_ekf *h)
{
    if (!h) return HV_ERR_INVALID;
    return (h->e.batch > 65535 || h->e.n > 1024) ? HV_ERR_UNSUPPORTED : HV_OK;
}

}  // namespace

extern "C" {

void hv_session_default_params(hv_session_params *p)
{
    if (!p) return;
    p->targetFps = 30;                               // codegen/parameter_definitions.c:220
    p->visualUpdateForEveryNFrame = 1;               // :4
    p->goodFramesTimeWindowSeconds = 2.0;            // :204
    p->goodFramesToTracking = 0.75;                  // :201
    p->goodFramesToTrackingFailed = 0.05;            // :202
    p->resetUntilInitSucceeds = 0;                   // :193
    p->resetOnFailedTracking = 0;                    // :195
    p->resetAfterTrackingFailsToInitialize = 3.0;    // :197
    p->freezeOnFailedTracking = 0;                   // :199
}

int hv_session_init_dev(hv_ekf *h, const hv_session_params *p, const hv_session *st)
{
    if (!p || !session_complete(st)) return HV_ERR_INVALID;
    int W = 0;
    if (const int rc = ring_size(p, &W)) return rc;
    if (const int rc = check_filter(h)) return rc;
    Ekf *e = &h->e; Ctx *c = e->c;
    hv::InitArgs a{*st, W};
    hv::ScopedKernelTime tm(c, HV_K_EKF_CONTROL);
    hipLaunchKernelGGL(hv::session_init_kernel, dim3((unsigned)e->batch), dim3(hv::SES_THREADS), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_session_imu_dev(hv_ekf *h, const hv_session *st, int n_samples, const double *t_dev, const double *acc_dev,
                       const unsigned char *active_dev, double *dt_dev, double *time_dev)
{
    if (!session_complete(st) || !t_dev || !acc_dev || !dt_dev || !time_dev) return HV_ERR_INVALID;
    if (n_samples < 1 || n_samples > HV_EKF_MAX_PREDICT_SAMPLES) return HV_ERR_INVALID;
    if (const int rc = check_filter(h)) return rc;
    Ekf *e = &h->e; Ctx *c = e->c;
    hv::ImuArgs a{};
    a.st = *st; a.n = e->n; a.batch = e->batch; a.n_samples = n_samples; a.m = e->fixed.m; a.P = e->fixed.P;
    a.t = t_dev; a.acc = acc_dev; a.active = active_dev; a.dt_out = dt_dev; a.time_out = time_dev;
    a.gravity = e->par.gravity; a.ori_var = hv::ekf_fresh(e->par, e->n, e->noise_scale).ori_init;
    hv::ScopedKernelTime tm(c, HV_K_EKF_CONTROL);
    hipLaunchKernelGGL(hv::session_imu_kernel, dim3((unsigned)e->batch), dim3(hv::SES_THREADS), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_session_status_dev(hv_ekf *h, const hv_session_params *p, const hv_session *st, const unsigned char *good_frame_dev,
                          const unsigned char *full_update_dev, int32_t *status_dev, unsigned char *frozen_dev,
                          int32_t *reset_kind_dev)
{
    if (!p || !session_complete(st) || !good_frame_dev || !reset_kind_dev) return HV_ERR_INVALID;
    int W = 0;
    if (const int rc = ring_size(p, &W)) return rc;
    if (const int rc = check_filter(h)) return rc;
    Ekf *e = &h->e; Ctx *c = e->c;
    hv::StatusArgs a{};
    a.st = *st; a.W = W;
    a.to_tracking = p->goodFramesToTracking; a.to_failed = p->goodFramesToTrackingFailed;
    a.reset_after = p->resetAfterTrackingFailsToInitialize;
    a.reset_until_init = p->resetUntilInitSucceeds; a.reset_on_failed = p->resetOnFailedTracking; a.freeze = p->freezeOnFailedTracking;
    a.good = good_frame_dev; a.full = full_update_dev; a.status = status_dev; a.frozen = frozen_dev; a.reset_kind = reset_kind_dev;
    hv::ScopedKernelTime tm(c, HV_K_EKF_CONTROL);
    hipLaunchKernelGGL(hv::session_status_kernel, dim3((unsigned)e->batch), dim3(hv::SES_THREADS), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_session_reset_dev(hv_ekf *h, const hv_session_params *p, const hv_session *st, const hv_ekf_control *ctl,
                         const hv_track_table_params *tracks_p, const hv_track_table *table,
                         const hv_trail_index_params *trail_p, const hv_trail_index *trail, const int32_t *reset_kind_dev)
{
    if (!p || !session_complete(st) || !reset_kind_dev) return HV_ERR_INVALID;
    if (const int rc = hv::ekf_control_check(ctl)) return rc;
    if (const int rc = hv::tracks_check_table(tracks_p, 0, table)) return rc;
    if (const int rc = hv::trail_check_params(trail_p, 0)) return rc;
    if (const int rc = hv::trail_check_state(trail)) return rc;
    if (tracks_p->maxTracks != trail_p->maxTracks) return HV_ERR_INVALID;
    int W = 0;
    if (const int rc = ring_size(p, &W)) return rc;
    if (tracks_p->maxTracks > HV_TRACKS_MAX_TRACKS || trail_p->cameraTrailLength + 1 > HV_TRAIL_MAX_POSES) return HV_ERR_UNSUPPORTED;
    if (const int rc = check_filter(h)) return rc;
    Ekf *e = &h->e; Ctx *c = e->c;
    hv::ResetArgs a{};
    a.st = *st; a.W = W; a.n = e->n;
    a.m = e->fixed.m; a.P = e->fixed.P; a.Q = e->fixed.Q; a.dydx = e->fixed.dydx;      // P: whichever buffer the ping-pong made current
    a.fresh = hv::ekf_fresh(e->par, e->n, e->noise_scale);
    a.gravity = e->par.gravity;
    a.ctl = *ctl; a.table = *table; a.max_tracks = tracks_p->maxTracks; a.radius0 = hv::track_mask_radius(c, tracks_p, 0);
    a.trail = *trail; a.K = trail_p->cameraTrailLength + 1;
    a.kind = reset_kind_dev;
    hv::ScopedKernelTime tm(c, HV_K_EKF_CONTROL);
    hipLaunchKernelGGL(hv::session_reset_kernel, dim3((unsigned)e->batch), dim3(hv::RESET_THREADS), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

}  // extern "C"
