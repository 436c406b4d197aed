// EKF control updates for a batch of resident filters, one workgroup per filter: the updates of odometry::EKF whose measurement
// matrix is a block of unit rows (updateZupt, updateZuptInitialization, updateZrupt, updatePosition, updateZeroHeight,
// updateOrientation: ekf.cpp:573-625, 651-677), the scalar pseudo-velocity update (ekf.cpp:628-649), and the two control steps of
// Session::process that decide them per IMU sample and per frame (backend.cpp:738-749, 774-796) from flags and clocks that live in
// caller-owned device memory (hv_ekf_control). Oracle: oracle/ekf_oracle.c:457-523.
//
// update() + updateCommon() (ekf.cpp:25-32, 57-82) for H = W E, E = kc consecutive unit rows starting at col0, W the identity or the
// 1 x 2 unit vector of the pseudo-velocity update, with the reference's operands (P is only symmetrised at
// maintainPositiveSemiDefinite, so rows and columns of P are not interchangeable):
//     HP = W P[col0 : col0 + kc, :]          rows of P: kc adjacent doubles per column of the column-major matrix
//     S  = HP[:, col0 : col0 + kc] W' + r I  k x k, factored from its lower triangle (Eigen's LDLT reads the same triangle)
//     K' = S^-1 HP,  m += K v,  P -= K HP    one read and one write of P: 2 * 8 n^2 + 8 k n bytes per active filter
// None of hv_ekf_update's work exists here: no H to copy or multiply, no tall matrix, no blocked Cholesky.
#include <math.h>

#include "ekf_device.hpp"
#include "ekf_host.hpp"
#include "fresh_state.hpp"

// (as ekf_update.hip: the EKF is judged against a relative tolerance; the library's default is -ffp-contract=off)
#pragma clang fp contract(fast)

namespace hv {
namespace {

constexpr int CTL_THREADS = 512;
enum { CTL_BLOCK = 0, CTL_PSEUDO_VELOCITY = 1, CTL_IMU = 2, CTL_FRAME = 3 };

struct ControlArgs {
    int kind, n, map_dim;
    double *m, *P;                                   // [batch][n], [batch][n][n]
    const unsigned char *active;                     // [batch] or null
    unsigned char *applied;                          // [batch] or null
    // CTL_BLOCK
    int col0, rows, normalize_all;
    const double *y, *r_dev;                         // [batch][rows] or null (zeros); [batch] or null (r0)
    double r0;
    // pseudo-velocity (CTL_PSEUDO_VELOCITY, CTL_IMU): r already scaled by noiseScale
    double pv_limit, pv_target, pv_r;
    // control steps
    hv_ekf_control ctl;
    const double *time;                              // [batch] the filter clock
    int use_init_zupt, use_pseudo_velocity, use_visual_stationarity, frame_count_threshold;
    double init_zupt_r, visual_zupt_r;               // initZuptR * noiseScale, visualZuptR * noiseScale
    const int32_t *keyframe;                         // [batch]
    const unsigned char *full_update;                // [batch] or null (every frame is full)
    int32_t *keyframe_out;
    unsigned char *undo_active, *stationary;
};

__device__ __forceinline__ void quat_normalize(double *q)
{
    const double nn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (nn > 0.0) { q[0] /= nn; q[1] /= nn; q[2] /= nn; q[3] /= nn; }
}

// EKF::horizontalSpeed (ekf.cpp:568-570). Compared against thresholds, so it is formed as the reference's compiler forms it:
// two rounded products and a rounded sum.
__device__ __forceinline__ double horizontal_speed(const double *m)
{
#pragma clang fp contract(off)
    const double x = m[VEL], y = m[VEL + 1];
    const double xx = x * x, yy = y * y;
    return sqrt(xx + yy);
}

// One update of one filter by the whole workgroup. H = W E: `pv` false: W = I (rows = kc), true: W = (w0, w1), kc = 2, one row.
// v = y - H m, formed by the caller from the mean BEFORE the call (the first barrier inside separates those reads from the writes
// of m). HP, Kt: LDS, 4 n doubles each, row-major k x n. Returns whether the update was applied -- the same value in every thread:
// a pivot of S that is not positive leaves m and P untouched (the library's rule for S). Ends synchronised, every store of m and P
// completed, so a second update of the same launch reads what this one wrote.
template <int NT>
__device__ __forceinline__ bool unit_block_update(double *m, double *P, int odd_base, int n, int map_dim, int col0, int kc, bool pv,
                                                  double w0, double w1, const double (&v)[4], double r, int normalize_all,
                                                  double *HP, double *Kt)
{
    const int t = threadIdx.x;
    const int rows = pv ? 1 : kc;
    // ---- stage HP: column j of P holds the kc row entries next to each other; one thread per column ----
    for (int j = t; j < n; j += NT) {
        const double *col = P + (size_t)j * n + col0;
        if (pv) HP[j] = w0 * col[0] + w1 * col[1];
        else for (int a = 0; a < kc; a++) HP[a * n + j] = col[a];
    }
    // the last read of those rows from global memory is above, the first write to P below: the rows lie in columns that other
    // threads write
    __syncthreads();
    // ---- S (lower triangle) padded to 4 x 4 with the identity, and its Cholesky factor, in the registers of every thread ----
    double L[4][4];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        double d = 1.0;
        if (c < rows) d = (pv ? w0 * HP[col0] + w1 * HP[col0 + 1] : HP[c * n + col0 + c]) + r;
#pragma unroll
        for (int k = 0; k < c; k++) d -= L[c][k] * L[c][k];
        if (c < rows) ok = ok && d > 0.0;
        const double ld = sqrt(d);
        L[c][c] = ld;
#pragma unroll
        for (int i = c + 1; i < 4; i++) {
            double s = i < rows ? HP[i * n + col0 + c] : 0.0;      // (pv has one row: never read)
#pragma unroll
            for (int k = 0; k < c; k++) s -= L[i][k] * L[c][k];
            L[i][c] = s / ld;
        }
    }
    if (!ok) return false;                                          // (uniform: every thread factored the same S)
    // ---- K' = S^-1 HP and m += K v, one thread per column of K' ----
    for (int j = t; j < n; j += NT) {
        double x[4];
#pragma unroll
        for (int a = 0; a < 4; a++) x[a] = a < rows ? HP[a * n + j] : 0.0;
#pragma unroll
        for (int a = 0; a < 4; a++) {
            double s = x[a];
#pragma unroll
            for (int k = 0; k < a; k++) s -= L[a][k] * x[k];
            x[a] = s / L[a][a];
        }
#pragma unroll
        for (int a = 3; a >= 0; a--) {
            double s = x[a];
#pragma unroll
            for (int k = a + 1; k < 4; k++) s -= L[k][a] * x[k];
            x[a] = s / L[a][a];
        }
        double dm = 0.0;
#pragma unroll
        for (int a = 0; a < 4; a++)
            if (a < rows) { Kt[a * n + j] = x[a]; dm += x[a] * v[a]; }
        m[j] += dm;
    }
    __syncthreads();
    // ---- P -= K HP in one streaming pass: P[i, j] -= sum_a K[i, a] HP[a, j] ----
    // The filter's n * n doubles are walked as one array. Pairs start where the ADDRESS is a multiple of 16 bytes: the covariances
    // are packed, so for odd n every other filter starts on an odd double (odd_base) and a pair can straddle two columns; what is
    // left in front and behind is a scalar element each.
    auto delta = [&](int i, int j) -> double {
        double s = 0.0;
        for (int a = 0; a < rows; a++) s += Kt[a * n + i] * HP[a * n + j];
        return s;
    };
    const int nn = n * n, npairs = (nn - odd_base) >> 1, tail = odd_base + 2 * npairs;
    if (odd_base && t == 0) P[0] -= delta(0, 0);
    if (tail < nn && t == NT - 1) P[tail] -= delta(n - 1, n - 1);
    {
        constexpr int U = 4;                                        // loads in flight per thread
        const int step = 2 * NT, si = step % n, sj = step / n;      // what one stride adds to (row, column)
        int e = odd_base + 2 * t, i = e % n, j = e / n;
        for (int p0 = t; p0 < npairs; p0 += U * NT) {
            double2 x[U];
            int eu[U], iu[U], ju[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                eu[u] = e; iu[u] = i; ju[u] = j;
                if (p0 + u * NT < npairs) x[u] = *reinterpret_cast<const double2 *>(P + e);
                e += step; i += si; j += sj;
                if (i >= n) { i -= n; j++; }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (p0 + u * NT < npairs) {
                    const bool wrap = iu[u] + 1 == n;               // the pair's second element opens the next column
                    x[u].x -= delta(iu[u], ju[u]);
                    x[u].y -= delta(wrap ? 0 : iu[u] + 1, wrap ? ju[u] + 1 : ju[u]);
                    *reinterpret_cast<double2 *>(P + eu[u]) = x[u];
                }
            }
        }
    }
    __syncthreads();
    // ---- updateCommon: the current orientation; normalizeQuaternions() of updateOrientation: the trail's as well ----
    const int nq = normalize_all ? 1 + (n - map_dim - CAM) / POSE : 1;
    if (t < nq) quat_normalize(m + (t == 0 ? ORI : CAM + POSE * (t - 1) + 3));
    __syncthreads();
    return true;
}

// every filter's control block as fresh_state.hpp defines it
__global__ void ekf_control_init_kernel(int batch, hv_ekf_control ctl)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    ekf_control_fresh(ctl, b);
}

template <int NT>
__global__ __launch_bounds__(NT) void ekf_block_update_kernel(ControlArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double ctl_lds[];
    const int b = blockIdx.x, t = threadIdx.x, n = a.n;
    double *m = a.m + (size_t)b * n, *P = a.P + (size_t)b * n * n;
    const int odd_base = (int)(((size_t)b * n * n) & 1);
    double *HP = ctl_lds, *Kt = ctl_lds + 4 * n;
    const bool on = !a.active || a.active[b];

    // updatePseudoVelocity from the mean as it stands (for CTL_IMU: after the first update); false: skipped by a gate
    auto pseudo_velocity = [&]() -> bool {
        const double h = horizontal_speed(m);
        if (h <= 1e-7 || (a.pv_limit >= 0.0 && h <= a.pv_limit)) return false;
        const double v[4] = {a.pv_target - h, 0.0, 0.0, 0.0};
        return unit_block_update<NT>(m, P, odd_base, n, a.map_dim, VEL, 2, true, m[VEL] / h, m[VEL + 1] / h, v, a.pv_r, 0, HP, Kt);
    };
    // a zero-velocity update with R = r I
    auto zupt = [&](double r) -> bool {
        const double v[4] = {-m[VEL], -m[VEL + 1], -m[VEL + 2], 0.0};
        return unit_block_update<NT>(m, P, odd_base, n, a.map_dim, VEL, 3, false, 1.0, 0.0, v, r, 0, HP, Kt);
    };

    if (a.kind == CTL_BLOCK) {
        bool ok = false;
        if (on) {
            double v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = i < a.rows ? (a.y ? a.y[(size_t)b * a.rows + i] : 0.0) - m[a.col0 + i] : 0.0;
            ok = unit_block_update<NT>(m, P, odd_base, n, a.map_dim, a.col0, a.rows, false, 1.0, 0.0, v, a.r_dev ? a.r_dev[b] : a.r0,
                                       a.normalize_all, HP, Kt);
        }
        if (a.applied && t == 0) a.applied[b] = ok;
    } else if (a.kind == CTL_PSEUDO_VELOCITY) {
        const bool ok = on && pseudo_velocity();
        if (a.applied && t == 0) a.applied[b] = ok;
    } else if (a.kind == CTL_IMU) {
        // backend.cpp:738-749. Every thread reads the flags; thread 0 writes the clock behind the update's barriers.
        if (!on) return;
        const double time = a.time[b];
        const bool init = a.use_init_zupt && !(a.ctl.was_stationary[b] != 0 || time > 60.0 || time - a.ctl.init_zupt_time[b] < 0.1);
        if (init) {
            zupt(a.init_zupt_r * exp(0.5 * time));
            if (t == 0) a.ctl.init_zupt_time[b] = time;
        }
        if (a.use_pseudo_velocity) pseudo_velocity();              // (horizontalSpeed > pseudoVelocityLimit: the gate inside)
    } else {
        // backend.cpp:774-796
        const bool keyframe = a.keyframe[b] != 0;
        const int since = keyframe ? 0 : a.ctl.frames_since_keyframe[b] + 1;
        const bool stationary = since >= a.frame_count_threshold;
        const double time = a.time[b];
        const bool fire = a.use_visual_stationarity && stationary && !(time - a.ctl.zupt_time[b] < 0.25);
        const bool keyframe_out = keyframe && (!a.full_update || a.full_update[b]);
        __syncthreads();                                            // every thread has read the state thread 0 writes now
        if (t == 0) {
            a.ctl.frames_since_keyframe[b] = since;
            if (fire) { a.ctl.zupt_time[b] = time; a.ctl.was_stationary[b] = 1; }
            if (a.keyframe_out) a.keyframe_out[b] = keyframe_out;
            if (a.undo_active) a.undo_active[b] = !keyframe_out;
            if (a.stationary) a.stationary[b] = stationary;
        }
        const bool ok = fire && zupt(a.visual_zupt_r);
        if (a.applied && t == 0) a.applied[b] = ok;
    }
}

}  // namespace
}  // namespace hv

using hv::Ctx;
using hv::Ekf;

namespace {

// the launch all entries share; no allocation, no synchronisation
int launch_control(Ekf *e, hv::ControlArgs &a)
{
    Ctx *c = e->c;
    a.n = e->n; a.map_dim = e->map_dim; a.m = e->fixed.m; a.P = e->fixed.P;
    const size_t shmem = sizeof(double) * 8 * (size_t)e->n;        // HP | K', 4 x n each
    if (shmem > hv::LDS_DEFAULT_LIMIT) return HV_ERR_UNSUPPORTED;
    hv::ScopedKernelTime tm(c, HV_K_EKF_CONTROL);
    hipLaunchKernelGGL(hv::ekf_block_update_kernel<hv::CTL_THREADS>, dim3((unsigned)e->batch), dim3(hv::CTL_THREADS), shmem, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

bool control_complete(const hv_ekf_control *ctl)
{
    return ctl && ctl->zupt_time && ctl->init_zupt_time && ctl->was_stationary && ctl->frames_since_keyframe;
}

void fill_control(hv::ControlArgs &a, const Ekf *e, const hv_ekf_control_params *p, const hv_ekf_control *ctl, const double *time_dev)
{
    a.ctl = *ctl; a.time = time_dev;
    a.use_init_zupt = p->useDecayingZeroVelocityUpdate; a.use_pseudo_velocity = p->usePseudoVelocity;
    a.use_visual_stationarity = p->useVisualStationarity; a.frame_count_threshold = p->visualStationarityFrameCountThreshold;
    a.pv_limit = p->pseudoVelocityLimit; a.pv_target = p->pseudoVelocityTarget; a.pv_r = p->pseudoVelocityR * e->noise_scale;
    a.init_zupt_r = e->par.initZuptR * e->noise_scale; a.visual_zupt_r = p->visualZuptR * e->noise_scale;
}

}  // namespace

// the HV_ERR_INVALID check of the control block, for session.hip (hv_internal.hpp)
int hv::ekf_control_check(const hv_ekf_control *ctl) { return control_complete(ctl) ? HV_OK : HV_ERR_INVALID; }

void hv_ekf_control_default_params(hv_ekf_control_params *p)
{
    if (!p) return;
    p->useDecayingZeroVelocityUpdate = 0;            // codegen/parameter_definitions.c:87
    p->usePseudoVelocity = 0;                        // :95
    p->pseudoVelocityLimit = 1.4;                    // :97
    p->pseudoVelocityTarget = 0.0;                   // :99
    p->pseudoVelocityR = 1e-4;                       // :101
    p->useVisualStationarity = 1;                    // :109
    p->visualStationarityFrameCountThreshold = 3;    // :116
    p->visualZuptR = 1e-7;                           // :119
}

int hv_ekf_block_update_dev(hv_ekf *h, int col0, int rows, const double *y_dev, const double *r_dev, double r0,
                            const unsigned char *active_dev, int normalize_all, unsigned char *applied_dev)
{
    if (!h) return HV_ERR_INVALID;
    Ekf *e = &h->e;
    if (rows < 1 || rows > 4 || col0 < 0 || col0 + rows > e->n) return HV_ERR_INVALID;
    hv::ControlArgs a{};
    a.kind = hv::CTL_BLOCK; a.col0 = col0; a.rows = rows; a.normalize_all = normalize_all;
    a.y = y_dev; a.r_dev = r_dev; a.r0 = r0; a.active = active_dev; a.applied = applied_dev;
    return launch_control(e, a);
}

int hv_ekf_pseudo_velocity_dev(hv_ekf *h, double limit, double target, double r, const unsigned char *active_dev,
                               unsigned char *applied_dev)
{
    if (!h) return HV_ERR_INVALID;
    Ekf *e = &h->e;
    hv::ControlArgs a{};
    a.kind = hv::CTL_PSEUDO_VELOCITY; a.pv_limit = limit; a.pv_target = target; a.pv_r = r * e->noise_scale;
    a.active = active_dev; a.applied = applied_dev;
    return launch_control(e, a);
}

int hv_ekf_control_init_dev(hv_ekf *h, const hv_ekf_control *ctl)
{
    if (!h || !control_complete(ctl)) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    hipLaunchKernelGGL(hv::ekf_control_init_kernel, dim3((unsigned)((e->batch + 255) / 256)), dim3(256), 0, c->stream, e->batch, *ctl);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_ekf_imu_control_dev(hv_ekf *h, const hv_ekf_control_params *p, const hv_ekf_control *ctl, const double *time_dev,
                           const unsigned char *active_dev)
{
    if (!h || !p || !control_complete(ctl) || !time_dev) return HV_ERR_INVALID;
    Ekf *e = &h->e;
    if (!p->useDecayingZeroVelocityUpdate && !p->usePseudoVelocity) return HV_OK;      // (nothing any filter could do)
    hv::ControlArgs a{};
    a.kind = hv::CTL_IMU; a.active = active_dev;
    fill_control(a, e, p, ctl, time_dev);
    return launch_control(e, a);
}

int hv_ekf_frame_control_dev(hv_ekf *h, const hv_ekf_control_params *p, const hv_ekf_control *ctl, const double *time_dev,
                             const int32_t *keyframe_dev, const unsigned char *full_update_dev, int32_t *keyframe_out_dev,
                             unsigned char *undo_active_dev, unsigned char *stationary_dev, unsigned char *applied_dev)
{
    if (!h || !p || !control_complete(ctl) || !time_dev || !keyframe_dev) return HV_ERR_INVALID;
    Ekf *e = &h->e;
    hv::ControlArgs a{};
    a.kind = hv::CTL_FRAME; a.applied = applied_dev;
    fill_control(a, e, p, ctl, time_dev);
    a.keyframe = keyframe_dev; a.full_update = full_update_dev; a.keyframe_out = keyframe_out_dev;
    a.undo_active = undo_active_dev; a.stationary = stationary_dev;
    return launch_control(e, a);
}
