// EKF covariance algebra for a batch of independent filters, one workgroup per filter.
//
// Replaces the dense parts of odometry::EKF (reference: src/odometry/ekf.cpp; oracle:
// oracle/ekf_oracle.c). State m (n) and covariance P (n x n, f64, column-major as Eigen) live in
// HBM; the mean-side scalar bookkeeping (sample times, augment counters, rate limits) stays in the
// host adapter. Design for CDNA4 (numbers: scripts/f64_ubench.hip, scripts/ekf_microbench.py):
//   * f64 vector and f64 matrix peak are the same 128 flop/clk/CU on gfx950; the matrix cores are
//     used because one v_mfma_f64_16x16x4_f64 retires 1024 MACs for two operand loads (one f64 per
//     lane each) where a v_fma_f64 needs two operands per MAC, and because a lone wavefront issues a
//     dependent v_fma_f64 only every ~7 cycles.
// The kernels live with their launchers, one family per file; the families call nothing of each other's:
//   ekf_predict.hip   predict kernels, hv_ekf_predict*
//   ekf_update.hip    visual update / chi2 gate kernels (ekf_update_kernel and its spec-long and dual forms), ekf_launch_update*
//   ekf_gate.hip      streaming dense gate and column-sparse gates, ekf_launch_gate_stream, ekf_launch_sparse_gate
//   ekf_augment.hip   pose augmentation, undo, symmetrise, normalise, transform, map points and their hv_ekf_* entries
//   ekf.hip           (this file) what launches no kernel of its own: parameters, create / destroy, state accessors, the
//                     host-pointer update entries (through ekf_launch_update), the families' LDS limits, the phase-stamp entry
// ekf_visit.hip (track visits, frame loops), ekf_control.hip (ZUPT, pseudo-velocity, block updates) and session.hip (sample clock,
// tracking status, resets in place) sit on top of these.
#include <new>

#include "ekf_device.hpp"
#include "ekf_host.hpp"

// (as the family files: the library's default is -ffp-contract=off, the EKF selects fused multiply-adds; see ekf_update.hip)
#pragma clang fp contract(fast)

namespace hv {

// the kernels' dynamic-LDS limits, set once per context (hv_create; never inside a launch that may be under capture)
int ekf_kernels_init(Ctx *c)
{
    if (const int rc = ekf_update_init(c)) return rc;
    if (const int rc = ekf_gate_init(c)) return rc;
    return ekf_augment_init(c);
}

}  // namespace hv

using hv::Ctx;
using hv::Ekf;

extern "C" {

void hv_ekf_default_params(hv_ekf_params *p)
{
    if (!p) return;
    p->cameraTrailLength = 20; p->hybridMapSize = 0;
    p->noiseScale = 100; p->gravity = 9.819; p->augmentR = 1e-9; p->initZuptR = 1e-4; p->rotationZuptR = 1e-6;
    p->noiseInitialPos = 1e-5; p->noiseInitialOri = 0.0316227766; p->noiseInitialVel = 0.1;
    p->noiseInitialPosTrail = 100; p->noiseInitialOriTrail = 3.16227766;
    p->noiseInitialBGA = 1e-3; p->noiseInitialBAA = 1e-6; p->noiseInitialBAT = 1e-5; p->noiseInitialSFT = 1e-5;
    p->noiseProcessAcc = 0.003; p->noiseProcessGyro = 0.00017; p->noiseProcessBAA = 1e-4; p->noiseProcessBGA = 0;
    p->noiseProcessBAARev = 0.1; p->noiseProcessBGARev = 0.1;
}

void hv_ekf_destroy(hv_ekf *h)
{
    if (!h) return;
    Ekf *e = &h->e;
    if (e->c) for (hipStream_t s : {e->c->stream, e->c->aux_stream}) if (s) (void)hipStreamSynchronize(s);   // both streams, before the first free
    if (e->longc.ev_fork) (void)hipEventDestroy(e->longc.ev_fork);
    if (e->longc.ev_join) (void)hipEventDestroy(e->longc.ev_join);
    delete h;
}

int hv_ekf_create(hv_ctx *ctx, const hv_ekf_params *par, int batch, hv_ekf **out)
{
    if (!ctx || !par || !out || batch < 1 || par->cameraTrailLength < 1 || par->hybridMapSize < 0) return HV_ERR_INVALID;
    *out = nullptr;
    Ctx *c = hv::ctx_of(ctx);
    hv_ekf *h = new (std::nothrow) hv_ekf();
    if (!h) return HV_ERR_NOMEM;
    Ekf *e = &h->e;
    e->c = c; e->par = *par; e->batch = batch;
    e->cam = par->cameraTrailLength; e->map_dim = 3 * par->hybridMapSize;
    const int n = e->n = hv::INER + hv::POSE * e->cam + e->map_dim;
    e->noise_scale = par->noiseScale * par->noiseScale;
    e->max_rows = n;
    const size_t nn = (size_t)n * n;
    bool ok = e->fixed.ensure(*e) == HV_OK;
    // the context's staging arena is made to hold every SMALL section of this batch's host-pointer entries at once -- residuals
    // [n x batch], IMU samples, the [batch] vectors -- so that only a Jacobian upload (up to n x n x batch) can still grow it
    hv::Stage small(c);
    const size_t B = batch;
    small.take<double>(n * B); small.take<double>(7 * HV_EKF_MAX_PREDICT_SAMPLES * B);
    small.take<double>(B); small.take<double>(B); small.take<int>(B); small.take<int>(B); small.take<unsigned char>(B);
    ok = ok && small.reserve() == HV_OK;
    if (ok && hipMemset(e->fixed.err_dev, 0, sizeof(int)) != hipSuccess) ok = false;
    if (!ok) { hv_ekf_destroy(h); return HV_ERR_NOMEM; }

    // initial state and covariance: EKFImplementation ctor, ekf.cpp:153-296
    // (dydx is zero until the first predict writes it: a reset filter and a new one are then equal in every array)
    std::vector<double> m0(n, 0.0), P0(nn, 0.0), Q0(144, 0.0);
    const hv::EkfFresh fresh = hv::ekf_fresh(*par, n, e->noise_scale);
    for (int i = 0; i < n; i++) { m0[i] = fresh.mean(i); P0[(size_t)i * n + i] = fresh.p_diag(i); }
    for (int i = 0; i < hv::QD; i++) Q0[i * (hv::QD + 1)] = fresh.q_diag(i);
    int rc = hipMemset(e->fixed.dydx, 0, sizeof(double) * 400 * batch) == hipSuccess ? HV_OK : HV_ERR_HIP;
    for (int b = 0; b < batch && rc == HV_OK; b++) {
        rc = hv_ekf_set_state(h, b, m0.data(), P0.data());
        if (rc == HV_OK) rc = hv_ekf_set_process_noise(h, b, Q0.data());
    }
    if (rc != HV_OK) { hv_ekf_destroy(h); return rc; }
    *out = h;
    return HV_OK;
}

void hv_vu_default_params(hv_vu_params *p)
{
    if (!p) return;
    *p = hv_vu_params{};
    p->triangulationConvergenceThreshold = 1e-2; p->triangulationConvergenceR = 11.0;            // parameter_definitions.c:37-44
    p->triangulationRcondThreshold = 1e-8; p->triangulationGaussNewtonIterations = 10;
    p->triangulationMinDist = 0; p->triangulationMaxDist = 1e300;
    p->estimateImuCameraTimeShift = 1;                                                          // :163
    p->trackRmseThreshold = -1.0; p->trackOutlierThresholdGrowthFactor = 1.0;                   // :21,27
    p->useStereo = 0;
    const double imu[9] = {1, 0, 0, 0, -1, 0, 0, 0, -1};                                         // :178 imuToCameraMatrix (symmetric)
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) {
        const double v = r < 3 && c < 3 ? imu[3 * r + c] : (r == c ? 1.0 : 0.0);
        p->imuToCamera[4 * r + c] = v; p->secondImuToCamera[4 * r + c] = v;
    }
    const double tr[3] = {0.0075, 0.013, -0.0003};                                               // :187 stereoCameraTranslation
    for (int r = 0; r < 3; ++r) p->secondImuToCamera[4 * r + 3] += tr[r];                         // tracker/util.cpp:100-105
}

int hv_ekf_frame_error(hv_ekf *h, int *flags)
{
    if (!h || !flags) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    HV_HIP(c, hipMemcpyAsync(flags, e->fixed.err_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    if (*flags) HV_HIP(c, hipMemsetAsync(e->fixed.err_dev, 0, sizeof(int), c->stream));
    return HV_OK;
}

/* developer aid (not in the public header): the 16 phase time stamps of the last predict, update and gate kernels; zeros unless the
   library was built with HV_EKF_PHASE_STAMPS. Every family file stamps an array of its own (ekf_device.hpp); a slot is the largest
   value among them: the stamps are cycle-counter readings, so the last writer wins, as it did when the families shared one array.
   That assumes counters that are comparable across the chip's dies, which nobody has checked. */
int hv_debug_ekf_phase_stamps(hv_ekf *h, long long *out8)
{
    if (!h || !out8) return HV_ERR_INVALID;
    Ctx *c = h->e.c;
    HV_HIP(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 16; i++) out8[i] = 0;
#ifdef HV_EKF_PHASE_STAMPS
    for (const auto read : {hv::ekf_predict_phase_stamps, hv::ekf_update_phase_stamps, hv::ekf_gate_phase_stamps}) {
        long long s[16];
        HV_HIP(c, read(s));
        for (int i = 0; i < 16; i++) if (s[i] > out8[i]) out8[i] = s[i];
    }
#endif
    return HV_OK;
}

int hv_ekf_state_dim(const hv_ekf *h) { return h ? h->e.n : HV_ERR_INVALID; }
int hv_ekf_batch(const hv_ekf *h) { return h ? h->e.batch : HV_ERR_INVALID; }

int hv_ekf_set_state(hv_ekf *h, int b, const double *m, const double *P)
{
    if (!h || b < 0 || b >= h->e.batch) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c; const size_t n = e->n;
    if (m) HV_HIP(c, hipMemcpyAsync(e->fixed.m + b * n, m, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    if (P) HV_HIP(c, hipMemcpyAsync(e->fixed.P + b * n * n, P, sizeof(double) * n * n, hipMemcpyHostToDevice, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    return HV_OK;
}

int hv_ekf_get_state(hv_ekf *h, int b, double *m, double *P)
{
    if (!h || b < 0 || b >= h->e.batch) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c; const size_t n = e->n;
    if (m) HV_HIP(c, hipMemcpyAsync(m, e->fixed.m + b * n, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    if (P) HV_HIP(c, hipMemcpyAsync(P, e->fixed.P + b * n * n, sizeof(double) * n * n, hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    return HV_OK;
}

int hv_ekf_get_means(hv_ekf *h, double *m_all)
{
    if (!h || !m_all) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    HV_HIP(c, hipMemcpyAsync(m_all, e->fixed.m, sizeof(double) * e->n * e->batch, hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    return HV_OK;
}

int hv_ekf_set_process_noise(hv_ekf *h, int b, const double *Q)
{
    if (!h || !Q || b < 0 || b >= h->e.batch) return HV_ERR_INVALID;
    Ctx *c = h->e.c;
    HV_HIP(c, hipMemcpyAsync(h->e.fixed.Q + (size_t)b * 144, Q, sizeof(double) * 144, hipMemcpyHostToDevice, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    return HV_OK;
}

int hv_ekf_get_process_noise(hv_ekf *h, int b, double *Q)
{
    if (!h || !Q || b < 0 || b >= h->e.batch) return HV_ERR_INVALID;
    Ctx *c = h->e.c;
    HV_HIP(c, hipMemcpyAsync(Q, h->e.fixed.Q + (size_t)b * 144, sizeof(double) * 144, hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    return HV_OK;
}

int hv_ekf_get_dydx(hv_ekf *h, int b, double *F)
{
    if (!h || !F || b < 0 || b >= h->e.batch) return HV_ERR_INVALID;
    Ctx *c = h->e.c;
    HV_HIP(c, hipMemcpyAsync(F, h->e.fixed.dydx + (size_t)b * 400, sizeof(double) * 400, hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    return HV_OK;
}

int hv_ekf_device_pointers(hv_ekf *h, double **m_dev, double **P_dev)
{
    if (!h) return HV_ERR_INVALID;
    if (m_dev) *m_dev = h->e.fixed.m;
    if (P_dev) *P_dev = h->e.fixed.P;
    return HV_OK;
}

// the staged inputs of an update launch: H [batch][nr x l], v [batch][nr], and where given R's diagonal [batch] and the flags [batch]
namespace {
struct UpdateStage : hv::Stage {
    hv::StageSection<double> H, v, r;
    hv::StageSection<unsigned char> active;
    UpdateStage(Ekf *e, size_t nr, size_t l, const double *h_H, const double *h_v, const double *rdiag, const unsigned char *h_active)
        : hv::Stage(e->c), H(in(h_H, nr * l * e->batch)), v(in(h_v, nr * e->batch)), r(in(rdiag, (size_t)e->batch)), active(in(h_active, (size_t)e->batch)) {}
};
}  // namespace

int hv_ekf_update(hv_ekf *h, int nr, int l, const double *H, const double *y, const double *r_diag,
                  const unsigned char *active, int normalize_all)
{
    if (!h || !H || !y || !r_diag) return HV_ERR_INVALID;
    Ekf *e = &h->e;
    if (nr < 1 || nr > e->max_rows || l < 1 || l > e->n) return HV_ERR_INVALID;
    UpdateStage u(e, nr, l, H, y, r_diag, active);
    int rc = u.upload();
    if (rc != HV_OK) return rc;
    hv::UpdateRequest rq;
    rq.nr = nr; rq.l = l; rq.H_dev = u.at(u.H); rq.v_dev = u.at(u.v); rq.rdiag_dev = u.at(u.r); rq.mode = 1; rq.generic = 1; rq.normalize_all = normalize_all;
    rq.active_dev = u.at_or_null(u.active);
    return hv::ekf_launch_update(e, rq);
}

int hv_ekf_visual_gate(hv_ekf *h, int nr, int l, const double *H, const double *v, double r, double *chi2, int *status)
{
    if (!h || !H || !v) return HV_ERR_INVALID;
    Ekf *e = &h->e;
    if (nr < 1 || nr > e->max_rows || l < 1 || l > e->n) return HV_ERR_INVALID;
    UpdateStage u(e, nr, l, H, v, nullptr, nullptr);
    const auto o_chi2 = u.out(chi2, (size_t)e->batch);
    const auto o_status = u.out(status, (size_t)e->batch);
    int rc = u.upload();
    if (rc != HV_OK) return rc;
    rc = hv::ekf_launch_update(e, hv::gate_request(nr, l, u.at(u.H), u.at(u.v), r * r * e->noise_scale, u.at(o_chi2), u.at(o_status)));
    return rc != HV_OK ? rc : u.download();
}

int hv_ekf_visual_update(hv_ekf *h, int nr, int l, const double *H, const double *v, double r, const unsigned char *active)
{
    if (!h || !H || !v) return HV_ERR_INVALID;
    Ekf *e = &h->e;
    if (nr < 1 || nr > e->max_rows || l < 1 || l > e->n) return HV_ERR_INVALID;
    UpdateStage u(e, nr, l, H, v, nullptr, active);
    int rc = u.upload();
    if (rc != HV_OK) return rc;
    return hv::ekf_launch_update(e, hv::inlier_update_request(nr, l, u.at(u.H), u.at(u.v), r * r * e->noise_scale, u.at_or_null(u.active)));
}

int hv_ekf_visual_dev(hv_ekf *h, int nr, int l, const double *H_dev, const double *v_dev, double r, int mode,
                      double *chi2_dev, int *status_dev)
{
    if (!h || !H_dev || !v_dev || mode < 0 || mode > 2) return HV_ERR_INVALID;
    Ekf *e = &h->e;
    const int stream_gate = e->c->knob.ekf_stream_gate;
    if (mode == 0 && (stream_gate == 1 || (stream_gate < 0 && e->batch > 256))) {      // gate only, many filters: two per CU
        bool done = false;
        hv::GateStreamRequest g;
        g.nr = nr; g.l = l; g.H_dev = H_dev; g.v_dev = v_dev; g.rd = r * r * e->noise_scale; g.chi2_dev = chi2_dev; g.status_dev = status_dev; g.done = &done;
        const int rc = hv::ekf_launch_gate_stream(e, g);
        if (rc != HV_OK || done) return rc;
    }
    hv::UpdateRequest rq = hv::gate_request(nr, l, H_dev, v_dev, r * r * e->noise_scale, chi2_dev, status_dev);
    rq.mode = mode; rq.normalize_all = 1;
    return hv::ekf_launch_update(e, rq);
}

}  // extern "C"
