// Track visits and frame loops of the EKF (hv_ekf_visual_track* / hv_ekf_visual_frame*): which prepare, gate and update launches serve a
// visit of a given shape, on which stream and in which order; the speculative and the batch loop; the host-pointer forms of these
// entries. The kernels and their launchers live in ekf_update.hip, ekf_gate.hip and vu_prepare.hip (triangulation, prepare, fused gates);
// the three small kernels here are launched by this file alone.
#include <algorithm>
#include <limits.h>

#include "chi2inv95.h"
#include "ekf_host.hpp"

namespace hv {

namespace {
__global__ void fill_doubles_kernel(double *dst, int n, double value)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = value;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Hybrid map (backend.cpp:1160-1168): an inlier pose-trail track that is OFFERED a map slot becomes a map point -- insertMapPoint
// (ekf.cpp:911-921: the slot's rows and columns of P zeroed, 1e6 on its diagonal, the triangulated point in the mean) -- INSTEAD of
// being applied. One workgroup per filter; active_out = the filters whose track still takes updateVisualTrack.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ekf_hybrid_insert_kernel(int n, int map_base, double *m_all, double *P_all, const unsigned char *active,
                                                                const int *gate, const int *map_index, const int *offer, const double *pf,
                                                                unsigned char *active_out)
{
    const int b = blockIdx.x, t = threadIdx.x;
    const bool act = active[b] != 0, inlier = act && gate[b] == 0;
    const int slot = (inlier && (!map_index || map_index[b] < 0) && offer) ? offer[b] : -1;
    if (t == 0) active_out[b] = (act && slot < 0) ? 1 : 0;
    if (slot < 0) return;
    const int off = map_base + 3 * slot;
    double *m = m_all + (size_t)b * n, *P = P_all + (size_t)b * n * n;
    for (int i = t; i < 3 * n; i += 256) {
        const int k = i / n, j = i - k * n;
        P[(size_t)(off + k) * n + j] = 0.0;
        P[(size_t)j * n + off + k] = 0.0;
    }
    __syncthreads();
    if (t < 3) { P[(size_t)(off + t) * n + off + t] = 1e6; m[off + t] = pf[3 * b + t]; }
}

// ---------------------------------------------------------------------------------------------
// batchVisualUpdate (backend.cpp:1001-1010, 1169-1183, 1255-1262): inside a batch every track is gated against the SAME (m, P) -- the
// updates are deferred --, so one speculative pass (every pending track prepared and gated in one launch) IS the reference's loop up to
// the next flush. This kernel is the bookkeeping of that loop for one filter: it walks the pending tracks in visit order, appends the
// inliers' blocks [H; v] to the filter's batch while they fit max_rows and the quota lasts, and leaves the stacked dense H (column-major,
// leading dimension = the batch's row count) and v for ONE updateVisualTrack launch (ragged dense update: rows_out). A block that does
// not fit ends the pass: the batch is flushed by that update, the block opens the NEXT batch unchanged (carry), and the next pass gates
// the tracks behind it against the updated state -- the reference's flush-then-append.
// ---------------------------------------------------------------------------------------------
struct BatchAssembleArgs {
    int n, n_tracks, batch, max_rows, max_successful, rows_stride, na_max, ncam;
    const double *Hc, *v;             // compact records of the gate launch: [n_tracks][batch] x (rows_stride x na_max), x rows_stride
    const int *acol, *nr_rec;         // [records][na_max]; rows of every record (null: rows_stride)
    const unsigned char *active; const int *gate;
    int *cursor, *success_counter, *carry;   // carry [batch]: the track whose block opens the next batch (-1: none)
    double *Hd, *vd;                  // [batch][max_rows x n], [batch][max_rows]
    int *rows_out; unsigned char *any_out;
};
constexpr int BATCH_THREADS = 256;
__global__ __launch_bounds__(BATCH_THREADS) void ekf_batch_assemble_kernel(BatchAssembleArgs a)
{
    __shared__ int s_list[64], s_off[64], s_cnt, s_rows;
    const int b = blockIdx.x, t = threadIdx.x;
    if (t == 0) {
        int succ = a.success_counter[b], rows = 0, cnt = 0, j = a.cursor[b];
        // the track whose block did not fit the previous batch opens this one AS IT WAS prepared and gated -- against the state before
        // the flush: the reference has its H, f, y in hand when it flushes and appends them afterwards (backend.cpp:1171-1182)
        const int cj = a.carry[b];
        if (cj >= 0) {
            const int rec = cj * a.batch + b;
            s_list[0] = cj; s_off[0] = 0; rows = a.nr_rec ? a.nr_rec[rec] : a.rows_stride; cnt = 1; ++succ;
            a.carry[b] = -1;
        }
        for (; j < a.n_tracks; ++j) {
            if (succ >= a.max_successful) break;                                   // quota (backend.cpp:1233): the next pass marks the rest NOT_VISITED
            const int rec = j * a.batch + b;
            if (!a.active[rec] || a.gate[rec] != 0) continue;                     // failed triangulation / outlier: final, nothing to apply
            const int nr = a.nr_rec ? a.nr_rec[rec] : a.rows_stride;
            if (rows + nr > a.max_rows || cnt == 64) { a.carry[b] = j; ++j; break; }      // flush first; the block waits for the next batch
            s_list[cnt] = j; s_off[cnt] = rows; rows += nr; ++cnt; ++succ;
        }
        a.cursor[b] = j;                                                           // (n_tracks when every pending track is final)
        a.success_counter[b] = succ;
        a.rows_out[b] = rows; a.any_out[b] = rows > 0 ? 1 : 0;
        s_cnt = cnt; s_rows = rows;
    }
    __syncthreads();
    const int cnt = s_cnt, rows = s_rows;
    if (rows == 0) return;
    double *Hd = a.Hd + (size_t)b * a.max_rows * a.n, *vd = a.vd + (size_t)b * a.max_rows;
    for (int i = t; i < rows * a.n; i += BATCH_THREADS) Hd[i] = 0.0;
    __syncthreads();
    for (int q = 0; q < cnt; ++q) {
        const int rec = s_list[q] * a.batch + b, off = s_off[q];
        const int nr = a.nr_rec ? a.nr_rec[rec] : a.rows_stride, na = 7 * (nr / (2 * a.ncam)) + 1;
        const double *Hc = a.Hc + (size_t)rec * a.rows_stride * a.na_max, *v = a.v + (size_t)rec * a.rows_stride;
        const int *acol = a.acol + (size_t)rec * a.na_max;
        for (int i = t; i < na * nr; i += BATCH_THREADS) {
            const int u = i / nr, r = i - u * nr;
            Hd[(size_t)acol[u] * rows + off + r] = Hc[i];                          // (compact column u of the record, leading dimension nr)
        }
        for (int r = t; r < nr; r += BATCH_THREADS) vd[off + r] = v[r];
    }
}

}  // namespace hv

using hv::Ctx;
using hv::Ekf;

extern "C" {

static int vu_fill_args(Ekf *e, const hv_vu_params *p, int np, const int *idx, const double *feat, const double *vel,
                        const double *y, hv::VuPrepareArgs &a)
{
    if (!p || !idx || !feat || !vel || np < 2 || np > e->cam + 1) return HV_ERR_INVALID;
    a = hv::VuPrepareArgs{};
    a.batch = e->batch; a.n = e->n; a.np = np; a.stereo = p->useStereo ? 1 : 0;
    a.m = e->fixed.m; a.pose_index = idx; a.features = feat; a.velocities = vel; a.y = y;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) {
        a.imu_to_cam[0][4 * r + c] = p->imuToCamera[4 * r + c];
        a.imu_to_cam[1][4 * r + c] = p->secondImuToCamera[4 * r + c];
    }
    a.conv_threshold = p->triangulationConvergenceThreshold; a.conv_r = p->triangulationConvergenceR;
    a.rcond_threshold = p->triangulationRcondThreshold; a.min_dist = p->triangulationMinDist; a.max_dist = p->triangulationMaxDist;
    a.gn_iters = (int)p->triangulationGaussNewtonIterations; a.est_shift = p->estimateImuCameraTimeShift ? 1 : 0;
    a.defer_h = e->c->knob.ekf_defer_jacobian != 0;
    a.linear = p->useLinearTriangulation ? 1 : 0;
    // adaptive outlier thresholds (ABI 3): the RMSE test applies everywhere the fused gate runs; the per-filter growth only inside a
    // frame loop (visual_frame_dev_impl hands the multiplier array over through Ekf::gate_scale_on)
    a.rmse_thr = p->trackRmseThreshold; a.growth = p->trackOutlierThresholdGrowthFactor;
    a.gate_scale = e->gate.on ? e->gate.scale : nullptr;
    if (!(a.growth > 0.0)) return HV_ERR_INVALID;
    return HV_OK;
}

// the `fused` group of a prepare launch: the compact Jacobian and its column list instead of the dense H, and what the chi2 gate inside
// the launch reads (R = rd_gate I, already scaled by noiseScale)
static void vu_fill_fused(const Ekf *e, hv::VuPrepareArgs &a, int fused, double *Hc, int *acol, int np, double rd_gate, double *chi2_dev)
{
    a.fused = fused; a.H = nullptr; a.Hc = Hc; a.acol = acol; a.na_max = 7 * np + 1; a.P = e->fixed.P;
    a.rd_gate = rd_gate; a.noise_scale = e->noise_scale; a.chi2 = chi2_dev;
}

// the speculative-record part of a prepare launch (speculative frame loops, batch loop): grid (filters, n_tracks), every array a
// [track][filter] record of the sp* buffers. Returns the per-record row counts the prepare launches write (ragged frames), or null.
static const int *vu_fill_spec(Ekf *e, hv::VuPrepareArgs &a, int n_tracks, const int *np_rec_dev, double *pf_dev, int *status_dev,
                               int *gate_status_dev, int *success_counter_dev, int max_successful)
{
    a.H = e->spec.H; a.v = e->spec.v; a.f = nullptr; a.pf = pf_dev ? pf_dev : e->spec.pf; a.status = status_dev; a.active = e->spec.active;
    a.gate_status = gate_status_dev; a.success_counter = success_counter_dev; a.max_successful = max_successful;
    a.spec_tracks = n_tracks; a.cursor = e->spec.cursor; a.epoch = e->spec.epoch;
    if (!np_rec_dev) return nullptr;
    a.np_rec = np_rec_dev; a.rows_out = e->spec.rec_rows;
    return e->spec.rec_rows;
}

// the apply launch of a speculative pass (spec 2): per filter the first pending record whose gate said INLIER (gate_in_dev) is applied
// and the cursor moves behind it
static hv::UpdateRequest spec_apply_request(Ekf *e, int nr, double rd, int n_tracks, const int *gate_in_dev, int *success_counter_dev,
                                            int max_successful, const int *nr_rec)
{
    hv::UpdateRequest rq = hv::inlier_update_request(nr, e->n, e->spec.H, e->spec.v, rd, e->spec.active);
    rq.gate_in_dev = gate_in_dev; rq.nr_rec_dev = nr_rec;
    hv::set_spec_pass(rq, 2, n_tracks, e->spec.cursor, success_counter_dev, max_successful);
    return rq;
}

int hv_ekf_visual_prepare_dev(hv_ekf *h, const hv_vu_params *p, int np, const int *idx, const double *feat, const double *vel,
                              const double *y, double *H_dev, double *v_dev, double *f_dev, double *pf_dev, int *status_dev,
                              unsigned char *active_dev)
{
    if (!h || !H_dev || !v_dev || !pf_dev || !status_dev) return HV_ERR_INVALID;
    Ekf *e = &h->e;
    hv::VuPrepareArgs a;
    int rc = vu_fill_args(e, p, np, idx, feat, vel, y, a);
    if (rc != HV_OK) return rc;
    a.H = H_dev; a.v = v_dev; a.f = f_dev; a.pf = pf_dev; a.status = status_dev; a.active = active_dev;
    return hv::launch_vu_prepare(e->c, a);
}

// (r06: where the split form serves the visit -- stereo, iterative triangulation, more filters than CUs -- the short class ends at
//  12 poses = 48 rows, what the record-fed gate stages three to a CU, instead of 11: 4 % of a ragged visit's records leave the long
//  class, its 158 KB gate and its two block updates)
static hv::VisitShape visit_shape(const Ekf *e, int np, bool stereo, bool linear)
{
    hv::VisitShape v{};
    v.ncam = stereo ? 2 : 1; v.np_short = 22 / v.ncam; v.rows = 2 * np * v.ncam;
    if (hv::vu_split_short_ok(e->c, e->n, stereo, e->batch, linear)) v.np_short = hv::vu_split_short_np(e->c);
    v.long_ok = e->c->knob.ekf_fused_gate != 0 && e->n <= 160 && v.rows > 48 && v.rows <= 96 && v.rows < HV_CHI2INV95_N && (v.rows + 3) / 4 * 2 <= 48;
    v.two_class = np > v.np_short && v.long_ok && hv::vu_fused_supported(e->c, e->n, v.np_short, stereo, e->batch);
    return v;
}

// One track visit of a session with a hybrid map (odometry.hybridMapSize > 0; backend.cpp:1016, 1075-1082, 1146, 1160-1168):
//   map_update_dev [batch]: the map point a mapPointUpdate track belongs to (>= 0) -- the point is read from the state, status
//                           HV_TRI_HYBRID, H carries dip R in the point's columns -- or -1 for a pose-trail track;
//   map_offer_dev [batch]:  the slot ekfStateIndex.offerMapPoint would hand to this track if the gate accepts it (-1: none; the offer
//                           does not depend on the filter, so the adapter evaluates it up front): such an inlier is INSERTED as a map
//                           point instead of being applied.
// Dense kernels (the state is wider than 160 columns). Either array may be NULL.
int hv_ekf_visual_track_hybrid_dev(hv_ekf *h, const hv_vu_params *p, int np, const int *idx, const double *feat, const double *vel,
                                   const double *y, const int *map_update_dev, const int *map_offer_dev, double r_gate, double r_update,
                                   int *status_dev, int *gate_status_dev, double *chi2_dev, double *pf_dev)
{
    if (!h || !status_dev || !gate_status_dev || !y) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    if (e->map_dim <= 0 && (map_update_dev || map_offer_dev)) return HV_ERR_INVALID;
    hv::VuPrepareArgs a;
    int rc = vu_fill_args(e, p, np, idx, feat, vel, y, a);
    if (rc != HV_OK) return rc;
    if (a.rmse_thr >= 0.0) return HV_ERR_UNSUPPORTED;                  // (the dense gate has no RMSE test)
    const int rows = 2 * np * (a.stereo ? 2 : 1);
    if (rows > e->max_rows || rows >= HV_CHI2INV95_N) return HV_ERR_INVALID;
    rc = e->visit.ensure(*e, rows);
    if (rc != HV_OK) return rc;
    const double ns = e->noise_scale;
    double *pf = pf_dev ? pf_dev : e->visit.pf;
    a.H = e->visit.H; a.v = e->visit.v; a.f = nullptr; a.pf = pf; a.status = status_dev; a.active = e->visit.active; a.gate_status = gate_status_dev;
    a.map_index = map_update_dev; a.map_base = e->n - e->map_dim;
    rc = hv::launch_vu_prepare(c, a);
    if (rc != HV_OK) return rc;
    // visualTrackOutlierCheck, then -- per filter -- insertMapPoint or updateVisualTrack where it passed
    rc = hv::ekf_launch_update(e, hv::gate_request(rows, e->n, e->visit.H, e->visit.v, r_gate * r_gate * ns, chi2_dev, gate_status_dev, e->visit.active));
    if (rc != HV_OK) return rc;
    hipLaunchKernelGGL(hv::ekf_hybrid_insert_kernel, dim3(e->batch), dim3(256), 0, c->stream, e->n, e->n - e->map_dim, e->fixed.m, e->fixed.P, e->visit.active,
                       gate_status_dev, map_update_dev, map_offer_dev, pf, e->visit.apply);
    HV_HIP(c, hipGetLastError());
    return hv::ekf_launch_update(e, hv::inlier_update_request(rows, e->n, e->visit.H, e->visit.v, r_update * r_update * ns, e->visit.apply, gate_status_dev));
}

// What the launch sequences of one visit share (visual_track_dev_impl): the shape, the thresholds, the compaction lists, the outputs.
struct Visit {
    Ekf *e; Ctx *c;
    int np, rows, ncam;
    double r_gate, r_update, ns;
    hipStream_t main_stream;
    int *cnt_long, *list_long;             // records of the long class (collected by the short class's launch, or presorted per frame)
    int *cnt_inl_long, *list_inl_long;     // ... those of them whose gate said INLIER
    const int *nr_rec;                     // ragged: rows of every record, written by the prepare launch
    int *gate_status_dev, *success_counter_dev;
    double *chi2_dev;

    // the gate launch `g` of one length class in split form: the triangulation front first, on the same stream; false = not a shape
    // the split form serves (the caller issues the fused launch)
    // phase: 0 = both launches, 1 = the triangulation only, 2 = the gate only (one-stream visits interleave the two classes' launches:
    // knob ekf_long_first)
    bool split_launch(hv::VuPrepareArgs &g, hipStream_t stream, int *rc_out, int phase = 0)
    {
        if (!hv::vu_split_supported(c, g, g.fused)) return false;
        int rc2 = e->tri.ensure(*e, hv::vu_tri_rec_stride(np, ncam), main_stream);
        g.tri_rec = e->tri.rec; g.tri_stride = e->tri.stride;
        if (rc2 == HV_OK && phase != 2) rc2 = hv::launch_vu_tri(c, g, stream);
        if (rc2 == HV_OK && phase != 1) { g.from_rec = 1; rc2 = hv::launch_vu_prepare(c, g, stream); }
        *rc_out = rc2;
        return true;
    }

    // prepare + gate of the long class on `stream` (nothing else touches c->stream: r03 swapped the context's stream for these calls)
    int long_prepare_gate(hv::VuPrepareArgs l_, double *Hc, double *vv, int *acol, unsigned char *act, bool listed, hipStream_t stream, int phase = 0)
    {
        l_.v = vv; l_.active = act;
        if (listed) { l_.rec_count = cnt_long; l_.rec_list = list_long; }
        const bool adaptive_gate = l_.rmse_thr >= 0.0 || l_.gate_scale;     // (served by the fused gates only)
        if (c->knob.ekf_long_fused == 0 && adaptive_gate) return HV_ERR_UNSUPPORTED;
        if (c->knob.ekf_long_fused != 0) {
            vu_fill_fused(e, l_, 3, Hc, acol, np, r_gate * r_gate * ns, chi2_dev);
            l_.inl_count = cnt_inl_long; l_.inl_list = list_inl_long;
            int rc_s = HV_OK;
            if (split_launch(l_, stream, &rc_s, phase)) return rc_s;
            if (phase == 1) return HV_OK;                      // (not a split shape: the fused launch is the gate phase)
            return hv::launch_vu_prepare(c, l_, stream);
        }
        // (its own gate launch: the prepare launch takes neither P nor the threshold; the pair has no triangulation-only form, so it
        //  is the gate phase of an interleaved one-stream visit -- launching it in both phases listed every long inlier twice)
        if (phase == 1) return HV_OK;
        l_.fused = 2; l_.H = nullptr; l_.Hc = Hc; l_.acol = acol; l_.na_max = 7 * np + 1; l_.chi2 = chi2_dev;
        const int rc2 = hv::launch_vu_prepare(c, l_, stream);
        if (rc2 != HV_OK) return rc2;
        hv::SparseGateRequest g;
        g.np = np; g.ncam = ncam; g.Hc_dev = Hc; g.v_dev = vv; g.acol_dev = acol; g.nr_rec_dev = nr_rec; g.active_dev = act;
        g.rd = r_gate * r_gate * ns; g.chi2_dev = chi2_dev; g.status_dev = gate_status_dev;
        if (listed) { g.rec_count = cnt_long; g.rec_list = list_long; }
        g.inl_count = cnt_inl_long; g.inl_list = list_inl_long; g.stream = stream;
        return hv::ekf_launch_sparse_gate(e, g);
    }

    // the two block updates of the long class's inliers on the context stream; with short_upd the short class's update shares their grids
    int long_updates(double *Hc, double *vv, int *acol, unsigned char *act, double *dm, const hv::UpdateRequest *short_upd)
    {
        const int half_rows = 2 * ((rows + 3) / 4);            // the longer of the two blocks of the longest record
        hv::UpdateRequest b1 = hv::inlier_update_request(half_rows, e->n, Hc, vv, r_update * r_update * ns, act, gate_status_dev);
        b1.nr_rec_dev = nr_rec; b1.nr_stride = rows;
        b1.compact = hv::compact_columns(acol, 7 * np + 1, ncam, cnt_inl_long, list_inl_long);
        b1.compact.nr_full = rows; b1.compact.dm = dm;
        hv::UpdateRequest b2 = b1;
        // (block 1 may turn a record's gate status into CHI2 when it meets a non-positive pivot: block 2 then skips it -- r03 advisor)
        b1.compact.half = 1; b1.compact.gate_rw = gate_status_dev; b1.normalize_all = -1;
        b2.compact.half = 2; b2.success_counter_dev = success_counter_dev;
        int rc2 = HV_OK;
        if (short_upd) {
            bool dual = false;
            rc2 = hv::ekf_launch_update_paired(e, *short_upd, b1, b2, &dual);
            if (rc2 != HV_OK || dual) return rc2;
            rc2 = hv::ekf_launch_update(e, *short_upd);
            if (rc2 == HV_OK) rc2 = hv::ekf_launch_update(e, b1);
        } else rc2 = hv::ekf_launch_update(e, b1);
        if (rc2 != HV_OK) return rc2;
        return hv::ekf_launch_update(e, b2);
    }
};

static int visual_track_dev_impl(hv_ekf *h, const hv_vu_params *p, int np, const int *idx, const double *feat, const double *vel,
                                 const double *y, double r_gate, double r_update, int *status_dev, int *gate_status_dev,
                                 double *chi2_dev, double *pf_dev, int *success_counter_dev, int max_successful,
                                 const int *np_rec_dev = nullptr)
{
    if (!h || !status_dev || !gate_status_dev || !y) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    hv::VuPrepareArgs a;
    int rc = vu_fill_args(e, p, np, idx, feat, vel, y, a);
    if (rc != HV_OK) return rc;
    const int rows = 2 * np * (a.stereo ? 2 : 1);
    if (rows > e->max_rows) return HV_ERR_INVALID;
    rc = e->visit.ensure(*e, rows);
    if (rc != HV_OK) return rc;
    // ragged batch (filters with tracks of different lengths, or none, in one visit): np is the longest track = the record stride;
    // the prepare launch writes every filter's row count for the gate / update launch
    const int *nr_rec = nullptr;
    if (np_rec_dev) {
        a.np_rec = np_rec_dev; a.rows_out = e->visit.rec_rows; nr_rec = e->visit.rec_rows;
    }
    a.H = e->visit.H; a.v = e->visit.v; a.f = nullptr; a.pf = pf_dev ? pf_dev : e->visit.pf; a.status = status_dev; a.active = e->visit.active;
    a.gate_status = gate_status_dev;                       // preset to NOT_COMPUTED; the gate overwrites it where it runs
    a.success_counter = success_counter_dev; a.max_successful = max_successful;
    const double ns = e->noise_scale;
    hipStream_t main_stream = c->stream;
    // r03 default: visualTrackOutlierCheck runs INSIDE the prepare launch on the active columns of H (vu_gate kernels: the Jacobian
    // of a rejected track never leaves LDS and only P(a, a) is read); updateVisualTrack then runs where the gate said INLIER, staging the
    // compact Jacobian through its column map (7 of 20 visits at most -- backend.cpp:1233-1238 -- pay the full H P + downdate).
    // Long tracks (more than 48 rows / 22 camera poses: 12 .. 21 stereo poses): prepare + column-sparse gate of up to 96 rows in ONE
    // launch (r04: vu_gate_long_kernel; r03: vu_compact_kernel + ekf_sparse_gate_big_kernel, kept behind knob ekf_long_fused = 0) and the
    // update as TWO block updates of at most 48 rows each on the P-resident kernel (UpdateArgs::half).
    const hv::VisitShape shape = visit_shape(e, np, a.stereo != 0, a.linear != 0);
    const int ncam = shape.ncam, np_short = shape.np_short;
    const bool long_ok = shape.long_ok;
    // compaction lists of this visit (VuPrepareArgs): zeroed here, filled by the kernels, consumed by the launches behind them
    const bool own_counts = e->visit_slot < 0 || e->visit_slot >= Ekf::VISIT_SLOTS;
    int *counts = e->fixed.visit_counts + 4 * (own_counts ? Ekf::VISIT_SLOTS : e->visit_slot);
    int *cnt_inl = counts, *list_inl = e->fixed.visit_lists;
    Visit vis{e, c, np, rows, ncam, r_gate, r_update, ns, main_stream, counts + 1, e->fixed.visit_lists + e->batch, counts + 2,
              e->fixed.visit_lists + 2 * (size_t)e->batch, nr_rec, gate_status_dev, success_counter_dev, chi2_dev};
    // frame loop with sorted visits (launch_visit_order): the long class's records are known -- longest first -- before the fused launch runs
    const bool presorted = !own_counts && e->visit_order_ok;
    if (presorted) { vis.cnt_long = e->fixed.visit_long_count + e->visit_slot; vis.list_long = e->fixed.visit_long + (size_t)e->visit_slot * e->batch; }
    if (own_counts) HV_HIP(c, hipMemsetAsync(counts, 0, 4 * sizeof(int), main_stream));
    // Ragged batch with long AND short tracks: two length CLASSES per visit. The short tracks -- 4 of 5 at the reference's defaults, see
    // bench.py sample_track_lengths -- run on the fused two-per-CU kernels, the long ones through the launches above; the records of a visit
    // belong to different filters, so the two launch sequences are independent up to the shared update grids. Every launch skips the
    // other class's records (VuPrepareArgs::np_lo / np_hi, `active`). Schedule of a visit inside a frame loop over more filters than CUs
    // (knob ekf_side_stream != 0, default; HIP-graph capturable: fork at the start of the visit, join in front of the updates):
    //     second stream (Ctx::aux_stream):  prepare + gate (long)              -- enqueued FIRST: it takes its CUs while all are free
    //     context stream:                   fused prepare + gate (short)  | join |  short update + long block 1  ->  rest of short + long block 2
    // Stand-alone visits and small batches: everything on the context's stream, short class first (its launch collects the long list).
    // (r03 also had the whole long chain on the second stream -- knob values 1 and 4 -- and the long class enqueued BEHIND the fused
    //  launch -- 2: all measured slower, removed in r04 together with the stream swap they needed.)
    if (np_rec_dev && shape.two_class) {
        rc = e->longc.ensure(*e, rows, main_stream);
        if (rc != HV_OK) return rc;
        bool use_aux = c->knob.ekf_side_stream != 0 && presorted && c->aux_stream;
        if (use_aux && c->knob.ekf_side_stream == 5) {
            // lanes (knob value 5, their default): no fork while the context stream is being CAPTURED. A captured fork does not run on
            // the library's high-priority second stream when the graph is replayed but on a stream the graph instance creates for the
            // branch -- default priority, bound to whichever hardware queue the process history left least used --, which is exactly the
            // placement lottery the lanes exist to end (r04, scripts/lanes_probe.py: 2 x 1024 sequences 19.2 / 16.3 ms per step with the
            // captured fork after two different process histories, 15.84 ms without it)
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(main_stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) use_aux = false;
        }
        hv::VuPrepareArgs s_ = a;                              // class "short": 2 .. np_short poses (and the records without a track)
        s_.np_lo = 2; s_.np_hi = np_short; s_.class_inactive = 1;
        vu_fill_fused(e, s_, 1, e->visit.H, e->visit.acol, np, r_gate * r_gate * ns, chi2_dev);
        s_.inl_count = cnt_inl; s_.inl_list = list_inl;
        if (!presorted) { s_.long_count = vis.cnt_long; s_.long_list = vis.list_long; }      // (else nothing to collect)
        if (presorted) s_.order = e->fixed.visit_order + (size_t)e->visit_slot * e->batch;     // (frame loop: sorted once per frame)
        hv::VuPrepareArgs l_ = a;
        l_.np_lo = np_short + 1; l_.np_hi = np; l_.class_inactive = 1;
        // fork ... join: every exit between the two goes through the join (a HIP-graph capture must not be left with a dangling fork)
        bool forked = false;
        if (use_aux) {
            hipError_t he = hipEventRecord(e->longc.ev_fork, main_stream);
            if (he == hipSuccess) he = hipStreamWaitEvent(c->aux_stream, e->longc.ev_fork, 0);
            if (he != hipSuccess) return hv::hip_fail(c, he, "fork onto the second stream");
            forked = true;
        }
        rc = HV_OK;
        // which class runs on which stream when the visit forks: the launch that has to START first -- the long class's, which needs
        // whole CUs and finds them only while the chip is empty -- belongs on the stream that does NOT wait for the fork event.
        // r04 default (knob 6, and 5 = the lanes' form of it): long class on the context stream, short class on the second stream.
        // Knob 3 = r03's arrangement: the long class on the second stream, enqueued first -- but released by the fork event about when
        // the short class's 810 two-per-CU workgroups are, so that part of it got its CUs a round late (144 us under that load against
        // 95 alone, profiles/r04/kernel_stats.csv). Measured, one context of 1024 sequences: eager 10.13 -> 9.82 ms per step, HIP-graph
        // replay 9.67 -> 9.63 (profiles/r04/lanes_probe.txt, session 9).
        const bool swap = forked && c->knob.ekf_side_stream != 3;
        hipStream_t long_stream = forked && !swap ? c->aux_stream : main_stream, short_stream = swap ? c->aux_stream : main_stream;
        const bool long_first = presorted && (forked || c->knob.ekf_long_first == 1);
        auto short_phase = [&](int phase) -> int {
            int rc_s = HV_OK;
            if (vis.split_launch(s_, short_stream, &rc_s, phase)) return rc_s;
            return phase == 1 ? HV_OK : hv::launch_vu_prepare(c, s_, short_stream);
        };
        auto long_phase = [&](hipStream_t stream, int phase) -> int {
            return vis.long_prepare_gate(l_, e->longc.H, e->longc.v, e->longc.acol, e->longc.active, true, stream, phase);
        };
        // one-stream sorted visits, knob ekf_long_first: 0 = short class (triangulation, gate) then long class; 1 = long class first;
        // 2 .. 4 (split form, r06) = both triangulations in front of both gates: T long, T short, G long, G short / T short, T long,
        // G short, G long / T long, T short, G short, G long (profiles/r06/visit_launch_order_sweep.txt)
        const int order = presorted && !forked ? c->knob.ekf_long_first : -1;
        if (order >= 2 && order <= 4) {
            const bool lf = order != 3;
            if (lf) rc = long_phase(main_stream, 1);
            if (rc == HV_OK) rc = short_phase(1);
            if (rc == HV_OK && !lf) rc = long_phase(main_stream, 1);
            const bool gl_first = order == 2;
            if (rc == HV_OK && gl_first) rc = long_phase(main_stream, 2);
            if (rc == HV_OK) rc = short_phase(2);
            if (rc == HV_OK && !gl_first) rc = long_phase(main_stream, 2);
        } else {
            if (long_first) rc = long_phase(long_stream, 0);
            if (rc == HV_OK) rc = short_phase(0);
            if (rc == HV_OK && !long_first) rc = long_phase(main_stream, 0);
        }
        if (forked) {
            hipError_t he = hipEventRecord(e->longc.ev_join, c->aux_stream);
            if (he == hipSuccess) he = hipStreamWaitEvent(main_stream, e->longc.ev_join, 0);
            if (he != hipSuccess && rc == HV_OK) rc = hv::hip_fail(c, he, "join of the second stream");
        }
        if (rc != HV_OK) return rc;
        // the short class's update: issued on its own, or -- knob ekf_dual_update (default 1) -- sharing a grid with the first block
        // update of the long class (the two serve different filters)
        hv::UpdateRequest short_upd = hv::inlier_update_request(2 * np_short * ncam, e->n, e->visit.H, e->visit.v, r_update * r_update * ns, e->visit.active, gate_status_dev);
        short_upd.success_counter_dev = success_counter_dev; short_upd.nr_rec_dev = nr_rec; short_upd.nr_stride = rows;
        short_upd.compact = hv::compact_columns(e->visit.acol, s_.na_max, ncam, cnt_inl, list_inl);
        const bool pair = c->knob.ekf_dual_update != 0;
        if (!pair) { rc = hv::ekf_launch_update(e, short_upd); if (rc != HV_OK) return rc; }
        return vis.long_updates(e->longc.H, e->longc.v, e->longc.acol, e->longc.active, e->longc.dm, pair ? &short_upd : nullptr);
    }
    if (long_ok && np > np_short) {                            // every record of the launch may be long (uniform 12 .. 21 stereo poses, or ragged)
        rc = e->longc.ensure(*e, rows, main_stream);
        if (rc != HV_OK) return rc;
        rc = vis.long_prepare_gate(a, e->visit.H, e->visit.v, e->visit.acol, e->visit.active, false, main_stream);
        if (rc != HV_OK) return rc;
        return vis.long_updates(e->visit.H, e->visit.v, e->visit.acol, e->visit.active, e->longc.dm, nullptr);
    }
    if (hv::vu_fused_supported(c, e->n, np, a.stereo, e->batch)) {
        // knob ekf_fused_gate: -1 auto / 1 = the gate inside the prepare launch (vu_gate kernels); 2 = its own launch (vu_compact kernels +
        // ekf_sparse_gate_kernel, three 43 KB workgroups per CU). Measured at 1024 filters x 10 stereo poses (r03, scripts/vu_microbench.py):
        // 156 us against 84 + 67 us per visit, and 9.0 against 9.25 ms for the chained C3 step -- the gate costs ~17 us of a CU per filter
        // in either form (a 40-pivot Cholesky chain on one wave + 430 MFMAs at low occupancy), so the form with one launch and no round trip
        // of Hc through HBM stays the default at every batch size.
        const int fg = c->knob.ekf_fused_gate;
        const bool split_gate = fg == 2;
        if (split_gate && (a.rmse_thr >= 0.0 || a.gate_scale)) return HV_ERR_UNSUPPORTED;   // (adaptive thresholds: fused gates only)
        vu_fill_fused(e, a, split_gate ? 2 : 1, e->visit.H, e->visit.acol, np, r_gate * r_gate * ns, chi2_dev);
        if (!split_gate) { a.inl_count = cnt_inl; a.inl_list = list_inl; }
        { int rc_s = HV_OK; rc = (!split_gate && vis.split_launch(a, main_stream, &rc_s)) ? rc_s : hv::launch_vu_prepare(c, a); }
        if (rc != HV_OK) return rc;
        if (split_gate) {
            hv::SparseGateRequest g;
            g.np = np; g.ncam = a.stereo ? 2 : 1; g.Hc_dev = e->visit.H; g.v_dev = e->visit.v; g.acol_dev = e->visit.acol; g.nr_rec_dev = nr_rec;
            g.active_dev = e->visit.active; g.rd = a.rd_gate; g.chi2_dev = chi2_dev; g.status_dev = gate_status_dev;
            g.inl_count = cnt_inl; g.inl_list = list_inl;
            rc = hv::ekf_launch_sparse_gate(e, g);
            if (rc != HV_OK) return rc;
        }
        hv::UpdateRequest u = hv::inlier_update_request(rows, e->n, e->visit.H, e->visit.v, r_update * r_update * ns, e->visit.active, gate_status_dev);
        u.success_counter_dev = success_counter_dev; u.nr_rec_dev = nr_rec;
        u.compact = hv::compact_columns(e->visit.acol, a.na_max, a.stereo ? 2 : 1, cnt_inl, list_inl);
        return hv::ekf_launch_update(e, u);
    }
    // (the dense kernels below know neither the RMSE test nor the per-filter threshold growth)
    if (a.rmse_thr >= 0.0 || a.gate_scale) return HV_ERR_UNSUPPORTED;
    rc = hv::launch_vu_prepare(c, a);
    if (rc != HV_OK) return rc;
    // Dense path (tracks of more than 48 rows, filters wider than 160, knob ekf_fused_gate = 0): visualTrackOutlierCheck with chiOutlierR,
    // then updateVisualTrack with visualR where everything passed: one launch when the shape runs on the register-resident kernel
    // (mode 3), otherwise a gate launch and an update launch.
    // knob ekf_stream_gate = 1 (experiment): the streaming gate kernel (two filters per CU) for everybody, then the
    // register-resident update where the gate passed. Measured at 1024 filters (r02): a rejected track costs 0.110 ms instead of the
    // fused launch's 0.130, an accepted one 0.110 + 0.21 instead of 0.23.
    hv::UpdateRequest gate = hv::gate_request(rows, e->n, e->visit.H, e->visit.v, r_gate * r_gate * ns, chi2_dev, gate_status_dev, e->visit.active);
    gate.nr_rec_dev = nr_rec;
    hv::UpdateRequest upd = hv::inlier_update_request(rows, e->n, e->visit.H, e->visit.v, r_update * r_update * ns, e->visit.active, gate_status_dev);
    upd.success_counter_dev = success_counter_dev; upd.nr_rec_dev = nr_rec;
    if (c->knob.ekf_stream_gate == 1 && !nr_rec) {
        bool done = false;
        hv::GateStreamRequest g;
        g.nr = rows; g.l = e->n; g.H_dev = e->visit.H; g.v_dev = e->visit.v; g.rd = r_gate * r_gate * ns; g.chi2_dev = chi2_dev; g.status_dev = gate_status_dev;
        g.active_dev = e->visit.active; g.success_counter_dev = success_counter_dev; g.max_successful = max_successful; g.done = &done;
        rc = hv::ekf_launch_gate_stream(e, g);
        if (rc != HV_OK) return rc;
        if (done) return hv::ekf_launch_update(e, upd);
    }
    bool fused = false;
    hv::UpdateRequest both = gate;                         // mode 3: the gate's request + the update's R, counter and normalisation
    both.mode = 3; both.normalize_all = 1; both.success_counter_dev = success_counter_dev; both.rd1 = r_update * r_update * ns; both.two_r_done = &fused;
    rc = hv::ekf_launch_update(e, both);
    if (rc != HV_OK || fused) return rc;
    rc = hv::ekf_launch_update(e, gate);
    if (rc != HV_OK) return rc;
    return hv::ekf_launch_update(e, upd);
}

int hv_ekf_visual_track_dev(hv_ekf *h, const hv_vu_params *p, int np, const int *idx, const double *feat, const double *vel,
                            const double *y, double r_gate, double r_update, int *status_dev, int *gate_status_dev,
                            double *chi2_dev, double *pf_dev)
{
    return visual_track_dev_impl(h, p, np, idx, feat, vel, y, r_gate, r_update, status_dev, gate_status_dev, chi2_dev, pf_dev, nullptr, 0);
}

int hv_ekf_visual_track_limited_dev(hv_ekf *h, const hv_vu_params *p, int np, const int *idx, const double *feat, const double *vel,
                                    const double *y, double r_gate, double r_update, int *status_dev, int *gate_status_dev,
                                    double *chi2_dev, double *pf_dev, int *success_counter_dev, int max_successful)
{
    if (!success_counter_dev) return HV_ERR_INVALID;
    // maxSuccessfulVisualUpdates <= 0 is the reference's "no limit" (backend.cpp:1233), as in the frame entry points (r03 advisor)
    if (max_successful <= 0) max_successful = INT_MAX;
    return visual_track_dev_impl(h, p, np, idx, feat, vel, y, r_gate, r_update, status_dev, gate_status_dev, chi2_dev, pf_dev,
                                 success_counter_dev, max_successful);
}


static int visual_frame_dev_impl(hv_ekf *h, const hv_vu_params *p, int n_tracks, int np, const int *np_rec_dev, const int *idx,
                                 const double *feat, const double *vel,
                            const double *y, double r_gate, double r_update, int *status_dev, int *gate_status_dev, double *chi2_dev,
                            double *pf_dev, int *success_counter_dev, int max_successful)
{
    if (!h || n_tracks < 0 || !success_counter_dev) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    // maxSuccessfulVisualUpdates <= 0 is the reference's "no limit" (backend.cpp:1233: the test is `> 0 && count >= max`): every track
    // is visited, which a quota of n_tracks expresses exactly (r02 advisor)
    if (max_successful <= 0 || max_successful > n_tracks) max_successful = n_tracks > 0 ? n_tracks : 1;
    const size_t B = (size_t)e->batch, nt = (size_t)np * (p && p->useStereo ? 2 : 1);
    HV_HIP(c, hipMemsetAsync(success_counter_dev, 0, sizeof(int) * B, c->stream));          // updateSuccessCount = 0 (backend.cpp:1017)
    // adaptive outlier thresholds (backend.cpp:994-996,1192-1193): every filter starts the frame at the base thresholds; a rejected
    // track multiplies its filter's thresholds for the tracks behind it. Kept per filter on the device, reset here.
    const bool adaptive = p && p->trackOutlierThresholdGrowthFactor != 1.0;
    struct ScaleScope { Ekf *e; ~ScaleScope() { e->gate.on = false; } } scale_scope{e};
    if (adaptive) {
        if (const int rc_gs = e->gate.ensure(*e)) return rc_gs;
        hipLaunchKernelGGL(hv::fill_doubles_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c->stream, e->gate.scale, (int)B, 1.0);
        HV_HIP(c, hipGetLastError());
        e->gate.on = true;
    }
    // Few sequences (one, for the reference's `main`): the frame is latency bound -- 20 dependent visits of a ~26 us prepare and a
    // ~34 us gate. While the GPU has idle CUs the loop is run SPECULATIVELY instead: a pass prepares and gates
    // EVERY pending track of a filter against the current (m, P) in parallel, applies the first inlier in visit order, and only the
    // tracks behind it are re-examined: <= min(max_successful, n_tracks) + 1 passes, the same statuses and the same filter as the
    // sequential loop (tracks in front of the first inlier saw the state they would have seen anyway).
    const int rows = 2 * (int)nt;
    // Long tracks (49 .. 84 rows; ragged frames whose longest track is that long: the reference's default stereo configuration, SURVEY
    // app. B) -- r04, VERDICT r03 item 6: the same speculative loop with the long build of the fused prepare + gate launch serving EVERY
    // pending record of whatever length (grid (filters, tracks), one 158 KB workgroup per CU while the chip is idle), and the first
    // pending inlier applied by the two block-update launches of the long class: a record of at most 48 rows whole by the first of them,
    // a longer one block by block (UpdateArgs::half_auto; sel_io hands the chosen track from the first launch to the second).
    // <= quota + 1 passes of three launches instead of n_tracks visits of four.
    if (!c->knob.ekf_no_speculation && !adaptive && n_tracks >= 2 && B * (size_t)n_tracks <= (size_t)c->num_cus && rows > 48 && p && idx && feat && vel && y &&
        c->knob.ekf_spec_split == 0 && c->knob.ekf_spec_mode != 3 && c->knob.ekf_long_fused != 0 && visit_shape(e, np, p->useStereo != 0, p->useLinearTriangulation != 0).long_ok) {
        const size_t rec = B * (size_t)n_tracks;
        if (const int rc_sp = e->spec.ensure(*e, rec, rows)) return rc_sp;
        if (const int rc_dm = e->longc.ensure_dm(*e, c->stream)) return rc_dm;
        HV_HIP(c, hipMemsetAsync(e->spec.cursor, 0, sizeof(int) * B, c->stream));
        HV_HIP(c, hipMemsetAsync(e->spec.cursor2, 0xFF, sizeof(int) * B, c->stream));                // sel_io: -1
        HV_HIP(c, hipMemsetAsync(e->spec.epoch, 0xFF, sizeof(int) * rec, c->stream));               // -1: nothing prepared yet
        hv::VuPrepareArgs a;
        int rc = vu_fill_args(e, p, np, idx, feat, vel, y, a);
        if (rc != HV_OK) return rc;
        const double ns = e->noise_scale;
        const int ncam = a.stereo ? 2 : 1;
        const int *nr_rec = vu_fill_spec(e, a, n_tracks, np_rec_dev, pf_dev, status_dev, gate_status_dev, success_counter_dev, max_successful);
        vu_fill_fused(e, a, 3, e->spec.H, e->spec.acol, np, r_gate * r_gate * ns, chi2_dev);
        // (rows per launch: a whole short record of up to 48 rows, or the longer block -- 2 ceil(rows / 4) rows, the first camera's --
        //  of a long one; 48 for everything visit_shape admits today, rows <= 96)
        hv::UpdateRequest u1 = spec_apply_request(e, std::max(48, 2 * ((rows + 3) / 4)), r_update * r_update * ns, n_tracks, gate_status_dev, success_counter_dev, max_successful, nr_rec);
        u1.nr_stride = rows;
        u1.compact = hv::compact_columns(e->spec.acol, a.na_max, ncam);
        u1.compact.nr_full = rows; u1.compact.dm = e->longc.dm; u1.compact.half_auto = 1; u1.compact.sel_io = e->spec.cursor2;
        hv::UpdateRequest u2 = u1;
        u1.compact.half = 1; u1.compact.gate_rw = gate_status_dev; u1.normalize_all = -1;
        u2.compact.half = 2; u2.compact.epoch = e->spec.epoch;
        const int n_pass = (max_successful < n_tracks ? max_successful : n_tracks) + 1;
        for (int pass = 0; pass < n_pass; ++pass) {
            rc = hv::launch_vu_prepare(c, a);
            if (rc == HV_OK) rc = hv::ekf_launch_update(e, u1);
            if (rc == HV_OK) rc = hv::ekf_launch_update(e, u2);
            if (rc != HV_OK) return rc;
        }
        return HV_OK;
    }
    // (a growth factor != 1 makes the threshold of a track depend on the verdicts of the tracks in front of it: no parallel gating)
    if (!c->knob.ekf_no_speculation && !adaptive && n_tracks >= 2 && B * (size_t)n_tracks <= 256 && e->n <= 160 && rows <= 48 && p && idx && feat && vel && y) {
        const size_t rec = B * (size_t)n_tracks;
        if (const int rc_sp = e->spec.ensure(*e, rec, rows)) return rc_sp;
        HV_HIP(c, hipMemsetAsync(e->spec.cursor, 0, sizeof(int) * B, c->stream));
        HV_HIP(c, hipMemsetAsync(e->spec.cursor2, 0, sizeof(int) * B, c->stream));                   // (ping-pong partner: never read uninitialised)
        HV_HIP(c, hipMemsetAsync(e->spec.epoch, 0xFF, sizeof(int) * rec, c->stream));               // -1: nothing prepared yet
        hv::VuPrepareArgs a;
        int rc = vu_fill_args(e, p, np, idx, feat, vel, y, a);
        if (rc != HV_OK) return rc;
        const int *nr_rec = vu_fill_spec(e, a, n_tracks, np_rec_dev, pf_dev, status_dev, gate_status_dev, success_counter_dev, max_successful);
        const double ns = e->noise_scale;
        const int n_pass = (max_successful < n_tracks ? max_successful : n_tracks) + 1;
        // Pass forms (knob ekf_spec_mode; -1 = auto):
        //   2  (r03 default where the fused gate serves the shape) launch A: every pending track prepared AND gated on its active columns
        //      (vu_gate kernel, grid (filters, tracks)); launch B: per filter the first pending inlier is applied, the cursor moves behind it.
        //      No hand-shake between workgroups: what a pass computes does not depend on how the dispatcher places them.
        //   3  (r02) dense prepare, then ONE launch that gates every pending track and lets the first inlier apply itself after a spin-wait
        //      on the decisions in front of it. A wait that times out raises the filter batch's error word (hv_ekf_frame_error).
        //   knob ekf_spec_split = 1: dense prepare + dense gate-all + apply (the first r02 form).
        const int spec_mode = c->knob.ekf_spec_mode;
        const bool split = c->knob.ekf_spec_split != 0;
        // launch B of form 2, and the second launch of the split form: the first pending inlier of every filter is applied
        hv::UpdateRequest apply = spec_apply_request(e, rows, r_update * r_update * ns, n_tracks, gate_status_dev, success_counter_dev, max_successful, nr_rec);
        if (!split && spec_mode != 3 && hv::vu_fused_supported(c, e->n, np, a.stereo, e->batch)) {
            vu_fill_fused(e, a, 1, e->spec.H, e->spec.acol, np, r_gate * r_gate * ns, chi2_dev);
            apply.compact = hv::compact_columns(e->spec.acol, a.na_max, a.stereo ? 2 : 1);
            for (int pass = 0; pass < n_pass; ++pass) {
                rc = hv::launch_vu_prepare(c, a);
                if (rc == HV_OK) rc = hv::ekf_launch_update(e, apply);
                if (rc != HV_OK) return rc;
            }
            return HV_OK;
        }
        if (a.rmse_thr >= 0.0) return HV_ERR_UNSUPPORTED;             // (the dense pass forms have no RMSE test)
        if (!split) HV_HIP(c, hipMemsetAsync(e->spec.pub, 0, sizeof(int) * rec, c->stream));
        int *cur = e->spec.cursor, *nxt = e->spec.cursor2;
        hv::UpdateRequest gate = hv::gate_request(rows, e->n, e->spec.H, e->spec.v, r_gate * r_gate * ns, chi2_dev, gate_status_dev, e->spec.active);
        gate.nr_rec_dev = nr_rec;
        for (int pass = 0; pass < n_pass; ++pass) {
            a.cursor = cur;
            rc = hv::launch_vu_prepare(c, a);
            if (rc != HV_OK) return rc;
            if (!split) {
                bool fused = false;
                hv::UpdateRequest both = gate;                        // form 3: gate + hand-shake + apply, the cursor ping-pongs
                both.mode = 3; both.normalize_all = 1; both.rd1 = r_update * r_update * ns; both.two_r_done = &fused;
                hv::set_spec_pass(both, 3, n_tracks, cur, success_counter_dev, max_successful);
                both.cursor_out_dev = nxt; both.pub_dev = e->spec.pub; both.pass_id = pass + 1;
                rc = hv::ekf_launch_update(e, both);
                if (rc != HV_OK) return rc;
                if (fused) { int *sw = cur; cur = nxt; nxt = sw; continue; }
                // (mode 3 not available for this shape: the two launches below, on the same cursor)
            }
            hv::UpdateRequest gate_all = gate;
            hv::set_spec_pass(gate_all, 1, n_tracks, cur, success_counter_dev, max_successful);
            rc = hv::ekf_launch_update(e, gate_all);
            if (rc != HV_OK) return rc;
            apply.cursor_dev = cur;
            rc = hv::ekf_launch_update(e, apply);
            if (rc != HV_OK) return rc;
        }
        return HV_OK;
    }
    HV_HIP(c, hipMemsetAsync(e->fixed.visit_counts, 0, 4 * sizeof(int) * Ekf::VISIT_SLOTS, c->stream));
    // ragged visits with two length classes: the short class's fused launches take their records longest track first (one sort per frame)
    e->visit_order_ok = false;
    // (many filters only: below one workgroup per CU nothing queues, and the sort, the fork and the join are pure launch overhead --
    //  a single sequence went from 1.14 to 1.51 ms per frame with them)
    if (p && np_rec_dev && c->knob.ekf_visit_order != 0 && n_tracks >= 1 && n_tracks <= Ekf::VISIT_SLOTS && (B > (size_t)c->num_cus || c->knob.ekf_visit_order == 2)) {
        // (only where the visits really run as two length classes: 12 stereo poses = 48 rows still ride the short class -- r03 advisor)
        const hv::VisitShape shape = visit_shape(e, np, p->useStereo != 0, p->useLinearTriangulation != 0);
        if (shape.two_class) {
            const int rc = hv::launch_visit_order(c, n_tracks, B, np_rec_dev, 2, shape.np_short, np, e->fixed.visit_order, e->fixed.visit_long, e->fixed.visit_long_count);
            if (rc != HV_OK) return rc;
            e->visit_order_ok = true;
        }
    }
    for (int k = 0; k < n_tracks; ++k) {
        e->visit_slot = k;
        const int rc = visual_track_dev_impl(h, p, np, idx + (size_t)k * B * np, feat + (size_t)k * B * nt * 2, vel + (size_t)k * B * nt * 2,
                                             y + (size_t)k * B * nt * 2, r_gate, r_update, status_dev + (size_t)k * B * 2,
                                             gate_status_dev + (size_t)k * B, chi2_dev ? chi2_dev + (size_t)k * B : nullptr,
                                             pf_dev ? pf_dev + (size_t)k * B * 3 : nullptr, success_counter_dev, max_successful,
                                             np_rec_dev ? np_rec_dev + (size_t)k * B : nullptr);
        e->visit_slot = -1;
        if (rc != HV_OK) { e->visit_order_ok = false; return rc; }
    }
    e->visit_order_ok = false;
    return HV_OK;
}

int hv_ekf_visual_frame_dev(hv_ekf *h, const hv_vu_params *p, int n_tracks, int np, const int *idx, const double *feat, const double *vel,
                            const double *y, double r_gate, double r_update, int *status_dev, int *gate_status_dev, double *chi2_dev,
                            double *pf_dev, int *success_counter_dev, int max_successful)
{
    return visual_frame_dev_impl(h, p, n_tracks, np, nullptr, idx, feat, vel, y, r_gate, r_update, status_dev, gate_status_dev, chi2_dev,
                                 pf_dev, success_counter_dev, max_successful);
}

int hv_ekf_visual_frame_ragged_dev(hv_ekf *h, const hv_vu_params *p, int n_tracks, int np_max, const int *n_poses_dev, const int *idx,
                                   const double *feat, const double *vel, const double *y, double r_gate, double r_update,
                                   int *status_dev, int *gate_status_dev, double *chi2_dev, double *pf_dev, int *success_counter_dev,
                                   int max_successful)
{
    if (!n_poses_dev) return HV_ERR_INVALID;
    return visual_frame_dev_impl(h, p, n_tracks, np_max, n_poses_dev, idx, feat, vel, y, r_gate, r_update, status_dev, gate_status_dev,
                                 chi2_dev, pf_dev, success_counter_dev, max_successful);
}

// Session::trackerVisualUpdate with batchVisualUpdate (or a frame that is not a "full visual update": backend.cpp:1005): see
// ekf_batch_assemble_kernel. <= min(quota, n_tracks) + 1 passes of (prepare + gate of every pending track | assemble | one dense update).
int hv_ekf_visual_frame_batch_dev(hv_ekf *h, const hv_vu_params *p, int n_tracks, int np, const int *np_rec_dev, const int *idx,
                                  const double *feat, const double *vel, const double *y, double r_gate, double r_update,
                                  int *status_dev, int *gate_status_dev, double *chi2_dev, double *pf_dev, int *success_counter_dev,
                                  int max_successful, int max_update_rows)
{
    if (!h || !p || n_tracks < 1 || !success_counter_dev || !status_dev || !gate_status_dev || !idx || !feat || !vel || !y) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    const int ncam = p->useStereo ? 2 : 1, rows = 2 * np * ncam;
    if (max_update_rows <= 0) max_update_rows = e->n;                        // batchVisualUpdateMaxSizeMultiplier 1 (parameter_definitions.c:17)
    if (max_successful <= 0 || max_successful > n_tracks) max_successful = n_tracks;
    // a batch holds at least one whole track (the reference would write past its batch matrix otherwise) and at most stateDim rows (the
    // dense update kernels' limit); the per-filter multiplier of the outlier thresholds would need the tracks of a pass in sequence
    if (max_update_rows < rows || max_update_rows > e->max_rows || n_tracks > 64) return HV_ERR_INVALID;
    if (p->trackOutlierThresholdGrowthFactor != 1.0) return HV_ERR_UNSUPPORTED;
    const size_t B = (size_t)e->batch, rec = B * (size_t)n_tracks;
    if (rec > 8192) return HV_ERR_UNSUPPORTED;                               // (every record's compact Jacobian is resident during a pass)
    const hv::VisitShape shape = visit_shape(e, np, p->useStereo != 0, p->useLinearTriangulation != 0);
    const bool long_build = rows > 48;
    if (long_build ? !(shape.long_ok && c->knob.ekf_long_fused != 0) : !hv::vu_fused_supported(c, e->n, np, p->useStereo != 0, (int)rec)) return HV_ERR_UNSUPPORTED;
    if (const int rc_sp = e->spec.ensure(*e, rec, rows, max_update_rows)) return rc_sp;
    HV_HIP(c, hipMemsetAsync(success_counter_dev, 0, sizeof(int) * B, c->stream));
    HV_HIP(c, hipMemsetAsync(e->spec.cursor, 0, sizeof(int) * B, c->stream));
    HV_HIP(c, hipMemsetAsync(e->spec.epoch, 0xFF, sizeof(int) * rec, c->stream));
    HV_HIP(c, hipMemsetAsync(e->spec.cursor2, 0xFF, sizeof(int) * B, c->stream));               // carry: -1
    hv::VuPrepareArgs a;
    int rc = vu_fill_args(e, p, np, idx, feat, vel, y, a);
    if (rc != HV_OK) return rc;
    const double ns = e->noise_scale;
    const int *nr_rec = vu_fill_spec(e, a, n_tracks, np_rec_dev, pf_dev, status_dev, gate_status_dev, success_counter_dev, max_successful);
    vu_fill_fused(e, a, long_build ? 3 : 1, e->spec.H, e->spec.acol, np, r_gate * r_gate * ns, chi2_dev);
    hv::BatchAssembleArgs g{};
    g.n = e->n; g.n_tracks = n_tracks; g.batch = e->batch; g.max_rows = max_update_rows; g.max_successful = max_successful;
    g.rows_stride = rows; g.na_max = a.na_max; g.ncam = ncam; g.Hc = e->spec.H; g.v = e->spec.v; g.acol = e->spec.acol; g.nr_rec = nr_rec;
    g.active = e->spec.active; g.gate = gate_status_dev; g.cursor = e->spec.cursor; g.success_counter = success_counter_dev; g.carry = e->spec.cursor2;
    g.Hd = e->spec.bH; g.vd = e->spec.bv; g.rows_out = e->spec.brows; g.any_out = e->spec.bany;
    // updateVisualTrack on the stacked batch of every filter that has one (ragged dense update)
    hv::UpdateRequest flush = hv::inlier_update_request(max_update_rows, e->n, e->spec.bH, e->spec.bv, r_update * r_update * ns, e->spec.bany);
    flush.nr_rec_dev = e->spec.brows;
    const int n_pass = max_successful + 1;
    for (int pass = 0; pass < n_pass; ++pass) {
        rc = hv::launch_vu_prepare(c, a);
        if (rc != HV_OK) return rc;
        hipLaunchKernelGGL(hv::ekf_batch_assemble_kernel, dim3(e->batch), dim3(hv::BATCH_THREADS), 0, c->stream, g);
        HV_HIP(c, hipGetLastError());
        rc = hv::ekf_launch_update(e, flush);
        if (rc != HV_OK) return rc;
    }
    return HV_OK;
}

// Staging of the host-pointer track entries (hv::Stage): the eight sections they share, for B records of np poses,
//     idx | status | gate | features | velocities | y | chi2 | pf
// four inputs and four outputs; an entry declares its own sections behind them, then upload() ... download()
namespace {
struct TrackStage : hv::Stage {
    hv::StageSection<int> idx, st, gs;
    hv::StageSection<double> feat, vel, y, chi, pf;
    TrackStage(Ctx *c, size_t B, int np, bool stereo, const int *h_idx, const double *h_feat, const double *h_vel, const double *h_y,
               int *status, int *gate_status, double *chi2, double *h_pf)
        : hv::Stage(c), idx(in(h_idx, B * np)), st(out(status, B * 2)), gs(out(gate_status, B)), feat(in(h_feat, B * np * (stereo ? 4 : 2))),
          vel(in(h_vel, B * np * (stereo ? 4 : 2))), y(in(h_y, B * np * (stereo ? 4 : 2))), chi(out(chi2, B)), pf(out(h_pf, B * 3)) {}
};
}  // namespace

int hv_ekf_visual_track(hv_ekf *h, const hv_vu_params *p, int np, const int *idx, const double *feat, const double *vel,
                        const double *y, double r_gate, double r_update, int *status, int *gate_status, double *chi2, double *pf)
{
    if (!h || !p || !idx || !feat || !vel || !y || !status || !gate_status || np < 2) return HV_ERR_INVALID;
    Ekf *e = &h->e;
    TrackStage t(e->c, (size_t)e->batch, np, p->useStereo != 0, idx, feat, vel, y, status, gate_status, chi2, pf);
    int rc = t.upload();
    if (rc == HV_OK) rc = hv_ekf_visual_track_dev(h, p, np, t.at(t.idx), t.at(t.feat), t.at(t.vel), t.at(t.y), r_gate, r_update, t.at(t.st), t.at(t.gs), t.at(t.chi), t.at(t.pf));
    return rc != HV_OK ? rc : t.download();
}

// batch_rows: 0 = the sequential visit loop (visual_frame_dev_impl); != 0 = the batchVisualUpdate loop with this max_update_rows (< 0: the
// library's default, stateDim)
static int visual_frame_host_impl(hv_ekf *h, const hv_vu_params *p, int n_tracks, int np, const int *n_poses, const int *idx,
                                  const double *feat, const double *vel,
                        const double *y, double r_gate, double r_update, int *status, int *gate_status, double *chi2, double *pf,
                        int *success_count, int max_successful, int batch_rows = 0)
{
    if (!h || !p || !idx || !feat || !vel || !y || !status || !gate_status || np < 2 || n_tracks < 1) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    const size_t B = (size_t)e->batch * n_tracks;
    TrackStage t(c, B, np, p->useStereo != 0, idx, feat, vel, y, status, gate_status, chi2, pf);
    const auto o_cnt = t.out(success_count, (size_t)e->batch);   // own sections: success counts [batch] | pose counts [B]
    const auto o_np = t.in(n_poses, B);
    int rc = t.upload();
    if (rc != HV_OK) return rc;
    rc = batch_rows == 0
        ? visual_frame_dev_impl(h, p, n_tracks, np, t.at_or_null(o_np), t.at(t.idx), t.at(t.feat), t.at(t.vel), t.at(t.y), r_gate, r_update, t.at(t.st), t.at(t.gs), t.at(t.chi),
                                t.at(t.pf), t.at(o_cnt), max_successful)
        : hv_ekf_visual_frame_batch_dev(h, p, n_tracks, np, t.at_or_null(o_np), t.at(t.idx), t.at(t.feat), t.at(t.vel), t.at(t.y), r_gate, r_update, t.at(t.st), t.at(t.gs),
                                        t.at(t.chi), t.at(t.pf), t.at(o_cnt), max_successful, batch_rows < 0 ? 0 : batch_rows);
    if (rc == HV_OK) rc = t.download();
    if (rc != HV_OK) return rc;
    int flags = 0;
    const int rc2 = hv_ekf_frame_error(h, &flags);                // the hand-shake form of the speculative pass never fails silently
    if (rc2 != HV_OK) return rc2;
    return flags ? HV_ERR_TIMEOUT : HV_OK;
}

int hv_ekf_visual_frame(hv_ekf *h, const hv_vu_params *p, int n_tracks, int np, const int *idx, const double *feat, const double *vel,
                        const double *y, double r_gate, double r_update, int *status, int *gate_status, double *chi2, double *pf,
                        int *success_count, int max_successful)
{
    return visual_frame_host_impl(h, p, n_tracks, np, nullptr, idx, feat, vel, y, r_gate, r_update, status, gate_status, chi2, pf,
                                  success_count, max_successful);
}

int hv_ekf_visual_frame_ragged(hv_ekf *h, const hv_vu_params *p, int n_tracks, int np_max, const int *n_poses, const int *idx,
                               const double *feat, const double *vel, const double *y, double r_gate, double r_update, int *status,
                               int *gate_status, double *chi2, double *pf, int *success_count, int max_successful)
{
    if (!n_poses) return HV_ERR_INVALID;
    return visual_frame_host_impl(h, p, n_tracks, np_max, n_poses, idx, feat, vel, y, r_gate, r_update, status, gate_status, chi2, pf,
                                  success_count, max_successful);
}

int hv_ekf_visual_frame_batch(hv_ekf *h, const hv_vu_params *p, int n_tracks, int np_max, const int *n_poses, const int *idx,
                              const double *feat, const double *vel, const double *y, double r_gate, double r_update, int *status,
                              int *gate_status, double *chi2, double *pf, int *success_count, int max_successful, int max_update_rows)
{
    return visual_frame_host_impl(h, p, n_tracks, np_max, n_poses, idx, feat, vel, y, r_gate, r_update, status, gate_status, chi2, pf,
                                  success_count, max_successful, max_update_rows > 0 ? max_update_rows : -1);
}

// host-pointer form of hv_ekf_visual_track_hybrid_dev: one track per filter, arrays [batch]...
int hv_ekf_visual_track_hybrid(hv_ekf *h, const hv_vu_params *p, int np, const int *idx, const double *feat, const double *vel, const double *y,
                               const int *map_update, const int *map_offer, double r_gate, double r_update, int *status, int *gate_status,
                               double *chi2, double *pf)
{
    if (!h || !p || !idx || !feat || !vel || !y || !status || !gate_status || np < 2) return HV_ERR_INVALID;
    Ekf *e = &h->e; Ctx *c = e->c;
    const size_t B = (size_t)e->batch;
    TrackStage t(c, B, np, p->useStereo != 0, idx, feat, vel, y, status, gate_status, chi2, pf);
    const auto o_mu = t.in(map_update, B), o_mo = t.in(map_offer, B);       // own sections: map_update [B] | map_offer [B]
    int rc = t.upload();
    if (rc != HV_OK) return rc;
    rc = hv_ekf_visual_track_hybrid_dev(h, p, np, t.at(t.idx), t.at(t.feat), t.at(t.vel), t.at(t.y), t.at_or_null(o_mu), t.at_or_null(o_mo), r_gate, r_update, t.at(t.st),
                                        t.at(t.gs), t.at(t.chi), t.at(t.pf));
    return rc != HV_OK ? rc : t.download();
}

}  // extern "C"
