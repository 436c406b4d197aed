// Host side of the EKF shared by the kernel families (ekf_predict.hip, ekf_update.hip, ekf_gate.hip, ekf_augment.hip: kernels, their
// launchers, the one-launch entries), ekf.hip (create / destroy, accessors) and ekf_visit.hip (track visits, frame loops): the filter
// object, the launch requests. Plain C++ and HIP host types, no kernel. The filter owns no staging: its host-pointer entries stage
// through hv::Stage in the arena of its context (hv_stage.hpp), as every other host-pointer entry of the library does.
#pragma once
#include "hv_internal.hpp"

namespace hv {

// The filter object. Its device buffers are grouped by lifetime: each group keeps its capacity beside its buffers and has ONE
// ensure(), called where the group is first needed; a group's once-only members are allocated by its first ensure().
struct Ekf {
    Ctx *c = nullptr;
    hv_ekf_params par{};
    int batch = 0, n = 0, cam = 0, map_dim = 0;
    double noise_scale = 0;
    int max_rows = 0;

    // allocated by hv_ekf_create, never regrown
    struct Fixed {
        DevBuf<double> m, P, P1, m1, Q, dydx, ws;             // state
        DevBuf<int> err_dev;                                  // device error word (UpdateArgs::err)
        DevBuf<int> visit_counts, visit_lists;                // compaction lists of a visit: counts {inliers short, long records, inliers long}, lists 3 x [batch]
        DevBuf<int> visit_order;                              // [VISIT_SLOTS][batch] launch_visit_order of the running frame loop, valid while visit_order_ok
        DevBuf<int> visit_long, visit_long_count;             // ... its long-class lists [VISIT_SLOTS][batch] and their lengths [VISIT_SLOTS]
        int ensure(const Ekf &e)
        {
            const size_t n = e.n, B = e.batch, nn = n * n;
            if (m.alloc(n * B) || P.alloc(nn * B) || P1.alloc(nn * B) || m1.alloc(n * B) || Q.alloc(144 * B) || dydx.alloc(400 * B) ||
                ws.alloc((2 * n + 1) * n * B) || err_dev.alloc(1) ||
                visit_counts.alloc(4 * (VISIT_SLOTS + 1)) || visit_order.alloc(VISIT_SLOTS * B) || visit_long.alloc(VISIT_SLOTS * B) ||
                visit_long_count.alloc(VISIT_SLOTS) || visit_lists.alloc(3 * B)) return HV_ERR_NOMEM;
            return HV_OK;
        }
    } fixed;

    // one track visit (hv_ekf_visual_track_dev, row f3): dense or compact Jacobians and residuals of `cap_rows` rows per filter, regrown
    // when a longer track arrives; once: point, active flags, the compact Jacobians' column lists, per-filter rows of a ragged visit,
    // and the hybrid visit's apply mask (hv_ekf_visual_track_hybrid_dev: the filters whose track still takes updateVisualTrack,
    // written by ekf_hybrid_insert_kernel and read by the update behind it; nothing else uses it)
    struct VisitBufs {
        DevBuf<double> H, v; int cap_rows = 0;
        DevBuf<double> pf; DevBuf<unsigned char> active, apply; DevBuf<int> acol, rec_rows;
        int ensure(const Ekf &e, int rows)
        {
            if (cap_rows >= rows) return HV_OK;
            const size_t n = e.n, B = e.batch;
            cap_rows = 0;
            if (const int rc = grow_buffers(e.c, {e.c->stream}, {{H, rows * n * B}, {v, rows * B}})) return rc;
            if (pf.alloc_once(3 * B) || active.alloc_once(B) || apply.alloc_once(B) || acol.alloc_once(n * B) || rec_rows.alloc_once(B)) return HV_ERR_NOMEM;
            cap_rows = rows;
            return HV_OK;
        }
    } visit;

    // long-track class of a ragged visit (ekf_visit.hip, Visit): compact Jacobians and residuals of `cap_rows` rows; once: active flags,
    // column lists, block 1's mean step `dm` (zeroed when allocated: r03 advisor, never read uninitialised), and the events of the
    // fork onto / join of the context's second stream (Ctx::aux_stream) inside a visit
    struct LongBufs {
        DevBuf<double> H, v; int cap_rows = 0;
        DevBuf<unsigned char> active; DevBuf<int> acol; DevBuf<double> dm;
        hipEvent_t ev_fork = nullptr, ev_join = nullptr;
        int ensure(const Ekf &e, int rows, hipStream_t main_stream)
        {
            Ctx *c = e.c;
            if (!ev_fork) {
                HV_HIP(c, hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
                HV_HIP(c, hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
            }
            if (cap_rows >= rows) return HV_OK;
            const size_t n = e.n, B = e.batch;
            cap_rows = 0;
            if (const int rc = grow_buffers(c, {main_stream, c->aux_stream}, {{H, rows * n * B}, {v, rows * B}})) return rc;
            if (active.alloc_once(B) || acol.alloc_once(n * B)) return HV_ERR_NOMEM;
            if (const int rc = ensure_dm(e, main_stream)) return rc;
            cap_rows = rows;
            return HV_OK;
        }
        // (the speculative loop applies long records through `dm` without the rest of the group)
        int ensure_dm(const Ekf &e, hipStream_t stream)
        {
            if (dm) return HV_OK;
            const size_t count = (size_t)e.n * e.batch;
            if (dm.alloc(count)) return HV_ERR_NOMEM;
            HV_HIP(e.c, hipMemsetAsync(dm, 0, sizeof(double) * count, stream));
            return HV_OK;
        }
    } longc;

    // factor records of vu_tri_kernel (split form of a visit, r06): [batch][stride]
    struct TriBufs {
        DevBuf<double> rec; int stride = 0;
        int ensure(const Ekf &e, int want, hipStream_t main_stream)
        {
            if (stride >= want) return HV_OK;
            Ctx *c = e.c;
            stride = 0;
            const GrowSlot g{rec, (size_t)want * e.batch};
            const int rc = c->aux_stream ? grow_buffers(c, {main_stream, c->aux_stream}, {g}) : grow_buffers(c, {main_stream}, {g});
            if (rc == HV_OK) stride = want;
            return rc;
        }
    } tri;

    // speculative frame loops and the batch loop: one record per (track, filter) -- compact or dense Jacobian, residual, point, flags,
    // column list, rows, the update count it was prepared at, published decision -- plus the per-filter cursors (cursor2: ping-pong);
    // grown on first use of a shape and never shrunk in either dimension (r04 advisor: reallocating to exactly (rec, rows) let
    // alternating shapes -- a short and a long frame, the speculative and the batch loop -- free and allocate on every call, which a
    // stream capture cannot hold). The batch loop (batch_rows > 0) adds batchVisualUpdate's stacked [H; v], rows and flags per filter.
    struct SpecBufs {
        DevBuf<double> H, v, pf; DevBuf<unsigned char> active; DevBuf<int> cursor, epoch, cursor2, pub, acol, rec_rows;
        size_t cap_records = 0; int cap_rows = 0;
        DevBuf<double> bH, bv; DevBuf<int> brows; DevBuf<unsigned char> bany; int b_cap_rows = 0;
        int ensure(const Ekf &e, size_t records, int rows, int batch_rows = 0)
        {
            Ctx *c = e.c;
            const size_t n = e.n, B = e.batch;
            if (cap_records < records || cap_rows < rows) {
                const size_t rec = records > cap_records ? records : cap_records;
                const size_t r = rows > cap_rows ? rows : cap_rows;
                cap_records = 0;
                if (const int rc = grow_buffers(c, {c->stream}, {{H, rec * r * n}, {v, rec * r}, {pf, rec * 3}, {active, rec}, {cursor, B}, {epoch, rec},
                                                                 {cursor2, B}, {pub, rec}, {acol, rec * n}, {rec_rows, rec}})) return rc;
                cap_records = rec; cap_rows = (int)r;
            }
            if (b_cap_rows < batch_rows) {
                b_cap_rows = 0;
                if (const int rc = grow_buffers(c, {c->stream}, {{bH, B * batch_rows * n}, {bv, B * batch_rows}, {brows, B}, {bany, B}})) return rc;
                b_cap_rows = batch_rows;
            }
            return HV_OK;
        }
    } spec;

    // [batch] per-filter multiplier of the outlier thresholds inside a frame loop (backend.cpp:1192-1193)
    struct GateScale {
        DevBuf<double> scale;
        bool on = false;                                      // set by the frame loop while its visits run with a growth factor != 1
        int ensure(const Ekf &e) { return scale.alloc_once(e.batch); }
    } gate;

    // the counts exist once per visit of a frame loop (VISIT_SLOTS x 4 ints, zeroed by ONE memset per frame; visit_slot = the running
    // visit, set by the loop) plus one set for stand-alone visits (zeroed per call): a memset node per visit was 20 more graph nodes
    static constexpr int VISIT_SLOTS = 64;
    int visit_slot = -1;
    bool visit_order_ok = false;
};

// shapes of a track visit: the longest track the short class's fused two-per-CU kernels serve, whether tracks of np poses take the
// long-class launches (49 .. 96 rows), and whether a ragged visit of up to np poses runs as TWO length classes
struct VisitShape { int ncam, np_short, rows; bool long_ok, two_class; };

// compact-H description of an update launch (null acol: dense H of l columns); half / nr_full / dm: block update of a long
// track (UpdateArgs::half)
struct CompactH { const int *acol = nullptr; int na_max = 0, ncam = 1; int half = 0, nr_full = 0; double *dm = nullptr; const int *rec_count = nullptr, *rec_list = nullptr; int *gate_rw = nullptr;
                  int half_auto = 0; int *sel_io = nullptr; int *epoch = nullptr; };

// an update launch prepared but not issued (UpdateRequest::defer); it holds the kernels' argument struct, so it is defined beside them
struct UpdateLaunch;

// one launch of the update kernels (ekf_launch_update); the fields mean what their namesakes in UpdateArgs mean
struct UpdateRequest {
    int nr = 0, l = 0;                                     // rows of the longest record this launch processes, columns of a dense H
    const double *H_dev = nullptr, *v_dev = nullptr, *rdiag_dev = nullptr;
    double rd0 = 0.0, rd1 = 0.0;                           // R = rd0 I (generic: rdiag_dev); mode 3: gate with rd0, update with rd1
    int mode = 0, generic = 0, normalize_all = 0;
    double *chi2_dev = nullptr;
    int *status_dev = nullptr, *success_counter_dev = nullptr;
    const unsigned char *active_dev = nullptr;
    const int *require_inlier_dev = nullptr, *gate_in_dev = nullptr, *nr_rec_dev = nullptr;
    bool *two_r_done = nullptr;                            // mode 3: false = the shape has no one-launch form, nothing was launched
    int spec = 0, n_tracks = 0, max_successful = 0, pass_id = 0;
    int *cursor_dev = nullptr, *cursor_out_dev = nullptr, *pub_dev = nullptr;
    CompactH compact;
    // ragged launches that serve one length class: rows of the LONGEST record of the batch = the record stride of H and v (0: nr);
    // nr is then the most rows this launch processes (kernel variant, LDS carve), longer records are skipped by their `active` flag
    int nr_stride = 0;
    UpdateLaunch *defer = nullptr;                         // non-null: validate and prepare only
};

// visualTrackOutlierCheck alone: chi2 and status of every active filter (no flags: of every filter), R = rd I
inline UpdateRequest gate_request(int nr, int l, const double *H_dev, const double *v_dev, double rd, double *chi2_dev, int *status_dev,
                                  const unsigned char *active_dev = nullptr)
{
    UpdateRequest rq;
    rq.nr = nr; rq.l = l; rq.H_dev = H_dev; rq.v_dev = v_dev; rq.rd0 = rd; rq.chi2_dev = chi2_dev; rq.status_dev = status_dev; rq.active_dev = active_dev;
    return rq;
}
// updateVisualTrack (R = rd I, quaternions normalised) where the filter is active and -- with require_inlier_dev -- its gate said inlier
inline UpdateRequest inlier_update_request(int nr, int l, const double *H_dev, const double *v_dev, double rd, const unsigned char *active_dev,
                                           const int *require_inlier_dev = nullptr)
{
    UpdateRequest rq;
    rq.nr = nr; rq.l = l; rq.H_dev = H_dev; rq.v_dev = v_dev; rq.rd0 = rd; rq.mode = 1; rq.normalize_all = 1;
    rq.active_dev = active_dev; rq.require_inlier_dev = require_inlier_dev;
    return rq;
}
// turns a request into a pass of the speculative frame loop over the records [n_tracks][batch]
inline void set_spec_pass(UpdateRequest &rq, int spec, int n_tracks, int *cursor_dev, int *success_counter_dev, int max_successful)
{
    rq.spec = spec; rq.n_tracks = n_tracks; rq.cursor_dev = cursor_dev; rq.success_counter_dev = success_counter_dev; rq.max_successful = max_successful;
}
// the compact Jacobian of a fused prepare launch: column lists acol [records][na_max]; rec_count / rec_list: the launch's own records
inline CompactH compact_columns(const int *acol, int na_max, int ncam, const int *rec_count = nullptr, const int *rec_list = nullptr)
{
    CompactH h;
    h.acol = acol; h.na_max = na_max; h.ncam = ncam; h.rec_count = rec_count; h.rec_list = rec_list;
    return h;
}

// ekf_sparse_gate_kernel over the compact records of a prepare launch (np = poses of the longest record)
struct SparseGateRequest {
    int np = 0, ncam = 1;
    const double *Hc_dev = nullptr, *v_dev = nullptr;
    const int *acol_dev = nullptr, *nr_rec_dev = nullptr;
    const unsigned char *active_dev = nullptr;
    double rd = 0.0, *chi2_dev = nullptr;
    int *status_dev = nullptr;
    const int *rec_count = nullptr, *rec_list = nullptr;   // the launch's own records (null: every filter)
    int *inl_count = nullptr, *inl_list = nullptr;         // appended: records whose gate said inlier
    hipStream_t stream = nullptr;                          // null = the context's
};

// streaming dense gate, two filters per CU (ekf_gate_stream_kernel); *done = false: not a shape it serves, the caller keeps its other route
struct GateStreamRequest {
    int nr = 0, l = 0, max_successful = 0;
    const double *H_dev = nullptr, *v_dev = nullptr;
    double rd = 0.0, *chi2_dev = nullptr;
    int *status_dev = nullptr;
    const unsigned char *active_dev = nullptr;
    const int *success_counter_dev = nullptr;
    bool *done = nullptr;
};

int ekf_launch_update(Ekf *e, const UpdateRequest &rq);
// `us` beside `b1`, then what did not fit on the chip beside `b2`, as two shared grids (ekf_update_dual_kernel); *done = false when the
// shapes do not allow it: nothing was launched and the caller issues the three one after the other
int ekf_launch_update_paired(Ekf *e, const UpdateRequest &us, const UpdateRequest &b1, const UpdateRequest &b2, bool *done);
int ekf_launch_gate_stream(Ekf *e, const GateStreamRequest &rq);
int ekf_launch_sparse_gate(Ekf *e, const SparseGateRequest &rq);

#ifdef HV_EKF_PHASE_STAMPS
// the 16 stamps of one family file's own array (ekf_device.hpp), merged by hv_debug_ekf_phase_stamps
hipError_t ekf_predict_phase_stamps(long long *out16);
hipError_t ekf_update_phase_stamps(long long *out16);
hipError_t ekf_gate_phase_stamps(long long *out16);
#endif

}  // namespace hv

struct hv_ekf { hv::Ekf e; };
