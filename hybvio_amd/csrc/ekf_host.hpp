// Host side of the EKF shared by ekf.hip (kernels, their launchers, the one-launch entries) and ekf_visit.hip (track visits, frame
// loops, host-pointer staging): the filter object, the launch requests. Plain C++ and HIP host types, no kernel.
#pragma once
#include "hv_internal.hpp"

namespace hv {

struct Ekf {
    Ctx *c = nullptr;
    hv_ekf_params par{};
    int batch = 0, n = 0, cam = 0, map_dim = 0;
    double noise_scale = 0;
    double *m = nullptr, *P = nullptr, *P1 = nullptr, *m1 = nullptr, *Q = nullptr, *dydx = nullptr, *ws = nullptr;
    double *sH = nullptr, *sv = nullptr, *sr = nullptr, *schi2 = nullptr, *simu = nullptr;   // staging for host-pointer calls
    int *sstatus = nullptr, *sdrop = nullptr;
    unsigned char *sactive = nullptr;
    size_t sH_cap = 0;
    int max_rows = 0;
    // buffers of hv_ekf_visual_track_dev (row f3), sized on first use
    double *vuH = nullptr, *vuv = nullptr, *vupf = nullptr;
    unsigned char *vuactive = nullptr;
    int *vurows = nullptr;                                // ragged batches: per-filter rows of the current visit (written by vu_prepare)
    int *sprows = nullptr;                                // ... and per (track, filter) record of the speculative loop
    int vu_rows = 0;
    // speculative frame loop: per (track, filter) records + per-filter cursor and the update count each record was prepared at
    double *spH = nullptr, *spv = nullptr, *sppf = nullptr;
    unsigned char *spactive = nullptr;
    int *spcursor = nullptr, *spepoch = nullptr;
    int *spcursor2 = nullptr, *sppub = nullptr;           // fused gate + apply passes: second cursor (ping-pong), published decisions
    size_t sp_records = 0; int sp_rows = 0;
    // fused prepare + gate (compact Jacobians live in vuH / spH): the active-column lists of the records
    int *vuacol = nullptr, *spacol = nullptr;
    // long-track classes of a ragged visit (ekf_visit.hip, Visit): own stream, events, Jacobian / residual / active buffers
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;    // fork onto / join of the context's second stream (Ctx::aux_stream) inside a visit
    double *sideH = nullptr, *sidev = nullptr;
    unsigned char *side_active = nullptr;
    int side_rows = 0;
    int *side_acol = nullptr; double *side_dm = nullptr;
    double *tri_rec = nullptr; int tri_stride = 0;        // factor records of vu_tri_kernel (split form of a visit, r06): [batch][tri_stride]
    int *err_dev = nullptr;                               // device error word (UpdateArgs::err)
    double *bH = nullptr, *bv = nullptr; int *brows = nullptr; unsigned char *bany = nullptr; int b_rows = 0;   // batchVisualUpdate: stacked [H; v], rows, flags
    double *gate_scale = nullptr;                         // [batch] per-filter multiplier of the outlier thresholds inside a frame loop (backend.cpp:1192-1193)
    bool gate_scale_on = false;                           // set by the frame loop while its visits run with a growth factor != 1
    int *visit_counts = nullptr, *visit_lists = nullptr;  // compaction lists of a visit: counts {inliers short, long records, inliers long}, lists 3 x [batch]
    // the counts exist once per visit of a frame loop (VISIT_SLOTS x 4 ints, zeroed by ONE memset per frame; visit_slot = the running
    // visit, set by the loop) plus one set for stand-alone visits (zeroed per call): a memset node per visit was 20 more graph nodes
    static constexpr int VISIT_SLOTS = 64;
    int visit_slot = -1;
    int *visit_order = nullptr;                           // [VISIT_SLOTS][batch] launch_visit_order of the running frame loop, valid while visit_order_ok
    int *visit_long = nullptr, *visit_long_count = nullptr;   // ... its long-class lists [VISIT_SLOTS][batch] and their lengths [VISIT_SLOTS]
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

}  // namespace hv

struct hv_ekf { hv::Ekf e; };
