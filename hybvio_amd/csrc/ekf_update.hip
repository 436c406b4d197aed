// EKF visual update / chi2 gate for a batch of independent filters, one workgroup per filter (the family map is in ekf.hip): the
// update kernels and their launchers, nothing else.
//   * visual update / chi2 gate (ekf_update_kernel): S = H P H' + R is factored and both triangular
//     solves are done in ONE blocked Cholesky pass over the tall matrix T = [S ; v' ; (HP)'] in LDS
//     (16-column blocks: MFMA panel / trailing updates, the 16 x 16 diagonal factor and its inverse
//     in the registers of one wavefront), after which chi2 = ns z'z, m += Y'z, P -= Y'Y with
//     Y = L^-1 HP. K is never formed; the reference forms K = (S^-1 HP)' with a pivoted LDLT and
//     P -= K HP, algebraically identical (parity 1e-9 relative per call, measured ~1e-13). At the
//     reference's sizes (n = 160, <= 47 rows) H is staged in LDS too and every wavefront owns whole
//     16-column blocks of P: the tiles it streams from HBM as MFMA operands of H P are already in the
//     accumulator layout of P -= Y'Y and stay in registers until then, so P is read once per update.
#include "ekf_device.hpp"
#include "ekf_host.hpp"

// The library is built with -ffp-contract=off for the tracker's bit-exact binary32 sequence; the
// EKF is judged against a relative tolerance, and a fused multiply-add is one rounding fewer and
// half the f64 instructions of its dependency chains.
#pragma clang fp contract(fast)

namespace hv {

namespace {

// ---------------------------------------------------------------------------------------------
// update / gate (ekf.cpp:57-82, 760-844)
// ---------------------------------------------------------------------------------------------
struct UpdateArgs {
    int n, nr, l, R, Rs;              // R = nr + n + 1 rows of the tall matrix; Rs = its column stride
    int mode;                         // 0 gate only, 1 update, 2 update only if the chi2 gate passes
    int generic;                      // residual = y - H m[0:l] (ekf.cpp:76-79) instead of the given v
    int normalize_all, use_lds, map_dim;
    double *m, *P;
    const double *H, *v;              // per filter: nr*l column-major, nr
    const double *rdiag;              // per filter diagonal of R (already scaled), or null -> rd0
    double rd0, noise_scale;
    double rd1;                       // mode 3 only: R of the update (rd0 is then the R of the gate)
    double *ws;                       // per filter R*nr doubles (used when the tall matrix exceeds LDS)
    double *chi2; int *status;        // optional outputs
    const unsigned char *active;      // optional per-filter enable
    const int *require_inlier;        // optional per-filter gate result of an earlier launch: run only where it is 0 (INLIER)
    int *success_counter;             // optional per-filter count of applied visual updates (updateSuccessCount, backend.cpp:1183)
    // speculative frame loop (small batches, hv_ekf_visual_frame_dev): inputs / outputs are [n_tracks][batch] records
    //   spec 1: grid (batch, n_tracks), chi2 gate of EVERY pending track (index >= cursor[filter]) against the current (m, P)
    //   spec 2: grid (batch): the first pending track whose gate said INLIER is applied (mode 1), cursor moves behind it
    //   spec 3: spec 1 and spec 2 in ONE launch (mode 3, grid (batch, n_tracks)): every pending track is gated; an inlier then waits
    //           for the gate results of the pending tracks in front of it (they belong to workgroups with a smaller linear index:
    //           dispatched earlier, so the wait cannot deadlock) and, if none of them is an inlier, carries on into the update with
    //           the H P it already holds. The workgroup of the last track closes the pass when nobody applied anything.
    int spec, n_tracks, max_successful;
    int *cursor;                      // [batch] first track of the filter that is not final yet
    const int *gate_in;               // spec 2: [n_tracks][batch] gate results of spec 1 (a.status stays free for this launch's own output)
    const int *nr_rec;                // ragged batches: rows of every record (<= nr, which is then the record stride of H and v; 0: none)
    int *cursor_out;                  // spec 3: the cursor after this pass (ping-pong: late workgroups still read the old one)
    int *pub;                         // spec 3: [n_tracks][batch] published gate decisions, pass_id * 4 + {1 not applicable, 2 inlier}
    int pass_id;                      // spec 3: > 0, distinct per pass of a frame (pub is zeroed per frame)
    int *err;                         // spec 3: device error word of the filter batch (bit 0: a hand-shake wait timed out)
    // compact Jacobian written by the fused prepare + gate kernel (VuPrepareArgs::fused): column u of a record is state column
    // acol[u]; the record holds na = 7 * (rows / (2 ncam)) + 1 columns with the record's row count as leading dimension. MODE 2 only.
    const int *acol;                  // [records][na_max] or null (dense H)
    int na_max, ncam;
    size_t h_stride;                  // doubles between the H records
    int v_stride;                     // doubles between the v records (= nr unless the launch serves one length class of a longer-strided batch)
    // Long tracks (49 .. 96 rows: 13 .. 21 stereo poses) as TWO sequential block updates of at most 48 rows each, which is the same
    // posterior (the blocks' measurement noises are independent: R = r^2 I, ekf.cpp:771) and keeps every update on the P-resident MODE 2
    // kernel: half 1 = the first h1 = 2 ceil(rows / 4) rows (the first camera's), half 2 = the rest (the second camera's) with its
    // innovation corrected by the first block's mean step, v2 - H2 dm1. Half 1 leaves dm1 in dm_out and skips the quaternion
    // normalisation; half 2 reads it (dm_in) and normalises. 0 = the whole record in one launch. Compact H, MODE 2 only.
    int half, nr_full;                // nr_full: rows of the whole record when neither nr_rec nor nr says so (uniform long tracks)
    double *dm_out; const double *dm_in;   // [batch][n]
    // half 1 only: the visit's gate statuses. A block 1 that meets a non-positive pivot applies nothing and turns its record's status
    // into CHI2 -- what every other mode reports for a broken factorisation --, so that block 2 (require_inlier) skips the record
    // instead of applying half an update on a stale dm_in (r03 advisor)
    int *gate_rw;
    // speculative frame loop over LONG records (spec 2 with half 1 / 2, r04): the record a filter applies is chosen by the scan of the
    // half-1 launch; `half_auto` makes the block split a per-record decision -- a record of at most 48 rows is applied whole by the
    // half-1 launch (normalisation, success count and cursor included) and skipped by the half-2 launch, a longer one takes both --,
    // and sel_io [batch] carries the chosen track of a long record (-1: none) from the half-1 launch to the half-2 launch, which
    // must not scan again: the first launch may have moved the cursor or turned the record's gate status into CHI2
    int half_auto; int *sel_io;
    // half_auto: the epochs of the frame's records, [n_tracks][batch] (VuPrepareArgs::epoch). A long record whose block 1 was applied and
    // whose block 2 then meets a non-positive pivot leaves (m, P) changed without a counted success: the filter's pending records are
    // marked "never prepared" (-1) so that the next pass prepares them against the state as it is now (r04 advisor)
    int *epoch;
    int batch;
    const int *rec_count, *rec_list;  // compaction list (VuPrepareArgs): workgroup i updates filter rec_list[i], i < *rec_count; the others exit
};

// spec 3 hand-shake between the workgroups of one filter (agent scope: they run on different CUs)
__device__ __forceinline__ void spec_publish(const UpdateArgs &a, int rec, int code)
{
    __hip_atomic_store(a.pub + rec, a.pass_id * 4 + code, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
// decision of record `rec` in this pass; bounded spin (0.2 s): a decision that never arrives is reported as -1
__device__ __forceinline__ int spec_wait(const UpdateArgs &a, int rec)
{
    for (int spin = 0; spin < (1 << 20); ++spin) {
        const int v = __hip_atomic_load(a.pub + rec, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if ((v >> 2) == a.pass_id) return v & 3;
        __builtin_amdgcn_s_sleep(8);
    }
    // never silently: the frame's result is then NOT the sequential loop's (a.err is read by hv_ekf_frame_error / the host-pointer entry points)
    if (a.err) atomicOr(a.err, 1);
    return -1;
}
// thread 0 of the workgroup of the LAST track, when that workgroup applies nothing: if no pending track of the filter was an
// inlier, nobody else moves the cursor -- every pending status is final (or the pass did not run: quota used up)
__device__ __forceinline__ void spec_close(const UpdateArgs &a, int b, int c0, bool pass_ran)
{
    bool any = false;
    for (int jj = c0; jj < a.n_tracks - 1 && !any; ++jj) any = spec_wait(a, jj * (int)gridDim.x + b) == 2;
    if (!any) a.cursor_out[b] = pass_ran ? a.n_tracks : c0;
}

constexpr int UPD_THREADS = 512;   // 8 waves = 2 per SIMD: 256 VGPRs each (whole column blocks of P stay in registers)

// MODE 0: T in the global workspace (tall matrix larger than LDS)
// MODE 1: T in LDS, H streamed from L2
// MODE 2: T and H in LDS (n <= 160, nr <= 48): K-split products, P read from HBM exactly once
// TI (MODE 2 only): 16-row tiles of H, nr <= 16 TI: a compile-time count keeps the MFMA loops free of
// branches (a uniform branch per tile made hipcc wait for each LDS operand right before its MFMA).
// AUTO: the half_auto form of the speculative loop over long records (its own kernel: the other instantiations keep their registers)
template <int MODE, int TI, bool AUTO = false>
__device__ __forceinline__ void ekf_update_body(const UpdateArgs &a, const int b_in /* filter: blockIdx.x, or an entry of a compaction list */)
{
    // (a list entry is a per-lane load: on the scalar unit the filter's base addresses are uniform and its gathers become scalar base +
    //  32-bit lane offset -- one VGPR and one VALU instruction per request instead of a 64-bit multiply-add pair)
    const int b = __builtin_amdgcn_readfirstlane(b_in);
    constexpr bool USE_LDS = MODE >= 1;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    int e = b;                                             // record of this workgroup's H, v, active, chi2, status
    int sel = -1;
    if (a.spec == 1) {
        const int j = blockIdx.y;
        if (j < a.cursor[b] || a.success_counter[b] >= a.max_successful) return;
        e = j * (int)gridDim.x + b;
    } else if (AUTO && a.spec == 2 && a.half == 2) {
        // second block of the long record the half-1 launch chose for this filter (if any)
        sel = a.sel_io[b];
        if (sel < 0) return;
        e = sel * (int)gridDim.x + b;
        if (a.gate_in[e] != 0) {                           // block 1 met a non-positive pivot (status CHI2 now): nothing applied, the track is final
            if (threadIdx.x == 0) a.cursor[b] = sel + 1;
            return;
        }
    } else if (a.spec == 2) {
        // every thread runs the same short scan (uniform): the first pending track that passed its gate
        const int c0 = a.cursor[b];
        if (AUTO && threadIdx.x == 0) a.sel_io[b] = -1;      // (thread 0 also writes the choice below: program order)
        if (c0 >= a.n_tracks || a.success_counter[b] >= a.max_successful) return;
        for (int j = c0; j < a.n_tracks && sel < 0; ++j) {
            const int ee = j * (int)gridDim.x + b;
            if (a.active[ee] && a.gate_in[ee] == 0) sel = j;
        }
        if (sel < 0) {                                     // nothing applicable is left: every pending status is final
            __syncthreads();
            if (threadIdx.x == 0) a.cursor[b] = a.n_tracks;
            return;
        }
        e = sel * (int)gridDim.x + b;
    }
    int c0_spec = 0;
    if (a.spec == 3) {
        const int j = blockIdx.y;
        c0_spec = a.cursor[b];
        e = j * (int)gridDim.x + b;
        const bool pass_runs = c0_spec < a.n_tracks && a.success_counter[b] < a.max_successful;
        if (!pass_runs || j < c0_spec || !a.active[e]) {      // nothing to gate here: still publish, and close the pass if last
            if (threadIdx.x == 0) {
                spec_publish(a, e, 1);
                if (j == a.n_tracks - 1) spec_close(a, b, c0_spec, pass_runs);
            }
            return;
        }
    }
    // The record's flags and its shape are requested TOGETHER: as a sequence of tests each of them was
    // a dependent HBM / L2 round trip of its own -- 15 k cycles went by before the first request for H was issued (r03 phase stamps)
    const int t = threadIdx.x, lane = t & 63;
    const unsigned char act_v = a.active ? a.active[e] : (unsigned char)1;
    const int req_v = a.require_inlier ? a.require_inlier[b] : 0;
    const int nr_rec_v0 = a.nr_rec ? a.nr_rec[e] : a.nr_full;
    int shape_pin = nr_rec_v0;
    asm volatile("" : "+v"(shape_pin));                     // (keeps the three requests in front of the first test)
    const int nr_rec_v = shape_pin;
    if (!act_v) return;
    if (req_v != 0) return;
#ifdef HV_DEBUG_SKIP_UPDATE
    // experiment only (scripts/lanes_probe.py, never in the shipped library): what do the update workgroups cost a step? An applied
    // update counts as a success and leaves (m, P) as they are
    if (a.mode == 1 && a.spec == 0) { if (a.success_counter && t == 0) a.success_counter[b] += 1; return; }
#endif
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);     // wave-uniform: tile indices and their addresses stay on the scalar unit
    constexpr int nwaves = UPD_THREADS / 64;
    const int n = a.n, l = a.l;
    int nr = a.nr, R = a.Rs, Rfull = a.R;                   // R is the column STRIDE of T below; Rfull rows are used
    int roff = 0, ld = a.nr;                               // first row of this launch's block inside the record; leading dimension of H
    int half = a.half;                                     // (half_auto: this record's own split, see UpdateArgs)
    if (a.nr_rec || a.half) {                              // ragged batch / block update: this record's own shape (uniform per workgroup)
        int nr_full = __builtin_amdgcn_readfirstlane(nr_rec_v);
        if (nr_full < 1 || nr_full > a.v_stride) return;    // no track (the prepare launch also cleared `active`)
        nr = nr_full; ld = nr_full;
        if constexpr (AUTO) {
            if (nr_full <= 48) {
                if (half == 2) return;
                half = 0;
            }
            if (half == 1 && t == 0) a.sel_io[b] = sel;
        }
        if (half) {
            if (MODE != 2) return;                         // (the host only asks the LDS-resident kernels for block updates)
            const int h1 = 2 * ((nr_full + 3) >> 2);
            roff = half == 2 ? h1 : 0;
            nr = half == 2 ? nr_full - h1 : h1;
        }
        if (nr < 1 || nr > a.nr) return;
        Rfull = nr + n + 1; R = Rfull;
        if (USE_LDS) R = lds_stride(R);
    }
    double *m = a.m + (size_t)b * n, *P = a.P + (size_t)b * n * n;
    const double *H = a.H + (size_t)e * a.h_stride;        // record stride: the launch's row count x columns; leading dimension: nr
    const double rd = a.rdiag ? a.rdiag[b] : a.rd0;
    // Tall matrix T (a.R rows x nr columns, column-major with stride R >= a.R: T(r, c) = T[c * R + r]; in LDS
    // the stride is padded to lds_stride):
    //   rows 0 .. nr-1   S = H P H' + R            -> L           (S = L L')
    //   row  nr          v'                        -> z' = (L^-1 v)'
    //   rows nr+1 ..     (H P)'  (n rows)          -> Y' = (L^-1 H P)'
    // One blocked Cholesky pass over T does the factorisation and both triangular solves. The gate
    // only needs rows 0 .. nr. All LDS comes from the dynamic region (keeps the base 16-byte aligned), carved as UpdateLds
    // says for this record's shape. USE_LDS is a template parameter so that the common case compiles to
    // ds_read / ds_write (a run-time select would turn every access into a flat load).
    const UpdateLds L = update_lds(R, nr, nwaves, USE_LDS, 0);
    double *T = USE_LDS ? smem + L.T : a.ws + (size_t)b * a.Rs * a.nr;
    double *W = smem + L.chol + CHOL_W, *col = smem + L.chol + CHOL_COL, *red = smem + L.red;
    int *s_stop = reinterpret_cast<int *>(smem + L.flag);
    double *Hs = smem + L.Hs;                     // MODE 2: H zero-padded to (16 TI) x (16 lb), column-major, stride nrp
    constexpr int nrp = 16 * (TI > 0 ? TI : 1);
    const bool gate_only = a.mode == 0;
    const int rv = nr, ry = nr + 1;
    // mode 3 (MODE 2 kernels only): visualTrackOutlierCheck with R = rd0, then -- where it passes -- updateVisualTrack with
    // R = rd1 on the SAME H P: S (without R) and v are parked in the H staging area after phase B, the gate runs the
    // Cholesky on the measurement rows only, and an inlier restores S + rd1 I and v and runs the full factorisation.
    const bool two_r = MODE == 2 && a.mode == 3;
    int Rlim = (gate_only || two_r) ? nr + 1 : Rfull;

    PHASE_STAMP(0);
    const int kq = lane >> 4, cl = lane & 15;      // MFMA lane coordinates: k sub-step / output row group, column
    // MODE 2 ownership: wavefront w owns the 16-column block J = w of P with all of its 16-row K
    // blocks ("item 0"); wavefronts 0..3 also own one K half of block 8 or 9 ("item 1": J = 8 + (w & 1),
    // half w >> 1), which gives every SIMD 2.5 column blocks of matrix work at n = 160. The four B
    // operands of a K block ARE the 16 x 16 tile P(K, J) in the MFMA C layout (lane (kq, c) holds
    // rows kq + 4 s), so the tiles fetched for H P stay in registers and serve as the old values of
    // P -= Y'Y: P crosses HBM once per update. All of a wave's P loads are issued before anything
    // else; K blocks are consumed in arrival order, so the HBM stream (~10 B/clk/CU when every CU
    // pulls at once) overlaps the MFMAs.
    constexpr int NBK = 10, NBH = 5;                // K blocks per column block / per half (n <= 160)
    double pres0[NBK][4], pres1[NBH][4];
    const int tiles_j = (n + 15) >> 4, lb = (l + 15) >> 4;
    const int hs = (tiles_j + 1) >> 1;
    const int J1 = 8 + (wave & 1), kb0_1 = (wave & 2) ? hs : 0, kb1_1 = (wave & 2) ? tiles_j : hs;
    const bool have0 = MODE == 2 && wave < tiles_j, have1 = MODE == 2 && wave < 4 && J1 < tiles_j;
    unsigned kbmask = 0xFFFFFFFFu;                  // K blocks of H P with matrix work (compact H: those that hold a non-zero column)
    if constexpr (MODE == 2) {
        // ---- A: HP = H * P[0:l, :] accumulated into rows ry.. of T (the two K halves of blocks 8, 9
        // meet through ds_add_f64 on the zeroed tile: two addends commute, the sum is reproducible) ----
        auto fetch_blk = [&](auto &pv, int bi, int J, int kb, int kend) {
            if (kb < kend && (kb < lb || !gate_only)) {
                const int jc = min(J * 16 + cl, n - 1);
#pragma unroll
                for (int sx = 0; sx < 4; sx++)
                    pv[bi][sx] = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(P) + (unsigned)(min(kb * 16 + 4 * sx + kq, n - 1) * n + jc) * 8u);
            }
        };
        // request order = arrival order: H first (every MFMA needs it), then the P tiles in the order
        // they are consumed. Only DEPTH K blocks are requested ahead of the MFMAs that use them: a
        // wave that queues its whole column block up front sits in the issue queue until most of it has
        // arrived, and the HBM stream no longer overlaps the matrix work.
        constexpr int HREG = (48 * 160 + UPD_THREADS - 1) / UPD_THREADS, DEPTH = 4;
        if (a.acol) {
            // compact H (fused prepare + gate): Hs is zeroed and the record's na x nr values are gathered BY COMPACT COLUMN and scattered
            // to their state columns -- the addresses of the gather do not depend on the column list, so Hc and the list travel
            // together: one HBM / L2 round trip, 8 values per thread at 11 stereo poses. (r03's first form built the inverse map
            // state column -> compact column in LDS first -- a dependent round trip and two barriers -- and walked all 48 x 160 cells
            // with 15 registers per thread.) kbmask: the 16-row K blocks of H P that hold a non-zero column of H at all.
            int *mask = reinterpret_cast<int *>(col);       // (the col scratch is free until the Cholesky)
            const int na = 7 * (ld / (2 * a.ncam)) + 1;     // (ld = rows of the whole record)
            const int *acol = a.acol + (size_t)e * a.na_max;
            const int total = na * nr;
            const unsigned inv_nr = (unsigned)((0x100000000ull + (unsigned)nr - 1) / (unsigned)nr);      // i / nr = umulhi(i, ceil(2^32 / nr)), i < 2^20
            constexpr int HC = 8;
            double hv[HC]; int hc[HC];
            auto request = [&](int base) {
#pragma unroll
                for (int u = 0; u < HC; u++) {
                    const int i = base + t + u * UPD_THREADS, uc = (int)__umulhi((unsigned)i, inv_nr), r = i - uc * nr;
                    const bool live = i < total;
                    hc[u] = live ? acol[uc] : -1;
                    hv[u] = live ? *reinterpret_cast<const double *>(reinterpret_cast<const char *>(H) + (unsigned)(uc * ld + roff + r) * 8u) : 0.0;
                }
            };
            auto scatter = [&](int base) {
#pragma unroll
                for (int u = 0; u < HC; u++) {
                    const int i = base + t + u * UPD_THREADS, uc = (int)__umulhi((unsigned)i, inv_nr), r = i - uc * nr;
                    if (hc[u] >= 0 && hc[u] < l) {
                        Hs[hc[u] * nrp + r] = hv[u];
                        if (r == 0) atomicOr(mask, 1 << (hc[u] >> 4));
                    }
                }
            };
            request(0);
            // The P tiles are requested BEHIND the gather, the block that is used last FIRST: the kernel sits at 255 VGPRs and the
            // register allocator spills one value of that block right behind its load, i.e. waits for it -- and loads return in order.
            // (r03's first form requested the tiles in front of the staging, block 0 first: the spill waited for all 16 of them,
            // 14 k cycles before the first request for H.)
#pragma unroll
            for (int bi = DEPTH - 1; bi >= 0; bi--) if (have0) fetch_blk(pres0, bi, wave, bi, tiles_j);     // (LAST block first: see below)
            PHASE_STAMP(8);
            for (int i = t; i < nrp * 16 * lb; i += UPD_THREADS) Hs[i] = 0.0;
            for (int i = t; i < R * nr; i += UPD_THREADS) T[i] = 0.0;
            if (t == 0) mask[0] = 0;
            __syncthreads();
            scatter(0);
            for (int base = HC * UPD_THREADS; base < total; base += HC * UPD_THREADS) { request(base); scatter(base); }     // (long mono tracks)
            __syncthreads();
            kbmask = (unsigned)mask[0];
        } else {
            double hreg[HREG];
#pragma unroll
            for (int u = 0; u < HREG; u++) {
                const int i = t + u * UPD_THREADS, k = i / nrp, r = i - k * nrp;
                hreg[u] = (i < nrp * 16 * lb && k < l && r < nr) ? H[(size_t)k * ld + roff + r] : 0.0;
            }
#pragma unroll
            for (int bi = 0; bi < DEPTH; bi++) if (have0) fetch_blk(pres0, bi, wave, bi, tiles_j);
            PHASE_STAMP(8);
            for (int i = t; i < R * nr; i += UPD_THREADS) T[i] = 0.0;
#pragma unroll
            for (int u = 0; u < HREG; u++) {
                const int i = t + u * UPD_THREADS;
                if (i < nrp * 16 * lb) Hs[i] = hreg[u];
            }
        }
        __syncthreads();
        PHASE_STAMP(9);
        const double *hbase = Hs + (size_t)kq * nrp + cl;
        // H operands of a K block: 4 k-steps x TI row tiles, double-buffered across blocks (the reads of
        // block b+1 are issued before the MFMAs of block b: a wavefront that only prefetches one or two
        // ds_reads ahead issues an MFMA every ~100 cycles instead of every 64)
        // (in HALF blocks of two k-steps: 2 x 2 x TI operand registers instead of 2 x 4 x TI -- the kernel sits at 255 VGPRs and the
        //  allocator took its last pair from the P prefetch, spilling a value right behind its load: a full stop in front of the staging)
        auto load_h = [&](int kb, int hf, double (&av)[2][TI]) {
#pragma unroll
            for (int sx = 0; sx < 2; sx++)
#pragma unroll
                for (int mt = 0; mt < TI; mt++) av[sx][mt] = hbase[(size_t)(kb * 16 + 4 * (2 * hf + sx)) * nrp + 16 * mt];
        };
        auto mfma_half = [&](auto &pv, int bi, int hf, const double (&av)[2][TI], double4v (&acc)[TI]) {
#pragma unroll
            for (int sx = 0; sx < 2; sx++)
#pragma unroll
                for (int mt = 0; mt < TI; mt++)
                    acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[sx][mt], pv[bi][2 * hf + sx], acc[mt], 0, 0, 0);
        };
        auto flush = [&](int J, double4v (&acc)[TI]) {
#pragma unroll
            for (int mt = 0; mt < TI; mt++) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int i = 16 * mt + kq + 4 * q, j = J * 16 + cl;
                    if (i < nr && j < n) unsafeAtomicAdd(&T[(size_t)i * R + ry + j], acc[mt][q]);
                }
            }
        };
        {
            double4v acc[TI];
#pragma unroll
            for (int mt = 0; mt < TI; mt++) acc[mt] = double4v{0.0, 0.0, 0.0, 0.0};
            const int nv = have0 ? min(tiles_j, lb) : 0;                   // K blocks with matrix work: 0 .. nv-1
            double av[2][2][TI];
            if (nv > 0) load_h(0, 0, av[0]);
#pragma unroll
            for (int bi = 0; bi < NBK; bi++) {
                if (bi + DEPTH < NBK) { if (have0) fetch_blk(pres0, bi + DEPTH, wave, bi + DEPTH, tiles_j); }
                else if (bi + DEPTH - NBK < NBH) { if (have1) fetch_blk(pres1, bi + DEPTH - NBK, J1, kb0_1 + bi + DEPTH - NBK, kb1_1); }
                if (bi < nv) {
                    const bool work = (kbmask >> bi) & 1;
                    load_h(bi, 1, av[1]);
                    if (work) mfma_half(pres0, bi, 0, av[0], acc);
                    if (bi + 1 < nv) load_h(bi + 1, 0, av[0]);
                    if (work) mfma_half(pres0, bi, 1, av[1], acc);
                }
            }
            if (have0) flush(wave, acc);
        }
        PHASE_STAMP(10);
        {
            double4v acc[TI];
#pragma unroll
            for (int mt = 0; mt < TI; mt++) acc[mt] = double4v{0.0, 0.0, 0.0, 0.0};
            const int nv = have1 ? max(min(kb1_1, lb) - kb0_1, 0) : 0;     // blocks kb0_1 .. kb0_1 + nv - 1
            double av[2][2][TI];
            if (nv > 0) load_h(kb0_1, 0, av[0]);
#pragma unroll
            for (int bi = 0; bi < NBH; bi++) {
                if (bi + DEPTH < NBH) { if (have1) fetch_blk(pres1, bi + DEPTH, J1, kb0_1 + bi + DEPTH, kb1_1); }
                if (bi < nv) {
                    const bool work = (kbmask >> (kb0_1 + bi)) & 1;
                    load_h(kb0_1 + bi, 1, av[1]);
                    if (work) mfma_half(pres1, bi, 0, av[0], acc);
                    if (bi + 1 < nv) load_h(kb0_1 + bi + 1, 0, av[0]);
                    if (work) mfma_half(pres1, bi, 1, av[1], acc);
                }
            }
            if (have1) flush(J1, acc);
        }
        PHASE_STAMP(11);
    } else {
        // ---- A: HP = H * P[0:l, :], stored transposed as rows ry .. ry+n-1 of T; residual row ----
        const int tiles_i = (nr + 15) / 16;
        for (int tile = wave; tile < tiles_i * tiles_j; tile += nwaves) {
            const int i0 = (tile % tiles_i) * 16, j0 = (tile / tiles_i) * 16;
            // A(i, k) = H(i0+i, k) = H[k*nr + i0+i];  B(k, j) = P(k, j0+j), read as P(j0+j, k) = P[k*n + j0+j]:
            // P is symmetric to rounding (predict builds P01/P10 separately, every other step keeps or
            // restores symmetry) and the transposed element is unit-stride across the 16 lanes of a k-row
            const double4v acc = mfma_tile<8>(H + i0, 1, nr, nr - i0, P + j0, n, 1, n - j0, l);
            const int j = j0 + cl;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int i = i0 + kq + 4 * q;
                if (i < nr && j < n) T[(size_t)i * R + ry + j] = acc[q];
            }
        }
    }
    for (int i = t; i < nr; i += UPD_THREADS) {
        double r = a.v[(size_t)e * a.v_stride + roff + i];
        if (a.generic) { double s = 0; for (int k = 0; k < l; k++) s += H[(size_t)k * nr + i] * m[k]; r -= s; }
        if constexpr (MODE == 2) {
            if (a.dm_in) {                                 // second block of a long track: v2 - H2 dm1 (Hs: the staged, zero-padded H of this block)
                const double *dm = a.dm_in + (size_t)b * n;
                double s = 0;
                for (int k = 0; k < l; k++) s += Hs[(size_t)k * nrp + i] * dm[k];
                r -= s;
            }
        }
        T[(size_t)i * R + rv] = r;
    }
    __syncthreads();

    PHASE_STAMP(1);
    // ---- B: S = HP[:, 0:l] * H' + R (lower triangle), rows 0 .. nr-1 of T ----
    {
        const int tb = (nr + 15) / 16;
        if constexpr (MODE == 2) {
            // (tile, K half) items, the halves combined with ds_add_f64 into the zeroed S block
            const int khalf = ((l / 2) + 15) & ~15;
            for (int it = wave; it < tb * (tb + 1); it += nwaves) {             // lower tiles only, two halves each
                const int hh = it & 1;
                int ib = it >> 1, cb = 0;
                while (ib >= tb - cb) { ib -= tb - cb; cb++; }                   // column cb holds tiles ib = cb .. tb-1
                ib += cb;
                const int i0 = ib * 16, c0 = cb * 16;
                const int kbeg = hh ? min(khalf, l) : 0, klen = hh ? l - kbeg : min(khalf, l);
                if (klen <= 0) continue;
                // A(i, k) = HP(i0+i, k) = T[(i0+i)*R + ry + k];  B(k, c) = H(c0+c, k) = Hs[k*nrp + c0+c]
                // (Hs is zero beyond k = l and c = nr; rows i >= nr are clamped and never stored)
                const double *pa = T + (size_t)min(i0 + cl, nr - 1) * R + ry + kbeg + kq;
                const double *pb = Hs + (size_t)(kbeg + kq) * nrp + c0 + cl;
                double4v acc = {0.0, 0.0, 0.0, 0.0};
                for (int k0 = 0; k0 < klen; k0 += 32) {          // 8 k-steps per trip, all 16 operands requested first
                    double av[8], bv[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        const bool live = k0 + 4 * u < klen;             // a partial last step meets the zero padding of Hs
                        const int kk = live ? k0 + 4 * u : 0;
                        av[u] = pa[kk]; bv[u] = pb[(size_t)kk * nrp];
                        if (!live) bv[u] = 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < 8; u++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
                }
                const int c = c0 + cl;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int i = i0 + kq + 4 * q;
                    if (i < nr && c < nr) unsafeAtomicAdd(&T[(size_t)c * R + i], acc[q] + ((i == c && hh == 0) ? rd : 0.0));
                }
            }
        } else {
            for (int tile = wave; tile < tb * tb; tile += nwaves) {
                const int ib = tile % tb, cb = tile / tb;
                if (ib < cb) continue;
                const int i0 = ib * 16, c0 = cb * 16;
                // A(i, k) = HP(i0+i, k) = T[(i0+i)*R + ry + k];  B(k, c) = H(c0+c, k) = H[k*nr + c0+c]
                const double4v acc = mfma_tile<8>(T + (size_t)i0 * R + ry, R, 1, nr - i0, H + c0, nr, 1, nr - c0, l);
                const int c = c0 + cl;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int i = i0 + kq + 4 * q;
                    if (i < nr && c < nr) T[(size_t)c * R + i] = acc[q] + (i == c ? rd : 0.0);
                }
            }
        }
    }
    __syncthreads();
    if constexpr (MODE == 2) {
        if (two_r) {                                          // Hs is dead after phase B: (nr + 1) x nr doubles fit (nrp x 16 lb >= that)
            // (+ 256: slack after the header area)
            for (int e = t; e < (nr + 1) * nr; e += UPD_THREADS) { const int c = e / (nr + 1), i = e - c * (nr + 1); Hs[256 + e] = T[(size_t)c * R + i]; }
            __syncthreads();
        }
    }

    PHASE_STAMP(2);
    for (int pass = 0; pass < (two_r ? 2 : 1); ++pass) {
    // ---- C: blocked left-looking Cholesky of the tall matrix, 16 columns per block, 3 barriers per
    // block (a column-at-a-time version needs one barrier + one LDS round trip + one rsqrt per COLUMN
    // on the critical path of all 16 waves: 1.3-1.7 k cycles per column measured). Per block j:
    //   U  every 16-row tile of block column j -= T(tile, 0:j0) * T(j0:j0+16, 0:j0)'         (MFMA)
    //   D  wave 0 factors the diagonal block in registers and inverts the factor   (factor_diag_block)
    //   P  every tile below the diagonal block *= Linv'                                       (MFMA)
    // Multiplying by the explicit inverse of a 16 x 16 diagonal block instead of substituting is the
    // usual blocked-TRSM trade: the error grows with cond(L_jj), not cond(L).
    for (int j0 = 0; j0 < nr; j0 += 16) {
        const int w = min(16, nr - j0);
        const int ntile = (Rlim - j0 + 15) / 16;
        const int i_l = lane >> 4, c_l = lane & 15;
        if (j0 > 0) {
            for (int tile = wave; tile < ntile; tile += nwaves) {
                const int i0 = j0 + 16 * tile, mi = Rlim - i0;
                // A(i, k) = T(i0+i, k) = T[k*R + i0+i];  B(k, c) = T(j0+c, k) = T[k*R + j0+c]
                const double4v acc = mfma_tile(T + i0, 1, R, mi, T + j0, R, 1, w, j0);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int i = i_l + 4 * q;
                    if (i < mi && c_l < w) T[(size_t)(j0 + c_l) * R + i0 + i] -= acc[q];
                }
            }
            __syncthreads();
        }
        if (j0 == 0) PHASE_STAMP(6);
        if (wave == 0) { if (w <= 8) factor_diag_block<8>(T, W, col, R, j0, w, lane); else factor_diag_block<16>(T, W, col, R, j0, w, lane); }
        __syncthreads();
        if (j0 == 0) PHASE_STAMP(7);
        for (int i0 = j0 + w + 16 * wave; i0 < Rlim; i0 += 16 * nwaves) {        // rows below the w x w diagonal block
            const int mi = Rlim - i0;
            // A(i, k) = T(i0+i, j0+k) = T[(j0+k)*R + i0+i];  B(k, c) = Linv(c, k) = W[k*16 + c]
            const double4v acc = mfma_tile(T + (size_t)j0 * R + i0, 1, R, mi, W, 16, 1, 16, w);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int i = i_l + 4 * q;
                if (i < mi && c_l < w) T[(size_t)(j0 + c_l) * R + i0 + i] = acc[q];
            }
        }
        __syncthreads();
    }

    PHASE_STAMP(3);
    // ---- D: chi2 = noise_scale * z'z ----
    {
        double s = 0;
        for (int c = t; c < nr; c += UPD_THREADS) { const double z = T[(size_t)c * R + rv]; s += z * z; }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        if (t == 0) {
            double tot = 0; for (int w2 = 0; w2 < nwaves; w2++) tot += red[w2];
            tot *= a.noise_scale;
            // A non-positive pivot (S not positive definite: r = 0 with a rank-deficient H) leaves NaN / inf in z: such a filter is
            // reported as CHI2 and left untouched in EVERY mode, where the reference's pivoted LDLT would carry on (r01 advisor)
            const bool broken = !(tot < 1e300);
            const int outlier = broken || ((nr < HV_CHI2INV95_N) ? (tot > d_chi2inv95[nr]) : 0);
            if (pass == 0) {
                if (a.chi2) a.chi2[e] = tot;
                if (a.status) a.status[e] = outlier ? 3 /*CHI2*/ : 0 /*INLIER*/;
            }
            *s_stop = (a.mode == 0) || broken || ((a.mode == 2 || (two_r && pass == 0)) && outlier);
            if (broken && a.gate_rw) a.gate_rw[e] = 3 /*CHI2*/;
            if (AUTO && broken && a.spec == 2 && half != 1) a.cursor[b] = sel + 1;     // (whole short record or block 2: not applied, the track is final)
            if (AUTO && broken && a.spec == 2 && half == 2 && a.epoch)                 // block 1 of this record HAS been applied
                for (int jj = sel + 1; jj < a.n_tracks; ++jj) a.epoch[jj * (int)gridDim.x + b] = -1;
            if (a.spec == 3 && pass == 0) {
                const int j = blockIdx.y;
                spec_publish(a, e, outlier ? 1 : 2);
                if (!outlier) {                               // first inlier in visit order applies; the others are re-examined next pass
                    bool lose = false;
                    for (int jj = c0_spec; jj < j && !lose; ++jj) lose = spec_wait(a, jj * (int)gridDim.x + b) != 1;
                    if (lose) *s_stop = 1;
                }
                if (*s_stop && j == a.n_tracks - 1 && outlier) spec_close(a, b, c0_spec, true);
            }
            // the applying workgroup met a non-positive pivot in the second factorisation: nothing is applied, the track is final
            if (a.spec == 3 && pass == 1 && *s_stop) a.cursor_out[b] = (int)blockIdx.y + 1;
        }
        __syncthreads();
        if (*s_stop) return;
    }
    if constexpr (MODE == 2) {
        if (two_r && pass == 0) {                             // inlier: S + rd1 I and v back, then the full factorisation
            const double shift = a.rd1 - rd;
            for (int e = t; e < (nr + 1) * nr; e += UPD_THREADS) {
                const int c = e / (nr + 1), i = e - c * (nr + 1);
                T[(size_t)c * R + i] = Hs[256 + e] + (i == c ? shift : 0.0);
            }
            Rlim = Rfull;
            __syncthreads();
        }
    }
    }   // pass

    PHASE_STAMP(4);
    // ---- E: m += Y' z ----
    for (int j = t; j < n; j += UPD_THREADS) {
        double s = 0;
        for (int c = 0; c < nr; c++) s += T[(size_t)c * R + ry + j] * T[(size_t)c * R + rv];
        m[j] += s;
        if (a.dm_out && !(AUTO && half == 0)) a.dm_out[(size_t)b * n + j] = s;
    }
    // ---- F: P -= Y' Y ----
    if constexpr (MODE == 2) {
        // tiles P(K, J) of the wave's items; old values are the registers filled in phase A
        auto down_item = [&](auto &pv, int nblk, int J, int kb0, int kb1) {
            const int jc = min(J * 16 + cl, n - 1);
            // B(c, j) = Y(c, J*16 + j) = T[c*R + ry + J*16 + j], c = 4 s + kq: shared by all tiles of the item
            constexpr int KS = 4 * TI;              // k-steps over the nr <= 16 TI rows of Y (zero beyond nr)
            double yj[KS];
#pragma unroll
            for (int sx = 0; sx < KS; sx++) {
                const int c = 4 * sx + kq;
                const double y = T[(size_t)min(c, nr - 1) * R + ry + jc];
                yj[sx] = c < nr ? y : 0.0;
            }
#pragma unroll
            for (int bi = 0; bi < nblk; bi++) {
                const int kb = kb0 + bi;
                if (kb < kb1) {
                    // A(i, c) = Y(c, kb*16 + i) = T[c*R + ry + kb*16 + i]; rows c >= nr meet yj = 0
                    const int ic = min(kb * 16 + cl, n - 1);
                    double av[KS];
#pragma unroll
                    for (int sx = 0; sx < KS; sx++) av[sx] = T[(size_t)min(4 * sx + kq, nr - 1) * R + ry + ic];
                    double4v acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int sx = 0; sx < KS; sx++) {
                        // only the last tile of rows can be (partly) empty: skip whole k-steps beyond nr
                        if (sx < KS - 4 || 4 * sx < nr) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[sx], yj[sx], acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int i = kb * 16 + kq + 4 * q, j = J * 16 + cl;
                        if (i < n && j < n) P[(size_t)i * n + j] = pv[bi][q] - acc[q];
                    }
                }
            }
        };
        if (have0) down_item(pres0, NBK, wave, 0, tiles_j);
        if (have1) down_item(pres1, NBH, J1, kb0_1, kb1_1);
    } else {
        // Y'Y is symmetric: entry (i, j) of a tile is applied to element (j, i), so the 16 lanes of a
        // row group touch 16 consecutive doubles. The old values of the NEXT tile are requested before
        // the MFMA loop of the current one: the ~1 us HBM round trip of P hides behind the matrix work
        // instead of stalling every tile.
        const int tb = (n + 15) / 16, ntiles = tb * tb;
        const int cj = lane & 15, ri = lane >> 4;
        auto p_addr = [&](int tile, int q) -> double * {
            const int i = min((tile % tb) * 16 + ri + 4 * q, n - 1), j = min((tile / tb) * 16 + cj, n - 1);
            return P + (size_t)i * n + j;
        };
        double cur[4], nxt[4] = {0.0, 0.0, 0.0, 0.0};
        if (wave < ntiles) {
#pragma unroll
            for (int q = 0; q < 4; q++) cur[q] = *p_addr(wave, q);
        }
        for (int tile = wave; tile < ntiles; tile += nwaves) {
            const int i0 = (tile % tb) * 16, j0 = (tile / tb) * 16;
            const int tn = min(tile + nwaves, ntiles - 1);
#pragma unroll
            for (int q = 0; q < 4; q++) nxt[q] = *p_addr(tn, q);
            // A(i, c) = Y(c, i0+i) = T[c*R + ry + i0+i];  B(c, j) = Y(c, j0+j) = T[c*R + ry + j0+j]
            const double4v acc = mfma_tile(T + ry + i0, 1, R, n - i0, T + ry + j0, R, 1, n - j0, nr);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int i = i0 + ri + 4 * q, j = j0 + cj;
                if (i < n && j < n) P[(size_t)i * n + j] = cur[q] - acc[q];
                cur[q] = nxt[q];
            }
        }
    }
    __syncthreads();
    PHASE_STAMP(5);
    // ---- G: quaternion normalisation (updateCommon ekf.cpp:29-31 / normalizeQuaternions 1024-1032) ----
    const bool first_block = AUTO ? half == 1 : a.normalize_all < 0;                              // of a long track: no normalisation yet
    const int nq = first_block ? 0 : (a.normalize_all != 0) ? 1 + (n - a.map_dim - CAM) / POSE : 1;      // map points behind the trail are not poses
    if (t < nq) normalize4(m + (t == 0 ? ORI : CAM + POSE * (t - 1) + 3));
    if (a.success_counter && t == 0 && !(AUTO && half == 1)) a.success_counter[b] += 1;
    if (a.spec == 2 && t == 0 && !(AUTO && half == 1)) a.cursor[b] = sel + 1;      // the tracks up to the applied one are final, the rest is re-examined
    if (a.spec == 3 && t == 0) a.cursor_out[b] = (int)blockIdx.y + 1;
}

template <int MODE, int TI>
__global__ __launch_bounds__(UPD_THREADS) void ekf_update_kernel(UpdateArgs a)
{
    // (r03 also tried one workgroup per CU pulling filters from a device queue: inside a loop the body lost its register allocation --
    // ~480 spilled VGPRs, 2.4x the time per filter -- and keeping P in the registers across the two blocks of a long track in ONE launch
    // -- 250 - 450 spilled VGPRs --, so masked launches use the compaction list and long tracks take two launches)
    int b = blockIdx.x;
    if (a.rec_list) { if ((int)blockIdx.x >= *a.rec_count) return; b = a.rec_list[blockIdx.x]; }
    ekf_update_body<MODE, TI>(a, b);
}

// the update launches of the speculative loop over long records (UpdateArgs::half_auto), MODE 2, three row tiles
__global__ __launch_bounds__(UPD_THREADS) void ekf_update_spec_long_kernel(UpdateArgs a)
{
    ekf_update_body<2, 3, true>(a, blockIdx.x);
}

// Two masked update launches in ONE grid (ragged visits: the inliers of the short class and the first block of the long class's
// inliers are different filters, ~200 + ~50 of 1024 at the reference's track mix -- one workgroup each on a CU of its own, so two
// launches were two latency chains back to back on a mostly idle chip): the first workgroups serve a1's list, the next ones a0's.
// The argument block is chosen by a uniform select; the body is instantiated once.
// Every workgroup needs a CU of its own, so a grid of more than num_cus live workgroups takes a second round. The long class follows
// with a second launch anyway (its second block update): `part` 0 = all of a1 + the entries of a0's list that fit beside them on the
// chip (cap = num_cus - *a1.rec_count), `part` 1 = all of a1 + the REST of a0's list -- the visit loop issues (a0 = short class, a1 =
// long block 1, part 0) and then (a0 = short class, a1 = long block 2, part 1); `part` < 0: all of both lists.
struct UpdatePair { UpdateArgs a[2]; };
template <int MODE, int TI>
__global__ __launch_bounds__(UPD_THREADS) void ekf_update_dual_kernel(UpdatePair p, int part, int num_cus)
{
    const int n0 = *p.a[0].rec_count, n1 = *p.a[1].rec_count, i = (int)blockIdx.x;
    const int cap = min(n0, max(num_cus - n1, 0));
    const int lo = part == 1 ? cap : 0, hi = part == 0 ? cap : n0;          // a[0]'s share of this launch
    const bool second = i < n1;
    // (ONE block is read, through a run-time index into the kernel-argument segment: with two by-value blocks and a select per field
    //  both sat in SGPRs -- 250 of them spilled into VGPR lanes, in a kernel that has no VGPR to spare)
    const UpdateArgs &a = p.a[second ? 1 : 0];
    const int j = second ? i : i - n1 + lo;
    if (!second && j >= hi) return;
    ekf_update_body<MODE, TI>(a, a.rec_list[j]);
}

// (r05, measured and dropped: the same grid with a long record's workgroup running block 2 right behind block 1 -- P through L2 in
// between -- and a second launch that only serves the short records that found no CU: one lane 10.04 / 10.00 -> 10.13 / 10.10 ms per
// step, four lanes 29.44 / 29.27 -> 29.40 / 29.23: the visit's length is the long records' block-1 -> block-2 chain either way, and two
// instances of the body cost 12 more spilled VGPRs. profiles/r05/long_blocks_one_launch_ab.txt)

}  // namespace

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// an update launch prepared but not issued (UpdateRequest::defer): two of them can share one grid (ekf_launch_update_dual)
struct UpdateLaunch { UpdateArgs a; int kmode = -1, ti = 0, lbk = 0; };

int ekf_launch_update(Ekf *e, const UpdateRequest &rq)
{
    Ctx *c = e->c;
    const int nr = rq.nr, l = rq.l, mode = rq.mode, generic = rq.generic, spec = rq.spec;
    const int nr_stride = rq.nr_stride <= 0 ? nr : rq.nr_stride;
    if (nr < 1 || nr > e->max_rows || l < 1 || l > e->n) return HV_ERR_INVALID;
    // the chi2 gate needs chi2inv95[nr] (the reference asserts n < chi2inv95.size(): ekf.cpp:806); mode 1 with an
    // inlier requirement is the update half of a gate that already ran
    if (!generic && mode != 1 && nr >= HV_CHI2INV95_N) return HV_ERR_INVALID;
    UpdateArgs a{};
    a.n = e->n; a.nr = nr; a.l = l; a.R = nr + e->n + 1;
    const UpdateShape shape = update_shape(e->n, nr, l, UPD_THREADS / 64);
    a.Rs = shape.Rs;                                     // (lds_stride; unpadded where T lives in the global workspace)
    a.mode = mode; a.generic = generic; a.normalize_all = rq.normalize_all; a.map_dim = e->map_dim;
    a.m = e->fixed.m; a.P = e->fixed.P; a.H = rq.H_dev; a.v = rq.v_dev; a.rdiag = rq.rdiag_dev; a.rd0 = rq.rd0; a.rd1 = rq.rd1; a.noise_scale = e->noise_scale;
    a.ws = e->fixed.ws; a.chi2 = rq.chi2_dev; a.status = rq.status_dev; a.active = rq.active_dev; a.require_inlier = rq.require_inlier_dev; a.success_counter = rq.success_counter_dev;
    a.spec = spec; a.n_tracks = rq.n_tracks; a.cursor = rq.cursor_dev; a.max_successful = rq.max_successful; a.gate_in = rq.gate_in_dev;
    a.cursor_out = rq.cursor_out_dev; a.pub = rq.pub_dev; a.pass_id = rq.pass_id; a.nr_rec = rq.nr_rec_dev; a.err = e->fixed.err_dev;
    a.h_stride = (size_t)nr_stride * l; a.v_stride = nr_stride;
    if (rq.compact.acol) {
        const CompactH *compact = &rq.compact;
        a.acol = compact->acol; a.na_max = compact->na_max; a.ncam = compact->ncam; a.h_stride = (size_t)nr_stride * compact->na_max;
        a.half = compact->half; a.nr_full = compact->nr_full;
        if (a.half == 1) { a.dm_out = compact->dm; a.gate_rw = compact->gate_rw; }
        if (a.half == 2) a.dm_in = compact->dm;
        a.rec_count = compact->rec_count; a.rec_list = compact->rec_list;
        a.half_auto = compact->half_auto; a.sel_io = compact->sel_io; a.epoch = compact->epoch;
        if (a.half_auto && (spec != 2 || !a.half || !a.sel_io || !a.dm_out == !a.dm_in)) return HV_ERR_INVALID;
    }
    const int ti = shape.ti, lbk = shape.lbk;
    int kmode = shape.kmode;
    a.use_lds = kmode != 0;
    // HV_EKF_GATE_KMODE (environment, experiments only): kernel variant for gate-only launches (1 = H streamed from L2, 2 WGs / CU)
    if (c->knob.ekf_gate_kmode == 1 && mode == 0 && !spec && kmode == 2) kmode = 1;
    if (a.acol && kmode != 2) return HV_ERR_UNSUPPORTED; // compact H is staged by the LDS-resident kernel only (vu_fused_supported)
    if (mode == 3) {                                     // gate (rd0) + update (rd1) in one launch: MODE 2 kernels only
        const bool can = kmode == 2 && shape.two_r;
        if (rq.two_r_done) *rq.two_r_done = can;
        if (!can) return HV_OK;                          // the caller falls back to two launches
    }
    if (spec && kmode != 2) return HV_ERR_UNSUPPORTED;   // the speculative loop keeps every record in the LDS-resident kernel
    const size_t shmem = lds_bytes(update_lds(shape.Rs, nr, UPD_THREADS / 64, kmode != 0, kmode == 2 ? shape.hs : 0));
    a.batch = e->batch;
    if (UpdateLaunch *defer = rq.defer) {
        if (mode == 3 || spec) return HV_ERR_INVALID;
        defer->a = a; defer->kmode = kmode; defer->ti = ti; defer->lbk = lbk;
        return HV_OK;
    }
    using Kern = void (*)(UpdateArgs);
    if (a.half_auto && (kmode != 2 || ti != 3)) return HV_ERR_INVALID;
    const Kern kern = a.half_auto ? (Kern)ekf_update_spec_long_kernel : kmode == 0 ? (Kern)ekf_update_kernel<0, 0> : kmode == 1 ? (Kern)ekf_update_kernel<1, 0>
                    : ti == 1 ? (Kern)ekf_update_kernel<2, 1> : ti == 2 ? (Kern)ekf_update_kernel<2, 2> : (Kern)ekf_update_kernel<2, 3>;
    ScopedKernelTime tm(c, HV_K_EKF_UPDATE);
    hipLaunchKernelGGL(kern, dim3(e->batch, (spec == 1 || spec == 3) ? rq.n_tracks : 1), dim3(UPD_THREADS), shmem, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

// two deferred masked MODE 2 launches over disjoint filters as one grid; *done = false when their shapes do not allow it (the caller
// then issues them one after the other)
static int ekf_launch_update_dual(Ekf *e, const UpdateLaunch &A, const UpdateLaunch &B, int part, bool *done)
{
    Ctx *c = e->c;
    *done = false;
    if (A.kmode != 2 || B.kmode != 2 || !A.a.rec_list || !B.a.rec_list || !A.a.rec_count || !B.a.rec_count) return HV_OK;
    const int ti = A.ti > B.ti ? A.ti : B.ti;
    if (ti != 3) return HV_OK;                                     // (the only pairing the visit loop produces: 44 + 42 rows)
    const auto bytes = [ti](const UpdateLaunch &u) { return lds_bytes(update_lds(u.a.Rs, u.a.nr, UPD_THREADS / 64, true, (size_t)(16 * ti) * (16 * u.lbk))); };
    const size_t sa = bytes(A), sb = bytes(B), shmem = sa > sb ? sa : sb;
    if (shmem > LDS_UPDATE_LIMIT) return HV_OK;
    ScopedKernelTime tm(c, HV_K_EKF_UPDATE);
    UpdatePair pair;
    pair.a[0] = A.a; pair.a[1] = B.a;
    hipLaunchKernelGGL((ekf_update_dual_kernel<2, 3>), dim3(e->batch), dim3(UPD_THREADS), shmem, c->stream, pair, part, c->num_cus);
    HV_HIP(c, hipGetLastError());
    *done = true;
    return HV_OK;
}

int ekf_launch_update_paired(Ekf *e, const UpdateRequest &us, const UpdateRequest &b1, const UpdateRequest &b2, bool *done)
{
    // (short class beside block 1, what did not fit on the chip beside block 2: see ekf_update_dual_kernel)
    UpdateLaunch s, u1, u2;
    *done = false;
    const auto prepare = [e](UpdateRequest rq, UpdateLaunch *out) { rq.defer = out; return ekf_launch_update(e, rq); };
    int rc = prepare(us, &s);
    if (rc == HV_OK) rc = prepare(b1, &u1);
    if (rc == HV_OK) rc = prepare(b2, &u2);
    if (rc != HV_OK) return rc;
    rc = ekf_launch_update_dual(e, s, u1, 0, done);
    if (rc != HV_OK || !*done) return rc;
    bool again = false;
    return ekf_launch_update_dual(e, s, u2, 1, &again);              // (same shapes: accepted again)
}

// the kernels' dynamic-LDS limits (ekf_kernels_init)
int ekf_update_init(Ctx *c)
{
    HV_HIP(c, set_lds_limit(ekf_update_kernel<1, 0>, LDS_UPDATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_update_kernel<2, 1>, LDS_UPDATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_update_kernel<2, 2>, LDS_UPDATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_update_kernel<2, 3>, LDS_UPDATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_update_spec_long_kernel, LDS_UPDATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_update_dual_kernel<2, 3>, LDS_UPDATE_LIMIT));
    return HV_OK;
}

#ifdef HV_EKF_PHASE_STAMPS
hipError_t ekf_update_phase_stamps(long long *out16) { return hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_phase_stamp), sizeof(long long) * 16); }
#endif

}  // namespace hv
