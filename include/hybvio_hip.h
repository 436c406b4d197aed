/*
 * hybvio_hip.h -- C ABI of libhybvio_hip.so: the MI355X (gfx950) implementation of HybVIO's
 * per-frame hot path (image pyramid + pyramidal Lucas-Kanade tracker + EKF covariance algebra) and of
 * its GFTT feature detector with the detector's sub-pixel corner refinement.
 *
 * Plain pointers and sizes only; no C++/torch types cross this boundary. Every entry point
 * returns HV_OK (0) or a negative hv_status; nothing throws. All device work of one hv_ctx is
 * issued on one HIP stream (the reference runs Tracker::add and every EKF method on a single
 * thread: src/api/api.cpp:82,425; src/util/bounded_processing_queue.hpp:18).
 *
 * Each group cites the reference interface (file:line under the HybVIO tree) that it replaces;
 * INTEGRATION.md shows the C++ adapters a maintainer adds on the reference side.
 *
 * Names ending in _dev take DEVICE pointers and are asynchronous on the context stream
 * (throughput / multi-session mode: many independent sequences per GPU in one launch).
 * All other entry points take HOST pointers and are synchronous on return unless stated.
 */
#ifndef HYBVIO_HIP_H_
#define HYBVIO_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HV_ABI_VERSION 4   /* 4 (r05; later additions within 4: hv_subpix_default_params, hv_corner_subpix, hv_corner_subpix_batch_dev, HV_K_SUBPIX; hv_ransac5_default_params, hv_ransac5, hv_ransac5_batch_dev, hv_hybrid_ransac_lk_batch_dev, HV_K_RANSAC5; hv_stereo_gate_default_params, hv_flow_status_batch_dev, hv_track_gate, hv_track_gate_batch_dev, hv_detection_filter, hv_detection_filter_batch_dev, HV_K_STEREO_GATE): host-pointer forms of the r04 frame entries (hv_ekf_visual_frame_batch, hv_ekf_visual_track_hybrid, hv_ekf_symmetrize_augment), hv_ekf_insert_map_point / hv_ekf_get_map_point; 3 (r04): hv_lanes_*, hv_get_stream; 2 (r03): hv_debug_*_knob, hv_ekf_frame_error, HV_ERR_TIMEOUT; maxSuccessfulVisualUpdates <= 0 = no limit */
#define HV_MAX_LEVELS 6

typedef enum hv_status {
    HV_OK = 0,
    HV_ERR_INVALID = -1,      /* bad argument                                  */
    HV_ERR_UNSUPPORTED = -2,  /* parameter combination not implemented          */
    HV_ERR_NO_DEVICE = -3,    /* no HIP device / HIP runtime failed to start    */
    HV_ERR_HIP = -4,          /* a HIP call failed; see hv_last_error()         */
    HV_ERR_POOL = -5,         /* pyramid pool exhausted / bad slot              */
    HV_ERR_NOMEM = -6,
    HV_ERR_TIMEOUT = -7       /* a device-side wait gave up; the call's result must not be used */
} hv_status;

typedef struct hv_ctx hv_ctx;

/* Mirror of the few odometry::ParametersTracker fields the path reads
 * (codegen/parameter_definitions.c:262,336-344). */
typedef struct hv_params {
    int device;            /* HIP device ordinal                                         */
    int width, height;     /* level-0 image size (all images of a context share it)      */
    int levels;            /* pyrLKMaxLevel + 1                        (default 3 + 1)   */
    int win;               /* pyrLKWindowSize                          (default 31)      */
    int max_iter;          /* pyrLKMaxIter                             (default 20)      */
    double eps;            /* pyrLKEpsilon                             (default 0.03)    */
    double min_eig;        /* pyrLKMinEigThreshold                     (default 1e-3)    */
    int max_tracks;        /* tracker.maxTracks: points per LK call    (default 200)     */
    int pool_size;         /* pyramid slots kept on the device (util::Allocator analogue)*/
    int max_pairs;         /* max (prev,next) pyramid pairs per batched LK launch        */
} hv_params;

void hv_default_params(hv_params *p);                 /* fills the defaults listed above */
int hv_abi_version(void);
const char *hv_status_string(int status);
/* Test / measurement hooks: force a kernel variant that production code selects by shape or batch size (names: the fields of
 * hv::Knobs in csrc/hv_internal.hpp, e.g. "vu_threads" 384 / 768, "pyr_tail" 0 / 1, "rot_ransac_threads" 256 / 1024, "ekf_fused_gate"
 * 0). The same names in upper case with an HV_ prefix are read from the environment ONCE, by hv_create; nothing on the hot path
 * calls getenv. HV_ERR_INVALID for an unknown name. Not needed by an integration. */
int hv_debug_set_knob(hv_ctx *ctx, const char *name, int value);
int hv_debug_get_knob(hv_ctx *ctx, const char *name, int *value);

/* ---- context ---------------------------------------------------------------------------- */
/* Any positive image size. An image not larger than the LK window in either direction gets a pyramid of one level that the
 * pyramid build, the detector and the sub-pixel refinement serve; every LK entry (hv_klt_track, hv_optical_flow_compute,
 * hv_klt_track_batch_dev, hv_klt_track_batch_ragged_dev and the fused entries that track) returns HV_ERR_UNSUPPORTED on it. */
int hv_create(const hv_params *params, hv_ctx **out);
void hv_destroy(hv_ctx *ctx);
const char *hv_last_error(hv_ctx *ctx);               /* text of the last HV_ERR_HIP           */
int hv_set_stream(hv_ctx *ctx, void *hip_stream);     /* run on a caller-owned hipStream_t     */
void *hv_get_stream(hv_ctx *ctx);                     /* the hipStream_t the context issues on  */
int hv_synchronize(hv_ctx *ctx);

/* ---- lanes: several batched contexts of one process on one GPU ------------------------------
 * The reference runs one session per process (main.cpp); a GPU serves many. One batched context advances its B resident
 * sequences through a frame as a chain of dependent launches -- a VALU-bound tracker half, then a latency-bound EKF half whose
 * launches fill a fraction of the chip -- so TWO contexts whose chains run beside each other deliver more frames per second
 * than one context alone (107 k -> 130 k frames/s at 2 x 1024 sequences, 138 k at 4 x 1024). Whether their
 * launches really overlap is decided by the HARDWARE QUEUE each busy stream is bound to, and for default-priority streams that
 * depends on everything the process created before (r03 needed a particular creation order in the caller). A lane set owns that
 * placement: hv_lanes_create creates n_lanes contexts (same parameters) whose two streams each -- the context stream and the
 * library's second stream of the ragged visit loop -- come from the device's HIGH-priority queue pool, which holds a queue per
 * stream for up to two lanes regardless of process history. Drive every lane from its own host thread or round-robin from one;
 * the lanes share nothing but the device. hv_lanes_ctx returns a lane's context (owned by the set: do not hv_destroy it, do not
 * hv_set_stream it); hv_get_stream gives the stream to enqueue caller-side work (or a HIP-graph capture) on. */
#define HV_MAX_LANES 8
typedef struct hv_lanes hv_lanes;
int hv_lanes_create(const hv_params *params, int n_lanes, hv_lanes **out);
int hv_lanes_count(const hv_lanes *lanes);
hv_ctx *hv_lanes_ctx(hv_lanes *lanes, int lane);
void hv_lanes_destroy(hv_lanes *lanes);

/* ---- image pyramid ----------------------------------------------------------------------
 * Replaces tracker::ImagePyramid::Factory::compute (src/tracker/image_pyramid.hpp:35-41,
 * image_pyramid.cpp:40-48 -> cv::buildOpticalFlowPyramid(img, pyr, Size(win,win), maxLevel)).
 * A slot is one image's pyramid: gray levels 1..L-1 (u8, 5x5 binomial, (s+128)>>8) and Scharr
 * gradients (int16 [dx,dy] interleaved, scale 1/32: image_pyramid.hpp:19-26). Only the coarse levels (>= 2) keep
 * their gradient plane in memory; those of levels 0 and 1 are formed inside the tracker kernel from the gray
 * rows -- hv_pyramid_download still returns every level's gradients (computed on demand).
 * Levels 0 and 1 are stored without a border (applied virtually by the tracker: BORDER_REFLECT_101 for gray,
 * 0 for gradients, exactly as OpenCV pads); levels >= 2 carry OpenCV's border physically.
 * Slots are pooled like util::Allocator (src/util/allocator.hpp:55-67): acquire when an Image
 * first needs its pyramid (image.cpp:209-214), release when the Image dies. Like the reference's
 * allocator the pool grows on demand: when every slot is in use hv_pyramid_acquire doubles the slab
 * (synchronises the stream; slot numbers and contents are kept; HIP graphs captured earlier hold stale
 * addresses) and only reports HV_ERR_POOL when the device is out of memory. pool_size is the initial size. */
int hv_pyramid_acquire(hv_ctx *ctx, int *slot_out);
int hv_pyramid_release(hv_ctx *ctx, int slot);
int hv_pyramid_level_size(hv_ctx *ctx, int level, int *width, int *height);
/* H2D copy of a host gray image (stride_bytes per row) + all level kernels; asynchronous. */
int hv_pyramid_build(hv_ctx *ctx, int slot, const uint8_t *gray_host, int stride_bytes);
/* n images already resident in HBM: image i starts at gray_dev + i*image_stride_bytes and
 * is used in place as level 0 (it must stay valid until the slot is released/rebuilt).
 * slots_dev: n slot indices in device memory. Asynchronous. */
int hv_pyramid_build_batch_dev(hv_ctx *ctx, int n, const int *slots_dev, const uint8_t *gray_dev,
                               long long image_stride_bytes, int row_stride_bytes);
/* Test/debug read-back of one level (interior only): gray w*h u8 and/or grad w*h*2 int16;
 * either pointer may be NULL. Synchronous. (ImagePyramid::getGrayLevel/getGradientLevel/getOpenCv) */
int hv_pyramid_download(hv_ctx *ctx, int slot, int level, uint8_t *gray, int16_t *grad);

/* ---- pyramidal Lucas-Kanade --------------------------------------------------------------
 * hv_klt_track replaces cv::calcOpticalFlowPyrLK as called at src/tracker/optical_flow.cpp:46-49
 * (window win x win, levels, TermCriteria(COUNT|EPS, max_iter, eps), minEigThreshold, err != NULL).
 * next_xy is in/out: initial guess when use_initial_flow != 0 (OPTFLOW_USE_INITIAL_FLOW).
 * status: 1 tracked / 0 lost. max_iter_override <= 0 keeps the context value. err may be NULL (the
 * reference discards it: optical_flow.cpp:26); the level-0 range check that can clear status runs
 * either way. Synchronous.
 * Non-finite and out-of-range coordinates (every LK entry): a previous point or a guess with a NaN, an infinite or a
 * beyond-int-range coordinate is treated as cvFloor treats it on x86 (INT_MIN: outside every window test). Status 0,
 * err 0, and next_xy is the start value (the guess under use_initial_flow, else the previous point) scaled down to the
 * coarsest level and doubled back: the input value itself, a NaN coordinate staying NaN. Other points of the call are not
 * affected. tests/test_gpu_nonfinite.py holds this to the oracle. */
int hv_klt_track(hv_ctx *ctx, int prev_slot, int next_slot, int n, const float *prev_xy,
                 float *next_xy, uint8_t *status, float *err, int use_initial_flow,
                 int max_iter_override);
/* Replaces tracker::OpticalFlow::compute (src/tracker/optical_flow.hpp:31-38,
 * optical_flow.cpp:10-59,78-102): runs LK, maps to Feature::Status (track.hpp:9-21:
 * TRACKED=0, FAILED_FLOW=2) and overrides to FLOW_OUT_OF_RANGE=4 outside the level-0 image.
 * corners is in/out (input when use_initial_corners). n == 0 is a no-op. Synchronous.
 * A lost point whose returned corner has a NaN coordinate (NaN previous point or guess, see hv_klt_track) is FAILED_FLOW:
 * no comparison of the range test holds for NaN. Infinite and beyond-int-range ones are FLOW_OUT_OF_RANGE. */
int hv_optical_flow_compute(hv_ctx *ctx, int prev_slot, int cur_slot, int n,
                            const float *prev_corners, float *corners, int32_t *track_status,
                            int use_initial_corners, int override_max_iterations);
/* Batched: n_pairs independent (prev,next) pyramid pairs with pts_per_pair points each, one
 * launch; point j of pair p is element p*pts_per_pair + j of every array. All arrays are in
 * device memory (err_dev may be NULL); asynchronous. Non-finite and out-of-range points and guesses: status 0, as
 * described at hv_klt_track (predicted corners are NaN whenever the pose they come from is); hv_flow_status_batch_dev
 * then gives FAILED_FLOW for a NaN corner and FLOW_OUT_OF_RANGE for the others, as hv_optical_flow_compute does. */
int hv_klt_track_batch_dev(hv_ctx *ctx, int n_pairs, const int *prev_slots_dev,
                           const int *next_slots_dev, int pts_per_pair, const float *prev_xy_dev,
                           float *next_xy_dev, uint8_t *status_dev, float *err_dev,
                           int use_initial_flow, int max_iter_override);
/* The same for pairs with different point counts (sequences of a batch do not track the same number of features): pair p
 * holds pts_in_pair_dev[p] <= pts_per_pair points at the start of its record; the padding behind them falls through at once
 * (status 0, next_xy unspecified). */
int hv_klt_track_batch_ragged_dev(hv_ctx *ctx, int n_pairs, const int *prev_slots_dev, const int *next_slots_dev,
                                  int pts_per_pair, const int *pts_in_pair_dev, const float *prev_xy_dev, float *next_xy_dev,
                                  uint8_t *status_dev, float *err_dev, int use_initial_flow, int max_iter_override);


/* ---- EKF covariance algebra --------------------------------------------------------------
 * Replaces the dense work of odometry::EKF (src/odometry/ekf.hpp:62-174, ekf.cpp) for a BATCH of
 * independent filters that share one parameter set (batch = 1 is the reference's single session).
 * State m (n = 20 + 7*cameraTrailLength + 3*hybridMapSize) and covariance P (n x n, f64,
 * column-major like Eigen) stay on the device; the scalar bookkeeping of the reference class
 * (sample clock, ZUPT rate limits, augmentTimes) lives in the host adapter (hybvio_amd/host); a batch of
 * resident sequences keeps the rate limits and flags (hv_ekf_control) and the sample clock (hv_session) on the device instead.
 * Per-filter inputs are arrays indexed [filter][...]. Calls are asynchronous on the context
 * stream unless they return data to the host. */
typedef struct hv_ekf hv_ekf;

/* The odometry parameters EKFImplementation reads (codegen/parameter_definitions.c:68-160). */
typedef struct hv_ekf_params {
    int cameraTrailLength, hybridMapSize;
    double noiseScale, gravity, augmentR, initZuptR, rotationZuptR;
    double noiseInitialPos, noiseInitialOri, noiseInitialVel, noiseInitialPosTrail, noiseInitialOriTrail;
    double noiseInitialBGA, noiseInitialBAA, noiseInitialBAT, noiseInitialSFT;
    double noiseProcessAcc, noiseProcessGyro, noiseProcessBAA, noiseProcessBGA;
    double noiseProcessBAARev, noiseProcessBGARev;
} hv_ekf_params;

void hv_ekf_default_params(hv_ekf_params *p);
/* EKF::build (ekf.cpp:153-296, 1087-1092): initial m, P, Q as the reference constructor.
 * An hv_ekf must be destroyed before the hv_ctx it was created on. */
int hv_ekf_create(hv_ctx *ctx, const hv_ekf_params *params, int batch, hv_ekf **out);
void hv_ekf_destroy(hv_ekf *ekf);
int hv_ekf_state_dim(const hv_ekf *ekf);                         /* getStateDim            */
int hv_ekf_batch(const hv_ekf *ekf);
/* setState / setStateCovariance / getState / getStateCovariance (ekf.cpp:950-979); either
 * pointer may be NULL. Synchronous. Also the route for the rare mean-side edits the adapter does
 * on the host (lockBiases, conditionOnLastPose, insertMapPoint, setInertialState, translateTo). A batch of resident sequences
 * does not come here for initializeOrientation or for a reset: hv_session_imu_dev and hv_session_reset_dev do both in place. */
int hv_ekf_set_state(hv_ekf *ekf, int filter, const double *m, const double *P_colmajor);
int hv_ekf_get_state(hv_ekf *ekf, int filter, double *m, double *P_colmajor);
int hv_ekf_get_means(hv_ekf *ekf, double *m_all /* batch * n */);
int hv_ekf_set_process_noise(hv_ekf *ekf, int filter, const double *Q12x12);   /* setProcessNoise */
int hv_ekf_get_process_noise(hv_ekf *ekf, int filter, double *Q12x12);
int hv_ekf_get_dydx(hv_ekf *ekf, int filter, double *dydx20x20);               /* getDydx block   */
/* device addresses of the means (batch x n) and covariances (batch x n x n). hv_ekf_augment and
 * hv_ekf_undo_augment ping-pong between two covariance buffers: fetch P_dev again after either. */
int hv_ekf_device_pointers(hv_ekf *ekf, double **m_dev, double **P_dev);
/* predict (ekf.cpp:320-514): mean, Jacobians and P <- F P F' + L Q L' on the device. dt[f] <= 0
 * skips filter f. gyro/acc: [batch][3]. */
int hv_ekf_predict(hv_ekf *ekf, const double *dt, const double *gyro, const double *acc);
int hv_ekf_predict_dev(hv_ekf *ekf, const double *dt_dev, const double *gyro_dev, const double *acc_dev);
/* n_samples consecutive predicts (the IMU samples between two camera frames) in ONE launch: arrays are
 * [n_samples][batch] (dt) and [n_samples][batch][3]. The mean / Jacobian chain and the 20 x 20 block
 * run per sample on chip; the off-diagonal covariance blocks see the product of the samples' F once.
 * Equal to n_samples calls of hv_ekf_predict_dev up to rounding (1e-15 relative). */
int hv_ekf_predict_n_dev(hv_ekf *ekf, int n_samples, const double *dt_dev, const double *gyro_dev,
                         const double *acc_dev);
#define HV_EKF_MAX_PREDICT_SAMPLES 32
int hv_ekf_predict_n(hv_ekf *ekf, int n_samples, const double *dt, const double *gyro, const double *acc);   /* host arrays */
/* update(m,P,y,H,R,...) (ekf.cpp:57-82) with truncated H (n_rows x l, column-major, per filter),
 * R = r_diag[f] * I: used by ZUPT / ZRUPT / position / height / orientation updates. */
int hv_ekf_update(hv_ekf *ekf, int n_rows, int l, const double *H, const double *y, const double *r_diag,
                  const unsigned char *active /* optional [batch] */, int normalize_all_quaternions);
/* visualTrackOutlierCheck (ekf.cpp:787-819) given v = y - f: chi2[f] = noiseScale * v' S^-1 v and
 * status[f] = 0 (INLIER) / 3 (CHI2, chi2 > chi2inv95[n_rows]). Does not modify the filter. Synchronous.
 * n_rows must be < 201 (the size of the reference's chi2inv95 table, odometry/util.hpp:23; the reference asserts it):
 * HV_ERR_INVALID otherwise. Only the reference's defaults of the two optional branches are implemented: r > 0 (the
 * r < 0 "visualR-scaled" branch is not) and trackRmseThreshold = -1 (no RMSE test). S must be positive definite
 * (r > 0 guarantees it): where a pivot of the blocked Cholesky is not positive (the reference's pivoted LDLT would carry on) the
 * filter is reported as CHI2 and left untouched, by the gate and by every update entry point. */
int hv_ekf_visual_gate(hv_ekf *ekf, int n_rows, int l, const double *H, const double *v, double r,
                       double *chi2, int *status);
/* updateVisualTrack (ekf.cpp:829-844) given v = y - f; R = r^2 * noiseScale * I. */
int hv_ekf_visual_update(hv_ekf *ekf, int n_rows, int l, const double *H, const double *v, double r,
                         const unsigned char *active);
/* Device-resident variant: mode 0 = gate only, 1 = update, 2 = update only where the gate passes. */
int hv_ekf_visual_dev(hv_ekf *ekf, int n_rows, int l, const double *H_dev, const double *v_dev, double r,
                      int mode, double *chi2_dev, int *status_dev);
/* ---- per-track triangulation + prepareVisualUpdate on the device ----
 * Replaces, for one pose-trail track per filter, the host code between two EKF calls of the visual update loop
 * (src/odometry/backend.cpp:1063-1148): extractCameraPoseTrail (triangulation.cpp:65-103) from the DEVICE mean,
 * Triangulator::triangulate with derivatives (triangulation.cpp:120-407, the iterative default), the depth window,
 * the stereo derivative sum, prepareVisualUpdate (triangulation.cpp:897-987, full-width H). Parameter names are the
 * reference's (codegen/parameter_definitions.c:37-44,163,178-187). */
typedef struct hv_vu_params {
    double triangulationConvergenceThreshold, triangulationConvergenceR, triangulationRcondThreshold;
    unsigned triangulationGaussNewtonIterations;
    double triangulationMinDist, triangulationMaxDist;
    int estimateImuCameraTimeShift;
    int useStereo;
    double imuToCamera[16], secondImuToCamera[16];     /* 4 x 4 homogeneous, row-major (Parameters::imuToCamera) */
    int useLinearTriangulation;                         /* parameter_definitions.c:31 (default false): triangulateLinear instead of the
                                                          iterative PIVO method (triangulation.cpp:146-152, 820-895) */
    /* ABI 3 (r04): the adaptive outlier thresholds of Session::trackerVisualUpdate (backend.cpp:994-996,1159,1192-1193), applied by the
     * FRAME entry points (hv_ekf_visual_frame*): every track the chi2 / RMSE test rejects multiplies both thresholds of ITS filter by
     * the growth factor for the rest of the frame. trackRmseThreshold is in the units of r_gate (the caller divides by the focal length
     * as backend.cpp:995 does); < 0 = no RMSE test (ekf.cpp:797-801), the reference's default -1. Growth factor default 1
     * (parameter_definitions.c:21,27). The per-visit entry points (hv_ekf_visual_track*) apply the RMSE test with the threshold as
     * given and leave the growth to their caller. */
    double trackRmseThreshold, trackOutlierThresholdGrowthFactor;
} hv_vu_params;
void hv_vu_default_params(hv_vu_params *p);
/* odometry::TriangulatorStatus (output.hpp:21-29) and PrepareVuStatus (output.hpp:15-19) */
enum { HV_TRI_OK = 0, HV_TRI_HYBRID = 1, HV_TRI_BEHIND = 2, HV_TRI_BAD_COND = 3, HV_TRI_NO_CONVERGENCE = 4,
       HV_TRI_BAD_DEPTH = 5, HV_TRI_UNKNOWN_PROBLEM = 6,
       HV_TRI_NOT_VISITED = -1 /* not a reference value: the track was not processed (see hv_ekf_visual_track_limited_dev) */ };
enum { HV_PREPARE_VU_OK = 0, HV_PREPARE_VU_ZERO_DEPTH = 1, HV_PREPARE_VU_BEHIND = 2 };
/* All arrays in device memory, one track of n_poses poses per filter:
 *   pose_index_dev [batch][n_poses]            poseTrailIndex of the track (ekf_state_index: 0 = current pose)
 *   features_dev / velocities_dev [batch][ncam * n_poses][2]   normalized image points / their velocities, the first
 *                                              camera's poses then the second's (buildTrackVectors order)
 *   y_dev [batch][2 * ncam * n_poses]          measured points (the y of buildTrackVectors); may be NULL
 * Outputs: H_dev [batch][(2 * ncam * n_poses) x stateDim] column-major, v_dev = y - f, f_dev (may be NULL), pf_dev
 * [batch][3] world point, status_dev [batch][2] = {TriangulatorStatus, PrepareVuStatus}, active_dev (may be NULL)
 * [batch] = 1 where both are OK -- the inputs hv_ekf_visual_dev takes. Asynchronous. */
int hv_ekf_visual_prepare_dev(hv_ekf *ekf, const hv_vu_params *p, int n_poses, const int *pose_index_dev,
                              const double *features_dev, const double *velocities_dev, const double *y_dev,
                              double *H_dev, double *v_dev, double *f_dev, double *pf_dev, int *status_dev,
                              unsigned char *active_dev);
/* The whole per-track step in one call: prepare as above into internal buffers, then the chi2 gate and -- where the
 * triangulation, prepareVisualUpdate and the gate all pass -- updateVisualTrack (backend.cpp:1150-1185 with
 * batchVisualUpdate false). r_gate = trackChiTestOutlierR (the R of visualTrackOutlierCheck), r_update = visualR.
 * status_dev [batch][2] = {TriangulatorStatus, PrepareVuStatus}; gate_status_dev [batch] = VuOutlierStatus (0 INLIER,
 * 3 CHI2, 1 NOT_COMPUTED where the track never reached the gate); chi2_dev / pf_dev may be NULL. Asynchronous. */
int hv_ekf_visual_track_dev(hv_ekf *ekf, const hv_vu_params *p, int n_poses, const int *pose_index_dev,
                            const double *features_dev, const double *velocities_dev, const double *y_dev,
                            double r_gate, double r_update, int *status_dev, int *gate_status_dev, double *chi2_dev,
                            double *pf_dev);
/* The same with the reference's per-frame stopping rule for a BATCH of sequences: success_counter_dev [batch] counts the
 * visual updates applied to each filter (the caller zeroes it at the start of a frame); a filter whose count has reached
 * max_successful (odometry.maxSuccessfulVisualUpdates = 5, parameter_definitions.c:10) is not visited any more
 * (backend.cpp:1233-1238: status {HV_TRI_NOT_VISITED, HV_TRI_NOT_VISITED}, gate NOT_COMPUTED, filter untouched). */
int hv_ekf_visual_track_limited_dev(hv_ekf *ekf, const hv_vu_params *p, int n_poses, const int *pose_index_dev,
                                    const double *features_dev, const double *velocities_dev, const double *y_dev,
                                    double r_gate, double r_update, int *status_dev, int *gate_status_dev, double *chi2_dev,
                                    double *pf_dev, int *success_counter_dev, int max_successful);
/* One track visit of a session with a HYBRID MAP (odometry.hybridMapSize > 0: backend.cpp:1016, 1075-1082, 1146, 1160-1168; ABI 3, r04).
 * map_update_dev [batch]: the map point a mapPointUpdate track belongs to (>= 0), -1 for a pose-trail track. Such a track is not
 *   triangulated: the point is the state m[stateDim - 3 hybridMapSize + 3 idx ..], status {HV_TRI_HYBRID, prepare status}, H carries
 *   dip R in the point's three columns and no point-derivative terms (triangulation.cpp:968-985); gate and update as usual.
 * map_offer_dev [batch]: the slot ekfStateIndex.offerMapPoint hands to this (pose-trail) track if the gate accepts it, -1: none --
 *   the offer depends on the track and the index, not on the filter, so the adapter evaluates it before the call. Such an inlier is
 *   inserted as a map point (insertMapPoint, ekf.cpp:911-921) INSTEAD of being applied; its gate status reads INLIER.
 * Either array may be NULL. Dense kernels (state wider than 160 columns); trackRmseThreshold < 0 only. Asynchronous. */
int hv_ekf_visual_track_hybrid_dev(hv_ekf *ekf, const hv_vu_params *p, int n_poses, const int *pose_index_dev, const double *features_dev,
                                   const double *velocities_dev, const double *y_dev, const int *map_update_dev, const int *map_offer_dev,
                                   double r_gate, double r_update, int *status_dev, int *gate_status_dev, double *chi2_dev, double *pf_dev);
/* The whole visual-update loop of one frame (Session::trackerVisualUpdate, backend.cpp:1012-1252, with batchVisualUpdate false)
 * in ONE call: n_tracks track visits in the caller's order (the reference's score order), each seeing the mean the previous one
 * left, a filter leaving the loop after max_successful applied updates. Arrays are TRACK-major so that a visit is one contiguous
 * batch: pose_index_dev [n_tracks][batch][n_poses], features_dev / velocities_dev [n_tracks][batch][ncam * n_poses][2], y_dev
 * [n_tracks][batch][2 * ncam * n_poses]; outputs status_dev [n_tracks][batch][2], gate_status_dev [n_tracks][batch], chi2_dev
 * (may be NULL) [n_tracks][batch], pf_dev (may be NULL) the triangulated world points. success_counter_dev [batch] is zeroed here and
 * holds the applied updates on return.
 * Nothing crosses the host between the visits; the call is asynchronous and HIP-graph capturable once it has run once
 * (its work buffers are allocated on first use). The adaptive thresholds of backend.cpp:1192-1193 (hv_vu_params::
 * trackOutlierThresholdGrowthFactor != 1, trackRmseThreshold >= 0; gate status 2 = RMSE) are kept per filter on the device; with a
 * growth factor != 1 the loop always runs sequentially (a rejection changes the threshold of the NEXT track).
 * max_successful <= 0 means "no limit" (the reference's maxSuccessfulVisualUpdates <= 0, backend.cpp:1233).
 * With few sequences the loop runs speculatively: each pass prepares and gates every pending track of a filter in parallel against the
 * current (m, P), applies the first inlier in visit order and re-examines only the tracks behind it -- at most min(max_successful,
 * n_tracks) + 1 passes, the same statuses and the same filter as the sequential loop. Which frames take that form:
 *   - longest track <= 48 rows (12 stereo poses): batch * n_tracks <= 256, n_tracks >= 2, trackOutlierThresholdGrowthFactor == 1;
 *   - longest track 49 .. 84 rows (21 stereo poses, the reference's default stereo configuration; r04): batch * n_tracks <= the device's
 *     CU count (256 on MI355X), the same conditions, and the library's default kernel selection (knobs ekf_long_fused != 0,
 *     ekf_spec_split == 0, ekf_spec_mode != 3, ekf_no_speculation == 0);
 *   - every other frame (more filters, adaptive thresholds) runs the sequential visit loop, with the same results.
 * chi2_dev / pf_dev entries of tracks the loop never visits (status HV_TRI_NOT_VISITED) are 0.
 * hv_vu_params: always start from hv_vu_default_params() -- fields added in later ABI versions then hold their defaults. */
int hv_ekf_visual_frame_dev(hv_ekf *ekf, const hv_vu_params *p, int n_tracks, int n_poses, const int *pose_index_dev,
                            const double *features_dev, const double *velocities_dev, const double *y_dev, double r_gate,
                            double r_update, int *status_dev, int *gate_status_dev, double *chi2_dev, double *pf_dev /* [n_tracks][batch][3] or NULL */,
                            int *success_counter_dev, int max_successful);
/* Host-pointer form (arrays track-major as above): what a single session calls once per frame instead of n_tracks round trips
 * through hv_ekf_visual_track. chi2, pf and success_count may be NULL. Synchronous. */
/* The same loop over RAGGED tracks: the sequences of a batch do not share track lengths (nor the number of candidate tracks).
 * n_poses_dev [n_tracks][batch]: poses of every (visit, filter) track, 2 .. n_poses_max; anything else (0) = this filter has no
 * track at this visit (its statuses read HV_TRI_NOT_VISITED, nothing is gated). Every other array keeps the layout of
 * hv_ekf_visual_frame_dev with n_poses_max as the record size: a track's poses (first camera's, then the second's) sit at the
 * start of its record, the rest is padding. */
int hv_ekf_visual_frame_ragged_dev(hv_ekf *ekf, const hv_vu_params *p, int n_tracks, int n_poses_max, const int *n_poses_dev,
                                   const int *pose_index_dev, const double *features_dev, const double *velocities_dev,
                                   const double *y_dev, double r_gate, double r_update, int *status_dev, int *gate_status_dev,
                                   double *chi2_dev, double *pf_dev, int *success_counter_dev, int max_successful);
/* Session::trackerVisualUpdate with batchVisualUpdate -- or on a frame that is not a "full visual update" -- (backend.cpp:1001-1010,
 * 1169-1183, 1255-1262; ABI 3, r04): the inliers' blocks [H; f; y] are collected and applied as ONE updateVisualTrack per batch; a block
 * that would take the batch beyond max_update_rows flushes it first and opens the next one. Every track between two flushes is prepared
 * and gated against the same state, which the device does in one launch per batch (<= quota + 1 passes per frame). Arguments as
 * hv_ekf_visual_frame_ragged_dev (n_poses_dev may be NULL: every track has n_poses_max poses); max_update_rows = int(stateDim *
 * batchVisualUpdateMaxSizeMultiplier + 0.5), <= 0: stateDim. Valid for trackOutlierThresholdGrowthFactor 1 (HV_ERR_UNSUPPORTED
 * otherwise), n_tracks <= 64, n_tracks * batch <= 8192, max_update_rows >= the rows of the longest track and <= stateDim. */
int hv_ekf_visual_frame_batch_dev(hv_ekf *ekf, const hv_vu_params *p, int n_tracks, int n_poses_max, const int *n_poses_dev,
                                  const int *pose_index_dev, const double *features_dev, const double *velocities_dev, const double *y_dev,
                                  double r_gate, double r_update, int *status_dev, int *gate_status_dev, double *chi2_dev, double *pf_dev,
                                  int *success_counter_dev, int max_successful, int max_update_rows);
/* Reads (and clears) the error word of the filter batch: non-zero when a device-side wait of an asynchronous frame call gave up
 * (only the experimental hand-shake form of the speculative pass, knob ekf_spec_mode = 3, can raise it); the host-pointer entry
 * points check it themselves and return HV_ERR_TIMEOUT. Synchronous. */
int hv_ekf_frame_error(hv_ekf *ekf, int *flags);
int hv_ekf_visual_frame(hv_ekf *ekf, const hv_vu_params *p, int n_tracks, int n_poses, const int *pose_index, const double *features,
                        const double *velocities, const double *y, double r_gate, double r_update, int *status, int *gate_status,
                        double *chi2, double *pf, int *success_count, int max_successful);
/* host-pointer form of hv_ekf_visual_frame_ragged_dev (n_poses [n_tracks][batch] in host memory); synchronous */
int hv_ekf_visual_frame_ragged(hv_ekf *ekf, const hv_vu_params *p, int n_tracks, int n_poses_max, const int *n_poses, const int *pose_index,
                               const double *features, const double *velocities, const double *y, double r_gate, double r_update,
                               int *status, int *gate_status, double *chi2, double *pf, int *success_count, int max_successful);
/* host-pointer form of hv_ekf_visual_frame_batch_dev (ABI 4): what a single session with batchVisualUpdate calls once per frame
 * (backend.cpp:1001-1010,1169-1183,1255-1262). n_poses may be NULL (every track has n_poses_max poses). Synchronous. */
int hv_ekf_visual_frame_batch(hv_ekf *ekf, const hv_vu_params *p, int n_tracks, int n_poses_max, const int *n_poses, const int *pose_index,
                              const double *features, const double *velocities, const double *y, double r_gate, double r_update,
                              int *status, int *gate_status, double *chi2, double *pf, int *success_count, int max_successful,
                              int max_update_rows);
/* host-pointer form of hv_ekf_visual_track_hybrid_dev (ABI 4): one track visit per filter with the hybrid-map branches
 * (backend.cpp:1075-1082 mapPointUpdate tracks, :1146-1168 insertMapPoint for an offered slot). map_update / map_offer [batch] or NULL.
 * chi2 / pf may be NULL. Synchronous. */
int hv_ekf_visual_track_hybrid(hv_ekf *ekf, const hv_vu_params *p, int n_poses, const int *pose_index, const double *features,
                               const double *velocities, const double *y, const int *map_update, const int *map_offer, double r_gate,
                               double r_update, int *status, int *gate_status, double *chi2, double *pf);
/* EKF::insertMapPoint / getMapPoint (ekf.hpp:129-131, ekf.cpp:905-921) on the resident state of filter `filter` (ABI 4): the slot's rows
 * and columns of P are zeroed, 1e6 goes on its diagonal, pf into the mean -- 24 bytes cross the bus instead of the covariance twice.
 * insert is asynchronous (pf is read before the call returns), get synchronous. map_index in [0, hybridMapSize). */
int hv_ekf_insert_map_point(hv_ekf *ekf, int filter, int map_index, const double *pf);
int hv_ekf_get_map_point(hv_ekf *ekf, int filter, int map_index, double *pf);
/* Host-pointer form of hv_ekf_visual_track_dev (arrays [batch][...] as above): about 1 KB per track goes to the device
 * and 40 bytes come back, instead of the mean coming back and a (2 * ncam * n_poses) x stateDim Jacobian going up.
 * chi2 / pf may be NULL. Synchronous. */
int hv_ekf_visual_track(hv_ekf *ekf, const hv_vu_params *p, int n_poses, const int *pose_index, const double *features,
                        const double *velocities, const double *y, double r_gate, double r_update, int *status,
                        int *gate_status, double *chi2, double *pf);
/* updateVisualPoseAugmentation(discarded[f]) (ekf.cpp:848-885; -1 = last pose) incl. the Joseph form,
 * maintainPositiveSemiDefinite and normalizeQuaternions; updateUndoAugmentation (ekf.cpp:888-903). */
int hv_ekf_augment(hv_ekf *ekf, const int *discarded /* [batch] or NULL */, const unsigned char *active);
/* The same with device arrays (either may be NULL): no host copy, so a batch of sequences stays HIP-graph capturable. */
int hv_ekf_augment_dev(hv_ekf *ekf, const int *discarded_dev, const unsigned char *active_dev);
/* hv_ekf_symmetrize followed by hv_ekf_augment_dev in ONE pass over the covariances (ABI 3, r04): the end of a frame's visual
 * updates (maintainPositiveSemiDefinite, backend.cpp:1267) and the pose augmentation that follows it. The augmentation reads
 * every covariance element together with its mirror, so (P + P') / 2 is formed on the fly; results are bit-identical to the
 * two calls in sequence (tests/test_gpu_ekf.py), inactive filters come out symmetrised and otherwise untouched. */
int hv_ekf_symmetrize_augment_dev(hv_ekf *ekf, const int *discarded_dev, const unsigned char *active_dev);
/* host-array form (ABI 4): maintainPositiveSemiDefinite + updateVisualPoseAugmentation as the backend issues them at the end of a frame
 * (backend.cpp:1267, 804-805). States with map points fall back to the two separate calls (same results). */
int hv_ekf_symmetrize_augment(hv_ekf *ekf, const int *discarded /* [batch] or NULL */, const unsigned char *active);
int hv_ekf_undo_augment(hv_ekf *ekf, const unsigned char *active);
int hv_ekf_symmetrize(hv_ekf *ekf);                                 /* maintainPositiveSemiDefinite */
int hv_ekf_normalize_quaternions(hv_ekf *ekf, int only_current);    /* ekf.cpp:1024-1032            */
/* transformTo (ekf.cpp:704-758): the adapter computes pChangeMat (3x3), qChangeMat (4x4) (both
 * row-major) and the translation from the host mirror; the device applies m = A m, P = A P A'. */
int hv_ekf_transform(hv_ekf *ekf, int filter, const double *pChange3x3, const double *qChange4x4,
                     const double *translation3);

/* ---- GFTT feature detector ----------------------------------------
 * Replaces tracker::FeatureDetector (featureDetector "GPU-GFTT" on its CPU path:
 * src/tracker/feature_detector.cpp:279-315 cv::cornerMinEigenVal, :393-417 CollectMax, :610-634
 * detect(); src/tracker/feature_detector_legacy.cpp:177-213 applyMinDistance). Field names are the
 * reference's parameters (codegen/parameter_definitions.c:262,317-324). */
typedef struct hv_gftt_params {
    int    gfttBlockSize;      /* box filter of the structure matrix: 3 (default; tuned kernels), 5 or 7 (plain kernel) */
    double gfttMinDistance;    /* selects the arg-max block edge: >= 32 -> 32, >= 16 -> 16, else 8          */
    float  gfttMinResponse;    /* key points need 16 * minEigenVal > this                                   */
    int    maxTracks;          /* applyMinDistance stops after this many corners                            */
} hv_gftt_params;
void hv_gftt_default_params(hv_gftt_params *p);
int hv_gftt_block_size(const hv_gftt_params *p);                    /* CollectMax::blockSize()            */
int hv_gftt_keypoint_count(hv_ctx *ctx, const hv_gftt_params *p);   /* floor(w/bs) * floor(h/bs)          */
/* FeatureDetector::detect(image, corners, prevCorners, maskRadius) on the level-0 image of a pyramid
 * slot that has been built (or is being built on the context stream): response + block arg-max on
 * the device, then the reference's host tail (stable sort by response, one (0,0) point prepended per
 * key point -- feature_detector.cpp:629-631 --, applyMinDistance when mask_radius > 0). corners_xy
 * must hold 2 * hv_gftt_keypoint_count() points. Synchronous. */
int hv_gftt_detect(hv_ctx *ctx, const hv_gftt_params *p, int slot, const float *prev_xy, int n_prev,
                   int mask_radius, float *corners_xy, int capacity, int *n_out);
/* Device half only, batched: kp_dev[n_images][hv_gftt_keypoint_count()][3] = (x, y, 16 * response) per
 * block in block raster order ((0, 0, -1e10) where no pixel exceeds gfttMinResponse). Asynchronous. */
int hv_gftt_keypoints_batch_dev(hv_ctx *ctx, const hv_gftt_params *p, int n_images, const int *slots_dev,
                                float *kp_dev);
/* FeatureDetector::applyMinDistance (host only, no device work): in place, *n_inout updated. */
void hv_apply_min_distance(float *corners_xy, int *n_inout, const float *prev_xy, int n_prev, int r,
                           int max_tracks);

/* ---- device tail of detect(): stable sort, zero prefix, min-distance filter and track cap (added within ABI 4) ----------
 * The batched, asynchronous forms of the host tail above: n_sets independent sets, one workgroup each, on the context stream
 * with no allocation or synchronisation inside (capturable in a HIP graph). Bit-identical to hv_gftt_detect /
 * hv_apply_min_distance: the same points in the same order with the same count (the distance test is the reference's binary32
 * `dx*dx + dy*dy < (float)(r*r)`, two rounded products and one rounded sum, never contracted).
 * Layouts: set s has n_*_dev[s] entries (clamped to [0, max_*]) at s * max_* of its array; the radius is per set
 * (TrackerImplementation::maskRadius depends on the tracker's adaptive maskScale, tracker.cpp:569-576).
 * Checks made before the context is looked at: HV_ERR_INVALID for NULL required arrays or parameters, negative sizes or
 * max_tracks < 1; HV_ERR_UNSUPPORTED for n_sets > 65535, max_prev > HV_DETECT_TAIL_MAX_PREV, max_tracks >
 * HV_DETECT_TAIL_MAX_TRACKS or max_corners > HV_DETECT_TAIL_MAX_CORNERS; with the context,
 * HV_ERR_UNSUPPORTED for more than HV_DETECT_TAIL_MAX_KEYPOINTS key points per image. */
#define HV_DETECT_TAIL_MAX_KEYPOINTS 16384   /* per image: 1280 x 720 at block edge 8 has 14 400 */
#define HV_DETECT_TAIL_MAX_CORNERS   32768   /* max_corners of every entry: 2 * HV_DETECT_TAIL_MAX_KEYPOINTS */
#define HV_DETECT_TAIL_MAX_PREV      4096    /* live tracks per set */
#define HV_DETECT_TAIL_MAX_TRACKS    4096    /* maxTracks / max_tracks */
/* FeatureDetector::applyMinDistance (feature_detector_legacy.cpp:177-213) on arbitrary lists, the second branch of
 * findKeypoints (image.cpp:77: pending corners against the current mask): corners_dev [n_sets][max_corners][2] is filtered in
 * place against prev_dev [n_sets][max_prev][2] (NULL, with n_prev_dev, allowed when max_prev == 0) and the corners kept so far,
 * stopped at max_tracks; n_out_dev[s] = the kept count, entries at and beyond it are unspecified. radius_dev[s] <= 0: the first
 * min(n, max_tracks) corners are kept. */
int hv_apply_min_distance_batch_dev(hv_ctx *ctx, int n_sets, int max_corners, const int *n_corners_dev, float *corners_dev,
                                    int max_prev, const int *n_prev_dev, const float *prev_dev, const int *radius_dev,
                                    int max_tracks, int *n_out_dev);
/* The tail of FeatureDetectorImplementation::detect (feature_detector.cpp:624-633) on the key points of
 * hv_gftt_keypoints_batch_dev, kp_dev [n_images][hv_gftt_keypoint_count()][3]: stable sort by descending response (equal
 * responses, -0.0 and +0.0 among them, keep block raster order), one (0, 0) point in front per key point (:629-631),
 * applyMinDistance with mask_radius_dev[s] against the image's live tracks, stopped at p->maxTracks. corners_dev
 * [n_images][max_corners][2], n_out_dev[s] = the corner count. Capacity: max_corners >= min(maxTracks, 2 nk) is required
 * (HV_ERR_INVALID below it), which holds every result of a radius > 0. A set with radius <= 0 has all 2 nk points as its
 * result, uncapped, exactly as hv_gftt_detect returns them: where max_corners < 2 nk such a set writes no corner and reports
 * n_out_dev[s] = -1 (the radii are device data, so the host cannot refuse it). */
int hv_gftt_corners_batch_dev(hv_ctx *ctx, const hv_gftt_params *p, int n_images, const float *kp_dev, int max_prev,
                              const int *n_prev_dev, const float *prev_dev, const int *mask_radius_dev, int max_corners,
                              float *corners_dev, int *n_out_dev);
/* hv_gftt_keypoints_batch_dev followed by hv_gftt_corners_batch_dev on the context stream: FeatureDetector::detect of
 * n_images pyramid slots (slots_dev [n_images]) with no host step. kp_dev [n_images][nk][3] is workspace and by-product. */
int hv_gftt_detect_batch_dev(hv_ctx *ctx, const hv_gftt_params *p, int n_images, const int *slots_dev, float *kp_dev,
                             int max_prev, const int *n_prev_dev, const float *prev_dev, const int *mask_radius_dev,
                             int max_corners, float *corners_dev, int *n_out_dev);

/* ---- FAST feature detector: segment test, score, non-max suppression, track mask, detect() tail (added within ABI 4) ------
 * Replaces tracker::FeatureDetector with featureDetector "FAST" (src/tracker/feature_detector.cpp:659-680 FeatureDetector::build;
 * src/tracker/feature_detector_legacy.cpp:141-174 CustomFastFeatureDetector = cv::FastFeatureDetector, FAST-9 on the 16-pixel
 * circle with non-max suppression; :20-51, :70-83 MaskedFeatureDetector::detect / setMask / drawMask; :177-213 applyMinDistance;
 * codegen/parameter_definitions.c:310-311) on the level-0 image of pyramid slots. The rules, restated in
 * tests/fast_restatement.py (written from the algorithm; not pinned against an OpenCV build):
 *   corner   a pixel v, 3 <= x <= w - 4, 3 <= y <= h - 4, with 9 consecutive circle pixels all > v + threshold or all < v - threshold;
 *   score    the largest threshold at which it still is one (threshold .. 254); kept when strictly above its 8 neighbours' scores;
 *   mask     every live track (px, py) with 0 < px < w and 0 < py < h (binary32; NaN draws nothing) removes the key points in
 *            columns [max(ix - r, 0), min(ix + r, w - 1)) and the like rows, ix = (int)px: the upper end is exclusive;
 *   tail     std::stable_sort by descending score (equal scores keep row-major order; no zero prefix, that is GPU-GFTT's alone),
 *            then applyMinDistance(corners, {}, maskRadius) stopped at maxTracks, the distance test of the section above.
 * Everything is asynchronous on the context stream with no allocation or synchronisation inside (capturable in a HIP graph),
 * two launches per call, timed under HV_K_GFTT (score map) and HV_K_DETECT_TAIL (mask, counting sort, walk).
 * Checks made before the context is looked at: HV_ERR_INVALID for NULL required pointers, negative sizes, maxTracks < 1,
 * threshold outside 0 .. 255 or max_corners < min(maxTracks, max_keypoints) (hv_fast_detect also for mask_radius < 1); then
 * HV_ERR_UNSUPPORTED for n_images > 65535, max_prev > HV_DETECT_TAIL_MAX_PREV or maxTracks > HV_DETECT_TAIL_MAX_TRACKS.
 * Counts read from device memory are clamped to their capacity. The radius is device data: a set with mask_radius_dev[s] < 1
 * (where the reference asserts) writes no row and reports n_kp_dev[s] = n_out_dev[s] = -1. An image with more key points than
 * max_keypoints, or whose slot is no valid slot (or holds no image), reports n_kp_dev[s] = -1 and n_out_dev[s] = -1 and writes
 * no row either: it is never truncated, because the sort would then pick other corners. max_keypoints =
 * hv_fast_keypoint_bound() cannot overflow. With the context: HV_ERR_UNSUPPORTED for images of more than about 2^27 pixels
 * ((w + 259) * h > 2^27; the select kernel's packed indices). A context that runs both detectors reads the sums of both under
 * HV_K_GFTT and HV_K_DETECT_TAIL. */
#define HV_FAST_TILE_W 64   /* the score kernel's tile (one workgroup); tests place their cases across its seams */
#define HV_FAST_TILE_H 16
typedef struct hv_fast_params {
    int threshold;   /* 10: cv::FastFeatureDetector::create() */
    int maxTracks;   /* 200: applyMinDistance stops after this many corners (parameter_definitions.c:262) */
} hv_fast_params;
void hv_fast_default_params(hv_fast_params *p);
void hv_fast_tile_size(int *tile_w, int *tile_h);      /* HV_FAST_TILE_W, HV_FAST_TILE_H as the library was built */
int hv_fast_keypoint_bound(hv_ctx *ctx);               /* ceil((w-6)/2) * ceil((h-6)/2): suppressed key points are never 8-adjacent */
size_t hv_fast_work_bytes(hv_ctx *ctx, int n_images);  /* the score maps, one byte per pixel (the histograms stay in LDS) */
/* cv::FastFeatureDetector::detect without a mask: kp_dev [n_images][max_keypoints][3] = (x, y, score) in row-major order (y, then
 * x, ascending), n_kp_dev [n_images]; work_dev: hv_fast_work_bytes(ctx, n_images) bytes, 16-byte aligned. */
int hv_fast_keypoints_batch_dev(hv_ctx *ctx, const hv_fast_params *p, int n_images, const int *slots_dev, void *work_dev,
                                int max_keypoints, float *kp_dev, int *n_kp_dev);
/* FeatureDetector::detect of the FAST detector, no host step. kp_dev / n_kp_dev: by-product, the key points that survived the
 * mask, in sorted order. prev_dev [n_images][max_prev][2] with n_prev_dev [n_images] (both NULL allowed when max_prev == 0),
 * mask_radius_dev [n_images], corners_dev [n_images][max_corners][2], n_out_dev [n_images]. */
int hv_fast_detect_batch_dev(hv_ctx *ctx, const hv_fast_params *p, int n_images, const int *slots_dev, void *work_dev,
                             int max_keypoints, float *kp_dev, int *n_kp_dev, int max_prev, const int *n_prev_dev,
                             const float *prev_dev, const int *mask_radius_dev, int max_corners, float *corners_dev,
                             int *n_out_dev);
/* One image, host pointers, synchronous (staged through the context's arena, hv_stage.hpp): capacity >= min(maxTracks,
 * hv_fast_keypoint_bound()) corners (HV_ERR_INVALID below it); HV_ERR_POOL for a slot that is not in use or holds no image. */
int hv_fast_detect(hv_ctx *ctx, const hv_fast_params *p, int slot, const float *prev_xy, int n_prev, int mask_radius,
                   float *corners_xy, int capacity, int *n_out);

/* ---- legacy GFTT feature detector: cv::goodFeaturesToTrack behind the track mask (added within ABI 4) ---------------------
 * Replaces tracker::FeatureDetector with featureDetector "GFTT" (src/tracker/feature_detector.cpp:659-680 FeatureDetector::build;
 * src/tracker/feature_detector_legacy.cpp:53-139 GFTTFeatureDetector = cv::GFTTDetector, i.e. cv::goodFeaturesToTrack(gray,
 * corners, maxTracks, gfttQualityLevel, minDistance, mask, gfttBlockSize, 3, false); :20-51 MaskedFeatureDetector::detect /
 * setMask / drawMask; codegen/parameter_definitions.c:310-311) on the level-0 image of pyramid slots. The rules, restated in
 * tests/gftt_legacy_restatement.py (written from the algorithm of OpenCV 4.x; not pinned against an OpenCV build):
 *   mask        every live track (px, py) with 0 < px < w and 0 < py < h (binary32; NaN draws nothing) masks columns
 *               [max(ix - r, 0), min(ix + r, w - 1)) and the like rows, ix = (int)px: the upper end is exclusive;
 *   response    eig = cv::cornerMinEigenVal(gray, gfttBlockSize, 3), binary32, the operation order of oracle/gftt_oracle.c;
 *   threshold   maxVal = the maximum of eig over the unmasked pixels of the whole image (0 when there is none),
 *               t = (float)((double)maxVal * gfttQualityLevel), eig[p] = eig[p] > t ? eig[p] : 0 at every pixel, masked or not;
 *   candidates  (x, y), 1 <= x <= w - 2, 1 <= y <= h - 2, unmasked, whose thresholded value v is not 0 and equals the maximum of
 *               the thresholded values of its 3 x 3 neighbourhood (masked neighbours suppress; equal neighbours are both candidates);
 *   order       descending v; among equal v the larger raster index y * w + x first (OpenCV 4.x's greaterThanPtr);
 *   walk        minDistance = gfttMinDistance * (min(w, h) / 720.0) in binary64. minDistance >= 1: a candidate is accepted unless
 *               an accepted corner lies at dx dx + dy dy < minDistance^2 (integer coordinates); minDistance < 1: every candidate is
 *               accepted; either way the walk stops at maxTracks corners. The corners are (float)x, (float)y in acceptance order:
 *               no applyMinDistance and no zero prefix behind it.
 * Everything is asynchronous on the context stream with no allocation or synchronisation inside (capturable in a HIP graph): one
 * memset and three launches per call, timed under HV_K_GFTT (mask, response, candidates) and HV_K_DETECT_TAIL (order and walk).
 * The result is deterministic: the order in which candidates are appended to the work memory is not, and the select kernel sorts.
 * Checks made before the context is looked at: HV_ERR_INVALID for NULL required pointers, negative sizes, maxTracks < 1,
 * gfttQualityLevel <= 0, gfttMinDistance < 0 or max_corners < min(maxTracks, max_keypoints) (hv_gftt_legacy_detect also for
 * mask_radius < 1); then HV_ERR_UNSUPPORTED for a gfttBlockSize other than 3, 5 and 7, n_images > 65535, max_prev >
 * HV_DETECT_TAIL_MAX_PREV or maxTracks > HV_DETECT_TAIL_MAX_TRACKS. With the context: HV_ERR_UNSUPPORTED for an image edge below
 * 8 (one reflection serves every halo) or above 32767 (the walk's squared distances are 32-bit integers). Counts read from device
 * memory are clamped to their capacity. The radius is device data: a set with mask_radius_dev[s] < 1 (where the reference
 * asserts), a set whose slot is no valid slot or holds no image, and a set with more candidates than max_keypoints write no row
 * and report n_cand_dev[s] = n_out_dev[s] = -1: never truncated, because the order would then pick other corners.
 * max_keypoints = hv_gftt_legacy_keypoint_bound() cannot overflow. The select kernel itself has no limit below that: it takes
 * the keys from the top in groups of at most 4096, and a group of equal responses larger than that is split by raster index. */
#define HV_GFTT_LEGACY_TILE_W 64   /* the tile of the response and candidate kernels (one workgroup); tests place their cases across its seams */
#define HV_GFTT_LEGACY_TILE_H 16
typedef struct hv_gftt_legacy_params {
    int    gfttBlockSize;      /* 3: the box of cv::cornerMinEigenVal; 3, 5 and 7 are built (parameter_definitions.c)          */
    double gfttQualityLevel;   /* 0.01: candidates lie above this share of the masked maximum                                   */
    double gfttMinDistance;    /* 50: pixels at 720p, scaled by min(w, h) / 720 (feature_detector_legacy.cpp:53-68)             */
    int    maxTracks;          /* 200: maxCorners of cv::goodFeaturesToTrack                                                    */
} hv_gftt_legacy_params;
void hv_gftt_legacy_default_params(hv_gftt_legacy_params *p);
void hv_gftt_legacy_tile_size(int *tile_w, int *tile_h);   /* HV_GFTT_LEGACY_TILE_W, HV_GFTT_LEGACY_TILE_H as the library was built */
double hv_gftt_legacy_min_distance(hv_ctx *ctx, const hv_gftt_legacy_params *p);   /* the scaled binary64 distance (-1: NULL argument) */
int hv_gftt_legacy_keypoint_bound(hv_ctx *ctx);             /* (w - 2)(h - 2): candidates lie inside the 1-pixel border */
/* header, max_keypoints 64-bit keys, the response map (4 bytes per pixel) and the mask (1 byte per pixel) per image */
size_t hv_gftt_legacy_work_bytes(hv_ctx *ctx, int n_images, int max_keypoints);
/* MaskedFeatureDetector::detect of the GFTT detector (feature_detector_legacy.cpp:20-51, :53-139), no host step. work_dev:
 * hv_gftt_legacy_work_bytes(ctx, n_images, max_keypoints) bytes, 16-byte aligned. prev_dev [n_images][max_prev][2] with
 * n_prev_dev [n_images] (both NULL allowed when max_prev == 0), mask_radius_dev [n_images], corners_dev
 * [n_images][max_corners][2], resp_dev [n_images][max_corners] or NULL (the responses of the accepted corners, OpenCV's
 * cornersQuality), n_cand_dev [n_images] (the candidate count before the walk), n_out_dev [n_images]. */
int hv_gftt_legacy_detect_batch_dev(hv_ctx *ctx, const hv_gftt_legacy_params *p, int n_images, const int *slots_dev, void *work_dev,
                                    int max_keypoints, int *n_cand_dev, int max_prev, const int *n_prev_dev, const float *prev_dev,
                                    const int *mask_radius_dev, int max_corners, float *corners_dev, float *resp_dev,
                                    int *n_out_dev);
/* The same without live tracks: cv::goodFeaturesToTrack with no mask (feature_detector_legacy.cpp:53-139). */
int hv_gftt_legacy_keypoints_batch_dev(hv_ctx *ctx, const hv_gftt_legacy_params *p, int n_images, const int *slots_dev,
                                       void *work_dev, int max_keypoints, int *n_cand_dev, int max_corners, float *corners_dev,
                                       float *resp_dev, int *n_out_dev);
/* One image, host pointers, synchronous (staged through the context's arena, hv_stage.hpp; feature_detector_legacy.cpp:20-51,
 * :53-139): capacity >= min(maxTracks, hv_gftt_legacy_keypoint_bound()) corners (HV_ERR_INVALID below it); HV_ERR_POOL for a
 * slot that is not in use or holds no image. */
int hv_gftt_legacy_detect(hv_ctx *ctx, const hv_gftt_legacy_params *p, int slot, const float *prev_xy, int n_prev, int mask_radius,
                          float *corners_xy, int capacity, int *n_out);

/* ---- dense stereo depth: StereoBM block matching, speckle filter, track depth, point cloud (added within ABI 4) --------------
 * Replaces tracker.computeDenseStereoDepth (src/tracker/tracker.cpp:532 and :784-796 computeDenseStereoDepth; src/tracker/image.cpp:
 * 108-139, whose line 115 notes "Currently only supported on the CPU, even if rectification was done on the GPU"; all of
 * src/tracker/stereo_disparity.cpp: cv::StereoBM::create(nd) with speckle window 500 and range 10, getDepth :66-77,
 * computePointCloud :79-94; the cloud is what backend.cpp:1328 hands out) on the level-0 images of pyramid slots, the rectified pair
 * the ingest wrote there. The rules, restated in tests/stereo_bm_restatement.py (written from the algorithm; NOT pinned against an
 * OpenCV build -- the doubts: the prefilter's edge rows, the tie order of a SIMD path, the unscaled speckle range, the left edge of
 * the valid rectangle, Eigen's summation order; DESIGN.md lists them under "not pinned"):
 *   prefilter  XSOBEL, out = clamp(S, -c, c) + c; rows mirror without repeating the edge row; columns 0 and W - 1, and the last row
 *              of an odd height, are c;
 *   rectangle  nd - 1 + 10 <= x < W - 10, 10 <= y < H - 10; everything else is FILTERED = -16; output int16 = disparity x 16;
 *   pixel      sad[d] over the 21 x 21 window, textsum < textureThreshold -> FILTERED; the first strictly smallest sad in OpenCV's
 *              index k = nd - 1 - d (a tie goes to the larger disparity); a rival further than 1 away with sad <= m + m * ratio / 100
 *              -> FILTERED; the sub-pixel step ((nd - mink - 1) * 256 + (dd ? (p - n) * 256 / dd : 0) + 15) >> 4;
 *   speckles   4-neighbour components of the pixels != FILTERED joined where |a - b| <= speckleRange (unscaled); a component of
 *              <= speckleWindowSize pixels becomes FILTERED;
 *   getDepth / computePointCloud  binary32: Qf . (x, y, v / 16, 1) summed left to right, IEEE division, sqrt((x^2 + y^2) + z^2).
 * blockSize 21 is the one size served: other odd sizes >= 5 return HV_ERR_UNSUPPORTED, as do numDisparities > 256,
 * uniquenessRatio > 100 and textureThreshold > 65535. Everything `_dev` is asynchronous on the context stream with no allocation or
 * synchronisation inside (capturable in a HIP graph). The image kernels (prefilter, matching, speckles, count) are timed under
 * HV_K_INGEST, the depth and cloud kernels under HV_K_STEREO_GATE. The matching kernel keeps no cost volume in global memory.
 * Checks made before the context is looked at: HV_ERR_INVALID for NULL required pointers, negative sizes, numDisparities not a
 * positive multiple of 16, blockSize even or < 5, preFilterCap outside 1 .. 63, negative textureThreshold / uniquenessRatio,
 * cloud_stride < 1; then HV_ERR_UNSUPPORTED for the limits above and n_sets > 32767 (65535 for the other entries). With the
 * context: HV_ERR_INVALID for a set stride below width * height. */
typedef struct hv_stereo_bm_params {
    int numDisparities;     /* std::ceil(width * 0.1f / 32) * 32 (stereo_disparity.cpp:39): hv_stereo_num_disparities(width) */
    int blockSize;          /* 21 */
    int preFilterCap;       /* 31 */
    int textureThreshold;   /* 10 */
    int uniquenessRatio;    /* 15 */
    int speckleWindowSize;  /* 500 (stereo_disparity.cpp:19); <= 0: no speckle filter */
    int speckleRange;       /* 10 (stereo_disparity.cpp:18); < 0: no speckle filter */
} hv_stereo_bm_params;
#define HV_STEREO_FILTERED (-16)
int hv_stereo_num_disparities(int width);                                      /* 752 -> 96, 1280 -> 128, 320 -> 32, 160 -> 32 */
void hv_stereo_bm_default_params(hv_stereo_bm_params *p, int width);
/* work_dev of hv_stereo_disparity_batch_dev (16-byte aligned): two prefiltered byte planes and the int32 labels and counters of the
 * speckle filter per set; 0 for a NULL context or refused parameters */
size_t hv_stereo_work_bytes(hv_ctx *ctx, const hv_stereo_bm_params *p, int n_sets);
size_t hv_filter_speckles_work_bytes(int width, int height, int n_sets);       /* work_dev of hv_filter_speckles_batch_dev */
int hv_stereo_cloud_bound(hv_ctx *ctx, int cloud_stride);                      /* ceil(W / s) * ceil(H / s): a max_points that cannot overflow */
/* OpenCvStereoDisparity::computeDisparity for n_sets pairs: the level-0 images of left_slots_dev[s] / right_slots_dev[s] ->
 * disp_dev [n_sets][H][W] int16 (set s at disp_dev + s * disp_set_stride elements, rows W apart). The speckle filter runs when
 * speckleWindowSize > 0 && speckleRange >= 0. n_valid_dev (NULL allowed) [n_sets]: the pixels != FILTERED. A set whose slot is no
 * valid slot or holds no image reports -1 and writes nothing. */
int hv_stereo_disparity_batch_dev(hv_ctx *ctx, const hv_stereo_bm_params *p, int n_sets, const int *left_slots_dev,
                                  const int *right_slots_dev, void *work_dev, int16_t *disp_dev, long long disp_set_stride,
                                  int *n_valid_dev);
/* cv::filterSpeckles(disp, new_val, max_size, max_diff) in place on n_sets int16 maps of width x height (any size, not the
 * context's); work_dev: hv_filter_speckles_work_bytes(width, height, n_sets) bytes, 16-byte aligned. */
int hv_filter_speckles_batch_dev(hv_ctx *ctx, int n_sets, int width, int height, int16_t *disp_dev, long long set_stride, int new_val,
                                 int max_size, int max_diff, void *work_dev);
/* getDepth for every track: xy_dev [n_sets][max_points][2], n_points_dev [n_sets] (clamped to 0 .. max_points), depth_dev
 * [n_sets][max_points] binary32, -1 where the reference returns -1 and for a non-finite coordinate or one beyond int range (the
 * reference's cast is undefined there). Q: disparityToDepthQ, 16 row-major doubles on the host, formed by the caller as
 * stereo_rectifier.cpp:64-93 does; it is rounded to binary32 as Q.cast<float>() does. disp_dev / stride: as written above. */
int hv_stereo_track_depth_batch_dev(hv_ctx *ctx, int n_sets, int max_points, const int *n_points_dev, const float *xy_dev,
                                    const int16_t *disp_dev, long long stride, const double *Q, float *depth_dev);
/* computePointCloud: y, then x, in steps of cloud_stride (stereoPointCloudStride, 5); xyz_dev [n_sets][max_points][3] in that
 * row-major order, n_points_dev [n_sets]. A set with more points than max_points reports -1 and writes nothing: never truncated. */
int hv_stereo_point_cloud_batch_dev(hv_ctx *ctx, int n_sets, const int16_t *disp_dev, long long stride, const double *Q,
                                    int cloud_stride, int max_points, float *xyz_dev, int *n_points_dev);
/* One pair, host pointers, synchronous (staged through the context's arena, hv_stage.hpp): disp_host rows `stride` elements apart
 * (>= width); HV_ERR_POOL for a slot that is not in use or holds no image. */
int hv_stereo_disparity(hv_ctx *ctx, const hv_stereo_bm_params *p, int left_slot, int right_slot, int16_t *disp_host,
                        long long stride);
/* getDepth / computePointCloud on a disparity image the caller holds on the host (rows `stride` == width elements apart), one set,
 * synchronous, the image staged through the arena with the points: what the C++ adapter calls. hv_stereo_point_cloud: capacity >=
 * the number of points (hv_stereo_cloud_bound() always is), HV_ERR_INVALID when they do not fit. */
int hv_stereo_track_depth(hv_ctx *ctx, int n_points, const float *xy_host, const int16_t *disp_host, long long stride, const double *Q,
                          float *depth_host);
int hv_stereo_point_cloud(hv_ctx *ctx, const int16_t *disp_host, long long stride, const double *Q, int cloud_stride, float *xyz_host,
                          int capacity, int *n_out);

/* ---- sub-pixel corner refinement (added within ABI 4) ----------------------------------------
 * Replaces tracker::SubPixelAdjuster::adjust (src/tracker/subpixel_adjuster.cpp:18-42): cv::cornerSubPix(image, corners,
 * Size(win, win), Size(-1, -1), TermCriteria(COUNT | EPS, maxIter, epsilon)) on the level-0 image of a pyramid slot, then
 * every refined point outside the image goes back to its input value. Bit-identical to OpenCV 4.x's float / double
 * evaluation order (restated in tests/subpix_restatement.py). Field names are the reference's parameters
 * (codegen/parameter_definitions.c:328-332). The reference builds no adjuster when subPixMaxIter <= 0 (image.cpp:54);
 * these entries clamp it to one iteration, as cornerSubPix does, and leave that choice to the caller.
 * HV_ERR_INVALID: window < 1, or the image is smaller than 2 * win + 5 in either dimension (where OpenCV asserts);
 * HV_ERR_UNSUPPORTED: window > HV_SUBPIX_MAX_WIN (the kernel keeps the (2 win + 1)^2 gradient terms of a corner in LDS).
 * An input point outside [0, w) x [0, h) (OpenCV asserts on it) is returned unchanged with 0 updates. */
#define HV_SUBPIX_MAX_WIN 16
typedef struct hv_subpix_params { int subPixWindowSize; int subPixMaxIter; double subPixEpsilon; } hv_subpix_params;
void hv_subpix_default_params(hv_subpix_params *p);            /* 10, 20, 0.03 (parameter_definitions.c:328-332) */
/* SubPixelAdjuster::adjust on level 0 of `slot`: xy [n][2] in/out; iters [n] (NULL ok) = position updates applied (0 after an
 * immediate det break). n == 0 returns HV_OK after the argument checks. Synchronous. */
int hv_corner_subpix(hv_ctx *ctx, const hv_subpix_params *p, int slot, int n, float *xy, int *iters);
/* n_sets independent point lists, xy_dev [n_sets][max_points][2] in place, n_points_dev [n_sets] (<= max_points; larger values
 * are clamped), slots_dev [n_sets], iters_dev [n_sets][max_points] or NULL; asynchronous on the context stream, no allocation or
 * synchronisation inside (capturable in a HIP graph). A set whose slot is not a valid slot index is left untouched.
 * n_sets <= 65535 (HV_ERR_UNSUPPORTED beyond). */
int hv_corner_subpix_batch_dev(hv_ctx *ctx, const hv_subpix_params *p, int n_sets, const int *slots_dev, int max_points,
                               const int *n_points_dev, float *xy_dev, int *iters_dev);

/* ---- image ingest --------------------------------------------------
 * Replaces the per-frame work of tracker::Image::Factory::build / buildStereo (src/tracker/image.cpp:272-306):
 * the colour -> gray copy (image.cpp:351-367, coefficients 0.299 / 0.587 / 0.114 on channels 0, 1, 2) and
 * tracker::Undistorter::undistort (src/tracker/undistorter.cpp:71-110, the CPU branch: bilinear remap through
 * rectifiedCamera.pixelToRay -> originalCamera.rayToPixel), followed by the pyramid level kernels. The result is
 * level 0 of the slot, so the tracker never sees the raw frame.
 * channels: 1 (gray), 3 (RGB / BGR) or 4 (RGBA / BGRA), 8 bits each, interleaved.
 * camera: -1 = no remap (tracker.useRectification false, the default: parameter_definitions.c:356), otherwise the
 * index (0 first / 1 second camera: image.cpp:322-328) of a table installed with hv_ingest_set_undistort_map. */
#define HV_INGEST_CAMERAS 2
/* Installs (pix_orig_xy != NULL) or removes (NULL) the remap table of one camera. pix_orig_xy[(y*w + x)*2 + {0,1}]
 * = the position in the original image of rectified pixel (x, y), i.e. what undistortCpu (undistorter.cpp:56-60)
 * returns for it, evaluated by the caller with the reference's own Camera objects; valid[y*w + x] = its boolean
 * result (NULL = all true). The cameras are constant for a session, so this runs once (the reference's GPU branch
 * makes the same assumption: undistorter.cpp:113-121). Synchronous. */
int hv_ingest_set_undistort_map(hv_ctx *ctx, int camera, const double *pix_orig_xy, const uint8_t *valid);
/* H2D copy of one host frame + ingest + all pyramid level kernels into `slot`; asynchronous like hv_pyramid_build. */
int hv_ingest_build(hv_ctx *ctx, int slot, const uint8_t *image_host, int stride_bytes, int channels, int camera);
/* n frames resident in HBM (frame i at src_dev + i*image_stride_bytes; base and strides multiples of 4 bytes).
 * Unlike hv_pyramid_build_batch_dev the result is written into the slots, so the frames may be reused at once.
 * Asynchronous. */
int hv_ingest_build_batch_dev(hv_ctx *ctx, int n, const int *slots_dev, const uint8_t *src_dev,
                              long long image_stride_bytes, int row_stride_bytes, int channels, int camera);

/* ---- 2-point rotation RANSAC -----------------------------------------
 * Replaces tracker::rot_ransac::RotRansac::fit (src/tracker/rot_ransac.cpp:41-120) as doRansac2 calls it on the
 * TRACKED features of every frame (src/tracker/ransac_pipeline.cpp:197-216). The camera models are the reference's
 * (src/tracker/camera.cpp): fill the first block of fields and call hv_camera_model_init. */
typedef struct hv_camera_model {
    int kind;                         /* 0 pinhole (radial k1 k2 k3, camera.cpp:93-221), 1 fisheye (k1..k4, :264-398) */
    double fx, fy, ppx, ppy;          /* api::CameraParameters */
    int n_coeffs; double coeffs[4];   /* distortionCoeffs: 0 or 3 (pinhole), 0 or 4 (fisheye) */
    int rotation_enabled; double rotation[9];   /* pinhole only (rectified cameras), row-major */
    double max_valid_fov_deg;         /* fisheye: validCameraFov */
    /* derived by hv_camera_model_init (the constructors of camera.cpp) */
    int distortion_enabled;
    double kinv[9], max_theta, max_r;
    int n_table; double table[50];
} hv_camera_model;
int hv_camera_model_init(hv_camera_model *m);
/* One point set = the n TRACKED features of one frame: c1 / c2 = pixel coordinates in the previous / current frame
 * (cameras[0][0] / cameras[0][1]). pairs[k] = {rng() % n, rng() % n} for k = 0..99 drawn by the caller from its
 * std::mt19937 (rot_ransac.cpp:82-83); afterwards the caller discards nothing and keeps 2 * hypotheses_visited draws
 * consumed (the reference loop stops at the first hypothesis that makes every point an inlier). threshold_pow2 =
 * RotRansac::threshold_pow2 (ransac_pipeline.cpp:91-93). status[i] = 0 TRACKED / 3 RANSAC_OUTLIER (track.hpp:9-21),
 * R = the returned cv::Matx33f (row-major), best_inlier_count = RotRansac::bestInlierCount. Synchronous. */
int hv_rot_ransac(hv_ctx *ctx, int n, const float *c1_xy, const float *c2_xy, const hv_camera_model *camera1,
                  const hv_camera_model *camera2, const int *pairs, float threshold_pow2, int *status, float *R,
                  int *best_inlier_count, int *hypotheses_visited);
/* n_sets point sets in device memory, set s holding n_points_dev[s] <= max_points (<= 1024) points at
 * c*_dev + s * max_points * 2, pairs_dev [n_sets][100][2], status_dev [n_sets][max_points], R_dev [n_sets][9],
 * summary_dev [n_sets][2] = {bestInlierCount, hypotheses_visited}. Sets with fewer than 2 points are skipped
 * (ransac_pipeline.cpp:209). Asynchronous. */
int hv_rot_ransac_batch_dev(hv_ctx *ctx, int n_sets, int max_points, const int *n_points_dev, const float *c1_dev,
                            const float *c2_dev, const hv_camera_model *camera1, const hv_camera_model *camera2,
                            const int *pairs_dev, float threshold_pow2, int *status_dev, float *R_dev, int *summary_dev);

/* The same fed straight from the LK outputs of hv_klt_track_batch_dev, nothing passing through the host: set s = the
 * n_points_dev[s] features of pair s (prev_xy / next_xy / status of the LK call, max_points = pts_per_pair); only features
 * whose lk_status equals lk_tracked_value (1 for hv_klt_track_batch_dev) take part, in feature order -- the c1 / c2 of
 * ransac_pipeline.cpp:106-112. draws_dev [n_sets][200] = the next 200 raw outputs of each set's std::mt19937; the kernel
 * forms rng() % n itself because n is only known on the device. status_dev [n_sets][max_points] is written at the ORIGINAL
 * feature numbers (0 / 3), other entries stay; summary_dev as above. Asynchronous. */
int hv_rot_ransac_lk_batch_dev(hv_ctx *ctx, int n_sets, int max_points, const int *n_points_dev, const float *c1_dev,
                               const float *c2_dev, const uint8_t *lk_status_dev, int lk_tracked_value,
                               const hv_camera_model *camera1, const hv_camera_model *camera2, const uint32_t *draws_dev,
                               float threshold_pow2, int *status_dev, float *R_dev, int *summary_dev);

/* ---- five-point essential-matrix RANSAC and the hybrid RANSAC2 / RANSAC5 filter (added within ABI 4) ---------------
 * Replaces doRansac5 without Theia (src/tracker/ransac_pipeline.cpp:274-397): Camera::normalizePixel of both frames
 * (camera.cpp:471-476; failing points are outliers and take no part), threshold = 2 ransac5Threshold / (f1 + f2) with
 * f = (fx + fy) / 2, then findEssentialMatRansacMaxIter (five_point.cpp:404-416): RANSACPointSetRegistrator::run
 * (ptsetreg.hpp:130-220) with a fresh cv::RNG((uint64)-1), getSubset, Nister's solver (five_point.cpp:41-146), the float
 * Sampson error (:374-400) and RANSACUpdateNumIters (ptsetreg.cpp:58-79). Equal to the numpy restatement in
 * tests/ransac5_restatement.py; where it departs from OpenCV (null-space basis, elimination, solvePoly restated, the
 * null vector of B(z)) see DESIGN.md. Fewer than 5 points or 5 valid ones: not done, every point an outlier. Exactly 5
 * valid points: every valid point an inlier (the single kernel call decides nothing). No model ever qualifying: every
 * valid point an inlier (the pre-filled mask survives). Field names are the reference's parameters
 * (codegen/parameter_definitions.c:268-282). HV_ERR_UNSUPPORTED: ransacMaxIters > HV_RANSAC5_MAX_ITERS or more than
 * 1024 points; HV_ERR_INVALID: ransac5Prob outside (0, 1) (OpenCV asserts) or ransacMaxIters < 1. The parameter and size
 * checks come before the context is looked at. */
#define HV_RANSAC5_MAX_ITERS 75
typedef struct hv_ransac5_params {
    double ransac5Prob; double ransac5Threshold; int ransacMaxIters;
    double ransac2InliersToSkipRansac5; double ransacMinInlierFraction; double ransac2InliersOverRansac5Needed;
} hv_ransac5_params;
void hv_ransac5_default_params(hv_ransac5_params *p);   /* 0.999, 2.0, 75, 0.9, 0.3, 0.9 (parameter_definitions.c:270-282) */
/* doRansac5 on one set of n points (c1 = previous, c2 = current frame pixels, camera1 / camera2 = cameras[0][0] /
 * cameras[0][1]): status[n] 0 TRACKED / 3 RANSAC_OUTLIER, E[9] (row-major, unit norm; zeros without a model; NULL ok),
 * summary[4] (NULL ok) = {inlier count, iteration of the best model (-1: none), iterations run, valid points}.
 * Synchronous. */
int hv_ransac5(hv_ctx *ctx, const hv_ransac5_params *p, int n, const float *c1_xy, const float *c2_xy,
               const hv_camera_model *camera1, const hv_camera_model *camera2, int *status, double *E, int *summary);
/* n_sets sets in device memory: set s = n_points_dev[s] <= max_points (<= 1024) points at c*_dev + s * max_points * 2;
 * status_dev [n_sets][max_points], E_dev [n_sets][9] and summary_dev [n_sets][4] as above (E / summary NULL ok).
 * Asynchronous on the context stream, no allocation or synchronisation inside (capturable in a HIP graph).
 * n_sets <= 65535. */
int hv_ransac5_batch_dev(hv_ctx *ctx, const hv_ransac5_params *p, int n_sets, int max_points, const int *n_points_dev,
                         const float *c1_dev, const float *c2_dev, const hv_camera_model *camera1,
                         const hv_camera_model *camera2, int *status_dev, double *E_dev, int *summary_dev);
/* The mono device chain step after hv_rot_ransac_lk_batch_dev: RansacPipeline::compute on the hybrid path
 * (ransac_pipeline.cpp:95-151, 158-195). Set s = the features of LK pair s: c1 / c2 as for hv_rot_ransac_lk_batch_dev,
 * track_status_dev [n_sets][max_points] int32 Feature::Status (TRACKED = 0 selects the set, in feature order),
 * r2_status_dev / r2_summary_dev = the status_dev / summary_dev of hv_rot_ransac_lk_batch_dev on the same set.
 * RANSAC5 runs unless RANSAC2's bestInlierCount > ransac2InliersToSkipRansac5 * n; the selection follows :174-194.
 * track_status_dev is rewritten at the original feature numbers: the chosen result's outliers -> 3 (updateTrackStatus,
 * :29-40); SKIPPED -> every entry < n_points_dev[s] becomes 3 (:139-144). result_dev [n_sets][2] = {type 0 SKIPPED /
 * 1 R2 / 3 R5, inlierCount}, score_dev [n_sets] = RANSAC2 inliers / n (0 when n == 0), the return value of compute.
 * E_dev / r5_summary_dev (NULL ok) as for hv_ransac5_batch_dev; where RANSAC5 did not run the summary is {0, -1, 0, m}
 * with m = the valid (normalisable) points when n >= 5 and RANSAC2 did not skip it, else m = 0.
 * Asynchronous, capturable. */
int hv_hybrid_ransac_lk_batch_dev(hv_ctx *ctx, const hv_ransac5_params *p, int n_sets, int max_points,
                                  const int *n_points_dev, const float *c1_dev, const float *c2_dev, int *track_status_dev,
                                  const int *r2_status_dev, const int *r2_summary_dev, const hv_camera_model *camera1,
                                  const hv_camera_model *camera2, int *result_dev, double *score_dev, double *E_dev,
                                  int *r5_summary_dev);

/* ---- stereo RANSAC3: P3P absolute-pose track filter (added within ABI 4) ----------------------------------------------
 * Replaces doRansac3 (src/tracker/ransac_pipeline.cpp:218-272) and the RANSAC3 branch of RansacPipeline::compute
 * (:121-123, 137-149) without Theia. Per feature with status TRACKED (0), in feature order: the status becomes
 * RANSAC_OUTLIER (3); Camera::normalizePixel of the previous-left (camera0), previous-right (camera1) and current-left
 * (camera0) corner; triangulateStereoFeatureIdp (src/odometry/triangulation.cpp:711-764) of the previous pair with
 * second_to_first = imuToCamera * secondImuToCamera^-1 (16 row-major doubles formed by the caller: the library does not
 * restate Eigen's inverse); world point = (idp.x, idp.y, 1) / idp.z. A feature failing any step takes no part. With at
 * least 3 correspondences a P3P RANSAC estimates the current-left camera pose and its inliers go back to TRACKED.
 * The sample-consensus loop, the sampler and the minimal solver are the ones stated in tests/ransac3_restatement.py
 * (Theia is not in the reference tree; DESIGN.md 3.14 lists what follows a recollection of it and what departs from it).
 * draws = the next 3 * ransac3MaxIterations raw outputs of the caller's std::mt19937 (the kernel forms
 * i + raw % (m - i) itself because m is only known on the device); afterwards the caller keeps 3 * iterations-run of them
 * consumed. Field names are the reference's parameters (codegen/parameter_definitions.c:282, 292-296).
 * HV_ERR_UNSUPPORTED: ransac3MaxIterations > HV_RANSAC3_MAX_ITERS or more than 1024 points; HV_ERR_INVALID:
 * ransac3FailureProbability outside (0, 1), ransac3ErrorThresh <= 0, ransac3MaxIterations < 1, ransac3MinIterations >
 * ransac3MaxIterations, ransacMinInlierFraction outside [0, 1] or a NULL required pointer. The parameter and size checks
 * come before the context is looked at. */
#define HV_RANSAC3_MAX_ITERS 500
typedef struct hv_ransac3_params {
    double ransac3ErrorThresh; double ransac3FailureProbability; int ransac3MaxIterations; int ransac3MinIterations;
    int ransac3UseMle; double ransacMinInlierFraction;
} hv_ransac3_params;
void hv_ransac3_default_params(hv_ransac3_params *p);   /* 1e-4, 1e-4, 500, 50, 1, 0.3 */
/* doRansac3 on one set of n features: status[n] int32 Feature::Status in/out (entries other than TRACKED stay), pose[12]
 * (NULL ok) = R row-major then the camera position c, x_cam = R (X - c), zeros without a model; summary[4] (NULL ok) =
 * {inlier count, iteration of the best model (-1: none), iterations run, correspondences m}. Fewer than 3
 * correspondences: not run, {0, -1, 0, m}. Synchronous. */
int hv_ransac3(hv_ctx *ctx, const hv_ransac3_params *p, int n, const float *prev_left_xy, const float *prev_right_xy,
               const float *cur_left_xy, const hv_camera_model *camera0, const hv_camera_model *camera1,
               const double *second_to_first, const uint32_t *draws, int *status, double *pose, int *summary);
/* n_sets sets in device memory: set s = n_points_dev[s] <= max_points (<= 1024) features at *_dev + s * max_points * 2,
 * draws_dev [n_sets][3 * ransac3MaxIterations], status_dev [n_sets][max_points] in/out (entries >= n_points_dev[s] are
 * never written), pose_dev [n_sets][12] and summary_dev [n_sets][4] as above (NULL ok). Asynchronous on the context
 * stream, no allocation or synchronisation inside (capturable in a HIP graph). n_sets <= 65535. */
int hv_ransac3_batch_dev(hv_ctx *ctx, const hv_ransac3_params *p, int n_sets, int max_points, const int *n_points_dev,
                         const float *prev_left_dev, const float *prev_right_dev, const float *cur_left_dev,
                         const hv_camera_model *camera0, const hv_camera_model *camera1, const double *second_to_first,
                         const uint32_t *draws_dev, int *status_dev, double *pose_dev, int *summary_dev);
/* The stereo device chain step after hv_rot_ransac_lk_batch_dev: RansacPipeline::compute on the RANSAC3 branch.
 * track_status_dev [n_sets][max_points] in/out as above, and when RANSAC3 did not run or produced no model (SKIPPED)
 * every entry < n_points_dev[s] becomes 3 (:139-144). r2_summary_dev = the summary_dev of hv_rot_ransac_lk_batch_dev on
 * the same set. result_dev [n_sets][2] = {type 0 SKIPPED / 2 R3, inlierCount}, score_dev [n_sets] = RANSAC2 inliers /
 * TRACKED count on entry (0 when that is 0), the return value of compute. The corner arguments are table.xy,
 * table.second_xy and the current corners of the track-table chain: call it before hv_tracks_update_batch_dev overwrites
 * them. Asynchronous, capturable. */
int hv_ransac3_lk_batch_dev(hv_ctx *ctx, const hv_ransac3_params *p, int n_sets, int max_points, const int *n_points_dev,
                            const float *prev_left_dev, const float *prev_right_dev, const float *cur_left_dev,
                            int *track_status_dev, const int *r2_summary_dev, const hv_camera_model *camera0,
                            const hv_camera_model *camera1, const double *second_to_first, const uint32_t *draws_dev,
                            int *result_dev, double *score_dev, double *pose_dev, int *summary_dev);

/* ---- stereo track gate: flow status, epipolar check, crop, blacklist and the detection filter (added within ABI 4) -----
 * Replaces the per-track status rules between the LK calls and RansacPipeline::compute in TrackerImplementation::track
 * (src/tracker/tracker.cpp:441-478) and the filter of new corners in detectFeatures (:266-311), with the helpers
 * computeEpipolarCurve (:81-106), withinDistanceFromCurve (:128-151), isPointInCrop (:315-320),
 * markOutOfDetectionCropCornersAsFailed (:322-346) and markCornersFailedByEpipolarConstraint (:348-376). Statuses are
 * int32 Feature::Status (TRACKED 0, FAILED_FLOW 2, FLOW_OUT_OF_RANGE 4, OUT_OF_RANGE 5, FAILED_EPIPOLAR_CHECK 6,
 * BLACKLISTED 8). Equal to the numpy restatement in tests/stereo_gate_restatement.py: the curve in binary64 through the
 * cameras of hv_rot_ransac (8 points, s = 0.5, 1, ..., 64, transformVec3ByMat4's order), its points and the distance
 * tests in binary32, dist = (float)((double)(maxStereoEpipolarDistance * (float)min(w, h)) / 720.0), the crop test in
 * binary64; w and h are the context's level-0 size. An empty curve (pixelToRay on camera0 or any rayToPixel on camera1
 * failing) leaves the status as it is.
 * cam0ToCam1 = secondImuToCamera * imuToCamera^-1 (tracker.cpp:362), 16 row-major doubles formed by the caller: the
 * library does not restate Eigen's 4 x 4 inverse, so the caller's product is what the reference's must equal.
 * second_corners == NULL: mono (stereo_status must be NULL too; no epipolar check, no right crop, camera1 may be NULL).
 * Layouts of the _dev forms: those of hv_klt_track_batch_dev / _ragged_dev, set s = n_points_dev[s] <= max_points entries
 * at s * max_points; entries at and beyond n_points_dev[s] are not touched. The _dev forms are asynchronous on the context
 * stream with no allocation or synchronisation inside (capturable in a HIP graph). Checks made before the context is
 * looked at: HV_ERR_INVALID for NULL required arrays or parameters, negative sizes, or a stereo / mono mismatch;
 * HV_ERR_UNSUPPORTED for n_sets > 65535 or, in the detection filter, max_points > 1024. */
#define HV_DETECTION_FILTER_MAX_POINTS 1024
typedef struct hv_stereo_gate_params {
    float maxStereoEpipolarDistance;      /* 10  codegen/parameter_definitions.c:217; <= 0: no epipolar check */
    double partOfImageToDetectFeatures;   /* 1   :353; < 1: the crop test of isPointInCrop */
    int fisheyeCamera;                    /* 0   :246; != 0: a corner whose pixelToRay fails is OUT_OF_RANGE */
    int independentStereoOpticalFlow;     /* 0   :210; != 0: track() skips the epipolar check (detectFeatures does not) */
    double cam0ToCam1[16];                /* row-major; default identity */
} hv_stereo_gate_params;
void hv_stereo_gate_default_params(hv_stereo_gate_params *p);
/* OpticalFlow::compute's status mapping (optical_flow.cpp:52-58) on the device: status = lk == 0 ? FAILED_FLOW : TRACKED,
 * then FLOW_OUT_OF_RANGE where x < 0 || x >= w || y < 0 || y >= h (binary32, w / h the level-0 size). xy_dev / lk_status_dev
 * = the next_xy_dev / status_dev of hv_klt_track_batch_dev (or _ragged_dev), [n_sets][max_points]; status_dev int32. */
int hv_flow_status_batch_dev(hv_ctx *ctx, int n_sets, int max_points, const int *n_points_dev, const float *xy_dev,
                             const uint8_t *lk_status_dev, int32_t *status_dev);
/* tracker.cpp:441-478 on n features, in the reference's order, track_status in / out (the left flow status on entry):
 * (1) stereo_status == FAILED_FLOW -> FAILED_FLOW (only that value is merged); (2) stereo, maxStereoEpipolarDistance > 0
 * and !independentStereoOpticalFlow: a TRACKED feature whose right corner is not within dist of the left corner's
 * non-empty curve -> FAILED_EPIPOLAR_CHECK; (3) the crop marks of the left corners (camera0), then of the right ones
 * (camera1) -> OUT_OF_RANGE, overwriting any status; (4) blacklist[i] != 0 (NULL: none) -> BLACKLISTED (the tracks whose
 * status is BLACKLISTED). corners = the current left corners, second_corners = the current right ones. Synchronous. */
int hv_track_gate(hv_ctx *ctx, const hv_stereo_gate_params *p, int n, const float *corners, const float *second_corners,
                  const int32_t *stereo_status, const uint8_t *blacklist, const hv_camera_model *camera0,
                  const hv_camera_model *camera1, int32_t *track_status);
/* The same for n_sets sets in device memory. tracked_mask_dev (NULL ok) [n_sets][max_points] uint8 = (status == TRACKED):
 * hv_rot_ransac_lk_batch_dev with lk_tracked_value 1 on it selects the features RansacPipeline::compute selects
 * (ransac_pipeline.cpp:106-112). */
int hv_track_gate_batch_dev(hv_ctx *ctx, const hv_stereo_gate_params *p, int n_sets, int max_points, const int *n_points_dev,
                            const float *corners_dev, const float *second_corners_dev, const int32_t *stereo_status_dev,
                            const uint8_t *blacklist_dev, const hv_camera_model *camera0, const hv_camera_model *camera1,
                            int32_t *track_status_dev, uint8_t *tracked_mask_dev);
/* detectFeatures after the stereo LK of the n <= 1024 new corners (tracker.cpp:266-311): the status starts as stereo_status
 * (mono: TRACKED); stereo and maxStereoEpipolarDistance > 0: the epipolar check (whatever independentStereoOpticalFlow);
 * the crop marks, left then right; then the TRACKED pairs are compacted in input order into out_corners / out_second
 * (*n_out of them). status (NULL ok) receives the n final statuses. The outputs may be the inputs. Synchronous. */
int hv_detection_filter(hv_ctx *ctx, const hv_stereo_gate_params *p, int n, const float *corners, const float *second_corners,
                        const int32_t *stereo_status, const hv_camera_model *camera0, const hv_camera_model *camera1,
                        int32_t *status, float *out_corners, float *out_second, int *n_out);
/* The same for n_sets sets of <= max_points <= 1024 corners, one workgroup per set: set s compacted at s * max_points of
 * out_corners_dev / out_second_dev, its count in n_out_dev[s]. */
int hv_detection_filter_batch_dev(hv_ctx *ctx, const hv_stereo_gate_params *p, int n_sets, int max_points,
                                  const int *n_points_dev, const float *corners_dev, const float *second_corners_dev,
                                  const int32_t *stereo_status_dev, const hv_camera_model *camera0,
                                  const hv_camera_model *camera1, int32_t *status_dev, float *out_corners_dev,
                                  float *out_second_dev, int *n_out_dev);

/* ---- device track table: updateTracks, culling, keyframes and new-track append (added within ABI 4) -----------------
 * Replaces the bookkeeping of TrackerImplementation::add / track from the keyframe decision onwards
 * (src/tracker/tracker.cpp:199-229, 527-558) for n_sets resident sequences: computeVisualStationarity (:578-602) with
 * computeMaxPixelCoordinateMovement (:21-41), updateTracks (:604-670), setMask (:766-777), detectNewFeatures' append and
 * ID rule (:672-703, :199), the maskScale tuning (:540-546, changeMaskSize :561-567) and maskRadius (:569-576), the
 * construction of prevCorners / prevSecondCorners (:548-558), the reset below five tracks (:209-229) with resetAllTracks
 * (:705-719), and deleteTrack (:726-738). Equal, array for array, to the literal restatement in
 * tests/track_table_restatement.py; every rule is integer or IEEE arithmetic, so there is no tolerance.
 * The table is device memory owned by the caller; set s is at s * maxTracks of every per-track array. Entries of a set at
 * and beyond n_tracks[s] are unspecified, except that kf_valid and blacklist are 0 there after an update.
 * lastKeyframeCornerByTrackId (an unordered_map keyed by track ID) is the per-slot pair kf_xy / kf_valid: IDs are unique and
 * an entry is erased exactly when its track is, so a slot that moves with its track under compaction is the same thing.
 * maskScale only moves by -1.0 and +0.5 inside [-5, 5] and is held as mask_steps = 2 * maskScale; the 21 possible radii
 * std::round(std::pow(1.3, steps / 2.0) * min(w, h) * relativeMaskRadius), floor 2 (:569-576; w, h = the context's level-0
 * size), are computed on the host inside each entry and passed to the kernel.
 * All _dev entries: asynchronous on the context stream, no allocation or synchronisation inside (capturable in a HIP
 * graph), one workgroup per set. Checks made before the context is looked at: HV_ERR_INVALID for a NULL required pointer
 * (a table member included; second_xy may be NULL = mono), a negative size, maxTracks < 1, or a stereo / mono mismatch
 * between the second_* argument and table->second_xy; then HV_ERR_UNSUPPORTED for n_sets > 65535 or maxTracks >
 * HV_TRACKS_MAX_TRACKS (a call that is both invalid and too large is HV_ERR_INVALID). Counts read from device memory are
 * clamped to their capacity. */
#define HV_TRACKS_MAX_TRACKS 1024          /* = HV_DETECTION_FILTER_MAX_POINTS: one workgroup per set */
typedef struct hv_track_table_params {
    int maxTracks;                               /* 200    codegen/parameter_definitions.c:262 */
    int maxTrackLength;                          /* 21     :265 */
    double relativeMaskRadius;                   /* 0.0667 :308 */
    double visualStationarityMovementThreshold;  /* 3.0    :111 */
    double visualStationarityScoreThreshold;     /* 0.95   :113 */
} hv_track_table_params;
typedef struct hv_track_table {            /* set s at s * maxTracks of every per-track array */
    int32_t *n_tracks;     /* [n_sets]               tracks.size() */
    int32_t *ids;          /* [n_sets][maxTracks]    Feature::id */
    float   *xy;           /* [..][2]  points[0] = next frame's prevCorners (prev_xy of hv_klt_track_batch_ragged_dev) */
    float   *second_xy;    /* [..][2]  points[1]; NULL = mono */
    int32_t *status;       /* Feature::status: NEW (1) when appended, the frame's status after an update, BLACKLISTED (8) after a delete */
    uint8_t *blacklist;    /* status == BLACKLISTED, in the form hv_track_gate_batch_dev reads */
    float   *kf_xy;        /* [..][2] */
    uint8_t *kf_valid;     /* lastKeyframeCornerByTrackId: the entry of the track in this slot, moved with it */
    int32_t *frame_num;    /* [n_sets] frameNum on entry to add() */
    int32_t *mask_steps;   /* [n_sets] 2 * maskScale, in [-10, 10] */
    int32_t *mask_radius;  /* [n_sets] maskRadius() for the NEXT detect: mask_radius_dev of hv_gftt_detect_batch_dev */
    uint8_t *frame_flags;  /* [n_sets] written by update, read by append: bit 0 = reset frame */
} hv_track_table;
void hv_track_table_default_params(hv_track_table_params *p);
/* Every set becomes a fresh TrackerImplementation (tracker.cpp:165-174): no tracks, frame_num 0, mask_steps 0, mask_radius =
 * the radius of step 0; kf_valid, blacklist and frame_flags cleared. */
int hv_tracks_init_batch_dev(hv_ctx *ctx, const hv_track_table_params *p, int n_sets, const hv_track_table *table);
/* The table step of one frame after the RANSAC filter. corners_dev / second_corners_dev [n_sets][maxTracks][2] = the current
 * corners of the table's tracks (second: NULL exactly when table->second_xy is), track_status_dev [n_sets][maxTracks] int32
 * in / out = the statuses hv_hybrid_ransac_lk_batch_dev left, score_dev [n_sets] = its stationarity score (NULL: 0, never
 * stationary). Per set, with f = frame_num[s] and n = n_tracks[s], in this order:
 * - reset frame, f == 0 or n < 5 (:201-205, 209, 222-229): the table and its keyframe entries are cleared, n_mask = 0
 *   (setMask({}, {})), keyframe = 1, max_movement = -1, frame_flags bit 0 set; track_status_dev is untouched. (The
 *   reference leaves output.keyframe alone in the n < 5 branch; 1 is this library's choice.)
 * - otherwise setMask first (:492, 766-777): the TRACKED corners in order go to mask_xy_dev [n_sets][maxTracks][2] with
 *   their count in n_mask_dev [n_sets]; this is before the culling, so culled corners stay in the mask.
 * - keyframe_dev [n_sets] int32 = (f + 1 < maxTrackLength) || !stationary (:527-528; frameNum is f + 1 there). maxMovement
 *   (:21-41) runs over the TRACKED tracks with a keyframe entry: the largest binary64 sqrt(dx*dx + dy*dy), dx and dy
 *   binary32 differences widened to binary64, uncontracted; -1 without such a track, and then not stationary; else
 *   stationary = score * (maxMovement < visualStationarityMovementThreshold ? 1 : 0) > visualStationarityScoreThreshold.
 *   max_movement_dev [n_sets] double (NULL ok) receives maxMovement.
 * - culling, only when n == maxTracks (:621-639): all pairs i < j in generation order with dist2 in the same arithmetic,
 *   std::stable_sort by dist2, the walk that puts j into a set and CULLED (7) into track_status[j] whatever it held, stopped
 *   once the set holds more than maxTracks / 20 members. The kernel selects the same tracks without the sort.
 * - write-back and erase (:641-669): a TRACKED track takes its new points, and its keyframe entry when keyframe is set;
 *   every other track is erased with its keyframe entry; the survivors are compacted in order (status TRACKED, blacklist
 *   0); src_index_dev [n_sets][maxTracks] int32 (NULL ok) receives each survivor's old slot; n_tracks is written.
 * frame_num is not changed here. Every input is read before any output is written, so corners_dev may be table->xy. */
int hv_tracks_update_batch_dev(hv_ctx *ctx, const hv_track_table_params *p, int n_sets, const hv_track_table *table,
                               const float *corners_dev, const float *second_corners_dev, int32_t *track_status_dev,
                               const double *score_dev, int32_t *keyframe_dev, float *mask_xy_dev, int32_t *n_mask_dev,
                               int32_t *src_index_dev, double *max_movement_dev);
/* The end of the frame: the pairs hv_detection_filter_batch_dev compacted, new_xy_dev / new_second_dev
 * [n_sets][max_new][2] with n_new_dev [n_sets] (clamped to [0, max_new]; max_new == 0: no array is read). On a reset frame,
 * or when missing = maxTracks - n_tracks >= maxTracks / 10 (:686), the first min(n_new, missing) pairs are appended in
 * order with IDs f * maxTracks + 1, + 2, ... (:199, 692-698), status NEW (1), no keyframe entry. Unless the frame was a
 * reset frame the mask is tuned from the new count n (:540-546): steps -= 2 when n < (3 * maxTracks) / 4, else steps += 1
 * when n == maxTracks, clamped to +-10. On every frame mask_radius = radius(steps), frame_num = f + 1 and frame_flags is
 * cleared. n_added_dev [n_sets] int32 (NULL ok) receives the number appended. */
int hv_tracks_append_batch_dev(hv_ctx *ctx, const hv_track_table_params *p, int n_sets, const hv_track_table *table,
                               int max_new, const int32_t *n_new_dev, const float *new_xy_dev, const float *new_second_dev,
                               int32_t *n_added_dev);
/* deleteTrack (:726-738) for the ids_dev [n_sets][max_ids] int32 listed per set (n_ids_dev [n_sets], clamped to
 * [0, max_ids]): the track that carries a listed ID gets status BLACKLISTED (8) and blacklist 1; unknown IDs and repeats
 * are ignored. */
int hv_tracks_delete_batch_dev(hv_ctx *ctx, const hv_track_table_params *p, int n_sets, const hv_track_table *table,
                               int max_ids, const int32_t *n_ids_dev, const int32_t *ids_dev);

/* ---- EKF control updates: ZUPT, pseudo-velocity, unit-block updates and the per-frame rules (added within ABI 4) -------
 * Replaces, for a batch of resident filters, the control part of Session::process (src/odometry/backend.cpp:738-749,
 * 774-796) and the updates it calls (ekf.cpp:573-677): every one of them has a measurement matrix made of unit rows
 * (pseudo-velocity: one 1 x 2 unit vector), so HP is rows of P, S a sub-block of P plus r I, and the update one rank-k
 * downdate that reads and writes P once (csrc/ekf_control.hip). The reference's operands are kept -- HP
 * from the ROWS of P, S factored from its lower triangle -- because P is only symmetrised at maintainPositiveSemiDefinite.
 * A filter whose S has a pivot that is not positive is left untouched (applied = 0), the library's rule for S.
 * All entries: one launch, one workgroup per filter, asynchronous on the context stream, no allocation or synchronisation
 * inside (capturable in a HIP graph). HV_ERR_INVALID for a NULL handle, a NULL required pointer (a member of hv_ekf_control
 * included) or the argument ranges stated below, decided before any device work; HV_ERR_UNSUPPORTED for a state of more
 * than 1024 entries. Masked-out filters are not touched at all. */
/* update(m, P, y, H, R) + updateCommon for H = the `rows` (1 .. 4) unit rows of the state entries col0 .. col0 + rows - 1
 * (col0 >= 0, col0 + rows <= stateDim): updateZupt / updateZuptInitialization (VEL = 3, 3), updateZrupt (BGA = 10, 3),
 * updatePosition (POS = 0, 3), updateZeroHeight (2, 1), updateOrientation (ORI = 6, 4, normalize_all = 1); the caller follows
 * it with hv_ekf_symmetrize where the reference calls maintainPositiveSemiDefinite and applies the reference's rate limits
 * itself (or uses the control steps below). y_dev [batch][rows] (NULL: zeros); R = r I with r = r_dev[f] (r_dev [batch]) or,
 * r_dev NULL, r0 for every filter: already scaled by noiseScale^2, like the r_diag of hv_ekf_update. active_dev [batch]
 * uint8 (NULL: all). normalize_all != 0: normalizeQuaternions() on the trail as well (the current orientation always is).
 * applied_dev [batch] uint8 (NULL ok) = 1 where the update was applied, 0 where masked out or refused. */
int hv_ekf_block_update_dev(hv_ekf *ekf, int col0, int rows, const double *y_dev, const double *r_dev, double r0,
                            const unsigned char *active_dev, int normalize_all, unsigned char *applied_dev);
/* updatePseudoVelocity(target, r) (ekf.cpp:628-649) behind the caller's speed test (backend.cpp:744-745), the mean read on
 * the device: h = |m[VEL : VEL + 2]| (two rounded products, one rounded sum, sqrt); skipped when h <= 1e-7 or h <= limit
 * (limit < 0: no limit test); otherwise the scalar update with H = m[VEL : VEL + 2]' / h, residual target - h and
 * R = r * noiseScale^2. applied_dev as above (0 for a skipped filter). */
int hv_ekf_pseudo_velocity_dev(hv_ekf *ekf, double limit, double target, double r, const unsigned char *active_dev,
                               unsigned char *applied_dev);
/* hv_ekf_undo_augment with the mask in device memory (NULL: all): the same kernel and ping-pong (fetch P_dev again
 * afterwards), masked-out filters carried over unchanged. active_dev is what hv_ekf_frame_control_dev writes as undo_active_dev. */
int hv_ekf_undo_augment_dev(hv_ekf *ekf, const unsigned char *active_dev);
/* The odometry parameters the control steps read (codegen/parameter_definitions.c:87-119); initZuptR is hv_ekf_params'. */
typedef struct hv_ekf_control_params {
    int useDecayingZeroVelocityUpdate;            /* 0 */
    int usePseudoVelocity;                        /* 0 */
    double pseudoVelocityLimit;                   /* 1.4 */
    double pseudoVelocityTarget;                  /* 0 */
    double pseudoVelocityR;                       /* 1e-4 */
    int useVisualStationarity;                    /* 1 */
    int visualStationarityFrameCountThreshold;    /* 3 */
    double visualZuptR;                           /* 1e-7 */
} hv_ekf_control_params;
void hv_ekf_control_default_params(hv_ekf_control_params *p);
/* The scalar members of odometry::EKF and Session the control steps keep, as device arrays of [batch] owned by the caller
 * (like hv_track_table). */
typedef struct hv_ekf_control {
    double  *zupt_time;              /* EKF::ZUPTtime */
    double  *init_zupt_time;         /* EKF::initZUPTtime */
    int32_t *was_stationary;         /* EKF::wasStationary */
    int32_t *frames_since_keyframe;  /* Session::framesSinceKeyframe */
} hv_ekf_control;
/* A fresh session: both clocks -1.0, the flag and the counter 0. */
int hv_ekf_control_init_dev(hv_ekf *ekf, const hv_ekf_control *ctl);
/* The control updates behind an IMU sample's predict (backend.cpp:738-749). time_dev [batch] double = the filter clock
 * t - firstSampleT (ekf.cpp:360): the last row of hv_session_imu_dev's time_dev, or the caller's own. Per active filter, in this order:
 * - useDecayingZeroVelocityUpdate: updateZuptInitialization (ekf.cpp:594-611), skipped when was_stationary, time > 60 or
 *   time - init_zupt_time < 0.1; otherwise init_zupt_time = time and the zero-velocity update with
 *   R = initZuptR * noiseScale^2 * exp(0.5 * time);
 * - usePseudoVelocity: hv_ekf_pseudo_velocity_dev(pseudoVelocityLimit, pseudoVelocityTarget, pseudoVelocityR) on the mean
 *   the first update left.
 * With both switches off nothing is launched. */
int hv_ekf_imu_control_dev(hv_ekf *ekf, const hv_ekf_control_params *p, const hv_ekf_control *ctl, const double *time_dev,
                           const unsigned char *active_dev);
/* The control part of a frame (backend.cpp:774-796), every filter. keyframe_dev [batch] int32 = what
 * hv_tracks_update_batch_dev writes; full_update_dev [batch] uint8 (NULL: every frame is a full visual update, the default
 * visualUpdateForEveryNFrame = 1). Per filter:
 * - frames_since_keyframe = keyframe ? 0 : frames_since_keyframe + 1; stationary = frames_since_keyframe >=
 *   visualStationarityFrameCountThreshold;
 * - useVisualStationarity && stationary: updateZupt(visualZuptR) (ekf.cpp:573-590), skipped when time - zupt_time < 0.25;
 *   otherwise zupt_time = time, was_stationary = 1 and the zero-velocity update with R = visualZuptR * noiseScale^2;
 * - keyframe_out = keyframe && full; undo_active = !keyframe_out (the filters hv_ekf_undo_augment_dev shifts).
 * Outputs, each [batch] and each NULL ok: keyframe_out_dev int32, undo_active_dev / stationary_dev / applied_dev uint8
 * (applied: the ZUPT was due and applied). */
int hv_ekf_frame_control_dev(hv_ekf *ekf, const hv_ekf_control_params *p, const hv_ekf_control *ctl, const double *time_dev,
                             const int32_t *keyframe_dev, const unsigned char *full_update_dev, int32_t *keyframe_out_dev,
                             unsigned char *undo_active_dev, unsigned char *stationary_dev, unsigned char *applied_dev);

/* ---- device pose-trail index: keyframes, visual-update track selection, blacklist (added within ABI 4) ----------------
 * Replaces, for n_sets resident sequences, what Session does with odometry::EKFStateIndex between the track table and the
 * filter (src/odometry/ekf_state_index.{hpp,cpp}; backend.cpp:793-805, 909-1052, 1189-1213, 1240-1243, 1269-1274): which
 * observation of which track sits in which pose of the trail, which tracks visit the filter and in what order, the arrays
 * hv_ekf_visual_frame_ragged_dev reads, the used / blacklist marks afterwards and the pose the augmentation drops. Equal,
 * array for array, to the literal restatement in tests/trail_index_restatement.py: every rule is integer or single-rounded
 * IEEE arithmetic (the pixel normalisation is Camera::normalizePixel of hv_camera_model, as in hv_ransac3*).
 * The state is device memory owned by the caller. Keyframe push, pop and remove and the erasure of tracks are index
 * permutations: kf_row maps a keyframe (0 = head) to the physical row of its observations, a live track owns one column,
 * and because a track's observations are contiguous from keyframe 0 once prune() has run, col_len says which keyframes
 * hold it. Between finish and the next select the head is the new, empty keyframe and a column's col_len
 * observations sit in keyframes 1 .. col_len; after select they sit in keyframes 0 .. col_len - 1.
 * All entries: one launch, one workgroup per set, asynchronous on the context stream, no allocation or synchronisation
 * inside (capturable in a HIP graph). Checks made before the context is looked at: HV_ERR_INVALID for a NULL required
 * pointer (a state member included), a negative size, maxTracks < 1, cameraTrailLength < 1, a negative Hanoi / strided
 * length, cameraTrailHanoiLength + cameraTrailStridedLength + 1 >= maxSize (= cameraTrailLength + 1; the reference's
 * constructor asserts), a strided stride < 1 with a strided part, a trackSampling that is no TrackSampling; then
 * HV_ERR_UNSUPPORTED for n_sets > 65535, maxTracks > HV_TRACKS_MAX_TRACKS, maxSize > HV_TRAIL_MAX_POSES, maxVisualUpdates
 * outside 1 .. HV_TRAIL_MAX_VISITS, TrackSampling::RANDOM (its draws depend on the visit outcomes), hybridMapSize > 0,
 * useIndependentStereoTriangulation and fullPointCloud = 1: these entries state the loop that breaks at its stop; the tracks
 * behind the stop are hv_full_point_cloud_dev's (below), which a caller runs between the visit loop and finish, with
 * fullPointCloud left 0 here. Counts read from device memory are clamped to their capacity. */
#define HV_TRAIL_MAX_POSES 64
#define HV_TRAIL_MAX_VISITS 64
enum { HV_TRACK_SAMPLING_GAP = 0, HV_TRACK_SAMPLING_ALL = 1, HV_TRACK_SAMPLING_RANDOM = 2 };
typedef struct hv_trail_index_params {
    int cameraTrailLength;                  /* 20   codegen/parameter_definitions.c */
    int cameraTrailHanoiLength;             /* 3 */
    int cameraTrailStridedLength;           /* 0 */
    int cameraTrailStridedStride;           /* 2 */
    int cameraTrailFixedScheme;             /* 0 */
    int trackSampling;                      /* HV_TRACK_SAMPLING_GAP */
    int trackMinFrames;                     /* 4 */
    int scoreVisualUpdateTracks;            /* 1 */
    int blacklistTracks;                    /* 1 */
    int maxVisualUpdates;                   /* 20 */
    int maxSuccessfulVisualUpdates;         /* 5 */
    int estimateImuCameraTimeShift;         /* 1 */
    int useStereo;                          /* 1 */
    int maxTracks;                          /* 200 */
    int hybridMapSize;                      /* 0; > 0 unsupported */
    int useIndependentStereoTriangulation;  /* 0; unsupported */
    int fullPointCloud;                     /* 0; 1 is refused here: call hv_full_point_cloud_dev */
} hv_trail_index_params;
void hv_trail_index_default_params(hv_trail_index_params *p);
/* K = maxSize, M = maxTracks, C = useStereo ? 2 : 1, V = maxVisualUpdates; set s at s * (the size of one set) of every array. */
typedef struct hv_trail_index {
    int32_t *n_keyframes;    /* [n_sets]           keyframes.size() */
    int32_t *frame_counter;  /* [n_sets]           EKFStateIndex::frameCounter */
    int32_t *kf_row;         /* [n_sets][K]        keyframe -> physical row: a permutation of 0 .. K - 1, rows of no keyframe behind n_keyframes */
    int32_t *frame_number;   /* [n_sets][K]        KeyFrame::frameNumber, by physical row */
    double  *timestamp;      /* [n_sets][K]        KeyFrame::timestamp, by physical row */
    int32_t *col_id;         /* [n_sets][M]        track ID of a column; -1 where col_len is 0 */
    int32_t *col_len;        /* [n_sets][M]        keyframes that hold the track; 0 = free column */
    float   *image_point;    /* [n_sets][K][M][C][2]  Feature::Frame::imagePoint (a binary32 corner, widened where it is used) */
    double  *norm_point;     /* [n_sets][K][M][C][2]  normalizedImagePoint */
    double  *norm_velocity;  /* [n_sets][K][M][C][2]  normalizedVelocity */
    uint8_t *used;           /* [n_sets][K][M]     Feature::usedForVisualUpdate */
    int32_t *n_blacklist;    /* [n_sets] */
    int32_t *blacklist_ids;  /* [n_sets][M]        Session::blacklistedPrev, in the reference's order */
    /* what select leaves for finish */
    int32_t *n_order;        /* [n_sets]           trackOrder.size() */
    int32_t *n_skipped;      /* [n_sets]           tracks skipped for the previous blacklist ... */
    int32_t *skipped_pos;    /* [n_sets][M]        ... their positions in the order, ascending ... */
    int32_t *skipped_id;     /* [n_sets][M]        ... and their IDs */
    int32_t *cand_pos;       /* [n_sets][V]        position in the order of every candidate */
    int32_t *cand_col;       /* [n_sets][V]        and its column */
} hv_trail_index;
/* The constructor (ekf_state_index.hpp:100-107): one keyframe (0, 0.0) without features, frame_counter 0, every column free,
 * empty blacklist, kf_row the identity. */
int hv_trail_init_batch_dev(hv_ctx *ctx, const hv_trail_index_params *p, int n_sets, const hv_trail_index *trail);
/* Everything up to the visit loop (backend.cpp:793-800, 909-1052). table: n_tracks, ids, xy and (useStereo) second_xy of the
 * hv_track_table after hv_tracks_append_batch_dev, with maxTracks slots per set; camera1 may be NULL without useStereo.
 * keyframe_dev [n_sets] int32 = keyframe_out_dev of hv_ekf_frame_control_dev; full_update_dev [n_sets] uint8 (NULL: every frame
 * is full); frame_num_dev [n_sets] int32 and time_dev [n_sets] double stamp the head; draws_dev [n_sets][maxTracks] = the next
 * raw std::mt19937 outputs of each sequence, of which draws_used_dev [n_sets] = max(n - 1, 0) are consumed (n = trackOrder.size()).
 * Per set, in this order:
 * - pop and stamp: not a keyframe -> popHeadKeyframe (:33-39); with a single keyframe, where the reference asserts, nothing is
 *   popped. The head takes frame_num and time.
 * - insert, every table track in slot order: imagePoint = the corner; normalizePixel per camera (the second only with useStereo,
 *   and not after a failure of the first); on success insertFeatureUnlessExists, updateVelocities (:361-384) when
 *   estimateImuCameraTimeShift -- with its early returns on non-increasing timestamps and the rewrite of keyframe 1's velocity --
 *   and the track enters trackOrder.
 * - prune (:220-242): a track that is not in the head leaves every keyframe; its column is free.
 * - shuffleDeterministic (util/util.hpp:39-44) over trackOrder.
 * - trackScore (:41-87) per track: a binary32 sum, each term the binary64 L1 norm of the first camera's pixel difference, added
 *   in binary64 and rounded to binary32 at every step; with scoreVisualUpdateTracks, minTrackScore = the element size / 2 of the
 *   sorted int-truncated scores (-1 without tracks), else 0.
 * - filter, in shuffled order, with createTrackIndex (:90-147): skipped when scoreVisualUpdateTracks and score < minTrackScore,
 *   then when nValid < trackMinFrames, then on a frame that is not full, then (blacklistTracks) when the ID is in the previous
 *   blacklist -- such a track is remembered with its position; every other track is a candidate, up to maxVisualUpdates of them.
 * - gather, buildTrackVectors (:192-218) for candidate v, in the layout of hv_ekf_visual_frame_ragged_dev with n_tracks =
 *   maxVisualUpdates and n_poses_max = maxSize: n_poses_dev [V][n_sets] (0: the set has no candidate v), pose_index_dev
 *   [V][n_sets][K], features_dev / velocities_dev [V][n_sets][C * K][2] and y_dev [V][n_sets][2 * C * K], the first camera's poses
 *   then the second's at the start of a record (the rest of a record is not written); cand_id_dev [V][n_sets] = the track ID
 *   (-1: none), n_candidates_dev [n_sets]. */
int hv_trail_select_batch_dev(hv_ctx *ctx, const hv_trail_index_params *p, int n_sets, const hv_trail_index *trail,
                              const hv_track_table *table, const hv_camera_model *camera0, const hv_camera_model *camera1,
                              const int32_t *keyframe_dev, const uint8_t *full_update_dev, const int32_t *frame_num_dev,
                              const double *time_dev, const uint32_t *draws_dev, int32_t *draws_used_dev, int32_t *n_poses_dev,
                              int32_t *pose_index_dev, double *features_dev, double *velocities_dev, double *y_dev,
                              int32_t *cand_id_dev, int32_t *n_candidates_dev);
/* The bookkeeping behind the visit loop (backend.cpp:1189, 1204-1213, 1240-1243, 1269-1274, 804). cand_id_dev / n_candidates_dev
 * as select wrote them; status_dev [V][n_sets][2] and gate_status_dev [V][n_sets] as hv_ekf_visual_frame_ragged_dev wrote them;
 * stationary_dev [n_sets] uint8 (NULL: 0) = stationary_dev of hv_ekf_frame_control_dev. Per set, the candidates in visit order:
 * - visited = status[v][0] != HV_TRI_NOT_VISITED; a visited candidate with gate status 0 (INLIER) is a success: markTrackUsed
 *   (:156-181); every other visited candidate is blacklisted and deleted when blacklistTracks.
 * - the loop stopped at the candidate whose visit brought the successes to maxSuccessfulVisualUpdates (<= 0: no such limit) or
 *   the attempts to maxVisualUpdates; candidates behind it are not counted. If it never stopped, the stop position is the end of
 *   the order. A track skipped for the previous blacklist enters the new one exactly when its position precedes the stop position.
 * - delete_ids_dev [n_sets][maxTracks] / n_delete_dev [n_sets]: the visited non-inliers in visit order (the input of
 *   hv_tracks_delete_batch_dev with max_ids = maxTracks); the new blacklist replaces the state's, in the order of the reference.
 * - good_frame_dev [n_sets] uint8 = (stationary || stopped) && !(attempts - successes > 5); n_attempts_dev, n_success_dev [n_sets].
 * - pushHeadKeyframe (:23-31) with removeKeyframe (:244-281): free-slot rule, strided rule, Hanoi rule, frame_counter;
 *   discarded_dev [n_sets] int32 = removedIdx - 1, the argument of hv_ekf_augment_dev / hv_ekf_symmetrize_augment_dev.
 * Every output but delete_ids_dev, n_delete_dev and discarded_dev may be NULL. */
int hv_trail_finish_batch_dev(hv_ctx *ctx, const hv_trail_index_params *p, int n_sets, const hv_trail_index *trail,
                              const int32_t *cand_id_dev, const int32_t *n_candidates_dev, const int32_t *status_dev,
                              const int32_t *gate_status_dev, const uint8_t *stationary_dev, int32_t *delete_ids_dev,
                              int32_t *n_delete_dev, uint8_t *good_frame_dev, int32_t *n_attempts_dev, int32_t *n_success_dev,
                              int32_t *discarded_dev);

/* ---- device optical-flow predictor: LK start points from the filter mean and the pose-trail index (added within ABI 4) ----
 * Replaces, for the hv_ekf_batch(ekf) resident sequences of a filter batch (set s is filter s), the OpticalFlowPredictor lambda of
 * Session::applyTracker (src/odometry/backend.cpp:545-664), which Tracker::track calls before its temporal and its stereo LK
 * call (src/tracker/tracker.cpp:58-62, predictOpticalFlow = true): pred_xy_dev is the next_xy of hv_klt_track_batch*_dev with
 * use_initial_flow = 1. Per table track i < n_tracks[s], in binary64 and in the operation order of
 * tests/flow_predict_restatement.py:
 * - distance: EKFStateIndex::widestBaseline (ekf_state_index.cpp:312-339), the first and the last keyframe that hold the track's
 *   ID; when they are at least minBaselinePoses apart, triangulateWithTwoCameras (triangulation.cpp:610-646) between the first
 *   camera's poses of the two keyframes (extractCameraPoseTrail, :65-103, through imuToCamera: keyframe k is historyPosition(k - 1)
 *   of the mean, keyframe 0 the current pose) on the first camera's norm_point, and |pf| when pf(2) > 0; otherwise -1; then
 *   clamped from below at predictOpticalFlowMinTriangulationDistance. A track without a column (a new track, or one whose
 *   normalizePixel failed) gets the minimum. All three types triangulate with the first camera, as the reference does.
 * - prediction: pixelToRay(c0) * distance through camToWorld0 and worldToCam1 (util::toCameraToWorld / toWorldToCamera,
 *   src/odometry/util.cpp:132-158, with the supplied inverse), rayToPixel, rounded to binary32; c0 itself when either camera call
 *   fails. LEFT: history pose 0 -> current pose through imuToCamera, camera0 for both calls; RIGHT: the same through
 *   secondImuToCamera with camera1; STEREO: current pose through imuToCamera -> current pose through secondImuToCamera, camera0
 *   into camera1 (backend.cpp:575-612).
 * The entry belongs between hv_trail_finish_batch_dev of the previous frame and hv_trail_select_batch_dev of this one (where
 * applyTracker runs: after the frame's IMU predicts, the head keyframe empty), and reads the index as it is there: keyframe k
 * holds a column's track exactly when 1 <= k <= col_len.
 * c0_dev [n_sets][maxTracks][2] = the lambda's c0 (LEFT: table->xy; STEREO: the left corners the temporal LK produced);
 * pred_xy_dev [n_sets][maxTracks][2]; distance_dev [n_sets][maxTracks] double or NULL. reuse_distance = 0 triangulates and writes
 * distance_dev when it is given; 1 reads distance_dev instead (neither the index nor the mean changes between the two LK calls
 * of a frame). Slots at and behind n_tracks[s] are not written. tp: maxTracks, cameraTrailLength and useStereo (the layout of the
 * index) are read. A non-finite mean gives whatever this arithmetic yields in its own set and touches no other.
 * One launch of one workgroup per set on the filter's context stream, timed under HV_K_TRAIL_INDEX, no allocation or
 * synchronisation inside (capturable in a HIP graph). Checks made before the handle is looked at: HV_ERR_INVALID for a NULL
 * required pointer (p, tp, trail and its members, table and its n_tracks / ids, c0_dev, camera0, pred_xy_dev; camera1 for RIGHT
 * and STEREO), the parameter ranges of hv_trail_index_params, a type outside 0 .. 2, reuse_distance with a NULL distance_dev,
 * minBaselinePoses < 1; then HV_ERR_UNSUPPORTED for maxTracks > HV_TRACKS_MAX_TRACKS or maxSize > HV_TRAIL_MAX_POSES; then
 * HV_ERR_INVALID for a NULL handle and HV_ERR_UNSUPPORTED for a state of fewer than 20 + 7 * cameraTrailLength entries. Counts
 * and indices read from device memory (n_tracks, n_keyframes, col_len, kf_row) are clamped to their capacity. */
typedef struct hv_flow_predict_params {
    double predictOpticalFlowMinTriangulationDistance;   /* 3.0  codegen/parameter_definitions.c:213 */
    int    minBaselinePoses;                             /* 10   MIN_TWO_CAMERA_FLOW_TRIANGULATION_BASELINE, backend.cpp:627 */
    double imuToCamera[16], secondImuToCamera[16];       /* row-major */
    double cameraToImu[16], secondCameraToImu[16];       /* their inverses, formed once by the integrator (like
                                                            hv_stereo_gate_params.cam0ToCam1): Eigen's 4x4 inverse is not restated on the device */
} hv_flow_predict_params;
void hv_flow_predict_default_params(hv_flow_predict_params *p);   /* the scalars as above, the four matrices identity */
enum { HV_FLOW_PREDICT_LEFT = 0, HV_FLOW_PREDICT_RIGHT = 1, HV_FLOW_PREDICT_STEREO = 2 };   /* OpticalFlowPredictor::Type */
int hv_flow_predict_batch_dev(hv_ekf *ekf, const hv_flow_predict_params *p, int type, const hv_trail_index_params *tp,
                              const hv_trail_index *trail, const hv_track_table *table, const float *c0_dev,
                              const hv_camera_model *camera0, const hv_camera_model *camera1, float *pred_xy_dev,
                              double *distance_dev, int reuse_distance);

/* ---- stereo upright 2-point RANSAC: gravity-aware track filter (added within ABI 4) -----------------------------------
 * Replaces StereoUpright2p::compute (src/tracker/stereo_upright_2p.cpp:110-183, the error :72-81) and the UPRIGHT_2P
 * branch of RansacPipeline::compute (src/tracker/ransac_pipeline.cpp:124-127, 137-149) without Theia. poses = the
 * camera-to-world matrices of the previous and the current frame (two row-major 4x4, src/odometry/backend.cpp:667-679); the
 * filter reads their rotations R0, R1. Per feature with status TRACKED (0), in feature order: the status becomes
 * RANSAC_OUTLIER (3); Camera::normalizePixel of the previous-left (camera0) and previous-right (camera1) corner;
 * triangulateStereoFeatureIdp of the pair with second_to_first (as hv_ransac3); Camera::pixelToRay of the current-left
 * corner (camera0); the correspondence is modelPoint = R0 X, ray = R1 ray_cam, rayNormalized = ray_cam.xy / ray_cam.z. A
 * feature failing any step takes no part. With at least 2 correspondences a 2-point RANSAC estimates the rotation about
 * the world's z axis (gravity) and the translation between the two frames, and its inliers go back to TRACKED.
 * The sample-consensus loop, the sampler and the minimal solver are the ones stated in tests/upright2p_restatement.py
 * (Theia is not in the reference tree; DESIGN.md 3.21 lists what follows a recollection of it and what departs from it).
 * draws = the next 2 * ransacStereoUpright2pMaxIterations raw outputs of the caller's std::mt19937; afterwards the caller
 * keeps 2 * iterations-run of them consumed. Field names are the reference's parameters
 * (codegen/parameter_definitions.c:282, 299-303).
 * HV_ERR_UNSUPPORTED: ransacStereoUpright2pMaxIterations > HV_UPRIGHT2P_MAX_ITERS, more than 1024 points or more than 65535
 * sets; HV_ERR_INVALID: ...FailureProbability outside (0, 1), ...ErrorThresh <= 0, ...MaxIterations < 1, ...MinIterations >
 * ...MaxIterations, ransacMinInlierFraction outside [0, 1] or a NULL required pointer. The parameter and size checks come
 * before the context is looked at. The launches are timed under HV_K_RANSAC3. */
#define HV_UPRIGHT2P_MAX_ITERS 500
typedef struct hv_upright2p_params {
    double ransacStereoUpright2pErrorThresh; double ransacStereoUpright2pFailureProbability;
    int ransacStereoUpright2pMaxIterations; int ransacStereoUpright2pMinIterations; int ransacStereoUpright2pUseMle;
    double ransacMinInlierFraction;
} hv_upright2p_params;
void hv_upright2p_default_params(hv_upright2p_params *p);   /* 1e-4, 1e-4, 500, 50, 1, 0.3 */
/* StereoUpright2p::compute on one set of n features: poses[32], status[n] int32 Feature::Status in/out (entries other than
 * TRACKED stay), model[12] (NULL ok) = R row-major then t, world1 = R world0 + t, zeros without a model; summary[4]
 * (NULL ok) = {inlier count, iteration of the best model (-1: none), iterations run, correspondences m}. Fewer than 2
 * correspondences: not run, {0, -1, 0, m}. Synchronous; host pointers, staged through the context's arena. */
int hv_upright2p(hv_ctx *ctx, const hv_upright2p_params *p, int n, const float *prev_left_xy, const float *prev_right_xy,
                 const float *cur_left_xy, const hv_camera_model *camera0, const hv_camera_model *camera1,
                 const double *second_to_first, const double *poses, const uint32_t *draws, int *status, double *model,
                 int *summary);
/* n_sets sets in device memory, laid out as for hv_ransac3_batch_dev; poses_dev [n_sets][2][16], draws_dev
 * [n_sets][2 * ransacStereoUpright2pMaxIterations], model_dev [n_sets][12] and summary_dev [n_sets][4] (NULL ok).
 * Asynchronous on the context stream, no allocation or synchronisation inside (capturable in a HIP graph). */
int hv_upright2p_batch_dev(hv_ctx *ctx, const hv_upright2p_params *p, int n_sets, int max_points, const int *n_points_dev,
                           const float *prev_left_dev, const float *prev_right_dev, const float *cur_left_dev,
                           const hv_camera_model *camera0, const hv_camera_model *camera1, const double *second_to_first,
                           const double *poses_dev, const uint32_t *draws_dev, int *status_dev, double *model_dev,
                           int *summary_dev);
/* The stereo device chain step after hv_rot_ransac_lk_batch_dev for the hv_ekf_batch(ekf) resident sequences of a filter
 * batch (set s is filter s), on the filter's context stream: RansacPipeline::compute on the UPRIGHT_2P branch with the poses
 * of backend.cpp:667-679 formed on the device from the mean, poses[0] = toCameraToWorld(historyPosition(0),
 * historyOrientation(0)) and poses[1] = toCameraToWorld(position(), orientation()) (src/odometry/util.cpp:144-158) with
 * cam_params->cameraToImu, the caller's inverse of imuToCamera (as hv_flow_predict_batch_dev; the other members are not
 * read). It belongs where Session::applyTracker runs: after the frame's IMU predicts and before the visual update.
 * track_status_dev, r2_summary_dev, score_dev and the corner arguments are those of hv_ransac3_lk_batch_dev; result_dev
 * [n_sets][2] = {type 0 SKIPPED / 4 UPRIGHT_2P, inlierCount}. A set whose mean is non-finite ends SKIPPED and touches no
 * other set. After the checks above: HV_ERR_INVALID for a NULL handle, HV_ERR_UNSUPPORTED for a state of fewer than 27
 * entries. Asynchronous, capturable. */
int hv_upright2p_lk_batch_dev(hv_ekf *ekf, const hv_upright2p_params *p, const hv_flow_predict_params *cam_params,
                              int max_points, const int *n_points_dev, const float *prev_left_dev,
                              const float *prev_right_dev, const float *cur_left_dev, int *track_status_dev,
                              const int *r2_summary_dev, const hv_camera_model *camera0, const hv_camera_model *camera1,
                              const double *second_to_first, const uint32_t *draws_dev, int *result_dev, double *score_dev,
                              double *model_dev, int *summary_dev);

/* ---- device session lifecycle: tracking status, reset rules, in-place re-initialisation (added within ABI 4) ------------
 * Replaces, for the hv_ekf_batch(ekf) resident sequences of a filter batch (set s is filter s), what Session and Control do
 * around a frame besides the filter algebra: the filter's sample clock (src/odometry/ekf.cpp:357-366) and
 * initializeOrientation on the first IMU sample (ekf.cpp:299-317, backend.cpp:728-731), the ring of good-frame flags that
 * decides Session::trackingStatus (backend.cpp:195-198, 807-819; CircularBuffer, odometry/util.hpp:111-149), Control's
 * persistent status, freeze flag and reset rules (control.cpp:117-149), and the reset itself (control.cpp:49-65): a new Session --
 * filter, tracker, trail index, control flags -- written in place for the sets that reset, with initializeAtPose
 * (backend.cpp:224-229) for reset(true). Equal, array for array, to the literal restatement in tests/session_restatement.py.
 * The state is device memory owned by the caller (like hv_track_table).
 * All _dev entries: one launch, one workgroup per set, asynchronous on the filter's context stream, timed under
 * HV_K_EKF_CONTROL, no allocation, copy-back or synchronisation inside (capturable in a HIP graph). Checks, in this order, the
 * first two groups decided before the handle is looked at: HV_ERR_INVALID for a NULL required pointer (a member of a state
 * struct included) or the argument ranges stated below; HV_ERR_UNSUPPORTED for a ring of more than HV_SESSION_MAX_WINDOW
 * entries; HV_ERR_INVALID for a NULL handle; HV_ERR_UNSUPPORTED for more than 65535 sets or a state of more than 1024 entries.
 * Masked-out sets (hv_session_imu_dev) and sets that do not reset (hv_session_reset_dev) are not touched at all.
 * The zero-vector rule: initializeOrientation normalises the acceleration with Eigen's normalized(), which leaves a zero vector
 * zero (Eigen >= 3.3); FromTwoVectors then sees c = 0 and a zero axis and returns q = (sqrt(2) / 2, 0, 0, 0), which is not a unit
 * quaternion. initializeAtPose calls initializeOrientation(0), so this is the q0 of every reset(true); it is kept as it is. */
#define HV_SESSION_MAX_WINDOW 256
enum { HV_TRACKING_INIT = 0, HV_TRACKING_TRACKING = 1, HV_TRACKING_LOST = 2 };      /* api::TrackingStatus */
enum { HV_RESET_NONE = 0, HV_RESET_FRESH = 1, HV_RESET_KEEP_POSE = 2 };             /* none, reset(false), reset(true) */
typedef struct hv_session_params {
    double targetFps;                              /* 30    codegen/parameter_definitions.c:220 */
    int visualUpdateForEveryNFrame;                /* 1     :4   */
    double goodFramesTimeWindowSeconds;            /* 2.0   :204 */
    double goodFramesToTracking;                   /* 0.75  :201 */
    double goodFramesToTrackingFailed;             /* 0.05  :202 */
    int resetUntilInitSucceeds;                    /* 0     :193 */
    int resetOnFailedTracking;                     /* 0     :195 */
    double resetAfterTrackingFailsToInitialize;    /* 3.0   :197 */
    int freezeOnFailedTracking;                    /* 0     :199 */
} hv_session_params;
void hv_session_default_params(hv_session_params *p);
/* The ring holds W = (size_t)((double)targetFps / (double)visualUpdateForEveryNFrame * goodFramesTimeWindowSeconds) flags
 * (backend.cpp:195-197; 60 with the defaults), computed on the host in every entry that takes the parameters:
 * visualUpdateForEveryNFrame < 1 or W < 1 is HV_ERR_INVALID, W > HV_SESSION_MAX_WINDOW is HV_ERR_UNSUPPORTED. */
typedef struct hv_session {                /* [n_sets] unless noted */
    float   *good_ring;               /* [n_sets][W]  Session::visualUpdateCounter.mBuffer */
    int32_t *ring_head;               /* mHead */
    int32_t *ring_entries;            /* mEntries */
    int32_t *tracking_status;         /* Session::trackingStatus */
    int32_t *control_status;          /* Control::controlTrackingStatus */
    double  *last_reset_time;         /* Control::lastResetTime */
    uint8_t *first_sample;            /* EKF::firstSample */
    double  *first_sample_t;          /* EKF::firstSampleT */
    double  *prev_sample_t;           /* EKF::prevSampleT */
    double  *time;                    /* EKF::time */
    uint8_t *initialized_orientation; /* Session::initializedOrientation */
} hv_session;
/* A Control with its first Session, straight after construction: the ring empty (its W entries 0, head and entries 0), both
 * statuses INIT, last_reset_time 0.0, first_sample 1, first_sample_t and prev_sample_t -1.0, time 0.0,
 * initialized_orientation 0. The filter is not touched. */
int hv_session_init_dev(hv_ekf *ekf, const hv_session_params *p, const hv_session *st);
/* The session part of the n_samples IMU samples in front of a frame (1 <= n_samples <= HV_EKF_MAX_PREDICT_SAMPLES), in the layout
 * of hv_ekf_predict_n_dev: t_dev [n_samples][batch] the sample times, acc_dev [n_samples][batch][3]; active_dev [batch] uint8
 * (NULL: all). Per active filter, in sample order:
 * - while initialized_orientation is 0: initializeOrientation(acc) as oracle/ekf_oracle.c:285-311 (its antiparallel branch
 *   included) under the zero-vector rule above, then the flag is set. Writes m[ORI .. ORI + 3] and the 4 x 4 ORI block of P,
 *   nothing else of the filter.
 * - the clock: first_sample set: first_sample_t = t, the flag cleared, dt = 0; otherwise dt = t - prev_sample_t and
 *   time = t - first_sample_t, one rounded subtraction each; then prev_sample_t = t.
 * dt_dev [n_samples][batch] receives dt: the dt_dev of hv_ekf_predict_n_dev, whose kernels skip a sample unless dt > 0
 * (csrc/ekf_predict.hip), as ekf.cpp:367 does. time_dev [n_samples][batch] receives the clock after the sample: row
 * n_samples - 1 is the time_dev of hv_ekf_imu_control_dev, hv_ekf_frame_control_dev and hv_trail_select_batch_dev.
 * A masked filter gets dt 0 and its stored time in every row. */
int hv_session_imu_dev(hv_ekf *ekf, const hv_session *st, int n_samples, const double *t_dev, const double *acc_dev,
                       const unsigned char *active_dev, double *dt_dev, double *time_dev);
/* Once per processed frame, behind hv_trail_finish_batch_dev. good_frame_dev [batch] uint8 as that entry wrote it;
 * full_update_dev [batch] uint8 (NULL: every frame is a full update). Per set:
 * - backend.cpp:807-819: on a full update put(good ? 1.0f : 0.0f); when entries > W / 2 (integer division) the mean as
 *   CircularBuffer::mean() forms it (a binary32 sum over mBuffer[0 .. entries) divided by the count), widened to binary64, moves
 *   tracking_status to TRACKING above goodFramesToTracking and from TRACKING to LOST below goodFramesToTrackingFailed.
 * - control.cpp:121-149 with t = first_sample_t + time: status_dev [batch] int32 = control_status BEFORE its update (what
 *   output.trackingStatus carries); frozen_dev [batch] uint8 = freezeOnFailedTracking && control_status != INIT &&
 *   tracking_status != TRACKING; then control_status takes tracking_status unless that would return it to INIT; then, with
 *   expired = last_reset_time + resetAfterTrackingFailsToInitialize < t, the first rule that holds of
 *     control_status == INIT && expired && resetUntilInitSucceeds         -> HV_RESET_FRESH
 *     resetOnFailedTracking && tracking_status == LOST                    -> HV_RESET_KEEP_POSE
 *     control_status != INIT && tracking_status == INIT && expired        -> HV_RESET_KEEP_POSE
 *   goes to reset_kind_dev [batch] int32 (else HV_RESET_NONE).
 * status_dev and frozen_dev may be NULL. The entry decides a reset; hv_session_reset_dev performs it. */
int hv_session_status_dev(hv_ekf *ekf, const hv_session_params *p, const hv_session *st, const unsigned char *good_frame_dev,
                          const unsigned char *full_update_dev, int32_t *status_dev, unsigned char *frozen_dev,
                          int32_t *reset_kind_dev);
/* Control::reset for the sets whose reset_kind_dev [batch] int32 is HV_RESET_FRESH or HV_RESET_KEEP_POSE, in one launch:
 * - pos = m[POS ..] and q = m[ORI ..] are read first; last_reset_time = first_sample_t + time of the old clock.
 * - the filter becomes what hv_ekf_create writes: m, all of P (in the covariance buffer that is current: fetch nothing again,
 *   the ping-pong of hv_ekf_augment is not moved), the 12 x 12 Q, dydx zero.
 * - HV_RESET_KEEP_POSE: initializeOrientation(0) under the zero-vector rule, then transformTo(pos, q) (ekf.cpp:704-758)
 *   applied literally with that q0 = (sqrt(2) / 2, 0, 0, 0): qChange has norm sqrt(1 / 2), so the mean's orientation is q / 2
 *   until the next predict normalises it, and the P blocks carry the factor 1 / 4 or 1 / 2 the reference's have. The fresh P
 *   is block diagonal, so A P A' is formed block by block. initialized_orientation = 1. HV_RESET_FRESH: initialized_orientation = 0.
 * - the set's slice of table, trail and ctl as hv_tracks_init_batch_dev, hv_trail_init_batch_dev and hv_ekf_control_init_dev
 *   write it (the argument checks of those entries apply, their limits HV_TRACKS_MAX_TRACKS and HV_TRAIL_MAX_POSES included;
 *   tracks_p->maxTracks must equal trail_p->maxTracks: HV_ERR_INVALID otherwise).
 * - the session: ring empty, tracking_status INIT, first_sample 1, first_sample_t and prev_sample_t -1.0, time 0.0;
 *   control_status is Control's and is kept.
 * Sequence-wide random draws (sharedData->rng) survive a reset in the reference; they are the caller's (draws_dev). */
int hv_session_reset_dev(hv_ekf *ekf, const hv_session_params *p, const hv_session *st, const hv_ekf_control *ctl,
                         const hv_track_table_params *tracks_p, const hv_track_table *table,
                         const hv_trail_index_params *trail_p, const hv_trail_index *trail, const int32_t *reset_kind_dev);

/* ---- device output stage: pose, covariances, pose trail, point cloud (added within ABI 4) ------------------------------
 * Replaces, for the hv_ekf_batch(ekf) resident sequences of a filter batch (set s is filter s), what a session hands back at the
 * end of a frame: src/odometry/backend.cpp:840-860 (transformInertialState :69-79, setFromEKF output.cpp:50-77, computePose
 * :1368-1386, getPointCloud :255-280 over the point-cloud lines of the visit loop :905, 1066-1070, 1118, 1124, 1191, 1239-1251),
 * Control's overwrite of t and trackingStatus (control.cpp:117-128) and the API's convertOutputPose (src/api/api.cpp:726-742,
 * 759-808). One small record per set instead of a read-back of m, P and the index. Literal restatement:
 * tests/output_restatement.py. Position in a frame: behind hv_trail_finish_batch_dev, the frame's augmentation and
 * hv_session_status_dev, in front of hv_session_reset_dev. Per set, in binary64 and in the operation order of the restatement:
 * - a set whose frozen_dev is 1 is not written at all (control.cpp:128);
 * - t = first_sample_t + time, one rounded addition; tracking_status = tracking_status_dev; stationary_visual = stationary_dev;
 * - the inertial state: (pos, ori) = toOdometryPose(toWorldToCamera(m[POS], m[ORI], imuToCamera) * slamToOdometry, imuToCamera)
 *   (util.cpp:121-142; rmat2quat = Eigen::Quaterniond(Matrix3d), the inverse of the 4 x 4 through its cofactors with one
 *   reciprocal of the determinant), then EKF::transformTo(pos, ori) (ekf.cpp:704-757) on m[0 .. 20) and P[0 .. 20, 0 .. 20): A is
 *   block diagonal, so only its POS, VEL and ORI blocks of A P A' are formed. inertial_mean [20], inertial_cov_diag [20],
 *   position_cov / velocity_cov [9] row-major. A set that is not ready, or NULL matrices, use the identity for both transforms;
 * - the pose trail: n_trail = n_keyframes - 1 as finish left it; trail_time[i] = the timestamp of keyframe i + 1; trail_pose[i]
 *   [7] = position, orientation (w, x, y, z) of computePose(i) from history pose i of the mean, zeros for a set that is not
 *   ready; entries behind n_trail are not written. Deviation: with exactly one historical pose the reference leaves element 0 as
 *   setFromEKF of its coordinate filter wrote it, a slot that filter never initialises; here it is computePose(0) like every other;
 * - the point cloud: the candidates in visit order; visited = status[v][0] != HV_TRI_NOT_VISITED; the loop stops at the visit
 *   that brings the successes (gate status INLIER) to maxSuccessfulVisualUpdates (<= 0: no such limit) or the attempts to
 *   maxVisualUpdates, the rule of hv_trail_finish_batch_dev, and that candidate is NOT appended (the break at :1244 precedes the
 *   push at :1249); every visited candidate in front of it whose triangulation status is HV_TRI_OK is appended with its ID,
 *   point_status 4 (OUTLIER) when its prepare status is HV_PREPARE_VU_OK and its gate status is not INLIER, else 1 (POSE_TRAIL),
 *   point_first_pixel = image_point of the candidate's column (cand_col), first camera, in keyframe 1 (the frame's keyframe,
 *   which finish's push leaves untouched), and point_xyz = odometryToSlam applied to pf_dev. A set that is not ready has
 *   n_points = 0; entries behind n_points are not written;
 * - api_pose [7] and api_trail_pose[i] [7]: convertOutputPose of the transformed inertial pose and of trail_pose[i], with the
 *   reference's inverted test: a non-identity imuToOutput passes the pose through, the identity sends it through
 *   toWorldToCamera / toOdometryPose, so the orientation carries rmat2quat's sign, not the filter's.
 * A non-finite mean gives whatever this arithmetic yields in its own set and touches no other. The cloud of fullPointCloud -- this
 * one, the stopping candidate and every remaining track -- is hv_full_point_cloud_dev's (below); the hybrid map and the stereo-depth
 * cloud are unsupported, like in the index; SLAM itself is the caller's (setCoordinates supplies the matrices).
 * One launch of one wavefront per set on the filter's context stream, timed under HV_K_EKF_CONTROL, no allocation, copy-back or
 * synchronisation inside (capturable in a HIP graph). Checks, the first two groups decided before the handle is looked at:
 * HV_ERR_INVALID for a NULL required pointer (p, st and its first_sample_t / time, trail and every member, in and its members
 * but frozen_dev, stationary_dev, ready_dev and the two matrices -- of which both or none are given --, out and every member),
 * cameraTrailLength, maxTracks or maxVisualUpdates < 1; HV_ERR_UNSUPPORTED for maxVisualUpdates > HV_TRAIL_MAX_VISITS or
 * cameraTrailLength + 1 > HV_TRAIL_MAX_POSES; HV_ERR_INVALID for a NULL handle; HV_ERR_UNSUPPORTED for more than 65535 sets, a
 * state of more than 1024 or of fewer than 20 + 7 * cameraTrailLength entries. Counts and indices read from device memory
 * (n_keyframes, n_candidates, kf_row, cand_col) are clamped to their capacity. */
typedef struct hv_output_params {
    double imuToCamera[16], imuToOutput[16];   /* row-major; identity */
    int maxVisualUpdates;                      /* 20   V of the visit arrays */
    int maxSuccessfulVisualUpdates;            /* 5 */
    int cameraTrailLength;                     /* 20   K = cameraTrailLength + 1 of the index */
    int maxTracks;                             /* 200  M of the index */
    int useStereo;                             /* 1    C of the index */
} hv_output_params;
void hv_output_default_params(hv_output_params *p);
/* What the frame's other entries wrote, device memory; V = maxVisualUpdates. */
typedef struct hv_output_frame {
    const int32_t *cand_id_dev;           /* [V][n_sets]      hv_trail_select_batch_dev */
    const int32_t *n_candidates_dev;      /* [n_sets] */
    const int32_t *status_dev;            /* [V][n_sets][2]   hv_ekf_visual_frame_ragged_dev */
    const int32_t *gate_status_dev;       /* [V][n_sets] */
    const double  *pf_dev;                /* [V][n_sets][3] */
    const int32_t *tracking_status_dev;   /* [n_sets]         status_dev of hv_session_status_dev */
    const uint8_t *frozen_dev;            /* [n_sets]         frozen_dev of hv_session_status_dev; NULL: nothing is frozen */
    const uint8_t *stationary_dev;        /* [n_sets]         stationary_dev of hv_ekf_frame_control_dev; NULL: 0 */
    const double  *slam_to_odometry_dev;  /* [n_sets][16]     row-major, odo.inverse() * slam (backend.cpp:61); NULL (both): identity */
    const double  *odometry_to_slam_dev;  /* [n_sets][16]     slam.inverse() * odo (:62) */
    const uint8_t *ready_dev;             /* [n_sets]         isReady(); NULL: ready (the reference without -useSlam) */
} hv_output_frame;
/* The record, device memory owned by the caller; [n_sets] unless noted, T = cameraTrailLength. */
typedef struct hv_output {
    double  *t;                  /* Output::t as Control leaves it */
    int32_t *tracking_status;    /* api::TrackingStatus */
    uint8_t *stationary_visual;
    double  *inertial_mean;      /* [n_sets][20] */
    double  *inertial_cov_diag;  /* [n_sets][20] */
    double  *position_cov;       /* [n_sets][9] */
    double  *velocity_cov;       /* [n_sets][9] */
    int32_t *n_trail;
    double  *trail_time;         /* [n_sets][T] */
    double  *trail_pose;         /* [n_sets][T][7] */
    double  *api_pose;           /* [n_sets][7] */
    double  *api_trail_pose;     /* [n_sets][T][7] */
    int32_t *n_points;
    int32_t *point_id;           /* [n_sets][V] */
    int32_t *point_status;       /* [n_sets][V]  PointFeature::Status: 1 POSE_TRAIL, 4 OUTLIER */
    float   *point_first_pixel;  /* [n_sets][V][2] */
    double  *point_xyz;          /* [n_sets][V][3] */
} hv_output;
int hv_output_dev(hv_ekf *ekf, const hv_output_params *p, const hv_session *st, const hv_trail_index *trail,
                  const hv_output_frame *in, const hv_output *out);

/* ---- device full point cloud: triangulate every remaining track of a frame (added within ABI 4) ----
 * odometry.fullPointCloud ("triangulate all tracks on each frame to get the full point cloud", codegen/parameter_definitions.c:
 * 54-56) for the hv_ekf_batch(ekf) resident sequences of a filter batch (set s is filter s). With it the visit loop of
 * Session::trackerVisualUpdate (backend.cpp:1012-1252) does not break where its limits set needMoreVisualUpdates = false
 * (:1242-1247). Calling this entry is the switch: the fullPointCloud field of tp is not read, and hv_trail_*_batch_dev and
 * hv_output_dev keep stating the loop that breaks. Literal restatement: tests/full_cloud_restatement.py.
 * Position in a frame: behind hv_ekf_visual_frame_ragged_dev, in front of hv_trail_finish_batch_dev and the augmentation: the
 * index is as select left it (the head is keyframe 0 and holds this frame's corners, the `used` marks and the previous blacklist
 * are last frame's, the pose indices match the mean). The entry only reads the filter, the index and the table. Per set:
 * - the prefix: the candidates in visit order under the stop rule of hv_trail_finish_batch_dev / hv_output_dev; every visited
 *   candidate up to AND INCLUDING the stopping one (its push at :1249-1251 is no longer behind a break) whose triangulation status
 *   is HV_TRI_OK is appended with its ID, point_status 4 (OUTLIER) when its prepare status is HV_PREPARE_VU_OK and its gate status
 *   is not INLIER, else 1 (POSE_TRAIL), point_first_pixel = image_point of its column, first camera, keyframe 0, and point_xyz =
 *   odometryToSlam applied to pf_dev;
 * - the tail: every track behind the stop in the shuffled trackOrder -- derived again from the table, the index and draws_dev by
 *   the rules of select -- that passes the filter of :1017-1038: skipped when scoreVisualUpdateTracks and score < minTrackScore,
 *   then when nValid < trackMinFrames, then on a frame that is not a full update. The previous-blacklist test (:1039-1046) is
 *   conditioned on needMoreVisualUpdates: a track blacklisted in the previous frame is triangulated and not blacklisted again
 *   (hv_trail_finish_batch_dev agrees: a skipped track enters the new blacklist only when its position precedes the stop);
 * - each tail track: createTrackIndex (GAP or ALL) as tail_pose_mask, buildTrackVectors read in place from norm_point,
 *   extractCameraPoseTrail (triangulation.cpp:65-103) from the current mean through imuToCamera / secondImuToCamera of vp,
 *   Triangulator::triangulate (:120-407), the iterative method without derivatives -- triangulateWithTwoCameras between pose 0
 *   and the last pose of the first camera, inverseDepth, Gauss-Newton with the 3 x 3 solve and its rcond, the convergence test,
 *   the way back, pf == p0, isBehind -- then the depth window of backend.cpp:1096-1099 from vp; tail_status is the
 *   TriangulatorStatus after that window (the reference's triangulationForPointCloud statistics); an OK track is appended behind
 *   the prefix in tail order with status POSE_TRAIL (:1126-1132). pf and the status do not depend on calculateDerivatives;
 * - n_attempts = the visits the loop counted + n_tail (:1121) and good_frame = (stationary || stopped) && !(n_attempts -
 *   successes > 5) (:1272-1274), the reference's values WITH fullPointCloud: the tail's attempts make tooManyFailures true on
 *   almost every frame with more than a handful of tail tracks. hv_trail_finish_batch_dev reports the values without the tail;
 *   the caller decides which one feeds hv_session_status_dev;
 * - a loop that never stopped has no tail: the cloud is the one hv_output_dev reports; a set that is not ready has n_points = 0
 *   (getPointCloud, :255-280), its tail and counters are still reported. Entries behind n_points / n_tail are not written.
 * Nothing is gated, applied, marked used, blacklisted or deleted; mean, covariance, index and table are not written.
 * Two launches, one workgroup per set each, on the filter's context stream: the index kernel, timed under HV_K_TRAIL_INDEX, and
 * the triangulation kernel, one lane per tail track, timed under HV_K_VU_TRI; no allocation, copy-back or synchronisation inside
 * (capturable in a HIP graph). Checks, in this order: HV_ERR_INVALID for the parameter errors of hv_trail_*_batch_dev, a NULL
 * required pointer (tp, vp, trail and every member, table and its n_tracks / ids, in and its members but full_update_dev,
 * stationary_dev, odometry_to_slam_dev and ready_dev, out and every member but n_attempts and good_frame) or a useStereo that
 * differs between tp and vp; HV_ERR_UNSUPPORTED for the index's limits (maxTracks > HV_TRACKS_MAX_TRACKS, maxSize >
 * HV_TRAIL_MAX_POSES, maxVisualUpdates outside 1 .. HV_TRAIL_MAX_VISITS, TrackSampling::RANDOM, hybridMapSize > 0,
 * useIndependentStereoTriangulation) and for useLinearTriangulation (the tail states the iterative method only: the closed form
 * has no Gauss-Newton loop to share with it, and the visit loop's own linear front carries derivatives the cloud never reads);
 * HV_ERR_INVALID for a NULL handle; HV_ERR_UNSUPPORTED for more than 65535 sets or a state shorter than 20 + 7 *
 * cameraTrailLength. Counts and indices read from device memory (n_tracks, n_keyframes, n_candidates, kf_row, col_len, cand_col,
 * cand_pos, and the entry's own n_tail / tail_col between its two kernels) are clamped to their capacity. */
typedef struct hv_full_cloud_frame {      /* device memory; V = maxVisualUpdates, M = maxTracks */
    const uint32_t *draws_dev;            /* [n_sets][M]      as given to hv_trail_select_batch_dev */
    const uint8_t  *full_update_dev;      /* [n_sets]         as given to select; NULL: every frame is full */
    const int32_t  *cand_id_dev;          /* [V][n_sets]      hv_trail_select_batch_dev */
    const int32_t  *n_candidates_dev;     /* [n_sets] */
    const int32_t  *status_dev;           /* [V][n_sets][2]   hv_ekf_visual_frame_ragged_dev */
    const int32_t  *gate_status_dev;      /* [V][n_sets] */
    const double   *pf_dev;               /* [V][n_sets][3] */
    const uint8_t  *stationary_dev;       /* [n_sets]         stationary_dev of hv_ekf_frame_control_dev; NULL: 0 */
    const double   *odometry_to_slam_dev; /* [n_sets][16]     row-major, slam.inverse() * odo (backend.cpp:62); NULL: identity */
    const uint8_t  *ready_dev;            /* [n_sets]         isReady(); NULL: ready */
} hv_full_cloud_frame;
typedef struct hv_full_cloud {            /* device memory owned by the caller; [n_sets] unless noted */
    int32_t  *n_points;
    int32_t  *point_id;           /* [n_sets][M]     the visited prefix with the stopping candidate, then the tail's OK tracks */
    int32_t  *point_status;       /* [n_sets][M]     PointFeature::Status: 1 POSE_TRAIL, 4 OUTLIER */
    float    *point_first_pixel;  /* [n_sets][M][2] */
    double   *point_xyz;          /* [n_sets][M][3] */
    int32_t  *n_tail;
    int32_t  *tail_id;            /* [n_sets][M]     the tail in trackOrder order */
    int32_t  *tail_status;        /* [n_sets][M]     TriangulatorStatus after the depth window */
    int32_t  *tail_col;           /* [n_sets][M]     the track's column of the index */
    uint64_t *tail_pose_mask;     /* [n_sets][M]     bit k = keyframe k is in poseTrailIndex */
    int32_t  *n_attempts;         /* optional: updateAttemptCount with the tail */
    uint8_t  *good_frame;         /* optional: goodFrame with the tail */
} hv_full_cloud;
int hv_full_point_cloud_dev(hv_ekf *ekf, const hv_trail_index_params *tp, const hv_vu_params *vp, const hv_trail_index *trail,
                            const hv_track_table *table, const hv_full_cloud_frame *in, const hv_full_cloud *out);

/* ---- device std::mt19937 streams: the draws of the RANSAC filters and of the shuffle (added within ABI 4) --------------
 * Replaces, for n_sets resident sequences, the host generators whose raw outputs the entries above take as draws_dev and
 * the step "read the consumed count back, advance the generator" behind them: a std::mt19937 per sequence and per generator
 * in device memory owned by the caller (like hv_trail_index), one hv_rng each for
 * - the pipeline's generator (src/tracker/ransac_pipeline.cpp:46,66), read by RotRansac::fit (src/tracker/rot_ransac.cpp:74-96),
 *   two outputs per hypothesis visited: draw 200, hv_rot_ransac_lk_batch_dev, advance(summary_dev + 1, 2, 2, 200);
 * - RANSAC3's own (ransac_pipeline.cpp:78), three outputs per iteration run: draw 3 * ransac3MaxIterations, hv_ransac3*_batch_dev,
 *   advance(summary_dev + 2, 4, 3, 3 * ransac3MaxIterations);
 * - the upright 2-point filter's own (src/tracker/stereo_upright_2p.cpp:101), two per iteration: draw 2 *
 *   ransacStereoUpright2pMaxIterations, hv_upright2p*_batch_dev, advance(summary_dev + 2, 4, 2, 2 * ...MaxIterations);
 * - the odometry generator (src/odometry/backend.cpp:107,117,193), read by shuffleDeterministic (src/util/util.hpp:39-44,
 *   backend.cpp:964): draw maxTracks, hv_trail_select_batch_dev, the visit loop, hv_full_point_cloud_dev on the same buffer,
 *   advance(draws_used_dev, 1, 1, maxTracks).
 * Control::reset (src/odometry/control.cpp:49-65) builds a new Session and with it a new tracker, whose three generators start again
 * from ransacRngSeed; the odometry generator belongs to the shared data and survives (backend.cpp:107-117,193). So a caller
 * runs hv_rng_seed_batch_dev(..., reset_kind_dev) on the three tracker generators behind hv_session_reset_dev, never on the
 * odometry one.
 * The stored state is the engine's own, lazy as in libstdc++ (bits/random.tcc): mt is the array of the last twist and pos the
 * number of its words already handed out; a twist happens only when an output needs it, so pos is 624 after seeding and
 * 1 .. 624 after any output, and mt / pos compare bit for bit with tests/rng_restatement.py and with the state of numpy's
 * legacy-seeded MT19937.
 * All entries: one launch of one wavefront per set on the context stream, timed under HV_K_TRAIL_INDEX, no allocation or
 * synchronisation inside (capturable in a HIP graph). Checks made before the context is looked at: HV_ERR_INVALID for a NULL
 * required pointer (a state member included), a negative size, n_draws < 1, multiplier < 1, count_stride < 1; then
 * HV_ERR_UNSUPPORTED for n_sets > 65535, n_draws or max_draws above HV_RNG_MAX_DRAWS. n_sets = 0 returns HV_OK without a
 * launch. Values read from device memory are clamped: pos to 0 .. 624, counts as stated at hv_rng_advance_batch_dev. */
#define HV_RNG_STATE_WORDS 624
#define HV_RNG_MAX_DRAWS   2048          /* >= 3 * HV_RANSAC3_MAX_ITERS */
typedef struct hv_rng {                  /* device memory owned by the caller */
    uint32_t *mt;                        /* [n_sets][624] */
    int32_t  *pos;                       /* [n_sets]  words of mt already handed out: 1 .. 624, 624 = twist before the next output */
} hv_rng;
/* std::mt19937(seed) (the constructors of ransac_pipeline.cpp:66,78, stereo_upright_2p.cpp:101 and backend.cpp:117):
 * mt[0] = seed, mt[i] = 1812433253 * (mt[i-1] ^ (mt[i-1] >> 30)) + i, pos = 624. seed_dev [n_sets] or NULL (every set takes
 * `seed`). reset_kind_dev [n_sets] int32 or NULL (every set): only sets whose entry is HV_RESET_FRESH or HV_RESET_KEEP_POSE are
 * written, the others keep mt and pos bit for bit. */
int hv_rng_seed_batch_dev(hv_ctx *ctx, int n_sets, const hv_rng *rng, uint32_t seed, const uint32_t *seed_dev,
                          const int32_t *reset_kind_dev);
/* draws_dev [n_sets][n_draws] = what the next n_draws calls of rng() would return (the rng() of rot_ransac.cpp:75-76 and of
 * util.hpp:39-44); the state is NOT changed: the consumer decides how many of them count, and hv_full_point_cloud_dev reads
 * the same draws as hv_trail_select_batch_dev did. 1 <= n_draws <= HV_RNG_MAX_DRAWS. */
int hv_rng_draw_batch_dev(hv_ctx *ctx, int n_sets, const hv_rng *rng, int n_draws, uint32_t *draws_dev);
/* The state after c further calls of rng(), c = min(multiplier * clamp(count_dev[s * count_stride], 0, max_draws), max_draws),
 * 0 <= max_draws <= HV_RNG_MAX_DRAWS: what the loop of rot_ransac.cpp:74-96 leaves behind when it ends at the first all-inlier
 * hypothesis, and the samplers of the two own generators and the shuffle likewise. count_dev = summary_dev + 1, stride 2,
 * multiplier 2 for RANSAC2; summary_dev + 2, stride 4, multiplier 3 (RANSAC3) or 2 (upright 2-point); draws_used_dev, stride 1,
 * multiplier 1. A set with c = 0 is not written at all; after c > 0, pos is in 1 .. 624. */
int hv_rng_advance_batch_dev(hv_ctx *ctx, int n_sets, const hv_rng *rng, const int32_t *count_dev, int count_stride,
                             int multiplier, int max_draws);

/* ---- intensity matching: stereo and successive-frame equalisation -----------------------------
 * tracker::util::matchIntensities (src/tracker/util.cpp:173-179: cv::meanStdDev of l, then setIntensities(r, r, mean, stddev,
 * weight), util.cpp:16-52) as the command line runs it in front of everything else on every frame (src/commandline/main.cpp:763-777;
 * options tracker.matchStereoIntensities / matchSuccessiveIntensities, codegen/parameter_definitions.c:533-534), for a batch of
 * resident sequences. Per set:
 * - matchSuccessiveIntensities = w > 0 (main.cpp:763-769): the left frame is matched against prevGrayFrame with weight w;
 *   prevGrayFrame is the frame itself on the first frame (:766), and the MATCHED frame becomes the next prevGrayFrame (:768);
 * - right_dev != NULL and matchStereoIntensities (main.cpp:770-777, useStereo && matchStereoIntensities): the right frame is
 *   matched against the left one -- the already matched one if the first step ran -- with weight 1.
 * setIntensities, all in binary64: stddev0 = meanStdDev(in).stddev; stddev = stddev0 + weight (stddev - stddev0); k = stddev /
 * stddev0; mean0 = double(sum in) k / (rows cols); mean = mean0 + weight (mean - mean0); every pixel x becomes
 * clamp((int)round(double(x) k + mean - mean0), 0, 255), round() rounding halves away from zero. cv::meanStdDev of an 8-bit
 * image: exact integer sums, scale = 1 / N, mean = sum scale, stddev = sqrt(max(sqsum scale - mean^2, 0)) (the reference pins no
 * OpenCV version; every 4.x source computes this). A matched pixel depends on the input byte alone, so the kernels work on
 * 256-bin histograms and 256-entry tables, and prevGrayFrame is kept as the two exact sums of the matched frame
 * (hv_intensity_state): tests/intensity_match_restatement.py, DESIGN.md 3.23. prevGrayFrame is a local of run_algorithm and
 * survives Control::reset, so nothing here is tied to hv_session_reset_dev.
 * Two cases the reference leaves open:
 * - a constant image (stddev0 == 0): the reference asserts (util.cpp:33; Debug is its default build) and divides by zero without
 *   asserts. Here the image is left bit for bit as it is, HV_INTENSITY_CONSTANT_* is set in the set's record, and -- for the left
 *   frame -- its statistics still become the prev statistics;
 * - colour frames: the command line converts them with cv::cvtColor (main.cpp:765,774-775); these entries take 8-bit gray
 *   frames only, the conversion stays with the caller (hv_ingest_build* converts for the pyramid, not in the caller's buffer).
 * rows * cols is an int in the reference (util.cpp:41); here the pixel count is exact for every supported size. */
typedef struct hv_intensity_params {
    double matchSuccessiveIntensities;   /* weight of the successive step, 0 = off (default 0.0) */
    int matchStereoIntensities;          /* (default 0) */
} hv_intensity_params;
void hv_intensity_default_params(hv_intensity_params *p);   /* 0.0, 0 (parameter_definitions.c:533-534) */
typedef struct hv_intensity_state {      /* device memory owned by the caller */
    uint64_t *prev_sum, *prev_sqsum;     /* [n_sets] sum and squared sum of the previous matched left frame (prevGrayFrame) */
    int32_t  *has_prev;                  /* [n_sets] 0 until the first successive step of the set */
    uint32_t *hist;                      /* [n_sets][2][256] workspace: all zero between calls */
} hv_intensity_state;
enum { HV_INTENSITY_CONSTANT_LEFT = 1, HV_INTENSITY_CONSTANT_RIGHT = 2,     /* stddev0 == 0: the frame was left as it is */
       HV_INTENSITY_MATCHED_LEFT = 4, HV_INTENSITY_MATCHED_RIGHT = 8 };     /* the frame was rewritten */
typedef struct hv_intensity_record {     /* index 0 = left, 1 = right */
    uint64_t in_sum[2], in_sqsum[2];     /* of the frame as given; 0 for a frame the call does not look at */
    uint64_t out_sum[2], out_sqsum[2];   /* of the frame as left behind (= in_* unless HV_INTENSITY_MATCHED_*) */
    double k[2], mean0[2], mean[2];      /* devDivDev0, mean0 and the blended mean of setIntensities; 1, 0, 0 unless MATCHED */
    int32_t flags;                       /* HV_INTENSITY_* */
    int32_t reserved;                    /* 0 */
} hv_intensity_record;
/* has_prev, the prev sums and the workspace := 0. Every state member must be given. */
int hv_intensity_init_batch_dev(hv_ctx *ctx, int n_sets, const hv_intensity_state *state);
/* One frame of n_sets sequences. The frames are the caller's gray buffers (set s at left_dev + s * left_image_stride_bytes, rows
 * row_stride_bytes apart, likewise right_dev) and are modified in place; bytes between width and the row stride are neither read
 * nor written. Any alignment is served; 16-byte aligned bases and strides take 16-byte loads throughout. The call runs in front
 * of hv_pyramid_build_batch_dev or hv_ingest_build_batch_dev(channels = 1) on the same buffers and, as in the reference, before
 * any rectifying remap. right_dev NULL = mono. active_dev [n_sets] bytes or NULL (every set): an inactive set keeps its pixels,
 * state and record bit for bit. record_dev [n_sets] or NULL.
 * Three launches on the context stream (histograms; tables + rewrite; state, record and the cleared workspace), timed under
 * HV_K_INGEST, no allocation or synchronisation inside (capturable in a HIP graph); the result does not depend on scheduling.
 * Checks made before the context is looked at: HV_ERR_INVALID for a NULL params, left_dev, state or state->hist -- and, when the
 * successive step is on, a NULL prev_sum, prev_sqsum or has_prev --, a weight outside [0, 1], n_sets < 0, width or height < 1,
 * row_stride_bytes < width; then HV_ERR_UNSUPPORTED for width or height above 65535 or n_sets above 65535 (a grid dimension).
 * n_sets = 0, or neither step on (matchStereoIntensities with right_dev NULL included), returns HV_OK without a launch. */
int hv_match_intensities_batch_dev(hv_ctx *ctx, const hv_intensity_params *params, int n_sets, int width, int height,
                                   uint8_t *left_dev, long long left_image_stride_bytes, uint8_t *right_dev,
                                   long long right_image_stride_bytes, int row_stride_bytes, const hv_intensity_state *state,
                                   const unsigned char *active_dev, hv_intensity_record *record_dev);
/* matchIntensities(l, r, weight) (util.cpp:173-179) on one pair of host images: l is read, r is rewritten in place (a constant r
 * stays as it is). Synchronous; staged through the context's arena. weight in [0, 1] (util.cpp:26). */
int hv_match_intensities(hv_ctx *ctx, int width, int height, const uint8_t *l_host, int l_stride_bytes, uint8_t *r_host,
                         int r_stride_bytes, double weight);

/* ---- resident VIO engine: one object, one call per frame (added within ABI 4) ------------------------------------------
 * The default stereo session of n_sets resident sequences as ONE owned object: Session::process (src/odometry/backend.cpp:716-860)
 * with Tracker::add in front of it, assembled from the _dev entries above in the order INTEGRATION.md states ("The whole frame on
 * the device", "Between the table and the filter", "Around the frame"; "One call per frame" lists the calls of hv_vio_frame). The
 * engine adds no arithmetic of its own: every stage is the entry documented above, with the engine's buffers as its arguments.
 * What it adds is the ownership of those buffers and the per-frame state a caller of the long chains keeps on the host, here in
 * device memory (csrc/vio_engine.hip): the frame number of every set (frame->num = ++frameCount, src/odometry/sample_sync.cpp:138: the
 * first frame is 1, and a reset does not restart it), the rule fullVisualUpdate = frame->num %
 * visualUpdateForEveryNFrame == 0 || !canPopKeyframe() (backend.cpp:765, ekf_state_index.hpp:109), the zeroing of the per-frame
 * counters, the "has a previous frame" flag, and the roles of the three pyramid slots of a set.
 * hv_vio_params: one member per owned entry, each with that entry's own defaults (hv_vio_default_params calls their default
 * functions), the two cameras, and the scalars the reference derives per session:
 *   ransac2Threshold (4.0)        threshold_pow2 = (float)pow(ransac2Threshold * (min(w, h) / 720.0), 2), ransac_pipeline.cpp:87-88;
 *   trackChiTestOutlierR (1.5), visualR (0.05)   both divided by the focal length (fx + fy) / 2 of camera0, backend.cpp:996-997
 *                                 (a vu.trackRmseThreshold >= 0 likewise, :995);
 *   ransacRngSeed (4649), odometryRngSeed (0)    the seeds of the two tracker generators and of the odometry generator;
 *   imu_samples_max               the most IMU samples a frame may bring, 1 .. HV_EKF_MAX_PREDICT_SAMPLES (default: that limit);
 *   featureDetector, useRansac3, predictOpticalFlow, batchVisualUpdate   the reference's switches whose other settings the engine
 *                                 refuses (defaults HV_DETECTOR_GPU_GFTT, 1, 1, 0);
 *   ransac5, upright2p, fast, gftt_legacy, useStereoUpright2p (0), useHybridRansac (1)   the entries and switches only
 *                                 hv_vio_create_session reads (below), each struct with its own default function's values
 *                                 (parameter_definitions.c:298, 268 for the switches).
 * second_to_first of RANSAC3 is flow.imuToCamera * flow.secondCameraToImu; gate.cam0ToCam1 and the four matrices of `flow` are
 * the caller's, as for the entries themselves.
 * hv_vio_create decides, before the device is touched and in this order: HV_ERR_INVALID for a NULL params or out, n_sets < 1,
 * imu_samples_max outside 1 .. HV_EKF_MAX_PREDICT_SAMPLES, tracks.maxTracks != trail.maxTracks (or != gftt.maxTracks /
 * output.maxTracks), a cameraTrailLength, maxVisualUpdates or maxSuccessfulVisualUpdates that differs between ekf, trail and
 * output, trail.useStereo and output.useStereo disagreeing (vu.useStereo is not read: the engine's copy of vu takes
 * trail.useStereo, because hv_vu_default_params leaves it 0); then HV_ERR_UNSUPPORTED for everything outside the default
 * stereo session: mono (useStereo 0), featureDetector != HV_DETECTOR_GPU_GFTT, useRansac3 0 (hybrid RANSAC5, upright 2-point),
 * gate.independentStereoOpticalFlow, predictOpticalFlow 0, batchVisualUpdate, trail.fullPointCloud, ekf.hybridMapSize > 0, n_sets >
 * 65535, 3 * ransac3.ransac3MaxIterations > HV_RNG_MAX_DRAWS; then HV_ERR_INVALID for a NULL context, a context whose max_tracks is below
 * maxTracks or whose pool has fewer than 3 * n_sets free slots (the pool is never grown here: the caller sizes it). Whatever the
 * owned entries themselves refuse comes back from hv_vio_create (the init entries and the filter) or from the first hv_vio_frame.
 * hv_vio_create allocates everything the frame needs through the library's owning buffer type (one block for the engine's
 * arrays; the filter's lazily grown visit buffers are grown here by one visit loop over empty candidate lists), runs every *_init*
 * entry and the three seeds, and synchronises once. An hv_vio must be destroyed before its context.
 * hv_vio_frame is one frame of every set: left_dev / right_dev are 8-bit gray images, set s at s * image_stride_bytes, rows
 * row_stride_bytes apart (base and strides multiples of 4 bytes: the images are copied into the engine's pyramid slots by
 * hv_ingest_build_batch_dev and may be overwritten as soon as the call has run on the stream); t_dev [n_samples][n_sets], gyro_dev /
 * acc_dev [n_samples][n_sets][3] as hv_session_imu_dev and hv_ekf_predict_n_dev take them, 1 <= n_samples <= imu_samples_max. A
 * set with fewer samples repeats its last time stamp: dt = 0 is skipped (ekf.cpp:367). Intensity matching and a rectifying ingest
 * work on the caller's buffers in front of the call. The call allocates nothing, copies nothing to the host and synchronises
 * nothing; no per-frame state is kept on the host, so it can be captured (hipStreamBeginCapture, torch.cuda.graph) and replayed.
 * The first frame of a set after create or after a reset has no previous image: its table is empty and "has a previous frame" is
 * 0 in device memory, so the temporal and stereo LK, the gate and the RANSAC filters see zero points and the frame is the
 * detection-only frame of a fresh tracker.
 * hv_vio_replay_period: the number of consecutive frames that form the unit a graph may hold. It is 1: a frame issues
 * hv_ekf_undo_augment_dev and hv_ekf_symmetrize_augment_dev exactly once each, unconditionally (their masks are device data),
 * and each swaps the two covariance buffers (hv_ekf_device_pointers above), so every frame starts on the buffer it found; the slot
 * roles and the frame number are device arrays that vio_frame_end_kernel rotates and advances.
 * hv_vio_view hands out the owned objects and the device pointers of the frame's stage outputs; nothing is copied, the pointers
 * stay valid until hv_vio_destroy. */
enum { HV_DETECTOR_GPU_GFTT = 0, HV_DETECTOR_FAST = 1, HV_DETECTOR_GFTT = 2 };   /* tracker.featureDetector */
typedef struct hv_vio_params {
    hv_ekf_params ekf;                   /* (the LK parameters are hv_params of the context the engine is built on) */
    hv_gftt_params gftt;
    hv_subpix_params subpix;
    hv_stereo_gate_params gate;
    hv_ransac3_params ransac3;
    hv_track_table_params tracks;
    hv_trail_index_params trail;
    hv_flow_predict_params flow;
    hv_vu_params vu;
    hv_ekf_control_params control;
    hv_session_params session;
    hv_output_params output;
    hv_camera_model camera0, camera1;
    double ransac2Threshold;
    double trackChiTestOutlierR, visualR;
    int ransacRngSeed, odometryRngSeed;
    int imu_samples_max;
    int featureDetector, useRansac3, predictOpticalFlow, batchVisualUpdate;
    /* read by hv_vio_create_session alone (hv_vio_create ignores them) */
    hv_ransac5_params ransac5;
    hv_upright2p_params upright2p;
    hv_fast_params fast;
    hv_gftt_legacy_params gftt_legacy;
    int useStereoUpright2p, useHybridRansac;
} hv_vio_params;
void hv_vio_default_params(hv_vio_params *p);
typedef struct hv_vio hv_vio;
typedef struct hv_vio_view {              /* device memory unless noted; V = trail.maxVisualUpdates */
    hv_ekf *ekf;                          /* host handle of the filter batch (batch = n_sets) */
    hv_track_table table;
    hv_trail_index trail;
    hv_session session;
    hv_ekf_control control;
    hv_rng rng_pipeline, rng_ransac3, rng_odometry;
    hv_output record;
    const int32_t *frame_num;             /* [n_sets] the number of the NEXT frame of every set */
    const uint8_t *has_previous;          /* [n_sets] as the last frame's begin kernel read it */
    const uint8_t *full_update;           /* [n_sets] */
    const int32_t *keyframe;              /* [n_sets] keyframe_dev of hv_tracks_update_batch_dev */
    const int32_t *keyframe_out;          /* [n_sets] keyframe_out_dev of hv_ekf_frame_control_dev */
    const uint8_t *good_frame;            /* [n_sets] hv_trail_finish_batch_dev */
    const int32_t *reset_kind;            /* [n_sets] hv_session_status_dev */
    const int32_t *tracking_status;       /* [n_sets] status_dev of hv_session_status_dev */
    const int32_t *n_candidates;          /* [n_sets] hv_trail_select_batch_dev */
    const int32_t *cand_id;               /* [V][n_sets] */
    const int32_t *status;                /* [V][n_sets][2] hv_ekf_visual_frame_ragged_dev */
    const int32_t *gate_status;           /* [V][n_sets] */
    const int32_t *slot_prev_left, *slot_cur_left, *slot_right;   /* [n_sets] the slot roles of the NEXT frame; slot_right NULL: mono */
    const int32_t *ransac_result;         /* [n_sets][2] result_dev of the session's filter: {RansacResult type, inlierCount} */
    const double *ransac_score;           /* [n_sets] its score_dev, the stationarity score hv_tracks_update_batch_dev read */
    const int32_t *r5_summary;            /* [n_sets][4] r5_summary_dev of hv_hybrid_ransac_lk_batch_dev; NULL unless hybrid */
} hv_vio_view;
int hv_vio_create(hv_ctx *ctx, const hv_vio_params *p, int n_sets, hv_vio **out);
/* Every session the reference's useStereo, useRansac3, useStereoUpright2p, useHybridRansac and featureDetector select, as the same
 * object with the same call per frame. With default parameters it builds exactly the engine of hv_vio_create: the same buffers,
 * the same launches, the same bits.
 * Mono (trail.useStereo == output.useStereo == 0; tracker.useStereo is false by default, codegen/parameter_definitions.c:349): the
 * mono path of TrackerImplementation::track and detectFeatures (src/tracker/tracker.cpp:378-559, 241-312). hv_vio_frame takes
 * right_dev == NULL (a right image on a mono engine is HV_ERR_INVALID, as is none on a stereo engine); a set holds two pyramid
 * slots, previous and current left; no stereo LK runs, hv_track_gate_batch_dev, hv_tracks_update_batch_dev,
 * hv_detection_filter_batch_dev and hv_tracks_append_batch_dev run in their mono forms (every new corner starts TRACKED,
 * tracker.cpp:291), the visual update runs with vu.useStereo 0. The stereo-only arrays do not exist: table.second_xy and slot_right
 * of the view are NULL.
 * The filter behind RANSAC2 (which always runs) is chosen once, on the host, as RansacPipeline::compute chooses it
 * (src/tracker/ransac_pipeline.cpp:119-150):
 *   useRansac3 and stereo                  hv_ransac3_lk_batch_dev, as in hv_vio_create (:121-123);
 *   else useStereoUpright2p and stereo     hv_upright2p_lk_batch_dev (:124-127) behind the frame's predicts, fed from the second
 *                                          tracker generator (rng_ransac3 of the view, seeded with ransacRngSeed as
 *                                          src/tracker/stereo_upright_2p.cpp:101 seeds its own): 2 * MaxIterations draws, 2 *
 *                                          iterations-run kept consumed;
 *   else useHybridRansac                   hv_hybrid_ransac_lk_batch_dev (:128-133) with camera0 twice (tracker.cpp:482-487), in a
 *                                          mono session and in a stereo one alike; it draws nothing;
 *   else                                   no filter (:134-136): the statuses stay as the gate left them, ransac_result is {0, 0}
 *                                          and the score is RANSAC2 inliers / TRACKED count without a guard, so no TRACKED feature
 *                                          gives 0 / 0 = NaN, which the table's stationarity rule reads as "not stationary"
 *                                          (score * ... > threshold is false). This is the engine's one piece of arithmetic.
 * A mono session with useStereoUpright2p falls through to the hybrid filter (:124 asks for two cameras). The second tracker
 * generator of a session whose filter draws nothing is seeded at creation and never touched again.
 * featureDetector selects hv_gftt_detect_batch_dev, hv_fast_detect_batch_dev (params `fast`) or hv_gftt_legacy_detect_batch_dev
 * (params `gftt_legacy`), each with the table's mask, radius and cap; hv_corner_subpix_batch_dev follows every one of them
 * (src/tracker/image.cpp:69-85). The key point capacity of the last two is their own bound, so no image is refused for its count.
 * The checks, in hv_vio_create's order: every HV_ERR_INVALID of hv_vio_create (gftt.maxTracks included, whatever the detector); the
 * selected detector's maxTracks differing from tracks.maxTracks or an unknown featureDetector, HV_ERR_INVALID; then
 * HV_ERR_UNSUPPORTED for gate.independentStereoOpticalFlow, predictOpticalFlow 0, batchVisualUpdate, trail.fullPointCloud,
 * ekf.hybridMapSize > 0, n_sets > 65535 and a draw count of the selected filter below 1 or above HV_RNG_MAX_DRAWS; then the context
 * checks, where a mono engine needs 2 * n_sets free pyramid slots and a stereo engine 3 * n_sets. hv_vio_replay_period is 1 for
 * every session. */
int hv_vio_create_session(hv_ctx *ctx, const hv_vio_params *p, int n_sets, hv_vio **out);
void hv_vio_destroy(hv_vio *vio);
int hv_vio_frame(hv_vio *vio, const uint8_t *left_dev, const uint8_t *right_dev, long long image_stride_bytes,
                 int row_stride_bytes, int n_samples, const double *t_dev, const double *gyro_dev, const double *acc_dev);
int hv_vio_view_get(hv_vio *vio, hv_vio_view *out);
int hv_vio_replay_period(const hv_vio *vio);
int hv_vio_sets(const hv_vio *vio);

/* ---- per-kernel timing (hipEvents on the context stream) ---------------------------------- */
enum { HV_K_PYR_L0 = 0, HV_K_PYR_LN = 1, HV_K_KLT = 2, HV_K_EKF_PREDICT = 3, HV_K_EKF_UPDATE = 4,
       HV_K_EKF_AUGMENT = 5, HV_K_GFTT = 6, HV_K_INGEST = 7 /* also the image kernels of hv_stereo_disparity*, hv_filter_speckles_batch_dev */, HV_K_VU_PREPARE = 8, HV_K_ROT_RANSAC = 9, HV_K_EKF_GATE = 10,
       HV_K_VU_TRI = 11 /* r06: the triangulation front of the split form (vu_tri_kernel); HV_K_VU_PREPARE then times the record-fed gates; also the tail kernel of hv_full_point_cloud_dev */,
       HV_K_SUBPIX = 12 /* added within ABI 4: hv_corner_subpix* */,
       HV_K_RANSAC5 = 13 /* added within ABI 4: hv_ransac5*, hv_hybrid_ransac_lk_batch_dev */,
       HV_K_STEREO_GATE = 14 /* added within ABI 4: hv_flow_status_batch_dev, hv_track_gate*, hv_detection_filter*, hv_stereo_track_depth_batch_dev, hv_stereo_point_cloud_batch_dev */,
       HV_K_DETECT_TAIL = 15 /* added within ABI 4: hv_apply_min_distance_batch_dev, hv_gftt_corners_batch_dev, hv_gftt_detect_batch_dev */,
       HV_K_TRACK_TABLE = 16 /* added within ABI 4: hv_tracks_*_batch_dev */,
       HV_K_RANSAC3 = 17 /* added within ABI 4: hv_ransac3*, hv_upright2p* */,
       HV_K_EKF_CONTROL = 18 /* added within ABI 4: hv_ekf_block_update_dev, hv_ekf_pseudo_velocity_dev, hv_ekf_imu_control_dev, hv_ekf_frame_control_dev, hv_session_*_dev, hv_output_dev, the two kernels of hv_vio_frame */,
       HV_K_TRAIL_INDEX = 19 /* added within ABI 4: hv_trail_*_batch_dev, hv_flow_predict_batch_dev, the index kernel of hv_full_point_cloud_dev, hv_rng_*_batch_dev */,
       HV_K_COUNT = 20 };
int hv_profile_enable(hv_ctx *ctx, int on);
int hv_profile_reset(hv_ctx *ctx);
/* Synchronizes, then returns accumulated device milliseconds and launch count of a kernel class. */
int hv_profile_read(hv_ctx *ctx, int kernel_id, double *total_ms, long long *launches);

#ifdef __cplusplus
}
#endif
#endif /* HYBVIO_HIP_H_ */
