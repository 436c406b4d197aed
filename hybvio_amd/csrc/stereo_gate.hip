// Stereo track gate: the per-track status rules between the LK calls and RansacPipeline::compute, and the filter of newly
// detected stereo corners.
//
// Reference: src/tracker/optical_flow.cpp:50-58 (LK status -> Feature::Status), src/tracker/tracker.cpp:441-478 (stereo
// FAILED_FLOW merge, markCornersFailedByEpipolarConstraint, markOutOfDetectionCropCornersAsFailed, blacklist) and :266-311
// (detectFeatures: epipolar check, crop marks and the stable compaction of the accepted stereo pairs), with the helpers
// computeEpipolarCurve (:81-106), withinDistanceFromCurve (:128-151), isPointInCrop (:315-320) and markCornersFailedBy-
// EpipolarConstraint (:348-376).
//
// flow_status_kernel and track_gate_kernel: one thread per feature. detection_filter_kernel: one workgroup per set (<= 1024
// points, one thread each); the accepted pairs are compacted in input order with a wave64 ballot, the lane prefix count and
// per-wave offsets in LDS.
// Arithmetic follows the reference operation by operation (the library is built with -ffp-contract=off): the curve in
// binary64 through hv_camera.hpp, its points rounded to binary32, the distance tests in binary32; the crop test in binary64.
// The curve is walked once, front to back: withinDistanceFromCurve's tests have no side effects, so the order in which the
// reference visits the vertices (reversed) and the segments does not change its answer, and no point array is kept.
#include "hv_camera.hpp"
#include "hv_internal.hpp"

#include <algorithm>

namespace hv {
namespace {

// tracker::Feature::Status (src/tracker/track.hpp:9-21)
constexpr int ST_TRACKED = 0, ST_FAILED_FLOW = 2, ST_FLOW_OUT_OF_RANGE = 4, ST_OUT_OF_RANGE = 5, ST_FAILED_EPIPOLAR = 6,
              ST_BLACKLISTED = 8;
constexpr int GATE_THREADS = 256;
constexpr int DF_MAX_PTS = HV_DETECTION_FILTER_MAX_POINTS;
constexpr int CURVE_POINTS = 8;                 // computeEpipolarCurve's CURVE_POINTS

struct GateArgs {
    hv_camera_model cam0, cam1;                 // cameras of the left / right image, by value
    double T[12];                               // cam0ToCam1, the top three rows, row-major
    double crop_x0, crop_x1, crop_y0, crop_y1;  // isPointInCrop: [x_delta, width - x_delta) x [y_delta, height - y_delta)
    float dist2;                                // withinDistanceFromCurve's dist2
    int stereo, epipolar, fisheye, crop;
    int max_points;
    const int *n_points;
    const float *corners, *second;              // [n_sets][max_points][2]; second = NULL: mono
    const int32_t *stereo_status;               // [n_sets][max_points] (stereo only)
    const uint8_t *blacklist;                   // [n_sets][max_points], NULL: none
    int32_t *status;                            // gate: in / out; filter: out (NULL ok)
    uint8_t *mask;                              // gate: status == TRACKED (NULL ok)
    float *out_corners, *out_second;            // filter: compacted pairs
    int *n_out;                                 // filter: accepted pairs per set
};

// computeEpipolarCurve + withinDistanceFromCurve: true when the curve is non-empty and (x1, y1) is not within dist of it
__device__ bool fails_epipolar(const GateArgs &a, float x0, float y0, float x1, float y1)
{
    double ray[3];
    if (!pixel_to_ray(a.cam0, (double)x0, (double)y0, ray)) return false;     // empty curve: the status stays
    bool within = false;
    float px = 0.0f, py = 0.0f;
    float s = 0.5f;
#pragma unroll 1
    for (int j = 0; j < CURVE_POINTS; ++j) {
        const double r0[3] = {(double)s * ray[0], (double)s * ray[1], (double)s * ray[2]};
        double r1[3], pix[2];
        for (int i = 0; i < 3; ++i)                                            // transformVec3ByMat4 (odometry/util.hpp:77-85)
            r1[i] = ((a.T[4 * i] * r0[0] + a.T[4 * i + 1] * r0[1]) + a.T[4 * i + 2] * r0[2]) + a.T[4 * i + 3];
        if (!ray_to_pixel(a.cam1, r1, pix)) return false;                      // any failed projection empties the curve
        const float cx = (float)pix[0], cy = (float)pix[1];
        const float dx = cx - x1, dy = cy - y1;                                // the vertex test (:136-139)
        if (dx * dx + dy * dy < a.dist2) within = true;
        if (j > 0) {                                                           // the segment (previous point, this one) (:140-149)
            const float ex = cx - px, ey = cy - py;
            const float s2 = ex * ex + ey * ey;
            const float qx = x1 - px, qy = y1 - py;
            const float t = (qx * ex + qy * ey) / s2;
            if (t > 0 && t < 1) {
                const float rx = x1 - (px + t * ex), ry = y1 - (py + t * ey);
                if (rx * rx + ry * ry < a.dist2) within = true;
            }
        }
        px = cx; py = cy;
        s *= 2;
    }
    return !within;
}

// markOutOfDetectionCropCornersAsFailed for one corner (tracker.cpp:322-346)
__device__ inline bool out_of_crop(const GateArgs &a, const hv_camera_model &cam, float x, float y)
{
    if (a.fisheye) {
        double ray[3];
        if (!pixel_to_ray(cam, (double)x, (double)y, ray)) return true;
    }
    if (a.crop) {
        const double dx = x, dy = y;
        if (!(dx >= a.crop_x0 && dx < a.crop_x1 && dy >= a.crop_y0 && dy < a.crop_y1)) return true;
    }
    return false;
}

__device__ inline int set_count(const int *n_points, int set, int max_points)
{
    return min(max(n_points[set], 0), max_points);
}

// optical_flow.cpp:52-58
__global__ __launch_bounds__(GATE_THREADS) void flow_status_kernel(int max_points, const int *n_points, const float *xy,
                                                                   const uint8_t *lk, int32_t *status, float w, float h)
{
    const int set = blockIdx.y, i = blockIdx.x * GATE_THREADS + threadIdx.x;
    if (i >= set_count(n_points, set, max_points)) return;
    const size_t k = (size_t)set * max_points + i;
    const float x = xy[2 * k], y = xy[2 * k + 1];
    int s = lk[k] == 0 ? ST_FAILED_FLOW : ST_TRACKED;
    if (x < 0.0f || x >= w || y < 0.0f || y >= h) s = ST_FLOW_OUT_OF_RANGE;
    status[k] = s;
}

// tracker.cpp:441-478, in the reference's order
__global__ __launch_bounds__(GATE_THREADS) void track_gate_kernel(GateArgs a)
{
    const int set = blockIdx.y, i = blockIdx.x * GATE_THREADS + threadIdx.x;
    if (i >= set_count(a.n_points, set, a.max_points)) return;
    const size_t k = (size_t)set * a.max_points + i;
    int st = a.status[k];
    const float x0 = a.corners[2 * k], y0 = a.corners[2 * k + 1];
    float x1 = 0.0f, y1 = 0.0f;
    if (a.stereo) {
        x1 = a.second[2 * k]; y1 = a.second[2 * k + 1];
        if (a.stereo_status[k] == ST_FAILED_FLOW) st = ST_FAILED_FLOW;                      // :441-446, FAILED_FLOW only
        if (a.epipolar && st == ST_TRACKED && fails_epipolar(a, x0, y0, x1, y1)) st = ST_FAILED_EPIPOLAR;   // :448-457
    }
    if (out_of_crop(a, a.cam0, x0, y0)) st = ST_OUT_OF_RANGE;                                // :465-468, overwrites any status
    if (a.stereo && out_of_crop(a, a.cam1, x1, y1)) st = ST_OUT_OF_RANGE;
    if (a.blacklist && a.blacklist[k] != 0) st = ST_BLACKLISTED;                             // :471-478
    a.status[k] = st;
    if (a.mask) a.mask[k] = st == ST_TRACKED ? 1 : 0;
}

// tracker.cpp:266-311 after the stereo LK of the new corners. Every input is read before the barrier and every output written
// after it, so the outputs may be the inputs (in-place compaction).
__global__ __launch_bounds__(DF_MAX_PTS) void detection_filter_kernel(GateArgs a)
{
    __shared__ int s_wave[DF_MAX_PTS / 64];
    const int set = blockIdx.x, i = threadIdx.x, lane = i & 63, wave = i >> 6;
    const int n = set_count(a.n_points, set, a.max_points);
    const size_t k = (size_t)set * a.max_points + i;
    bool keep = false;
    float x0 = 0.0f, y0 = 0.0f, x1 = 0.0f, y1 = 0.0f;
    if (i < n) {
        x0 = a.corners[2 * k]; y0 = a.corners[2 * k + 1];
        int st = ST_TRACKED;
        if (a.stereo) {
            x1 = a.second[2 * k]; y1 = a.second[2 * k + 1];
            st = a.stereo_status[k];
            if (a.epipolar && st == ST_TRACKED && fails_epipolar(a, x0, y0, x1, y1)) st = ST_FAILED_EPIPOLAR;
        }
        if (out_of_crop(a, a.cam0, x0, y0)) st = ST_OUT_OF_RANGE;
        if (a.stereo && out_of_crop(a, a.cam1, x1, y1)) st = ST_OUT_OF_RANGE;
        if (a.status) a.status[k] = st;
        keep = st == ST_TRACKED;
    }
    const unsigned long long b = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wave; ++w) off += s_wave[w];
    if (keep) {
        const size_t o = (size_t)set * a.max_points + off + __popcll(b & ((1ull << lane) - 1ull));
        a.out_corners[2 * o] = x0; a.out_corners[2 * o + 1] = y0;
        if (a.stereo) { a.out_second[2 * o] = x1; a.out_second[2 * o + 1] = y1; }
    }
    if (i == 0) {
        int total = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) total += s_wave[w];
        a.n_out[set] = total;
    }
}

// the host-side checks, made before the context is looked at
int check_sizes(const hv_stereo_gate_params *p, int n_sets, int max_points, int filter)
{
    if (!p || n_sets < 0 || max_points < 0) return HV_ERR_INVALID;
    if (n_sets > 65535 || (filter && max_points > DF_MAX_PTS)) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}

// mono: second_corners and stereo_status both NULL; stereo: both given, and camera1 too
int check_stereo(const float *second, const int32_t *stereo_status, const hv_camera_model *cam0, const hv_camera_model *cam1)
{
    if ((second == nullptr) != (stereo_status == nullptr) || !cam0 || (second && !cam1)) return HV_ERR_INVALID;
    return HV_OK;
}

void fill_common(GateArgs &a, const Ctx *c, const hv_stereo_gate_params *p, int max_points, const float *second,
                 const hv_camera_model *cam0, const hv_camera_model *cam1)
{
    const int w = c->L.w[0], h = c->L.h[0];
    a.cam0 = *cam0;
    a.cam1 = cam1 ? *cam1 : *cam0;
    for (int i = 0; i < 12; ++i) a.T[i] = p->cam0ToCam1[i];
    const float scale = static_cast<float>(std::min(w, h));                  // tracker.cpp:356-357
    const float prod = p->maxStereoEpipolarDistance * scale;
    const float dist = static_cast<float>(static_cast<double>(prod) / 720.0);
    a.dist2 = dist * dist;                                                    // (float) std::pow(dist, 2): exact in double
    const double xd = w * (1 - p->partOfImageToDetectFeatures) / 2;          // :317-318
    const double yd = h * (1 - p->partOfImageToDetectFeatures) / 2;
    a.crop_x0 = xd; a.crop_x1 = w - xd; a.crop_y0 = yd; a.crop_y1 = h - yd;
    a.stereo = second != nullptr;
    a.fisheye = p->fisheyeCamera != 0;
    a.crop = p->partOfImageToDetectFeatures < 1.0;
    a.max_points = max_points;
}

}  // namespace
}  // namespace hv

using hv::Ctx;

extern "C" {

void hv_stereo_gate_default_params(hv_stereo_gate_params *p)
{
    if (!p) return;
    p->maxStereoEpipolarDistance = 10.0f;          // codegen/parameter_definitions.c:217
    p->partOfImageToDetectFeatures = 1.0;          // :353
    p->fisheyeCamera = 0;                          // :246
    p->independentStereoOpticalFlow = 0;           // :210
    for (int i = 0; i < 16; ++i) p->cam0ToCam1[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

int hv_flow_status_batch_dev(hv_ctx *h, int n_sets, int max_points, const int *n_points_dev, const float *xy_dev,
                             const uint8_t *lk_status_dev, int32_t *status_dev)
{
    if (n_sets < 0 || max_points < 0) return HV_ERR_INVALID;
    if (n_sets > 65535) return HV_ERR_UNSUPPORTED;
    if (n_sets > 0 && max_points > 0 && (!n_points_dev || !xy_dev || !lk_status_dev || !status_dev)) return HV_ERR_INVALID;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0 || max_points == 0) return HV_OK;
    const dim3 grid((unsigned)((max_points + hv::GATE_THREADS - 1) / hv::GATE_THREADS), (unsigned)n_sets);
    hv::ScopedKernelTime tm(c, HV_K_STEREO_GATE);
    hipLaunchKernelGGL(hv::flow_status_kernel, grid, dim3(hv::GATE_THREADS), 0, c->stream, max_points, n_points_dev, xy_dev,
                       lk_status_dev, status_dev, (float)c->L.w[0], (float)c->L.h[0]);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_track_gate_batch_dev(hv_ctx *h, const hv_stereo_gate_params *p, int n_sets, int max_points, const int *n_points_dev,
                            const float *corners_dev, const float *second_corners_dev, const int32_t *stereo_status_dev,
                            const uint8_t *blacklist_dev, const hv_camera_model *camera0, const hv_camera_model *camera1,
                            int32_t *track_status_dev, uint8_t *tracked_mask_dev)
{
    if (const int rc = hv::check_sizes(p, n_sets, max_points, 0)) return rc;
    if (const int rc = hv::check_stereo(second_corners_dev, stereo_status_dev, camera0, camera1)) return rc;
    if (n_sets > 0 && max_points > 0 && (!n_points_dev || !corners_dev || !track_status_dev)) return HV_ERR_INVALID;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0 || max_points == 0) return HV_OK;
    hv::GateArgs a{};
    hv::fill_common(a, c, p, max_points, second_corners_dev, camera0, camera1);
    a.epipolar = a.stereo && p->maxStereoEpipolarDistance > 0 && !p->independentStereoOpticalFlow;   // tracker.cpp:449
    a.n_points = n_points_dev; a.corners = corners_dev; a.second = second_corners_dev; a.stereo_status = stereo_status_dev;
    a.blacklist = blacklist_dev; a.status = track_status_dev; a.mask = tracked_mask_dev;
    const dim3 grid((unsigned)((max_points + hv::GATE_THREADS - 1) / hv::GATE_THREADS), (unsigned)n_sets);
    hv::ScopedKernelTime tm(c, HV_K_STEREO_GATE);
    hipLaunchKernelGGL(hv::track_gate_kernel, grid, dim3(hv::GATE_THREADS), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_detection_filter_batch_dev(hv_ctx *h, const hv_stereo_gate_params *p, int n_sets, int max_points, const int *n_points_dev,
                                  const float *corners_dev, const float *second_corners_dev, const int32_t *stereo_status_dev,
                                  const hv_camera_model *camera0, const hv_camera_model *camera1, int32_t *status_dev,
                                  float *out_corners_dev, float *out_second_dev, int *n_out_dev)
{
    if (const int rc = hv::check_sizes(p, n_sets, max_points, 1)) return rc;
    if (const int rc = hv::check_stereo(second_corners_dev, stereo_status_dev, camera0, camera1)) return rc;
    if (n_sets > 0 && max_points > 0 &&
        (!n_points_dev || !corners_dev || !out_corners_dev || !n_out_dev || (second_corners_dev && !out_second_dev)))
        return HV_ERR_INVALID;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    if (max_points == 0) {
        HV_HIP(c, hipMemsetAsync(n_out_dev, 0, sizeof(int) * (size_t)n_sets, c->stream));
        return HV_OK;
    }
    hv::GateArgs a{};
    hv::fill_common(a, c, p, max_points, second_corners_dev, camera0, camera1);
    a.epipolar = a.stereo && p->maxStereoEpipolarDistance > 0;                 // tracker.cpp:275, no independentStereoOpticalFlow term
    a.n_points = n_points_dev; a.corners = corners_dev; a.second = second_corners_dev; a.stereo_status = stereo_status_dev;
    a.status = status_dev; a.out_corners = out_corners_dev; a.out_second = out_second_dev; a.n_out = n_out_dev;
    const int threads = (max_points + 63) / 64 * 64;
    hv::ScopedKernelTime tm(c, HV_K_STEREO_GATE);
    hipLaunchKernelGGL(hv::detection_filter_kernel, dim3((unsigned)n_sets), dim3((unsigned)threads), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_track_gate(hv_ctx *h, const hv_stereo_gate_params *p, int n, const float *corners, const float *second_corners,
                  const int32_t *stereo_status, const uint8_t *blacklist, const hv_camera_model *camera0,
                  const hv_camera_model *camera1, int32_t *track_status)
{
    if (const int rc = hv::check_sizes(p, 1, n, 0)) return rc;
    if (const int rc = hv::check_stereo(second_corners, stereo_status, camera0, camera1)) return rc;
    if (n > 0 && (!corners || !track_status)) return HV_ERR_INVALID;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n == 0) return HV_OK;
    const size_t N = (size_t)n;
    hv::Stage s(c);
    const auto o_n = s.in(&n, 1);
    const auto o_c = s.in(corners, 2 * N), o_s = s.in(second_corners, 2 * N);
    const auto o_ss = s.in(stereo_status, N), o_ts = s.inout(track_status, N);
    const auto o_bl = s.in(blacklist, N);
    int rc = s.upload();
    if (rc != HV_OK) return rc;
    rc = hv_track_gate_batch_dev(h, p, 1, n, s.at(o_n), s.at(o_c), s.at_or_null(o_s), s.at_or_null(o_ss), s.at_or_null(o_bl), camera0, camera1,
                                 s.at(o_ts), nullptr);
    return rc != HV_OK ? rc : s.download();
}

int hv_detection_filter(hv_ctx *h, const hv_stereo_gate_params *p, int n, const float *corners, const float *second_corners,
                        const int32_t *stereo_status, const hv_camera_model *camera0, const hv_camera_model *camera1,
                        int32_t *status, float *out_corners, float *out_second, int *n_out)
{
    if (const int rc = hv::check_sizes(p, 1, n, 1)) return rc;
    if (const int rc = hv::check_stereo(second_corners, stereo_status, camera0, camera1)) return rc;
    if (!n_out || (n > 0 && (!corners || !out_corners || (second_corners && !out_second)))) return HV_ERR_INVALID;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n == 0) { *n_out = 0; return HV_OK; }
    const bool stereo = second_corners != nullptr;
    const size_t N = (size_t)n;
    hv::Stage s(c);
    const auto o_n = s.in(&n, 1), o_no = s.take<int>(1);
    const auto o_c = s.in(corners, 2 * N), o_s = s.in(second_corners, 2 * N);
    const auto o_oc = s.take<float>(2 * N), o_os = s.take<float>(2 * N);      // (downloaded below, once the count is known)
    const auto o_ss = s.in(stereo_status, N), o_st = s.out(status, N);
    int rc = s.upload();
    if (rc != HV_OK) return rc;
    rc = hv_detection_filter_batch_dev(h, p, 1, n, s.at(o_n), s.at(o_c), s.at_or_null(o_s), s.at_or_null(o_ss), camera0, camera1, s.at(o_st),
                                       s.at(o_oc), stereo ? s.at(o_os) : nullptr, s.at(o_no));
    if (rc != HV_OK) return rc;
    int cnt = 0;
    rc = s.fetch(&cnt, o_no, 1);
    if (rc == HV_OK) rc = s.sync();
    if (rc != HV_OK) return rc;
    if (cnt < 0 || cnt > n) return HV_ERR_HIP;
    if (cnt > 0) {
        rc = s.fetch(out_corners, o_oc, 2 * (size_t)cnt);
        if (rc == HV_OK && stereo) rc = s.fetch(out_second, o_os, 2 * (size_t)cnt);
        if (rc != HV_OK) return rc;
    }
    rc = s.download();
    if (rc != HV_OK) return rc;
    *n_out = cnt;
    return HV_OK;
}

}  // extern "C"
