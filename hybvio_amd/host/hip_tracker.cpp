// HIP-backed tracker::ImagePyramid::Factory and tracker::OpticalFlow (see hybvio_host.hpp).
// Counterparts of CpuImagePyramidFactory (src/tracker/image_pyramid.cpp:27-49) and
// OpenCvOpticalFlow (src/tracker/optical_flow.cpp:61-103).
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <stdexcept>

#include "hybvio_host.hpp"

namespace hybvio {

Session::Session(const hv_params &params) : params_(params)
{
    const int rc = hv_create(&params_, &ctx_);
    if (rc != HV_OK) throw std::runtime_error(std::string("hv_create: ") + hv_status_string(rc));
}

Session::~Session() { if (owned_) hv_destroy(ctx_); }

Lanes::Lanes(const hv_params &params, int n)
{
    const int rc = hv_lanes_create(&params, n, &lanes_);
    if (rc != HV_OK) throw std::runtime_error(std::string("hv_lanes_create: ") + hv_status_string(rc));
    for (int i = 0; i < hv_lanes_count(lanes_); ++i) sessions_.emplace_back(new Session(hv_lanes_ctx(lanes_, i), params));
}

Lanes::~Lanes()
{
    sessions_.clear();                     // (the borrowed contexts die with the set)
    hv_lanes_destroy(lanes_);
}

void Session::check(int rc, const char *what) const
{
    if (rc == HV_OK) return;
    std::string msg = std::string(what) + ": " + hv_status_string(rc);
    if (rc == HV_ERR_HIP) msg += std::string(" (") + hv_last_error(ctx_) + ")";
    throw DeviceError(rc, msg);
}

namespace tracker {

ImagePyramid::~ImagePyramid() = default;
ImagePyramid::Factory::~Factory() = default;
OpticalFlow::~OpticalFlow() = default;
FeatureDetector::~FeatureDetector() = default;
SubPixelAdjuster::~SubPixelAdjuster() = default;
Undistorter::~Undistorter() = default;
rot_ransac::RotRansac::~RotRansac() = default;
RansacPipeline::~RansacPipeline() = default;
StereoGate::~StereoGate() = default;
StereoDisparity::~StereoDisparity() = default;

void FeatureDetector::applyMinDistance(std::vector<Feature::Point> &corners, const std::vector<Feature::Point> &prevCorners,
                                       int minDistance) const
{
    static_assert(sizeof(Feature::Point) == 2 * sizeof(float), "Point must be two packed floats");
    int n = (int)corners.size();
    hv_apply_min_distance(reinterpret_cast<float *>(corners.data()), &n,
                          reinterpret_cast<const float *>(prevCorners.data()), (int)prevCorners.size(),
                          minDistance, maxTracks);
    corners.resize((size_t)n);
}

namespace {

// One pooled device slot. util::Allocator (src/util/allocator.hpp:55-67) recycles a pyramid when
// only the pool still references it; here the shared_ptr's last owner returns the slot to the
// device pool, which has the same effect: a pyramid lives exactly as long as an Image refers to it.
struct HipImagePyramid : ImagePyramid {
    Session &session;
    hv_ctx *ctx;
    int slot;
    HipImagePyramid(Session &s, int sl) : session(s), ctx(s.ctx()), slot(sl) {}
    ~HipImagePyramid() override { hv_pyramid_release(ctx, slot); }
    int deviceSlot() const final { return slot; }

    std::vector<GrayType> getGrayLevel(std::size_t i, int &w, int &h) final {
        session.check(hv_pyramid_level_size(ctx, (int)i, &w, &h), "hv_pyramid_level_size");
        std::vector<GrayType> out((size_t)w * h);
        session.check(hv_pyramid_download(ctx, slot, (int)i, out.data(), nullptr), "hv_pyramid_download");
        return out;
    }
    std::vector<GradientType> getGradientLevel(std::size_t i, int &w, int &h) final {
        session.check(hv_pyramid_level_size(ctx, (int)i, &w, &h), "hv_pyramid_level_size");
        std::vector<GradientType> out((size_t)w * h * GRADIENT_CHANNELS);
        session.check(hv_pyramid_download(ctx, slot, (int)i, nullptr, out.data()), "hv_pyramid_download");
        return out;
    }
};

class HipImagePyramidFactory : public ImagePyramid::Factory {
    Session &session;
public:
    explicit HipImagePyramidFactory(Session &s) : session(s) {}
    std::shared_ptr<ImagePyramid> compute(const GrayImage &img) final {
        assert(img.width == session.params().width && img.height == session.params().height);
        int slot = -1;
        session.check(hv_pyramid_acquire(session.ctx(), &slot), "hv_pyramid_acquire");   // the pool grows on demand
        auto pyramid = std::make_shared<HipImagePyramid>(session, slot);
        session.check(hv_pyramid_build(session.ctx(), slot, img.data, img.strideBytes), "hv_pyramid_build");   // H2D + kernels, asynchronous
        // the caller's pixels were handed to an asynchronous copy: fence before they may be reused
        session.check(hv_synchronize(session.ctx()), "hv_synchronize");
        return pyramid;
    }
    std::shared_ptr<ImagePyramid> computeFromFrame(const InputImage &img) final {
        assert(img.width == session.params().width && img.height == session.params().height);
        int slot = -1;
        session.check(hv_pyramid_acquire(session.ctx(), &slot), "hv_pyramid_acquire");   // the pool grows on demand
        auto pyramid = std::make_shared<HipImagePyramid>(session, slot);
        session.check(hv_ingest_build(session.ctx(), slot, img.data, img.strideBytes, img.channels, -1), "hv_ingest_build");
        session.check(hv_synchronize(session.ctx()), "hv_synchronize");
        return pyramid;
    }
};

// Counterpart of UndistorterImplementation (src/tracker/undistorter.cpp:43-135). Like the reference's GPU branch
// (:113-121) the remap is built once, from the first camera seen; later per-frame intrinsics are ignored with a
// warning. The table is the reference's own per-pixel evaluation (undistortCpu, :56-60) done once on the host.
class HipUndistorter : public Undistorter {
    Session &session;
    const int cameraIndex;
    std::shared_ptr<const Camera> originalCamera, undistortedCamera;
public:
    HipUndistorter(Session &s, int idx, std::shared_ptr<const Camera> rectified)
        : session(s), cameraIndex(idx), undistortedCamera(std::move(rectified)) {}
    ~HipUndistorter() override { hv_ingest_set_undistort_map(session.ctx(), cameraIndex, nullptr, nullptr); }

    Result undistort(const InputImage &image, std::shared_ptr<const Camera> camera) final {
        const int w = session.params().width, h = session.params().height;
        assert(image.width == w && image.height == h);
        if (originalCamera) {
            if (originalCamera->getFocalLength() - camera->getFocalLength() > 1e-6)          // undistorter.cpp:114-117
                std::fprintf(stderr, "Per-frame camera parameters ignored in HIP undistortion\n");
        } else {
            originalCamera = camera;
            std::vector<double> pixOrig((size_t)w * h * 2, 0.0);
            std::vector<std::uint8_t> valid((size_t)w * h, 0);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    const double pixRect[2] = {(double)x, (double)y};
                    double ray[3], *out = &pixOrig[2 * ((size_t)y * w + x)];
                    valid[(size_t)y * w + x] = undistortedCamera->pixelToRay(pixRect, ray) && originalCamera->rayToPixel(ray, out);
                }
            session.check(hv_ingest_set_undistort_map(session.ctx(), cameraIndex, pixOrig.data(), valid.data()), "hv_ingest_set_undistort_map");
        }
        int slot = -1;
        session.check(hv_pyramid_acquire(session.ctx(), &slot), "hv_pyramid_acquire");   // the pool grows on demand
        auto pyramid = std::make_shared<HipImagePyramid>(session, slot);
        session.check(hv_ingest_build(session.ctx(), slot, image.data, image.strideBytes, image.channels, cameraIndex), "hv_ingest_build");
        session.check(hv_synchronize(session.ctx()), "hv_synchronize");
        return {undistortedCamera, pyramid};
    }
};

class HipOpticalFlow : public OpticalFlow {
    Session &session;
    std::vector<std::int32_t> workStatus;
public:
    explicit HipOpticalFlow(Session &s) : session(s) {}
    void compute(ImagePyramid &prevImagePyramid, ImagePyramid &imagePyramid,
                 const std::vector<Feature::Point> &prevCorners, std::vector<Feature::Point> &corners,
                 std::vector<Feature::Status> &trackStatus, bool useInitialCorners,
                 int overrideMaxIterations) final {
        // optical_flow.cpp:26-40: outputs are cleared and sized by the callee; empty input returns early
        const size_t n = prevCorners.size();
        trackStatus.clear();
        trackStatus.resize(n, Feature::Status::FAILED_FLOW);
        if (n == 0) { corners.clear(); return; }
        if (!useInitialCorners) corners.assign(n, Feature::Point{0.f, 0.f});
        assert(corners.size() == n);
        workStatus.assign(n, 2);
        static_assert(sizeof(Feature::Point) == 2 * sizeof(float), "Point must be two packed floats (optical_flow.cpp:21-22)");
        session.check(hv_optical_flow_compute(session.ctx(), prevImagePyramid.deviceSlot(), imagePyramid.deviceSlot(),
                                               (int)n, reinterpret_cast<const float *>(prevCorners.data()),
                                               reinterpret_cast<float *>(corners.data()), workStatus.data(),
                                               useInitialCorners ? 1 : 0, overrideMaxIterations), "hv_optical_flow_compute");
        for (size_t i = 0; i < n; ++i) trackStatus[i] = static_cast<Feature::Status>(workStatus[i]);
    }
};

// Counterpart of FeatureDetectorImplementation (src/tracker/feature_detector.cpp:566-652) on its
// CPU-fallback path: corner response + block arg-max on the device, the reference's sort /
// zero-prefix / applyMinDistance tail inside hv_gftt_detect.
class HipFeatureDetector : public FeatureDetector {
    Session &session;
public:
    HipFeatureDetector(Session &s, const hv_gftt_params &p) : FeatureDetector(p), session(s) {}
    void detect(ImagePyramid &imagePyramid, std::vector<Feature::Point> &corners,
                const std::vector<Feature::Point> &prevCorners, int maskRadius) final {
        const int nk = hv_gftt_keypoint_count(session.ctx(), &parameters);
        assert(nk >= 0);
        corners.assign((size_t)(2 * nk), Feature::Point{0.f, 0.f});
        int n = 0;
        session.check(hv_gftt_detect(session.ctx(), &parameters, imagePyramid.deviceSlot(),
                                      reinterpret_cast<const float *>(prevCorners.data()), (int)prevCorners.size(),
                                      maskRadius, reinterpret_cast<float *>(corners.data()), 2 * nk, &n), "hv_gftt_detect");
        corners.resize((size_t)n);
    }
};

// Counterpart of the legacy FAST detector (src/tracker/feature_detector_legacy.cpp:141-174 behind MaskedFeatureDetector, :20-83, and
// the tail of FeatureDetector::detect): segment test, suppression, track mask, stable sort and applyMinDistance inside hv_fast_detect.
class HipFastFeatureDetector : public FeatureDetector {
    Session &session;
    const hv_fast_params fast;
public:
    HipFastFeatureDetector(Session &s, const hv_fast_params &p) : FeatureDetector(p.maxTracks), session(s), fast(p) {}
    void detect(ImagePyramid &imagePyramid, std::vector<Feature::Point> &corners,
                const std::vector<Feature::Point> &prevCorners, int maskRadius) final {
        const int bound = hv_fast_keypoint_bound(session.ctx());
        assert(bound >= 0 && maskRadius >= 1);                             // feature_detector_legacy.cpp:72
        const int cap = std::min(fast.maxTracks, bound);
        corners.assign((size_t)std::max(cap, 0), Feature::Point{0.f, 0.f});
        int n = 0;
        session.check(hv_fast_detect(session.ctx(), &fast, imagePyramid.deviceSlot(),
                                      reinterpret_cast<const float *>(prevCorners.data()), (int)prevCorners.size(),
                                      maskRadius, reinterpret_cast<float *>(corners.data()), cap, &n), "hv_fast_detect");
        corners.resize((size_t)n);
    }
};

// Counterpart of the legacy GFTT detector (src/tracker/feature_detector_legacy.cpp:53-139 behind MaskedFeatureDetector, :20-51):
// track mask, cv::goodFeaturesToTrack's response, threshold, local maxima, order and minimum-distance walk inside hv_gftt_legacy_detect.
class HipGfttLegacyFeatureDetector : public FeatureDetector {
    Session &session;
    const hv_gftt_legacy_params gftt;
public:
    HipGfttLegacyFeatureDetector(Session &s, const hv_gftt_legacy_params &p) : FeatureDetector(p.maxTracks), session(s), gftt(p) {}
    void detect(ImagePyramid &imagePyramid, std::vector<Feature::Point> &corners,
                const std::vector<Feature::Point> &prevCorners, int maskRadius) final {
        const int bound = hv_gftt_legacy_keypoint_bound(session.ctx());
        assert(bound >= 0 && maskRadius >= 1);                             // feature_detector_legacy.cpp:36
        const int cap = std::min(gftt.maxTracks, bound);
        corners.assign((size_t)std::max(cap, 0), Feature::Point{0.f, 0.f});
        int n = 0;
        session.check(hv_gftt_legacy_detect(session.ctx(), &gftt, imagePyramid.deviceSlot(),
                                             reinterpret_cast<const float *>(prevCorners.data()), (int)prevCorners.size(),
                                             maskRadius, reinterpret_cast<float *>(corners.data()), cap, &n), "hv_gftt_legacy_detect");
        corners.resize((size_t)n);
    }
};

// Counterpart of SubPixelAdjusterImplementation (src/tracker/subpixel_adjuster.cpp:9-42): cornerSubPix and the revert of
// points outside the image both run inside hv_corner_subpix, on level 0 of the frame's pyramid.
class HipSubPixelAdjuster : public SubPixelAdjuster {
    Session &session;
    const hv_subpix_params parameters;
public:
    HipSubPixelAdjuster(Session &s, const hv_subpix_params &p) : session(s), parameters(p) {}
    void adjust(ImagePyramid &imagePyramid, std::vector<Feature::Point> &corners) final {
        if (corners.empty()) return;                                       // subpixel_adjuster.cpp:21-23
        static_assert(sizeof(Feature::Point) == 2 * sizeof(float), "Point must be two packed floats");
        session.check(hv_corner_subpix(session.ctx(), &parameters, imagePyramid.deviceSlot(), (int)corners.size(),
                                        reinterpret_cast<float *>(corners.data()), nullptr), "hv_corner_subpix");
    }
};

}  // namespace

namespace {
class HipRotRansac : public rot_ransac::RotRansac {
    Session &session;
    std::vector<int> pairs, status;
public:
    explicit HipRotRansac(Session &s) : session(s), pairs(200) {}
    std::array<float, 9> fit(const std::vector<Feature::Point> &c1, const std::vector<Feature::Point> &c2,
                             const hv_camera_model &camera1, const hv_camera_model &camera2,
                             std::vector<Feature::Status> &bestInliers, std::mt19937 &rng) final {
        assert(c1.size() == c2.size());
        const std::size_t n = c1.size();
        assert(n >= 2 && bestInliers.size() >= n);
        // draw the 100 index pairs from a COPY of the generator, then advance the real one by what the reference loop
        // would have consumed (it stops at the first hypothesis that makes every point an inlier)
        std::mt19937 ahead = rng;
        for (int k = 0; k < 100; ++k) {
            pairs[2 * k] = static_cast<int>(ahead() % n);
            pairs[2 * k + 1] = static_cast<int>(ahead() % n);
        }
        status.assign(n, 3);
        std::array<float, 9> R{};
        int best = 0, visited = 0;
        static_assert(sizeof(Feature::Point) == 2 * sizeof(float), "Point must be two packed floats");
        session.check(hv_rot_ransac(session.ctx(), static_cast<int>(n), reinterpret_cast<const float *>(c1.data()),
                                     reinterpret_cast<const float *>(c2.data()), &camera1, &camera2, pairs.data(), threshold_pow2,
                                     status.data(), R.data(), &best, &visited), "hv_rot_ransac");
        rng.discard(2ull * static_cast<unsigned long long>(visited));
        bestInlierCount = static_cast<std::size_t>(best);
        for (std::size_t i = 0; i < n; ++i) bestInliers.at(i) = static_cast<Feature::Status>(status[i]);
        return R;
    }
};
}  // namespace

std::unique_ptr<rot_ransac::RotRansac> rot_ransac::RotRansac::buildHip(Session &s)
{
    return std::unique_ptr<rot_ransac::RotRansac>(new HipRotRansac(s));
}

namespace {
// Counterpart of RansacPipelineImplementation (src/tracker/ransac_pipeline.cpp:43-151) on its RANSAC2, hybrid, RANSAC3 and upright 2-point paths.
class HipRansacPipeline : public RansacPipeline {
    Session &session;
    const RansacPipelineParameters parameters;
    std::mt19937 rng, rng3, rngUpright;                                      // :66, :78, stereo_upright_2p.cpp:101
    const bool stereo;                                                       // built with secondToFirstCamera
    const bool upright;                                                      // built by buildHipUpright2p
    hv_upright2p_params upright2p{};
    std::array<double, 16> secondToFirstCamera{};
    std::unique_ptr<rot_ransac::RotRansac> rotRansac;
    RansacResult ransacResult, ransac2Result, ransac5Result;
    std::vector<Feature::Point> c1, c2;
    std::vector<int> status5, status3;
    std::vector<std::uint32_t> draws3;

    static void initialize(RansacResult &r, std::size_t n) {                 // RansacResult::initialize (:20-27)
        r.type = RansacResult::Type::SKIPPED;
        r.inlierCount = 0;
        r.inliers.assign(n, Feature::Status::RANSAC_OUTLIER);
        r.R.fill(0.0);
        r.t.fill(0.0);
    }

    static void updateTrackStatus(const RansacResult &r, std::vector<Feature::Status> &trackStatus) {   // :29-40
        if (r.type == RansacResult::Type::SKIPPED) return;
        std::size_t j = 0;
        for (auto &st : trackStatus) {
            if (st != Feature::Status::TRACKED) continue;
            if (r.inliers.at(j) != Feature::Status::TRACKED) st = Feature::Status::RANSAC_OUTLIER;
            j++;
        }
        assert(j == r.inliers.size());
    }

    bool doRansac2(const hv_camera_model &camera1, const hv_camera_model &camera2) {   // :197-216
        const std::size_t n = c1.size();
        initialize(ransac2Result, n);
        if (n < 2) return false;
        const std::array<float, 9> R = rotRansac->fit(c1, c2, camera1, camera2, ransac2Result.inliers, rng);
        for (int k = 0; k < 9; ++k) ransac2Result.R[k] = R[k];
        ransac2Result.inlierCount = rotRansac->bestInlierCount;
        ransac2Result.type = RansacResult::Type::R2;
        return true;
    }

    bool doRansac5(const hv_camera_model &camera1, const hv_camera_model &camera2) {   // :274-397 (non-Theia)
        const std::size_t n = c1.size();
        initialize(ransac5Result, n);
        if (n < 5) return false;
        status5.assign(n, 3);
        double E[9];
        int summary[4];
        static_assert(sizeof(Feature::Point) == 2 * sizeof(float), "Point must be two packed floats");
        session.check(hv_ransac5(session.ctx(), &parameters.ransac5, static_cast<int>(n), reinterpret_cast<const float *>(c1.data()),
                                 reinterpret_cast<const float *>(c2.data()), &camera1, &camera2, status5.data(), E, summary),
                      "hv_ransac5");
        if (summary[3] < 5) return false;                                    // fewer than 5 valid points (:344)
        for (std::size_t i = 0; i < n; ++i) ransac5Result.inliers[i] = static_cast<Feature::Status>(status5[i]);
        ransac5Result.inlierCount = static_cast<std::size_t>(summary[0]);
        ransac5Result.type = RansacResult::Type::R5;
        return true;
    }

    // The body of doRansac3 (:218-272) and of StereoUpright2p::compute (stereo_upright_2p.cpp:110-183): a filter with samples of
    // `sample` features, drawn from gen; call(n, previous-left, previous-right, current-left, draws, status, summary) is the library call.
    template <class Call>
    bool doStereoFilter(std::mt19937 &gen, unsigned sample, int maxIterations, RansacResult::Type type,
                        const std::vector<std::array<const std::vector<Feature::Point> *, 2>> &corners,
                        std::vector<Feature::Status> &trackStatus, Call call) {
        const std::size_t n = corners[0][0]->size();
        assert(corners[1][0]->size() == n && corners[0][1]->size() == n && trackStatus.size() == n);
        initialize(ransacResult, n);
        status3.resize(n);
        for (std::size_t i = 0; i < n; ++i) status3[i] = static_cast<int>(trackStatus[i]);
        // the next sample * maxIterations raw outputs of a COPY of the generator; the real one advances by what the loop consumed
        std::mt19937 ahead = gen;
        draws3.resize(sample * static_cast<std::size_t>(maxIterations));
        for (auto &d : draws3) d = static_cast<std::uint32_t>(ahead());
        int summary[4];
        static_assert(sizeof(Feature::Point) == 2 * sizeof(float), "Point must be two packed floats");
        auto xy = [](const std::vector<Feature::Point> *v) { return reinterpret_cast<const float *>(v->data()); };
        call(static_cast<int>(n), xy(corners[0][0]), xy(corners[1][0]), xy(corners[0][1]), draws3.data(), status3.data(), summary);
        gen.discard(static_cast<unsigned long long>(sample) * static_cast<unsigned long long>(summary[2]));
        for (std::size_t i = 0; i < n; ++i) trackStatus[i] = static_cast<Feature::Status>(status3[i]);
        if (summary[3] < static_cast<int>(sample) || summary[1] < 0) return false;   // :253-255, 261-263; stereo_upright_2p.cpp:161-163, 172-174
        ransacResult.inlierCount = static_cast<std::size_t>(summary[0]);
        ransacResult.type = type;
        return true;
    }

    bool doRansac3(const std::vector<std::array<const hv_camera_model *, 2>> &cameras,
                   const std::vector<std::array<const std::vector<Feature::Point> *, 2>> &corners,
                   std::vector<Feature::Status> &trackStatus) {
        return doStereoFilter(rng3, 3, parameters.ransac3.ransac3MaxIterations, RansacResult::Type::R3, corners, trackStatus,
            [&](int n, const float *pl, const float *pr, const float *cl, const std::uint32_t *draws, int *status, int *summary) {
                session.check(hv_ransac3(session.ctx(), &parameters.ransac3, n, pl, pr, cl, cameras[0][0], cameras[1][0],
                                         secondToFirstCamera.data(), draws, status, nullptr, summary), "hv_ransac3");
            });
    }

    bool doUpright2p(const std::vector<std::array<const hv_camera_model *, 2>> &cameras,
                     const std::vector<std::array<const std::vector<Feature::Point> *, 2>> &corners, const double *poses,
                     std::vector<Feature::Status> &trackStatus) {
        return doStereoFilter(rngUpright, 2, upright2p.ransacStereoUpright2pMaxIterations, RansacResult::Type::UPRIGHT_2P, corners, trackStatus,
            [&](int n, const float *pl, const float *pr, const float *cl, const std::uint32_t *draws, int *status, int *summary) {
                session.check(hv_upright2p(session.ctx(), &upright2p, n, pl, pr, cl, cameras[0][0], cameras[1][0],
                                           secondToFirstCamera.data(), poses, draws, status, nullptr, summary), "hv_upright2p");
            });
    }

    void computeHybridRansac(const hv_camera_model &camera1, const hv_camera_model &camera2, bool ransac2Done) {   // :158-195
        const auto &p = parameters.ransac5;
        const std::size_t n = c1.size();
        const bool useRansac2Inliers = ransac2Result.inlierCount > p.ransac2InliersToSkipRansac5 * n;
        bool ransac5Done = !useRansac2Inliers && doRansac5(camera1, camera2);
        const double f5 = static_cast<double>(ransac5Result.inlierCount) / static_cast<double>(n);
        const double f2 = static_cast<double>(ransac2Result.inlierCount) / static_cast<double>(n);
        if (f5 < p.ransacMinInlierFraction) ransac5Done = false;
        if (f2 < p.ransacMinInlierFraction) ransac2Done = false;
        if (ransac2Done && !ransac5Done) ransacResult = ransac2Result;
        else if (ransac5Done && !ransac2Done) ransacResult = ransac5Result;
        else if (ransac2Done && ransac5Done)
            ransacResult = (useRansac2Inliers || ransac2Result.inlierCount > p.ransac2InliersOverRansac5Needed * ransac5Result.inlierCount)
                               ? ransac2Result : ransac5Result;
        else ransacResult = RansacResult();
    }

public:
    HipRansacPipeline(Session &s, int width, int height, const RansacPipelineParameters &p, const std::array<double, 16> *secondToFirst,
                      const hv_upright2p_params *up = nullptr)
        : session(s), parameters(p), rng(p.ransacRngSeed), rng3(p.ransacRngSeed), rngUpright(p.ransacRngSeed),
          stereo(secondToFirst != nullptr), upright(up != nullptr), rotRansac(rot_ransac::RotRansac::buildHip(s)) {
        if (secondToFirst) secondToFirstCamera = *secondToFirst;
        if (up) upright2p = *up;
        const double su = std::min(height, width) / 720.0;                   // :91-93
        rotRansac->threshold_pow2 = static_cast<float>(std::pow(p.ransac2Threshold * su, 2));
    }

    double compute(const std::vector<std::array<const hv_camera_model *, 2>> &cameras,
                   const std::vector<std::array<const std::vector<Feature::Point> *, 2>> &corners, const void *poses,
                   std::vector<Feature::Status> &trackStatus) final {
        assert(!cameras.empty() && !corners.empty());
        c1.clear();
        c2.clear();
        for (std::size_t i = 0; i < trackStatus.size(); i++) {             // :106-112
            if (trackStatus[i] != Feature::Status::TRACKED) continue;
            c1.push_back((*corners[0][0])[i]);
            c2.push_back((*corners[0][1])[i]);
        }
        const std::size_t n = c1.size();
        const bool ransac2Done = doRansac2(*cameras[0][0], *cameras[0][1]);
        if (stereo && parameters.useRansac3 && cameras.size() >= 2 && corners.size() >= 2) {   // :121-123
            doRansac3(cameras, corners, trackStatus);
        } else if (upright && parameters.useStereoUpright2p && cameras.size() >= 2 && corners.size() >= 2 && poses) {   // :124-127
            doUpright2p(cameras, corners, static_cast<const double *>(poses), trackStatus);
        } else if (parameters.useHybridRansac) {
            computeHybridRansac(*cameras[0][0], *cameras[0][1], ransac2Done);
            if (ransacResult.type != RansacResult::Type::SKIPPED) updateTrackStatus(ransacResult, trackStatus);
        } else {
            return ransac2Result.inlierCount / static_cast<double>(n);       // :133-135
        }
        if (ransacResult.type == RansacResult::Type::SKIPPED)
            for (auto &st : trackStatus) st = Feature::Status::RANSAC_OUTLIER;   // :139-144
        if (n == 0) return 0.0;
        return ransac2Result.inlierCount / static_cast<double>(n);
    }

    const RansacResult &lastResult() const final { return ransacResult; }
};
}  // namespace

std::unique_ptr<RansacPipeline> RansacPipeline::buildHip(Session &s, int width, int height, const RansacPipelineParameters &p)
{
    if (p.useRansac3)
        throw std::invalid_argument("RansacPipeline::buildHip: tracker.useRansac3 needs the stereo transform: call the overload that "
                                    "takes secondToFirstCamera, or set useRansac3 false to use the hybrid RANSAC2 / RANSAC5 path");
    if (p.useStereoUpright2p)
        throw std::invalid_argument("RansacPipeline::buildHip: tracker.useStereoUpright2p needs the stereo transform and the upright parameters: call buildHipUpright2p");
    return std::unique_ptr<RansacPipeline>(new HipRansacPipeline(s, width, height, p, nullptr));
}

std::unique_ptr<RansacPipeline> RansacPipeline::buildHip(Session &s, int width, int height, const RansacPipelineParameters &p,
                                                         const std::array<double, 16> &secondToFirstCamera)
{
    if (p.useStereoUpright2p)
        throw std::invalid_argument("RansacPipeline::buildHip: tracker.useStereoUpright2p needs the upright parameters: call buildHipUpright2p");
    return std::unique_ptr<RansacPipeline>(new HipRansacPipeline(s, width, height, p, &secondToFirstCamera));
}

std::unique_ptr<RansacPipeline> RansacPipeline::buildHipUpright2p(Session &s, int width, int height, const RansacPipelineParameters &p,
                                                                  const std::array<double, 16> &secondToFirstCamera,
                                                                  const hv_upright2p_params &upright2p)
{
    return std::unique_ptr<RansacPipeline>(new HipRansacPipeline(s, width, height, p, &secondToFirstCamera, &upright2p));
}

namespace {
class HipStereoGate : public StereoGate {
    Session &session;
    hv_stereo_gate_params params;
    std::vector<std::int32_t> status, stereoStatus;
    std::vector<std::uint8_t> blacklist;

    static const float *xy(const std::vector<Feature::Point> &v) { return reinterpret_cast<const float *>(v.data()); }

public:
    HipStereoGate(Session &s, const StereoGateParameters &p, const std::array<double, 16> &cam0ToCam1) : session(s) {
        hv_stereo_gate_default_params(&params);
        params.maxStereoEpipolarDistance = p.maxStereoEpipolarDistance;
        params.partOfImageToDetectFeatures = p.partOfImageToDetectFeatures;
        params.fisheyeCamera = p.fisheyeCamera ? 1 : 0;
        params.independentStereoOpticalFlow = p.independentStereoOpticalFlow ? 1 : 0;
        for (int i = 0; i < 16; ++i) params.cam0ToCam1[i] = cam0ToCam1[i];
    }

    void markTrackStatus(const std::vector<Feature::Point> &corners, const std::vector<Feature::Point> *secondCorners,
                         const std::vector<Feature::Status> *trackStatusStereo, const std::vector<Feature> &tracks,
                         const hv_camera_model &camera0, const hv_camera_model &camera1,
                         std::vector<Feature::Status> &trackStatus) final {
        static_assert(sizeof(Feature::Point) == 2 * sizeof(float), "Point must be two packed floats");
        const std::size_t n = corners.size();
        assert(trackStatus.size() == n && tracks.size() == n);
        assert(!secondCorners || (secondCorners->size() == n && trackStatusStereo && trackStatusStereo->size() == n));
        if (n == 0) return;
        status.resize(n);
        blacklist.resize(n);
        for (std::size_t i = 0; i < n; ++i) {
            status[i] = static_cast<std::int32_t>(trackStatus[i]);
            blacklist[i] = tracks[i].status == Feature::Status::BLACKLISTED ? 1 : 0;   // tracker.cpp:473-477
        }
        if (secondCorners) {
            stereoStatus.resize(n);
            for (std::size_t i = 0; i < n; ++i) stereoStatus[i] = static_cast<std::int32_t>((*trackStatusStereo)[i]);
        }
        session.check(hv_track_gate(session.ctx(), &params, static_cast<int>(n), xy(corners), secondCorners ? xy(*secondCorners) : nullptr,
                                    secondCorners ? stereoStatus.data() : nullptr, blacklist.data(), &camera0,
                                    secondCorners ? &camera1 : nullptr, status.data()),
                      "hv_track_gate");
        for (std::size_t i = 0; i < n; ++i) trackStatus[i] = static_cast<Feature::Status>(status[i]);
    }

    void filterDetections(std::vector<Feature::Point> &corners, std::vector<Feature::Point> *secondCorners,
                          const std::vector<Feature::Status> *detectionStatus, const hv_camera_model &camera0,
                          const hv_camera_model &camera1) final {
        const std::size_t n = corners.size();
        assert(!secondCorners || (secondCorners->size() == n && detectionStatus && detectionStatus->size() == n));
        if (n == 0) return;
        if (n > HV_DETECTION_FILTER_MAX_POINTS)
            throw std::invalid_argument("StereoGate::filterDetections: more than HV_DETECTION_FILTER_MAX_POINTS new corners");
        if (secondCorners) {
            stereoStatus.resize(n);
            for (std::size_t i = 0; i < n; ++i) stereoStatus[i] = static_cast<std::int32_t>((*detectionStatus)[i]);
        }
        int kept = 0;
        float *c = reinterpret_cast<float *>(corners.data());
        float *c2 = secondCorners ? reinterpret_cast<float *>(secondCorners->data()) : nullptr;
        session.check(hv_detection_filter(session.ctx(), &params, static_cast<int>(n), c, c2, secondCorners ? stereoStatus.data() : nullptr,
                                          &camera0, secondCorners ? &camera1 : nullptr, nullptr, c, c2, &kept),
                      "hv_detection_filter");
        corners.resize(static_cast<std::size_t>(kept));                        // tracker.cpp:309-310
        if (secondCorners) secondCorners->resize(static_cast<std::size_t>(kept));
    }
};
}  // namespace

std::unique_ptr<StereoGate> StereoGate::buildHip(Session &s, int width, int height, const StereoGateParameters &p,
                                                 const std::array<double, 16> &cam0ToCam1)
{
    if (width != s.params().width || height != s.params().height)
        throw std::invalid_argument("StereoGate::buildHip: width / height differ from the session's image size");
    return std::unique_ptr<StereoGate>(new HipStereoGate(s, p, cam0ToCam1));
}

// Counterpart of OpenCvStereoDisparity (src/tracker/stereo_disparity.cpp:21-138): every method is one synchronous C-ABI call.
class HipStereoDisparity : public StereoDisparity {
    Session &session;
    const int width, height, cloudStride;
    const hv_stereo_bm_params params;
public:
    HipStereoDisparity(Session &s, int w, int h, const hv_stereo_bm_params &p, int stride)
        : session(s), width(w), height(h), cloudStride(stride), params(p) {}
    DisparityImage buildDisparityImage() const final { return DisparityImage((size_t)width * height, (std::int16_t)HV_STEREO_FILTERED); }
    void computeDisparity(ImagePyramid &first, ImagePyramid &second, DisparityImage &out) final {
        out.resize((size_t)width * height);
        session.check(hv_stereo_disparity(session.ctx(), &params, first.deviceSlot(), second.deviceSlot(), out.data(), width),
                      "hv_stereo_disparity");
    }
    float getDepth(const std::array<double, 16> &Q, const DisparityImage &disparity, const Feature::Point &pixCoords) const final {
        assert(disparity.size() == (size_t)width * height);
        float depth = -1;
        session.check(hv_stereo_track_depth(session.ctx(), 1, &pixCoords.x, disparity.data(), width, Q.data(), &depth),
                      "hv_stereo_track_depth");
        return depth;
    }
    void getDepths(const std::array<double, 16> &Q, const DisparityImage &disparity, const std::vector<Feature::Point> &pixCoords,
                   std::vector<float> &depths) const final {
        assert(disparity.size() == (size_t)width * height);
        depths.assign(pixCoords.size(), -1.f);
        session.check(hv_stereo_track_depth(session.ctx(), (int)pixCoords.size(), reinterpret_cast<const float *>(pixCoords.data()),
                                            disparity.data(), width, Q.data(), depths.data()), "hv_stereo_track_depth");
    }
    void computePointCloud(const std::array<double, 16> &Q, const DisparityImage &disparity, PointCloud &out) final {
        assert(disparity.size() == (size_t)width * height);
        const int bound = hv_stereo_cloud_bound(session.ctx(), cloudStride);
        if (bound < 0) session.check(bound, "hv_stereo_cloud_bound");
        out.resize((size_t)std::max(bound, 0));
        int n = 0;
        session.check(hv_stereo_point_cloud(session.ctx(), disparity.data(), width, Q.data(), cloudStride,
                                            reinterpret_cast<float *>(out.data()), bound, &n), "hv_stereo_point_cloud");
        out.resize((size_t)n);
    }
};

std::unique_ptr<StereoDisparity> StereoDisparity::buildHip(Session &s, int width, int height, const hv_stereo_bm_params &p,
                                                           int stereoPointCloudStride)
{
    if (width != s.params().width || height != s.params().height)
        throw std::invalid_argument("StereoDisparity::buildHip: width / height differ from the session's image size");
    if (stereoPointCloudStride < 1) throw std::invalid_argument("StereoDisparity::buildHip: stereoPointCloudStride < 1");
    return std::unique_ptr<StereoDisparity>(new HipStereoDisparity(s, width, height, p, stereoPointCloudStride));
}

std::unique_ptr<Undistorter> Undistorter::buildRectifiedHip(Session &s, int cameraIndex, std::shared_ptr<const Camera> rectified)
{
    assert(cameraIndex >= 0 && cameraIndex < HV_INGEST_CAMERAS);
    return std::unique_ptr<Undistorter>(new HipUndistorter(s, cameraIndex, std::move(rectified)));
}

std::unique_ptr<FeatureDetector> FeatureDetector::buildHip(Session &s, const hv_gftt_params &p)
{
    return std::unique_ptr<FeatureDetector>(new HipFeatureDetector(s, p));
}

std::unique_ptr<FeatureDetector> FeatureDetector::buildHipFast(Session &s, const hv_fast_params &p)
{
    return std::unique_ptr<FeatureDetector>(new HipFastFeatureDetector(s, p));
}

std::unique_ptr<FeatureDetector> FeatureDetector::buildHipGftt(Session &s, const hv_gftt_legacy_params &p)
{
    return std::unique_ptr<FeatureDetector>(new HipGfttLegacyFeatureDetector(s, p));
}

std::unique_ptr<SubPixelAdjuster> SubPixelAdjuster::buildHip(Session &s, const hv_subpix_params &p)
{
    return std::unique_ptr<SubPixelAdjuster>(new HipSubPixelAdjuster(s, p));
}

std::unique_ptr<ImagePyramid::Factory> ImagePyramid::Factory::buildHip(Session &s)
{
    return std::unique_ptr<ImagePyramid::Factory>(new HipImagePyramidFactory(s));
}

std::unique_ptr<OpticalFlow> OpticalFlow::buildHip(Session &s)
{
    return std::unique_ptr<OpticalFlow>(new HipOpticalFlow(s));
}

namespace util {
void matchIntensities(Session &s, const GrayImage &l, GrayImage &r, double weight)
{
    assert(l.data && r.data && l.width == r.width && l.height == r.height);   // util.cpp:174-175, :25
    assert(weight >= 0.0 && weight <= 1.0);                                   // util.cpp:26
    s.check(hv_match_intensities(s.ctx(), l.width, l.height, l.data, l.strideBytes, const_cast<std::uint8_t *>(r.data), r.strideBytes,
                                 weight), "hv_match_intensities");
}
}  // namespace util

}  // namespace tracker
}  // namespace hybvio
