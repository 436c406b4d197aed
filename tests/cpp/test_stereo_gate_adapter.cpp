// C++ test of the StereoGate adapter: StereoGate::buildHip, markTrackStatus (tracker.cpp:441-478) and filterDetections
// (:266-311), driven as TrackerImplementation would drive them. Writes, per gate frame, the gated statuses and, per detection
// set, the kept pairs for tests/test_stereo_gate_adapter.py to compare with the numpy restatement.
//
// usage: test_stereo_gate_adapter <dir>      (dir/in.txt, writes dir/out.txt)
//        test_stereo_gate_adapter --refuse   (buildHip must refuse an image size other than the session's)
#include <array>
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../hybvio_amd/host/hybvio_host.hpp"

using namespace hybvio;
using tracker::Feature;

static int refuse()
{
    hv_params params; hv_default_params(&params);
    params.width = 752; params.height = 480;
    Session session(params);
    std::array<double, 16> T{};
    for (int i = 0; i < 4; ++i) T[5 * i] = 1;
    try { tracker::StereoGate::buildHip(session, 640, 480, tracker::StereoGateParameters(), T); }
    catch (const std::invalid_argument &e) { std::printf("%s\n", e.what()); return tracker::StereoGate::buildHip(session, 752, 480, {}, T) ? 0 : 1; }
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::printf("usage: %s <dir> | --refuse\n", argv[0]); return 2; }
    if (std::string(argv[1]) == "--refuse") return refuse();
    const std::string dir = argv[1];
    std::ifstream f(dir + "/in.txt");
    int w = 0, h = 0, fisheye = 0, independent = 0;
    hv_camera_model cam{};
    f >> w >> h >> cam.kind >> cam.fx >> cam.fy >> cam.ppx >> cam.ppy >> cam.n_coeffs;
    for (int k = 0; k < 4; ++k) f >> cam.coeffs[k];
    f >> cam.max_valid_fov_deg;
    std::array<double, 16> T{};
    for (double &t : T) f >> t;
    tracker::StereoGateParameters p;
    f >> p.maxStereoEpipolarDistance >> p.partOfImageToDetectFeatures >> fisheye >> independent;
    p.fisheyeCamera = fisheye != 0; p.independentStereoOpticalFlow = independent != 0;
    if (!f || hv_camera_model_init(&cam) != HV_OK) { std::printf("bad in.txt\n"); return 2; }

    hv_params params; hv_default_params(&params);
    params.width = w; params.height = h;
    Session session(params);
    auto gate = tracker::StereoGate::buildHip(session, w, h, p, T);
    std::FILE *out = std::fopen((dir + "/out.txt").c_str(), "w");
    int frames = 0;
    f >> frames;
    for (int fr = 0; fr < frames; ++fr) {
        int n = 0;
        f >> n;
        std::vector<Feature::Point> left((size_t)n), right((size_t)n);
        std::vector<Feature::Status> stereo((size_t)n), status((size_t)n);
        std::vector<Feature> tracks((size_t)n);
        for (int i = 0; i < n; ++i) {
            int ss, ts, bl;
            f >> left[i].x >> left[i].y >> right[i].x >> right[i].y >> ss >> ts >> bl;
            stereo[i] = static_cast<Feature::Status>(ss);
            status[i] = static_cast<Feature::Status>(ts);
            tracks[i].status = bl ? Feature::Status::BLACKLISTED : Feature::Status::TRACKED;
        }
        gate->markTrackStatus(left, &right, &stereo, tracks, cam, cam, status);
        for (int i = 0; i < n; ++i) std::fprintf(out, "%d ", static_cast<int>(status[i]));
        std::fprintf(out, "\n");
    }
    int sets = 0;
    f >> sets;
    for (int k = 0; k < sets; ++k) {
        int n = 0;
        f >> n;
        std::vector<Feature::Point> left((size_t)n), right((size_t)n);
        std::vector<Feature::Status> detectionStatus((size_t)n);
        for (int i = 0; i < n; ++i) {
            int ss;
            f >> left[i].x >> left[i].y >> right[i].x >> right[i].y >> ss;
            detectionStatus[i] = static_cast<Feature::Status>(ss);
        }
        gate->filterDetections(left, &right, &detectionStatus, cam, cam);
        std::fprintf(out, "%zu\n", left.size());
        for (std::size_t i = 0; i < left.size(); ++i) std::fprintf(out, "%.9g %.9g %.9g %.9g ", left[i].x, left[i].y, right[i].x, right[i].y);
        std::fprintf(out, "\n");
    }
    if (!f) { std::printf("bad in.txt body\n"); return 2; }
    std::fclose(out);
    std::printf("stereo gate adapter: %d frames, %d detection sets\n", frames, sets);
    return 0;
}
