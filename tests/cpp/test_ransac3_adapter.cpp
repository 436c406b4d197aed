// C++ test of the RansacPipeline adapter on the stereo RANSAC3 branch: the buildHip overload with secondToFirstCamera
// (src/tracker/ransac_pipeline.cpp:95-151, 218-272), driven like TrackerImplementation drives the reference pipeline, frame
// after frame with one pipeline (its two generators run on). Writes, per frame, the result type, inlier count, the size of
// lastResult().inliers, the returned score and the rewritten statuses for tests/test_ransac3_adapter.py to compare with the
// Python path (hv_rot_ransac + hv_ransac3_lk_batch_dev, or hv_hybrid_ransac_lk_batch_dev for a mono call).
//
// usage: test_ransac3_adapter <dir>      (dir/in.txt, writes dir/out.txt)
//        test_ransac3_adapter --refuse   (the overload accepts useRansac3 and must refuse useStereoUpright2p)
#include <array>
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../hybvio_amd/host/hybvio_host.hpp"

using namespace hybvio;

static int refuse()
{
    hv_params params; hv_default_params(&params);
    Session session(params);
    const std::array<double, 16> T{1, 0, 0, 0.11, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int refused = 0;
    tracker::RansacPipelineParameters p;                               // the reference's defaults: useRansac3 true
    auto ok = tracker::RansacPipeline::buildHip(session, 752, 480, p, T);
    p.useStereoUpright2p = true;
    try { tracker::RansacPipeline::buildHip(session, 752, 480, p, T); } catch (const std::invalid_argument &e) { std::printf("%s\n", e.what()); refused++; }
    return refused == 1 && ok ? 0 : 1;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::printf("usage: %s <dir> | --refuse\n", argv[0]); return 2; }
    if (std::string(argv[1]) == "--refuse") return refuse();
    const std::string dir = argv[1];
    std::ifstream f(dir + "/in.txt");
    int w = 0, h = 0, frames = 0;
    hv_camera_model cam{};
    std::array<double, 16> T{};
    f >> w >> h >> cam.kind >> cam.fx >> cam.fy >> cam.ppx >> cam.ppy >> cam.n_coeffs;
    for (int k = 0; k < 4; ++k) f >> cam.coeffs[k];
    f >> cam.max_valid_fov_deg;
    for (double &v : T) f >> v;
    f >> frames;
    if (!f || hv_camera_model_init(&cam) != HV_OK) { std::printf("bad in.txt\n"); return 2; }

    hv_params params; hv_default_params(&params);
    params.width = w; params.height = h;
    Session session(params);
    tracker::RansacPipelineParameters p;                               // a default stereo session
    auto pipeline = tracker::RansacPipeline::buildHip(session, w, h, p, T);
    std::FILE *out = std::fopen((dir + "/out.txt").c_str(), "w");
    for (int fr = 0; fr < frames; ++fr) {
        int n = 0, cams = 0;
        f >> cams >> n;
        std::vector<tracker::Feature::Point> prev((size_t)n), prevRight((size_t)n), cur((size_t)n);
        std::vector<tracker::Feature::Status> status((size_t)n);
        for (int i = 0; i < n; ++i) {
            int st;
            f >> prev[i].x >> prev[i].y >> prevRight[i].x >> prevRight[i].y >> cur[i].x >> cur[i].y >> st;
            status[i] = static_cast<tracker::Feature::Status>(st);
        }
        if (!f) { std::printf("bad frame %d\n", fr); return 2; }
        // corners[camera][frame]: the second camera's current corners are not read by compute (ransac_pipeline.cpp:236-247)
        double score;
        if (cams == 2) score = pipeline->compute({{&cam, &cam}, {&cam, &cam}}, {{&prev, &cur}, {&prevRight, &prevRight}}, nullptr, status);
        else score = pipeline->compute({{&cam, &cam}}, {{&prev, &cur}}, nullptr, status);
        const auto &r = pipeline->lastResult();
        std::fprintf(out, "%d %zu %zu %.17g\n", static_cast<int>(r.type), r.inlierCount, r.inliers.size(), score);
        for (int i = 0; i < n; ++i) std::fprintf(out, "%d ", static_cast<int>(status[i]));
        std::fprintf(out, "\n");
    }
    std::fclose(out);
    std::printf("ransac3 adapter: %d frames\n", frames);
    return 0;
}
