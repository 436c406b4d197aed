// C++ test of the RansacPipeline adapter on the stereo upright 2-point branch: buildHipUpright2p
// (src/tracker/ransac_pipeline.cpp:121-128, src/tracker/stereo_upright_2p.cpp:110-183), driven like TrackerImplementation drives
// the reference pipeline, frame after frame with one pipeline (its generators run on). Writes, per frame, the result type, inlier
// count, the size of lastResult().inliers, the returned score and the rewritten statuses for tests/test_upright2p_adapter.py to
// compare with the Python path (hv_rot_ransac + hv_upright2p, hv_ransac3 when useRansac3 takes precedence, or
// hv_hybrid_ransac_lk_batch_dev for a mono call and for a stereo call without poses).
//
// usage: test_upright2p_adapter <dir>      (dir/in.txt, writes dir/out.txt)
//        test_upright2p_adapter --refuse   (the two buildHip overloads still refuse useStereoUpright2p; buildHipUpright2p accepts it)
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
    hv_upright2p_params up; hv_upright2p_default_params(&up);
    int refused = 0;
    tracker::RansacPipelineParameters p;
    p.useRansac3 = false; p.useStereoUpright2p = true;
    try { tracker::RansacPipeline::buildHip(session, 752, 480, p); } catch (const std::invalid_argument &e) { std::printf("%s\n", e.what()); refused++; }
    try { tracker::RansacPipeline::buildHip(session, 752, 480, p, T); } catch (const std::invalid_argument &e) { std::printf("%s\n", e.what()); refused++; }
    auto ok = tracker::RansacPipeline::buildHipUpright2p(session, 752, 480, p, T, up);
    p.useRansac3 = true;
    auto both = tracker::RansacPipeline::buildHipUpright2p(session, 752, 480, p, T, up);
    return refused == 2 && ok && both ? 0 : 1;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::printf("usage: %s <dir> | --refuse\n", argv[0]); return 2; }
    if (std::string(argv[1]) == "--refuse") return refuse();
    const std::string dir = argv[1];
    std::ifstream f(dir + "/in.txt");
    int w = 0, h = 0, frames = 0, useRansac3 = 0;
    hv_camera_model cam{};
    std::array<double, 16> T{};
    f >> w >> h >> cam.kind >> cam.fx >> cam.fy >> cam.ppx >> cam.ppy >> cam.n_coeffs;
    for (int k = 0; k < 4; ++k) f >> cam.coeffs[k];
    f >> cam.max_valid_fov_deg;
    for (double &v : T) f >> v;
    f >> useRansac3 >> frames;
    if (!f || hv_camera_model_init(&cam) != HV_OK) { std::printf("bad in.txt\n"); return 2; }

    hv_params params; hv_default_params(&params);
    params.width = w; params.height = h;
    Session session(params);
    tracker::RansacPipelineParameters p;
    p.useRansac3 = useRansac3 != 0; p.useStereoUpright2p = true;
    hv_upright2p_params up; hv_upright2p_default_params(&up);
    auto pipeline = tracker::RansacPipeline::buildHipUpright2p(session, w, h, p, T, up);
    std::FILE *out = std::fopen((dir + "/out.txt").c_str(), "w");
    for (int fr = 0; fr < frames; ++fr) {
        int n = 0, cams = 0, havePoses = 0;
        std::array<double, 32> poses{};
        f >> cams >> havePoses >> n;
        for (double &v : poses) f >> v;
        std::vector<tracker::Feature::Point> prev((size_t)n), prevRight((size_t)n), cur((size_t)n);
        std::vector<tracker::Feature::Status> status((size_t)n);
        for (int i = 0; i < n; ++i) {
            int st;
            f >> prev[i].x >> prev[i].y >> prevRight[i].x >> prevRight[i].y >> cur[i].x >> cur[i].y >> st;
            status[i] = static_cast<tracker::Feature::Status>(st);
        }
        if (!f) { std::printf("bad frame %d\n", fr); return 2; }
        const void *pp = havePoses ? poses.data() : nullptr;
        double score;
        if (cams == 2) score = pipeline->compute({{&cam, &cam}, {&cam, &cam}}, {{&prev, &cur}, {&prevRight, &prevRight}}, pp, status);
        else score = pipeline->compute({{&cam, &cam}}, {{&prev, &cur}}, pp, status);
        const auto &r = pipeline->lastResult();
        std::fprintf(out, "%d %zu %zu %.17g\n", static_cast<int>(r.type), r.inlierCount, r.inliers.size(), score);
        for (int i = 0; i < n; ++i) std::fprintf(out, "%d ", static_cast<int>(status[i]));
        std::fprintf(out, "\n");
    }
    std::fclose(out);
    std::printf("upright2p adapter: %d frames\n", frames);
    return 0;
}
