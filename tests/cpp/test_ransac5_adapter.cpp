// C++ test of the RansacPipeline adapter: RansacPipeline::buildHip on the hybrid path (src/tracker/ransac_pipeline.cpp:95-195),
// driven like TrackerImplementation drives the reference pipeline, frame after frame with one generator. Writes, per frame,
// the result type, inlier count, the returned score and the rewritten statuses for tests/test_ransac5_adapter.py to compare
// with the Python path (hv_rot_ransac + hv_hybrid_ransac_lk_batch_dev).
//
// usage: test_ransac5_adapter <dir>      (dir/in.txt, writes dir/out.txt)
//        test_ransac5_adapter --refuse   (buildHip must refuse useRansac3 and useStereoUpright2p)
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
    int refused = 0;
    tracker::RansacPipelineParameters p;                               // the reference's defaults: useRansac3 true
    try { tracker::RansacPipeline::buildHip(session, 752, 480, p); } catch (const std::invalid_argument &e) { std::printf("%s\n", e.what()); refused++; }
    p.useRansac3 = false; p.useStereoUpright2p = true;
    try { tracker::RansacPipeline::buildHip(session, 752, 480, p); } catch (const std::invalid_argument &e) { std::printf("%s\n", e.what()); refused++; }
    p.useStereoUpright2p = false;
    auto ok = tracker::RansacPipeline::buildHip(session, 752, 480, p);   // the hybrid path builds
    return refused == 2 && ok ? 0 : 1;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::printf("usage: %s <dir> | --refuse\n", argv[0]); return 2; }
    if (std::string(argv[1]) == "--refuse") return refuse();
    const std::string dir = argv[1];
    std::ifstream f(dir + "/in.txt");
    int w = 0, h = 0, frames = 0;
    hv_camera_model cam{};
    f >> w >> h >> cam.kind >> cam.fx >> cam.fy >> cam.ppx >> cam.ppy >> cam.n_coeffs;
    for (int k = 0; k < 4; ++k) f >> cam.coeffs[k];
    f >> cam.max_valid_fov_deg >> frames;
    if (!f || hv_camera_model_init(&cam) != HV_OK) { std::printf("bad in.txt\n"); return 2; }

    hv_params params; hv_default_params(&params);
    params.width = w; params.height = h;
    Session session(params);
    tracker::RansacPipelineParameters p;
    p.useRansac3 = false;                                              // a mono session (ransac_pipeline.cpp:124-129)
    auto pipeline = tracker::RansacPipeline::buildHip(session, w, h, p);
    std::FILE *out = std::fopen((dir + "/out.txt").c_str(), "w");
    for (int fr = 0; fr < frames; ++fr) {
        int n = 0;
        f >> n;
        std::vector<tracker::Feature::Point> prev((size_t)n), cur((size_t)n);
        std::vector<tracker::Feature::Status> status((size_t)n);
        for (int i = 0; i < n; ++i) {
            int st;
            f >> prev[i].x >> prev[i].y >> cur[i].x >> cur[i].y >> st;
            status[i] = static_cast<tracker::Feature::Status>(st);
        }
        if (!f) { std::printf("bad frame %d\n", fr); return 2; }
        const double score = pipeline->compute({{&cam, &cam}}, {{&prev, &cur}}, nullptr, status);
        const auto &r = pipeline->lastResult();
        std::fprintf(out, "%d %zu %.17g\n", static_cast<int>(r.type), r.inlierCount, score);
        for (int i = 0; i < n; ++i) std::fprintf(out, "%d ", static_cast<int>(status[i]));
        std::fprintf(out, "\n");
    }
    std::fclose(out);
    std::printf("ransac5 adapter: %d frames\n", frames);
    return 0;
}
