// C++ test of the legacy GFTT detector adapter: FeatureDetector::buildHipGftt (featureDetector "GFTT", src/tracker/feature_detector.cpp:
// 659-680, feature_detector_legacy.cpp:53-139) on the frame's device pyramid, the binding INTEGRATION.md gives. Writes the detected
// corners for tests/test_gftt_legacy_adapter.py to compare with the numpy restatement.
//
// usage: test_gftt_legacy_adapter <dir>   (dir/dims.txt = "w h mask_radius block_size quality min_distance max_tracks n_prev",
//                                          dir/img.raw = w*h u8, dir/prev.raw = n_prev * 2 binary32; writes detected.txt)
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../hybvio_amd/host/hybvio_host.hpp"

using namespace hybvio;

int main(int argc, char **argv)
{
    if (argc != 2) { std::printf("usage: %s <dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    int w = 0, h = 0, maskRadius = 0, blockSize = 0, maxTracks = 0, nPrev = 0;
    double quality = 0, minDistance = 0;
    { std::ifstream f(dir + "/dims.txt"); f >> w >> h >> maskRadius >> blockSize >> quality >> minDistance >> maxTracks >> nPrev;
      if (!f || nPrev < 0) { std::printf("bad dims.txt\n"); return 2; } }
    std::vector<std::uint8_t> img((size_t)w * h);
    { std::ifstream f(dir + "/img.raw", std::ios::binary); f.read(reinterpret_cast<char *>(img.data()), (std::streamsize)img.size());
      if (!f) { std::printf("bad img.raw\n"); return 2; } }
    std::vector<tracker::Feature::Point> prev((size_t)nPrev);
    if (nPrev > 0) {
        std::ifstream f(dir + "/prev.raw", std::ios::binary);
        f.read(reinterpret_cast<char *>(prev.data()), (std::streamsize)(prev.size() * sizeof(tracker::Feature::Point)));
        if (!f) { std::printf("bad prev.raw\n"); return 2; }
    }

    hv_params params; hv_default_params(&params);
    params.width = w; params.height = h;
    Session session(params);
    auto pyramidFactory = tracker::ImagePyramid::Factory::buildHip(session);
    hv_gftt_legacy_params gp; hv_gftt_legacy_default_params(&gp);
    if (gp.gfttBlockSize != 3 || gp.gfttQualityLevel != 0.01 || gp.gfttMinDistance != 50.0 || gp.maxTracks != 200) {
        std::printf("unexpected defaults\n");
        return 1;
    }
    gp.gfttBlockSize = blockSize; gp.gfttQualityLevel = quality; gp.gfttMinDistance = minDistance; gp.maxTracks = maxTracks;
    auto detector = tracker::FeatureDetector::buildHipGftt(session, gp);
    if (detector->supportsAsync()) { std::printf("the legacy detector is synchronous\n"); return 1; }

    auto pyramid = pyramidFactory->compute(tracker::GrayImage{img.data(), w, h, w});
    std::vector<tracker::Feature::Point> corners;
    detector->detect(*pyramid, corners, prev, maskRadius);
    {
        std::FILE *f = std::fopen((dir + "/detected.txt").c_str(), "w");
        for (const auto &p : corners) std::fprintf(f, "%.9g %.9g\n", p.x, p.y);
        std::fclose(f);
    }
    // a second frame through the same detector: the staging arena is reused, the result is the same
    std::vector<tracker::Feature::Point> again;
    detector->detect(*pyramid, again, prev, maskRadius);
    if (again.size() != corners.size()) { std::printf("the second call gave %zu corners, the first %zu\n", again.size(), corners.size()); return 1; }
    for (size_t i = 0; i < corners.size(); ++i)
        if (again[i].x != corners[i].x || again[i].y != corners[i].y) { std::printf("the second call differs at %zu\n", i); return 1; }
    std::printf("gftt legacy adapter: %zu corners\n", corners.size());
    return 0;
}
