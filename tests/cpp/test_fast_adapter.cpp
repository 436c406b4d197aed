// C++ test of the FAST detector adapter: FeatureDetector::buildHipFast (featureDetector "FAST", src/tracker/feature_detector.cpp:
// 659-680) on the frame's device pyramid, the binding INTEGRATION.md gives. Writes the detected corners for
// tests/test_fast_adapter.py to compare with the numpy restatement, and checks that the base class's applyMinDistance stops at the
// maxTracks of whichever parameter struct the detector was built from.
//
// usage: test_fast_adapter <dir>   (dir/dims.txt = "w h mask_radius threshold max_tracks n_prev", dir/img.raw = w*h u8,
//                                   dir/prev.raw = n_prev * 2 binary32; writes detected.txt)
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
    int w = 0, h = 0, maskRadius = 0, threshold = 0, maxTracks = 0, nPrev = 0;
    { std::ifstream f(dir + "/dims.txt"); f >> w >> h >> maskRadius >> threshold >> maxTracks >> nPrev;
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
    hv_fast_params fp; hv_fast_default_params(&fp);
    if (fp.threshold != 10 || fp.maxTracks != 200) { std::printf("unexpected defaults\n"); return 1; }
    fp.threshold = threshold; fp.maxTracks = maxTracks;
    auto detector = tracker::FeatureDetector::buildHipFast(session, fp);
    if (detector->supportsAsync()) { std::printf("the legacy detector is synchronous\n"); return 1; }

    auto pyramid = pyramidFactory->compute(tracker::GrayImage{img.data(), w, h, w});
    std::vector<tracker::Feature::Point> corners;
    detector->detect(*pyramid, corners, prev, maskRadius);
    {
        std::FILE *f = std::fopen((dir + "/detected.txt").c_str(), "w");
        for (const auto &p : corners) std::fprintf(f, "%.9g %.9g\n", p.x, p.y);
        std::fclose(f);
    }

    // applyMinDistance of the base class: a row of points 10 apart, none within 3 of another, is cut at each detector's maxTracks
    hv_gftt_params gp; hv_gftt_default_params(&gp);
    gp.maxTracks = 7;
    auto gftt = tracker::FeatureDetector::buildHip(session, gp);
    std::vector<tracker::Feature::Point> row, none;
    for (int i = 0; i < 3 * maxTracks + 30; ++i) row.push_back(tracker::Feature::Point{10.f * (float)i, 5.f});
    auto a = row, b = row;
    detector->applyMinDistance(a, none, 3);
    gftt->applyMinDistance(b, none, 3);
    if ((int)a.size() != maxTracks || b.size() != 7) { std::printf("applyMinDistance kept %zu and %zu\n", a.size(), b.size()); return 1; }
    std::printf("fast adapter: %zu corners\n", corners.size());
    return 0;
}
