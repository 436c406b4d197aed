// C++ test of the dense-stereo adapter: StereoDisparity::buildHip (src/tracker/stereo_disparity.cpp) on two frames' device pyramids,
// the binding INTEGRATION.md gives. Writes the disparity image, the depths of the given points and the point cloud for
// tests/test_stereo_bm_adapter.py to compare with the numpy restatement.
//
// usage: test_stereo_bm_adapter <dir>   (dir/dims.txt = "w h nd cloud_stride n_points", dir/left.raw and dir/right.raw = w*h u8,
//                                        dir/q.raw = 16 binary64 row-major, dir/points.raw = n_points * 2 binary32;
//                                        writes disp.raw (int16), depth.raw and cloud.raw (binary32))
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../hybvio_amd/host/hybvio_host.hpp"

using namespace hybvio;

template <class T> static bool readAll(const std::string &path, T *dst, size_t count)
{
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char *>(dst), (std::streamsize)(count * sizeof(T)));
    return (bool)f;
}
template <class T> static void writeAll(const std::string &path, const T *src, size_t count)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(src), (std::streamsize)(count * sizeof(T)));
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::printf("usage: %s <dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    int w = 0, h = 0, nd = 0, cloudStride = 0, nPoints = 0;
    { std::ifstream f(dir + "/dims.txt"); f >> w >> h >> nd >> cloudStride >> nPoints;
      if (!f || nPoints < 0) { std::printf("bad dims.txt\n"); return 2; } }
    std::vector<std::uint8_t> left((size_t)w * h), right((size_t)w * h);
    std::array<double, 16> Q;
    std::vector<tracker::Feature::Point> points((size_t)nPoints);
    if (!readAll(dir + "/left.raw", left.data(), left.size()) || !readAll(dir + "/right.raw", right.data(), right.size()) ||
        !readAll(dir + "/q.raw", Q.data(), 16) || (nPoints > 0 && !readAll(dir + "/points.raw", points.data(), points.size()))) {
        std::printf("bad input files\n"); return 2;
    }

    hv_params params; hv_default_params(&params);
    params.width = w; params.height = h; params.levels = 1;
    Session session(params);
    auto pyramidFactory = tracker::ImagePyramid::Factory::buildHip(session);
    hv_stereo_bm_params bp; hv_stereo_bm_default_params(&bp, 752);
    if (bp.numDisparities != 96 || bp.blockSize != 21 || bp.speckleWindowSize != 500 || bp.speckleRange != 10) {
        std::printf("unexpected defaults\n"); return 1;
    }
    bp.numDisparities = nd;
    bool refused = false;
    try { tracker::StereoDisparity::buildHip(session, w + 1, h, bp); } catch (const std::invalid_argument &) { refused = true; }
    if (!refused) { std::printf("a wrong size was accepted\n"); return 1; }
    auto stereo = tracker::StereoDisparity::buildHip(session, w, h, bp, cloudStride);

    auto first = pyramidFactory->compute(tracker::GrayImage{left.data(), w, h, w});
    auto second = pyramidFactory->compute(tracker::GrayImage{right.data(), w, h, w});
    auto disparity = stereo->buildDisparityImage();
    stereo->computeDisparity(*first, *second, disparity);
    std::vector<float> depths;
    stereo->getDepths(Q, disparity, points, depths);
    if (nPoints > 0 && stereo->getDepth(Q, disparity, points[0]) != depths[0]) { std::printf("getDepth differs from getDepths\n"); return 1; }
    tracker::StereoDisparity::PointCloud cloud;
    stereo->computePointCloud(Q, disparity, cloud);
    writeAll(dir + "/disp.raw", disparity.data(), disparity.size());
    writeAll(dir + "/depth.raw", depths.data(), depths.size());
    writeAll(dir + "/cloud.raw", reinterpret_cast<const float *>(cloud.data()), 3 * cloud.size());
    std::printf("stereo adapter: %zu cloud points\n", cloud.size());
    return 0;
}
