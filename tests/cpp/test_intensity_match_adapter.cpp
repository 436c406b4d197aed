// C++ test of the intensity-matching adapter: hybvio::tracker::util::matchIntensities(session, l, r, weight), the sibling of the
// reference's free function (src/tracker/util.cpp:173-179) as main.cpp:767,776 calls it. Matches r against l twice -- with the
// default weight and with the one given -- and writes both results, padding included, for tests/test_gpu_intensity_match.py to
// compare with the restatement.
//
// usage: test_intensity_match_adapter <dir>   (dir/dims.txt = "w h r_stride weight", dir/l.raw = w*h u8, dir/r.raw = r_stride*h u8;
//                                              writes r_default.raw and r_weighted.raw, r_stride*h u8 each)
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../hybvio_amd/host/hybvio_host.hpp"

using namespace hybvio;

static bool readFile(const std::string &path, std::vector<std::uint8_t> &out)
{
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char *>(out.data()), (std::streamsize)out.size());
    return (bool)f;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::printf("usage: %s <dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    int w = 0, h = 0, stride = 0;
    double weight = 0;
    { std::ifstream f(dir + "/dims.txt"); f >> w >> h >> stride >> weight; if (!f) { std::printf("bad dims.txt\n"); return 2; } }
    std::vector<std::uint8_t> l((size_t)w * h), r((size_t)stride * h);
    if (!readFile(dir + "/l.raw", l) || !readFile(dir + "/r.raw", r)) { std::printf("bad image file\n"); return 2; }

    hv_params params; hv_default_params(&params);       // the context's own image size does not matter to this call
    Session session(params);
    const std::vector<std::uint8_t> lBefore = l;
    auto run = [&](const char *name, bool withWeight) {
        std::vector<std::uint8_t> out = r;
        const tracker::GrayImage left{l.data(), w, h, w};
        tracker::GrayImage right{out.data(), w, h, stride};
        if (withWeight) tracker::util::matchIntensities(session, left, right, weight);
        else tracker::util::matchIntensities(session, left, right);
        std::ofstream f(dir + "/" + name, std::ios::binary);
        f.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)out.size());
        return (bool)f;
    };
    if (!run("r_default.raw", false) || !run("r_weighted.raw", true)) { std::printf("cannot write\n"); return 2; }
    std::printf("intensity adapter: %d x %d matched twice\n", w, h);
    return l == lBefore ? 0 : 1;
}
