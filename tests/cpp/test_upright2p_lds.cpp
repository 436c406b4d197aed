// Stand-alone test of the upright 2-point kernel's dynamic-LDS layout (hybvio_amd/csrc/ransac_lds.hpp: upright2p_lds), plain g++
// -std=c++17, no HIP: the sections ascend and do not overlap, the double sections are 8-byte aligned (the int sections 4-byte), the
// total is the closed form worked out by hand, and the largest shape fits a compute unit beside the kernel's static LDS.
// Run by tests/test_upright2p_lds.py.
#include <cstdio>
#include <initializer_list>
#include "../../hybvio_amd/csrc/lds_layout.hpp"
#include "../../hybvio_amd/csrc/ransac_lds.hpp"

using namespace hv;

static int failures = 0;
#define CHECK(cond, ...)                                                                      \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            if (++failures <= 20) { std::printf("FAILED %s:%d  %s  [", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("]\n"); } \
        }                                                                                     \
    } while (0)

struct Section { const char *name; size_t at, bytes; };

static void test_upright2p(int mp)
{
    const size_t m = (size_t)mp, chunk = 4 * ((m + 63) / 64 + 1);
    const Upright2pLds L = upright2p_lds(mp);
    const Section s[] = {{"mx", L.mx, 8 * m}, {"my", L.my, 8 * m}, {"mz", L.mz, 8 * m}, {"rx", L.rx, 8 * m}, {"ry", L.ry, 8 * m},
                         {"rz", L.rz, 8 * m}, {"nu", L.nu, 8 * m}, {"nv", L.nv, 8 * m}, {"mod", L.mod, 8 * 256 * 5}, {"cost", L.cost, 8 * 256},
                         {"best", L.best, 8 * 5}, {"rot", L.rot, 8 * 18},
                         {"map", L.map, 4 * m}, {"vmap", L.vmap, 4 * m}, {"st", L.st, 4 * m}, {"idx", L.idx, 4 * m}, {"chunk", L.chunk, chunk},
                         {"pair", L.pair, 4 * 2 * 128}, {"draw", L.draw, 4 * 2 * 128}, {"cnt", L.cnt, 4 * 256}, {"ctl", L.ctl, 4 * 16}};
    const size_t N = sizeof(s) / sizeof(s[0]), n_doubles = 12;
    CHECK(s[0].at == 0, "mp %d", mp);
    for (size_t i = 0; i < N; i++) {
        CHECK(s[i].at % (i < n_doubles ? 8 : 4) == 0, "mp %d: %s at %zu", mp, s[i].name, s[i].at);
        const size_t next = i + 1 < N ? s[i + 1].at : L.end;
        CHECK(s[i].bytes > 0 && s[i].at + s[i].bytes == next, "mp %d: %s [%zu, +%zu) then %zu", mp, s[i].name, s[i].at, s[i].bytes, next);
    }
    CHECK(L.end == 8 * (8 * m + 256 * 5 + 256 + 5 + 18) + 4 * (4 * m + (m + 63) / 64 + 1 + 2 * 128 * 2 + 256 + 16), "mp %d: %zu", mp, L.end);
}

int main()
{
    for (int mp : {1, 2, 5, 63, 64, 65, 257, 1024}) test_upright2p(mp);
    CHECK(U2_THREADS == 256 && U2_WAVES == 4 && U2_CHUNK == 128 && U2_MODEL == 5, "upright2p constants");
    CHECK(upright2p_lds(1024).end == 97596, "%zu", upright2p_lds(1024).end);          // 8 * 9751 + 4 * 4897
    // the largest shape (1024 points) beside the kernel's static LDS (two camera models, T)
    CHECK(upright2p_lds(1024).end + 2048 <= LDS_CU_BYTES, "the largest shape fits a CU");
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all upright2p lds layout tests passed\n");
    return 0;
}
