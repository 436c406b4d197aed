// hybvio_amd/csrc/hv_mt19937.hpp against <random>'s std::mt19937, built with the host compiler alone: the seed step, the tempering, and
// the three-phase twist run the way rng.hip runs it -- 64 simulated lanes, four words per lane and phase, every read of a phase into
// the lanes' registers before any write -- over several twists and seeds, with the lazy position rule of hv_rng on top (draw from a
// position, advance by a count). Also run with the lanes in reverse order: the schedule must not depend on which lane goes first.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "../../hybvio_amd/csrc/hv_mt19937.hpp"

using namespace hv;

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

constexpr int LANES = 64, CHUNKS = (mt::N - mt::M + LANES - 1) / LANES;

static void seed_array(uint32_t seed, uint32_t *w)
{
    w[0] = seed;
    for (int i = 1; i < mt::N; ++i) w[i] = mt::seed_step(w[i - 1], i);
}

// wave_twist of rng.hip with the lanes run one after the other inside each half of a phase
static void lanes_twist(uint32_t *w, bool reverse)
{
    for (int ph = 0; ph < mt::PHASES; ++ph) {
        const int begin = mt::PHASE_BEGIN[ph], end = mt::PHASE_BEGIN[ph + 1];
        uint32_t v[LANES][CHUNKS];
        for (int l = 0; l < LANES; ++l) {
            const int lane = reverse ? LANES - 1 - l : l;
            for (int q = 0; q < CHUNKS; ++q) {
                const int i = begin + q * LANES + lane;
                v[lane][q] = i < end ? mt::twist_word(w, i) : 0u;
            }
        }
        for (int l = 0; l < LANES; ++l) {
            const int lane = reverse ? LANES - 1 - l : l;
            for (int q = 0; q < CHUNKS; ++q) {
                const int i = begin + q * LANES + lane;
                if (i < end) w[i] = v[lane][q];
            }
        }
    }
    w[mt::N - 1] = mt::twist_last(w);
}

// the next n outputs from (w, pos) without changing them: rng_draw_kernel
static std::vector<uint32_t> draw(const uint32_t *w0, int pos, int n, bool reverse)
{
    std::vector<uint32_t> w(w0, w0 + mt::N), out;
    int p = pos, twists = 0;
    for (int k = 0; k < n;) {
        if (p == mt::N) { lanes_twist(w.data(), reverse); p = 0; ++twists; }
        const int m = (mt::N - p < n - k) ? mt::N - p : n - k;
        for (int j = 0; j < m; ++j) out.push_back(mt::temper(w[p + j]));
        k += m; p += m;
    }
    CHECK(twists == mt::twists_for(pos, n));
    return out;
}

// rng_advance_kernel
static void advance(uint32_t *w, int &pos, int c, bool reverse)
{
    if (c == 0) return;
    const int twists = mt::twists_for(pos, c);
    for (int t = 0; t < twists; ++t) lanes_twist(w, reverse);
    pos = pos + c - mt::N * twists;
    CHECK(pos >= 1 && pos <= mt::N);
}

static void test_constants()
{
    CHECK(mt::PHASE_BEGIN[0] == 0 && mt::PHASE_BEGIN[1] == 227 && mt::PHASE_BEGIN[2] == 454 && mt::PHASE_BEGIN[3] == 623);
    CHECK(CHUNKS == 4 && CHUNKS * LANES >= mt::N - mt::M);
    CHECK(mt::twists_for(624, 1) == 1 && mt::twists_for(1, 623) == 0 && mt::twists_for(1, 624) == 1 && mt::twists_for(624, 624) == 1);
    CHECK(mt::twists_for(624, 625) == 2 && mt::twists_for(624, 2048) == 4 && mt::twists_for(0, 2048) == 3 && mt::twists_for(17, 0) == 0);
    CHECK(mt::temper(0u) == 0u);
}

static void test_known_answer()
{
    uint32_t w[mt::N];
    seed_array(5489u, w);
    int pos = mt::N;
    for (int left = 9999; left > 0;) { const int c = left < 2048 ? left : 2048; advance(w, pos, c, false); left -= c; }
    CHECK(draw(w, pos, 1, false)[0] == 4123659995u);
}

static void test_against_std(uint32_t seed, bool reverse)
{
    uint32_t w[mt::N];
    seed_array(seed, w);
    std::mt19937 ref(seed);
    // six twists' worth of outputs in one go (the stops below read up to 2048 + 1300 of them): every phase boundary and the wrap 623 -> 0, six times
    const std::vector<uint32_t> got = draw(w, mt::N, 6 * mt::N, reverse);
    std::vector<uint32_t> want(6 * mt::N);
    for (uint32_t &x : want) x = (uint32_t)ref();
    CHECK(got == want);
    // positions at and around the phase bounds: advance there, draw across the next two twists, compare with the skipped stream
    const int stops[] = {1, 226, 227, 396, 397, 453, 454, 622, 623, 624, 625, 1248, 2048};
    for (int a : stops) {
        uint32_t v[mt::N];
        seed_array(seed, v);
        int pos = mt::N;
        advance(v, pos, a, reverse);
        const std::vector<uint32_t> d = draw(v, pos, 1300, reverse);
        bool same = true;
        for (int i = 0; i < 1300; ++i) same = same && d[i] == want[a + i];
        CHECK(same);
        // an advance by 0 changes nothing, at pos = 624 too (no early twist)
        int pos2 = pos;
        uint32_t v2[mt::N];
        for (int i = 0; i < mt::N; ++i) v2[i] = v[i];
        advance(v2, pos2, 0, reverse);
        bool untouched = pos2 == pos;
        for (int i = 0; i < mt::N; ++i) untouched = untouched && v2[i] == v[i];
        CHECK(untouched);
    }
}

int main()
{
    test_constants();
    test_known_answer();
    for (uint32_t seed : {0u, 1u, 4649u, 5489u, 0xffffffffu})
        for (bool reverse : {false, true}) test_against_std(seed, reverse);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all mt19937 schedule tests passed\n");
    return 0;
}
