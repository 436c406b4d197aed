// Stand-alone test of hybvio_amd/csrc/hv_stage.hpp (plain g++ -std=c++17, no HIP): the arena is a DevBuf over the counting allocator
// of test_dev_buf.cpp, the five runtime operations are memcpy / no-ops that log their calls. Carving, the copies of upload() and
// download() (which, how many bytes, in which order), growth, a failed allocation, overflow of the pending-copy record, and a round
// trip of real arrays between sentinel bytes. Run by tests/test_stage.py, plain and under the address / undefined-behaviour sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>
#include "../../hybvio_amd/csrc/hv_stage.hpp"

using namespace hv;

static int failures = 0;
#define CHECK(cond, ...)                                                                      \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            if (++failures <= 20) { std::printf("FAILED %s:%d  %s  [", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("]\n"); } \
        }                                                                                     \
    } while (0)

// what the runtime was asked to do, in order: 'A'lloc, 'F'ree, 'D'rain, 'U'pload, 'H' download to the host, 'S'ynchronise
struct Event { char kind; const void *dst, *src; size_t bytes; };
static std::vector<Event> events;
static size_t count_of(char kind) { size_t n = 0; for (const Event &e : events) n += e.kind == kind; return n; }

static std::set<void *> live;
static long n_alloc = 0, bad_free = 0, fail_at = 0;                  // fail_at: the allocation (1-based, counted from arm()) that fails
static void arm(long k) { n_alloc = 0; fail_at = k; }

namespace hv {
struct Ctx { DevBuf<unsigned char> d_stage; int drain_rc = HV_OK; };

int dev_alloc(void **p, size_t bytes)
{
    *p = nullptr;
    if (++n_alloc == fail_at) return HV_ERR_NOMEM;
    *p = std::malloc(bytes ? bytes : 1);
    live.insert(*p);
    events.push_back({'A', *p, nullptr, bytes});
    return HV_OK;
}
void dev_free(void *p)
{
    events.push_back({'F', p, nullptr, 0});
    if (!p || live.erase(p) != 1) ++bad_free;
    else std::free(p);
}
DevBuf<unsigned char> &stage_arena(Ctx *c) { return c->d_stage; }
int stage_drain(Ctx *c) { events.push_back({'D', nullptr, nullptr, 0}); return c->drain_rc; }
int stage_to_device(Ctx *, void *dst, const void *src, size_t bytes) { events.push_back({'U', dst, src, bytes}); std::memcpy(dst, src, bytes); return HV_OK; }
int stage_to_host(Ctx *, void *dst, const void *src, size_t bytes) { events.push_back({'H', dst, src, bytes}); std::memcpy(dst, src, bytes); return HV_OK; }
int stage_sync(Ctx *) { events.push_back({'S', nullptr, nullptr, 0}); return HV_OK; }
}  // namespace hv

static size_t pad16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

static void test_carving()
{
    Ctx c;
    arm(0); events.clear();
    Stage s(&c);
    const auto a = s.take<uint8_t>(5);
    const auto b = s.take<double>(3);
    const auto z = s.take<int>(0);
    const auto d = s.in<float>(nullptr, 7);
    const auto e = s.take<int>(4);
    CHECK(a.off == 0 && b.off == 16 && z.off == 16 + 32 && d.off == z.off && e.off == d.off + 32, "offsets %zu %zu %zu %zu %zu", a.off, b.off, z.off, d.off, e.off);
    CHECK(s.total == pad16(5) + pad16(24) + 0 + pad16(28) + pad16(16), "total is the sum of the padded sizes (%zu)", s.total);
    for (size_t off : {a.off, b.off, z.off, d.off, e.off}) CHECK(off % 16 == 0, "16-byte alignment (%zu)", off);
    CHECK(events.empty(), "declaring sections touches nothing");
    CHECK(s.upload() == HV_OK && c.d_stage.count() == s.total, "first upload allocates exactly the request");
    CHECK((uintptr_t)s.at(a) % 16 == 0 && (unsigned char *)s.at(b) == c.d_stage + 16 && (unsigned char *)s.at(e) + 16 == c.d_stage + s.total, "device pointers");
    CHECK(s.at_or_null(d) == nullptr && s.at(d) != nullptr && s.at_or_null(a) == s.at(a), "a null host array reads as null through the nullable accessor only");
    CHECK(count_of('U') == 0 && count_of('H') == 0, "nothing to copy");
}

static void test_copies()
{
    Ctx c;
    arm(0); events.clear();
    int n = 3; float xy[6] = {1, 2, 3, 4, 5, 6}; double chi[3] = {}; uint8_t flags[3] = {7, 8, 9}; int status[5] = {};
    Stage s(&c);
    const auto o_n = s.in(&n, 1);
    const auto o_xy = s.inout(xy, 6);
    const auto o_none = s.in<double>(nullptr, 9);
    const auto o_chi = s.out(chi, 3);
    const auto o_skip = s.out<int>(nullptr, 2);
    const auto o_flags = s.in(flags, 3);
    const auto o_st = s.out(status, 5);
    CHECK(s.upload() == HV_OK, "upload");
    std::vector<Event> up;
    for (const Event &e : events) if (e.kind == 'U') up.push_back(e);
    CHECK(up.size() == 3, "%zu uploads", up.size());
    if (up.size() == 3) {
        CHECK(up[0].dst == s.at(o_n) && up[0].src == &n && up[0].bytes == sizeof(int), "first: n");
        CHECK(up[1].dst == s.at(o_xy) && up[1].src == xy && up[1].bytes == 6 * sizeof(float), "second: xy");
        CHECK(up[2].dst == s.at(o_flags) && up[2].src == flags && up[2].bytes == 3, "third: flags");
    }
    CHECK(events.back().kind == 'U' && count_of('D') == 1 && count_of('S') == 0 && count_of('H') == 0, "reserve, then the uploads, no synchronise");
    CHECK(s.at_or_null(o_none) == nullptr && s.at_or_null(o_skip) == nullptr && s.at(o_none) && s.at(o_skip), "null host arrays are carved, not copied");
    events.clear();
    CHECK(s.download() == HV_OK, "download");
    CHECK(events.size() == 4 && events[3].kind == 'S', "three downloads and one synchronise behind them (%zu events)", events.size());
    if (events.size() == 4) {
        CHECK(events[0].kind == 'H' && events[0].dst == xy && events[0].src == s.at(o_xy) && events[0].bytes == 6 * sizeof(float), "first: xy");
        CHECK(events[1].kind == 'H' && events[1].dst == chi && events[1].src == s.at(o_chi) && events[1].bytes == 3 * sizeof(double), "second: chi2");
        CHECK(events[2].kind == 'H' && events[2].dst == status && events[2].src == s.at(o_st) && events[2].bytes == 5 * sizeof(int), "third: status");
    }
    events.clear();
    int first2[2] = {-1, -1};
    CHECK(s.fetch(first2, o_st, 2) == HV_OK && events.size() == 1 && events[0].kind == 'H' && events[0].bytes == 2 * sizeof(int) && events[0].src == s.at(o_st),
          "fetch copies the leading elements now, without a synchronise");
    CHECK(s.sync() == HV_OK && events.back().kind == 'S', "sync");
}

static void test_growth()
{
    Ctx c;
    arm(0); events.clear();
    { Stage s(&c); s.take<uint8_t>(1000); CHECK(s.reserve() == HV_OK && c.d_stage.count() == 1008, "first reservation (%zu)", c.d_stage.count()); }
    CHECK(events.size() == 2 && events[0].kind == 'D' && events[1].kind == 'A', "drain, then allocate");
    events.clear();
    { Stage s(&c); s.take<double>(126); CHECK(s.upload() == HV_OK && events.empty(), "a request that fits changes nothing"); }
    { Stage s(&c); s.take<uint8_t>(1009); CHECK(s.reserve() == HV_OK && c.d_stage.count() == 2016, "a little more doubles the arena (%zu)", c.d_stage.count()); }
    CHECK(events.size() == 3 && events[0].kind == 'D' && events[1].kind == 'F' && events[2].kind == 'A' && events[2].bytes == 2016, "drain before the free, free before the allocation");
    events.clear();
    { Stage s(&c); s.take<uint8_t>(10000); CHECK(s.reserve() == HV_OK && c.d_stage.count() == 10000, "much more allocates the request (%zu)", c.d_stage.count()); }
    events.clear();
    c.drain_rc = HV_ERR_HIP;
    { Stage s(&c); s.take<uint8_t>(30000); CHECK(s.upload() == HV_ERR_HIP && c.d_stage.count() == 10000 && count_of('F') == 0, "a failed drain frees nothing"); }
    c.drain_rc = HV_OK;
}

static void test_failed_allocation()
{
    for (long k = 1; k <= 2; k++) {
        Ctx c;
        arm(k); events.clear();
        float in[4] = {1, 2, 3, 4};
        int rc1 = HV_OK;
        if (k == 2) { Stage s(&c); s.take<float>(4); rc1 = s.reserve(); }
        Stage s(&c);
        s.in(in, 4); s.in(in, 4); s.in(in, 4);
        const int rc = s.upload();
        CHECK(rc1 == HV_OK && rc == HV_ERR_NOMEM, "allocation %ld fails", k);
        CHECK(count_of('U') == 0, "nothing was copied");
        CHECK(c.d_stage.count() == 0 && c.d_stage.get() == nullptr && live.empty(), "the arena is left empty (%zu live)", live.size());
        arm(0);
        CHECK(s.upload() == HV_OK && count_of('U') == 3 && c.d_stage.count() == 48, "the same call works once memory is there");
    }
}

static void test_overflow()
{
    Ctx c;
    arm(0); events.clear();
    float v[2] = {1, 2};
    Stage s(&c);
    for (int i = 0; i < Stage::MAX_COPIES; i++) s.in(v, 2);
    { Stage t = s; CHECK(t.upload() == HV_OK && count_of('U') == (size_t)Stage::MAX_COPIES, "a full record is served"); }
    events.clear();
    s.out(v, 2);
    CHECK(s.upload() == HV_ERR_INVALID && s.download() == HV_ERR_INVALID, "one declaration too many is an error");
    CHECK(count_of('U') == 0 && count_of('H') == 0 && count_of('S') == 0, "... with nothing copied");
}

template <class T> static std::vector<T> pattern(size_t n, int seed)
{
    std::vector<T> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (T)((i * 37 + seed) % 251);
    return v;
}

static void test_values()
{
    Ctx c;
    arm(0);
    for (size_t n : {(size_t)1, (size_t)3, (size_t)67}) {
        const std::vector<uint8_t> u0 = pattern<uint8_t>(n, 1);
        const std::vector<int> i0 = pattern<int>(n, 2);
        const std::vector<float> f0 = pattern<float>(n, 3);
        const std::vector<double> d0 = pattern<double>(n, 4);
        std::vector<uint8_t> u = u0; std::vector<int> i = i0; std::vector<float> f = f0; std::vector<double> d = d0;
        Stage s(&c);
        const auto o_u = s.inout(u.data(), n);
        const auto gap = s.take<uint8_t>(5);
        const auto o_i = s.inout(i.data(), n);
        const auto o_f = s.inout(f.data(), n);
        const auto o_d = s.inout(d.data(), n);
        CHECK(s.reserve() == HV_OK, "reserve");
        std::memset(c.d_stage.get(), 0xA5, c.d_stage.count());
        CHECK(s.upload() == HV_OK, "upload");
        const unsigned char *base = c.d_stage;
        const size_t used[5][2] = {{o_u.off, n}, {gap.off, 0}, {o_i.off, n * sizeof(int)}, {o_f.off, n * sizeof(float)}, {o_d.off, n * sizeof(double)}};
        std::vector<bool> written(c.d_stage.count(), false);
        for (const auto &r : used) for (size_t k = 0; k < r[1]; k++) written[r[0] + k] = true;
        size_t touched = 0;
        for (size_t k = 0; k < c.d_stage.count(); k++) if (!written[k] && base[k] != 0xA5) ++touched;
        CHECK(touched == 0, "%zu bytes outside the declared arrays changed (n = %zu)", touched, n);
        CHECK(std::memcmp(s.at(o_u), u0.data(), n) == 0 && std::memcmp(s.at(o_i), i0.data(), n * sizeof(int)) == 0 &&
              std::memcmp(s.at(o_f), f0.data(), n * sizeof(float)) == 0 && std::memcmp(s.at(o_d), d0.data(), n * sizeof(double)) == 0, "the arena holds the arrays (n = %zu)", n);
        std::fill(u.begin(), u.end(), 0); std::fill(i.begin(), i.end(), 0); std::fill(f.begin(), f.end(), 0.f); std::fill(d.begin(), d.end(), 0.0);
        CHECK(s.download() == HV_OK, "download");
        CHECK(u == u0 && i == i0 && std::memcmp(f.data(), f0.data(), n * sizeof(float)) == 0 && std::memcmp(d.data(), d0.data(), n * sizeof(double)) == 0,
              "the round trip is byte-equal (n = %zu)", n);
    }
}

int main()
{
    test_carving();
    test_copies();
    test_growth();
    test_failed_allocation();
    test_overflow();
    test_values();
    std::printf("live blocks at exit: %zu\n", live.size());
    if (failures || !live.empty() || bad_free) { std::printf("%d checks failed, %ld bad frees\n", failures, bad_free); return 1; }
    std::printf("all stage tests passed\n");
    return 0;
}
