// Stand-alone test of hybvio_amd/csrc/dev_buf.hpp (plain g++ -std=c++17, no HIP): dev_alloc / dev_free are a counting allocator that
// can fail the k-th allocation. Every block is freed exactly once and never a null pointer (DevBuf: alloc, reset, destructor, move
// construction, move assignment); grow_buffers drains before it frees, frees the whole group before it allocates, and a failure in the
// middle leaves what the contract says. Run by tests/test_dev_buf.py, plain and under the address / undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include "../../hybvio_amd/csrc/dev_buf.hpp"

using namespace hv;

static int failures = 0;
#define CHECK(cond, ...)                                                                      \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            if (++failures <= 20) { std::printf("FAILED %s:%d  %s  [", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("]\n"); } \
        }                                                                                     \
    } while (0)

// the counting allocator
static std::set<void *> live;
static long n_alloc = 0, n_free = 0, bad_free = 0, fail_at = 0;      // fail_at: the allocation (1-based, counted from arm()) that fails
static size_t last_bytes = 0;
static void arm(long k) { n_alloc = 0; fail_at = k; }

namespace hv {
int dev_alloc(void **p, size_t bytes)
{
    *p = nullptr;
    if (++n_alloc == fail_at) return HV_ERR_NOMEM;
    *p = std::malloc(bytes ? bytes : 1);
    live.insert(*p);
    last_bytes = bytes;
    return HV_OK;
}
void dev_free(void *p)
{
    ++n_free;
    if (!p || live.erase(p) != 1) ++bad_free;                            // null, never allocated, or freed twice
    else std::free(p);
}
}  // namespace hv

static void test_single()
{
    arm(0);
    {
        DevBuf<double> a;
        CHECK(!a && a.get() == nullptr && a.count() == 0, "a new buffer is empty");
        a.reset();
        CHECK(n_free == 0, "reset of an empty buffer frees nothing");
        CHECK(a.alloc(5) == HV_OK && a && a.count() == 5 && last_bytes == 5 * sizeof(double) && live.size() == 1, "alloc");
        double *first = a;
        CHECK(first == a.get() && live.count(first) == 1, "conversion to T *");
        CHECK(a.alloc(9) == HV_OK && a.count() == 9 && live.size() == 1 && n_free == 1, "alloc frees what it held");
        CHECK(a.alloc_once(100) == HV_OK && a.count() == 9 && live.size() == 1, "alloc_once leaves a held block alone");
        DevBuf<double> b(std::move(a));
        CHECK(!a && a.count() == 0 && b.count() == 9 && live.size() == 1, "move construction");
        DevBuf<double> c;
        CHECK(c.alloc_once(3) == HV_OK && c.count() == 3 && live.size() == 2, "alloc_once of an empty buffer");
        double *held = b;
        c = std::move(b);
        CHECK(!b && c.get() == held && c.count() == 9 && live.size() == 1, "move assignment frees the target's block");
        DevBuf<double> &self = c;
        c = std::move(self);
        CHECK(c.get() == held && live.size() == 1, "self move assignment");
        a = std::move(b);                                                // empty into empty
        CHECK(!a && live.size() == 1, "move of an empty buffer");
        DevBuf<int> d;
        arm(1);
        CHECK(d.alloc(4) == HV_ERR_NOMEM && !d && d.count() == 0, "a failed alloc reads as empty");
        arm(2);
        CHECK(d.alloc(4) == HV_OK && d.alloc(8) == HV_ERR_NOMEM && !d && d.count() == 0 && live.size() == 1, "a failed re-alloc has freed the old block");
        arm(0);
        c.reset();
        CHECK(!c && c.count() == 0 && live.empty(), "reset");
        CHECK(d.alloc(2) == HV_OK && live.size() == 1, "alloc after a failure");
    }                                                                    // d's destructor frees its block; the others are empty
    CHECK(live.empty(), "%zu blocks live after the destructors", live.size());
    CHECK(bad_free == 0, "%ld null / double / foreign frees", bad_free);
}

// a three-buffer group with its capacity field, grown the way the library's groups grow
struct Group {
    DevBuf<double> a; DevBuf<int> b; DevBuf<unsigned char> c;
    size_t cap = 0;
    int drains = 0;
    int ensure(size_t n, int drain_rc = HV_OK)
    {
        if (cap >= n) return HV_OK;
        cap = 0;
        const size_t live_before = live.size();
        const long free_before = n_free, alloc_before = n_alloc;
        const int rc = grow_buffers([&]() -> int {
            ++drains;
            CHECK(live.size() == live_before && n_free == free_before && n_alloc == alloc_before, "the drain runs before anything is freed or allocated");
            return drain_rc;
        }, {{a, n}, {b, 2 * n}, {c, 3 * n}});
        if (rc == HV_OK) cap = n;
        return rc;
    }
};

static void test_group()
{
    for (int k = 1; k <= 3; k++) {
        Group g;
        arm(0);
        CHECK(g.ensure(4) == HV_OK && g.cap == 4 && g.a.count() == 4 && g.b.count() == 8 && g.c.count() == 12 && live.size() == 3, "first growth");
        CHECK(g.ensure(3) == HV_OK && g.drains == 1 && n_alloc == 3, "a smaller request allocates nothing");
        const long frees = n_free;
        arm(k);
        CHECK(g.ensure(10) == HV_ERR_NOMEM, "allocation %d of the growth fails", k);
        CHECK(n_free - frees == 3, "the whole group is freed before the first allocation (%ld frees)", n_free - frees);
        CHECK(g.cap == 0, "the group reads as empty");
        CHECK((int)live.size() == k - 1, "only the %d blocks allocated before the failure live (%zu)", k - 1, live.size());
        CHECK((g.a.count() == 10) == (k > 1) && (g.b.count() == 20) == (k > 2) && !g.c, "members in front of the failure hold the new count, the others are empty");
        CHECK(!!g.a == (k > 1) && !!g.b == (k > 2), "pointer and count agree");
        arm(0);
        CHECK(g.ensure(2) == HV_OK && g.cap == 2 && g.a.count() == 2 && g.b.count() == 4 && g.c.count() == 6 && live.size() == 3,
              "an empty group grows again, at any size");
        CHECK(g.ensure(10) == HV_OK && g.cap == 10 && g.c.count() == 30 && live.size() == 3, "a later growth works");
        const long frees2 = n_free, allocs2 = n_alloc;
        CHECK(g.ensure(11, HV_ERR_HIP) == HV_ERR_HIP && n_free == frees2 && n_alloc == allocs2 && live.size() == 3 && g.a.count() == 10,
              "a failed drain ends the call with nothing freed");
        CHECK(g.cap == 0, "... and the group reads as empty to its owner");
    }
    CHECK(live.empty(), "%zu blocks live after the groups", live.size());
    CHECK(bad_free == 0, "%ld null / double / foreign frees", bad_free);
}

// locals that are moved into their owner on success and free themselves on an error exit (grow_pool, hv_ingest_set_undistort_map)
static int replace_pair(DevBuf<float> &x, DevBuf<float> &y, size_t n)
{
    DevBuf<float> nx, ny;
    if (nx.alloc(n) || ny.alloc(n)) return HV_ERR_NOMEM;
    x = std::move(nx); y = std::move(ny);
    return HV_OK;
}

static void test_replace()
{
    DevBuf<float> x, y;
    arm(0);
    CHECK(replace_pair(x, y, 4) == HV_OK && live.size() == 2, "first tables");
    float *px = x, *py = y;
    arm(2);
    CHECK(replace_pair(x, y, 6) == HV_ERR_NOMEM && x.get() == px && y.get() == py && x.count() == 4 && live.size() == 2, "a failure leaves the owner as it was");
    arm(0);
    CHECK(replace_pair(x, y, 6) == HV_OK && x.count() == 6 && y.count() == 6 && live.size() == 2 && !live.count(px) && !live.count(py), "replaced");
    CHECK(replace_pair(x, y, 0) == HV_OK, "zero elements");
    x.reset(); y.reset();
    CHECK(live.empty() && bad_free == 0, "%zu live, %ld bad frees", live.size(), bad_free);
}

int main()
{
    test_single();
    test_group();
    test_replace();
    std::printf("live blocks at exit: %zu\n", live.size());
    if (failures || !live.empty()) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all dev_buf tests passed\n");
    return 0;
}
