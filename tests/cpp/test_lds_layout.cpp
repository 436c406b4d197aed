// Stand-alone test of hybvio_amd/csrc/lds_layout.hpp (plain g++ -std=c++17, no HIP): the stride rule, and for every layout that the
// regions are in order and disjoint, aligned where the kernels need it, add up to the total, hold every record a launch may carry and
// stay within the kernel's dynamic-LDS limit; then the byte counts of known shapes, worked out by hand from the launchers' formulas.
// Likewise ransac_lds.hpp, the layouts of the two RANSAC kernels.
// Run by tests/test_lds_layout.py.
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

constexpr int UPD_WAVES = 8, GATE_WAVES = 4, SGATE_WAVES = 4, SGATE_BIG_WAVES = 12, AUG_WAVES = 16;     // the kernels' workgroup sizes / 64

static bool stride_ok(int s) { return s % 32 == 15 || s % 32 == 17; }

static void test_stride()
{
    for (int r = 1; r <= 400; r++) {
        const int s = lds_stride(r);
        CHECK(s >= r && stride_ok(s), "rows %d -> %d", r, s);
        for (int q = r; q < s; q++) CHECK(!stride_ok(q), "rows %d: %d qualifies before %d", r, q, s);
        const int o = lds_stride_tight(r);
        CHECK(o >= r && o <= r + 1 && o % 2 == 1, "rows %d -> tight %d", r, o);
    }
}

static void test_update(int n, int nr, int l)
{
    const UpdateShape s = update_shape(n, nr, l, UPD_WAVES);
    const size_t hs = (size_t)(16 * s.ti) * (16 * s.lbk);
    CHECK(s.hs == hs, "n %d nr %d l %d", n, nr, l);
    CHECK(s.ti * 16 >= nr && (s.ti - 1) * 16 < nr && s.lbk * 16 >= l && (s.lbk - 1) * 16 < l, "n %d nr %d l %d", n, nr, l);
    CHECK(s.kmode == 0 ? s.Rs == nr + n + 1 : s.Rs == lds_stride(nr + n + 1), "n %d nr %d: Rs %d mode %d", n, nr, s.Rs, s.kmode);
    CHECK(s.kmode != 2 || (n <= 160 && nr <= 48), "n %d nr %d", n, nr);
    for (int kmode : {s.kmode, 1}) {                               // (1: HV_EKF_GATE_KMODE turns a mode-2 gate into mode 1)
        if (kmode != s.kmode && s.kmode != 2) continue;
        const UpdateLds L = update_lds(s.Rs, nr, UPD_WAVES, kmode != 0, kmode == 2 ? s.hs : 0);
        const size_t t_doubles = kmode ? (size_t)s.Rs * nr : 0, h_doubles = kmode == 2 ? hs : 0;
        CHECK(L.T == 0 && L.T + t_doubles <= L.chol && L.chol - t_doubles <= 1, "n %d nr %d mode %d", n, nr, kmode);
        CHECK(L.chol + chol_scratch_doubles(UPD_WAVES) == L.flag && L.chol + CHOL_RED == L.red, "n %d nr %d mode %d", n, nr, kmode);
        CHECK(L.flag + 2 == L.Hs && L.Hs + h_doubles == L.end, "n %d nr %d mode %d", n, nr, kmode);
        CHECK(L.chol % 2 == 0 && (L.chol + CHOL_COL) % 2 == 0 && L.Hs % 2 == 0, "n %d nr %d mode %d", n, nr, kmode);
        CHECK(lds_bytes(L) == 8 * (((t_doubles + 1) & ~(size_t)1) + CHOL_RED + UPD_WAVES + 2 + h_doubles), "n %d nr %d mode %d", n, nr, kmode);
        CHECK(lds_bytes(L) <= (kmode ? LDS_UPDATE_LIMIT : LDS_DEFAULT_LIMIT), "n %d nr %d mode %d: %zu bytes", n, nr, kmode, lds_bytes(L));
        if (kmode == 2 && s.two_r) CHECK((size_t)(nr + 1) * nr + 256 <= L.end - L.Hs, "n %d nr %d l %d", n, nr, l);
        // a ragged launch: the kernel carves for the record's own rows, inside the launch's bytes
        for (int rec = 1; rec <= nr && kmode; rec++) {
            const UpdateLds Lr = update_lds(lds_stride(rec + n + 1), rec, UPD_WAVES, true, h_doubles);
            CHECK(Lr.end <= L.end, "n %d nr %d record of %d rows", n, nr, rec);
        }
    }
    // the next mode up must not have fitted
    if (s.kmode == 0) CHECK(lds_bytes(update_lds(lds_stride(nr + n + 1), nr, UPD_WAVES, true, 0)) > LDS_UPDATE_LIMIT, "n %d nr %d", n, nr);
    if (s.kmode == 1 && n <= 160 && nr <= 48) CHECK(lds_bytes(update_lds(s.Rs, nr, UPD_WAVES, true, hs)) > LDS_UPDATE_LIMIT, "n %d nr %d l %d", n, nr, l);
}

static void test_gate_stream(int nr, int l)
{
    const int Rs = lds_stride(nr + 1);
    const GateStreamLds L = gate_stream_lds(tiles16(nr), tiles16(l), Rs, nr);
    const size_t hs = (size_t)(16 * tiles16(nr)) * (16 * tiles16(l));
    CHECK(L.Hs == 0 && L.T == L.Hs + hs && L.end == L.T + (size_t)Rs * nr + 2, "nr %d l %d", nr, l);
    CHECK(L.T % 2 == 0 && (L.Hs + CHOL_COL) % 2 == 0, "nr %d l %d", nr, l);
    CHECK(lds_bytes(L) == 8 * (hs + (size_t)Rs * nr + 2), "nr %d l %d", nr, l);
    // the launcher's rule as it stood before the layouts: the H area holds 808 doubles of scratch, the launch stays within 96 KB
    CHECK(gate_stream_admitted(L) == (hs >= 256 + 544 + 8 && 8 * (hs + (size_t)Rs * nr + 2) <= 96 * 1024), "nr %d l %d", nr, l);
    if (gate_stream_admitted(L)) {
        CHECK(L.Hs + chol_scratch_doubles(GATE_WAVES) <= L.T, "nr %d l %d: the scratch leaves the H area", nr, l);
        CHECK(lds_bytes(L) <= LDS_GATE_LIMIT, "nr %d l %d", nr, l);
    }
}

static void test_sparse_gate(int np, int ncam)
{
    const int nr = 2 * np * ncam, na_max = 7 * np + 1, na4 = (na_max + 3) & ~3;
    const SparseGateLds L = sparse_gate_lds(np, ncam);
    const size_t ints = 4 * (size_t)(na_max + 2);
    const size_t limit = nr > 48 ? LDS_SGATE_BIG_LIMIT : LDS_GATE_LIMIT;
    CHECK(L.big == (nr > 48), "np %d x %d", np, ncam);
    CHECK(L.Hs == 0 && L.Hs < L.T && L.T < L.acol && L.T % 2 == 0, "np %d x %d", np, ncam);
    CHECK(L.T - L.Hs >= (size_t)CHOL_SCRATCH_FLOOR && L.T - L.Hs >= (size_t)na4 * L.shape.nrp, "np %d x %d", np, ncam);
    CHECK((size_t)chol_scratch_doubles(L.big ? SGATE_BIG_WAVES : SGATE_WAVES) <= L.T - L.Hs, "np %d x %d", np, ncam);
    CHECK(L.acol - L.T >= (size_t)L.shape.Rs * nr, "np %d x %d", np, ncam);
    CHECK(L.bytes == 8 * ((L.T - L.Hs) + (L.acol - L.T)) + ints, "np %d x %d", np, ncam);
    CHECK(!L.shape.tight || (L.big && L.shape.nrp == HV_GATE_TIGHT_ROWS && L.shape.Rs % 2 == 1), "np %d x %d", np, ncam);
    CHECK(L.shape.tight || (L.shape.nrp == 16 * tiles16(nr) && stride_ok(L.shape.Rs)), "np %d x %d", np, ncam);
    CHECK(L.shape.Rs >= nr + 1 && L.shape.nrp >= nr, "np %d x %d", np, ncam);
    if (!L.supported) return;
    CHECK(L.bytes <= limit, "np %d x %d: %zu bytes", np, ncam, L.bytes);
    // every record the launch may carry, carved by the kernel for its own rows within the launch's Hs and T doubles
    for (int p = 1; p <= np; p++) {
        const int r = 2 * p * ncam, a4 = (7 * p + 1 + 3) & ~3;
        const SparseGateShape s = sparse_gate_shape(L.big, r, a4, L.acol - L.Hs);
        CHECK((size_t)a4 * s.nrp <= L.T - L.Hs, "np %d x %d, record of %d poses: Hc leaves its area", np, ncam, p);
        CHECK(8 * (L.T + (size_t)s.Rs * r) + 4 * (size_t)(7 * p + 1) <= L.bytes, "np %d x %d, record of %d poses", np, ncam, p);
        CHECK(s.Rs >= r + 1 && s.nrp >= r && (!s.tight || r <= HV_GATE_TIGHT_ROWS), "np %d x %d, record of %d poses", np, ncam, p);
    }
}

static void test_augment(int n)
{
    const AugmentLds L = augment_lds(n, AUG_WAVES);
    // Alignment: the kernel reads and writes these regions one double at a time (f64 MFMA operands are one double per lane; no double2
    // access), so 8 bytes is all they need and an even start is not a property of this layout: K = 7 n is odd for odd n. What holds:
    // the base is even, and with an even n so is every [HP | K | G] row block.
    CHECK(L.HP % 2 == 0 && (n % 2 || (L.K % 2 == 0 && L.G % 2 == 0 && L.S0 % 2 == 0)), "n %d", n);
    CHECK(L.HP == 0 && L.K == L.HP + 7 * n && L.G == L.K + 7 * n && L.S0 == L.G + 7 * n, "n %d", n);      // [HP | K | G] contiguous
    CHECK(L.Lc == L.S0 + 49 && L.vres == L.Lc + 49 && L.scratch == L.vres + 8, "n %d", n);
    CHECK(L.end - L.scratch >= AUG_WAVES * 16 * 17 && L.T14 == L.scratch + 14 * n && L.T14 + 14 * 14 <= L.end, "n %d", n);
    CHECK(L.end - L.scratch == AUG_WAVES * 16 * 17 || L.end == L.T14 + 14 * 14, "n %d", n);
    CHECK(lds_bytes(L) == 8 * (size_t)(21 * n + 49 + 49 + 8 + (L.end - L.scratch)), "n %d", n);
    CHECK(lds_bytes(L) <= LDS_AUGMENT_LIMIT, "n %d: %zu bytes", n, lds_bytes(L));
}

// The RANSAC kernels' layouts (ransac_lds.hpp, byte offsets): the sections ascend and do not overlap, the double sections are 8-byte
// aligned (the int sections 4-byte), and the total is the closed form that ransac5.hip / ransac3.hip carried before the layouts.
struct Section { const char *name; size_t at, bytes; };
template <size_t N> static void check_sections(const char *what, const Section (&s)[N], size_t n_doubles, size_t end, int mp, int it)
{
    for (size_t i = 0; i < N; i++) {
        CHECK(s[i].at % (i < n_doubles ? 8 : 4) == 0, "%s mp %d it %d: %s at %zu", what, mp, it, s[i].name, s[i].at);
        const size_t next = i + 1 < N ? s[i + 1].at : end;
        CHECK(s[i].bytes > 0 && s[i].at + s[i].bytes == next, "%s mp %d it %d: %s [%zu, +%zu) then %zu", what, mp, it, s[i].name, s[i].at, s[i].bytes, next);
    }
    CHECK(s[0].at == 0, "%s mp %d it %d", what, mp, it);
}

static void test_ransac(int mp, int it)
{
    const size_t m = (size_t)mp, t = (size_t)it, chunk = 4 * ((m + 63) / 64 + 1);
    const Ransac5Lds L = ransac5_lds(mp, it);
    const Section s5[] = {{"px1", L.px1, 8 * m}, {"py1", L.py1, 8 * m}, {"px2", L.px2, 8 * m}, {"py2", L.py2, 8 * m},
                          {"recs", L.recs, 8 * t * 106}, {"ws", L.ws, 8 * 4 * 290},
                          {"good", L.good, 4 * t * 10}, {"sub", L.sub, 4 * t * 5}, {"nroot", L.nroot, 4 * t}, {"ok", L.ok, 4 * t},
                          {"map", L.map, 4 * m}, {"vmap", L.vmap, 4 * m}, {"st", L.st, 4 * m}, {"chunk", L.chunk, chunk}, {"misc", L.misc, 4 * 16}};
    check_sections("ransac5", s5, 6, L.end, mp, it);
    CHECK(L.end == 8 * (4 * m + t * 106 + 4 * 290) + 4 * (t * 17 + 3 * m + (m + 63) / 64 + 1 + 16), "ransac5 mp %d it %d: %zu", mp, it, L.end);
    CHECK(REC == 106 && WS == 290 && R5_WAVES == 4 && REC_EE + 36 == REC_B && REC_B + 39 == REC_C && REC_C + 11 == REC_RE && REC_RE + 10 == REC_IM &&
          REC_IM + 10 == REC && WS_EET + 90 == WS_A && WS_A + 200 == WS, "ransac5 record and scratch");
    if (it != 1) return;                                           // (ransac3's layout does not depend on the iteration count)
    const Ransac3Lds K = ransac3_lds(mp);
    const Section s3[] = {{"wx", K.wx, 8 * m}, {"wy", K.wy, 8 * m}, {"wz", K.wz, 8 * m}, {"fu", K.fu, 8 * m}, {"fv", K.fv, 8 * m},
                          {"mod", K.mod, 8 * 256 * 12}, {"cost", K.cost, 8 * 256}, {"best", K.best, 8 * 12},
                          {"map", K.map, 4 * m}, {"vmap", K.vmap, 4 * m}, {"st", K.st, 4 * m}, {"idx", K.idx, 4 * m}, {"chunk", K.chunk, chunk},
                          {"tri", K.tri, 4 * 3 * 64}, {"draw", K.draw, 4 * 3 * 64}, {"cnt", K.cnt, 4 * 256}, {"ctl", K.ctl, 4 * 16}};
    check_sections("ransac3", s3, 8, K.end, mp, 0);
    CHECK(K.end == 8 * (5 * m + 256 * 12 + 256 + 12) + 4 * (4 * m + (m + 63) / 64 + 1 + 3 * 64 * 2 + 256 + 16), "ransac3 mp %d: %zu", mp, K.end);
    CHECK(R3_THREADS == 256 && R3_CHUNK == 64, "ransac3 constants");
}

// byte counts and decisions of known shapes, worked out by hand from the launchers' formulas as they stood before the layouts
static void test_pinned()
{
    struct U { int n, nr, l, Rs, kmode; size_t bytes; };
    for (const U &u : {U{160, 44, 160, 207, 2, 140784}, U{160, 48, 160, 209, 2, 148176}, U{160, 80, 160, 241, 1, 160720},
                       U{160, 84, 160, 245, 0, 6480}, U{205, 44, 205, 271, 1, 0}}) {
        const UpdateShape s = update_shape(u.n, u.nr, u.l, UPD_WAVES);
        CHECK(s.Rs == u.Rs && s.kmode == u.kmode, "update n %d nr %d: Rs %d mode %d", u.n, u.nr, s.Rs, s.kmode);
        const size_t bytes = lds_bytes(update_lds(s.Rs, u.nr, UPD_WAVES, s.kmode != 0, s.kmode == 2 ? s.hs : 0));
        if (u.bytes) CHECK(bytes == u.bytes, "update n %d nr %d: %zu", u.n, u.nr, bytes);
    }
    CHECK(update_shape(160, 44, 160, UPD_WAVES).two_r && !update_shape(160, 80, 160, UPD_WAVES).two_r, "mode 3");
    const SparseGateLds a = sparse_gate_lds(10, 2), b = sparse_gate_lds(20, 2), c = sparse_gate_lds(21, 2);
    CHECK(!a.big && a.supported && a.bytes == 42980, "sparse 10 x 2: %zu", a.bytes);
    CHECK(b.big && b.supported && !b.shape.tight && b.bytes == 144572, "sparse 20 x 2: %zu", b.bytes);
    CHECK(c.big && c.supported && c.shape.tight && c.bytes == 157848 && c.T - c.Hs == 12432 && c.acol - c.T == 7224, "sparse 21 x 2: %zu", c.bytes);
    CHECK(!sparse_gate_lds(24, 2).supported, "sparse 24 x 2 (96 rows) has no layout");
    CHECK(lds_bytes(augment_lds(160, AUG_WAVES)) == 62544 && lds_bytes(augment_lds(160, AUG_WAVES)) <= LDS_DEFAULT_LIMIT, "augment n 160");
    CHECK(lds_bytes(augment_lds(205, AUG_WAVES)) == 70104 && lds_bytes(augment_lds(205, AUG_WAVES)) > LDS_DEFAULT_LIMIT, "augment n 205");
    const GateStreamLds g = gate_stream_lds(3, 10, lds_stride(41), 40), d = gate_stream_lds(1, 3, lds_stride(9), 8);
    CHECK(lds_bytes(g) == 76496 && gate_stream_admitted(g), "streaming gate 40 x 160");
    CHECK(!gate_stream_admitted(d), "streaming gate 8 x 41 is declined");
    CHECK(chol_scratch_doubles(4) == 804 && CHOL_COL == 256 && CHOL_RED == 800, "Cholesky scratch");
    CHECK(LDS_CU_BYTES == 163840 && LDS_DEFAULT_LIMIT == 65536 && LDS_GATE_LIMIT == 98304 && LDS_SGATE_BIG_LIMIT == 163776 && LDS_AUGMENT_LIMIT == 161792, "limits");
}

int main()
{
    test_stride();
    for (int n : {27, 55, 160, 169, 188, 205}) {
        for (int nr = 1; nr <= 96; nr++)
            for (int l : {1, 16, 17, n}) {
                test_update(n, nr, l);
                if (nr <= 48) test_gate_stream(nr, l);
            }
        test_augment(n);
    }
    for (int ncam = 1; ncam <= 2; ncam++)
        for (int np = 2; np <= 21; np++) test_sparse_gate(np, ncam);
    for (int mp : {1, 5, 63, 64, 65, 1024})
        for (int it : {1, 4, 5, 75}) test_ransac(mp, it);
    // the largest shapes (1024 points; 75 iterations, HV_RANSAC5_MAX_ITERS) beside the kernels' static LDS (two camera models, T)
    CHECK(ransac5_lds(1024, 75).end + 2048 <= LDS_CU_BYTES && ransac3_lds(1024).end + 2048 <= LDS_CU_BYTES, "the largest RANSAC shapes fit a CU");
    test_pinned();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all lds layout tests passed\n");
    return 0;
}
