// Dynamic-LDS layouts of the tracker-side RANSAC kernels (ransac5.hip, ransac3.hip, upright2p.hip), written once in the idiom of lds_layout.hpp:
// the launcher and the *_init function take the byte count, and the kernel carves its pointers, from the same description. Offsets are
// in BYTES from the base of the dynamic region, doubles first, then ints. Plain C++, no HIP header (tests/cpp/test_lds_layout.cpp).
#pragma once
#include "lds_layout.hpp"

namespace hv {

struct LdsCursor {                                              // hands out consecutive sections; `at` ends as the total
    size_t at = 0;
    HV_HD constexpr size_t doubles(size_t n) { const size_t o = at; at += sizeof(double) * n; return o; }
    HV_HD constexpr size_t ints(size_t n) { const size_t o = at; at += sizeof(int) * n; return o; }
};

// ---- ransac5_kernel ----
constexpr int R5_THREADS = 256, R5_WAVES = R5_THREADS / 64;
// per-hypothesis record (doubles): null basis EE[4][9], B[3][13], det polynomial c[11], roots re[10], im[10]
constexpr int REC_EE = 0, REC_B = 36, REC_C = 75, REC_RE = 86, REC_IM = 96, REC = 106;
constexpr int WS_EET = 0, WS_A = 90, WS = 290;                  // per-wave scratch: E E^T quadratics (later the minors), A[10][20]
// px1 .. py2 [max_points]: the normalised points; recs [iters][REC]; ws [R5_WAVES][WS]; good [iters][10]: inlier count of (hypothesis,
// root), -1 = no model; sub [iters][5]; nroot, ok [iters]; map: tracked k -> feature; vmap: valid j -> tracked k; st [max_points];
// chunk: block_compact's scratch; misc [16]
struct Ransac5Lds { size_t px1, py1, px2, py2, recs, ws, good, sub, nroot, ok, map, vmap, st, chunk, misc, end; };
HV_HD constexpr Ransac5Lds ransac5_lds(int max_points, int iters)
{
    const size_t mp = (size_t)max_points, it = (size_t)iters;
    LdsCursor c;                                                // (a braced list is evaluated left to right)
    return Ransac5Lds{c.doubles(mp), c.doubles(mp), c.doubles(mp), c.doubles(mp), c.doubles(it * REC), c.doubles(R5_WAVES * WS),
                      c.ints(it * 10), c.ints(it * 5), c.ints(it), c.ints(it), c.ints(mp), c.ints(mp), c.ints(mp),
                      c.ints((mp + 63) / 64 + 1), c.ints(16), c.at};
}

// ---- ransac3_kernel ----
constexpr int R3_THREADS = 256, R3_WAVES = R3_THREADS / 64;
constexpr int R3_CHUNK = 64;                       // iterations per round; R3_CHUNK * 4 solutions = one lane each in the cost phase
static_assert(R3_CHUNK * 4 == R3_THREADS, "one lane per (hypothesis, solution)");
// wx .. fv [max_points]: world points and image points; mod [R3_THREADS][12]: R row-major, c; cost [R3_THREADS] (P3P: the quartic's
// roots); best [12]; map: tracked k -> feature; vmap: valid j -> tracked k; st, idx [max_points]; chunk: block_compact's scratch;
// tri [R3_CHUNK][3]; draw [R3_CHUNK][3] (unsigned); cnt [R3_THREADS]: inlier count, -1 = no model; ctl [16]
struct Ransac3Lds { size_t wx, wy, wz, fu, fv, mod, cost, best, map, vmap, st, idx, chunk, tri, draw, cnt, ctl, end; };
HV_HD constexpr Ransac3Lds ransac3_lds(int max_points)
{
    const size_t mp = (size_t)max_points;
    LdsCursor c;
    return Ransac3Lds{c.doubles(mp), c.doubles(mp), c.doubles(mp), c.doubles(mp), c.doubles(mp), c.doubles(R3_THREADS * 12),
                      c.doubles(R3_THREADS), c.doubles(12), c.ints(mp), c.ints(mp), c.ints(mp), c.ints(mp), c.ints((mp + 63) / 64 + 1),
                      c.ints(3 * R3_CHUNK), c.ints(3 * R3_CHUNK), c.ints(R3_THREADS), c.ints(16), c.at};
}

// ---- upright2p_kernel ----
constexpr int U2_THREADS = 256, U2_WAVES = U2_THREADS / 64;
constexpr int U2_CHUNK = 128;                      // iterations per round; U2_CHUNK * 2 roots = one lane each (solver and cost phase)
static_assert(U2_CHUNK * 2 == U2_THREADS, "one lane per (hypothesis, root)");
constexpr int U2_MODEL = 5;                        // a model: c, s of the rotation about z, then t
// mx .. mz, rx .. rz, nu, nv [max_points]: rotated model points, rotated rays, normalised rays; mod [U2_THREADS][U2_MODEL];
// cost [U2_THREADS]; best [U2_MODEL]; rot [2][9]: R0, R1; map: tracked k -> feature; vmap: valid j -> tracked k; st, idx [max_points];
// chunk: block_compact's scratch; pair [U2_CHUNK][2]; draw [U2_CHUNK][2] (unsigned); cnt [U2_THREADS]: inlier count, -1 = no model; ctl [16]
struct Upright2pLds { size_t mx, my, mz, rx, ry, rz, nu, nv, mod, cost, best, rot, map, vmap, st, idx, chunk, pair, draw, cnt, ctl, end; };
HV_HD constexpr Upright2pLds upright2p_lds(int max_points)
{
    const size_t mp = (size_t)max_points;
    LdsCursor c;
    return Upright2pLds{c.doubles(mp), c.doubles(mp), c.doubles(mp), c.doubles(mp), c.doubles(mp), c.doubles(mp), c.doubles(mp),
                        c.doubles(mp), c.doubles(U2_THREADS * U2_MODEL), c.doubles(U2_THREADS), c.doubles(U2_MODEL), c.doubles(18),
                        c.ints(mp), c.ints(mp), c.ints(mp), c.ints(mp), c.ints((mp + 63) / 64 + 1), c.ints(2 * U2_CHUNK),
                        c.ints(2 * U2_CHUNK), c.ints(U2_THREADS), c.ints(16), c.at};
}

}  // namespace hv
