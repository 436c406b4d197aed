// Five-point essential-matrix RANSAC (doRansac5 without Theia) and the hybrid RANSAC2 / RANSAC5 track filter.
//
// Reference: src/tracker/ransac_pipeline.cpp:95-151 (compute), :158-195 (computeHybridRansac), :274-397 (doRansac5),
// src/tracker/ptsetreg.hpp:130-220 + ptsetreg.cpp:58-79 (RANSACPointSetRegistrator::run, getSubset, findInliers,
// RANSACUpdateNumIters), src/tracker/five_point.cpp:41-146, 374-400 (EMEstimatorCallback: Nister's solver, Sampson
// error), src/tracker/camera.cpp:471-476 (normalizePixel).
//
// One 256-thread workgroup per point set. The hypotheses of the registrator loop depend on the data only through the
// point count (fresh cv::RNG per call), so every hypothesis is solved up front and the loop's bookkeeping (strict `>`,
// adaptive niters) is replayed afterwards over the stored inlier counts:
//   1. the set: TRACKED features in feature order, normalised pixels (failures dropped), compacted with ballots
//   2. thread 0 replays cv::RNG and getSubset: max_iters x 5 indices
//   3. the minimal solve, one hypothesis per wavefront (4 in flight), its matrices in LDS:
//      Householder QR of the 9 x 5 transpose (columns in lanes, reflectors broadcast by __shfl) -> 4-dim null basis;
//      the 10 x 20 cubic-constraint matrix by polynomial products (one row per lane); Gaussian elimination with
//      partial pivoting of the left block, one column per lane, solved against the right block; B (3 x 13) and its
//      degree-10 determinant by polynomial convolution (one coefficient per lane)
//   4. cv::solvePoly's Durand-Kerner loop, one hypothesis per lane (the in-place update order is sequential per root)
//   5. one lane per (hypothesis, root): back-substitution of the root, E, and its inlier count over all points
//   6. thread 0 replays the loop; every lane rebuilds the best E and classifies its points; hybrid selection
// Arithmetic is binary64 in the operation order of tests/ransac5_restatement.py (the library is built without FMA
// contraction), so statuses, summaries and E equal the restatement except where pow / log of the niters update differ
// in the last bit.
#include "hv_camera.hpp"
#include "hv_internal.hpp"
#include "ransac_lds.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace hv {
namespace {

#include "hv_geometry.hpp"    // cross3, dot3
#include "hv_workgroup.hpp"   // block_compact, block_gather_front, stage_cameras

constexpr int R5_MAX_PTS = 1024;
constexpr int R5_MAX_ITERS = HV_RANSAC5_MAX_ITERS;
constexpr int DK_ITERS = 300;                                   // cv::solvePoly's default maxIters
// R5_THREADS, R5_WAVES, the per-hypothesis record REC_* and the per-wave scratch WS_*: ransac_lds.hpp

// quadratic monomial of two linear ones ([x, y, z, 1]); cubic column (Nister's order) of quadratic q times linear b
__device__ constexpr int IDX2[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
__device__ constexpr int IDX3[10][4] = {{0, 2, 4, 5}, {2, 3, 8, 9}, {4, 8, 10, 11}, {5, 9, 11, 12}, {3, 1, 6, 7},
                                        {8, 6, 13, 14}, {9, 7, 14, 15}, {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};

struct R5Args {
    int max_points, max_iters;
    const int *n_points;
    const float *c1, *c2;                 // [sets][max_points][2]
    int *track_status;                    // hybrid: [sets][max_points] Feature::Status in/out; NULL: every point is in the set
    const int *r2_status, *r2_summary;    // hybrid: RANSAC2's per-feature status and {bestInlierCount, visited}
    int *result;                          // hybrid: [sets][2] {type, inlierCount}
    double *score;                        // hybrid: [sets]
    int *status;                          // plain: [sets][max_points] 0 / 3
    double *E;                            // [sets][9] or NULL
    int *summary;                         // [sets][4] or NULL
    float thr2;                           // (float)(thr * thr)
    double prob, skip5, min_frac, over5;
    hv_camera_model cam1, cam2;
};

// a workgroup's LDS: the sections of Ransac5Lds as pointers (ws: this wavefront's scratch) and the staged cameras
struct R5View {
    double *px1, *py1, *px2, *py2, *recs, *ws;
    int *good, *sub, *nroot, *ok, *map, *vmap, *st, *chunk, *misc;
    const hv_camera_model *cam;
};
__device__ __forceinline__ R5View r5_view(unsigned char *base, const Ransac5Lds &L, int wave, const hv_camera_model *cam)
{
    auto d = [&](size_t off) { return reinterpret_cast<double *>(base + off); };
    auto i = [&](size_t off) { return reinterpret_cast<int *>(base + off); };
    return R5View{d(L.px1), d(L.py1), d(L.px2), d(L.py2), d(L.recs), d(L.ws) + wave * WS,
                  i(L.good), i(L.sub), i(L.nroot), i(L.ok), i(L.map), i(L.vmap), i(L.st), i(L.chunk), i(L.misc), cam};
}

// RANSACUpdateNumIters (ptsetreg.cpp:58-79), model points 5
__device__ int update_num_iters(double p, double ep, int max_iters)
{
    p = fmin(fmax(p, 0.0), 1.0);
    ep = fmin(fmax(ep, 0.0), 1.0);
    double num = fmax(1.0 - p, DBL_MIN);
    double denom = 1.0 - pow(1.0 - ep, 5.0);
    if (denom < DBL_MIN) return 0;
    num = log(num);
    denom = log(denom);
    return (denom >= 0 || -num >= max_iters * (-denom)) ? max_iters : __double2int_rn(num / denom);
}

// the model of root r of hypothesis rec (five_point.cpp:100-140): false when the root is dropped
__device__ bool model_of_root(const double *rec, int nroot, int r, double *E)
{
    if (r >= nroot || fabs(rec[REC_IM + r]) > 1e-10) return false;
    const double z1 = rec[REC_RE + r], z2 = z1 * z1, z3 = z2 * z1, z4 = z3 * z1;
    double row[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double *b = rec + REC_B + 13 * j;
        row[j][0] = ((b[0] * z3 + b[1] * z2) + b[2] * z1) + b[3];
        row[j][1] = ((b[4] * z3 + b[5] * z2) + b[6] * z1) + b[7];
        row[j][2] = (((b[8] * z4 + b[9] * z3) + b[10] * z2) + b[11] * z1) + b[12];
    }
    // null vector of B(z): the longest cross product of two rows (pairs 01, 02, 12; first maximum)
    double best[3], c[3];
    cross3(row[0], row[1], best);
    double bs = dot3(best, best);
    cross3(row[0], row[2], c);
    double s = dot3(c, c);
    if (s > bs) { best[0] = c[0]; best[1] = c[1]; best[2] = c[2]; bs = s; }
    cross3(row[1], row[2], c);
    s = dot3(c, c);
    if (s > bs) { best[0] = c[0]; best[1] = c[1]; best[2] = c[2]; bs = s; }
    const double nrm = sqrt(bs);
    if (!(nrm > 0)) return false;
    const double w0 = best[0] / nrm, w1 = best[1] / nrm, w2 = best[2] / nrm;
    if (fabs(w2) < 1e-10) return false;
    const double x = w0 / w2, y = w1 / w2;
    const double *N = rec + REC_EE;
    double e[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) e[i] = ((N[i] * x + N[9 + i] * y) + N[18 + i] * z1) + N[27 + i];
    double ss = e[0] * e[0];
#pragma unroll
    for (int i = 1; i < 9; ++i) ss = ss + e[i] * e[i];
    const double inv = 1.0 / (ss > 0 ? sqrt(ss) : 1.0);
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = e[i] * inv;
    return true;
}

// computeError (five_point.cpp:374-400) compared as findInliers does (ptsetreg.hpp:66-77)
__device__ __forceinline__ bool sampson_inlier(const double *e, double a1, double b1, double a2, double b2, float thr2)
{
    const double ex0 = (e[0] * a1 + e[1] * b1) + e[2], ex1 = (e[3] * a1 + e[4] * b1) + e[5], ex2 = (e[6] * a1 + e[7] * b1) + e[8];
    const double et0 = (e[0] * a2 + e[3] * b2) + e[6], et1 = (e[1] * a2 + e[4] * b2) + e[7];
    const double x2tex1 = (a2 * ex0 + b2 * ex1) + ex2;
    const double den = ((ex0 * ex0 + ex1 * ex1) + et0 * et0) + et1 * et1;
    return (float)((x2tex1 * x2tex1) / den) <= thr2;
}

// cv::solvePoly's Durand-Kerner loop on the trimmed polynomial, d[j] = c[n - j]; roots updated in place, in order
__device__ void durand_kerner(const double *d_lds, int n, double *re_out, double *im_out)
{
    double d[11], rr[10], ri[10];
#pragma unroll
    for (int j = 0; j < 11; ++j) d[j] = j <= n ? d_lds[n - j] : 0.0;
    double pr = 1.0, pi = 0.0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        rr[i] = pr; ri[i] = pi;
        const double tr = pr * 0.4 - pi * 0.9, ti = pr * 0.9 + pi * 0.4;
        pr = tr; pi = ti;
    }
    for (int it = 0; it < DK_ITERS; ++it) {
        double md = 0.0;
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            if (i < n) {
                const double qr0 = rr[i], qi0 = ri[i];
                double nr = d[0], ni = 0.0, dr = d[0], di = 0.0;
#pragma unroll
                for (int j = 0; j < 10; ++j) {
                    if (j < n) {
                        const double tr = nr * qr0 - ni * qi0, ti = nr * qi0 + ni * qr0;
                        nr = tr + d[j + 1]; ni = ti + 0.0;
                        if (j != i) {
                            const double sr = qr0 - rr[j], si = qi0 - ri[j];
                            const double ur = dr * sr - di * si, ui = dr * si + di * sr;
                            dr = ur; di = ui;
                        }
                    }
                }
                const double t = 1.0 / (dr * dr + di * di);
                const double qr = (nr * dr + ni * di) * t, qi = ((-nr) * di + ni * dr) * t;
                rr[i] = qr0 - qr; ri[i] = qi0 - qi;
                const double a = sqrt(qr * qr + qi * qi);
                md = md < a ? a : md;
            }
        }
        if (md <= 0) break;
    }
#pragma unroll
    for (int i = 0; i < 10; ++i) { re_out[i] = rr[i]; im_out[i] = ri[i]; }
}

// ---- the phases of ransac5_kernel, in the terms of tests/ransac5_restatement.py. Every thread of the workgroup calls every phase;
// each header says which barriers the phase holds and what they publish ----

// normalizePixel of both frames (camera.cpp:471-476) for the n tracked features, the valid ones compacted to the front (doRansac5
// :331-343); returns their number m. Begins without a barrier (s_map and s_cam are published by the caller). Barriers: one after the
// normalisation (publishes s_st and the points), block_compact's three, block_gather_front's one. Ends WITHOUT one: the gathered
// points are published by the caller's next barrier (draw_subsets').
__device__ __forceinline__ int normalise_set(const R5View &v, const float *c1, const float *c2, int n, int tid)
{
    for (int k = tid; k < n; k += R5_THREADS) {
        const int src = v.map[k];
        double h1[2], h2[2];
        const bool ok1 = normalize_pixel_positive(v.cam[0], c1[2 * src], c1[2 * src + 1], h1);
        const bool ok2 = normalize_pixel_positive(v.cam[1], c2[2 * src], c2[2 * src + 1], h2);
        v.st[k] = ok1 && ok2 ? 1 : 0;
        if (v.st[k]) { v.px1[k] = h1[0]; v.py1[k] = h1[1]; v.px2[k] = h2[0]; v.py2[k] = h2[1]; }
    }
    __syncthreads();
    const int m = block_compact<R5_WAVES>([&](int k) { return v.st[k] != 0; }, v.vmap, n, v.chunk);
    static_assert(R5_MAX_PTS <= 4 * R5_THREADS, "four points per thread");
    double *const pts[4] = {v.px1, v.py1, v.px2, v.py2};
    block_gather_front<R5_THREADS>(pts, v.vmap, m);
    return m;
}

// getSubset with cv::RNG((uint64)-1) (ptsetreg.hpp:79-125, 142) on thread 0: H x 5 indices into s_sub. Ends with a barrier, which
// publishes s_sub and the gathered points of normalise_set.
__device__ __forceinline__ void draw_subsets(const R5View &v, int m, int H, int tid)
{
    if (tid == 0) {
        if (m == 5) {
            for (int i = 0; i < 5; ++i) v.sub[i] = i;
        } else {
            unsigned long long state = ~0ull;
            for (int h = 0; h < H; ++h)
                for (int i = 0; i < 5; ++i) {
                    int x;
                    for (;;) {
                        state = (unsigned long long)(unsigned)state * 4164903690ull + (unsigned)(state >> 32);
                        x = (int)((unsigned)state % (unsigned)m);
                        int j = 0;
                        while (j < i && v.sub[5 * h + j] != x) ++j;
                        if (j == i) break;
                    }
                    v.sub[5 * h + i] = x;
                }
        }
    }
    __syncthreads();
}

// linear polynomial ([x, y, z, 1]) of entry (r, c) of E over the null basis N
__device__ __forceinline__ void e_lin(const double *N, int r, int c, double *p)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) p[q] = N[9 * q + 3 * r + c];
}

// 3a. Householder QR of M = Q^T (9 x 5) of hypothesis h, one per wavefront: lanes 0..4 hold the columns of M, lanes 5..13 the columns
// of P = H4 ... H0 (rows 5..8 of P = the null basis, into rec[REC_EE]). Ends with a barrier, which publishes the null basis.
__device__ __forceinline__ void null_basis(const R5View &v, double *rec, int h, bool act, int lane)
{
    double col[9];
    if (lane < 5) {
        const int s = act ? v.sub[5 * h + lane] : 0;
        const double x1 = act ? v.px1[s] : 0.0, y1 = act ? v.py1[s] : 0.0, x2 = act ? v.px2[s] : 0.0, y2 = act ? v.py2[s] : 0.0;
        col[0] = x1 * x2; col[1] = y1 * x2; col[2] = x2; col[3] = x1 * y2; col[4] = y1 * y2; col[5] = y2;
        col[6] = x1; col[7] = y1; col[8] = 1.0;
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) col[i] = (lane - 5 == i) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        double u[9];
#pragma unroll
        for (int i = k; i < 9; ++i) u[i] = __shfl(col[i], k);
        double s = u[k] * u[k];
#pragma unroll
        for (int i = k + 1; i < 9; ++i) s = s + u[i] * u[i];
        const double nrm = sqrt(s);
        const double alpha = u[k] >= 0 ? -nrm : nrm;
        u[k] = u[k] - alpha;
        double vv = u[k] * u[k];
#pragma unroll
        for (int i = k + 1; i < 9; ++i) vv = vv + u[i] * u[i];
        if (((lane > k && lane < 5) || (lane >= 5 && lane < 14)) && vv > 0) {
            double d = u[k] * col[k];
#pragma unroll
            for (int i = k + 1; i < 9; ++i) d = d + u[i] * col[i];
            const double f = (d + d) / vv;
#pragma unroll
            for (int i = k; i < 9; ++i) col[i] = col[i] - f * u[i];
        }
    }
    if (act && lane >= 5 && lane < 14) {
#pragma unroll
        for (int j = 0; j < 4; ++j) rec[REC_EE + 9 * j + (lane - 5)] = col[5 + j];
    }
    __syncthreads();
}

// 3b + 3c. The 10 x 20 cubic-constraint matrix A into the wave's scratch: E E^T (quadratics, one entry per lane), a barrier that
// publishes them, then the rows of A: (E E^T - tr(E E^T) / 2) E (rows 0..8, lanes 0..8) and det E (row 9, lane 9). Ends with a barrier,
// which publishes A.
__device__ __forceinline__ void coeff_matrix(const R5View &v, const double *rec, bool act, int lane)
{
    double *ws = v.ws;
    const double *N = rec + REC_EE;
    if (act && lane < 9) {
        const int i = lane / 3, k = lane % 3;
        double acc[10];
#pragma unroll
        for (int t = 0; t < 10; ++t) acc[t] = 0.0;
#pragma unroll
        for (int mm = 0; mm < 3; ++mm) {
            double p[4], q[4];
            e_lin(N, i, mm, p); e_lin(N, k, mm, q);
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) acc[IDX2[x][y]] = acc[IDX2[x][y]] + p[x] * q[y];
        }
#pragma unroll
        for (int t = 0; t < 10; ++t) ws[WS_EET + 10 * lane + t] = acc[t];
    }
    __syncthreads();
    if (act && lane < 9) {
        const int i = lane / 3, j = lane % 3;
        double acc[20];
#pragma unroll
        for (int t = 0; t < 20; ++t) acc[t] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double Mq[10], e[4];
#pragma unroll
            for (int t = 0; t < 10; ++t) {
                const double x = ws[WS_EET + 10 * (3 * i + k) + t];
                const double ht = 0.5 * ((ws[WS_EET + t] + ws[WS_EET + 40 + t]) + ws[WS_EET + 80 + t]);
                Mq[t] = i == k ? x - ht : x;
            }
            e_lin(N, k, j, e);
#pragma unroll
            for (int t = 0; t < 10; ++t)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[IDX3[t][b]] = acc[IDX3[t][b]] + Mq[t] * e[b];
        }
#pragma unroll
        for (int t = 0; t < 20; ++t) ws[WS_A + 20 * lane + t] = acc[t];
    } else if (act && lane == 9) {
        double acc[20];
#pragma unroll
        for (int t = 0; t < 20; ++t) acc[t] = 0.0;
        auto minor = [&](int r0, int c0, int r1, int c1_, int r2, int c2_, int r3, int c3, double *mo) {
            double p[4], q[4], r[4], s[4];
            e_lin(N, r0, c0, p); e_lin(N, r1, c1_, q); e_lin(N, r2, c2_, r); e_lin(N, r3, c3, s);
#pragma unroll
            for (int t = 0; t < 10; ++t) mo[t] = 0.0;
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) mo[IDX2[x][y]] = mo[IDX2[x][y]] + p[x] * q[y];
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) mo[IDX2[x][y]] = mo[IDX2[x][y]] - r[x] * s[y];
        };
#pragma unroll
        for (int term = 0; term < 3; ++term) {
            double mo[10], e[4];
            if (term == 0) minor(1, 1, 2, 2, 1, 2, 2, 1, mo);
            else if (term == 1) minor(1, 0, 2, 2, 1, 2, 2, 0, mo);
            else minor(1, 0, 2, 1, 1, 1, 2, 0, mo);
            e_lin(N, 0, term, e);
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int t = 0; t < 10; ++t) {
                    const int c = IDX3[t][x];
                    acc[c] = term == 1 ? acc[c] - e[x] * mo[t] : acc[c] + e[x] * mo[t];
                }
        }
#pragma unroll
        for (int t = 0; t < 20; ++t) ws[WS_A + 20 * 9 + t] = acc[t];
    }
    __syncthreads();
}

// 3d. Gaussian elimination with partial pivoting of the left block of A, one column per lane (0..19), solved against columns 10..19;
// rows 4..9 of the solution go back into A, the pivots' verdict into s_ok[h]. Ends with a barrier, which publishes both.
__device__ __forceinline__ void eliminate(const R5View &v, int h, bool act, int lane)
{
    double *ws = v.ws;
    double cl[10];
#pragma unroll
    for (int r = 0; r < 10; ++r) cl[r] = lane < 20 ? ws[WS_A + 20 * r + lane] : 0.0;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        double ck[10];
#pragma unroll
        for (int r = k; r < 10; ++r) ck[r] = __shfl(cl[r], k);
        int p = k;
        double bestv = fabs(ck[k]);
#pragma unroll
        for (int r = k + 1; r < 10; ++r)
            if (fabs(ck[r]) > bestv) { bestv = fabs(ck[r]); p = r; }
#pragma unroll
        for (int r = k + 1; r < 10; ++r)
            if (r == p) {
                double t = cl[k]; cl[k] = cl[r]; cl[r] = t;
                t = ck[k]; ck[k] = ck[r]; ck[r] = t;
            }
        const double piv = ck[k];
        ok = ok && piv != 0;
        const double pivs = piv != 0 ? piv : 1.0;
        if (lane > k && lane < 20) {
#pragma unroll
            for (int r = k + 1; r < 10; ++r) {
                const double l = ck[r] / pivs;
                cl[r] = cl[r] - l * cl[k];
            }
        }
    }
#pragma unroll
    for (int i = 9; i >= 0; --i) {
        double s = cl[i];
#pragma unroll
        for (int j = i + 1; j < 10; ++j) s = s - __shfl(cl[i], j) * cl[j];
        const double u = __shfl(cl[i], i);
        const double x = s / (u != 0 ? u : 1.0);
        if (lane >= 10 && lane < 20) cl[i] = x;
    }
    if (act && lane >= 10 && lane < 20) {
#pragma unroll
        for (int r = 4; r < 10; ++r) ws[WS_A + 20 * r + lane] = cl[r];
    }
    if (act && lane == 0) v.ok[h] = ok ? 1 : 0;
    __syncthreads();
}

// 3e. B (3 x 13) into rec[REC_B], one entry per lane: row i = <2i+4> - z <2i+5> (five_point.cpp:75-95). Ends with a barrier, which
// publishes B.
__device__ __forceinline__ void b_matrix(const R5View &v, double *rec, bool act, int lane)
{
    const double *ws = v.ws;
    if (act && lane < 39) {
        const int i = lane / 13, t = lane % 13;
        const int m1 = t == 0 || t == 4 || t == 8 ? -1 : t < 4 ? t - 1 : t < 8 ? t - 2 : t - 3;
        const int m2 = t == 3 || t == 7 || t == 12 ? -1 : t < 3 ? t : t < 7 ? t - 1 : t - 2;
        const double v1 = m1 >= 0 ? ws[WS_A + 20 * (2 * i + 4) + 10 + m1] : 0.0;
        const double v2 = m2 >= 0 ? ws[WS_A + 20 * (2 * i + 5) + 10 + m2] : 0.0;
        rec[REC_B + lane] = v1 - v2;
    }
    __syncthreads();
}

// ascending coefficient i of the x / y / 1 polynomial (part 0 / 1 / 2) of row j of B, and the polynomial's length
__device__ __forceinline__ double b_poly(const double *B, int j, int part, int i)
{
    return part == 0 ? (i < 4 ? B[13 * j + 3 - i] : 0.0) : part == 1 ? (i < 4 ? B[13 * j + 7 - i] : 0.0)
                                                                     : (i < 5 ? B[13 * j + 12 - i] : 0.0);
}
__device__ __forceinline__ int b_poly_len(int part) { return part == 2 ? 5 : 4; }

// 3f. det B(z) into rec[REC_C] by polynomial convolution: the three 2 x 2 minors of rows 1 and 2 (one coefficient per lane, into the
// wave's scratch), a barrier that publishes them, then the degree-10 polynomial (one coefficient per lane). Ends with a barrier, which
// publishes the polynomial and frees the scratch for the next round.
__device__ __forceinline__ void det_poly(const R5View &v, double *rec, bool act, int lane)
{
    double *ws = v.ws;
    const double *B = rec + REC_B;
    if (act && lane < 23) {
        const int which = lane < 8 ? 0 : lane < 16 ? 1 : 2, k = lane < 8 ? lane : lane < 16 ? lane - 8 : lane - 16;
        // m0 = y1 c2 - c1 y2, m1 = x1 c2 - c1 x2, m2 = x1 y2 - y1 x2
        const int pa = which == 0 ? 1 : 0, qa = which == 2 ? 1 : 2, ra = which == 2 ? 1 : 2, sa = which == 0 ? 1 : 0;
        double acc = 0.0;
        for (int i = 0; i < b_poly_len(pa); ++i) {
            const int j = k - i;
            if (j >= 0 && j < b_poly_len(qa)) acc = acc + b_poly(B, 1, pa, i) * b_poly(B, 2, qa, j);
        }
        for (int i = 0; i < b_poly_len(ra); ++i) {
            const int j = k - i;
            if (j >= 0 && j < b_poly_len(sa)) acc = acc - b_poly(B, 1, ra, i) * b_poly(B, 2, sa, j);
        }
        ws[WS_EET + 8 * which + k] = acc;
    }
    __syncthreads();
    if (act && lane < 11) {
        const int k = lane;
        double acc = 0.0;
        for (int i = 0; i < 4; ++i) { const int j = k - i; if (j >= 0 && j < 8) acc = acc + b_poly(B, 0, 0, i) * ws[WS_EET + j]; }
        for (int i = 0; i < 4; ++i) { const int j = k - i; if (j >= 0 && j < 8) acc = acc - b_poly(B, 0, 1, i) * ws[WS_EET + 8 + j]; }
        for (int i = 0; i < 5; ++i) { const int j = k - i; if (j >= 0 && j < 7) acc = acc + b_poly(B, 0, 2, i) * ws[WS_EET + 16 + j]; }
        rec[REC_C + k] = acc;
    }
    __syncthreads();
}

// 4. cv::solvePoly on the trimmed polynomial, one hypothesis per lane: roots into the record, their number into s_nroot (0: the
// elimination met a zero pivot). Ends with a barrier, which publishes both.
__device__ __forceinline__ void solve_poly(const R5View &v, int H, int tid)
{
    for (int h = tid; h < H; h += R5_THREADS) {
        double *rec = v.recs + (size_t)h * REC;
        int nr = 0;
        if (v.ok[h]) {
            nr = 10;
            while (nr > 1 && !(fabs(rec[REC_C + nr]) > DBL_EPSILON)) --nr;
            double re[10], im[10];
            durand_kerner(rec + REC_C, nr, re, im);
#pragma unroll
            for (int i = 0; i < 10; ++i) { rec[REC_RE + i] = re[i]; rec[REC_IM + i] = im[i]; }
        }
        v.nroot[h] = nr;
    }
    __syncthreads();
}

// 5. models_from_roots and their inlier counts over all m points, one (hypothesis, root) per lane, into s_good (-1: no model). Ends
// with a barrier, which publishes s_good.
__device__ __forceinline__ void score_models(const R5View &v, int H, int m, float thr2, int tid)
{
    for (int w = tid; w < H * 10; w += R5_THREADS) {
        const int h = w / 10, r = w - 10 * h;
        double E[9];
        int g = -1;
        if (model_of_root(v.recs + (size_t)h * REC, v.nroot[h], r, E)) {
            g = 0;
            for (int j = 0; j < m; ++j) g += sampson_inlier(E, v.px1[j], v.py1[j], v.px2[j], v.py2[j], thr2) ? 1 : 0;
        }
        v.good[w] = g;
    }
    __syncthreads();
}

// what the registrator loop leaves: bestInlierCount, the best model's hypothesis and root, the iterations made
struct R5Best { int best, bh, br, iters; };

// 6. registrator_runs: the loop of RANSACPointSetRegistrator::run (ptsetreg.hpp:176-199) replayed by thread 0 over the stored counts
// (strict `>`, adaptive niters). Ends with a barrier, which publishes the outcome through s_misc[0..3]; every thread returns it.
__device__ __forceinline__ R5Best registrator_runs(const R5View &v, int IT, int m, double prob, int tid)
{
    if (tid == 0) {
        int best = 0, bh = -1, br = -1;
        int niters = max(IT, 1), it = 0;
        for (; it < niters; ++it)
            for (int r = 0; r < 10; ++r) {
                const int g = v.good[10 * it + r];
                if (g >= 0 && g > max(best, 4)) {
                    best = g; bh = it; br = r;
                    niters = update_num_iters(prob, (double)(m - g) / (double)m, niters);
                }
            }
        v.misc[0] = best; v.misc[1] = bh; v.misc[2] = br; v.misc[3] = it;
    }
    __syncthreads();
    return R5Best{v.misc[0], v.misc[1], v.misc[2], v.misc[3]};
}

// The mask and E: every lane rebuilds the best model and classifies its points into s_st (0 inlier / 3 outlier, by tracked index);
// without a model the pre-filled all-1 mask stays (doRansac5 :345). Thread 0 writes E (E_out may be NULL). One barrier, between the
// fill of s_st and the scattered inlier writes. Ends WITHOUT one: s_st is published by the caller's next barrier.
__device__ __forceinline__ void mask_and_E(const R5View &v, const R5Best &b, int n, int m, float thr2, double *E_out, int tid)
{
    double Eb[9];
    const bool have = b.best > 0 && model_of_root(v.recs + (size_t)b.bh * REC, v.nroot[b.bh], b.br, Eb);
    for (int k = tid; k < n; k += R5_THREADS) v.st[k] = 3;
    __syncthreads();
    for (int j = tid; j < m; j += R5_THREADS)
        v.st[v.vmap[j]] = (!have || sampson_inlier(Eb, v.px1[j], v.py1[j], v.px2[j], v.py2[j], thr2)) ? 0 : 3;
    if (tid == 0) {
        double E[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (have) {
            for (int i = 0; i < 9; ++i) E[i] = Eb[i];
        } else if (m == 5) {                                       // count == modelPoints: the kernel's first model
#pragma unroll 1                                                   // (a rare path on one lane: ten inlined copies of the model only grow the kernel)
            for (int r = 0; r < 10; ++r)
                if (model_of_root(v.recs, v.nroot[0], r, E)) break;
                else for (int i = 0; i < 9; ++i) E[i] = 0.0;
        }
        if (E_out) for (int i = 0; i < 9; ++i) E_out[i] = E[i];
    }
}

// The inlier count of the RANSAC5 result (ransac_pipeline.cpp:390-394), 0 when it did not run. Begins with a barrier (s_st complete),
// a second one publishes the zeroed counter, the last one the sum.
__device__ __forceinline__ int count_inliers(const R5View &v, bool run5, int n, int tid)
{
    __syncthreads();
    if (tid == 0) v.misc[4] = 0;
    __syncthreads();
    if (run5) {
        int cnt = 0;
        for (int k = tid; k < n; k += R5_THREADS) cnt += v.st[k] == 0;
        if (cnt) atomicAdd(&v.misc[4], cnt);
    }
    __syncthreads();
    return v.misc[4];
}

// hybrid_select (ransac_pipeline.cpp:158-195) and the status rewrite (:29-40, 139-144). No barrier.
__device__ __forceinline__ void hybrid_select(const R5Args &a, const R5View &v, int set, int *ts, int n_all, int n, int r2count,
                                              int r5count, bool use_r2, bool run5, int tid)
{
    bool r2_done = n >= 2, r5_done = run5;
    const double f5 = (double)r5count / (double)n, f2 = (double)r2count / (double)n;
    if (f5 < a.min_frac) r5_done = false;
    if (f2 < a.min_frac) r2_done = false;
    int type;
    if (r2_done && !r5_done) type = 1;
    else if (r5_done && !r2_done) type = 3;
    else if (r2_done && r5_done) type = (use_r2 || (double)r2count > a.over5 * (double)r5count) ? 1 : 3;
    else type = 0;
    if (type == 0) {
        for (int i = tid; i < n_all; i += R5_THREADS) ts[i] = 3;
    } else {
        const int *r2s = a.r2_status + (size_t)set * a.max_points;
        for (int k = tid; k < n; k += R5_THREADS) {
            const int src = v.map[k];
            const bool inl = type == 1 ? r2s[src] == 0 : v.st[k] == 0;
            if (!inl) ts[src] = 3;
        }
    }
    if (tid == 0) {
        a.result[2 * (size_t)set] = type;
        a.result[2 * (size_t)set + 1] = type == 1 ? r2count : type == 3 ? r5count : 0;
        a.score[set] = n ? (double)r2count / (double)n : 0.0;
    }
}

__global__ __launch_bounds__(R5_THREADS) void ransac5_kernel(R5Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char r5_lds[];
    __shared__ hv_camera_model s_cam[2];
    const int set = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int MP = a.max_points, IT = a.max_iters;
    const R5View v = r5_view(r5_lds, ransac5_lds(MP, IT), wave, s_cam);
    stage_cameras<R5_THREADS>(s_cam, a.cam1, a.cam2);
    __syncthreads();                                            // publishes s_cam
    const int n_all = min(max(a.n_points[set], 0), MP);
    const float *c1 = a.c1 + (size_t)set * MP * 2, *c2 = a.c2 + (size_t)set * MP * 2;
    const bool hybrid = a.track_status != nullptr;
    int *ts = hybrid ? a.track_status + (size_t)set * MP : nullptr;

    // 1. the set: TRACKED features in feature order (ransac_pipeline.cpp:106-112)
    const int n = block_compact<R5_WAVES>([&](int i) { return !hybrid || ts[i] == 0; }, v.map, n_all, v.chunk);
    // hybrid: RANSAC2's outcome and the skip rule (ransac_pipeline.cpp:165-167)
    const int r2count = hybrid && n >= 2 ? a.r2_summary[2 * set] : 0;
    const bool use_r2 = hybrid && (double)r2count > a.skip5 * (double)n;
    const bool want5 = n >= 5 && !use_r2;
    // Every condition below is uniform over the workgroup -- n, m, r2count and the parameters are the same in all of its threads --
    // so the barriers inside the phases are met by every thread or by none.
    int m = 0;
    if (want5) m = normalise_set(v, c1, c2, n, tid);
    const bool run5 = want5 && m >= 5;
    const int H = m == 5 ? 1 : IT;
    R5Best b{0, -1, -1, 0};
    if (run5) {
        draw_subsets(v, m, H, tid);                             // 2
        const int rounds = (H + R5_WAVES - 1) / R5_WAVES;       // 3. the minimal solves, one hypothesis per wavefront
        for (int rb = 0; rb < rounds; ++rb) {                   // (every wavefront makes every round: an idle one has act = false)
            const int h = rb * R5_WAVES + wave;
            const bool act = h < H;
            double *rec = v.recs + (size_t)(act ? h : 0) * REC;
            null_basis(v, rec, h, act, lane);                   // 3a
            coeff_matrix(v, rec, act, lane);                    // 3b, 3c
            eliminate(v, h, act, lane);                         // 3d
            b_matrix(v, rec, act, lane);                        // 3e
            det_poly(v, rec, act, lane);                        // 3f
        }
        solve_poly(v, H, tid);                                  // 4
        if (m > 5) {                                            // m == 5 is count == modelPoints: no loop, the first model is taken
            score_models(v, H, m, a.thr2, tid);                 // 5
            b = registrator_runs(v, IT, m, a.prob, tid);        // 6
        }
        mask_and_E(v, b, n, m, a.thr2, a.E ? a.E + 9 * (size_t)set : nullptr, tid);
    } else {
        for (int k = tid; k < n; k += R5_THREADS) v.st[k] = 3;
        if (tid == 0 && a.E)
            for (int i = 0; i < 9; ++i) a.E[9 * (size_t)set + i] = 0.0;
    }
    const int r5count = count_inliers(v, run5, n, tid);
    if (tid == 0 && a.summary) {
        int *sm = a.summary + 4 * (size_t)set;
        sm[0] = run5 ? r5count : 0; sm[1] = run5 ? b.bh : -1; sm[2] = run5 ? b.iters : 0; sm[3] = m;
    }
    if (!hybrid) {
        int *st = a.status + (size_t)set * MP;
        for (int k = tid; k < n; k += R5_THREADS) st[k] = v.st[k];
        return;
    }
    hybrid_select(a, v, set, ts, n_all, n, r2count, r5count, use_r2, run5, tid);
}


// the host-side checks, made before the context is looked at: HV_ERR_INVALID for what OpenCV asserts on or what cannot be a set,
// HV_ERR_UNSUPPORTED for what the kernel's LDS plan does not cover
int check_params(const hv_ransac5_params *p, int max_points, int n_sets)
{
    if (!p || !(p->ransac5Prob > 0 && p->ransac5Prob < 1) || p->ransacMaxIters < 1 || max_points < 1 || n_sets < 0) return HV_ERR_INVALID;
    if (max_points > R5_MAX_PTS || p->ransacMaxIters > R5_MAX_ITERS || n_sets > 65535) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}

void fill_common(R5Args &a, const hv_ransac5_params *p, int max_points, const hv_camera_model *cam1, const hv_camera_model *cam2)
{
    a.max_points = max_points; a.max_iters = p->ransacMaxIters;
    a.cam1 = *cam1; a.cam2 = *cam2;
    const double f1 = (cam1->fx + cam1->fy) * 0.5, f2 = (cam2->fx + cam2->fy) * 0.5;    // Camera::getFocalLength
    const double thr = 2 * p->ransac5Threshold / (f1 + f2);                              // ransac_pipeline.cpp:330
    a.thr2 = (float)(thr * thr);
    a.prob = p->ransac5Prob; a.skip5 = p->ransac2InliersToSkipRansac5; a.min_frac = p->ransacMinInlierFraction;
    a.over5 = p->ransac2InliersOverRansac5Needed;
}

int launch(Ctx *c, int n_sets, const R5Args &a)
{
    const size_t bytes = ransac5_lds(a.max_points, a.max_iters).end;
    hipLaunchKernelGGL(ransac5_kernel, dim3((unsigned)n_sets), dim3(R5_THREADS), bytes, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

}  // namespace

int ransac5_init(Ctx *c)
{
    HV_HIP(c, set_lds_limit(ransac5_kernel, ransac5_lds(R5_MAX_PTS, R5_MAX_ITERS).end));
    return HV_OK;
}

}  // namespace hv

using hv::Ctx;

extern "C" {

void hv_ransac5_default_params(hv_ransac5_params *p)
{
    if (!p) return;
    p->ransac5Prob = 0.999;                       // codegen/parameter_definitions.c:280
    p->ransac5Threshold = 2.0;                    // :278
    p->ransacMaxIters = 75;                       // :270
    p->ransac2InliersToSkipRansac5 = 0.9;         // :272
    p->ransacMinInlierFraction = 0.3;             // :282
    p->ransac2InliersOverRansac5Needed = 0.9;     // :274
}

int hv_ransac5_batch_dev(hv_ctx *h, const hv_ransac5_params *p, int n_sets, int max_points, const int *n_points_dev,
                         const float *c1_dev, const float *c2_dev, const hv_camera_model *cam1, const hv_camera_model *cam2,
                         int *status_dev, double *E_dev, int *summary_dev)
{
    if (const int rc = hv::check_params(p, max_points, n_sets)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c || !cam1 || !cam2) return HV_ERR_INVALID;
    if (n_sets > 0 && (!n_points_dev || !c1_dev || !c2_dev || !status_dev)) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    hv::R5Args a{};
    hv::fill_common(a, p, max_points, cam1, cam2);
    a.n_points = n_points_dev; a.c1 = c1_dev; a.c2 = c2_dev; a.status = status_dev; a.E = E_dev; a.summary = summary_dev;
    hv::ScopedKernelTime tm(c, HV_K_RANSAC5);
    return hv::launch(c, n_sets, a);
}

int hv_hybrid_ransac_lk_batch_dev(hv_ctx *h, const hv_ransac5_params *p, int n_sets, int max_points, const int *n_points_dev,
                                  const float *c1_dev, const float *c2_dev, int *track_status_dev, const int *r2_status_dev,
                                  const int *r2_summary_dev, const hv_camera_model *cam1, const hv_camera_model *cam2,
                                  int *result_dev, double *score_dev, double *E_dev, int *r5_summary_dev)
{
    if (const int rc = hv::check_params(p, max_points, n_sets)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c || !cam1 || !cam2) return HV_ERR_INVALID;
    if (n_sets > 0 && (!n_points_dev || !c1_dev || !c2_dev || !track_status_dev || !r2_status_dev || !r2_summary_dev || !result_dev ||
                       !score_dev))
        return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    hv::R5Args a{};
    hv::fill_common(a, p, max_points, cam1, cam2);
    a.n_points = n_points_dev; a.c1 = c1_dev; a.c2 = c2_dev; a.track_status = track_status_dev; a.r2_status = r2_status_dev;
    a.r2_summary = r2_summary_dev; a.result = result_dev; a.score = score_dev; a.E = E_dev; a.summary = r5_summary_dev;
    hv::ScopedKernelTime tm(c, HV_K_RANSAC5);
    return hv::launch(c, n_sets, a);
}

int hv_ransac5(hv_ctx *h, const hv_ransac5_params *p, int n, const float *c1, const float *c2, const hv_camera_model *cam1,
               const hv_camera_model *cam2, int *status, double *E, int *summary)
{
    if (n < 0) return HV_ERR_INVALID;
    if (const int rc = hv::check_params(p, std::max(n, 1), 1)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c || (n > 0 && (!c1 || !c2 || !status)) || !cam1 || !cam2) return HV_ERR_INVALID;
    const int mp = std::max(n, 1);
    const bool any = n > 0;                                       // (n == 0: one-point sections, nothing of the caller's arrays read or written)
    hv::Stage s(c);
    const auto o_c1 = s.in(any ? c1 : nullptr, 2 * (size_t)mp), o_c2 = s.in(any ? c2 : nullptr, 2 * (size_t)mp);
    const auto o_n = s.in(&n, 1);
    const auto o_st = s.out(any ? status : nullptr, mp), o_sum = s.out(summary, 4);
    const auto o_E = s.out(E, 9);
    int rc = s.upload();
    if (rc != HV_OK) return rc;
    rc = hv_ransac5_batch_dev(h, p, 1, mp, s.at(o_n), s.at(o_c1), s.at(o_c2), cam1, cam2, s.at(o_st), s.at(o_E), s.at(o_sum));
    return rc != HV_OK ? rc : s.download();
}

}  // extern "C"
