// Sub-pixel corner refinement: cv::cornerSubPix + SubPixelAdjuster::adjust's revert rule on level 0 of a pyramid slot.
//
// Replaces tracker::SubPixelAdjuster (src/tracker/subpixel_adjuster.cpp:18-42), which the reference runs on every newly
// detected corner with its default parameters (tracker.subPixMaxIter 20 > 0: image.cpp:54, 81-84). The arithmetic is
// OpenCV 4.x imgproc/src/cornersubpix.cpp (cv::cornerSubPix) with the two samplers of imgproc/src/samplers.cpp that
// getRectSubPix(u8 -> CV_32F) takes: getRectSubPix_8u32f where the patch and its lower/right neighbour row/column lie inside
// the image, getRectSubPix_Cn_ + adjustRect (replicated border rows and columns) otherwise. Every float and double
// operation is kept in OpenCV's order and width (-ffp-contract=off is global), so the results are bit-identical to the
// numpy restatement in tests/subpix_restatement.py, which cites the upstream steps one by one.
//
// Design for CDNA4: one 64-lane wavefront (one workgroup) per corner; the iteration loop is uniform across the wave.
//   1. the (W+2)^2 patch (23^2 at window 10): every sample is independent (the 8u32f sampler's running `prev` is the
//      previous column's t times s, recomputed from two more byte loads), spread over the 64 lanes, into LDS;
//   2. the W^2 per-term products (441 at window 10: tgx, tgy in binary32, gxx, gxy, gyy and the two bb terms in f64), again
//      one term per lane and step, into LDS as five rows of doubles;
//   3. the five accumulations a, b, c, bb1, bb2 are serial f64 chains in OpenCV's row-major order: lane l < 5 walks row l
//      (16-byte LDS reads one pair ahead of the adds), so the five chains overlap and the order is the reference's;
//   4. every lane reads the five sums and solves the 2x2 system redundantly (uniform control flow, no broadcast needed).
// The Gaussian weights exp(-t^2) are formed on the host with the platform expf, as OpenCV does, and travel in the kernel
// arguments; the device forms mask[i][j] = g[i] * g[j] with the same single binary32 product.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "hv_internal.hpp"

namespace hv {

namespace {

constexpr int SUBPIX_MAX_WW = 2 * HV_SUBPIX_MAX_WIN + 1;

struct SubpixArgs {
    const uint8_t *const *l0_ptr;     // per-slot level-0 image table (filled by the pyramid build)
    const int *l0_stride;
    const int *slots;                 // [n_sets], or null: the single set on slot0
    int slot0, pool_size;
    const int *n_points;              // [n_sets], or null: n0 points
    int n0, max_points;
    int w, h, win, max_iters;
    double eps;                       // squared
    float *xy;                        // [n_sets][max_points][2], in place
    int *iters;                       // [n_sets][max_points] or null
    float g[SUBPIX_MAX_WW];           // exp(-t^2), t = (float)(i - win) / win (cornersubpix.cpp mask loop)
};

// terms of one corner: five rows of KS doubles (KS = W^2 rounded up to even: 16-byte aligned rows), then the patch
__host__ __device__ inline int subpix_ks(int ww) { return (ww * ww + 1) & ~1; }
inline size_t subpix_lds_bytes(int win)
{
    const int ww = 2 * win + 1, pw = ww + 2;
    return sizeof(double) * 5 * subpix_ks(ww) + sizeof(float) * pw * pw;
}

__global__ __launch_bounds__(64) void subpix_kernel(SubpixArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double sp_lds[];
    __shared__ double sums[5];
    const int t = threadIdx.x, set = blockIdx.y, pt = blockIdx.x;
    const int n = a.n_points ? min(a.n_points[set], a.max_points) : a.n0;
    if (pt >= n) return;
    const int slot = a.slots ? a.slots[set] : a.slot0;
    if (slot < 0 || slot >= a.pool_size) return;                      // not a slot: the set is left untouched
    const size_t rec = (size_t)set * a.max_points + pt;
    float *xy = a.xy + 2 * rec;
    const float tx = xy[0], ty = xy[1];
    const int w = a.w, h = a.h;
    // OpenCV asserts Rect(0, 0, cols, rows).contains(cT): such an input (NaN included) comes back as it went in
    const bool inside = tx >= 0.f && tx < (float)w && ty >= 0.f && ty < (float)h;
    int updates = 0;
    float cx = tx, cy = ty;
    if (inside) {
        const uint8_t *src = a.l0_ptr[slot];
        const int st = a.l0_stride[slot];
        const int win = a.win, ww = 2 * win + 1, pw = ww + 2, nt = ww * ww, ks = subpix_ks(ww);
        double *T = sp_lds;
        float *P = reinterpret_cast<float *>(sp_lds + 5 * ks);
        auto px_at = [&](int r, int c) -> float {                     // clamped: a read never leaves the image
            r = min(max(r, 0), h - 1); c = min(max(c, 0), w - 1);
            return (float)src[(size_t)r * st + c];
        };
        int iter = 0;
        for (;;) {
            // ---- getRectSubPix(src, Size(pw, pw), cI, patch, CV_32F) ----
            const float hx = cx - (float)(pw - 1) * 0.5f, hy = cy - (float)(pw - 1) * 0.5f;
            const int ipx = (int)floorf(hx), ipy = (int)floorf(hy);
            if (0 <= ipx && ipx + pw < w && 0 <= ipy && ipy + pw < h) {
                // getRectSubPix_8u32f: dst[j] = prev + t_j, prev = (1 - a)(b1 s0 + b2 s1) at j = 0, else (float)(t_{j-1} * s)
                float fa = hx - (float)ipx;
                const float fb = hy - (float)ipy;
                fa = fa < 0.0001f ? 0.0001f : fa;
                const float a12 = fa * (1.f - fb), a22 = fa * fb, b1 = 1.f - fb, b2 = fb, oma = 1.f - fa;
                const double s = (1. - (double)fa) / (double)fa;
                for (int e = t; e < pw * pw; e += 64) {
                    const int r = e / pw, j = e - r * pw;
                    const uint8_t *r0 = src + (size_t)(ipy + r) * st + ipx, *r1 = r0 + st;
                    const float tj = a12 * (float)r0[j + 1] + a22 * (float)r1[j + 1];
                    float prev;
                    if (j == 0) {
                        prev = oma * (b1 * (float)r0[0] + b2 * (float)r1[0]);
                    } else {
                        const float tp = a12 * (float)r0[j] + a22 * (float)r1[j];
                        prev = (float)((double)tp * s);
                    }
                    P[e] = prev + tj;
                }
            } else {
                // getRectSubPix_Cn_<uchar, float, float> outside branch with adjustRect's rectangle
                const float fa = hx - (float)ipx, fb = hy - (float)ipy;
                const float a11 = (1.f - fa) * (1.f - fb), a12 = fa * (1.f - fb), a21 = (1.f - fa) * fb, a22 = fa * fb;
                const float b1 = 1.f - fb, b2 = fb;
                int col0, rx, rw, row0, ry, rh;
                if (ipx >= 0) { col0 = ipx; rx = 0; } else { rx = min(-ipx, pw); col0 = 0; }
                if (ipx < w - pw) rw = pw; else { rw = w - ipx - 1; if (rw < 0) { col0 += rw; rw = 0; } }
                col0 -= rx;
                if (ipy >= 0) { row0 = ipy; ry = 0; } else { ry = -ipy; row0 = 0; }
                if (ipy < h - pw) rh = pw; else { rh = h - ipy - 1; if (rh < 0) { row0 += rh; rh = 0; } }
                for (int e = t; e < pw * pw; e += 64) {
                    const int i = e / pw, j = e - i * pw;
                    const int rt = row0 + max(0, min(i, rh) - ry);            // row pair of patch row i
                    const int rb = rt + ((i >= ry && i < rh) ? 1 : 0);
                    float v;
                    if (j >= rw || j < rx) {                                  // right border wins where the two overlap
                        const int c = col0 + (j >= rw ? rw : rx);
                        v = px_at(rt, c) * b1 + px_at(rb, c) * b2;
                    } else {
                        const int c = col0 + j;
                        v = ((px_at(rt, c) * a11 + px_at(rt, c + 1) * a12) + px_at(rb, c) * a21) + px_at(rb, c + 1) * a22;
                    }
                    P[e] = v;
                }
            }
            __syncthreads();
            // ---- per-term products (cornersubpix.cpp "process gradient" loop body) ----
            for (int k = t; k < nt; k += 64) {
                const int i = k / ww, j = k - i * ww;
                const float *q = P + (i + 1) * pw + (j + 1);
                const double m = (double)(a.g[i] * a.g[j]);
                const double tgx = (double)(q[1] - q[-1]), tgy = (double)(q[pw] - q[-pw]);
                const double gxx = tgx * tgx * m, gxy = tgx * tgy * m, gyy = tgy * tgy * m;
                const double px = (double)(j - win), py = (double)(i - win);
                T[k] = gxx;
                T[ks + k] = gxy;
                T[2 * ks + k] = gyy;
                T[3 * ks + k] = gxx * px + gxy * py;
                T[4 * ks + k] = gxy * px + gyy * py;
            }
            __syncthreads();
            // ---- the five serial sums, one lane each, in row-major term order ----
            if (t < 5) {
                const double2 *q2 = reinterpret_cast<const double2 *>(T + t * ks);
                double acc = 0.0;
                double2 v = q2[0];
                int p2 = 0;
                while (2 * p2 + 2 < nt) {
                    const double2 nv = q2[p2 + 1];
                    acc += v.x;
                    acc += v.y;
                    v = nv;
                    ++p2;
                }
                acc += v.x;
                if (2 * p2 + 1 < nt) acc += v.y;
                sums[t] = acc;
            }
            __syncthreads();
            const double sa = sums[0], sb = sums[1], sc = sums[2], bb1 = sums[3], bb2 = sums[4];
            const double det = sa * sc - sb * sb;
            if (fabs(det) <= DBL_EPSILON * DBL_EPSILON) break;
            const double scale = 1.0 / det;
            const float x2 = (float)((double)cx + sc * scale * bb1 - sb * scale * bb2);
            const float y2 = (float)((double)cy - sb * scale * bb1 + sa * scale * bb2);
            const float err = (x2 - cx) * (x2 - cx) + (y2 - cy) * (y2 - cy);
            cx = x2; cy = y2;
            ++updates;
            if (cx < 0.f || cx >= (float)w || cy < 0.f || cy >= (float)h) break;
            if (!(++iter < a.max_iters && (double)err > a.eps)) break;
        }
        // cornerSubPix: too far from the start -> the start; adjust: outside the image -> the input (the same point)
        if (fabsf(cx - tx) > (float)win || fabsf(cy - ty) > (float)win) { cx = tx; cy = ty; }
        if (cx < 0.f || cx >= (float)w || cy < 0.f || cy >= (float)h) { cx = tx; cy = ty; }
    }
    if (t == 0) {
        xy[0] = cx; xy[1] = cy;
        if (a.iters) a.iters[rec] = updates;
    }
}

int check_params(Ctx *c, const hv_subpix_params *p)
{
    const int win = p->subPixWindowSize;
    if (win < 1) return HV_ERR_INVALID;
    if (win > HV_SUBPIX_MAX_WIN) return HV_ERR_UNSUPPORTED;
    if (c->L.w[0] < 2 * win + 5 || c->L.h[0] < 2 * win + 5) return HV_ERR_INVALID;
    return HV_OK;
}

int launch(Ctx *c, const hv_subpix_params *p, int n_sets, const int *slots_dev, int slot0, int max_points,
           const int *n_points_dev, int n0, float *xy, int *iters)
{
    SubpixArgs a{};
    a.l0_ptr = c->d_l0_ptr; a.l0_stride = c->d_l0_stride;
    a.slots = slots_dev; a.slot0 = slot0; a.pool_size = c->p.pool_size;
    a.n_points = n_points_dev; a.n0 = n0; a.max_points = max_points;
    a.w = c->L.w[0]; a.h = c->L.h[0];
    a.win = p->subPixWindowSize;
    a.max_iters = std::min(std::max(p->subPixMaxIter, 1), 100);       // cornersubpix.cpp: MIN(MAX(maxCount, 1), MAX_ITERS)
    const double e = std::max(p->subPixEpsilon, 0.);
    a.eps = e * e;
    a.xy = xy; a.iters = iters;
    for (int i = 0; i < 2 * a.win + 1; ++i) {
        const float y = (float)(i - a.win) / a.win;
        a.g[i] = std::exp(-y * y);                                      // std::exp(float), as OpenCV
    }
    ScopedKernelTime tm(c, HV_K_SUBPIX);
    hipLaunchKernelGGL(subpix_kernel, dim3((unsigned)max_points, (unsigned)n_sets), dim3(64), subpix_lds_bytes(a.win), c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

}  // namespace

}  // namespace hv

using hv::Ctx;

extern "C" {

void hv_subpix_default_params(hv_subpix_params *p)
{
    if (!p) return;
    p->subPixWindowSize = 10; p->subPixMaxIter = 20; p->subPixEpsilon = 0.03;   // parameter_definitions.c:328-332
}

int hv_corner_subpix(hv_ctx *ctx, const hv_subpix_params *p, int slot, int n, float *xy, int *iters)
{
    if (!ctx || !p || n < 0 || (n > 0 && !xy)) return HV_ERR_INVALID;
    Ctx *c = hv::ctx_of(ctx);
    if (slot < 0 || slot >= c->p.pool_size || !c->slot_used[slot]) return HV_ERR_POOL;
    int rc = hv::check_params(c, p);
    if (rc != HV_OK) return rc;
    if (n == 0) return HV_OK;
    hv::Stage s(c);
    const auto o_xy = s.inout(xy, 2 * (size_t)n);
    const auto o_it = s.out(iters, n);
    rc = s.upload();
    if (rc != HV_OK) return rc;
    rc = hv::launch(c, p, 1, nullptr, slot, n, nullptr, n, s.at(o_xy), s.at(o_it));
    return rc != HV_OK ? rc : s.download();
}

int hv_corner_subpix_batch_dev(hv_ctx *ctx, const hv_subpix_params *p, int n_sets, const int *slots_dev, int max_points,
                               const int *n_points_dev, float *xy_dev, int *iters_dev)
{
    if (!ctx || !p || n_sets < 0 || max_points < 0) return HV_ERR_INVALID;
    if (n_sets > 65535) return HV_ERR_UNSUPPORTED;                      // grid y
    if (n_sets > 0 && max_points > 0 && (!slots_dev || !n_points_dev || !xy_dev)) return HV_ERR_INVALID;
    Ctx *c = hv::ctx_of(ctx);
    const int rc = hv::check_params(c, p);
    if (rc != HV_OK) return rc;
    if (n_sets == 0 || max_points == 0) return HV_OK;
    return hv::launch(c, p, n_sets, slots_dev, 0, max_points, n_points_dev, 0, xy_dev, iters_dev);
}

}  // extern "C"
