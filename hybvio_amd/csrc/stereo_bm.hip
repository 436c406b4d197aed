// Dense stereo depth (tracker.computeDenseStereoDepth): cv::StereoBM block matching with the speckle filter, the per-track depth
// lookup and the strided point cloud, batched, no allocation and no synchronisation (capturable in a HIP graph).
//
// Reference: src/tracker/tracker.cpp:532 and :784-796 (computeDenseStereoDepth), src/tracker/image.cpp:108-139, and all of
// src/tracker/stereo_disparity.cpp (cv::StereoBM::create(nd), speckle window 500 and range 10; getDepth :66-77; computePointCloud
// :79-94). The rules are restated in tests/stereo_bm_restatement.py, written from the algorithm and NOT pinned against an OpenCV
// build; everything up to the disparity image is integer arithmetic.
//
// Launches of hv_stereo_disparity_batch_dev (HV_K_INGEST):
//   bm_prefilter_kernel   a thread per pixel of both images of a set: the XSOBEL prefilter into two byte planes of the work memory,
//       and FILTERED into the whole disparity image (the matching kernel then writes the valid rectangle).
//   bm_match_kernel       one workgroup per strip of BM_TX columns and band of BM_ROWS rows of the valid rectangle. NO cost volume
//       in global memory: the 21 x 21 window sums sad[d][x] of the strip's current row live in LDS as 16-bit values (nd + 1 planes
//       of BM_TX columns: plane nd is the texture sum), and move down one row per step: a work item (plane d, segment of BM_SEG
//       columns) slides the 21-wide sums of |L' - R'| of the row that enters and of the row that leaves along its segment and adds
//       their difference. Then a thread per column reads its sad vector (conflict-free: consecutive lanes, consecutive halfwords)
//       twice: minimum with OpenCV's tie order, then the uniqueness test; sub-pixel step; one int16 store. A band starts with 21
//       steps that only add. 441 * 126 < 65536, so 16 bits hold every sum, and additions that wrap on the way still end right.
//   speckle filter (hv_filter_speckles_batch_dev on its own): union-find over int32 labels, label[i] <= i always.
//       spk_local_kernel   a 64 x 16 tile in LDS: every pixel joins its left and upper neighbour inside the tile (atomicMin on the
//                          roots), then writes the global index of its root (or -1) and zeroes its counter;
//       spk_seam_kernel    pixels of a tile's first column / first row join across the seam, atomicMin in global memory;
//       spk_count_kernel   find, path compression (label[i] = root), one count per root (a wavefront whose pixels share a root
//                          adds once);
//       spk_apply_kernel   components of <= max_size pixels become new_val.
//   bm_count_kernel       n_valid per set (or -1 for a set without an image), one workgroup per set.
// Every loop is bounded by construction: a find only ever moves to a smaller label (it stops at the first label that is not
// smaller than its index, whatever it reads), a union either ends or continues from a strictly smaller root, nothing waits for
// another workgroup, nothing spins.
// Depth and cloud (HV_K_STEREO_GATE): a thread per track / one workgroup per set with a prefix sum for the cloud's order; binary32
// with IEEE division, uncontracted sums and the correctly rounded square root of hv_sqrt_rn.hpp.
#include "hv_internal.hpp"
#include "hv_sqrt_rn.hpp"

#include <algorithm>
#include <cmath>

namespace hv {
namespace {

constexpr int FILTERED = -16;                      // (minDisparity - 1) << 4
constexpr int BM_BLOCK = 21, BM_W2 = BM_BLOCK / 2;
constexpr int BM_THREADS = 256;
constexpr int BM_TX = 256;                         // columns of a strip: one per thread of the decision phase
constexpr int BM_SEG = 16;                         // columns a work item slides along
constexpr int BM_NSEG = BM_TX / BM_SEG;
constexpr int BM_ROWS = 64;                        // output rows of a band (it runs BM_ROWS + 20 steps)
constexpr int BM_PITCH = BM_TX + 2;                // halfwords per plane: 129 dwords, so planes d, d + 1, .. fall on different banks
constexpr int BM_LW = BM_TX + 2 * BM_W2;           // staged columns of a left row: x0 - 10 .. x0 + BM_TX + 9
constexpr int BM_MAX_ND = 256;
constexpr int SPK_TW = 64, SPK_TH = 16;            // the labelling tile
static_assert(BM_TX == BM_THREADS && BM_TX % BM_SEG == 0 && (BM_PITCH / 2) % 2 == 1, "one decision thread per column; odd dword pitch");

struct BmArgs {
    const uint8_t *const *l0_ptr;     // per-slot level-0 image table
    const int *l0_stride;
    const int *left_slots, *right_slots;   // [n_sets], or null: slot0 / slot1
    int slot0, slot1, pool_size;
    int w, h, nd, cap, texture_threshold, uniqueness_ratio;
    int ps;                           // bytes per row of a prefiltered plane
    unsigned char *work; size_t work_stride;    // per set: left plane, right plane, labels, counters
    size_t label_off;                 // of the labels in a set's work memory; the counters follow
    int16_t *disp; long long disp_stride;
    int *n_valid;
    int x0v, x1v, y0v, y1v, strips, bands;
};

__device__ __forceinline__ bool set_images(const BmArgs &a, int set, const uint8_t **l, int *ls, const uint8_t **r, int *rs)
{
    const int sl = a.left_slots ? a.left_slots[set] : a.slot0, sr = a.right_slots ? a.right_slots[set] : a.slot1;
    if (sl < 0 || sl >= a.pool_size || sr < 0 || sr >= a.pool_size) return false;
    *l = a.l0_ptr[sl]; *ls = a.l0_stride[sl];
    *r = a.l0_ptr[sr]; *rs = a.l0_stride[sr];
    return *l != nullptr && *r != nullptr;
}

// ---- prefilter -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bm_prefilter_kernel(BmArgs a)
{
    const int set = blockIdx.y >> 1, cam = blockIdx.y & 1;
    const uint8_t *img[2]; int stride[2];
    if (!set_images(a, set, &img[0], &stride[0], &img[1], &stride[1])) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)a.w * a.h) return;
    const int y = (int)(i / a.w), x = (int)(i - (long long)y * a.w);
    const uint8_t *src = cam ? img[1] : img[0];
    const int st = cam ? stride[1] : stride[0];
    int v = a.cap;
    if (x > 0 && x < a.w - 1 && a.h >= 2 && !((a.h & 1) && y == a.h - 1)) {
        const int yu = y == 0 ? 1 : y - 1, yd = y == a.h - 1 ? a.h - 2 : y + 1;
        const uint8_t *r0 = src + (size_t)yu * st + x, *r1 = src + (size_t)y * st + x, *r2 = src + (size_t)yd * st + x;
        const int s = ((int)r0[1] - (int)r0[-1]) + 2 * ((int)r1[1] - (int)r1[-1]) + ((int)r2[1] - (int)r2[-1]);
        v = min(max(s, -a.cap), a.cap) + a.cap;
    }
    unsigned char *plane = a.work + (size_t)set * a.work_stride + (size_t)cam * a.ps * a.h;
    plane[(size_t)y * a.ps + x] = (unsigned char)v;
    if (cam == 0) a.disp[(long long)set * a.disp_stride + i] = (int16_t)FILTERED;
}

// ---- block matching ------------------------------------------------------------------------------------------------------------
// |L'(c) - R'(c - d)| of a staged row pair; plane nd: |L'(c) - cap|. lrow[c] is column xs0 - 10 + c, rrow[c] column xs0 - 10 - (nd - 1) + c.
__device__ __forceinline__ int bm_ad(const uint8_t *lrow, const uint8_t *rrow, int c, int roff, bool tex, int cap)
{
    const int l = lrow[c], r = tex ? cap : (int)rrow[c + roff];
    return abs(l - r);
}

__global__ __launch_bounds__(BM_THREADS) void bm_match_kernel(BmArgs a)
{
    extern __shared__ __align__(16) unsigned char bm_lds[];
    const int nd = a.nd, rw = BM_LW + nd - 1;                       // staged columns of a right row
    const int rwp = (rw + 3) & ~3;
    uint16_t *sad = reinterpret_cast<uint16_t *>(bm_lds);            // [nd + 1][BM_PITCH]
    uint8_t *lrow = bm_lds + (size_t)(nd + 1) * BM_PITCH * 2;        // [2][BM_LW]: the row that enters, the row that leaves
    uint8_t *rrow = lrow + 2 * BM_LW;                                // [2][rwp]
    const int t = threadIdx.x;
    const int per_set = a.strips * a.bands;
    const int set = blockIdx.x / per_set, rest = blockIdx.x - set * per_set;
    const int band = rest / a.strips, strip = rest - band * a.strips;
    const uint8_t *il, *ir; int sl, sr;
    if (!set_images(a, set, &il, &sl, &ir, &sr)) return;
    const unsigned char *lp = a.work + (size_t)set * a.work_stride, *rp = lp + (size_t)a.ps * a.h;
    const int xs0 = a.x0v + strip * BM_TX;                           // first output column of the strip
    const int yb0 = a.y0v + band * BM_ROWS, yb1 = min(yb0 + BM_ROWS, a.y1v);
    int16_t *disp = a.disp + (long long)set * a.disp_stride;

    for (int e = t; e < (nd + 1) * BM_PITCH; e += BM_THREADS) sad[e] = 0;
    const int items = (nd + 1) * BM_NSEG;
    const int first = yb0 - BM_W2, last = yb1 - 1 + BM_W2;          // rows that enter; all inside the image
    for (int r = first; r <= last; ++r) {
        const int ro = r - BM_BLOCK;                                 // the row that leaves
        const bool has_old = ro >= first;
        __syncthreads();                                             // the decision phase of the step before has read sad
        // ---- stage the two row pairs; columns outside the image read 0 (only columns right of the valid rectangle see them)
        for (int e = t; e < 2 * BM_LW; e += BM_THREADS) {
            const int k = e / BM_LW, c = e - k * BM_LW, x = xs0 - BM_W2 + c, y = k ? ro : r;
            lrow[e] = (x >= 0 && x < a.w && (k == 0 || has_old)) ? lp[(size_t)y * a.ps + x] : 0;
        }
        for (int e = t; e < 2 * rw; e += BM_THREADS) {
            const int k = e / rw, c = e - k * rw, x = xs0 - BM_W2 - (nd - 1) + c, y = k ? ro : r;
            rrow[k * rwp + c] = (x >= 0 && x < a.w && (k == 0 || has_old)) ? rp[(size_t)y * a.ps + x] : 0;
        }
        __syncthreads();
        // ---- move the window sums down one row
        for (int it = t; it < items; it += BM_THREADS) {
            const int seg = it / (nd + 1), d = it - seg * (nd + 1);
            const bool tex = d == nd;
            const int roff = nd - 1 - d, c0 = seg * BM_SEG;          // window of output column c0 + j: staged columns c0 + j .. c0 + j + 20
            uint16_t *row = sad + d * BM_PITCH + c0;
            int in = 0, out = 0;
            for (int i = 0; i < BM_BLOCK - 1; ++i) in += bm_ad(lrow, rrow, c0 + i, roff, tex, a.cap);
            if (has_old)
                for (int i = 0; i < BM_BLOCK - 1; ++i) out += bm_ad(lrow + BM_LW, rrow + rwp, c0 + i, roff, tex, a.cap);
#pragma unroll 4
            for (int j = 0; j < BM_SEG; ++j) {
                in += bm_ad(lrow, rrow, c0 + j + BM_BLOCK - 1, roff, tex, a.cap);
                if (has_old) out += bm_ad(lrow + BM_LW, rrow + rwp, c0 + j + BM_BLOCK - 1, roff, tex, a.cap);
                row[j] = (uint16_t)(row[j] + in - out);
                in -= bm_ad(lrow, rrow, c0 + j, roff, tex, a.cap);
                if (has_old) out -= bm_ad(lrow + BM_LW, rrow + rwp, c0 + j, roff, tex, a.cap);
            }
        }
        const int y = r - BM_W2;
        if (y < yb0) continue;                                       // (uniform: the window is not whole yet)
        __syncthreads();
        // ---- the decision of one pixel per thread
        const int x = xs0 + t;
        if (x >= a.x1v) continue;
        const uint16_t *col = sad + t;
        int value = FILTERED;
        if ((int)col[nd * BM_PITCH] >= a.texture_threshold) {
            int m = 0x7fffffff, mink = 0;
            for (int k = 0; k < nd; ++k) {                           // OpenCV's index k = nd - 1 - d: the first strictly smallest
                const int v = col[(nd - 1 - k) * BM_PITCH];
                if (v < m) { m = v; mink = k; }
            }
            const int thresh = m + m * a.uniqueness_ratio / 100;
            bool rival = false;
            for (int k = 0; k < nd; ++k) {
                const int v = col[(nd - 1 - k) * BM_PITCH];
                rival |= (k < mink - 1 || k > mink + 1) && v <= thresh;
            }
            if (!rival) {
                const int kp = mink + 1 >= nd ? nd - 2 : mink + 1, kn = mink - 1 < 0 ? 1 : mink - 1;
                const int p = col[(nd - 1 - kp) * BM_PITCH], n = col[(nd - 1 - kn) * BM_PITCH];
                const int dd = p + n - 2 * m + abs(p - n);
                value = ((nd - mink - 1) * 256 + (dd != 0 ? (p - n) * 256 / dd : 0) + 15) >> 4;
            }
        }
        disp[(long long)y * a.w + x] = (int16_t)value;
    }
}

// ---- speckles ------------------------------------------------------------------------------------------------------------------
struct SpkArgs {
    int w, h, tiles_x, tiles_y;
    int16_t *disp; long long disp_stride;
    int new_val, max_size, max_diff;
    unsigned char *work; size_t work_stride, label_off;     // labels int32 [h * w] at label_off of a set's work memory, then the counters
    // the sets a disparity call skips (null: none)
    const uint8_t *const *l0_ptr; const int *left_slots, *right_slots; int slot0, slot1, pool_size; bool check_slots;
};

__device__ __forceinline__ bool spk_set_ok(const SpkArgs &a, int set)
{
    if (!a.check_slots) return true;
    const int sl = a.left_slots ? a.left_slots[set] : a.slot0, sr = a.right_slots ? a.right_slots[set] : a.slot1;
    if (sl < 0 || sl >= a.pool_size || sr < 0 || sr >= a.pool_size) return false;
    return a.l0_ptr[sl] != nullptr && a.l0_ptr[sr] != nullptr;
}
__device__ __forceinline__ int *spk_labels(const SpkArgs &a, int set) { return reinterpret_cast<int *>(a.work + (size_t)set * a.work_stride + a.label_off); }
__device__ __forceinline__ int *spk_counts(const SpkArgs &a, int set) { return spk_labels(a, set) + (size_t)a.w * a.h; }

__device__ __forceinline__ int uf_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// label[i] <= i is the invariant; the walk moves only to a strictly smaller index, so it ends within i steps whatever it reads
__device__ __forceinline__ int uf_find(const int *lab, int i)
{
    int p;
    while ((p = uf_load(lab + i)) < i && p >= 0) i = p;
    return i;
}
// joins the sets of a and b. Each round either ends (equal roots, or this thread's atomicMin hung root a below b) or goes on from
// the label the atomic returned, which is strictly smaller than a: at most a rounds. When another thread had hung a below `old`
// first and this atomicMin replaced that link by b, the round that follows joins old and b, so no link is lost.
__device__ __forceinline__ void uf_union(int *lab, int a, int b)
{
    while (true) {
        a = uf_find(lab, a); b = uf_find(lab, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(lab + a, b);
        if (old >= a) return;
        a = old;
    }
}

__device__ __forceinline__ bool spk_joined(int va, int vb, int new_val, int max_diff) { return va != new_val && vb != new_val && abs(va - vb) <= max_diff; }

__global__ __launch_bounds__(256) void spk_local_kernel(SpkArgs a)
{
    __shared__ int lab[SPK_TW * SPK_TH];
    __shared__ short val[SPK_TW * SPK_TH];
    const int set = blockIdx.y;
    if (!spk_set_ok(a, set)) return;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int x0 = tx * SPK_TW, y0 = ty * SPK_TH, t = threadIdx.x;
    const int16_t *disp = a.disp + (long long)set * a.disp_stride;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int li = t + 256 * k, lx = li % SPK_TW, ly = li / SPK_TW, x = x0 + lx, y = y0 + ly;
        val[li] = (x < a.w && y < a.h) ? disp[(long long)y * a.w + x] : (short)a.new_val;
        lab[li] = li;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int li = t + 256 * k, lx = li % SPK_TW, ly = li / SPK_TW;
        const int v = val[li];
        if (lx > 0 && spk_joined(v, val[li - 1], a.new_val, a.max_diff)) uf_union(lab, li, li - 1);
        if (ly > 0 && spk_joined(v, val[li - SPK_TW], a.new_val, a.max_diff)) uf_union(lab, li, li - SPK_TW);
    }
    __syncthreads();
    int *labels = spk_labels(a, set), *counts = spk_counts(a, set);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int li = t + 256 * k, lx = li % SPK_TW, ly = li / SPK_TW, x = x0 + lx, y = y0 + ly;
        if (x >= a.w || y >= a.h) continue;
        const int r = uf_find(lab, li);                              // row-major order in the tile is row-major order in the image
        const int g = y * a.w + x;
        labels[g] = val[li] != a.new_val ? (y0 + r / SPK_TW) * a.w + x0 + r % SPK_TW : -1;
        counts[g] = 0;
    }
}

__global__ __launch_bounds__(256) void spk_seam_kernel(SpkArgs a)
{
    const int set = blockIdx.y;
    if (!spk_set_ok(a, set)) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)a.w * a.h) return;
    const int y = (int)(i / a.w), x = (int)(i - (long long)y * a.w);
    const bool sx = x > 0 && x % SPK_TW == 0, sy = y > 0 && y % SPK_TH == 0;
    if (!sx && !sy) return;
    const int16_t *disp = a.disp + (long long)set * a.disp_stride;
    int *labels = spk_labels(a, set);
    const int v = disp[i];
    if (sx && spk_joined(v, disp[i - 1], a.new_val, a.max_diff)) uf_union(labels, (int)i, (int)i - 1);
    if (sy && spk_joined(v, disp[i - a.w], a.new_val, a.max_diff)) uf_union(labels, (int)i, (int)i - a.w);
}

__global__ __launch_bounds__(256) void spk_count_kernel(SpkArgs a)
{
    const int set = blockIdx.y;
    if (!spk_set_ok(a, set)) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int *labels = spk_labels(a, set), *counts = spk_counts(a, set);
    int root = -1;
    if (i < (long long)a.w * a.h && labels[i] >= 0) {
        root = uf_find(labels, (int)i);
        labels[i] = root;                                            // (a racing walk through i reads the old link or the root: both lead there)
    }
    // a wavefront inside one component adds once
    const int lead = __builtin_amdgcn_readfirstlane(root);
    const unsigned long long same = __ballot(root == lead && root >= 0);
    if (root >= 0) {
        if (root != lead) atomicAdd(counts + root, 1);
        else if ((int)(threadIdx.x & 63) == __ffsll((long long)same) - 1) atomicAdd(counts + root, __popcll(same));
    }
}

__global__ __launch_bounds__(256) void spk_apply_kernel(SpkArgs a)
{
    const int set = blockIdx.y;
    if (!spk_set_ok(a, set)) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)a.w * a.h) return;
    const int *labels = spk_labels(a, set), *counts = spk_counts(a, set);
    const int r = labels[i];
    if (r >= 0 && counts[r] <= a.max_size) a.disp[(long long)set * a.disp_stride + i] = (int16_t)a.new_val;
}

__global__ __launch_bounds__(1024) void bm_count_kernel(BmArgs a)
{
    __shared__ int part[16];
    const int set = blockIdx.x, t = threadIdx.x;
    const uint8_t *il, *ir; int sl, sr;
    if (!set_images(a, set, &il, &sl, &ir, &sr)) { if (t == 0) a.n_valid[set] = -1; return; }
    const int16_t *disp = a.disp + (long long)set * a.disp_stride;
    int n = 0;
    for (long long i = t; i < (long long)a.w * a.h; i += 1024) n += disp[i] != FILTERED;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
    if ((t & 63) == 0) part[t >> 6] = n;
    __syncthreads();
    if (t == 0) { int s = 0; for (int k = 0; k < 16; ++k) s += part[k]; a.n_valid[set] = s; }
}

// ---- depth and cloud -----------------------------------------------------------------------------------------------------------
struct DepthArgs {
    int w, h;
    const int16_t *disp; long long disp_stride;
    float q[16];                                                     // Q.cast<float>()
    int max_points; const int *n_points; const float *xy; float *depth;          // tracks
    int cloud_stride, gx, gy; float *xyz; int *n_out;                            // cloud
};

// val of a disparity value, or a negative number where the reference returns / skips
__device__ __forceinline__ float disparity_value(int v)
{
    const float val = (float)v / 16.0f;
    return (val <= 0.f || val < 1.0f) ? -1.f : val;
}
// (Qf . (x, y, val, 1)).hnormalized(): every row summed left to right, IEEE division (the build has contraction off)
__device__ __forceinline__ void reproject(const float (&q)[16], int x, int y, float val, float (&pos)[3])
{
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = ((q[4 * r] * (float)x + q[4 * r + 1] * (float)y) + q[4 * r + 2] * val) + q[4 * r + 3] * 1.0f;
#pragma unroll
    for (int r = 0; r < 3; ++r) pos[r] = v[r] / v[3];
}
__device__ __forceinline__ float squared_norm(const float (&p)[3]) { return (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]; }

__global__ __launch_bounds__(256) void stereo_track_depth_kernel(DepthArgs a)
{
    const int set = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = min(max(a.n_points[set], 0), a.max_points);
    if (i >= n) return;
    const float px = a.xy[((size_t)set * a.max_points + i) * 2], py = a.xy[((size_t)set * a.max_points + i) * 2 + 1];
    float depth = -1.f;
    // a non-finite coordinate or one beyond int range has no (int) value: -1 (NaN fails both comparisons)
    if (fabsf(px) < 2147483648.f && fabsf(py) < 2147483648.f) {
        const int x = (int)px, y = (int)py;                          // toward zero
        if (x >= 0 && y >= 0 && x < a.w && y < a.h) {
            const float val = disparity_value(a.disp[(long long)set * a.disp_stride + (long long)y * a.w + x]);
            if (val > 0.f) {
                float pos[3];
                reproject(a.q, x, y, val, pos);
                depth = sqrt_rn(squared_norm(pos));
            }
        }
    }
    a.depth[(size_t)set * a.max_points + i] = depth;
}

constexpr int CLOUD_THREADS = 1024;
// pass 0 counts, pass 1 writes: both walk the grid in chunks of CLOUD_THREADS points in row-major order
__global__ __launch_bounds__(CLOUD_THREADS) void stereo_point_cloud_kernel(DepthArgs a)
{
    __shared__ int wave_n[CLOUD_THREADS / 64];
    const int set = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int16_t *disp = a.disp + (long long)set * a.disp_stride;
    const int total = a.gx * a.gy;
    float *out = a.xyz + (size_t)set * a.max_points * 3;
    for (int pass = 0; pass < 2; ++pass) {
        int base = 0;
        for (int g0 = 0; g0 < total; g0 += CLOUD_THREADS) {
            const int g = g0 + t;
            bool keep = false;
            float pos[3] = {0.f, 0.f, 0.f};
            if (g < total) {
                const int gy = g / a.gx, y = gy * a.cloud_stride, x = (g - gy * a.gx) * a.cloud_stride;
                const float val = disparity_value(disp[(long long)y * a.w + x]);
                if (val > 0.f) {
                    reproject(a.q, x, y, val, pos);
                    keep = !(squared_norm(pos) < 1.0f);
                }
            }
            const unsigned long long m = __ballot(keep);
            if (lane == 0) wave_n[wave] = __popcll(m);
            __syncthreads();
            int before = 0, all = 0;
            for (int k = 0; k < CLOUD_THREADS / 64; ++k) { const int c = wave_n[k]; all += c; if (k < wave) before += c; }
            if (pass == 1 && keep) {
                const int o = base + before + __popcll(m & ((1ull << lane) - 1ull));
                out[3 * (size_t)o] = pos[0]; out[3 * (size_t)o + 1] = pos[1]; out[3 * (size_t)o + 2] = pos[2];
            }
            base += all;
            __syncthreads();
        }
        if (pass == 0) {
            if (base > a.max_points) { if (t == 0) a.n_out[set] = -1; return; }       // never truncated (uniform exit)
            if (t == 0) a.n_out[set] = base;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
int plane_stride(int w) { return (w + 15) & ~15; }
size_t label_offset(int w, int h) { return align16(2 * (size_t)plane_stride(w) * h); }
size_t speckle_bytes(int w, int h) { return align16(2 * sizeof(int) * (size_t)w * h); }
size_t set_work_bytes(int w, int h) { return label_offset(w, h) + speckle_bytes(w, h); }
size_t match_lds(int nd) { return (size_t)(nd + 1) * BM_PITCH * 2 + 2 * BM_LW + 2 * (size_t)((BM_LW + nd - 1 + 3) & ~3); }

int check_params(const hv_stereo_bm_params *p)
{
    if (!p || p->numDisparities < 16 || p->numDisparities % 16 != 0 || p->blockSize < 5 || p->blockSize % 2 == 0 ||
        p->preFilterCap < 1 || p->preFilterCap > 63 || p->textureThreshold < 0 || p->uniquenessRatio < 0) return HV_ERR_INVALID;
    return HV_OK;
}
int check_limits(const hv_stereo_bm_params *p)
{
    if (p->blockSize != BM_BLOCK || p->numDisparities > BM_MAX_ND || p->uniquenessRatio > 100 || p->textureThreshold > 65535 ||
        p->speckleWindowSize > (1 << 30)) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}
bool speckles_on(const hv_stereo_bm_params *p) { return p->speckleWindowSize > 0 && p->speckleRange >= 0; }

int launch_speckles(Ctx *c, const SpkArgs &a, int n_sets)
{
    const unsigned px_blocks = (unsigned)(((long long)a.w * a.h + 255) / 256);
    hipLaunchKernelGGL(spk_local_kernel, dim3((unsigned)(a.tiles_x * a.tiles_y), (unsigned)n_sets), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(spk_seam_kernel, dim3(px_blocks, (unsigned)n_sets), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(spk_count_kernel, dim3(px_blocks, (unsigned)n_sets), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(spk_apply_kernel, dim3(px_blocks, (unsigned)n_sets), dim3(256), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

bool image_too_large(long long w, long long h) { return w * h >= (1ll << 31) - 256 || ((w * h + 255) / 256) > 0x7fffffffll; }

// every launch of a disparity call, on the context stream; slots null: the single pair slot0 / slot1
int launch_disparity(Ctx *c, const hv_stereo_bm_params *p, int n_sets, const int *left_slots_dev, const int *right_slots_dev, int slot0,
                     int slot1, void *work_dev, int16_t *disp_dev, long long disp_set_stride, int *n_valid_dev)
{
    const int w = c->L.w[0], h = c->L.h[0];
    if (image_too_large(w, h)) return HV_ERR_UNSUPPORTED;
    BmArgs a{};
    a.l0_ptr = c->d_l0_ptr; a.l0_stride = c->d_l0_stride; a.left_slots = left_slots_dev; a.right_slots = right_slots_dev;
    a.slot0 = slot0; a.slot1 = slot1; a.pool_size = c->p.pool_size;
    a.w = w; a.h = h; a.nd = p->numDisparities; a.cap = p->preFilterCap; a.texture_threshold = p->textureThreshold;
    a.uniqueness_ratio = p->uniquenessRatio; a.ps = plane_stride(w);
    a.work = static_cast<unsigned char *>(work_dev); a.work_stride = set_work_bytes(w, h); a.label_off = label_offset(w, h);
    a.disp = disp_dev; a.disp_stride = disp_set_stride; a.n_valid = n_valid_dev;
    a.x0v = a.nd - 1 + BM_W2; a.x1v = w - BM_W2; a.y0v = BM_W2; a.y1v = h - BM_W2;
    const bool any = a.x1v > a.x0v && a.y1v > a.y0v;
    a.strips = any ? (a.x1v - a.x0v + BM_TX - 1) / BM_TX : 0; a.bands = any ? (a.y1v - a.y0v + BM_ROWS - 1) / BM_ROWS : 0;
    if ((long long)a.strips * a.bands * n_sets > 0x7fffffffll) return HV_ERR_UNSUPPORTED;
    ScopedKernelTime tm(c, HV_K_INGEST);
    const unsigned px_blocks = (unsigned)(((long long)w * h + 255) / 256);
    hipLaunchKernelGGL(bm_prefilter_kernel, dim3(px_blocks, 2u * (unsigned)n_sets), dim3(256), 0, c->stream, a);
    if (any)
        hipLaunchKernelGGL(bm_match_kernel, dim3((unsigned)(a.strips * a.bands * n_sets)), dim3(BM_THREADS), match_lds(a.nd), c->stream, a);
    HV_HIP(c, hipGetLastError());
    if (speckles_on(p) && any) {
        SpkArgs s{};
        s.w = w; s.h = h; s.tiles_x = (w + SPK_TW - 1) / SPK_TW; s.tiles_y = (h + SPK_TH - 1) / SPK_TH;
        s.disp = disp_dev; s.disp_stride = disp_set_stride; s.new_val = FILTERED; s.max_size = p->speckleWindowSize;
        s.max_diff = std::min(p->speckleRange, 65536);
        s.work = a.work; s.work_stride = a.work_stride; s.label_off = a.label_off;
        s.l0_ptr = a.l0_ptr; s.left_slots = left_slots_dev; s.right_slots = right_slots_dev; s.slot0 = slot0; s.slot1 = slot1;
        s.pool_size = a.pool_size; s.check_slots = true;
        if (const int rc = launch_speckles(c, s, n_sets)) return rc;
    }
    if (n_valid_dev) {
        hipLaunchKernelGGL(bm_count_kernel, dim3((unsigned)n_sets), dim3(1024), 0, c->stream, a);
        HV_HIP(c, hipGetLastError());
    }
    return HV_OK;
}

void fill_q(DepthArgs &a, const double *q) { for (int i = 0; i < 16; ++i) a.q[i] = (float)q[i]; }

}  // namespace

// the matching kernel's dynamic-LDS limit, set once per context (never inside a launch that may be under capture)
int stereo_bm_init(Ctx *c)
{
    HV_HIP(c, set_lds_limit(bm_match_kernel, match_lds(BM_MAX_ND)));
    return HV_OK;
}

}  // namespace hv

using hv::Ctx;

extern "C" {

int hv_stereo_num_disparities(int width)
{
    if (width < 1) return 0;
    return (int)(std::ceil((float)width * 0.1f / 32) * 32);              // stereo_disparity.cpp:39, in binary32 as written there
}

void hv_stereo_bm_default_params(hv_stereo_bm_params *p, int width)
{
    if (!p) return;
    p->numDisparities = hv_stereo_num_disparities(width);
    p->blockSize = 21; p->preFilterCap = 31; p->textureThreshold = 10; p->uniquenessRatio = 15;       // cv::StereoBM::create
    p->speckleWindowSize = 500; p->speckleRange = 10;                                                 // stereo_disparity.cpp:18-19
}

size_t hv_stereo_work_bytes(hv_ctx *ctx, const hv_stereo_bm_params *p, int n_sets)
{
    if (!ctx || hv::check_params(p) != HV_OK || n_sets <= 0) return 0;
    const Ctx *c = hv::ctx_of(ctx);
    return hv::set_work_bytes(c->L.w[0], c->L.h[0]) * (size_t)n_sets;
}

size_t hv_filter_speckles_work_bytes(int width, int height, int n_sets)
{
    if (width < 1 || height < 1 || n_sets <= 0) return 0;
    return hv::speckle_bytes(width, height) * (size_t)n_sets;
}

int hv_stereo_cloud_bound(hv_ctx *ctx, int cloud_stride)
{
    if (!ctx || cloud_stride < 1) return HV_ERR_INVALID;
    const Ctx *c = hv::ctx_of(ctx);
    const long long n = (long long)((c->L.w[0] + cloud_stride - 1) / cloud_stride) * ((c->L.h[0] + cloud_stride - 1) / cloud_stride);
    return n > 0x7fffffffll ? HV_ERR_UNSUPPORTED : (int)n;
}

int hv_stereo_disparity_batch_dev(hv_ctx *h, const hv_stereo_bm_params *p, int n_sets, const int *left_slots_dev,
                                  const int *right_slots_dev, void *work_dev, int16_t *disp_dev, long long disp_set_stride,
                                  int *n_valid_dev)
{
    if (const int rc = hv::check_params(p)) return rc;
    if (n_sets < 0 || disp_set_stride < 0) return HV_ERR_INVALID;
    if (n_sets > 0 && (!left_slots_dev || !right_slots_dev || !work_dev || !disp_dev)) return HV_ERR_INVALID;
    if (const int rc = hv::check_limits(p)) return rc;
    if (n_sets > 32767) return HV_ERR_UNSUPPORTED;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    if (disp_set_stride < (long long)c->L.w[0] * c->L.h[0]) return HV_ERR_INVALID;
    return hv::launch_disparity(c, p, n_sets, left_slots_dev, right_slots_dev, 0, 0, work_dev, disp_dev, disp_set_stride, n_valid_dev);
}

int hv_filter_speckles_batch_dev(hv_ctx *h, int n_sets, int width, int height, int16_t *disp_dev, long long set_stride, int new_val,
                                 int max_size, int max_diff, void *work_dev)
{
    if (n_sets < 0 || width < 1 || height < 1 || max_size < 0 || max_diff < 0 || new_val < -32768 || new_val > 32767 ||
        set_stride < (long long)width * height) return HV_ERR_INVALID;
    if (n_sets > 0 && (!disp_dev || !work_dev)) return HV_ERR_INVALID;
    if (n_sets > 65535 || hv::image_too_large(width, height)) return HV_ERR_UNSUPPORTED;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    hv::SpkArgs s{};
    s.w = width; s.h = height; s.tiles_x = (width + hv::SPK_TW - 1) / hv::SPK_TW; s.tiles_y = (height + hv::SPK_TH - 1) / hv::SPK_TH;
    s.disp = disp_dev; s.disp_stride = set_stride; s.new_val = new_val; s.max_size = max_size; s.max_diff = std::min(max_diff, 65536);
    s.work = static_cast<unsigned char *>(work_dev); s.work_stride = hv::speckle_bytes(width, height); s.label_off = 0;
    s.check_slots = false;
    hv::ScopedKernelTime tm(c, HV_K_INGEST);
    return hv::launch_speckles(c, s, n_sets);
}

int hv_stereo_track_depth_batch_dev(hv_ctx *h, int n_sets, int max_points, const int *n_points_dev, const float *xy_dev,
                                    const int16_t *disp_dev, long long stride, const double *Q, float *depth_dev)
{
    if (n_sets < 0 || max_points < 0 || stride < 0 || !Q) return HV_ERR_INVALID;
    if (n_sets > 0 && (!n_points_dev || !disp_dev || (max_points > 0 && (!xy_dev || !depth_dev)))) return HV_ERR_INVALID;
    if (n_sets > 65535) return HV_ERR_UNSUPPORTED;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0 || max_points == 0) return HV_OK;
    if (stride < (long long)c->L.w[0] * c->L.h[0]) return HV_ERR_INVALID;
    hv::DepthArgs a{};
    a.w = c->L.w[0]; a.h = c->L.h[0]; a.disp = disp_dev; a.disp_stride = stride; hv::fill_q(a, Q);
    a.max_points = max_points; a.n_points = n_points_dev; a.xy = xy_dev; a.depth = depth_dev;
    hv::ScopedKernelTime tm(c, HV_K_STEREO_GATE);
    hipLaunchKernelGGL(hv::stereo_track_depth_kernel, dim3((unsigned)((max_points + 255) / 256), (unsigned)n_sets), dim3(256), 0,
                       c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_stereo_point_cloud_batch_dev(hv_ctx *h, int n_sets, const int16_t *disp_dev, long long stride, const double *Q,
                                    int cloud_stride, int max_points, float *xyz_dev, int *n_points_dev)
{
    if (n_sets < 0 || max_points < 0 || stride < 0 || !Q || cloud_stride < 1) return HV_ERR_INVALID;
    if (n_sets > 0 && (!disp_dev || !n_points_dev || (max_points > 0 && !xyz_dev))) return HV_ERR_INVALID;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    if (stride < (long long)c->L.w[0] * c->L.h[0]) return HV_ERR_INVALID;
    const int bound = hv_stereo_cloud_bound(h, cloud_stride);
    if (bound < 0) return bound;
    hv::DepthArgs a{};
    a.w = c->L.w[0]; a.h = c->L.h[0]; a.disp = disp_dev; a.disp_stride = stride; hv::fill_q(a, Q);
    a.max_points = max_points; a.cloud_stride = cloud_stride;
    a.gx = (a.w + cloud_stride - 1) / cloud_stride; a.gy = (a.h + cloud_stride - 1) / cloud_stride;
    a.xyz = xyz_dev; a.n_out = n_points_dev;
    hv::ScopedKernelTime tm(c, HV_K_STEREO_GATE);
    hipLaunchKernelGGL(hv::stereo_point_cloud_kernel, dim3((unsigned)n_sets), dim3(hv::CLOUD_THREADS), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_stereo_disparity(hv_ctx *ctx, const hv_stereo_bm_params *p, int left_slot, int right_slot, int16_t *disp_host, long long stride)
{
    if (const int rc = hv::check_params(p)) return rc;
    if (!ctx || !disp_host) return HV_ERR_INVALID;
    if (const int rc = hv::check_limits(p)) return rc;
    Ctx *c = hv::ctx_of(ctx);
    const int w = c->L.w[0], hgt = c->L.h[0];
    if (stride < w) return HV_ERR_INVALID;
    for (const int slot : {left_slot, right_slot})
        if (slot < 0 || slot >= c->p.pool_size || !c->slot_used[slot]) return HV_ERR_POOL;
    int n_valid = 0;
    hv::Stage s(c);
    const auto o_valid = s.out(&n_valid, 1);
    const auto o_work = s.take<unsigned char>(hv::set_work_bytes(w, hgt));
    const auto o_disp = s.take<int16_t>((size_t)w * hgt);
    int rc = s.upload();
    if (rc != HV_OK) return rc;
    rc = hv::launch_disparity(c, p, 1, nullptr, nullptr, left_slot, right_slot, s.at(o_work), s.at(o_disp), (long long)w * hgt,
                              s.at(o_valid));
    if (rc == HV_OK) rc = s.download();
    if (rc != HV_OK) return rc;
    if (n_valid < 0) return HV_ERR_POOL;                       // a slot holds no image yet
    if (stride == w) rc = s.fetch(disp_host, o_disp, (size_t)w * hgt);
    else
        for (int y = 0; y < hgt && rc == HV_OK; ++y)
            rc = hv::stage_to_host(c, disp_host + (long long)y * stride, s.at(o_disp) + (size_t)y * w, sizeof(int16_t) * (size_t)w);
    if (rc == HV_OK) rc = s.sync();
    return rc;
}

// the two lookups on a disparity image the caller holds on the host (the C++ adapter's): staged through the arena, image included
int hv_stereo_track_depth(hv_ctx *ctx, int n_points, const float *xy_host, const int16_t *disp_host, long long stride, const double *Q,
                          float *depth_host)
{
    if (!ctx || n_points < 0 || !disp_host || !Q || (n_points > 0 && (!xy_host || !depth_host))) return HV_ERR_INVALID;
    Ctx *c = hv::ctx_of(ctx);
    const int w = c->L.w[0], hgt = c->L.h[0];
    if (stride != w) return HV_ERR_INVALID;
    if (n_points == 0) return HV_OK;
    hv::Stage s(c);
    const auto o_n = s.in(&n_points, 1);
    const auto o_xy = s.in(xy_host, 2 * (size_t)n_points);
    const auto o_disp = s.in(disp_host, (size_t)w * hgt);
    const auto o_depth = s.out(depth_host, (size_t)n_points);
    int rc = s.upload();
    if (rc != HV_OK) return rc;
    rc = hv_stereo_track_depth_batch_dev(ctx, 1, n_points, s.at(o_n), s.at(o_xy), s.at(o_disp), (long long)w * hgt, Q, s.at(o_depth));
    return rc == HV_OK ? s.download() : rc;
}

int hv_stereo_point_cloud(hv_ctx *ctx, const int16_t *disp_host, long long stride, const double *Q, int cloud_stride, float *xyz_host,
                          int capacity, int *n_out)
{
    if (!ctx || !disp_host || !Q || cloud_stride < 1 || capacity < 0 || !n_out || (capacity > 0 && !xyz_host)) return HV_ERR_INVALID;
    Ctx *c = hv::ctx_of(ctx);
    const int w = c->L.w[0], hgt = c->L.h[0];
    if (stride != w) return HV_ERR_INVALID;
    const int bound = hv_stereo_cloud_bound(ctx, cloud_stride);
    if (bound < 0) return bound;
    const int cap = std::min(capacity, bound);
    int count = 0;
    hv::Stage s(c);
    const auto o_disp = s.in(disp_host, (size_t)w * hgt);
    const auto o_count = s.out(&count, 1);
    const auto o_xyz = s.take<float>(3 * (size_t)std::max(cap, 1));
    int rc = s.upload();
    if (rc != HV_OK) return rc;
    rc = hv_stereo_point_cloud_batch_dev(ctx, 1, s.at(o_disp), (long long)w * hgt, Q, cloud_stride, cap, s.at(o_xyz), s.at(o_count));
    if (rc == HV_OK) rc = s.download();
    if (rc != HV_OK) return rc;
    if (count < 0) return HV_ERR_INVALID;                      // more points than the capacity: nothing is written
    if (count > 0) {
        rc = s.fetch(xyz_host, o_xyz, 3 * (size_t)count);
        if (rc == HV_OK) rc = s.sync();
        if (rc != HV_OK) return rc;
    }
    *n_out = count;
    return HV_OK;
}

}  // extern "C"
