// Legacy GFTT corner detector (featureDetector "GFTT"): cv::goodFeaturesToTrack behind the track mask, batched, no allocation and
// no synchronisation (capturable in a HIP graph).
//
// Reference: src/tracker/feature_detector_legacy.cpp:53-139 (GFTTFeatureDetector = cv::GFTTDetector, i.e.
// cv::goodFeaturesToTrack(gray, corners, maxTracks, gfttQualityLevel, minDistance, mask, gfttBlockSize, 3, false)), :20-51
// (MaskedFeatureDetector::detect / setMask / drawMask) and src/tracker/feature_detector.cpp:659-680 (FeatureDetector::build);
// codegen/parameter_definitions.c:310-311. The rules are restated in tests/gftt_legacy_restatement.py and in the header.
//
// One memset and three launches per call:
//   memset                    the per-image header (masked maximum, candidate count) to zero
//   legacy_response_kernel    one workgroup per HV_GFTT_LEGACY_TILE_W x _H tile of one image. The tile of the mask (a box per live track,
//       drawMask) is drawn in LDS and written as one byte per pixel; the response cv::cornerMinEigenVal(gray, blockSize, 3) of the
//       tile is evaluated in LDS in the oracle's operation order (the three-pass form of gftt.hip's box kernel: products at
//       BORDER_REFLECT_101 mirrored centres, row sums left to right, column sums top to bottom, sqrt_rn) and written as a float
//       map; the maximum over the tile's unmasked pixels goes to the image's header with ONE atomic max per workgroup, on an
//       order-preserving unsigned image of the float (0 = no unmasked pixel yet).
//   legacy_candidates_kernel  the same tiles with a 1-pixel halo: the thresholded response (THRESH_TOZERO at (float)((double)max *
//       quality)), the 3 x 3 maximum test, the mask. A candidate is appended to the image's key list as (ordered response bits <<
//       32 | raster index); keys are unique, so the append order does not matter. The responses are read from the map: evaluating
//       them again here instead was measured and is slower.
//   legacy_select_kernel      one workgroup per image. The keys are consumed from the top in groups of at most SEL_CAP: a histogram
//       of the keys below the previous group over 1024 equal buckets of the remaining key range finds the largest group of whole
//       buckets that fits (a top bucket that does not fit alone is split again, which ends because keys are unique: no limit on
//       equal responses); the group is gathered into LDS, sorted by a bitonic network (descending key = descending response, equal
//       responses by descending raster index: OpenCV 4.x's greaterThanPtr) and walked in blocks as fast.hip's tail does, with the
//       exact integer test dx dx + dy dy < ceil(minDistance^2). The walk stops at maxTracks, and so do the groups.
#include "hv_internal.hpp"
#include "hv_sqrt_rn.hpp"

#include <algorithm>
#include <cmath>

namespace hv {
namespace {

constexpr int TW = HV_GFTT_LEGACY_TILE_W, TH = HV_GFTT_LEGACY_TILE_H;
static_assert(TW == 64 && TH == 16, "256 threads, four pixels of a row each; a packed box holds tile coordinates in bytes");
constexpr int SEL_THREADS = 1024, SEL_WAVES = SEL_THREADS / 64;
constexpr int SEL_CAP = 4096;                     // keys of a sorted group (32 KB of LDS)
constexpr int SEL_BUCKETS = SEL_THREADS;          // one bucket per thread
constexpr int MAX_EDGE = 32767;                   // 2 * (MAX_EDGE - 1)^2 < 2^31: the walk's squared distances are ints
constexpr int MIN_EDGE = 8;                       // one reflection serves every halo (block size 7: 3 + 1 + 1 pixels)

struct LegacyArgs {
    const uint8_t *const *l0_ptr;     // per-slot level-0 image table (filled by the pyramid build)
    const int *l0_stride;
    const int *slots;                 // [n_images], or null: the single image slot0
    int slot0, pool_size;
    int w, h, tiles_x, tiles_y;
    float k0, k1;
    double quality;
    unsigned *head;                   // [n_images][2]: ordered bits of the masked maximum (0: none), candidate count
    unsigned long long *keys;         // [n_images][max_keypoints]
    float *resp_map;                  // [n_images][map_stride], rows of w floats
    unsigned char *mask;              // [n_images][mask_stride], rows of mstride bytes (w rounded up to 4); 1 = unmasked
    size_t map_stride, mask_stride;
    int mstride, max_keypoints;
    int max_prev; const int *n_prev; const float *prev; const int *radius;      // radius null: no live tracks (key points only)
    int dist2;                        // ceil(minDistance^2), or 0: no distance test (minDistance < 1)
    int max_tracks, max_corners; float *corners; float *resp; int *n_cand; int *n_out;
};

__device__ __forceinline__ const uint8_t *image_of(const LegacyArgs &a, int img, int *stride)
{
    const int slot = a.slots ? a.slots[img] : a.slot0;
    if (slot < 0 || slot >= a.pool_size) return nullptr;                // not a slot
    *stride = a.l0_stride[slot];
    return a.l0_ptr[slot];                                              // null: a slot no pyramid was built in
}

// order-preserving unsigned image of a float (negative values included; every float maps above 0) and back
__device__ __forceinline__ unsigned ordered(float f)
{
    const unsigned b = __float_as_uint(f);
    return b ^ ((unsigned)((int)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float unordered(unsigned u) { return __uint_as_float((u & 0x80000000u) ? u ^ 0x80000000u : ~u); }

// BORDER_REFLECT_101 for one reflection (-n < p < 2n - 1), clamped: positions further out are staging margin nothing reads
__device__ __forceinline__ int mirror(int p, int n)
{
    if (p < 0) p = -p;
    if (p >= n) p = 2 * n - 2 - p;
    return min(max(p, 0), n - 1);
}

// sizes of the LDS arrays of one tile's response with a box of 2 HB + 1
template <int HB>
struct TileDims {
    static constexpr int PW = TW + 2 * HB, PH = TH + 2 * HB;          // derivative products: column c <-> image x0 - HB + c
    static constexpr int GW = PW + 2, GH = PH + 2;                    // gray: column c <-> x0 - HB - 1 + c
};

// The responses of the tile at (x0, y0), into gray[TH][TW] (the gray tile's own memory). The oracle's float order
// (oracle/gftt_oracle.c, gftt.hip's box kernel): every product is evaluated at its BORDER_REFLECT_101 mirrored centre (= box-filtering
// the reflected product images, as cv::boxFilter does). Positions more than HB outside the image (the part of a ragged tile
// that no pixel of the image reads) are zero.
template <int HB>
__device__ __forceinline__ void tile_response(const uint8_t *src, int stride, int w, int h, int x0, int y0, float k0, float k1,
                                              float *gray, float (*prod)[TileDims<HB>::PW * TileDims<HB>::PH],
                                              float (*rsum)[TileDims<HB>::PH * TW])
{
    using D = TileDims<HB>;
    const int t = threadIdx.x;
    const int gx0 = x0 - HB - 1, gy0 = y0 - HB - 1;
    for (int i = t; i < D::GW * D::GH; i += 256) {
        const int r = i / D::GW, c = i - r * D::GW;
        gray[i] = (float)src[(size_t)mirror(gy0 + r, h) * stride + mirror(gx0 + c, w)];
    }
    __syncthreads();
    for (int i = t; i < D::PW * D::PH; i += 256) {
        const int pr = i / D::PW, pc = i - pr * D::PW;
        const int py = gy0 + 1 + pr, px = gx0 + 1 + pc;
        float vx = 0.f, vy = 0.f;
        if (py >= -HB && py <= h - 1 + HB && px >= -HB && px <= w - 1 + HB) {
            // the mirrored centre lies inside the image and inside the tile's product region: its 3 x 3 gray neighbourhood is staged
            const float *g = gray + (mirror(py, h) - gy0) * D::GW + (mirror(px, w) - gx0);
            const float dt = g[-D::GW + 1] - g[-D::GW - 1], dm = g[1] - g[-1], db = g[D::GW + 1] - g[D::GW - 1];
            vx = k0 * dm + k1 * (dt + db);
            const float st = k0 * g[-D::GW] + k1 * (g[-D::GW - 1] + g[-D::GW + 1]);
            const float sb = k0 * g[D::GW] + k1 * (g[D::GW - 1] + g[D::GW + 1]);
            vy = sb - st;
        }
        prod[0][i] = vx * vx; prod[1][i] = vx * vy; prod[2][i] = vy * vy;
    }
    __syncthreads();
    for (int i = t; i < D::PH * TW; i += 256) {
        const int pr = i / TW, x = i - pr * TW;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float *p = prod[ch] + pr * D::PW + x;                // product columns x - HB .. x + HB
            float s_ = p[0];
#pragma unroll
            for (int k = 1; k <= 2 * HB; k++) s_ = s_ + p[k];
            rsum[ch][i] = s_;
        }
    }
    __syncthreads();
    for (int i = t; i < TH * TW; i += 256) {
        const int y = i / TW, x = i - y * TW;
        float sm[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float *p = rsum[ch] + y * TW + x;                    // product rows y - HB .. y + HB
            float s_ = p[0];
#pragma unroll
            for (int k = 1; k <= 2 * HB; k++) s_ = s_ + p[k * TW];
            sm[ch] = s_;
        }
        const float aa = sm[0] * 0.5f, bb = sm[1], cc = sm[2] * 0.5f, amc = aa - cc;
        gray[i] = (aa + cc) - sqrt_rn(amc * amc + bb * bb);            // (the gray tile was last read before the second barrier)
    }
    __syncthreads();
}

// which tile of which image a workgroup serves
struct TileOf { int img, x0, y0; };
__device__ __forceinline__ TileOf tile_of(const LegacyArgs &a)
{
    const int tiles = a.tiles_x * a.tiles_y;
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);              // neighbouring tiles share halo rows: one XCD's L2
    const int img = lb / tiles, ti = lb - img * tiles;
    const int tyi = ti / a.tiles_x, txi = ti - tyi * a.tiles_x;
    return TileOf{img, txi * TW, tyi * TH};
}

template <int HB>
__global__ __launch_bounds__(256) void legacy_response_kernel(LegacyArgs a)
{
    using D = TileDims<HB>;
    __shared__ float gray[D::GW * D::GH];
    __shared__ float prod[3][D::PW * D::PH];
    __shared__ float rsum[3][D::PH * TW];
    __shared__ uint32_t s_box[256];
    __shared__ int s_nbox;
    __shared__ unsigned s_max;
    const int t = threadIdx.x, w = a.w, h = a.h;
    const TileOf tl = tile_of(a);
    const int x0 = tl.x0, y0 = tl.y0;
    int stride = 0;
    const uint8_t *src = image_of(a, tl.img, &stride);
    const int r = a.radius ? a.radius[tl.img] : 1;
    if (!src || r < 1) return;                                          // (the select kernel reports the image)

    // ---- drawMask on the tile: a box per live track inside the image, upper ends exclusive. 256 tracks at a time: a thread clips
    // one box to the tile and queues it (tile coordinates in four bytes) if anything is left; every thread then applies the queued
    // boxes to its four pixels. A zero is a zero whoever writes it, so the queue's order does not matter.
    const int row = t >> 4, x4 = (t & 15) * 4;                          // this thread's pixels: (x0 + x4 .. x4 + 3, y0 + row)
    uint32_t mword = 0x01010101u;
    if (t == 0) { s_nbox = 0; s_max = 0u; }
    __syncthreads();
    const int n_prev = (a.radius && a.n_prev && a.max_prev > 0) ? min(max(a.n_prev[tl.img], 0), a.max_prev) : 0;
    for (int base = 0; base < n_prev; base += 256) {
        const int i = base + t;
        if (i < n_prev) {
            const float *p = a.prev + ((size_t)tl.img * a.max_prev + i) * 2;
            const float px = p[0], py = p[1];
            if (0.f < px && px < (float)w && 0.f < py && py < (float)h) {                   // (NaN draws nothing)
                const long long ix = (int)px, iy = (int)py;
                const int xa = (int)max(max(ix - r, 0ll), (long long)x0), xb = (int)min(min(ix + r, (long long)w - 1), (long long)x0 + TW);
                const int ya = (int)max(max(iy - r, 0ll), (long long)y0), yb = (int)min(min(iy + r, (long long)h - 1), (long long)y0 + TH);
                if (xb > xa && yb > ya)
                    s_box[atomicAdd(&s_nbox, 1)] = (uint32_t)(xa - x0) | ((uint32_t)(xb - x0) << 8) | ((uint32_t)(ya - y0) << 16) | ((uint32_t)(yb - y0) << 24);
            }
        }
        __syncthreads();
        const int nb = s_nbox;
        for (int k = 0; k < nb; ++k) {
            const uint32_t b = s_box[k];
            const int xa = b & 0xFF, xb = (b >> 8) & 0xFF, ya = (b >> 16) & 0xFF, yb = b >> 24;
            if (row < ya || row >= yb) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) if (x4 + j >= xa && x4 + j < xb) mword &= ~(0xFFu << (8 * j));
        }
        __syncthreads();
        if (t == 0) s_nbox = 0;
        __syncthreads();
    }
    const int y = y0 + row, x = x0 + x4;
    const bool inside = y < h && x < a.mstride;
    if (inside) *reinterpret_cast<uint32_t *>(a.mask + (size_t)tl.img * a.mask_stride + (size_t)y * a.mstride + x) = mword;

    // ---- the response of the tile, its map and the maximum over the unmasked pixels
    tile_response<HB>(src, stride, w, h, x0, y0, a.k0, a.k1, gray, prod, rsum);
    unsigned best = 0u;
    if (inside) {
        float *o = a.resp_map + (size_t)tl.img * a.map_stride + (size_t)y * w + x;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x + j >= w) break;
            const float v = gray[row * TW + x4 + j];
            o[j] = v;
            if ((mword >> (8 * j)) & 0xFFu) best = max(best, ordered(v));
        }
    }
    if (best) atomicMax(&s_max, best);
    __syncthreads();
    if (t == 0 && s_max) atomicMax(a.head + 2 * (size_t)tl.img, s_max);
}

__global__ __launch_bounds__(256) void legacy_candidates_kernel(LegacyArgs a)
{
    constexpr int RW = TW + 2, RH = TH + 2;                             // the tile and its 1-pixel ring: column c <-> image x0 - 1 + c
    __shared__ float val[RW * RH];                                      // thresholded responses
    __shared__ int s_cnt;
    __shared__ unsigned s_base;
    const int t = threadIdx.x, w = a.w, h = a.h;
    const TileOf tl = tile_of(a);
    const int x0 = tl.x0, y0 = tl.y0;
    int stride = 0;
    const uint8_t *src = image_of(a, tl.img, &stride);
    const int r = a.radius ? a.radius[tl.img] : 1;
    if (!src || r < 1) return;
    if (t == 0) s_cnt = 0;

    // t = (float)((double)maxVal * qualityLevel); maxVal = 0 when no pixel is unmasked
    const unsigned mo = a.head[2 * (size_t)tl.img];
    const float thr = (float)((double)(mo ? unordered(mo) : 0.f) * a.quality);
    const float *map = a.resp_map + (size_t)tl.img * a.map_stride;
    for (int i = t; i < RW * RH; i += 256) {
        const int rr = i / RW, c = i - rr * RW;
        const int y = y0 - 1 + rr, x = x0 - 1 + c;
        float e = 0.f;                                                  // outside the image: never a candidate's neighbour
        if (y >= 0 && y < h && x >= 0 && x < w) e = map[(size_t)y * w + x];
        val[i] = e > thr ? e : 0.f;                                     // THRESH_TOZERO
    }
    __syncthreads();

    // ---- candidates: non-zero, the maximum of its 3 x 3 neighbourhood, inside the 1-pixel border, unmasked
    const int row = t >> 4, x4 = (t & 15) * 4;
    const int y = y0 + row, x = x0 + x4;
    unsigned long long mine[4];
    int nc = 0;
    if (y >= 1 && y <= h - 2 && x < a.mstride) {
        const uint32_t mword = *reinterpret_cast<const uint32_t *>(a.mask + (size_t)tl.img * a.mask_stride + (size_t)y * a.mstride + x);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xx = x + j;
            const float *p = val + (row + 1) * RW + x4 + j + 1;
            const float v = p[0];
            const bool ok = xx >= 1 && xx <= w - 2 && v != 0.f && ((mword >> (8 * j)) & 0xFFu) &&
                            v >= p[-RW - 1] && v >= p[-RW] && v >= p[-RW + 1] && v >= p[-1] && v >= p[1] &&
                            v >= p[RW - 1] && v >= p[RW] && v >= p[RW + 1];
            if (ok) mine[nc++] = ((unsigned long long)ordered(v) << 32) | (unsigned)(y * w + xx);
        }
    }
    const int off = nc ? atomicAdd(&s_cnt, nc) : 0;
    __syncthreads();
    if (t == 0 && s_cnt) s_base = atomicAdd(a.head + 2 * (size_t)tl.img + 1, (unsigned)s_cnt);
    __syncthreads();
    if (nc) {
        // the count runs on past max_keypoints (the select kernel reports the image); nothing is written past it
        unsigned long long *keys = a.keys + (size_t)tl.img * a.max_keypoints;
        const unsigned at = s_base + (unsigned)off;
#pragma unroll
        for (int j = 0; j < 4; ++j) if (j < nc && at + j < (unsigned)a.max_keypoints) keys[at + j] = mine[j];
    }
}

// LDS: static (keys of a group, histogram and its suffix sums) | dynamic int2 list[max_tracks], the accepted corners
__global__ __launch_bounds__(SEL_THREADS) void legacy_select_kernel(LegacyArgs a)
{
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ unsigned long long s_keys[SEL_CAP];
    __shared__ int s_hist[SEL_BUCKETS], s_scan[SEL_BUCKETS];
    __shared__ unsigned long long s_live[SEL_WAVES];
    __shared__ unsigned long long s_kmin, s_kmax, s_lo;
    __shared__ int s_total, s_m, s_refine, s_fill;
    int2 *list = reinterpret_cast<int2 *>(lds);
    const int set = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = a.w;

    int stride = 0;
    const bool image = image_of(a, set, &stride) != nullptr;
    const int r = a.radius ? a.radius[set] : 1;
    const unsigned n_all = a.head[2 * (size_t)set + 1];
    if (!image || r < 1 || n_all > (unsigned)a.max_keypoints) {       // never truncated: the sort would pick other corners
        if (tid == 0) { a.n_cand[set] = -1; a.n_out[set] = -1; }
        return;
    }
    const int n = (int)n_all;
    const unsigned long long *keys = a.keys + (size_t)set * a.max_keypoints;

    // ---- the smallest and the largest key: the range of the first histogram
    if (tid == 0) { s_kmin = ~0ull; s_kmax = 0ull; }
    __syncthreads();
    {
        unsigned long long km = ~0ull, kx = 0ull;
        for (int i = tid; i < n; i += SEL_THREADS) { const unsigned long long k = keys[i]; km = min(km, k); kx = max(kx, k); }
        if (kx) { atomicMin(&s_kmin, km); atomicMax(&s_kmax, kx); }
    }
    __syncthreads();
    const unsigned long long kmin = s_kmin;

    float *out = a.corners + (size_t)set * a.max_corners * 2;
    float *out_r = a.resp ? a.resp + (size_t)set * a.max_corners : nullptr;
    volatile int *acc = reinterpret_cast<volatile int *>(list);
    const int dist2 = a.dist2;
    unsigned long long hi = s_kmax + 1ull;                              // the keys not yet walked are those below hi
    int remaining = n, n_acc = 0;
    while (remaining > 0 && n_acc < a.max_tracks) {
        // ---- the next group [lo, hi): as many whole buckets from the top as SEL_CAP keys hold
        unsigned long long origin = kmin;
        int m = 0;
        unsigned long long lo = 0;
        while (true) {
            const unsigned long long span = hi - 1ull - origin;
            const int shift = span ? max(0, 64 - __clzll((long long)span) - 10) : 0;         // span >> shift < 1024
            s_hist[tid] = 0;
            if (tid == 0) s_refine = -1;
            __syncthreads();
            for (int i = tid; i < n; i += SEL_THREADS) {
                const unsigned long long k = keys[i];
                if (k >= origin && k < hi) atomicAdd(&s_hist[(int)((k - origin) >> shift)], 1);
            }
            __syncthreads();
            // suffix sums: s_scan[j] = the keys in buckets j .. 1023
            const int mine = s_hist[tid];
            int v = mine;
            s_scan[tid] = v;
            __syncthreads();
            for (int o = 1; o < SEL_BUCKETS; o <<= 1) {
                const int add = tid + o < SEL_BUCKETS ? s_scan[tid + o] : 0;
                __syncthreads();
                v += add;
                s_scan[tid] = v;
                __syncthreads();
            }
            if (mine > SEL_CAP && v == mine) s_refine = tid;          // the top bucket alone does not fit (at most one thread)
            if (v <= SEL_CAP && (tid == 0 || s_scan[tid - 1] > SEL_CAP)) { s_lo = origin + ((unsigned long long)tid << shift); s_m = v; }
            __syncthreads();
            const int refine = s_refine;
            if (refine < 0) { lo = s_lo; m = s_m; break; }
            // every key below hi and from that bucket's start up is in that bucket: both ends move, so the span shrinks by 10 bits
            origin += (unsigned long long)refine << shift;
            const unsigned long long top = origin + (1ull << shift);
            if (top > origin && top < hi) hi = top;
            __syncthreads();                                           // (s_refine is read before the next round resets it)
        }

        // ---- gather, pad to a power of two with keys below every real one, sort descending
        int M = 64;
        while (M < m) M <<= 1;
        if (tid == 0) s_fill = 0;
        __syncthreads();
        for (int i = tid; i < n; i += SEL_THREADS) {
            const unsigned long long k = keys[i];
            if (k >= lo && k < hi) s_keys[atomicAdd(&s_fill, 1)] = k;
        }
        for (int i = m + tid; i < M; i += SEL_THREADS) s_keys[i] = 0ull;
        __syncthreads();
        for (int k = 2; k <= M; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < M; i += SEL_THREADS) {
                    const int p = i ^ j;
                    if (p > i) {
                        const unsigned long long x = s_keys[i], y = s_keys[p];
                        if (((i & k) == 0) ? x < y : x > y) { s_keys[i] = y; s_keys[p] = x; }
                    }
                }
                __syncthreads();
            }
        }

        // ---- the greedy walk over the group in blocks of SEL_THREADS candidates (fast.hip's tail): every thread tests its candidate
        // against the corners accepted before the block; the first wavefront then walks the block's 16 chunks in order, testing the
        // survivors against the corners accepted inside the block, one ballot per accepted corner. The first wavefront reads and
        // writes the list through a volatile pointer, in program order (LDS operations of one wavefront complete in issue order).
        for (int base = 0; base < m && n_acc < a.max_tracks; base += SEL_THREADS) {
            const int i = base + tid;
            bool live = i < m;
            if (live && dist2 > 0) {
                const unsigned idx = (unsigned)s_keys[i];
                const int y = (int)(idx / (unsigned)w), x = (int)idx - y * w;
#pragma unroll 8
                for (int j = 0; j < n_acc; ++j) {
                    const int2 c = list[j];
                    const int dx = c.x - x, dy = c.y - y;
                    if (dx * dx + dy * dy < dist2) live = false;
                }
            }
            const unsigned long long alive = __ballot(live);
            if (lane == 0) s_live[wave] = alive;
            __syncthreads();
            if (wave == 0) {
                const int n0 = n_acc;
                for (int c = 0; c < SEL_WAVES && n_acc < a.max_tracks; ++c) {
                    const unsigned long long mk = s_live[c];
                    if (mk == 0) continue;
                    bool lv = (mk >> lane) & 1ull;
                    const unsigned long long key = lv ? s_keys[base + c * 64 + lane] : 0ull;
                    const unsigned idx = (unsigned)key;
                    const int qy = (int)(idx / (unsigned)w), qx = (int)idx - qy * w;
                    __builtin_amdgcn_wave_barrier();
                    if (dist2 > 0)
                        for (int j = n0; j < n_acc; ++j) {
                            const int dx = acc[2 * j] - qx, dy = acc[2 * j + 1] - qy;
                            if (dx * dx + dy * dy < dist2) lv = false;
                        }
                    while (true) {
                        const unsigned long long b = __ballot(lv);
                        if (b == 0) break;
                        const int lead = __ffsll((long long)b) - 1;
                        const int ax = __shfl(qx, lead), ay = __shfl(qy, lead);
                        if (lane == lead) {
                            acc[2 * n_acc] = ax; acc[2 * n_acc + 1] = ay;
                            out[2 * n_acc] = (float)ax; out[2 * n_acc + 1] = (float)ay;
                            if (out_r) out_r[n_acc] = unordered((unsigned)(key >> 32));
                            lv = false;
                        }
                        ++n_acc;
                        if (n_acc >= a.max_tracks) break;
                        if (lv && dist2 > 0) {
                            const int dx = ax - qx, dy = ay - qy;
                            if (dx * dx + dy * dy < dist2) lv = false;
                        }
                    }
                }
                if (lane == 0) s_total = n_acc;
            }
            __syncthreads();
            n_acc = s_total;
        }
        hi = lo;
        remaining -= m;
        __syncthreads();                                               // (the group's keys are read before the next gather)
    }
    if (tid == 0) { a.n_cand[set] = n; a.n_out[set] = n_acc; }
}

int mstride_of(const Ctx *c) { return (c->L.w[0] + 3) & ~3; }
size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
size_t mask_bytes(const Ctx *c) { return align16((size_t)mstride_of(c) * c->L.h[0]); }
size_t map_floats(const Ctx *c) { return align16(sizeof(float) * (size_t)c->L.w[0] * c->L.h[0]) / sizeof(float); }
size_t head_bytes(int n_images) { return align16(2 * sizeof(unsigned) * (size_t)n_images); }
size_t work_bytes(const Ctx *c, int n_images, int max_keypoints)
{
    return head_bytes(n_images) + (size_t)n_images * (sizeof(unsigned long long) * (size_t)max_keypoints + sizeof(float) * map_floats(c) + mask_bytes(c));
}
int keypoint_bound(const Ctx *c)
{
    const long long w = c->L.w[0], h = c->L.h[0];
    return (w < 3 || h < 3) ? 0 : (int)std::min((w - 2) * (h - 2), (long long)INT32_MAX);
}
double min_distance(const Ctx *c, const hv_gftt_legacy_params *p)
{
    return p->gfttMinDistance * (std::min(c->L.w[0], c->L.h[0]) / 720.0);         // feature_detector_legacy.cpp:53-68
}
size_t select_lds(int max_tracks) { return sizeof(int) * 2 * (size_t)std::max(max_tracks, 1); }

// the checks the entries share, made before the context is looked at
int check_params(const hv_gftt_legacy_params *p)
{
    if (!p || p->maxTracks < 1 || !(p->gfttQualityLevel > 0.0) || !(p->gfttMinDistance >= 0.0)) return HV_ERR_INVALID;
    return HV_OK;
}
int check_limits(const hv_gftt_legacy_params *p, int n_images, int max_prev)
{
    if ((p->gfttBlockSize != 3 && p->gfttBlockSize != 5 && p->gfttBlockSize != 7) || n_images > 65535 ||
        max_prev > HV_DETECT_TAIL_MAX_PREV || p->maxTracks > HV_DETECT_TAIL_MAX_TRACKS) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}

// the memset and the three launches, on the context stream; slots_dev null: the single image slot0; radius_dev null: no live tracks
int launch(Ctx *c, const hv_gftt_legacy_params *p, int n_images, const int *slots_dev, int slot0, void *work_dev, int max_keypoints,
           int *n_cand_dev, int max_prev, const int *n_prev_dev, const float *prev_dev, const int *radius_dev, int max_corners,
           float *corners_dev, float *resp_dev, int *n_out_dev)
{
    const int w = c->L.w[0], h = c->L.h[0];
    if (w < MIN_EDGE || h < MIN_EDGE || w > MAX_EDGE || h > MAX_EDGE) return HV_ERR_UNSUPPORTED;
    LegacyArgs a{};
    a.l0_ptr = c->d_l0_ptr; a.l0_stride = c->d_l0_stride; a.slots = slots_dev; a.slot0 = slot0; a.pool_size = c->p.pool_size;
    a.w = w; a.h = h; a.tiles_x = (w + TW - 1) / TW; a.tiles_y = (h + TH - 1) / TH;
    const double scale = 1.0 / (4.0 * p->gfttBlockSize * 255.0);         // cv::cornerMinEigenVal: aperture 3, uint8 input
    a.k1 = (float)scale; a.k0 = (float)(2.0 * scale);
    a.quality = p->gfttQualityLevel;
    unsigned char *work = static_cast<unsigned char *>(work_dev);
    a.head = reinterpret_cast<unsigned *>(work); work += head_bytes(n_images);
    a.keys = reinterpret_cast<unsigned long long *>(work); work += sizeof(unsigned long long) * (size_t)max_keypoints * n_images;
    a.resp_map = reinterpret_cast<float *>(work); a.map_stride = map_floats(c); work += sizeof(float) * a.map_stride * n_images;
    a.mask = work; a.mask_stride = mask_bytes(c); a.mstride = mstride_of(c);
    a.max_keypoints = max_keypoints;
    a.max_prev = max_prev; a.n_prev = n_prev_dev; a.prev = prev_dev; a.radius = radius_dev;
    const double md = min_distance(c, p);
    a.dist2 = md >= 1.0 ? (int)std::min(std::ceil(md * md), (double)INT32_MAX) : 0;
    a.max_tracks = std::min(p->maxTracks, std::max(max_keypoints, 1)); a.max_corners = max_corners;
    a.corners = corners_dev; a.resp = resp_dev; a.n_cand = n_cand_dev; a.n_out = n_out_dev;
    {
        ScopedKernelTime tm(c, HV_K_GFTT);
        HV_HIP(c, hipMemsetAsync(a.head, 0, head_bytes(n_images), c->stream));
        const unsigned grid = (unsigned)(a.tiles_x * a.tiles_y) * (unsigned)n_images;
        if (p->gfttBlockSize == 3) hipLaunchKernelGGL(legacy_response_kernel<1>, dim3(grid), dim3(256), 0, c->stream, a);
        else if (p->gfttBlockSize == 5) hipLaunchKernelGGL(legacy_response_kernel<2>, dim3(grid), dim3(256), 0, c->stream, a);
        else hipLaunchKernelGGL(legacy_response_kernel<3>, dim3(grid), dim3(256), 0, c->stream, a);
        HV_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(legacy_candidates_kernel, dim3(grid), dim3(256), 0, c->stream, a);
        HV_HIP(c, hipGetLastError());
    }
    ScopedKernelTime tm(c, HV_K_DETECT_TAIL);
    hipLaunchKernelGGL(legacy_select_kernel, dim3((unsigned)n_images), dim3(SEL_THREADS), select_lds(a.max_tracks), c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

}  // namespace

// the select kernel's dynamic-LDS limit, set once per context (never inside a launch that may be under capture)
int gftt_legacy_init(Ctx *c)
{
    HV_HIP(c, set_lds_limit(legacy_select_kernel, select_lds(HV_DETECT_TAIL_MAX_TRACKS)));
    return HV_OK;
}

}  // namespace hv

using hv::Ctx;

extern "C" {

void hv_gftt_legacy_default_params(hv_gftt_legacy_params *p)
{
    if (!p) return;
    p->gfttBlockSize = 3; p->gfttQualityLevel = 0.01; p->gfttMinDistance = 50.0; p->maxTracks = 200;   // parameter_definitions.c
}

void hv_gftt_legacy_tile_size(int *tile_w, int *tile_h)
{
    if (tile_w) *tile_w = hv::TW;
    if (tile_h) *tile_h = hv::TH;
}

double hv_gftt_legacy_min_distance(hv_ctx *ctx, const hv_gftt_legacy_params *p)
{
    if (!ctx || !p) return -1.0;
    return hv::min_distance(hv::ctx_of(ctx), p);
}

int hv_gftt_legacy_keypoint_bound(hv_ctx *ctx)
{
    if (!ctx) return HV_ERR_INVALID;
    return hv::keypoint_bound(hv::ctx_of(ctx));
}

size_t hv_gftt_legacy_work_bytes(hv_ctx *ctx, int n_images, int max_keypoints)
{
    if (!ctx || n_images <= 0 || max_keypoints < 0) return 0;
    return hv::work_bytes(hv::ctx_of(ctx), n_images, max_keypoints);
}

int hv_gftt_legacy_keypoints_batch_dev(hv_ctx *h, const hv_gftt_legacy_params *p, int n_images, const int *slots_dev, void *work_dev,
                                       int max_keypoints, int *n_cand_dev, int max_corners, float *corners_dev, float *resp_dev,
                                       int *n_out_dev)
{
    if (const int rc = hv::check_params(p)) return rc;
    if (n_images < 0 || max_keypoints < 0 || max_corners < 0) return HV_ERR_INVALID;
    if (n_images > 0 && (!slots_dev || !work_dev || !n_cand_dev || !n_out_dev || (max_corners > 0 && !corners_dev))) return HV_ERR_INVALID;
    if (max_corners < std::min(p->maxTracks, max_keypoints)) return HV_ERR_INVALID;
    if (const int rc = hv::check_limits(p, n_images, 0)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_images == 0) return HV_OK;
    return hv::launch(c, p, n_images, slots_dev, 0, work_dev, max_keypoints, n_cand_dev, 0, nullptr, nullptr, nullptr, max_corners,
                      corners_dev, resp_dev, n_out_dev);
}

int hv_gftt_legacy_detect_batch_dev(hv_ctx *h, const hv_gftt_legacy_params *p, int n_images, const int *slots_dev, void *work_dev,
                                    int max_keypoints, int *n_cand_dev, int max_prev, const int *n_prev_dev, const float *prev_dev,
                                    const int *mask_radius_dev, int max_corners, float *corners_dev, float *resp_dev, int *n_out_dev)
{
    if (const int rc = hv::check_params(p)) return rc;
    if (n_images < 0 || max_keypoints < 0 || max_prev < 0 || max_corners < 0) return HV_ERR_INVALID;
    if (n_images > 0 && (!slots_dev || !work_dev || !n_cand_dev || !mask_radius_dev || !n_out_dev || (max_corners > 0 && !corners_dev) ||
                         (max_prev > 0 && (!n_prev_dev || !prev_dev)))) return HV_ERR_INVALID;
    if (max_corners < std::min(p->maxTracks, max_keypoints)) return HV_ERR_INVALID;
    if (const int rc = hv::check_limits(p, n_images, max_prev)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_images == 0) return HV_OK;
    return hv::launch(c, p, n_images, slots_dev, 0, work_dev, max_keypoints, n_cand_dev, max_prev, n_prev_dev, prev_dev, mask_radius_dev,
                      max_corners, corners_dev, resp_dev, n_out_dev);
}

int hv_gftt_legacy_detect(hv_ctx *ctx, const hv_gftt_legacy_params *p, int slot, const float *prev_xy, int n_prev, int mask_radius,
                          float *corners_xy, int capacity, int *n_out)
{
    if (const int rc = hv::check_params(p)) return rc;
    if (!ctx || !corners_xy || !n_out || n_prev < 0 || (n_prev > 0 && !prev_xy) || capacity < 0 || mask_radius < 1) return HV_ERR_INVALID;
    if (const int rc = hv::check_limits(p, 1, n_prev)) return rc;
    Ctx *c = hv::ctx_of(ctx);
    if (slot < 0 || slot >= c->p.pool_size || !c->slot_used[slot]) return HV_ERR_POOL;
    const int bound = hv::keypoint_bound(c), cap = std::min(p->maxTracks, bound);
    if (capacity < cap) return HV_ERR_INVALID;
    *n_out = 0;
    if (bound == 0) return HV_OK;
    const int sizes[2] = {n_prev, mask_radius};
    int counts[2] = {0, 0};                                    // n_cand, n_out
    hv::Stage s(c);
    const auto o_sizes = s.in(sizes, 2);
    const auto o_prev = s.in(prev_xy, 2 * (size_t)n_prev);
    const auto o_counts = s.out(counts, 2);
    const auto o_work = s.take<unsigned char>(hv::work_bytes(c, 1, bound));
    const auto o_corners = s.take<float>(2 * (size_t)cap);
    int rc = s.upload();
    if (rc != HV_OK) return rc;
    rc = hv::launch(c, p, 1, nullptr, slot, s.at(o_work), bound, s.at(o_counts), n_prev, s.at(o_sizes), s.at_or_null(o_prev),
                    s.at(o_sizes) + 1, cap, s.at(o_corners), nullptr, s.at(o_counts) + 1);
    if (rc == HV_OK) rc = s.download();
    if (rc != HV_OK) return rc;
    if (counts[1] < 0) return HV_ERR_POOL;                     // the slot holds no image yet
    if (counts[1] > 0) {
        rc = s.fetch(corners_xy, o_corners, 2 * (size_t)counts[1]);
        if (rc == HV_OK) rc = s.sync();
        if (rc != HV_OK) return rc;
    }
    *n_out = counts[1];
    return HV_OK;
}

}  // extern "C"
