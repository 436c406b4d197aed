// FAST corner detector (featureDetector "FAST"): segment test, score, non-max suppression, track mask and the detect() tail, batched,
// no allocation and no synchronisation (capturable in a HIP graph).
//
// Reference: src/tracker/feature_detector_legacy.cpp:141-174 (CustomFastFeatureDetector: cv::FastFeatureDetector, FAST-9 on the
// 16-pixel circle, non-max suppression on), :20-51 and :70-83 (MaskedFeatureDetector::detect / setMask / drawMask: a box per live
// track, key points inside any box removed), :177-213 (applyMinDistance) and src/tracker/feature_detector.cpp:659-680
// (FeatureDetector::build). The rules are restated in tests/fast_restatement.py; everything is integer arithmetic up to the
// distance test of the walk, which is the one of detect_tail.hip (hv_min_distance.hpp).
//
// Two launches per call:
//   fast_score_kernel   one workgroup per HV_FAST_TILE_W x HV_FAST_TILE_H tile of one image. The gray tile with a 4-pixel halo (3
//       for the circle, 1 for the suppression) goes to LDS as bytes. A task is four pixels of a row of the tile or of its 1-pixel
//       ring: seven 12-byte row segments in registers serve their four circles, and two pixels at a time run side by side in
//       packed 16-bit arithmetic (v_perm_b32 picks a byte pair, v_pk_sub / min / max_i16 do the rest). Every pair takes the
//       4-point pre-test (k = 0, 4, 8, 12: an arc of 9 holds one of every opposite pair), and only where a lane of the wavefront
//       passes it does the wavefront run the 16-arc score (max over arcs of the min over the arc, by doubling: 2, 4, 8, 9, for
//       both signs); the scores go to LDS as bytes, a thread then suppresses four pixels against their 8 neighbours and writes
//       ONE dword of the score map (0 = no key point). The map is the only thing the kernel writes: w * h bytes per image.
//   fast_select_kernel  one workgroup per image, 16 wavefronts. <true> (detect): the boxes of the live tracks are zeroed in the
//       score map (the reference filters before it sorts, so this is its filter); every wavefront owns a contiguous row-major
//       range of the map and counts its key points per score in LDS; the bases of (score descending, wavefront ascending) are a
//       prefix sum; every wavefront then walks its range again, 256 pixels a step, in row-major lane order, and gives each key
//       point the next place of its score (the lanes of equal score found with 8 ballots, ranked by lane): a stable counting sort,
//       the order of std::stable_sort by descending response. The sorted key points go to kp_dev; then the ballot walk of
//       detect_tail.hip step 4 over them (no live tracks: applyMinDistance(corners, {}, maskRadius)), stopped at maxTracks: blocks
//       of 1024 candidates, all wavefronts against the corners accepted before the block, the first wavefront against those in it. <false> (key points only): one count per wavefront instead of one per score, which leaves row-major order.
#include "hv_internal.hpp"
#include "hv_min_distance.hpp"

#include <algorithm>

namespace hv {
namespace {

constexpr int TW = HV_FAST_TILE_W, TH = HV_FAST_TILE_H;
constexpr int GP = TW + 16, GH = TH + 8;          // gray tile: column c <-> image x0 - 4 + c, row r <-> y0 - 4 + r (pitch: 12-byte reads up to c + 11)
constexpr int SP = TW + 8, SH = TH + 2;           // score tile: column c <-> x0 - 1 + c, row r <-> y0 - 1 + r (pitch: dword reads up to c + 7)
static_assert(TW % 4 == 0 && TW * TH == 4 * 256 && GP % 4 == 0, "a thread suppresses four pixels; dword staging");
constexpr int SEL_THREADS = 1024, SEL_WAVES = SEL_THREADS / 64;
// pixels of an image the select kernel serves: a queue entry holds a pixel index within a wavefront's range (1 / 16 of the map)
// in 24 bits, and the box tasks of an image are counted in an int (launch() refuses larger contexts)
constexpr long long MAX_PIXELS = 1ll << 27;
constexpr int QUEUE = 256;                        // key points a wavefront's queue holds: 63 left over + the 128 of a step fit
static_assert(SEL_WAVES * QUEUE * sizeof(uint32_t) >= SEL_THREADS * sizeof(float2), "the walk reuses the queues' LDS");

struct FastArgs {
    const uint8_t *const *l0_ptr;     // per-slot level-0 image table (filled by the pyramid build)
    const int *l0_stride;
    const int *slots;                 // [n_images], or null: the single image slot0
    int slot0, pool_size;
    int w, h, tiles_x, tiles_y, threshold;
    int sstride;                      // bytes per row of a score map: w rounded up to 4
    unsigned char *work;              // [n_images][work_stride]
    size_t work_stride;
    // select only
    int max_keypoints; float *kp; int *n_kp;
    int max_prev; const int *n_prev; const float *prev; const int *radius;
    int max_tracks, max_corners; float *corners; int *n_out;
};

__device__ __forceinline__ const uint8_t *image_of(const FastArgs &a, int img, int *stride)
{
    const int slot = a.slots ? a.slots[img] : a.slot0;
    if (slot < 0 || slot >= a.pool_size) return nullptr;                // not a slot
    *stride = a.l0_stride[slot];
    return a.l0_ptr[slot];                                              // null: a slot no pyramid was built in
}

typedef short short2v __attribute__((ext_vector_type(2)));            // two pixels' values side by side (v_pk_*_i16)
__device__ __forceinline__ short2v pk_min(short2v a, short2v b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ short2v pk_max(short2v a, short2v b) { return __builtin_elementwise_max(a, b); }

// DARK: max over the 16 arcs of 9 consecutive circle pixels of the min over the arc; else the min over the arcs of the max (the
// bright sign, negated). By doubling: arcs of 2, 4, 8, then 8 + 1.
template <bool DARK>
__device__ __forceinline__ short2v arc9(const short2v (&d)[16])
{
    auto in = [](short2v a, short2v b) { return DARK ? pk_min(a, b) : pk_max(a, b); };
    auto over = [](short2v a, short2v b) { return DARK ? pk_max(a, b) : pk_min(a, b); };
    short2v m2[16], m4[16], m8[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) m2[k] = in(d[k], d[(k + 1) & 15]);
#pragma unroll
    for (int k = 0; k < 16; ++k) m4[k] = in(m2[k], m2[(k + 2) & 15]);
#pragma unroll
    for (int k = 0; k < 16; ++k) m8[k] = in(m4[k], m4[(k + 4) & 15]);
    short2v best = in(m8[0], d[8]);
#pragma unroll
    for (int k = 1; k < 16; ++k) best = over(best, in(m8[k], d[(k + 8) & 15]));
    return best;
}

// bytes i and i + 1 of a 12-byte row segment as two 16-bit values (one v_perm_b32; selector byte 0x0c reads as zero)
__device__ __forceinline__ short2v pair_at(const uint32_t (&row)[3], int i)
{
    const int j = i + 1 <= 7 ? i : i - 4;
    const uint32_t sel = (uint32_t)j | 0x0c00u | ((uint32_t)(j + 1) << 16) | 0x0c000000u;
    const uint32_t v = i + 1 <= 7 ? __builtin_amdgcn_perm(row[1], row[0], sel) : __builtin_amdgcn_perm(row[2], row[1], sel);
    return __builtin_bit_cast(short2v, v);
}

// (dx, dy) of circle pixel k
__device__ constexpr int CDX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
__device__ constexpr int CDY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};

__global__ __launch_bounds__(256) void fast_score_kernel(FastArgs a)
{
    __shared__ __align__(16) uint8_t gray[GH * GP];
    __shared__ __align__(16) uint8_t sc[SH * SP];
    const int t = threadIdx.x;
    const int tiles = a.tiles_x * a.tiles_y;
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);               // neighbouring tiles share halo rows: one XCD's L2
    const int img = lb / tiles, ti = lb - img * tiles;
    const int tyi = ti / a.tiles_x, txi = ti - tyi * a.tiles_x;
    const int x0 = txi * TW, y0 = tyi * TH, w = a.w, h = a.h;
    int stride = 0;
    const uint8_t *src = image_of(a, img, &stride);
    if (!src) return;                                                   // (the select kernel reports the image)

    // ---- the gray tile, a dword per task; outside the image 0 (never read by a pixel that can be a corner)
    for (int e = t; e < GH * (GP / 4); e += 256) {
        const int r = e / (GP / 4), g = e - r * (GP / 4);
        const int gy = y0 - 4 + r, gx = x0 - 4 + 4 * g;
        uint32_t v = 0;
        if (gy >= 0 && gy < h) {
            const uint8_t *p = src + (size_t)gy * stride;
            if (gx >= 0 && gx + 3 < w) __builtin_memcpy(&v, p + gx, 4);
            else {
#pragma unroll
                for (int k = 0; k < 4; ++k) if (gx + k >= 0 && gx + k < w) v |= (uint32_t)p[gx + k] << (8 * k);
            }
        }
        *reinterpret_cast<uint32_t *>(gray + r * GP + 4 * g) = v;
    }
    __syncthreads();

    // ---- scores of the tile and its 1-pixel ring: a task is four pixels of a row, two packed pairs; seven 12-byte row segments
    // of the gray tile in registers serve all four circles
    const int thr = a.threshold;
    constexpr int SG = (TW + 2 + 3) / 4;                                // tasks per score row
    for (int e = t; e < SH * SG; e += 256) {
        const int r = e / SG, cx = (e - r * SG) * 4;
        const int x = x0 - 1 + cx, y = y0 - 1 + r;
        uint32_t rows[7][3];                                            // gray rows y - 3 .. y + 3, columns x - 3 .. x + 8
#pragma unroll
        for (int dy = 0; dy < 7; ++dy) {
            const uint32_t *g = reinterpret_cast<const uint32_t *>(gray + (r + dy) * GP + cx);
            rows[dy][0] = g[0]; rows[dy][1] = g[1]; rows[dy][2] = g[2];
        }
        const bool row_ok = y >= 3 && y <= h - 4;
        uint32_t packed = 0;
#pragma unroll
        for (int pb = 0; pb < 4; pb += 2) {                             // pixels x + pb and x + pb + 1
            const bool ok0 = row_ok && x + pb >= 3 && x + pb <= w - 4, ok1 = row_ok && x + pb + 1 >= 3 && x + pb + 1 <= w - 4;
            const short2v v = pair_at(rows[3], 3 + pb);
            short2v d[16];
#pragma unroll
            for (int k = 0; k < 16; k += 4) d[k] = v - pair_at(rows[3 + CDY[k]], 3 + pb + CDX[k]);
            // 4-point pre-test: an arc of 9 holds one of every opposite pair
            const short2v dk = pk_min(pk_max(d[0], d[8]), pk_max(d[4], d[12])), br = pk_max(pk_min(d[0], d[8]), pk_min(d[4], d[12]));
            const bool cand = (ok0 && (dk.x > thr || br.x < -thr)) || (ok1 && (dk.y > thr || br.y < -thr));
            if (cand) {                                                 // (a wavefront none of whose lanes passes skips this)
#pragma unroll
                for (int k = 0; k < 16; ++k) if (k & 3) d[k] = v - pair_at(rows[3 + CDY[k]], 3 + pb + CDX[k]);
                const short2v zero = {0, 0};
                const short2v mm = pk_max(arc9<true>(d), zero - arc9<false>(d));   // the largest threshold that still passes, plus 1
                const int s0 = ok0 && mm.x > thr ? mm.x - 1 : 0, s1 = ok1 && mm.y > thr ? mm.y - 1 : 0;
                packed |= ((uint32_t)s0 | ((uint32_t)s1 << 8)) << (8 * pb);
            }
        }
        *reinterpret_cast<uint32_t *>(sc + r * SP + cx) = packed;
    }
    __syncthreads();

    // ---- non-max suppression: strictly greater than all 8 neighbours; four pixels, one dword of the map, per thread
    const int row = t / (TW / 4), x4 = (t - row * (TW / 4)) * 4;
    const int y = y0 + row, x = x0 + x4;
    if (y < h && x < a.sstride) {
        unsigned long long rw[3];
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
            const uint32_t *p = reinterpret_cast<const uint32_t *>(sc + (row + rr) * SP + x4);
            rw[rr] = (unsigned long long)p[0] | ((unsigned long long)p[1] << 32);      // columns x - 1 .. x + 6
        }
        auto at = [&](int rr, int j) { return (int)((rw[rr] >> (8 * j)) & 0xFFu); };
        uint32_t out = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int s = at(1, k + 1);
            const int nb = max(max(max(at(0, k), at(0, k + 1)), max(at(0, k + 2), at(1, k))),
                               max(max(at(1, k + 2), at(2, k)), max(at(2, k + 1), at(2, k + 2))));
            if (s > nb) out |= (uint32_t)s << (8 * k);
        }
        unsigned char *map = a.work + (size_t)img * a.work_stride;
        *reinterpret_cast<uint32_t *>(map + (size_t)y * a.sstride + x) = out;
    }
}

// LDS: static s_cnt [wave][score] (detect) or [wave][0] (key points only) | dynamic float2 list[max(max_prev, max_tracks)] (the live
// tracks while their boxes are drawn, then the accepted corners)
template <bool DETECT>
__global__ __launch_bounds__(SEL_THREADS) void fast_select_kernel(FastArgs a)
{
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ int s_cnt[SEL_WAVES][256];
    __shared__ int s_tot[256];
    __shared__ int s_total;
    // the scatter's per-wavefront queues of 256 packed key points (ring buffers); afterwards the walk's block of candidates
    __shared__ __align__(8) uint32_t s_buf[SEL_WAVES * QUEUE];
    float2 *s_xy = reinterpret_cast<float2 *>(s_buf);          // [SEL_THREADS]: the walk: a block's candidates ...
    __shared__ unsigned long long s_live[SEL_WAVES];           // ... and which of them no earlier corner rejects
    float2 *list = reinterpret_cast<float2 *>(lds);
    const int set = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = a.w, h = a.h, sstride = a.sstride;

    int stride = 0;
    const bool image = image_of(a, set, &stride) != nullptr;
    const int r = DETECT ? a.radius[set] : 1;
    if (!image || r < 1) {                                     // no such slot, or a radius the reference asserts on: nothing but the flags
        if (tid == 0) { a.n_kp[set] = -1; if (DETECT) a.n_out[set] = -1; }
        return;
    }
    unsigned char *map = a.work + (size_t)set * a.work_stride;

    for (int i = tid; i < SEL_WAVES * 256; i += SEL_THREADS) (&s_cnt[0][0])[i] = 0;
    if (DETECT) {
        // drawMask: a box per live track inside the image, upper ends exclusive
        const int n_prev = (a.n_prev && a.max_prev > 0) ? min(max(a.n_prev[set], 0), a.max_prev) : 0;
        for (int i = tid; i < n_prev; i += SEL_THREADS) {
            const float *p = a.prev + ((size_t)set * a.max_prev + i) * 2;
            list[i] = make_float2(p[0], p[1]);
        }
        __syncthreads();
        for (int i = 0; i < n_prev; ++i) {
            const float px = list[i].x, py = list[i].y;
            if (!(0.f < px && px < (float)w && 0.f < py && py < (float)h)) continue;      // (NaN draws nothing)
            const long long ix = (int)px, iy = (int)py;
            const int xa = (int)max(ix - r, 0ll), xb = (int)min(ix + r, (long long)w - 1);
            const int ya = (int)max(iy - r, 0ll), yb = (int)min(iy + r, (long long)h - 1);
            if (xb <= xa || yb <= ya) continue;
            // a row of the box is the aligned dwords it covers whole (one store each) and up to three bytes at either end (byte
            // stores: a zero is written whoever writes it, so overlapping boxes need no order); a row takes the next power of two
            // of dword slots, so that row and slot of a task are a shift and a mask (rows * slots < 2 w h / 4: MAX_PIXELS)
            const int d0 = xa >> 2, nd = ((xb - 1) >> 2) - d0 + 1;
            const int sh = nd > 1 ? 32 - __clz(nd - 1) : 0;
            for (int e = tid; e < ((yb - ya) << sh); e += SEL_THREADS) {
                const int dd = e & ((1 << sh) - 1);
                if (dd >= nd) continue;
                unsigned char *row = map + (size_t)(ya + (e >> sh)) * sstride;
                const int bx = (d0 + dd) * 4;
                if (bx >= xa && bx + 4 <= xb) *reinterpret_cast<uint32_t *>(row + bx) = 0u;
                else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) if (bx + k >= xa && bx + k < xb) row[bx + k] = 0;
                }
            }
        }
    }
    __syncthreads();                                           // the counters are zero, the boxes are drawn

    // ---- per wavefront: a contiguous row-major range of the map's dwords, counted per score
    const uint32_t *m32 = reinterpret_cast<const uint32_t *>(map);
    const int ndw = (sstride / 4) * h;
    const int seg = ((ndw + SEL_WAVES - 1) / SEL_WAVES + 63) / 64 * 64;
    const int beg = min(wave * seg, ndw), end = min(beg + seg, ndw);
    for (int i0 = beg + lane; i0 < end; i0 += 4 * 64) {          // four loads in flight
        uint32_t v4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v4[q] = i0 + 64 * q < end ? m32[i0 + 64 * q] : 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t v = v4[q];
            if (v == 0) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int b = (v >> (8 * k)) & 0xFFu;
                if (b) atomicAdd(&s_cnt[wave][DETECT ? b : 0], 1);
            }
        }
    }
    __syncthreads();
    if (tid < 256) {
        int tot = 0;
        for (int wv = 0; wv < SEL_WAVES; ++wv) tot += s_cnt[wv][tid];
        s_tot[tid] = tot;
    }
    __syncthreads();
    if (tid < 256) {
        int start = 0;                                         // key points of a higher score come first
        for (int s = tid + 1; s < 256; ++s) start += s_tot[s];
        if (tid == 0) s_total = start + s_tot[0];
        for (int wv = 0; wv < SEL_WAVES; ++wv) { const int c = s_cnt[wv][tid]; s_cnt[wv][tid] = start; start += c; }
    }
    __syncthreads();
    const int n = s_total;
    if (n > a.max_keypoints) {                                 // never truncated: the sort would pick other corners
        if (tid == 0) { a.n_kp[set] = -1; if (DETECT) a.n_out[set] = -1; }
        return;
    }

    // ---- scatter. A step reads 256 pixels; lane l of sub-step j holds pixel 64 j + l of them, so appending the non-zero ones of
    // sub-steps 0 .. 3 in lane order to the wavefront's queue keeps row-major order (an entry: pixel index within the wavefront's
    // range << 8 | score; at most every second pixel is a key point). Whenever 64 are queued they are placed: the lanes of equal
    // score are found with 8 ballots and ranked by lane, the last of them moves the score's counter on. The sparse part costs a
    // few instructions per sub-step; the placing runs on full wavefronts.
    // The queue and the counters are read and written through volatile pointers, in program order: LDS operations of one
    // wavefront complete in issue order, so no fence (which would also wait for the key-point stores in flight) is needed.
    float *kp = a.kp + (size_t)set * a.max_keypoints * 3;
    const unsigned long long lt = (1ull << lane) - 1ull;
    volatile int *cnt = s_cnt[wave];
    volatile uint32_t *queue = s_buf + wave * QUEUE;
    int head = 0, tail = 0;                                    // (uniform in the wavefront)
    auto place = [&](int count) {                              // the first `count` <= 64 queued key points
        const bool has = lane < count;
        const uint32_t ent = has ? queue[(head + lane) & (QUEUE - 1)] : 0u;
        head += count;
        const int b = ent & 0xFFu, key = DETECT ? b : 0;
        unsigned long long peers = __ballot(has);              // the lanes with this lane's score
        if (DETECT) {
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool one = (key >> bit) & 1;
                const unsigned long long bb = __ballot(has && one);
                peers &= one ? bb : ~bb;
            }
        }
        int pos = 0;
        if (has) pos = cnt[key] + __popcll(peers & lt);
        __builtin_amdgcn_wave_barrier();
        if (has && (peers >> lane) == 1ull) cnt[key] = pos + 1;                  // the last lane of a score moves its counter on
        __builtin_amdgcn_wave_barrier();
        if (has) {
            const int p = beg * 4 + (int)(ent >> 8);
            const int y = p / sstride, x = p - y * sstride;
            float *o = kp + (size_t)pos * 3;
            o[0] = (float)x; o[1] = (float)y; o[2] = (float)b;
        }
    };
    for (int base = beg; base < end; base += 64) {
        const int i = base + lane;
        const uint32_t v = i < end ? m32[i] : 0u;
        if (__ballot(v != 0) == 0) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t word = __shfl(v, 16 * j + (lane >> 2));
            const uint32_t b = (word >> (8 * (lane & 3))) & 0xFFu;
            const unsigned long long bal = __ballot(b != 0);
            if (b != 0) queue[(tail + __popcll(bal & lt)) & (QUEUE - 1)] = ((uint32_t)((base - beg) * 4 + 64 * j + lane) << 8) | b;
            tail += __popcll(bal);
        }
        __builtin_amdgcn_wave_barrier();
        while (tail - head >= 64) place(64);
    }
    __builtin_amdgcn_wave_barrier();
    while (tail - head > 0) place(min(tail - head, 64));
    if (tid == 0) a.n_kp[set] = n;
    if (!DETECT) return;
    __syncthreads();                                           // the sorted key points are written (workgroup scope)

    // ---- the greedy walk (detect_tail.hip step 4) over blocks of SEL_THREADS candidates; list[] now holds the accepted corners.
    // Every thread first tests its candidate against the corners accepted before the block (all wavefronts, the list is only read);
    // the first wavefront then walks the block's 16 chunks in order, testing the survivors against the corners accepted inside the
    // block only, with one ballot per accepted corner. Most candidates die in the parallel part; the serial part is what the
    // sequential filter's order needs. The first wavefront reads and writes the list through a volatile pointer, in program order
    // (LDS operations of one wavefront complete in issue order): the fences of detect_tail.hip's walk would also wait for the
    // corner stores in flight.
    volatile float *acc = reinterpret_cast<volatile float *>(list);
    const float r2 = (float)(r * r);
    float *out = a.corners + (size_t)set * a.max_corners * 2;
    int n_acc = 0;
    for (int base = 0; base < n && n_acc < a.max_tracks; base += SEL_THREADS) {
        const int i = base + tid;
        bool live = i < n;
        float x = 0.0f, y = 0.0f;
        if (live) { x = kp[3 * (size_t)i]; y = kp[3 * (size_t)i + 1]; }
#pragma unroll 8
        for (int j = 0; j < n_acc; ++j) {
            const float2 c = list[j];
            if (within(c.x, c.y, x, y, r2)) live = false;
        }
        s_xy[tid] = make_float2(x, y);
        const unsigned long long alive = __ballot(live);
        if (lane == 0) s_live[wave] = alive;
        __syncthreads();
        if (wave == 0) {
            const int n0 = n_acc;
            for (int c = 0; c < SEL_WAVES && n_acc < a.max_tracks; ++c) {
                const unsigned long long m = s_live[c];
                if (m == 0) continue;
                bool lv = (m >> lane) & 1ull;
                const float2 q = s_xy[c * 64 + lane];
                __builtin_amdgcn_wave_barrier();
                for (int j = n0; j < n_acc; ++j) if (within(acc[2 * j], acc[2 * j + 1], q.x, q.y, r2)) lv = false;
                while (true) {
                    const unsigned long long b = __ballot(lv);
                    if (b == 0) break;
                    const int lead = __ffsll((long long)b) - 1;
                    const float ax = __shfl(q.x, lead), ay = __shfl(q.y, lead);
                    if (lane == lead) {
                        acc[2 * n_acc] = ax; acc[2 * n_acc + 1] = ay;
                        out[2 * n_acc] = ax; out[2 * n_acc + 1] = ay;
                        lv = false;
                    }
                    ++n_acc;
                    if (n_acc >= a.max_tracks) break;
                    if (lv && within(ax, ay, q.x, q.y, r2)) lv = false;
                }
            }
            if (lane == 0) s_total = n_acc;
        }
        __syncthreads();
        n_acc = s_total;
    }
    if (tid == 0) a.n_out[set] = n_acc;
}

int sstride_of(const Ctx *c) { return (c->L.w[0] + 3) & ~3; }
size_t map_bytes(const Ctx *c) { return ((size_t)sstride_of(c) * c->L.h[0] + 15) & ~(size_t)15; }
int keypoint_bound(const Ctx *c)
{
    const int w = c->L.w[0], h = c->L.h[0];
    return (w < 7 || h < 7) ? 0 : ((w - 6 + 1) / 2) * ((h - 6 + 1) / 2);
}
size_t select_lds(int max_prev, int max_tracks) { return sizeof(float) * 2 * (size_t)std::max(std::max(max_prev, max_tracks), 1); }

// the checks the entries share, made before the context is looked at
int check_params(const hv_fast_params *p)
{
    if (!p || p->maxTracks < 1 || p->threshold < 0 || p->threshold > 255) return HV_ERR_INVALID;
    return HV_OK;
}

// both launches, on the context stream; slots_dev null: the single image slot0
int launch(Ctx *c, const hv_fast_params *p, bool detect, int n_images, const int *slots_dev, int slot0, void *work_dev, int max_keypoints,
           float *kp_dev, int *n_kp_dev, int max_prev, const int *n_prev_dev, const float *prev_dev, const int *radius_dev,
           int max_corners, float *corners_dev, int *n_out_dev)
{
    if (((long long)sstride_of(c) + 256) * c->L.h[0] > MAX_PIXELS) return HV_ERR_UNSUPPORTED;      // (a 2^27-pixel image: 11 585 squared)
    FastArgs a{};
    a.l0_ptr = c->d_l0_ptr; a.l0_stride = c->d_l0_stride; a.slots = slots_dev; a.slot0 = slot0; a.pool_size = c->p.pool_size;
    a.w = c->L.w[0]; a.h = c->L.h[0];
    a.tiles_x = (a.w + TW - 1) / TW; a.tiles_y = (a.h + TH - 1) / TH;
    a.threshold = p->threshold; a.sstride = sstride_of(c);
    a.work = static_cast<unsigned char *>(work_dev); a.work_stride = map_bytes(c);
    a.max_keypoints = max_keypoints; a.kp = kp_dev; a.n_kp = n_kp_dev;
    a.max_prev = max_prev; a.n_prev = n_prev_dev; a.prev = prev_dev; a.radius = radius_dev;
    a.max_tracks = std::min(p->maxTracks, std::max(max_keypoints, 1)); a.max_corners = max_corners;
    a.corners = corners_dev; a.n_out = n_out_dev;
    {
        ScopedKernelTime tm(c, HV_K_GFTT);
        const unsigned grid = (unsigned)(a.tiles_x * a.tiles_y) * (unsigned)n_images;
        hipLaunchKernelGGL(fast_score_kernel, dim3(grid), dim3(256), 0, c->stream, a);
        HV_HIP(c, hipGetLastError());
    }
    ScopedKernelTime tm(c, HV_K_DETECT_TAIL);
    if (detect)
        hipLaunchKernelGGL(fast_select_kernel<true>, dim3((unsigned)n_images), dim3(SEL_THREADS), select_lds(max_prev, a.max_tracks),
                           c->stream, a);
    else
        hipLaunchKernelGGL(fast_select_kernel<false>, dim3((unsigned)n_images), dim3(SEL_THREADS), select_lds(0, 0), c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

}  // namespace

// the select kernel's dynamic-LDS limit, set once per context (never inside a launch that may be under capture)
int fast_init(Ctx *c)
{
    const size_t cap = select_lds(HV_DETECT_TAIL_MAX_PREV, HV_DETECT_TAIL_MAX_TRACKS);
    HV_HIP(c, set_lds_limit(fast_select_kernel<true>, cap));
    HV_HIP(c, set_lds_limit(fast_select_kernel<false>, cap));
    return HV_OK;
}

}  // namespace hv

using hv::Ctx;

extern "C" {

void hv_fast_default_params(hv_fast_params *p)
{
    if (!p) return;
    p->threshold = 10; p->maxTracks = 200;              // cv::FastFeatureDetector::create(); parameter_definitions.c:262
}

void hv_fast_tile_size(int *tile_w, int *tile_h)
{
    if (tile_w) *tile_w = hv::TW;
    if (tile_h) *tile_h = hv::TH;
}

int hv_fast_keypoint_bound(hv_ctx *ctx)
{
    if (!ctx) return HV_ERR_INVALID;
    return hv::keypoint_bound(hv::ctx_of(ctx));
}

size_t hv_fast_work_bytes(hv_ctx *ctx, int n_images)
{
    if (!ctx || n_images <= 0) return 0;
    return hv::map_bytes(hv::ctx_of(ctx)) * (size_t)n_images;
}

int hv_fast_keypoints_batch_dev(hv_ctx *h, const hv_fast_params *p, int n_images, const int *slots_dev, void *work_dev,
                                int max_keypoints, float *kp_dev, int *n_kp_dev)
{
    if (const int rc = hv::check_params(p)) return rc;
    if (n_images < 0 || max_keypoints < 0) return HV_ERR_INVALID;
    if (n_images > 0 && (!slots_dev || !work_dev || !n_kp_dev || (max_keypoints > 0 && !kp_dev))) return HV_ERR_INVALID;
    if (n_images > 65535 || p->maxTracks > HV_DETECT_TAIL_MAX_TRACKS) return HV_ERR_UNSUPPORTED;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_images == 0) return HV_OK;
    return hv::launch(c, p, false, n_images, slots_dev, 0, work_dev, max_keypoints, kp_dev, n_kp_dev, 0, nullptr, nullptr, nullptr, 0,
                      nullptr, nullptr);
}

int hv_fast_detect_batch_dev(hv_ctx *h, const hv_fast_params *p, int n_images, const int *slots_dev, void *work_dev, int max_keypoints,
                             float *kp_dev, int *n_kp_dev, int max_prev, const int *n_prev_dev, const float *prev_dev,
                             const int *mask_radius_dev, int max_corners, float *corners_dev, int *n_out_dev)
{
    if (const int rc = hv::check_params(p)) return rc;
    if (n_images < 0 || max_keypoints < 0 || max_prev < 0 || max_corners < 0) return HV_ERR_INVALID;
    if (n_images > 0 && (!slots_dev || !work_dev || !n_kp_dev || (max_keypoints > 0 && !kp_dev) || !mask_radius_dev || !n_out_dev ||
                         (max_corners > 0 && !corners_dev) || (max_prev > 0 && (!n_prev_dev || !prev_dev)))) return HV_ERR_INVALID;
    if (max_corners < std::min(p->maxTracks, max_keypoints)) return HV_ERR_INVALID;
    if (n_images > 65535 || max_prev > HV_DETECT_TAIL_MAX_PREV || p->maxTracks > HV_DETECT_TAIL_MAX_TRACKS) return HV_ERR_UNSUPPORTED;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_images == 0) return HV_OK;
    return hv::launch(c, p, true, n_images, slots_dev, 0, work_dev, max_keypoints, kp_dev, n_kp_dev, max_prev, n_prev_dev, prev_dev,
                      mask_radius_dev, max_corners, corners_dev, n_out_dev);
}

int hv_fast_detect(hv_ctx *ctx, const hv_fast_params *p, int slot, const float *prev_xy, int n_prev, int mask_radius,
                   float *corners_xy, int capacity, int *n_out)
{
    if (const int rc = hv::check_params(p)) return rc;
    if (!ctx || !corners_xy || !n_out || n_prev < 0 || (n_prev > 0 && !prev_xy) || capacity < 0 || mask_radius < 1) return HV_ERR_INVALID;
    if (n_prev > HV_DETECT_TAIL_MAX_PREV || p->maxTracks > HV_DETECT_TAIL_MAX_TRACKS) return HV_ERR_UNSUPPORTED;
    Ctx *c = hv::ctx_of(ctx);
    if (slot < 0 || slot >= c->p.pool_size || !c->slot_used[slot]) return HV_ERR_POOL;
    const int bound = hv::keypoint_bound(c), cap = std::min(p->maxTracks, bound);
    if (capacity < cap) return HV_ERR_INVALID;
    *n_out = 0;
    if (bound == 0) return HV_OK;
    const int sizes[2] = {n_prev, mask_radius};
    int counts[2] = {0, 0};                                    // n_kp, n_out
    hv::Stage s(c);
    const auto o_sizes = s.in(sizes, 2);
    const auto o_prev = s.in(prev_xy, 2 * (size_t)n_prev);
    const auto o_counts = s.out(counts, 2);
    const auto o_work = s.take<unsigned char>(hv::map_bytes(c));
    const auto o_kp = s.take<float>(3 * (size_t)bound);
    const auto o_corners = s.take<float>(2 * (size_t)cap);
    int rc = s.upload();
    if (rc != HV_OK) return rc;
    rc = hv::launch(c, p, true, 1, nullptr, slot, s.at(o_work), bound, s.at(o_kp), s.at(o_counts), n_prev, s.at(o_sizes),
                    s.at_or_null(o_prev), s.at(o_sizes) + 1, cap, s.at(o_corners), s.at(o_counts) + 1);
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
