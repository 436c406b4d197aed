// Device tail of FeatureDetector::detect and FeatureDetector::applyMinDistance, batched: one workgroup per set, everything in LDS,
// no allocation and no synchronisation (capturable in a HIP graph).
//
// Reference: src/tracker/feature_detector.cpp:624-633 (std::stable_sort of the key points by descending response, corners.resize(n)
// followed by push_back: n points (0, 0) in front of the n sorted ones, applyMinDistance when maskRadius > 0) and
// src/tracker/feature_detector_legacy.cpp:177-213 (applyMinDistance: greedy, in order, against the live tracks and the corners
// kept so far, stopped at maxTracks). The host form of the same tail is hv_gftt_detect / hv_apply_min_distance (gftt.hip).
//
// detect_tail_kernel<true> (hv_gftt_corners_batch_dev), per image:
//   1. key (descending response, ascending block index) per key point: the response's bits mapped monotonically to an unsigned
//      word, -0.0 first made +0.0 (equal under the reference's comparator `a.response > b.response`, so equal here), inverted; the
//      block index is the tie-break, which is what a stable sort of the block raster order gives. The pairs are distinct, so any
//      correct sort gives the one order: up to 1024 key points a rank sort (a thread counts the pairs below its own), beyond that a
//      bitonic network in LDS over the next power of two, padded with keys that sort last.
//   2. the zero prefix: with radius > 0 the n points (0, 0) are ONE candidate -- when the first is kept every later one is within
//      the radius of it (0 < r * r), when a live track rejects it the same track rejects them all.
//   3. every candidate against the set's live tracks, all threads; the survivors are compacted in order, in place (a write never
//      passes the chunk being read).
//   4. the first wavefront walks the survivors in chunks of 64: each lane tests its candidate against the accepted list in LDS;
//      then one ballot per accepted corner -- the lowest live lane IS the next corner the sequential filter keeps (every earlier
//      candidate has been decided), its coordinates are broadcast and the lanes within the radius of it drop out. The walk stops
//      when maxTracks corners are accepted, as the reference's `nOut >= maxTracks` after every corner does. Serial steps: accepted
//      corners + chunks, not candidates.
// detect_tail_kernel<false> (hv_apply_min_distance_batch_dev): steps 3 and 4 on a caller's list, in place (an accepted corner is
// written at an index not above its own, and the chunk it belongs to is in registers by then).
// The distance test is the reference's binary32 expression, two rounded products and one rounded sum, strict `<` against
// (float)(r * r): the library is built with -ffp-contract=off and the function (hv_min_distance.hpp) also switches contraction off itself.
#include "hv_internal.hpp"
#include "hv_min_distance.hpp"

#include <algorithm>

namespace hv {
namespace {

constexpr int DT_MAX_THREADS = 1024;
constexpr int DT_MAX_WAVES = DT_MAX_THREADS / 64;
constexpr int DT_RANK_SORT_MAX = 1024;            // key points up to which the rank sort serves (the bitonic network beyond)

struct TailArgs {
    int nk;                      // sorted form: key points per image; list form: max_corners
    int pow2;                    // sorted form: the bitonic size (>= nk)
    int max_prev, max_tracks, max_corners;
    const float *kp;             // sorted form: [sets][nk][3]
    const int *n_corners;        // list form: [sets]
    float *corners;              // [sets][max_corners][2]: list form in / out, sorted form out
    const int *n_prev;           // [sets] (NULL: none)
    const float *prev;           // [sets][max_prev][2]
    const int *radius;           // [sets]
    int *n_out;                  // [sets]
};

// within() (the distance test, shared with fast.hip) and wave_sync(): hv_min_distance.hpp

// descending response, ties (-0.0 == +0.0 included) equal
__device__ __forceinline__ uint32_t response_key(float r)
{
    if (r == 0.0f) r = 0.0f;
    const uint32_t b = __float_as_uint(r);
    const uint32_t up = (b & 0x80000000u) ? ~b : (b | 0x80000000u);      // ascending with the value
    return ~up;
}

// LDS: [uint32 key[pow2]] (sorted form) | float2 list[max(max_prev, max_tracks)] (live tracks, then the accepted corners) |
// uint16 cand[pow2 or max_corners] (candidate ids in order, then the survivors)
template <bool SORTED>
__global__ __launch_bounds__(DT_MAX_THREADS) void detect_tail_kernel(TailArgs a)
{
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ int s_wave[2][DT_MAX_WAVES];
    __shared__ int s_flag;
    const int set = blockIdx.x, tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, waves = T >> 6;
    const int list_cap = max(a.max_prev, a.max_tracks);
    uint32_t *key = reinterpret_cast<uint32_t *>(lds);
    float2 *list = reinterpret_cast<float2 *>(lds + (SORTED ? sizeof(uint32_t) * (size_t)a.pow2 : 0));
    uint16_t *cand = reinterpret_cast<uint16_t *>(reinterpret_cast<unsigned char *>(list) + sizeof(float2) * (size_t)list_cap);

    const int r = a.radius[set];
    const int n_prev = (a.n_prev && a.max_prev > 0) ? min(max(a.n_prev[set], 0), a.max_prev) : 0;
    const float *src = SORTED ? a.kp + (size_t)set * a.nk * 3 : a.corners + (size_t)set * a.max_corners * 2;
    float *out = a.corners + (size_t)set * a.max_corners * 2;
    const int n = SORTED ? a.nk : min(max(a.n_corners[set], 0), a.max_corners);
    constexpr int STRIDE = SORTED ? 3 : 2;

    if (!SORTED && r <= 0) {                                   // nothing is filtered: the first min(n, maxTracks) stay where they are
        if (tid == 0) a.n_out[set] = min(n, a.max_tracks);
        return;
    }
    if (SORTED && r <= 0 && a.max_corners < 2 * a.nk) {        // all 2 nk points would be due: no room (the documented error flag)
        if (tid == 0) a.n_out[set] = -1;
        return;
    }

    if (SORTED) {
        for (int i = tid; i < a.pow2; i += T) {
            key[i] = i < n ? response_key(src[3 * i + 2]) : 0xFFFFFFFFu;
            cand[i] = i < n ? (uint16_t)i : (uint16_t)0xFFFFu;
        }
        __syncthreads();
        if (n <= DT_RANK_SORT_MAX) {
            // few key points: the rank of an element among the distinct (key, index) pairs is its place -- n independent broadcast
            // reads per thread instead of log2(P) (log2(P) + 1) / 2 dependent exchange stages
            for (int i = tid; i < n; i += T) {
                const uint32_t ki = key[i];
                int rank = 0;
                for (int j = 0; j < a.pow2; j += 4) {              // (pow2 >= 4; the padding keys are never below a real one)
                    const uint4 q = *reinterpret_cast<const uint4 *>(key + j);
                    rank += (q.x < ki || (q.x == ki && j < i)) + (q.y < ki || (q.y == ki && j + 1 < i)) +
                            (q.z < ki || (q.z == ki && j + 2 < i)) + (q.w < ki || (q.w == ki && j + 3 < i));
                }
                cand[rank] = (uint16_t)i;
            }
            __syncthreads();
        } else
        for (int k = 2; k <= a.pow2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (a.pow2 >> 1); t += T) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                    const uint32_t k0 = key[lo], k1 = key[hi];
                    const uint16_t c0 = cand[lo], c1 = cand[hi];
                    const bool greater = k0 > k1 || (k0 == k1 && c0 > c1);
                    if (greater == ((lo & k) == 0)) { key[lo] = k1; key[hi] = k0; cand[lo] = c1; cand[hi] = c0; }
                }
                // Which barrier a stage needs. The block has T = a multiple of 64 threads, so the 64 pairs t = 64 g .. 64 g + 63
                // ("group g") are always the work of one wavefront, wave g mod (T / 64), whatever the stage. In a stage with
                // j <= 64 group g reads and writes only elements 128 g .. 128 g + 127. So between two stages that both have
                // j <= 64 every element is handed from a wavefront to itself, and its own program order (wave_sync) is enough;
                // a stage with j > 64 exchanges across groups, and the whole block must meet before and after it (__syncthreads).
                const int j_next = j > 1 ? (j >> 1) : k;
                if (j > 64 || j_next > 64) __syncthreads();
                else wave_sync();
            }
        }
        if (r <= 0) {                                          // detect() without applyMinDistance: nk zero points, then the sorted ones
            for (int i = tid; i < n; i += T) {
                const int id = min((int)cand[i], n - 1);
                out[2 * i] = 0.0f; out[2 * i + 1] = 0.0f;
                out[2 * (n + i)] = src[3 * id]; out[2 * (n + i) + 1] = src[3 * id + 1];
            }
            if (tid == 0) a.n_out[set] = 2 * n;
            return;
        }
    }

    const float r2 = (float)(r * r);
    for (int i = tid; i < n_prev; i += T) {
        const float *p = a.prev + ((size_t)set * a.max_prev + i) * 2;
        list[i] = make_float2(p[0], p[1]);
    }
    if (tid == 0) s_flag = 0;
    __syncthreads();
    if (SORTED && n > 0) {                                     // the zero prefix: one candidate (0, 0)
        bool near = false;
        for (int i = tid; i < n_prev; i += T) near = near || within(list[i].x, list[i].y, 0.0f, 0.0f, r2);
        if (near) s_flag = 1;
    }

    // live-track test of every candidate, survivors compacted in order over cand[]
    int m = 0;
    for (int base = 0, it = 0; base < n; base += T, ++it) {
        const int i = base + tid;
        int id = 0;
        bool keep = false;
        float x = 0.0f, y = 0.0f;
        if (i < n) {
            id = SORTED ? min((int)cand[i], n - 1) : i;
            x = src[STRIDE * id]; y = src[STRIDE * id + 1];
            keep = true;
#pragma unroll 8
            for (int j = 0; j < n_prev; ++j) keep = keep & !within(list[j].x, list[j].y, x, y, r2);   // (no early exit: the reads stay in flight)
        }
        const unsigned long long b = __ballot(keep);
        if (lane == 0) s_wave[it & 1][wave] = __popcll(b);
        __syncthreads();                                       // every cand[] of this chunk has been read
        int off = m, total = 0;
        for (int w = 0; w < waves; ++w) { const int c = s_wave[it & 1][w]; total += c; if (w < wave) off += c; }
        if (keep) cand[off + __popcll(b & ((1ull << lane) - 1ull))] = (uint16_t)id;
        m += total;
    }
    __syncthreads();                                           // survivors and s_flag complete; the live tracks are no longer needed
    if (wave != 0) return;

    // the greedy walk: list[] now holds the accepted corners
    int n_acc = 0;
    if (SORTED && n > 0 && s_flag == 0) {
        if (lane == 0) { list[0] = make_float2(0.0f, 0.0f); out[0] = 0.0f; out[1] = 0.0f; }
        n_acc = 1;
    }
    float nx = 0.0f, ny = 0.0f;                                // the next chunk's coordinates, loaded one chunk ahead
    if (lane < m) { const int id = cand[lane]; nx = src[STRIDE * id]; ny = src[STRIDE * id + 1]; }
    for (int base = 0; base < m && n_acc < a.max_tracks; base += 64) {
        bool live = base + lane < m;
        const float x = nx, y = ny;
        // (list form: the chunk ahead is read before this chunk's corners are written, at indices below this chunk's own)
        if (base + 64 + lane < m) { const int id = cand[base + 64 + lane]; nx = src[STRIDE * id]; ny = src[STRIDE * id + 1]; }
        wave_sync();
#pragma unroll 8
        for (int j = 0; j < n_acc; ++j) {
            const float2 c = list[j];
            if (within(c.x, c.y, x, y, r2)) live = false;
        }
        while (true) {
            const unsigned long long b = __ballot(live);
            if (b == 0) break;
            const int lead = __ffsll((long long)b) - 1;
            const float ax = __shfl(x, lead), ay = __shfl(y, lead);
            if (lane == lead) {
                list[n_acc] = make_float2(ax, ay);
                if (n_acc < a.max_corners) { out[2 * n_acc] = ax; out[2 * n_acc + 1] = ay; }
                live = false;
            }
            ++n_acc;
            if (n_acc >= a.max_tracks) break;
            if (live && within(ax, ay, x, y, r2)) live = false;
        }
    }
    if (lane == 0) a.n_out[set] = n_acc;
}

size_t tail_lds(bool sorted, int cand_count, int max_prev, int max_tracks)
{
    const size_t list = sizeof(float) * 2 * (size_t)std::max(max_prev, max_tracks);
    return (sorted ? sizeof(uint32_t) * (size_t)cand_count : 0) + list + ((sizeof(uint16_t) * (size_t)cand_count + 15) & ~(size_t)15);
}

int tail_threads(int candidates)
{
    return std::min(DT_MAX_THREADS, std::max(64, (candidates + 63) / 64 * 64));
}

// the checks both entries share, made before the context is looked at
int check_common(int n_sets, int max_prev, const int *n_prev_dev, const float *prev_dev, const int *radius_dev, int max_tracks,
                 const int *n_out_dev)
{
    if (n_sets < 0 || max_prev < 0 || max_tracks < 1) return HV_ERR_INVALID;
    if (n_sets > 0 && (!radius_dev || !n_out_dev || (max_prev > 0 && (!n_prev_dev || !prev_dev)))) return HV_ERR_INVALID;
    if (n_sets > 65535 || max_prev > HV_DETECT_TAIL_MAX_PREV || max_tracks > HV_DETECT_TAIL_MAX_TRACKS) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}

}  // namespace

// the two kernels' dynamic-LDS limits, set once per context (never inside a launch that may be under capture)
int detect_tail_init(Ctx *c)
{
    const int cap = (int)tail_lds(true, HV_DETECT_TAIL_MAX_KEYPOINTS, HV_DETECT_TAIL_MAX_PREV, HV_DETECT_TAIL_MAX_TRACKS);
    HV_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(detect_tail_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, cap));
    HV_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(detect_tail_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)tail_lds(false, HV_DETECT_TAIL_MAX_CORNERS, HV_DETECT_TAIL_MAX_PREV, HV_DETECT_TAIL_MAX_TRACKS)));
    return HV_OK;
}

}  // namespace hv

using hv::Ctx;

extern "C" {

int hv_apply_min_distance_batch_dev(hv_ctx *h, int n_sets, int max_corners, const int *n_corners_dev, float *corners_dev, int max_prev,
                                    const int *n_prev_dev, const float *prev_dev, const int *radius_dev, int max_tracks, int *n_out_dev)
{
    if (max_corners < 0) return HV_ERR_INVALID;
    if (const int rc = hv::check_common(n_sets, max_prev, n_prev_dev, prev_dev, radius_dev, max_tracks, n_out_dev)) return rc;
    if (n_sets > 0 && (!n_corners_dev || (max_corners > 0 && !corners_dev))) return HV_ERR_INVALID;
    if (max_corners > HV_DETECT_TAIL_MAX_CORNERS) return HV_ERR_UNSUPPORTED;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    if (max_corners == 0) {
        HV_HIP(c, hipMemsetAsync(n_out_dev, 0, sizeof(int) * (size_t)n_sets, c->stream));
        return HV_OK;
    }
    hv::TailArgs a{};
    a.nk = max_corners; a.pow2 = 0; a.max_prev = max_prev; a.max_tracks = std::min(max_tracks, max_corners); a.max_corners = max_corners;
    a.n_corners = n_corners_dev; a.corners = corners_dev; a.n_prev = n_prev_dev; a.prev = prev_dev; a.radius = radius_dev;
    a.n_out = n_out_dev;
    const size_t shmem = hv::tail_lds(false, max_corners, max_prev, a.max_tracks);
    hv::ScopedKernelTime tm(c, HV_K_DETECT_TAIL);
    hipLaunchKernelGGL(hv::detect_tail_kernel<false>, dim3((unsigned)n_sets), dim3((unsigned)hv::tail_threads(max_corners)), shmem,
                       c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_gftt_corners_batch_dev(hv_ctx *h, const hv_gftt_params *p, int n_images, const float *kp_dev, int max_prev, const int *n_prev_dev,
                              const float *prev_dev, const int *mask_radius_dev, int max_corners, float *corners_dev, int *n_out_dev)
{
    if (!p || max_corners < 0) return HV_ERR_INVALID;
    if (const int rc = hv::check_common(n_images, max_prev, n_prev_dev, prev_dev, mask_radius_dev, p->maxTracks, n_out_dev)) return rc;
    if (n_images > 0 && (!kp_dev || !corners_dev)) return HV_ERR_INVALID;
    if (max_corners > HV_DETECT_TAIL_MAX_CORNERS) return HV_ERR_UNSUPPORTED;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    const int nk = hv_gftt_keypoint_count(h, p);
    if (nk > HV_DETECT_TAIL_MAX_KEYPOINTS) return HV_ERR_UNSUPPORTED;
    if (max_corners < std::min(p->maxTracks, 2 * nk)) return HV_ERR_INVALID;
    if (n_images == 0) return HV_OK;
    if (nk == 0) {
        HV_HIP(c, hipMemsetAsync(n_out_dev, 0, sizeof(int) * (size_t)n_images, c->stream));
        return HV_OK;
    }
    int pow2 = 4;
    while (pow2 < nk) pow2 <<= 1;
    hv::TailArgs a{};
    a.nk = nk; a.pow2 = pow2; a.max_prev = max_prev; a.max_tracks = std::min(p->maxTracks, nk + 1); a.max_corners = max_corners;
    a.kp = kp_dev; a.corners = corners_dev; a.n_prev = n_prev_dev; a.prev = prev_dev; a.radius = mask_radius_dev; a.n_out = n_out_dev;
    const size_t shmem = hv::tail_lds(true, pow2, max_prev, a.max_tracks);
    hv::ScopedKernelTime tm(c, HV_K_DETECT_TAIL);
    const int threads = hv::tail_threads(nk <= hv::DT_RANK_SORT_MAX ? nk : pow2 / 2);
    hipLaunchKernelGGL(hv::detect_tail_kernel<true>, dim3((unsigned)n_images), dim3((unsigned)threads), shmem,
                       c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_gftt_detect_batch_dev(hv_ctx *h, const hv_gftt_params *p, int n_images, const int *slots_dev, float *kp_dev, int max_prev,
                             const int *n_prev_dev, const float *prev_dev, const int *mask_radius_dev, int max_corners,
                             float *corners_dev, int *n_out_dev)
{
    if (!p || max_corners < 0) return HV_ERR_INVALID;
    if (const int rc = hv::check_common(n_images, max_prev, n_prev_dev, prev_dev, mask_radius_dev, p->maxTracks, n_out_dev)) return rc;
    if (n_images > 0 && (!slots_dev || !kp_dev || !corners_dev)) return HV_ERR_INVALID;
    if (max_corners > HV_DETECT_TAIL_MAX_CORNERS) return HV_ERR_UNSUPPORTED;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    const int nk = hv_gftt_keypoint_count(h, p);
    if (nk > HV_DETECT_TAIL_MAX_KEYPOINTS) return HV_ERR_UNSUPPORTED;
    if (max_corners < std::min(p->maxTracks, 2 * nk)) return HV_ERR_INVALID;     // before anything is launched
    if (const int rc = hv_gftt_keypoints_batch_dev(h, p, n_images, slots_dev, kp_dev)) return rc;
    return hv_gftt_corners_batch_dev(h, p, n_images, kp_dev, max_prev, n_prev_dev, prev_dev, mask_radius_dev, max_corners, corners_dev,
                                     n_out_dev);
}

}  // extern "C"
