// Device track table: the bookkeeping of TrackerImplementation::add / track from the keyframe decision onwards, for many resident
// sequences at once.
//
// Reference: src/tracker/tracker.cpp:199-229 (the ID rule, frameNum, the reset below five tracks), :527-558 (keyframe, updateTracks,
// detectNewFeatures, the maskScale tuning, prevCorners), computeMaxPixelCoordinateMovement (:21-41), computeVisualStationarity
// (:578-602), updateTracks (:604-670), detectNewFeatures (:672-703), resetAllTracks (:705-719), deleteTrack (:726-738), setMask
// (:766-777), changeMaskSize (:561-567) and maskRadius (:569-576).
//
// One workgroup per set, one thread per track slot (maxTracks <= 1024). Every rule is integer or IEEE arithmetic restated literally,
// with one exception that is an identity, not an approximation: the culling at capacity (:621-639) sorts all n (n - 1) / 2 pairs by
// dist2 with std::stable_sort and walks them, inserting j, until the set holds maxTracks / 20 + 1 tracks. Pairs are generated i-major,
// j-minor, so the sorted order is lexicographic in (dist2, i, j); a track j enters the set at its first pair, which is its smallest
// key (min over i < j of dist2(i, j), the first i attaining it, j); the walk therefore takes the maxTracks / 20 + 1 tracks j >= 1 with
// the smallest keys. Each thread forms the key of its own j from the corners in LDS and ranks it by counting the smaller keys (no
// atomics, no sort, deterministic). Compactions use a wave64 ballot, the lane prefix count and per-wave offsets in LDS.
// Every input of a set is read before the first barrier after which outputs are written, so the compaction is in place.
#include "fresh_state.hpp"

#include <algorithm>
#include <cmath>

namespace hv {
namespace {

// tracker::Feature::Status (src/tracker/track.hpp:9-21)
constexpr int ST_TRACKED = 0, ST_NEW = 1, ST_CULLED = 7, ST_BLACKLISTED = 8;
constexpr int TT_MAX = HV_TRACKS_MAX_TRACKS;
constexpr int TT_WAVES = TT_MAX / 64;
constexpr int MASK_STEPS = 10;                  // |2 * maskScale| <= 10 (changeMaskSize: [-5, 5])
constexpr unsigned FLAG_RESET = 1u;

struct TableArgs {
    hv_track_table t;
    int max_tracks, max_track_length;
    double movement_threshold, score_threshold;
    int radii[2 * MASK_STEPS + 1];              // maskRadius() at steps -10 .. 10
    // update
    const float *corners, *second;
    int32_t *track_status;
    const double *score;
    int32_t *keyframe;
    float *mask_xy;
    int32_t *n_mask, *src_index;
    double *max_movement;
    // append / delete
    int max_new;
    const int32_t *n_new;
    const float *new_xy, *new_second;
    int32_t *n_added;
};

#include "hv_workgroup.hpp"   // clampi

// computeDist2 (tracker.cpp:16-19): binary32 differences widened to binary64, two rounded products, one rounded sum
__device__ inline double dist2(float2 a, float2 b)
{
    const double dx = (double)(a.x - b.x), dy = (double)(a.y - b.y);
    return __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
}

// exclusive prefix of `flag` over the workgroup in thread order; *total = the number of set flags. s_wave: TT_WAVES ints, reused
// by every call, hence the trailing barrier.
__device__ inline int block_prefix(bool flag, int *s_wave, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < waves; ++w) { const int c = s_wave[w]; if (w < wave) off += c; tot += c; }
    __syncthreads();
    *total = tot;
    return off + __popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(TT_MAX) void tracks_init_kernel(TableArgs a)
{
    tracks_fresh_set(a.t, blockIdx.x, a.max_tracks, a.radii[MASK_STEPS]);
}

__global__ __launch_bounds__(TT_MAX) void tracks_update_kernel(TableArgs a)
{
    __shared__ float2 s_xy[TT_MAX];
    __shared__ double s_key[TT_MAX];            // the culling key's dist2; before that, the per-wave maxima of the movement
    __shared__ int s_first[TT_MAX];             // the culling key's i
    __shared__ int s_wave[TT_WAVES];
    __shared__ int s_any[TT_WAVES];

    const int set = blockIdx.x, i = threadIdx.x, lane = i & 63, wave = i >> 6, waves = blockDim.x >> 6;
    const int M = a.max_tracks;
    const int n = clampi(a.t.n_tracks[set], 0, M);
    const int f = a.t.frame_num[set];
    const size_t k = (size_t)set * M + i;
    const bool stereo = a.t.second_xy != nullptr;

    if (f == 0 || n < 5) {                      // initialize() / the else branch of add() (:201-205, 222-229)
        __syncthreads();                        // every wave has read n_tracks before thread 0 rewrites it (uniform branch)
        if (i < M) { a.t.kf_valid[k] = 0; a.t.blacklist[k] = 0; }
        if (i == 0) {
            a.t.n_tracks[set] = 0;
            a.n_mask[set] = 0;
            a.keyframe[set] = 1;
            a.t.frame_flags[set] = (uint8_t)FLAG_RESET;
            if (a.max_movement) a.max_movement[set] = -1.0;
        }
        return;
    }

    // ---- every input of the set, before anything is written ----
    const bool live = i < n;
    float2 c = make_float2(0.0f, 0.0f), c2 = c, kf = c;
    int st = -1, id = 0;
    bool kfv = false;
    if (live) {
        c = make_float2(a.corners[2 * k], a.corners[2 * k + 1]);
        if (stereo) c2 = make_float2(a.second[2 * k], a.second[2 * k + 1]);
        st = a.track_status[k];
        id = a.t.ids[k];
        kfv = a.t.kf_valid[k] != 0;
        if (kfv) kf = make_float2(a.t.kf_xy[2 * k], a.t.kf_xy[2 * k + 1]);
        s_xy[i] = c;
    }
    const bool tracked = live && st == ST_TRACKED;

    // ---- computeMaxPixelCoordinateMovement (:21-41): std::max(maxDist, d) never takes a NaN d, so a NaN counts as 0 ----
    const bool moves = tracked && kfv;
    double d = 0.0;
    if (moves) {
        d = __dsqrt_rn(dist2(c, kf));
        if (!(d == d)) d = 0.0;
    }
    for (int o = 32; o > 0; o >>= 1) { const double e = __shfl_xor(d, o); d = d < e ? e : d; }
    const unsigned long long mb = __ballot(moves);
    if (lane == 0) { s_key[wave] = d; s_any[wave] = mb != 0ull; }

    // ---- setMask (:766-777), before the culling ----
    int n_mask = 0;
    const int mpos = block_prefix(tracked, s_wave, &n_mask);       // its first barrier also publishes s_xy, s_key, s_any
    if (tracked) {
        const size_t o = (size_t)set * M + mpos;
        a.mask_xy[2 * o] = c.x; a.mask_xy[2 * o + 1] = c.y;
    }
    double max_movement = 0.0;
    bool any = false;
    for (int w = 0; w < waves; ++w) { const double e = s_key[w]; max_movement = max_movement < e ? e : max_movement; any |= s_any[w] != 0; }
    if (!any) max_movement = -1.0;
    __syncthreads();                             // s_key is reused below

    // ---- keyframe (:527-528 with frameNum = f + 1, :578-602) ----
    bool stationary = false;
    if (any) {
        const double score = a.score ? a.score[set] : 0.0;
        stationary = __dmul_rn(score, max_movement < a.movement_threshold ? 1.0 : 0.0) > a.score_threshold;
    }
    const bool keyframe = (f + 1 < a.max_track_length) || !stationary;

    // ---- culling at capacity (:621-639) ----
    if (n == M) {
        double best = 0.0;
        int first = 0;
        if (i >= 1 && live) {
            best = dist2(s_xy[0], c);
            for (int p = 1; p < i; ++p) {
                const double e = dist2(s_xy[p], c);
                if (e < best) { best = e; first = p; }
            }
            s_key[i] = best; s_first[i] = first;
        }
        __syncthreads();
        if (i >= 1 && live) {
            int rank = 0;
            for (int j = 1; j < n; ++j) {
                const double e = s_key[j];
                const int q = s_first[j];
                rank += (e < best || (e == best && (q < first || (q == first && j < i)))) ? 1 : 0;
            }
            if (rank < M / 20 + 1) { st = ST_CULLED; a.track_status[k] = ST_CULLED; }
        }
    }

    // ---- write-back, erase and compaction (:641-669) ----
    const bool keep = live && st == ST_TRACKED;
    int n_keep = 0;
    const int pos = block_prefix(keep, s_wave, &n_keep);           // every thread has read its inputs by this barrier
    if (keep) {
        const size_t o = (size_t)set * M + pos;
        a.t.ids[o] = id;
        a.t.xy[2 * o] = c.x; a.t.xy[2 * o + 1] = c.y;
        if (stereo) { a.t.second_xy[2 * o] = c2.x; a.t.second_xy[2 * o + 1] = c2.y; }
        a.t.status[o] = ST_TRACKED;
        a.t.blacklist[o] = 0;
        if (keyframe) kf = c;
        if (keyframe || kfv) { a.t.kf_xy[2 * o] = kf.x; a.t.kf_xy[2 * o + 1] = kf.y; }
        a.t.kf_valid[o] = (keyframe || kfv) ? 1 : 0;
        if (a.src_index) a.src_index[o] = i;
    }
    if (i >= n_keep && i < M) { a.t.kf_valid[k] = 0; a.t.blacklist[k] = 0; }
    if (i == 0) {
        a.t.n_tracks[set] = n_keep;
        a.n_mask[set] = n_mask;
        a.keyframe[set] = keyframe ? 1 : 0;
        a.t.frame_flags[set] = 0;
        if (a.max_movement) a.max_movement[set] = max_movement;
    }
}

// detectNewFeatures' append (:672-703) / resetAllTracks (:705-719), the maskScale tuning (:540-546) and frameNum
__global__ __launch_bounds__(TT_MAX) void tracks_append_kernel(TableArgs a)
{
    const int set = blockIdx.x, i = threadIdx.x;
    const int M = a.max_tracks;
    const int n = clampi(a.t.n_tracks[set], 0, M);
    const int f = a.t.frame_num[set];
    const bool reset = (a.t.frame_flags[set] & FLAG_RESET) != 0;
    const int missing = M - n;
    const int n_new = a.max_new > 0 ? clampi(a.n_new[set], 0, a.max_new) : 0;
    const int add = (reset || missing >= M / 10) ? min(n_new, missing) : 0;
    if (i < add) {
        const size_t o = (size_t)set * M + n + i, q = (size_t)set * a.max_new + i;
        a.t.ids[o] = f * M + 1 + i;                                  // nextTrackId = frameNum * maxTracks + 1 (:199)
        a.t.xy[2 * o] = a.new_xy[2 * q]; a.t.xy[2 * o + 1] = a.new_xy[2 * q + 1];
        if (a.t.second_xy) { a.t.second_xy[2 * o] = a.new_second[2 * q]; a.t.second_xy[2 * o + 1] = a.new_second[2 * q + 1]; }
        a.t.status[o] = ST_NEW;
        a.t.blacklist[o] = 0;
        a.t.kf_valid[o] = 0;
    }
    __syncthreads();                            // every wave has read n_tracks, frame_num and frame_flags before they are rewritten
    if (i == 0) {
        const int total = n + add;
        int steps = clampi(a.t.mask_steps[set], -MASK_STEPS, MASK_STEPS);
        if (!reset) {
            if (total < (3 * M) / 4) steps -= 2;                     // changeMaskSize(-1.0)
            else if (total == M) steps += 1;                         // changeMaskSize(0.5)
            steps = clampi(steps, -MASK_STEPS, MASK_STEPS);
        }
        a.t.n_tracks[set] = total;
        a.t.mask_steps[set] = steps;
        a.t.mask_radius[set] = a.radii[steps + MASK_STEPS];
        a.t.frame_num[set] = f + 1;
        a.t.frame_flags[set] = 0;
        if (a.n_added) a.n_added[set] = add;
    }
}

// deleteTrack (:726-738); n_new / max_new carry the ID lists here
__global__ __launch_bounds__(TT_MAX) void tracks_delete_kernel(TableArgs a, const int32_t *ids)
{
    const int set = blockIdx.x, i = threadIdx.x;
    const int M = a.max_tracks;
    if (i >= clampi(a.t.n_tracks[set], 0, M)) return;
    const size_t k = (size_t)set * M + i;
    const int id = a.t.ids[k];
    const int n_ids = clampi(a.n_new[set], 0, a.max_new);
    const int32_t *list = ids + (size_t)set * a.max_new;
    bool hit = false;
    for (int j = 0; j < n_ids; ++j) hit |= list[j] == id;
    if (hit) { a.t.status[k] = ST_BLACKLISTED; a.t.blacklist[k] = 1; }
}

// the host-side checks, made before the context is looked at
int check_table(const hv_track_table_params *p, int n_sets, const hv_track_table *t)
{
    if (!p || !t || n_sets < 0 || p->maxTracks < 1) return HV_ERR_INVALID;
    if (!t->n_tracks || !t->ids || !t->xy || !t->status || !t->blacklist || !t->kf_xy || !t->kf_valid || !t->frame_num ||
        !t->mask_steps || !t->mask_radius || !t->frame_flags)
        return HV_ERR_INVALID;
    return HV_OK;
}

// after every HV_ERR_INVALID check of the entry: a call that is both invalid and too large is reported as invalid
int check_limits(const hv_track_table_params *p, int n_sets)
{
    return (n_sets > 65535 || p->maxTracks > TT_MAX) ? HV_ERR_UNSUPPORTED : HV_OK;
}

void fill_common(TableArgs &a, const Ctx *c, const hv_track_table_params *p, const hv_track_table *t)
{
    a.t = *t;
    a.max_tracks = p->maxTracks;
    a.max_track_length = p->maxTrackLength;
    a.movement_threshold = p->visualStationarityMovementThreshold;
    a.score_threshold = p->visualStationarityScoreThreshold;
    for (int s = -MASK_STEPS; s <= MASK_STEPS; ++s) a.radii[s + MASK_STEPS] = track_mask_radius(c, p, s);   // maskRadius (:569-576) at maskScale = s / 2
}

inline unsigned block_threads(int max_tracks) { return (unsigned)((max_tracks + 63) / 64 * 64); }

}  // namespace

// the HV_ERR_INVALID checks of the table, for session.hip (hv_internal.hpp)
int tracks_check_table(const hv_track_table_params *p, int n_sets, const hv_track_table *t) { return check_table(p, n_sets, t); }

}  // namespace hv

using hv::Ctx;

extern "C" {

void hv_track_table_default_params(hv_track_table_params *p)
{
    if (!p) return;
    p->maxTracks = 200;                              // codegen/parameter_definitions.c:262
    p->maxTrackLength = 21;                          // :265
    p->relativeMaskRadius = 0.0667;                  // :308
    p->visualStationarityMovementThreshold = 3.0;    // :111
    p->visualStationarityScoreThreshold = 0.95;      // :113
}

int hv_tracks_init_batch_dev(hv_ctx *h, const hv_track_table_params *p, int n_sets, const hv_track_table *table)
{
    if (const int rc = hv::check_table(p, n_sets, table)) return rc;
    if (const int rc = hv::check_limits(p, n_sets)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    hv::TableArgs a{};
    hv::fill_common(a, c, p, table);
    hv::ScopedKernelTime tm(c, HV_K_TRACK_TABLE);
    hipLaunchKernelGGL(hv::tracks_init_kernel, dim3((unsigned)n_sets), dim3(hv::block_threads(p->maxTracks)), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_tracks_update_batch_dev(hv_ctx *h, const hv_track_table_params *p, int n_sets, const hv_track_table *table,
                               const float *corners_dev, const float *second_corners_dev, int32_t *track_status_dev,
                               const double *score_dev, int32_t *keyframe_dev, float *mask_xy_dev, int32_t *n_mask_dev,
                               int32_t *src_index_dev, double *max_movement_dev)
{
    if (const int rc = hv::check_table(p, n_sets, table)) return rc;
    if (!corners_dev || !track_status_dev || !keyframe_dev || !mask_xy_dev || !n_mask_dev) return HV_ERR_INVALID;
    if ((second_corners_dev == nullptr) != (table->second_xy == nullptr)) return HV_ERR_INVALID;
    if (const int rc = hv::check_limits(p, n_sets)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    hv::TableArgs a{};
    hv::fill_common(a, c, p, table);
    a.corners = corners_dev; a.second = second_corners_dev; a.track_status = track_status_dev; a.score = score_dev;
    a.keyframe = keyframe_dev; a.mask_xy = mask_xy_dev; a.n_mask = n_mask_dev; a.src_index = src_index_dev;
    a.max_movement = max_movement_dev;
    hv::ScopedKernelTime tm(c, HV_K_TRACK_TABLE);
    hipLaunchKernelGGL(hv::tracks_update_kernel, dim3((unsigned)n_sets), dim3(hv::block_threads(p->maxTracks)), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_tracks_append_batch_dev(hv_ctx *h, const hv_track_table_params *p, int n_sets, const hv_track_table *table, int max_new,
                               const int32_t *n_new_dev, const float *new_xy_dev, const float *new_second_dev,
                               int32_t *n_added_dev)
{
    if (const int rc = hv::check_table(p, n_sets, table)) return rc;
    if (max_new < 0) return HV_ERR_INVALID;
    if (max_new > 0 && (!n_new_dev || !new_xy_dev || (new_second_dev == nullptr) != (table->second_xy == nullptr)))
        return HV_ERR_INVALID;
    if (const int rc = hv::check_limits(p, n_sets)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    hv::TableArgs a{};
    hv::fill_common(a, c, p, table);
    a.max_new = max_new; a.n_new = n_new_dev; a.new_xy = new_xy_dev; a.new_second = new_second_dev; a.n_added = n_added_dev;
    hv::ScopedKernelTime tm(c, HV_K_TRACK_TABLE);
    hipLaunchKernelGGL(hv::tracks_append_kernel, dim3((unsigned)n_sets), dim3(hv::block_threads(p->maxTracks)), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_tracks_delete_batch_dev(hv_ctx *h, const hv_track_table_params *p, int n_sets, const hv_track_table *table, int max_ids,
                               const int32_t *n_ids_dev, const int32_t *ids_dev)
{
    if (const int rc = hv::check_table(p, n_sets, table)) return rc;
    if (max_ids < 0 || (max_ids > 0 && (!n_ids_dev || !ids_dev))) return HV_ERR_INVALID;
    if (const int rc = hv::check_limits(p, n_sets)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0 || max_ids == 0) return HV_OK;
    hv::TableArgs a{};
    hv::fill_common(a, c, p, table);
    a.max_new = max_ids; a.n_new = n_ids_dev;
    hv::ScopedKernelTime tm(c, HV_K_TRACK_TABLE);
    hipLaunchKernelGGL(hv::tracks_delete_kernel, dim3((unsigned)n_sets), dim3(hv::block_threads(p->maxTracks)), 0, c->stream, a, ids_dev);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

}  // extern "C"
