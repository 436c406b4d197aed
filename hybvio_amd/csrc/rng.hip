// Device-resident std::mt19937 streams for a batch of resident sequences: the random numbers of the RANSAC filters (rot_ransac.cpp:74-96
// on the pipeline's generator, ransac_pipeline.cpp:46,66; RANSAC3's own, :78; the upright 2-point filter's, stereo_upright_2p.cpp:101)
// and of shuffleDeterministic (util/util.hpp:39-44 on the odometry generator, backend.cpp:107,117,193,964) without a host generator:
// draw hands the consumer the next outputs and leaves the state alone, advance moves the state by the count the consumer left in device
// memory. Restatement: tests/rng_restatement.py. Arithmetic and phase schedule: hv_mt19937.hpp, DESIGN.md 3.22.
//
// One wavefront per set, RNG_SETS sets per workgroup. A set's 624 words are loaded coalesced into the wave's LDS slice and everything
// happens there; the waves of a workgroup never talk to each other, so there is no workgroup barrier anywhere (their trip counts
// differ with pos and with the count) and a wave whose set does not exist or has nothing to do returns at once. The phases of a twist
// are ordered inside the wave: DS operations of a wave execute in order, a wave-level fence keeps the compiler from moving them.
// Integer arithmetic only.
#include "hv_internal.hpp"
#include "hv_mt19937.hpp"

namespace hv {
namespace {

constexpr int RNG_SETS = 4;                                      // wavefronts = sets per workgroup
constexpr int RNG_THREADS = 64 * RNG_SETS;
constexpr int PHASE_CHUNKS = (mt::N - mt::M + 63) / 64;          // words of a phase per lane: 4 (227 words on 64 lanes)

struct SeedArgs { hv_rng st; int n_sets; uint32_t seed; const uint32_t *seeds; const int32_t *kind; };
struct DrawArgs { hv_rng st; int n_sets, n_draws; uint32_t *draws; };
struct AdvanceArgs { hv_rng st; int n_sets; const int32_t *count; int stride, multiplier, max_draws; };

__device__ __forceinline__ void wave_sync_lds()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// this wave's set, or -1; its LDS slice
__device__ __forceinline__ int wave_set(int n_sets)
{
    const int s = (int)blockIdx.x * RNG_SETS + (int)(threadIdx.x >> 6);
    return s < n_sets ? s : -1;
}

__device__ __forceinline__ void load_state(uint32_t *w, const uint32_t *g, int lane)
{
    for (int i = lane; i < mt::N; i += 64) w[i] = g[i];
    wave_sync_lds();
}

__device__ __forceinline__ void store_state(uint32_t *g, const uint32_t *w, int lane)
{
    wave_sync_lds();
    for (int i = lane; i < mt::N; i += 64) g[i] = w[i];
}

// One twist of the wave's array (hv_mt19937.hpp): per phase every lane reads the operands of its words, then -- behind a fence -- writes
// them; the next phase starts behind another. Ends with a fence: the array is ready to be read.
__device__ __forceinline__ void wave_twist(uint32_t *w, int lane)
{
#pragma unroll
    for (int ph = 0; ph < mt::PHASES; ++ph) {
        const int begin = mt::PHASE_BEGIN[ph], end = mt::PHASE_BEGIN[ph + 1];
        uint32_t v[PHASE_CHUNKS];
#pragma unroll
        for (int q = 0; q < PHASE_CHUNKS; ++q) {
            const int i = begin + q * 64 + lane;
            v[q] = i < end ? mt::twist_word(w, i) : 0u;
        }
        wave_sync_lds();                                         // every read of the phase precedes every write of it
#pragma unroll
        for (int q = 0; q < PHASE_CHUNKS; ++q) {
            const int i = begin + q * 64 + lane;
            if (i < end) w[i] = v[q];
        }
        wave_sync_lds();
    }
    if (lane == 0) w[mt::N - 1] = mt::twist_last(w);
    wave_sync_lds();
}

// pos as stored -> 0 .. 624; the same value in every lane, moved to a scalar so that the loops over it are uniform by construction
__device__ __forceinline__ int load_pos(const int32_t *pos, int s)
{
    return __builtin_amdgcn_readfirstlane(min(max(pos[s], 0), mt::N));
}

__global__ __launch_bounds__(RNG_THREADS) void rng_seed_kernel(SeedArgs a)
{
    __shared__ uint32_t s_mt[RNG_SETS][mt::N];
    const int lane = threadIdx.x & 63, s = wave_set(a.n_sets);
    if (s < 0) return;
    if (a.kind) {
        const int kind = a.kind[s];
        if (kind != HV_RESET_FRESH && kind != HV_RESET_KEEP_POSE) return;     // (wave-uniform) not reset: nothing of the set is touched
    }
    uint32_t *w = s_mt[threadIdx.x >> 6];
    if (lane == 0) {                                             // 623 dependent steps: one lane, in LDS
        uint32_t x = a.seeds ? a.seeds[s] : a.seed;
        w[0] = x;
        for (int i = 1; i < mt::N; ++i) { x = mt::seed_step(x, i); w[i] = x; }
    }
    store_state(a.st.mt + (size_t)s * mt::N, w, lane);
    if (lane == 0) a.st.pos[s] = mt::N;
}

__global__ __launch_bounds__(RNG_THREADS) void rng_draw_kernel(DrawArgs a)
{
    __shared__ uint32_t s_mt[RNG_SETS][mt::N];
    const int lane = threadIdx.x & 63, s = wave_set(a.n_sets);
    if (s < 0) return;
    uint32_t *w = s_mt[threadIdx.x >> 6];
    load_state(w, a.st.mt + (size_t)s * mt::N, lane);
    uint32_t *out = a.draws + (size_t)s * a.n_draws;
    int p = load_pos(a.st.pos, s);
    for (int k = 0; k < a.n_draws;) {                            // at most 1 + twists_for(624, HV_RNG_MAX_DRAWS) = 5 rounds
        if (p == mt::N) { wave_twist(w, lane); p = 0; }
        const int m = min(mt::N - p, a.n_draws - k);
        for (int j = lane; j < m; j += 64) out[k + j] = mt::temper(w[p + j]);
        wave_sync_lds();                                         // ... read before the next twist writes
        k += m; p += m;
    }
}

__global__ __launch_bounds__(RNG_THREADS) void rng_advance_kernel(AdvanceArgs a)
{
    __shared__ uint32_t s_mt[RNG_SETS][mt::N];
    const int lane = threadIdx.x & 63, s = wave_set(a.n_sets);
    if (s < 0) return;
    const int cnt = min(max(a.count[(size_t)s * a.stride], 0), a.max_draws);
    const int c = __builtin_amdgcn_readfirstlane((int)min((long long)cnt * a.multiplier, (long long)a.max_draws));
    if (c == 0) return;                                          // (wave-uniform) the set stays bit for bit
    const int p = load_pos(a.st.pos, s);
    const int twists = mt::twists_for(p, c);                     // <= twists_for(624, HV_RNG_MAX_DRAWS) = 4
    if (twists > 0) {
        uint32_t *w = s_mt[threadIdx.x >> 6];
        uint32_t *g = a.st.mt + (size_t)s * mt::N;
        load_state(w, g, lane);
        for (int t = 0; t < twists; ++t) wave_twist(w, lane);
        store_state(g, w, lane);
    }
    if (lane == 0) a.st.pos[s] = p + c - mt::N * twists;         // 1 .. 624
}

}  // namespace
}  // namespace hv

using hv::Ctx;

namespace {

// the checks every entry shares, in the header's order: INVALID first, then UNSUPPORTED
int check_common(int n_sets, const hv_rng *rng, bool invalid_extra, bool unsupported_extra)
{
    if (n_sets < 0 || !rng || !rng->mt || !rng->pos || invalid_extra) return HV_ERR_INVALID;
    if (n_sets > 65535 || unsupported_extra) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}

unsigned rng_grid(int n_sets) { return (unsigned)((n_sets + hv::RNG_SETS - 1) / hv::RNG_SETS); }

}  // namespace

extern "C" {

int hv_rng_seed_batch_dev(hv_ctx *h, int n_sets, const hv_rng *rng, uint32_t seed, const uint32_t *seed_dev,
                          const int32_t *reset_kind_dev)
{
    if (const int rc = check_common(n_sets, rng, false, false)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    hv::SeedArgs a{*rng, n_sets, seed, seed_dev, reset_kind_dev};
    hv::ScopedKernelTime tm(c, HV_K_TRAIL_INDEX);
    hipLaunchKernelGGL(hv::rng_seed_kernel, dim3(rng_grid(n_sets)), dim3(hv::RNG_THREADS), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_rng_draw_batch_dev(hv_ctx *h, int n_sets, const hv_rng *rng, int n_draws, uint32_t *draws_dev)
{
    if (const int rc = check_common(n_sets, rng, n_draws < 1 || !draws_dev, n_draws > HV_RNG_MAX_DRAWS)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    hv::DrawArgs a{*rng, n_sets, n_draws, draws_dev};
    hv::ScopedKernelTime tm(c, HV_K_TRAIL_INDEX);
    hipLaunchKernelGGL(hv::rng_draw_kernel, dim3(rng_grid(n_sets)), dim3(hv::RNG_THREADS), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

int hv_rng_advance_batch_dev(hv_ctx *h, int n_sets, const hv_rng *rng, const int32_t *count_dev, int count_stride, int multiplier,
                             int max_draws)
{
    if (const int rc = check_common(n_sets, rng, !count_dev || count_stride < 1 || multiplier < 1 || max_draws < 0,
                                    max_draws > HV_RNG_MAX_DRAWS))
        return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    hv::AdvanceArgs a{*rng, n_sets, count_dev, count_stride, multiplier, max_draws};
    hv::ScopedKernelTime tm(c, HV_K_TRAIL_INDEX);
    hipLaunchKernelGGL(hv::rng_advance_kernel, dim3(rng_grid(n_sets)), dim3(hv::RNG_THREADS), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

}  // extern "C"
