// Small workgroup-level tools shared by the tracker-side kernels (rot_ransac.hip, ransac5.hip, ransac3.hip and upright2p.hip -- there
// mostly through hv_sample_consensus.hpp --, trail_index.hip, flow_predict.hip, track_table.hip): the ordered ballot compaction, the gather that follows it in the RANSAC kernels, the staging of
// two camera models into LDS, and clampi. Device-only; wave64, one-dimensional workgroups.
//
// No include guard and no namespace of its own, like hv_geometry.hpp: a translation unit includes it once, inside its anonymous
// namespace, behind its contraction pragma if it has one (nothing here does floating-point arithmetic) and after hv_internal.hpp
// (hv_camera_model).

__device__ inline int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// The items i < count with pred(i), in order, into out[] (as Out); returns their number. Every thread of a workgroup of WAVES
// wavefronts calls it with the same count. 64-item chunks are counted with a ballot, the chunk offsets come from a serial scan on thread
// 0, and the lane prefix count of a second ballot places each item. s_chunk: ceil(count / 64) + 1 ints of LDS. No barrier at the
// start: what pred reads must be visible already. Three barriers; ends with one, which publishes out[] (and lets s_chunk be reused).
template <int WAVES, class Pred, class Out> __device__ inline int block_compact(Pred pred, Out *out, int count, int *s_chunk)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nch = (count + 63) / 64;
    for (int ch = wave; ch < nch; ch += WAVES) {
        const int i = ch * 64 + lane;
        const unsigned long long m = __ballot(i < count && pred(i));
        if (lane == 0) s_chunk[ch] = __popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int ch = 0; ch < nch; ++ch) { const int c = s_chunk[ch]; s_chunk[ch] = acc; acc += c; }
        s_chunk[nch] = acc;
    }
    __syncthreads();
    const int total = s_chunk[nch];
    for (int ch = wave; ch < nch; ch += WAVES) {
        const int i = ch * 64 + lane;
        const bool on = i < count && pred(i);
        const unsigned long long m = __ballot(on);
        if (on) out[s_chunk[ch] + __popcll(m & ((1ull << lane) - 1ull))] = (Out)i;
    }
    __syncthreads();
    return total;
}

// After block_compact(..., vmap, ...) = m: element vmap[j] of each of the NA arrays moves to position j, j < m <= 4 THREADS (four per
// thread, held in registers). One barrier, between the reads and the writes (vmap[j] >= j, so a write may land on an element that
// another thread still has to read). No barrier at the end: the caller's next one publishes the arrays.
template <int THREADS, int NA> __device__ __forceinline__ void block_gather_front(double *const (&arr)[NA], const int *vmap, int m)
{
    const int tid = threadIdx.x;
    double hv[4][NA];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = tid + q * THREADS;
        if (j < m) {
            const int k = vmap[j];
#pragma unroll
            for (int t = 0; t < NA; ++t) hv[q][t] = arr[t][k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = tid + q * THREADS;
        if (j < m) {
#pragma unroll
            for (int t = 0; t < NA; ++t) arr[t][j] = hv[q][t];
        }
    }
}

// Two camera models from kernel arguments into s_cam[2], word by word: read through the arguments they would occupy scalar registers
// for the whole kernel. NO barrier: the caller names the one that publishes s_cam.
template <int THREADS>
__device__ __forceinline__ void stage_cameras(hv_camera_model *s_cam, const hv_camera_model &c0, const hv_camera_model &c1)
{
    static_assert(sizeof(hv_camera_model) % 4 == 0, "word copy");
    constexpr int W = (int)(sizeof(hv_camera_model) / 4);
    const int *src0 = reinterpret_cast<const int *>(&c0), *src1 = reinterpret_cast<const int *>(&c1);
    int *dst = reinterpret_cast<int *>(s_cam);
    for (int i = threadIdx.x; i < 2 * W; i += THREADS) dst[i] = i < W ? src0[i] : src1[i - W];
}
