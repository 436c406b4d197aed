// Device tracker::util::matchIntensities (src/tracker/util.cpp:16-52,173-179) in the per-frame order of src/commandline/main.cpp:763-777
// for a batch of resident gray frames: the successive step (camera 0 against the previous matched frame, weight
// matchSuccessiveIntensities), then the stereo step (camera 1 against camera 0, weight 1). Restatement:
// tests/intensity_match_restatement.py; DESIGN.md 3.23.
//
// The matched pixel is a function of the input byte alone, so an image is a 256-bin histogram and a 256-entry table, and every
// number the reference derives from pixels follows EXACTLY from the histograms: sum x = sum hist[v] v, sum x^2 = sum hist[v] v^2
// of an input; sum hist[v] T[v] and sum hist[v] T[v]^2 of a matched image (the next frame's prevGrayFrame, and the left frame the right
// one is matched against). Three launches on the context stream:
//   1. intensity_hist_kernel   every image of the call once: 16-byte row loads, counts in per-wave replicated LDS histograms, merged
//                              into hist [set][camera][256] with integer atomics (order-independent)
//   2. intensity_apply_kernel  every workgroup derives its set's tables from the histograms and the OLD prev statistics (derive_set,
//                              the doubles in the reference's order of operations; -ffp-contract=off and the pragma below), builds
//                              the byte table of its image in LDS and rewrites its rows in place
//   3. intensity_state_kernel  one wavefront per set derives the same once more and writes the new prev statistics, has_prev and
//                              the record, then clears the set's histograms for the next call. A launch of its own because the
//                              workgroups of 2 read what it overwrites.
// Padding bytes between width and the row stride are neither read nor written: a 16-byte chunk that is not wholly inside the row is
// served byte by byte.
#include "hv_internal.hpp"

#pragma clang fp contract(off)

namespace hv {
namespace {

constexpr int IM_THREADS = 256, IM_WAVES = IM_THREADS / 64;
// LDS histograms of the counting kernel: per wavefront REPLICAS copies, a lane counts into copy lane % REPLICAS. On smooth frames
// neighbouring lanes (16 pixels apart) hit the same bin; same-address LDS atomics of a wave serialise, copies of 257 words put the
// same bin of neighbouring lanes on neighbouring banks instead.
#ifndef HV_IM_REPLICAS
#define HV_IM_REPLICAS 4
#endif
constexpr int REPLICAS = HV_IM_REPLICAS, REPLICA_STRIDE = 257;
static_assert(REPLICAS >= 1 && (REPLICAS & (REPLICAS - 1)) == 0 && REPLICAS <= 16, "a power of two");
constexpr int BLOCK_BYTES = 32768;                               // row bytes one workgroup counts / rewrites

struct Args {
    int n_sets, width, height, row_stride;
    int chunks_per_row, rows_per_block;                          // 16-byte chunks that can touch a row; rows of one workgroup
    uint8_t *img[2]; long long img_stride[2];                    // [1] null: camera 1 is not part of the call
    double w_left, w_right;                                      // weight of the successive step (0: off), of the stereo step (0: off)
    int stereo;                                                  // the stereo step runs (img[1] is counted and rewritten)
    hv_intensity_state st;
    const unsigned char *active;
    hv_intensity_record *record;
};

// sum of (a, b) over the workgroup's NT threads, in every thread. s_red: 2 * (NT / 64) words; two barriers when NT > 64.
template <int NT> __device__ __forceinline__ void block_sum2(unsigned long long &a, unsigned long long &b, unsigned long long *s_red)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    if (NT > 64) {
        const int wave = threadIdx.x >> 6;
        __syncthreads();                                         // the previous sums have been read
        if ((threadIdx.x & 63) == 0) { s_red[2 * wave] = a; s_red[2 * wave + 1] = b; }
        __syncthreads();
        a = b = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) { a += s_red[2 * w]; b += s_red[2 * w + 1]; }
    }
}

// cv::meanStdDev of a CV_8UC1 image from its exact sums (scale = 1 / N; mean = s scale; stddev = sqrt(max(sq scale - mean^2, 0)))
__device__ __forceinline__ void mean_std_dev(unsigned long long s, unsigned long long sq, double n, double &mean, double &stddev)
{
    const double scale = 1.0 / n;
    mean = (double)s * scale;
    stddev = sqrt(fmax((double)sq * scale - mean * mean, 0.0));
}

struct Table { double k, mean0, mean; bool constant; };

// setIntensities (util.cpp:28-42) up to the pixel loop
__device__ __forceinline__ Table make_table(unsigned long long total, unsigned long long sq, double n, double mean, double stddev, double weight)
{
    Table t;
    double m_in, stddev0;
    mean_std_dev(total, sq, n, m_in, stddev0);                   // :29-30
    stddev = stddev0 + weight * (stddev - stddev0);              // :31
    t.constant = !(stddev0 > 0.0);                               // :33 asserts; here the image stays as it is
    t.k = stddev / stddev0;                                      // :40
    t.mean0 = (double)total * t.k / n;                           // :41
    t.mean = t.mean0 + weight * (mean - t.mean0);                // :42
    if (t.constant) { t.k = 1.0; t.mean0 = t.mean = 0.0; }
    return t;
}

// the pixel loop's body (util.cpp:45-49)
__device__ __forceinline__ int map_pixel(const Table &t, int x)
{
    if (t.constant) return x;
    const double v = (double)x * t.k + t.mean - t.mean0;
    const double r = round(v);
    return r < 0.0 ? 0 : r > 255.0 ? 255 : (int)r;               // (int) then the clamp of :47-48, without the cast's overflow
}

struct Derived {
    unsigned long long in_sum[2], in_sq[2], out_sum[2], out_sq[2];
    Table t[2];
    int flags;
};

// Everything a set's frame needs, from its two histograms and its prev statistics, on NT threads (bin b of thread i: i + j NT).
// tab[cam][j] = this thread's table entries. Every thread returns the same Derived.
template <int NT>
__device__ __forceinline__ void derive_set(const Args &a, int set, unsigned long long *s_red, Derived &d, int (&tab)[2][256 / NT])
{
    constexpr int BPT = 256 / NT;
    const double n = (double)((long long)a.width * a.height);
    const uint32_t *hist = a.st.hist + (size_t)set * 512;
    uint32_t h[2][BPT];
    d.flags = 0;
#pragma unroll
    for (int cam = 0; cam < 2; ++cam) {
        unsigned long long s = 0, q = 0;
        if (cam == 0 || a.stereo) {
#pragma unroll
            for (int j = 0; j < BPT; ++j) {
                const int b = threadIdx.x + j * NT;
                h[cam][j] = hist[cam * 256 + b];
                s += (unsigned long long)h[cam][j] * (unsigned)b;
                q += (unsigned long long)h[cam][j] * (unsigned)(b * b);
            }
            block_sum2<NT>(s, q, s_red);
        } else {
#pragma unroll
            for (int j = 0; j < BPT; ++j) h[cam][j] = 0;
        }
        d.in_sum[cam] = d.out_sum[cam] = s;
        d.in_sq[cam] = d.out_sq[cam] = q;
        d.t[cam].k = 1.0; d.t[cam].mean0 = d.t[cam].mean = 0.0; d.t[cam].constant = true;      // not rewritten
    }
    // main.cpp:763-769: camera 0 against prevGrayFrame (the frame itself on the first frame, :766)
    if (a.w_left > 0.0) {
        const bool has = a.st.has_prev[set] != 0;
        double mean, stddev;
        mean_std_dev(has ? a.st.prev_sum[set] : d.in_sum[0], has ? a.st.prev_sqsum[set] : d.in_sq[0], n, mean, stddev);
        d.t[0] = make_table(d.in_sum[0], d.in_sq[0], n, mean, stddev, a.w_left);
        d.flags |= d.t[0].constant ? HV_INTENSITY_CONSTANT_LEFT : HV_INTENSITY_MATCHED_LEFT;
    }
    unsigned long long s = 0, q = 0;
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        const int v = map_pixel(d.t[0], threadIdx.x + j * NT);
        tab[0][j] = v;
        s += (unsigned long long)h[0][j] * (unsigned)v;
        q += (unsigned long long)h[0][j] * (unsigned)(v * v);
    }
    if (d.flags & HV_INTENSITY_MATCHED_LEFT) {                   // (uniform) the matched left frame's sums
        block_sum2<NT>(s, q, s_red);
        d.out_sum[0] = s; d.out_sq[0] = q;
    }
    // main.cpp:770-777: camera 1 against camera 0 as it is now
    if (a.stereo) {
        double mean, stddev;
        mean_std_dev(d.out_sum[0], d.out_sq[0], n, mean, stddev);
        d.t[1] = make_table(d.in_sum[1], d.in_sq[1], n, mean, stddev, a.w_right);
        d.flags |= d.t[1].constant ? HV_INTENSITY_CONSTANT_RIGHT : HV_INTENSITY_MATCHED_RIGHT;
    }
    s = q = 0;
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        const int v = map_pixel(d.t[1], threadIdx.x + j * NT);
        tab[1][j] = v;
        s += (unsigned long long)h[1][j] * (unsigned)v;
        q += (unsigned long long)h[1][j] * (unsigned)(v * v);
    }
    if (d.flags & HV_INTENSITY_MATCHED_RIGHT) {
        block_sum2<NT>(s, q, s_red);
        d.out_sum[1] = s; d.out_sq[1] = q;
    }
}

// The rows [r0, r1) of an image as 16-byte chunks on the 16-byte grid of memory: chunk c of row r covers the row's bytes
// [16 c - m, 16 c - m + 16) cut to [0, width), m = misalignment of the row's first byte. whole(p) serves a chunk wholly inside the row
// (p is 16-byte aligned), part(p, count) the bytes of one that is not.
template <class Whole, class Part>
__device__ __forceinline__ void for_each_chunk(const Args &a, uint8_t *img, int r0, int r1, Whole whole, Part part)
{
    const int items = (r1 - r0) * a.chunks_per_row;
    for (int i = threadIdx.x; i < items; i += IM_THREADS) {
        const int r = r0 + i / a.chunks_per_row, c = i % a.chunks_per_row;
        uint8_t *row = img + (size_t)r * a.row_stride;
        const int m = (int)(reinterpret_cast<uintptr_t>(row) & 15);
        const int lo = max(16 * c - m, 0), hi = min(16 * c - m + 16, a.width);
        if (hi - lo == 16) whole(row + lo);
        else if (hi > lo) part(row + lo, hi - lo);
    }
}

__device__ __forceinline__ bool set_active(const Args &a, int set) { return !a.active || a.active[set] != 0; }

__global__ __launch_bounds__(IM_THREADS) void intensity_hist_kernel(Args a)
{
    __shared__ uint32_t s_hist[IM_WAVES * REPLICAS * REPLICA_STRIDE];
    const int set = blockIdx.y, cam = blockIdx.z;
    if (!set_active(a, set)) return;                             // (uniform)
    for (int i = threadIdx.x; i < IM_WAVES * REPLICAS * REPLICA_STRIDE; i += IM_THREADS) s_hist[i] = 0;
    __syncthreads();
    uint32_t *mine = s_hist + ((threadIdx.x >> 6) * REPLICAS + (threadIdx.x & (REPLICAS - 1))) * REPLICA_STRIDE;
    const int r0 = blockIdx.x * a.rows_per_block, r1 = min(r0 + a.rows_per_block, a.height);
    for_each_chunk(a, a.img[cam] + (size_t)set * a.img_stride[cam], r0, r1,
        [&](const uint8_t *p) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int b = 0; b < 4; ++b) atomicAdd(&mine[(w[j] >> (8 * b)) & 255u], 1u);
            }
        },
        [&](const uint8_t *p, int count) {
            for (int j = 0; j < count; ++j) atomicAdd(&mine[p[j]], 1u);
        });
    __syncthreads();
    uint32_t total = 0;                                          // bin threadIdx.x over every copy
#pragma unroll
    for (int r = 0; r < IM_WAVES * REPLICAS; ++r) total += s_hist[r * REPLICA_STRIDE + threadIdx.x];
    if (total) atomicAdd(a.st.hist + ((size_t)set * 2 + cam) * 256 + threadIdx.x, total);
}

__global__ __launch_bounds__(IM_THREADS) void intensity_apply_kernel(Args a, int first_cam)
{
    __shared__ unsigned long long s_red[2 * IM_WAVES];
    __shared__ uint8_t s_tab[256];
    const int set = blockIdx.y, cam = first_cam + blockIdx.z;
    if (!set_active(a, set)) return;                             // (uniform)
    Derived d;
    int tab[2][1];
    derive_set<IM_THREADS>(a, set, s_red, d, tab);
    if (cam == 0 ? d.t[0].constant : d.t[1].constant) return;    // (uniform) bit for bit as it is
    s_tab[threadIdx.x] = (uint8_t)(cam == 0 ? tab[0][0] : tab[1][0]);   // (selects, not an index: d and tab stay in registers)
    __syncthreads();
    const int r0 = blockIdx.x * a.rows_per_block, r1 = min(r0 + a.rows_per_block, a.height);
    for_each_chunk(a, a.img[cam] + (size_t)set * a.img_stride[cam], r0, r1,
        [&](uint8_t *p) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p);
            uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                w[j] = (uint32_t)s_tab[w[j] & 255u] | (uint32_t)s_tab[(w[j] >> 8) & 255u] << 8 |
                       (uint32_t)s_tab[(w[j] >> 16) & 255u] << 16 | (uint32_t)s_tab[w[j] >> 24] << 24;
            }
            *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
        },
        [&](uint8_t *p, int count) {
            for (int j = 0; j < count; ++j) p[j] = s_tab[p[j]];
        });
}

__global__ __launch_bounds__(64) void intensity_state_kernel(Args a)
{
    const int set = blockIdx.x, lane = threadIdx.x;
    if (!set_active(a, set)) return;                             // (uniform)
    Derived d;
    int tab[2][4];
    derive_set<64>(a, set, nullptr, d, tab);
    uint32_t *hist = a.st.hist + (size_t)set * 512;
    for (int i = lane; i < 512; i += 64) hist[i] = 0;            // behind derive_set's loads of the same lanes: the next call's workspace
    if (lane == 0) {
        if (a.w_left > 0.0) {                                    // main.cpp:768: the MATCHED frame is the next prevGrayFrame
            a.st.prev_sum[set] = d.out_sum[0];
            a.st.prev_sqsum[set] = d.out_sq[0];
            a.st.has_prev[set] = 1;
        }
        if (a.record) {
            hv_intensity_record r;
            for (int cam = 0; cam < 2; ++cam) {
                r.in_sum[cam] = d.in_sum[cam]; r.in_sqsum[cam] = d.in_sq[cam];
                r.out_sum[cam] = d.out_sum[cam]; r.out_sqsum[cam] = d.out_sq[cam];
                r.k[cam] = d.t[cam].k; r.mean0[cam] = d.t[cam].mean0; r.mean[cam] = d.t[cam].mean;
            }
            r.flags = d.flags; r.reserved = 0;
            a.record[set] = r;
        }
    }
}

// the launches of one call; the caller has checked everything
int launch_match(Ctx *c, Args a)
{
    const bool aligned = ((reinterpret_cast<uintptr_t>(a.img[0]) | (a.stereo ? reinterpret_cast<uintptr_t>(a.img[1]) : 0) |
                           (uintptr_t)a.img_stride[0] | (a.stereo ? (uintptr_t)a.img_stride[1] : 0) | (uintptr_t)a.row_stride) & 15) == 0;
    a.chunks_per_row = (a.width + 15 + (aligned ? 0 : 15)) / 16;
    a.rows_per_block = max(1, BLOCK_BYTES / (16 * a.chunks_per_row));
    const unsigned blocks = (unsigned)((a.height + a.rows_per_block - 1) / a.rows_per_block);      // <= 65535 rows
    const int rewritten = (a.w_left > 0.0) + (a.stereo != 0), first_cam = a.w_left > 0.0 ? 0 : 1;
    ScopedKernelTime tm(c, HV_K_INGEST);
    hipLaunchKernelGGL(intensity_hist_kernel, dim3(blocks, a.n_sets, a.stereo ? 2 : 1), dim3(IM_THREADS), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(intensity_apply_kernel, dim3(blocks, a.n_sets, rewritten), dim3(IM_THREADS), 0, c->stream, a, first_cam);
    HV_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(intensity_state_kernel, dim3(a.n_sets), dim3(64), 0, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

// HV_ERR_INVALID first, then HV_ERR_UNSUPPORTED; nothing here looks at a context
int check_shape(int n_sets, int width, int height, int row_stride)
{
    if (n_sets < 0 || width < 1 || height < 1 || row_stride < width) return HV_ERR_INVALID;
    if (width > 65535 || height > 65535 || n_sets > 65535) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}

}  // namespace
}  // namespace hv

using hv::Ctx;

extern "C" {

void hv_intensity_default_params(hv_intensity_params *p)
{
    if (!p) return;
    p->matchSuccessiveIntensities = 0.0;
    p->matchStereoIntensities = 0;
}

int hv_intensity_init_batch_dev(hv_ctx *h, int n_sets, const hv_intensity_state *st)
{
    if (n_sets < 0 || !st || !st->prev_sum || !st->prev_sqsum || !st->has_prev || !st->hist) return HV_ERR_INVALID;
    if (n_sets > 65535) return HV_ERR_UNSUPPORTED;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    if (n_sets == 0) return HV_OK;
    HV_HIP(c, hipMemsetAsync(st->prev_sum, 0, sizeof(uint64_t) * (size_t)n_sets, c->stream));
    HV_HIP(c, hipMemsetAsync(st->prev_sqsum, 0, sizeof(uint64_t) * (size_t)n_sets, c->stream));
    HV_HIP(c, hipMemsetAsync(st->has_prev, 0, sizeof(int32_t) * (size_t)n_sets, c->stream));
    HV_HIP(c, hipMemsetAsync(st->hist, 0, sizeof(uint32_t) * 512 * (size_t)n_sets, c->stream));
    return HV_OK;
}

int hv_match_intensities_batch_dev(hv_ctx *h, const hv_intensity_params *p, int n_sets, int width, int height, uint8_t *left_dev,
                                   long long left_image_stride_bytes, uint8_t *right_dev, long long right_image_stride_bytes,
                                   int row_stride_bytes, const hv_intensity_state *st, const unsigned char *active_dev,
                                   hv_intensity_record *record_dev)
{
    if (!p || !left_dev || !st || !st->hist) return HV_ERR_INVALID;
    const double w = p->matchSuccessiveIntensities;
    if (!(w >= 0.0 && w <= 1.0)) return HV_ERR_INVALID;          // util.cpp:26 (NaN included)
    if (w > 0.0 && (!st->prev_sum || !st->prev_sqsum || !st->has_prev)) return HV_ERR_INVALID;
    if (const int rc = hv::check_shape(n_sets, width, height, row_stride_bytes)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    const int stereo = right_dev && p->matchStereoIntensities;   // main.cpp:770: useStereo && matchStereoIntensities
    if (n_sets == 0 || (!(w > 0.0) && !stereo)) return HV_OK;
    hv::Args a{};
    a.n_sets = n_sets; a.width = width; a.height = height; a.row_stride = row_stride_bytes;
    a.img[0] = left_dev; a.img_stride[0] = left_image_stride_bytes;
    a.img[1] = stereo ? right_dev : nullptr; a.img_stride[1] = stereo ? right_image_stride_bytes : 0;
    a.w_left = w; a.w_right = stereo ? 1.0 : 0.0; a.stereo = stereo;
    a.st = *st; a.active = active_dev; a.record = record_dev;
    return hv::launch_match(c, a);
}

int hv_match_intensities(hv_ctx *h, int width, int height, const uint8_t *l_host, int l_stride_bytes, uint8_t *r_host, int r_stride_bytes,
                         double weight)
{
    if (!l_host || !r_host || !(weight >= 0.0 && weight <= 1.0)) return HV_ERR_INVALID;
    if (const int rc = hv::check_shape(1, width, height, l_stride_bytes < r_stride_bytes ? l_stride_bytes : r_stride_bytes)) return rc;
    Ctx *c = hv::ctx_of(h);
    if (!c) return HV_ERR_INVALID;
    const size_t row = ((size_t)width + 15) & ~(size_t)15, image = row * (size_t)height;
    hv::Stage s(c);
    const auto o_img = s.take<uint8_t>(2 * image);
    const auto o_hist = s.take<uint32_t>(512);
    if (const int rc = s.reserve()) return rc;
    uint8_t *d_img = s.at(o_img);
    HV_HIP(c, hipMemcpy2DAsync(d_img, row, l_host, l_stride_bytes, width, height, hipMemcpyHostToDevice, c->stream));
    HV_HIP(c, hipMemcpy2DAsync(d_img + image, row, r_host, r_stride_bytes, width, height, hipMemcpyHostToDevice, c->stream));
    HV_HIP(c, hipMemsetAsync(s.at(o_hist), 0, sizeof(uint32_t) * 512, c->stream));
    hv::Args a{};
    a.n_sets = 1; a.width = width; a.height = height; a.row_stride = (int)row;
    a.img[0] = d_img; a.img[1] = d_img + image;
    a.w_left = 0.0; a.w_right = weight; a.stereo = 1;            // matchIntensities(l, r, weight): the stereo step with a weight
    a.st.hist = s.at(o_hist);
    if (const int rc = hv::launch_match(c, a)) return rc;
    HV_HIP(c, hipMemcpy2DAsync(r_host, r_stride_bytes, d_img + image, row, width, height, hipMemcpyDeviceToHost, c->stream));
    HV_HIP(c, hipStreamSynchronize(c->stream));
    return HV_OK;
}

}  // extern "C"
