// Stand-alone chi2 gates of the EKF for many filters at once (the family map is in ekf.hip): the streaming dense gate, the
// column-sparse gates over the compact Jacobians of a prepare launch, and their launchers. The designs are described at the kernels.
#include "ekf_device.hpp"
#include "ekf_host.hpp"

// The library is built with -ffp-contract=off for the tracker's bit-exact binary32 sequence; the
// EKF is judged against a relative tolerance, and a fused multiply-add is one rounding fewer and
// half the f64 instructions of its dependency chains.
#pragma clang fp contract(fast)

namespace hv {

namespace {

// ---------------------------------------------------------------------------------------------
// chi2 gate for MANY filters at once (throughput launches): S = H P H' + R without ever holding H P.
//
// ekf_update_kernel keeps P in registers (8 waves x 256 VGPRs) and the tall matrix in 134 KB of LDS so that an UPDATE reads P
// once -- one filter per CU at a time, its phases (products, S, a 40-pivot Cholesky) strictly one after the other: a gate launch over
// 1024 filters is 4 rounds of a 33 us latency chain at 32 % MFMA busy. A gate needs none of that state. Here a wavefront
// owns 16-column blocks J of P and chains two MFMA products per block through its accumulators:
//     G_J = P(J, :) H'          (16 x nr; A = tiles of P streamed from HBM, B = H' from LDS)
//     S  += H(:, J) G_J         (nr x nr; A = H from LDS, B = G_J -- the accumulator tile of the first product IS the B operand
//                                layout of the second: lane (kq, c) holds rows 4 v + kq, exactly the k order of a k-step)
// so H P never exists, LDS holds H (61 KB) + S (15 KB) and two workgroups of 4 waves share a CU: one filter's Cholesky runs under
// the other's MFMAs. P(J, k) is read as stored (no symmetry assumption). The factorisation / chi2 part is the blocked Cholesky of
// ekf_update_kernel restricted to the measurement rows.
// ---------------------------------------------------------------------------------------------
struct GateArgs {
    int n, nr, l, Rs;                 // Rs: column stride of the (nr + 1) x nr matrix [S; v'] in LDS
    const double *P;                  // [batch][n][n]
    const double *H, *v;              // [batch] records: nr x l column-major, nr
    double rd, noise_scale;
    double *chi2; int *status;
    const unsigned char *active;
    const int *success_counter; int max_successful;      // optional: filters whose quota is used up are skipped
};

constexpr int GATE_THREADS = 256;

template <int TI>
__global__ __launch_bounds__(GATE_THREADS, 2) void ekf_gate_stream_kernel(GateArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int b = blockIdx.x;
    if (a.active && !a.active[b]) return;
    if (a.success_counter && a.success_counter[b] >= a.max_successful) return;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    constexpr int nwaves = GATE_THREADS / 64, nrp = 16 * TI;
    const int n = a.n, nr = a.nr, l = a.l, R = a.Rs;
    const double *P = a.P + (size_t)b * n * n, *H = a.H + (size_t)b * nr * l;
    const int lb = (l + 15) >> 4;
    // LDS: Hs [16 lb][nrp] (k-major, zero padded) | T [(nr + 1) x nr, stride R] ; W / col / red live in Hs once the products are done
    const GateStreamLds L = gate_stream_lds(TI, lb, R, nr);
    double *Hs = smem + L.Hs, *T = smem + L.T;
    const int kq = lane >> 4, cl = lane & 15;
    // ---- stage H (zero padded) and zero T ----
    for (int i = t; i < nrp * 16 * lb; i += GATE_THREADS) {
        const int k = i / nrp, r = i - k * nrp;
        Hs[i] = (k < l && r < nr) ? H[(size_t)k * nr + r] : 0.0;
    }
    for (int i = t; i < R * nr; i += GATE_THREADS) T[i] = 0.0;
    __syncthreads();
    // ---- products: this wave's column blocks J = wave, wave + 4, .. ----
    double4v accS[TI * (TI + 1) / 2];
#pragma unroll
    for (int u = 0; u < TI * (TI + 1) / 2; u++) accS[u] = double4v{0.0, 0.0, 0.0, 0.0};
    constexpr int DEPTH = 4;                                    // K blocks of P requested ahead of their MFMAs
    for (int J = wave; J < lb; J += nwaves) {
        const int jrow = min(J * 16 + cl, n - 1);
        auto fetch = [&](double (&pv)[4], int kb) {
#pragma unroll
            for (int sx = 0; sx < 4; sx++) pv[sx] = P[(size_t)min(kb * 16 + 4 * sx + kq, n - 1) * n + jrow];   // A(i = cl, k): P(J16 + cl, k)
        };
        double pv[DEPTH][4];
#pragma unroll
        for (int d = 0; d < DEPTH; d++) if (d < lb) fetch(pv[d], d);
        double4v accG[TI];
#pragma unroll
        for (int ct = 0; ct < TI; ct++) accG[ct] = double4v{0.0, 0.0, 0.0, 0.0};
        for (int kb0 = 0; kb0 < lb; kb0 += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; d++) {
                const int kb = kb0 + d;
                if (kb < lb) {
                    double hb[4][TI];
#pragma unroll
                    for (int sx = 0; sx < 4; sx++)
#pragma unroll
                        for (int ct = 0; ct < TI; ct++) hb[sx][ct] = Hs[(size_t)(kb * 16 + 4 * sx + kq) * nrp + 16 * ct + cl];   // B(k, c) = H(c, k)
#pragma unroll
                    for (int sx = 0; sx < 4; sx++)
#pragma unroll
                        for (int ct = 0; ct < TI; ct++)
                            accG[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(pv[d][sx], hb[sx][ct], accG[ct], 0, 0, 0);
                    if (kb + DEPTH < lb) fetch(pv[d], kb + DEPTH);
                }
            }
        }
        // S(rt, ct) += H(16 rt + i, J16 + k) G_J(k, 16 ct + c), lower tiles; k-step v: A = H(.., J16 + 4 v + kq), B = accG[ct][v]
        if (J * 16 < n) {
#pragma unroll
            for (int v = 0; v < 4; v++) {
                double ha[TI];
#pragma unroll
                for (int rt = 0; rt < TI; rt++) ha[rt] = Hs[(size_t)(J * 16 + 4 * v + kq) * nrp + 16 * rt + cl];                 // A(i = cl, k)
                int u = 0;
#pragma unroll
                for (int ct = 0; ct < TI; ct++)
#pragma unroll
                    for (int rt = ct; rt < TI; rt++, u++)
                        accS[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(ha[rt], accG[ct][v], accS[u], 0, 0, 0);
            }
        }
    }
    // ---- the waves' partial S meet in LDS in WAVE ORDER (r05: one wave per round, a barrier between the rounds -- with ds_add_f64 in
    // arrival order, r01 .. r04, two runs could differ by ~1 ulp of S) ----
    for (int w_turn = 0; w_turn < nwaves; ++w_turn) {
        if (wave == w_turn) {
            int u = 0;
#pragma unroll
            for (int ct = 0; ct < TI; ct++)
#pragma unroll
                for (int rt = ct; rt < TI; rt++, u++)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int i = 16 * rt + kq + 4 * q, c = 16 * ct + cl;
                        if (i < nr && c < nr && i >= c) T[(size_t)c * R + i] += accS[u][q];
                    }
        }
        __syncthreads();
    }
    for (int i = t; i < nr; i += GATE_THREADS) { T[(size_t)i * R + i] += a.rd; T[(size_t)i * R + nr] = a.v[(size_t)b * nr + i]; }
    double *W = Hs + CHOL_W, *col = Hs + CHOL_COL, *red = Hs + CHOL_RED;    // H is dead from here on
    __syncthreads();
    // ---- blocked Cholesky of [S; v'] (see ekf_update_kernel phase C), rows 0 .. nr ----
    const int Rlim = nr + 1;
    for (int j0 = 0; j0 < nr; j0 += 16) {
        const int w = min(16, nr - j0);
        const int ntile = (Rlim - j0 + 15) / 16;
        if (j0 > 0) {
            for (int tile = wave; tile < ntile; tile += nwaves) {
                const int i0 = j0 + 16 * tile, mi = Rlim - i0;
                const double4v acc = mfma_tile(T + i0, 1, R, mi, T + j0, R, 1, w, j0);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int i = kq + 4 * q;
                    if (i < mi && cl < w) T[(size_t)(j0 + cl) * R + i0 + i] -= acc[q];
                }
            }
            __syncthreads();
        }
        if (wave == 0) { if (w <= 8) factor_diag_block<8>(T, W, col, R, j0, w, lane); else factor_diag_block<16>(T, W, col, R, j0, w, lane); }
        __syncthreads();
        for (int i0 = j0 + w + 16 * wave; i0 < Rlim; i0 += 16 * nwaves) {
            const int mi = Rlim - i0;
            const double4v acc = mfma_tile(T + (size_t)j0 * R + i0, 1, R, mi, W, 16, 1, 16, w);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int i = kq + 4 * q;
                if (i < mi && cl < w) T[(size_t)(j0 + cl) * R + i0 + i] = acc[q];
            }
        }
        __syncthreads();
    }
    // ---- chi2 = noise_scale * z'z ----
    double sz = 0;
    for (int c = t; c < nr; c += GATE_THREADS) { const double z = T[(size_t)c * R + nr]; sz += z * z; }
    for (int o = 32; o > 0; o >>= 1) sz += __shfl_down(sz, o);
    if (lane == 0) red[wave] = sz;
    __syncthreads();
    if (t == 0) {
        double tot = 0; for (int w2 = 0; w2 < nwaves; w2++) tot += red[w2];
        tot *= a.noise_scale;
        if (a.chi2) a.chi2[b] = tot;
        // (a non-positive pivot leaves NaN / inf in z: reported as CHI2, as by ekf_update_kernel phase D and the sparse gates -- the bare
        //  comparison is false for a NaN and called such a filter an inlier)
        const bool broken = !(tot < 1e300);
        if (a.status) a.status[b] = (broken || tot > d_chi2inv95[nr]) ? 3 /*CHI2*/ : 0 /*INLIER*/;
    }
}

// ---------------------------------------------------------------------------------------------
// Column-sparse chi2 gate as its own launch (many filters): visualTrackOutlierCheck on the compact Jacobians the prepare launch left
// in HBM (VuPrepareArgs::fused == 2). One 4-wave workgroup per filter -- four waves sit one per SIMD, so the (J, ct) items of
// sparse_gate spread evenly over the matrix pipes --, LDS = Hc (28 KB at 10 stereo poses) + [S; v'] (15 KB): three workgroups per CU,
// whose single-wave Cholesky chains (40 dependent pivots, ~10 us) run under each other's products. The same chain inside the
// prepare kernel (two 80 KB workgroups per CU, both latency chains themselves) cost 60 us per 1024 filters (r03 measurements).
// ---------------------------------------------------------------------------------------------
struct SparseGateArgs {
    int n, nr, ncam, na_max;          // state dimension; rows of the longest record (= record stride of v); cameras; columns per Hc record
    const double *P;                  // [batch][n][n]
    const double *Hc, *v;             // [batch][nr * na_max] compact Jacobians (leading dimension: the record's rows), [batch][nr]
    const int *acol;                  // [batch][na_max]
    const int *nr_rec;                // ragged batches: rows of every record, or null
    const unsigned char *active;      // [batch]: 1 where triangulation and prepareVisualUpdate passed (written by the prepare launch)
    double rd, noise_scale;
    double *chi2; int *status;        // chi2 optional
    int hs_doubles;                   // LDS carve (SparseGateLds::T): doubles reserved for the staged Hc (it is the Cholesky scratch afterwards)
    int lds_doubles;                  // doubles available for Hc + [S; v'] together (BIG build: decides between the padded and the tight layout)
    int batch;
    const int *rec_count, *rec_list;  // this launch's records (compaction list of the long class), or null
    int *inl_count, *inl_list;        // appended: records whose gate said INLIER
};

constexpr int SGATE_THREADS = 256;         // small build: four waves, one per SIMD, three workgroups per CU
constexpr int SGATE_BIG_THREADS = 768;     // big build (one workgroup per CU by its LDS): three waves per SIMD for the 20 (J, group) items of an 84-row track (512 threads: 70.9 us per 256 records of 21 poses, 768: 66.7, 1024: 87 spilled VGPRs)

// BIG = false: up to 48 rows (three 43 KB workgroups per CU at 10 stereo poses); BIG = true: 49 .. 96 rows (tracks of 13 .. 21 stereo
// poses: 13 .. 21 poses x 4 rows), one workgroup per CU with the whole register file, Hc staged with nrp = 16 TI rows per column where that
// fits 160 KB together with [S; v'] and with 84 rows (TIGHT) where it does not (84 rows: 99.5 + 58.5 KB).
template <bool BIG>
__device__ __forceinline__ void sparse_gate_kernel_body(const SparseGateArgs &a, const int b_in)
{
    // (the record index may come out of a compaction list, i.e. a per-lane load: on the scalar unit every base address below is
    //  uniform and the P gather becomes scalar base + 32-bit lane offset)
    const int b = __builtin_amdgcn_readfirstlane(b_in);
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int t = threadIdx.x;
    constexpr int NTH = BIG ? SGATE_BIG_THREADS : SGATE_THREADS;
    PHASE_STAMP(12);
    // (flag, shape, column list and residual requested together: one round trip instead of three dependent ones)
    const unsigned char act_v = a.active[b];
    const int nr_v = a.nr_rec ? a.nr_rec[b] : a.nr;
    int my_acol_raw = a.acol[(size_t)b * a.na_max + min(t, a.na_max - 1)];
    double my_v_raw = a.v[(size_t)b * a.nr + min(t, a.nr - 1)];
    asm volatile("" : "+v"(my_acol_raw), "+v"(my_v_raw));
    if (!act_v) return;                                        // status stays NOT_COMPUTED (preset by the prepare launch)
    const int nr = __builtin_amdgcn_readfirstlane(nr_v);
    if (nr < 2 || nr > a.nr) return;
    const int n = a.n, npose = nr / (2 * a.ncam), na = 7 * npose + 1, na4 = (na + 3) & ~3;
    const int ti = BIG ? max((nr + 15) >> 4, 4) : (nr + 15) >> 4;       // (the BIG build starts at the 4-tile instantiation; chooses the sparse_gate instantiation below)
    const SparseGateShape shape = sparse_gate_shape(BIG, nr, na4, (size_t)a.lds_doubles);    // (uniform) does the padded layout fit?
    const bool tight = shape.tight;
    const int Rs = shape.Rs, nrp = shape.nrp;
    if (tight && nr > HV_GATE_TIGHT_ROWS) return;              // (the launcher sizes LDS for <= 84 rows: never taken)
    double *Hs = smem, *T = smem + a.hs_doubles;
    int *s_acol = reinterpret_cast<int *>(T + (size_t)Rs * nr);
    const double *Hc = a.Hc + (size_t)b * a.nr * a.na_max;
    // stage Hc k-major with zero padding (rows >= nr, columns >= na), [S; v'] zeroed with the residual row in place
    // (8 elements per thread in flight: a load -> LDS store loop without unrolling waits one HBM / L2 round trip per iteration -- 14 of
    // them at 10 stereo poses, which made this staging half of the kernel)
    const int my_acol = t < na ? my_acol_raw : 0;
    const double my_v = t < nr ? my_v_raw : 0.0;
    const int total = na4 * nrp;
    const unsigned inv_nrp = (unsigned)((0x100000000ull + (unsigned)nrp - 1) / (unsigned)nrp);       // i / nrp = umulhi(i, ceil(2^32 / nrp))
    for (int base = 0; base < total; base += 8 * NTH) {
        double hv_[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int i = base + q * NTH + t, u = (int)__umulhi((unsigned)i, inv_nrp), r = i - u * nrp;
            const bool live = i < total && u < na && r < nr;
            hv_[q] = live ? Hc[(size_t)(live ? u : 0) * nr + (live ? r : 0)] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int i = base + q * NTH + t;
            if (i < total) Hs[i] = hv_[q];
        }
    }
    for (int i = t; i < Rs * nr; i += NTH) T[i] = 0.0;             // (row nr of column c is rewritten below by thread c: same thread order
    if (t < na) s_acol[t] = my_acol;                                           //  is not guaranteed, so the barrier comes first)
    __syncthreads();
    if (t < nr) T[(size_t)t * Rs + nr] = my_v;
    __syncthreads();
    PHASE_STAMP(13);
    const double *Pb = a.P + (size_t)b * n * n;
    // nobody reads chi2: the factorisation may stop once the track is certainly rejected (gate_exit_threshold, gate_factor_chi2)
    const bool early_exit = a.chi2 == nullptr;
    double chi;
    if constexpr (!BIG) {
        if (ti == 1)      chi = sparse_gate<1, NTH, true>(Pb, n, s_acol, na, Hs, T, Rs, nr, a.rd, a.noise_scale, Hs, BIG ? PHASE_STAMP_ARRAY : nullptr, early_exit);
        else if (ti == 2) chi = sparse_gate<2, NTH, true>(Pb, n, s_acol, na, Hs, T, Rs, nr, a.rd, a.noise_scale, Hs, BIG ? PHASE_STAMP_ARRAY : nullptr, early_exit);
        else              chi = sparse_gate<3, NTH, true>(Pb, n, s_acol, na, Hs, T, Rs, nr, a.rd, a.noise_scale, Hs, BIG ? PHASE_STAMP_ARRAY : nullptr, early_exit);
    } else {
        if (ti <= 4)      chi = sparse_gate<4, NTH, false>(Pb, n, s_acol, na, Hs, T, Rs, nr, a.rd, a.noise_scale, Hs, BIG ? PHASE_STAMP_ARRAY : nullptr, early_exit);
        else if (ti == 5) chi = sparse_gate<5, NTH, false>(Pb, n, s_acol, na, Hs, T, Rs, nr, a.rd, a.noise_scale, Hs, BIG ? PHASE_STAMP_ARRAY : nullptr, early_exit);
        else if (!tight)  chi = sparse_gate<6, NTH, false>(Pb, n, s_acol, na, Hs, T, Rs, nr, a.rd, a.noise_scale, Hs, BIG ? PHASE_STAMP_ARRAY : nullptr, early_exit);
        else              chi = sparse_gate<6, NTH, false, true>(Pb, n, s_acol, na, Hs, T, Rs, nr, a.rd, a.noise_scale, Hs, BIG ? PHASE_STAMP_ARRAY : nullptr, early_exit);
    }
    if (t == 0) {
        const bool broken = !(chi < 1e300);                    // non-positive pivot: reported as CHI2 (ekf_update_kernel phase D)
        const int outlier = broken || ((nr < HV_CHI2INV95_N) ? (chi > d_chi2inv95[nr]) : 0);
        a.status[b] = outlier ? 3 /*CHI2*/ : 0 /*INLIER*/;
        if (!outlier && a.inl_list) a.inl_list[atomicAdd(a.inl_count, 1)] = b;
        if (a.chi2) a.chi2[b] = chi;
    }
}

__global__ __launch_bounds__(SGATE_THREADS, 3) void ekf_sparse_gate_kernel(SparseGateArgs a) { sparse_gate_kernel_body<false>(a, blockIdx.x); }
__global__ __launch_bounds__(SGATE_BIG_THREADS, 1) void ekf_sparse_gate_big_kernel(SparseGateArgs a)
{
    int b = blockIdx.x;
    if (a.rec_list) { if (b >= *a.rec_count) return; b = a.rec_list[b]; }
    sparse_gate_kernel_body<true>(a, b);
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
int ekf_launch_gate_stream(Ekf *e, const GateStreamRequest &rq)
{
    Ctx *c = e->c;
    const int nr = rq.nr, l = rq.l;
    bool *done = rq.done;
    *done = false;
    if (nr < 1 || nr > 48 || nr >= HV_CHI2INV95_N || l < 1 || l > e->n) return HV_OK;        // the caller keeps its other route
    GateArgs a{};
    a.n = e->n; a.nr = nr; a.l = l;
    a.Rs = lds_stride(nr + 1);
    a.P = e->fixed.P; a.H = rq.H_dev; a.v = rq.v_dev; a.rd = rq.rd; a.noise_scale = e->noise_scale; a.chi2 = rq.chi2_dev; a.status = rq.status_dev;
    a.active = rq.active_dev; a.success_counter = rq.success_counter_dev; a.max_successful = rq.max_successful;
    const int ti = tiles16(nr);
    const GateStreamLds L = gate_stream_lds(ti, tiles16(l), a.Rs, nr);
    if (!gate_stream_admitted(L)) return HV_OK;                               // W / col / red borrow the H area; the gate limit
    using Kern = void (*)(GateArgs);
    const Kern kern = ti == 1 ? (Kern)ekf_gate_stream_kernel<1> : ti == 2 ? (Kern)ekf_gate_stream_kernel<2> : (Kern)ekf_gate_stream_kernel<3>;
    ScopedKernelTime tm(c, HV_K_EKF_UPDATE);
    hipLaunchKernelGGL(kern, dim3(e->batch), dim3(GATE_THREADS), lds_bytes(L), c->stream, a);
    HV_HIP(c, hipGetLastError());
    *done = true;
    return HV_OK;
}

int ekf_launch_sparse_gate(Ekf *e, const SparseGateRequest &rq)
{
    Ctx *c = e->c;
    const int np = rq.np, ncam = rq.ncam;
    const hipStream_t stream = rq.stream ? rq.stream : c->stream;
    const int nr = 2 * np * ncam, na_max = 7 * np + 1;
    if (nr < 2 || nr > 96 || nr >= HV_CHI2INV95_N || !rq.active_dev || !rq.status_dev) return HV_ERR_INVALID;
    const SparseGateLds L = sparse_gate_lds(np, ncam);      // sized for the launch's longest record
    if (!L.supported) return HV_ERR_UNSUPPORTED;
    SparseGateArgs a{};
    a.n = e->n; a.nr = nr; a.ncam = ncam; a.na_max = na_max; a.P = e->fixed.P; a.Hc = rq.Hc_dev; a.v = rq.v_dev; a.acol = rq.acol_dev; a.nr_rec = rq.nr_rec_dev;
    a.active = rq.active_dev; a.rd = rq.rd; a.noise_scale = e->noise_scale; a.chi2 = rq.chi2_dev; a.status = rq.status_dev;
    a.hs_doubles = (int)(L.T - L.Hs); a.lds_doubles = (int)(L.acol - L.Hs);
    ScopedKernelTime tm(c, HV_K_EKF_GATE, stream);
    a.rec_count = rq.rec_count; a.rec_list = rq.rec_list; a.inl_count = rq.inl_count; a.inl_list = rq.inl_list;
    a.batch = e->batch;
    if (L.big) hipLaunchKernelGGL(ekf_sparse_gate_big_kernel, dim3((unsigned)e->batch), dim3(SGATE_BIG_THREADS), L.bytes, stream, a);
    else       hipLaunchKernelGGL(ekf_sparse_gate_kernel, dim3(e->batch), dim3(SGATE_THREADS), L.bytes, stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

// the kernels' dynamic-LDS limits (ekf_kernels_init)
int ekf_gate_init(Ctx *c)
{
    HV_HIP(c, set_lds_limit(ekf_gate_stream_kernel<1>, LDS_GATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_gate_stream_kernel<2>, LDS_GATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_gate_stream_kernel<3>, LDS_GATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_sparse_gate_kernel, LDS_GATE_LIMIT));
    HV_HIP(c, set_lds_limit(ekf_sparse_gate_big_kernel, LDS_SGATE_BIG_LIMIT));
    return HV_OK;
}

#ifdef HV_EKF_PHASE_STAMPS
hipError_t ekf_gate_phase_stamps(long long *out16) { return hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_phase_stamp), sizeof(long long) * 16); }
#endif

}  // namespace hv
