// The sample-consensus skeleton of the stereo track filters (ransac3.hip, upright2p.hip): every phase that does not depend on the minimal
// problem, written once -- the tail of the correspondence phase, the sampler, the cost phase, the loop's rule, the output phase and the
// round loop that chains them -- and, on the host, the parameter check, the common kernel arguments and the staged synchronous entry.
// The loop follows the recollection of Theia's estimator stated in tests/ransac3_restatement.py and tests/upright2p_restatement.py.
//
// A file describes its problem as a struct P of constants and static device functions:
//   SAMPLE (points per hypothesis), SOLUTIONS (models per hypothesis), MODEL (doubles per model), THREADS, CHUNK (iterations per round;
//   CHUNK * SOLUTIONS = THREADS, one lane per model), TYPE (RansacResult::Type of a success), View (its LDS view, derived from ScView)
//   correspondences(v, pl, pr, cl, n, cap, tid) -> m   phase a: its own per-lane loop, then compact_and_init below
//   models(v, h, tid, M) -> have                       phase c: lane tid's model of the round's h hypotheses into M (and s_mod)
//   residual(M, v, j)                                  squared error of correspondence j under model M
//   write_model(out, best, success)                    the 12 doubles of the output
//
// No include guard and no namespace of its own, like hv_workgroup.hpp: a translation unit includes it once, inside its anonymous
// namespace, after hv_internal.hpp, ransac_lds.hpp and hv_workgroup.hpp (block_compact, block_gather_front).

constexpr int SC_MAX_PTS = 1024;

struct ScArgs {                           // the kernel arguments both filters carry
    int max_points, max_iters, min_iters, use_mle, cap, tail;
    const int *n_points;
    const float *pl, *pr, *cl;            // previous-left, previous-right, current-left corners [sets][max_points][2]
    const uint32_t *draws;                // [sets][SAMPLE * max_iters] raw std::mt19937 outputs
    int *status;                          // [sets][max_points] Feature::Status in/out (TRACKED selects)
    const int *r2_summary;                // tail: RANSAC2's {bestInlierCount, visited}
    int *result;                          // tail: [sets][2] {type, inlierCount}
    double *score;                        // tail: [sets]
    double *model;                        // [sets][12] or NULL
    int *summary;                         // [sets][4] or NULL
    double thr, logp;
    double T[16];                         // secondToFirstCamera, row-major
    hv_camera_model cam0, cam1;
};

// a workgroup's LDS: the sections both layouts of ransac_lds.hpp have, as pointers (sample: tri / pair), the staged cameras and
// secondToFirstCamera; a file's view adds its point arrays
struct ScView {
    double *mod, *cost, *best;
    int *map, *vmap, *st, *idx, *chunk, *sample;
    unsigned *draw;
    int *cnt, *ctl;
    const hv_camera_model *cam;
    const double *T;
};
template <class Lds>
__device__ __forceinline__ ScView sc_view(unsigned char *base, const Lds &L, size_t sample, const hv_camera_model *cam, const double *T)
{
    auto d = [&](size_t off) { return reinterpret_cast<double *>(base + off); };
    auto i = [&](size_t off) { return reinterpret_cast<int *>(base + off); };
    return ScView{d(L.mod), d(L.cost), d(L.best), i(L.map), i(L.vmap), i(L.st), i(L.idx), i(L.chunk), i(sample),
                  reinterpret_cast<unsigned *>(base + L.draw), i(L.cnt), i(L.ctl), cam, T};
}

// ComputeMaxIterations for a sample of K (restatements: compute_max_iterations); the power in their operation order
template <int K> __host__ __device__ inline int max_iterations_for(double ratio, double logp, int min_it, int max_it)
{
    static_assert(K == 2 || K == 3, "ratio * ratio, (ratio * ratio) * ratio");
    if (ratio <= 0.0) return max_it;
    if (ratio == 1.0) return min_it;
    const double lp = log(1.0 - (K == 2 ? ratio * ratio : (ratio * ratio) * ratio)) - DBL_EPSILON;
    double v = ceil(logp / lp);
    v = v < (double)min_it ? (double)min_it : v;
    v = v > (double)max_it ? (double)max_it : v;
    return (int)v;
}

// ---- the phases. Every thread of the workgroup calls every phase; each header says which barriers the phase holds and what they
// publish ----

// a, behind the problem's per-lane loop, which has filled s_st (1: a correspondence) and the NA point arrays for the n tracked features:
// the m survivors compacted to the front (order kept), every status preset to RANSAC_OUTLIER, the sampler's index vector and the loop's
// control words {iteration, limit, best iteration, inliers} initialised. Returns m. Barriers: one at the start (publishes s_st and the
// points), block_compact's three, block_gather_front's one; ends with one, which publishes the gathered points, s_st, s_idx and s_ctl.
template <class P, int NA> __device__ __forceinline__ int compact_and_init(const ScView &v, double *const (&pts)[NA], int n, int cap, int tid)
{
    static_assert(SC_MAX_PTS <= 4 * P::THREADS, "four points per thread");
    __syncthreads();
    const int m = block_compact<P::THREADS / 64>([&](int k) { return v.st[k] != 0; }, v.vmap, n, v.chunk);
    block_gather_front<P::THREADS>(pts, v.vmap, m);
    for (int k = tid; k < n; k += P::THREADS) v.st[k] = 3;
    for (int j = tid; j < m; j += P::THREADS) v.idx[j] = j;
    if (tid == 0) { v.ctl[0] = 0; v.ctl[1] = cap; v.ctl[2] = -1; v.ctl[3] = 0; }
    __syncthreads();
    return m;
}

// b. The sampler for the h iterations from it0: the raw draws go to LDS, a barrier publishes them, then lane 0 replays the partial
// shuffle idx[i] <-> idx[i + raw % (m - i)], i < SAMPLE (positions below SAMPLE are lane 0's registers head[], the rest is s_idx),
// and hands each sample over in ascending index order. Ends with a barrier, which publishes s_sample.
template <class P> __device__ __forceinline__ void sampler(const ScView &v, const uint32_t *draws, int it0, int h, int m, int (&head)[P::SAMPLE], int tid)
{
    constexpr int S = P::SAMPLE;
    static_assert(S * P::CHUNK <= P::THREADS, "one draw per thread");
    if (tid < S * h) v.draw[tid] = draws[S * it0 + tid];
    __syncthreads();
    if (tid == 0) {
        for (int k = 0; k < h; ++k) {
            unsigned raw[S];                                                // read before the first store to s_idx, which may alias
#pragma unroll
            for (int i = 0; i < S; ++i) raw[i] = v.draw[S * k + i];
#pragma unroll
            for (int i = 0; i < S; ++i) {
                const int j = i + (int)(raw[i] % (unsigned)(m - i));
                int &mine = head[i];
                if (j >= S) { const int o = v.idx[j]; v.idx[j] = mine; mine = o; }
                else {                                                      // (selects, not branches: lane 0's serial path)
#pragma unroll
                    for (int q = i + 1; q < S; ++q) { const int o = head[q]; head[q] = q == j ? mine : o; mine = q == j ? o : mine; }
                }
            }
            // the solver's canonical order: ascending indices (a repeated sample repeats its models bit for bit)
            int s[S];
#pragma unroll
            for (int i = 0; i < S; ++i) s[i] = head[i];
#pragma unroll
            for (int pass = S - 1; pass > 0; --pass)
#pragma unroll
                for (int i = 0; i < pass; ++i) { const int lo = min(s[i], s[i + 1]), hi = max(s[i], s[i + 1]); s[i] = lo; s[i + 1] = hi; }
#pragma unroll
            for (int i = 0; i < S; ++i) v.sample[S * k + i] = s[i];
        }
    }
    __syncthreads();
}

// d. Cost and inlier count of the lane's model (have: the lane has one, in M) over all m correspondences, added in order, into s_cost
// and s_cnt (-1: no model). Ends with a barrier, which publishes both (and s_mod, where phase c has no barrier of its own).
template <class P> __device__ __forceinline__ void cost_and_count(const typename P::View &v, bool have, const double *M, int m, double thr, int use_mle, int tid)
{
    double cost = 0.0;
    int cnt = -1;
    if (have) {
        cnt = 0;
        for (int j = 0; j < m; ++j) {
            const double r = P::residual(M, v, j);
            const bool in = r < thr;
            cnt += in ? 1 : 0;
            cost = cost + (in ? r : thr);
        }
        if (!use_mle) cost = (double)(m - cnt);
    }
    v.cnt[tid] = cnt; v.cost[tid] = cost;
    __syncthreads();
}

// e. The loop's rule, replayed by lane 0 over the stored costs of the round: strict `<`, adaptive limit; the best model goes to s_best,
// the control words are brought up to date. Ends with a barrier, which publishes s_ctl (the loop's condition reads it) and s_best.
template <class P> __device__ __forceinline__ void loop_rule(const ScView &v, const ScArgs &a, int it0, int limit, int h, int m, double &best_cost, int tid)
{
    if (tid == 0) {
        int it = it0, lim = limit;
        for (int k = 0; k < h && it < lim; ++k, ++it)
            for (int s = 0; s < P::SOLUTIONS; ++s) {
                const int w = P::SOLUTIONS * k + s, cnt = v.cnt[w];
                if (cnt >= 0 && v.cost[w] < best_cost) {
                    best_cost = v.cost[w];
                    for (int i = 0; i < P::MODEL; ++i) v.best[i] = v.mod[P::MODEL * w + i];
                    v.ctl[2] = it; v.ctl[3] = cnt;
                    const double ratio = (double)cnt / (double)m;
                    if (!(ratio < (double)P::SAMPLE / (double)m))
                        lim = min(max_iterations_for<P::SAMPLE>(ratio, a.logp, a.min_iters, a.max_iters), lim);
                }
            }
        v.ctl[0] = it; v.ctl[1] = lim;
    }
    __syncthreads();
}

// f. The best model's inliers go back to TRACKED; statuses, model, summary and the tail of RansacPipeline::compute
// (ransac_pipeline.cpp:139-144). Two barriers: one publishes the zeroed counter s_ctl[4], one the inlier count and s_st. Begins and
// ends without one.
template <class P>
__device__ __forceinline__ void inliers_and_outputs(const typename P::View &v, const ScArgs &a, int set, int *ts, int n_all, int n, int m, bool run, int tid)
{
    const int iters = v.ctl[0], best_it = v.ctl[2];
    const bool success = run && best_it >= 0;
    if (tid == 0) v.ctl[4] = 0;
    __syncthreads();
    if (success) {
        double M[P::MODEL];
#pragma unroll
        for (int i = 0; i < P::MODEL; ++i) M[i] = v.best[i];
        int cnt = 0;
        for (int j = tid; j < m; j += P::THREADS)
            if (P::residual(M, v, j) < a.thr) { v.st[v.vmap[j]] = 0; ++cnt; }
        if (cnt) atomicAdd(&v.ctl[4], cnt);
    }
    __syncthreads();
    const int count = v.ctl[4];
    if (tid == 0) {
        if (a.model) P::write_model(a.model + 12 * (size_t)set, v.best, success);
        if (a.summary) {
            int *sm = a.summary + 4 * (size_t)set;
            sm[0] = count; sm[1] = success ? best_it : -1; sm[2] = run ? iters : 0; sm[3] = m;
        }
    }
    if (a.tail && !success) {                                                // SKIPPED: every track is cleared (:139-144)
        for (int i = tid; i < n_all; i += P::THREADS) ts[i] = 3;
    } else {
        for (int k = tid; k < n; k += P::THREADS) ts[v.map[k]] = v.st[k];
    }
    if (a.tail && tid == 0) {
        a.result[2 * (size_t)set] = success ? P::TYPE : 0;
        a.result[2 * (size_t)set + 1] = count;
        const int r2count = n >= 2 ? a.r2_summary[2 * set] : 0;              // doRansac2 does not run below two tracks (:210)
        a.score[set] = n ? (double)r2count / (double)n : 0.0;
    }
}

// The body of both kernels, behind what the kernel itself stages (the cameras, secondToFirstCamera, upright 2-point: the rotations):
// one workgroup per point set, phases a .. f. Begins with the barrier that publishes the staged data.
template <class P> __device__ __forceinline__ void sample_consensus(const typename P::View &v, const ScArgs &a)
{
    static_assert(P::CHUNK * P::SOLUTIONS == P::THREADS, "one lane per (hypothesis, solution)");
    const int set = blockIdx.x, tid = threadIdx.x;
    const int MP = a.max_points;
    __syncthreads();
    const int n_all = min(max(a.n_points[set], 0), MP);
    const float *pl = a.pl + (size_t)set * MP * 2, *pr = a.pr + (size_t)set * MP * 2, *cl = a.cl + (size_t)set * MP * 2;
    int *ts = a.status + (size_t)set * MP;

    // the set: TRACKED features in feature order
    const int n = block_compact<P::THREADS / 64>([&](int i) { return ts[i] == 0; }, v.map, n_all, v.chunk);
    const int m = P::correspondences(v, pl, pr, cl, n, a.cap, tid);         // a
    // m, and the control words that the loop reads behind a barrier, are the same in every thread: the conditions below are uniform
    // over the workgroup, so the barriers inside the phases are met by every thread or by none
    const bool run = m >= P::SAMPLE;
    if (run) {
        int head[P::SAMPLE];                                                // lane 0, live across the rounds
#pragma unroll
        for (int i = 0; i < P::SAMPLE; ++i) head[i] = i;
        double best_cost = DBL_MAX;                                         // lane 0, likewise
        const uint32_t *draws = a.draws + (size_t)set * P::SAMPLE * a.max_iters;
        for (;;) {                                                          // rounds of up to CHUNK iterations
            const int it0 = v.ctl[0], limit = v.ctl[1];
            if (it0 >= limit) break;
            const int h = min(P::CHUNK, a.cap - it0);
            sampler<P>(v, draws, it0, h, m, head, tid);                     // b
            double M[P::MODEL];
            const bool have = P::models(v, h, tid, M);                      // c
            cost_and_count<P>(v, have, M, m, a.thr, a.use_mle, tid);        // d
            loop_rule<P>(v, a, it0, limit, h, m, best_cost, tid);           // e
        }
    }
    inliers_and_outputs<P>(v, a, set, ts, n_all, n, m, run, tid);           // f
}

// ---- the host side ----

// the six numbers both parameter structs carry; a null parameter struct becomes all zeros, which check() refuses as invalid
struct ScParams { double thr, fail_prob; int max_iters, min_iters, use_mle; double min_inlier_fraction; };

// the host-side checks, made before the context is looked at
inline int check(const ScParams &p, int max_points, int n_sets, int iters_limit)
{
    if (!(p.fail_prob > 0 && p.fail_prob < 1) || !(p.thr > 0) || p.max_iters < 1 || p.min_iters > p.max_iters ||
        !(p.min_inlier_fraction >= 0 && p.min_inlier_fraction <= 1) || max_points < 1 || n_sets < 0)
        return HV_ERR_INVALID;
    if (max_points > SC_MAX_PTS || p.max_iters > iters_limit || n_sets > 65535) return HV_ERR_UNSUPPORTED;
    return HV_OK;
}

template <int SAMPLE>
void fill_common(ScArgs &a, const ScParams &p, int max_points, const hv_camera_model *cam0, const hv_camera_model *cam1, const double *second_to_first)
{
    a.max_points = max_points; a.max_iters = p.max_iters; a.min_iters = p.min_iters;
    a.use_mle = p.use_mle ? 1 : 0;
    a.thr = p.thr; a.logp = std::log(p.fail_prob);
    a.cap = std::min(a.max_iters, max_iterations_for<SAMPLE>(p.min_inlier_fraction, a.logp, a.min_iters, a.max_iters));
    for (int i = 0; i < 16; ++i) a.T[i] = second_to_first[i];
    a.cam0 = *cam0; a.cam1 = *cam1;
}

template <class Kernel, class Args> int launch(Ctx *c, Kernel kernel, int threads, size_t lds, int n_sets, const Args &a)
{
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_sets), dim3(threads), lds, c->stream, a);
    HV_HIP(c, hipGetLastError());
    return HV_OK;
}

// one staged set, as the device pointers a batched entry takes (extra: the filter's own section, upright 2-point's poses)
struct StagedSet { int max_points; int *n, *status, *summary; float *pl, *pr, *cl; uint32_t *draws; double *model, *extra; };

// The synchronous host-pointer entry on one set of n features: checks, the set staged in the context's arena, `batch` (the file's
// batched entry on one StagedSet), results copied back. others_ok: the pointers the entry only hands on (cameras, secondToFirstCamera)
// are there; extra [n_extra]: the filter's own input section, required when n_extra > 0.
template <int SAMPLE, class Batch>
int staged_entry(hv_ctx *h, const ScParams &p, int iters_limit, int n, const float *prev_left_xy, const float *prev_right_xy,
                 const float *cur_left_xy, bool others_ok, const double *extra, size_t n_extra, const uint32_t *draws, int *status,
                 double *model, int *summary, Batch batch)
{
    if (n < 0) return HV_ERR_INVALID;
    if (const int rc = check(p, std::max(n, 1), 1, iters_limit)) return rc;
    Ctx *c = ctx_of(h);
    if (!c || (n > 0 && (!prev_left_xy || !prev_right_xy || !cur_left_xy || !status)) || !others_ok || (n_extra && !extra) || !draws)
        return HV_ERR_INVALID;
    const int mp = std::max(n, 1);
    const size_t nd = SAMPLE * (size_t)p.max_iters;
    const bool any = n > 0;                                       // (n == 0: one-point sections, nothing of the caller's arrays read or written)
    Stage s(c);
    const auto o_pl = s.in(any ? prev_left_xy : nullptr, 2 * (size_t)mp), o_pr = s.in(any ? prev_right_xy : nullptr, 2 * (size_t)mp);
    const auto o_cl = s.in(any ? cur_left_xy : nullptr, 2 * (size_t)mp);
    const auto o_n = s.in(&n, 1);
    const auto o_st = s.inout(any ? status : nullptr, mp);
    const auto o_sum = s.out(summary, 4);
    const auto o_dr = s.in(draws, nd);
    const auto o_model = s.out(model, 12);
    const auto o_extra = s.in(extra, n_extra);
    int rc = s.upload();
    if (rc != HV_OK) return rc;
    rc = batch(StagedSet{mp, s.at(o_n), s.at(o_st), s.at(o_sum), s.at(o_pl), s.at(o_pr), s.at(o_cl), s.at(o_dr), s.at(o_model), s.at(o_extra)});
    return rc != HV_OK ? rc : s.download();
}
