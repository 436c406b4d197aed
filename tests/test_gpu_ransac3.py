"""GPU tests of the stereo RANSAC3 filter (hv_ransac3*) against the numpy restatement tests/ransac3_restatement.py.

Corpus: 464 synthetic stereo sets (a rig of two equal cameras 0.11 apart, points 1.5-8 deep, a small motion between the
frames) on a pinhole, a radially distorted pinhole and a fisheye camera; n in {0, 2, 3, 4, 5, 20, 64, 65, 200, 257, 400}
and 1024, 0-75 % outliers (20-60 px off), 0-0.5 px noise; sets of 20 or more features carry non-TRACKED entries, features
whose triangulation is rejected and (fisheye) features outside the valid field of view, interleaved with the others.

Figures of the restatement alone on this corpus (CPU, before any GPU run) are in profiles/ransac3/README.md.
"""
import numpy as np
import pytest

import ransac3_restatement as R
import ransac5_restatement as R5
from hybvio_amd import capi

pytestmark = pytest.mark.gpu
NS = [0, 2, 3, 4, 5, 20, 64, 65, 200, 257, 400]
CELLS = [(0.0, 0.0), (0.2, 0.0), (0.4, 0.0), (0.6, 0.0), (0.75, 0.0), (0.0, 0.25), (0.2, 0.25), (0.4, 0.25), (0.6, 0.25),
         (0.0, 0.5), (0.2, 0.5), (0.4, 0.5), (0.6, 0.5), (0.75, 0.5)]                    # (outliers, noise px)
T = R.SECOND_TO_FIRST


def _cams(oracle, name):
    spec = R5.CAMERAS[name]
    o = oracle.Camera(spec[0], *spec[1:5], coeffs=spec[5], max_valid_fov_deg=spec[6])
    g = capi.camera_model(spec[0], *spec[1:5], coeffs=spec[5], max_valid_fov_deg=spec[6])
    return o, g


def _pack(sets, max_points, max_iters=R.MAX_ITERS):
    S = len(sets)
    xy = np.zeros((3, S, max_points, 2), np.float32)
    st = np.full((S, max_points), -9, np.int32)
    cnt = np.zeros(S, np.int32)
    for s, d in enumerate(sets):
        n = len(d["status"])
        xy[0, s, :n], xy[1, s, :n], xy[2, s, :n], st[s, :n], cnt[s] = d["prev_left"], d["prev_right"], d["cur_left"], d["status"], n
    draws = np.stack([d["draws"][:3 * max_iters] for d in sets])           # [sets][3 * ransac3MaxIterations]
    return xy, st, cnt, draws


def _run_batch(ctx, sets, gcam, max_points=400, params=None):
    import torch
    xy, st, cnt, draws = _pack(sets, max_points, params.ransac3MaxIterations if params is not None else R.MAX_ITERS)
    S = len(sets)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_xy, d_st, d_n, d_dr = dev(xy), dev(st), dev(cnt), dev(draws)
    d_pose = torch.full((S, 12), 7.0, dtype=torch.float64, device="cuda")
    d_sm = torch.full((S, 4), -5, dtype=torch.int32, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.ransac3_batch_dev(S, max_points, d_n.data_ptr(), d_xy[0].data_ptr(), d_xy[1].data_ptr(), d_xy[2].data_ptr(), gcam, gcam, T,
                          d_dr.data_ptr(), d_st.data_ptr(), d_pose.data_ptr(), d_sm.data_ptr(), params=params)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_pose.cpu().numpy(), d_sm.cpu().numpy()


def _reference(d, ocam, params=None):
    ts, done, cnt, pose, summ = R.do_ransac3(d["status"], d["prev_left"], d["prev_right"], d["cur_left"], ocam, ocam, T, d["draws"], params)
    return ts, pose, summ


def _make(rng, oracle, ocam, name, n, outl, noise, seed):
    extra = (3, 2, 2 if name == "fisheye" else 0) if 20 <= n < 400 else (0, 0, 0)
    d = R.make_set(rng, ocam, n - sum(extra), outl, noise, *extra)
    d.update(cam=name, n=n, outl=outl, noise=noise, draws=oracle.mt19937_draws(seed, 3 * R.MAX_ITERS))
    return d


@pytest.fixture(scope="module")
def corpus(oracle):
    rng = np.random.default_rng(2026)
    out = []
    with capi.Context(width=752, height=480) as ctx:
        for name in R5.CAMERAS:
            ocam, gcam = _cams(oracle, name)
            sets = [_make(rng, oracle, ocam, name, n, outl, noise, 1000 + len(out) + i * 11 + k)
                    for i, (outl, noise) in enumerate(CELLS) for k, n in enumerate(NS)]
            st, pose, sm = _run_batch(ctx, sets, gcam)
            for s, d in enumerate(sets):
                d.update(gpu=(st[s, :d["n"]], pose[s], sm[s].tolist()), ref=_reference(d, ocam))
                assert (st[s, d["n"]:] == -9).all()                                  # padding untouched
            out += sets
        ocam, gcam = _cams(oracle, "pinhole_radial")
        big = [_make(rng, oracle, ocam, "pinhole_radial", 1024, outl, 0.25, 77 + i) for i, outl in enumerate((0.2, 0.6))]
        st, pose, sm = _run_batch(ctx, big, gcam, 1024)
        for s, d in enumerate(big):
            d.update(gpu=(st[s], pose[s], sm[s].tolist()), ref=_reference(d, ocam))
        out += big
    return out


def _same(d):
    (sg, pg, mg), (sr, pr, mr) = d["gpu"], d["ref"]
    return np.array_equal(sg, sr) and mg == list(mr)


def _well_separated(d):
    return d["n"] >= 20 and d["noise"] <= 0.5 and d["outl"] <= 0.4


def test_corpus_against_the_restatement(corpus):
    assert 400 <= len(corpus) <= 480
    bad = [(i, d["cam"], d["n"], d["outl"], d["noise"], d["gpu"][2], list(d["ref"][2])) for i, d in enumerate(corpus) if not _same(d)]
    for b in bad:
        print("mismatch", b)
    print("sets", len(corpus), "differing", len(bad))
    assert len(bad) <= 0.01 * len(corpus), bad
    for i, *_ in bad:
        d = corpus[i]
        dn = abs(int((d["gpu"][0] == 0).sum()) - int((d["ref"][0] == 0).sum()))
        assert dn <= max(1, 0.01 * d["n"]), (i, dn)
    # the corpus reaches every branch: not run, ended at minIterations, ended adaptively in between, ended at the cap
    sm = np.array([d["ref"][2] for d in corpus])
    assert (sm[:, 3] < 3).any() and (sm[:, 2] == 50).any() and ((sm[:, 2] > 50) & (sm[:, 2] < 337)).any() and (sm[:, 2] == 337).any()
    assert (sm[:, 2] <= 337).all() and ((sm[:, 3] < 3) == (sm[:, 2] == 0)).all()
    # the compaction is exercised: sets where correspondences < TRACKED < features
    assert any(d["ref"][2][3] < int((d["status"] == 0).sum()) < d["n"] for d in corpus)


def _truth_recoverable(d):
    """Noise-free sets of 20 and more features whose mask must equal the ground truth exactly: every outlier level up to
    60 %, and 75 % from 64 features on. A 20-feature set carries 13 good features (the other 7 are the interleaved special
    entries), so at 75 % outliers it has 3 true inliers: a P3P model reproduces its own three sample points, every triple
    then has at least as many inliers as the true pose and the truth cannot be told from the data."""
    return d["noise"] == 0 and d["n"] >= 20 and (d["outl"] <= 0.6 or d["n"] >= 64)


def test_well_separated_sets_are_exact_and_near_the_truth(corpus):
    """Well-separated sets (n >= 20, noise <= 0.5 px, <= 40 % outliers): on the pinhole cameras the result is identical to
    the restatement and the pose matches to 1e-9; the noisy ones agree with the ground truth on >= 98 % of the points.
    Noise-free sets (every camera, every outlier level: _truth_recoverable) recover the ground truth exactly."""
    ws = [d for d in corpus if _well_separated(d)]
    assert len(ws) >= 150 and {d["cam"] for d in ws} == set(R5.CAMERAS)
    agree = total = 0
    for d in ws:
        (sg, pg, mg), (sr, pr, mr) = d["gpu"], d["ref"]
        if d["cam"] != "fisheye":
            assert np.array_equal(sg, sr) and mg == list(mr), (d["cam"], d["n"], d["outl"], d["noise"], mg, mr)
            assert np.abs(pg - pr).max() <= 1e-9
        if d["noise"] > 0:
            agree += int(((sg == 0) == d["truth"]).sum())
            total += d["n"]
    nf = [d for d in corpus if _truth_recoverable(d)]
    assert len(nf) >= 85 and {d["outl"] for d in nf} == {0.0, 0.2, 0.4, 0.6, 0.75}
    for d in nf:
        assert np.array_equal(d["gpu"][0] == 0, d["truth"]), (d["cam"], d["n"], d["outl"])
    print("noise-free sets", len(nf), "noisy agreement", agree, total, agree / total)
    assert agree >= 0.98 * total, (agree, total)


def test_more_sets_than_compute_units(oracle):
    ocam, gcam = _cams(oracle, "pinhole")
    rng = np.random.default_rng(9)
    sets = [_make(rng, oracle, ocam, "pinhole", 20, [0.0, 0.2, 0.4][i % 3], [0.0, 0.25][i % 2], 5000 + i) for i in range(600)]
    with capi.Context(width=752, height=480) as ctx:
        st, pose, sm = _run_batch(ctx, sets, gcam, 32)
    bad = 0
    for s, d in enumerate(sets):
        ts, pr, mr = _reference(d, ocam)
        if not (np.array_equal(st[s, :20], ts) and sm[s].tolist() == list(mr)):
            bad += 1
            print("mismatch", s, sm[s].tolist(), list(mr))
            assert abs(int((st[s, :20] == 0).sum()) - int((ts == 0).sum())) <= 1, s      # max(1, 1 % of n)
        assert (st[s, 20:] == -9).all()
    assert bad <= 6, bad


def test_synchronous_batched_and_graph_replayed_forms_agree(oracle):
    import torch
    ocam, gcam = _cams(oracle, "pinhole_radial")
    rng = np.random.default_rng(5)
    sets = [_make(rng, oracle, ocam, "pinhole_radial", n, 0.3, 0.5, 300 + n) for n in (2, 3, 5, 20, 65, 200, 400, 64)]
    S, MP = len(sets), 400
    with capi.Context(width=752, height=480) as ctx:
        sync = [ctx.ransac3(d["status"], d["prev_left"], d["prev_right"], d["cur_left"], gcam, gcam, T, d["draws"]) for d in sets]
        st, pose, sm = _run_batch(ctx, sets, gcam, MP)
        for s, d in enumerate(sets):
            n = d["n"]
            assert np.array_equal(st[s, :n], sync[s][0]) and np.array_equal(pose[s], sync[s][1]) and sm[s].tolist() == sync[s][2].tolist()
        xy, st0, cnt, draws = _pack(sets, MP)
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        d_xy, d_st0, d_n, d_dr = (torch.from_numpy(x).cuda() for x in (xy, st0, cnt, draws))
        d_st = torch.zeros((S, MP), dtype=torch.int32, device="cuda")
        d_pose = torch.zeros((S, 12), dtype=torch.float64, device="cuda"); d_sm = torch.zeros((S, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            ctx.ransac3_batch_dev(S, MP, d_n.data_ptr(), d_xy[0].data_ptr(), d_xy[1].data_ptr(), d_xy[2].data_ptr(), gcam, gcam, T,
                                  d_dr.data_ptr(), d_st.data_ptr(), d_pose.data_ptr(), d_sm.data_ptr())
        for _ in range(2):
            with torch.cuda.stream(stream):
                d_st.copy_(d_st0); d_pose.fill_(0); d_sm.fill_(0)
                g.replay()
            stream.synchronize()
            assert np.array_equal(d_st.cpu().numpy(), st) and np.array_equal(d_pose.cpu().numpy(), pose)
            assert np.array_equal(d_sm.cpu().numpy(), sm)
        del g


def test_use_mle_off_and_other_parameters_follow_the_restatement(oracle):
    ocam, gcam = _cams(oracle, "pinhole")
    rng = np.random.default_rng(21)
    sets = [_make(rng, oracle, ocam, "pinhole", n, 0.3, 0.25, 900 + n) for n in (20, 65, 200)]
    with capi.Context(width=752, height=480) as ctx:
        for kw in (dict(ransac3UseMle=0), dict(ransac3MinIterations=10, ransac3MaxIterations=100),
                   dict(ransac3MinIterations=100, ransac3MaxIterations=200),                               # more than one 64-iteration round
                   dict(ransac3ErrorThresh=2.5e-5)):
            st, pose, sm = _run_batch(ctx, sets, gcam, params=capi.ransac3_default_params(**kw))
            for s, d in enumerate(sets):
                ts, pr, mr = _reference(d, ocam, R.Params(**kw))
                if kw.get("ransac3MinIterations") == 100:
                    assert mr[3] < 3 or mr[2] > 64, (d["n"], mr)               # (by the restatement: the case spans rounds)
                assert np.array_equal(st[s, :d["n"]], ts) and sm[s].tolist() == list(mr), (kw, d["n"], sm[s], mr)
                assert np.abs(pose[s] - pr).max() <= 1e-9


def test_stereo_chain_lk_gate_rotation_ransac_and_ransac3(oracle):
    """hv_klt_track_batch_dev (previous stereo pair, temporal, current stereo pair) -> flow status -> gate ->
    hv_rot_ransac_lk_batch_dev -> hv_ransac3_lk_batch_dev, nothing through the host; statuses, type, inlier count and score
    must equal the restatement's RansacPipeline::compute on the same device outputs."""
    import torch
    from hybvio_amd import synth
    w, h, npts, S = 376, 240, 150, 4
    cam_args, radial = ("pinhole", 229.3, 228.6, 183.6, 124.2), [-0.28, 0.07, 0.0]
    ocam, gcam = oracle.Camera(*cam_args, coeffs=radial), capi.camera_model(*cam_args, coeffs=radial)
    thr = float(np.float32((4.0 * min(w, h) / 720.0) ** 2))
    T01 = np.eye(4); T01[0, 3] = -0.1                                   # cam0ToCam1 of the gate
    T10 = np.eye(4); T10[0, 3] = 0.1                                    # secondToFirstCamera of the triangulation
    gp = capi.stereo_gate_default_params(cam0ToCam1=T01)
    seqs = [synth.stereo_sequence(60 + s, w, h, 2) for s in range(S)]
    pts = np.stack([synth.grid_points(w, h, npts, margin=12, seed=s) for s in range(S)]).astype(np.float32)
    draws2 = np.stack([oracle.mt19937_draws(4649 + s, 200) for s in range(S)])
    draws3 = np.stack([oracle.mt19937_draws(4649 + s, 3 * R.MAX_ITERS) for s in range(S)])
    rng = np.random.default_rng(3)
    with capi.Context(width=w, height=h, pool_size=4 * S, max_tracks=npts) as ctx:
        slots = [[ctx.acquire() for _ in range(S)] for _ in range(4)]   # previous left / right, current left / right
        for s in range(S):
            for k, img in enumerate((seqs[s][0][0], seqs[s][1][0], seqs[s][0][1], seqs[s][1][1])):
                ctx.build(slots[k][s], img)
        dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()
        d_pl, d_pr, d_cl, d_cr = (dev(x, np.int32) for x in slots)
        d_pts, d_n = dev(pts, np.float32), dev(np.full(S, npts, np.int32), np.int32)
        new = lambda dt: torch.zeros((S, npts), dtype=dt, device="cuda")
        d_second, d_next, d_right = torch.zeros_like(d_pts), torch.zeros_like(d_pts), torch.zeros_like(d_pts)
        d_lk0, d_lk, d_lk2, d_mask, d_bl = (new(torch.uint8) for _ in range(5))
        d_ts, d_ss = new(torch.int32), new(torch.int32)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        klt = lambda a, b, src, dst, lk: ctx.klt_track_batch_dev(S, a.data_ptr(), b.data_ptr(), npts, src.data_ptr(), dst.data_ptr(),
                                                                 lk.data_ptr(), 0, use_initial_flow=False)
        klt(d_pl, d_pr, d_pts, d_second, d_lk0)                          # the previous frame's stereo corners (table.second_xy)
        klt(d_pl, d_cl, d_pts, d_next, d_lk)
        ctx.flow_status_batch_dev(S, npts, d_n.data_ptr(), d_next.data_ptr(), d_lk.data_ptr(), d_ts.data_ptr())
        klt(d_cl, d_cr, d_next, d_right, d_lk2)
        ctx.flow_status_batch_dev(S, npts, d_n.data_ptr(), d_right.data_ptr(), d_lk2.data_ptr(), d_ss.data_ptr())
        ctx.track_gate_batch_dev(S, npts, d_n.data_ptr(), d_next.data_ptr(), d_right.data_ptr(), d_ss.data_ptr(), d_bl.data_ptr(), gcam,
                                 gcam, d_ts.data_ptr(), d_mask.data_ptr(), params=gp)
        # set 1: a quarter of the current corners moved 12-30 px; set 2: two tracked features; set 3: none
        idx = torch.from_numpy(rng.choice(npts, npts // 4, replace=False)).cuda()
        d_next[1, idx] += torch.from_numpy(rng.uniform(12, 30, (npts // 4, 2)).astype(np.float32) * rng.choice([-1, 1], (npts // 4, 2))).cuda()
        two = torch.nonzero(d_ts[2] == 0)[:2, 0]
        keep = torch.zeros(npts, dtype=torch.bool, device="cuda"); keep[two] = True
        d_ts[2] = torch.where(keep, d_ts[2], torch.full_like(d_ts[2], 2)); d_mask[2] = keep.to(torch.uint8)
        d_ts[3] = 2; d_mask[3] = 0
        ts_in = d_ts.cpu().numpy()
        d_r2 = torch.full((S, npts), -7, dtype=torch.int32, device="cuda")
        d_R = torch.zeros((S, 9), dtype=torch.float32, device="cuda"); d_r2s = torch.zeros((S, 2), dtype=torch.int32, device="cuda")
        ctx.profile_enable(True)
        ctx.profile_reset()
        ctx.rot_ransac_lk_batch_dev(S, npts, d_n.data_ptr(), d_pts.data_ptr(), d_next.data_ptr(), d_mask.data_ptr(), 1, gcam, gcam,
                                    dev(draws2, np.uint32).data_ptr(), thr, d_r2.data_ptr(), d_R.data_ptr(), d_r2s.data_ptr())
        d_res = torch.full((S, 2), -1, dtype=torch.int32, device="cuda"); d_score = torch.full((S,), -1.0, dtype=torch.float64, device="cuda")
        d_sm = torch.zeros((S, 4), dtype=torch.int32, device="cuda")
        ctx.ransac3_lk_batch_dev(S, npts, d_n.data_ptr(), d_pts.data_ptr(), d_second.data_ptr(), d_next.data_ptr(), d_ts.data_ptr(),
                                 d_r2s.data_ptr(), gcam, gcam, T10, dev(draws3, np.uint32).data_ptr(), d_res.data_ptr(),
                                 d_score.data_ptr(), 0, d_sm.data_ptr())
        torch.cuda.synchronize()
        assert ctx.profile_read(capi.K_RANSAC3)[1] == 1 and ctx.profile_read(capi.K_RANSAC5)[1] == 0
        host = lambda t: t.cpu().numpy()
        ts, res, score, sm, nxt, sec, r2s = host(d_ts), host(d_res), host(d_score), host(d_sm), host(d_next), host(d_second), host(d_r2s)
    for s in range(S):
        want_ts, typ, cnt, sc, summ = R.compute(ts_in[s], pts[s], sec[s], nxt[s], ocam, ocam, T10, draws3[s], int(r2s[s, 0]))
        print("set", s, "type", typ, "inliers", cnt, "score", sc, "summary", summ, "gpu", res[s], sm[s])
        assert np.array_equal(ts[s], want_ts), s
        assert res[s].tolist() == [typ, cnt] and score[s] == sc and sm[s].tolist() == list(summ), (s, res[s], typ, cnt, score[s], sc)
    assert res[:, 0].tolist() == [R.TYPE_R3, R.TYPE_R3, R.TYPE_SKIPPED, R.TYPE_SKIPPED]
    assert int((ts_in[2] == 0).sum()) == 2 and (ts[2] == 3).all() and (ts[3] == 3).all() and score[3] == 0.0
    for s in (0, 1):                                                    # entries that were not TRACKED keep their status
        assert np.array_equal(ts[s][ts_in[s] != 0], ts_in[s][ts_in[s] != 0]) and 3 <= res[s, 1] == int((ts[s] == 0).sum())


def test_profile_class_counts_the_launches(oracle):
    ocam, gcam = _cams(oracle, "pinhole")
    d = _make(np.random.default_rng(1), oracle, ocam, "pinhole", 50, 0.2, 0.25, 3)
    with capi.Context(width=752, height=480) as ctx:
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(3):
            ctx.ransac3(d["status"], d["prev_left"], d["prev_right"], d["cur_left"], gcam, gcam, T, d["draws"])
        ms, n = ctx.profile_read(capi.K_RANSAC3)
        assert n == 3 and ms > 0
        assert ctx.profile_read(capi.K_RANSAC5)[1] == 0 and ctx.profile_read(capi.K_ROT_RANSAC)[1] == 0


EDGE_COUNTS = [0, 1, 4, 5, 6, 63, 64, 65, 128, 129, 769, 1023, 1024]


def test_compaction_and_gather_at_the_chunk_edges(oracle):
    """The ordered compaction (TRACKED features, then correspondences) and the gather behind it at their edges: one launch of
    hv_ransac3_lk_batch_dev with max_points = 1024, point counts around the 64-feature chunks and the 256-thread strides, and
    per count three masks: all TRACKED, every second feature, feature 0 and the last feature of every 64-feature chunk.
    Noise-free sets with 20 % outliers; counts from 63 up carry features whose triangulation is rejected, so the gather moves
    the correspondences behind them. Every set must equal the restatement's compute, none exempted."""
    import torch
    ocam, gcam = _cams(oracle, "pinhole_radial")
    rng = np.random.default_rng(78)
    MP = 1024
    sets = []
    for k, n in enumerate(EDGE_COUNTS):
        extra = 6 if n >= 63 else 0
        base = R.make_set(rng, ocam, n - extra, 0.2, 0.0, 0, extra, 0)
        i = np.arange(n)
        for j, mask in enumerate([np.ones(n, bool), i % 2 == 0, (i % 64 == 63) | (i == 0)]):
            d = dict(base, n=n, status=np.where(mask, 0, 2).astype(np.int32), draws=oracle.mt19937_draws(7000 + 3 * k + j, 3 * R.MAX_ITERS))
            d["r2count"] = int(mask.sum()) // 2
            sets.append(d)
    S = len(sets)
    xy, st, cnt, draws = _pack(sets, MP)
    r2s = np.zeros((S, 2), np.int32); r2s[:, 0] = [d["r2count"] for d in sets]
    with capi.Context(width=752, height=480) as ctx:
        d_xy, d_st, d_n, d_dr, d_r2s = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (xy, st, cnt, draws, r2s))
        d_res = torch.full((S, 2), -1, dtype=torch.int32, device="cuda"); d_score = torch.full((S,), -1.0, dtype=torch.float64, device="cuda")
        d_pose = torch.full((S, 12), 7.0, dtype=torch.float64, device="cuda"); d_sm = torch.full((S, 4), -5, dtype=torch.int32, device="cuda")
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.ransac3_lk_batch_dev(S, MP, d_n.data_ptr(), d_xy[0].data_ptr(), d_xy[1].data_ptr(), d_xy[2].data_ptr(), d_st.data_ptr(),
                                 d_r2s.data_ptr(), gcam, gcam, T, d_dr.data_ptr(), d_res.data_ptr(), d_score.data_ptr(), d_pose.data_ptr(),
                                 d_sm.data_ptr())
        torch.cuda.synchronize()
        g_st, g_res, g_score, g_pose, g_sm = (t.cpu().numpy() for t in (d_st, d_res, d_score, d_pose, d_sm))
    types, moved = [], 0
    for s, d in enumerate(sets):
        n = d["n"]
        want_ts, typ, count, score, summ = R.compute(d["status"], d["prev_left"], d["prev_right"], d["cur_left"], ocam, ocam, T, d["draws"], d["r2count"])
        pose = R.do_ransac3(d["status"], d["prev_left"], d["prev_right"], d["cur_left"], ocam, ocam, T, d["draws"])[3]
        print("set", s, "n", n, "tracked", int((d["status"] == 0).sum()), "type", typ, "count", count, "summary", list(summ), "gpu", g_res[s], g_sm[s])
        assert np.array_equal(g_st[s, :n], want_ts) and (g_st[s, n:] == -9).all(), (s, n)
        assert g_res[s].tolist() == [typ, count] and g_score[s] == score and g_sm[s].tolist() == list(summ), (s, n, g_res[s], g_sm[s], typ, count, summ)
        assert np.abs(g_pose[s] - pose).max() <= 1e-9, (s, n)
        types.append(typ)
        moved += 3 <= summ[3] < int((d["status"] == 0).sum())
    assert {R.TYPE_R3, R.TYPE_SKIPPED} <= set(types), types                     # (by the restatement: both outcomes are reached,
    assert moved >= 10                                                         # and sets where correspondences < TRACKED features)
