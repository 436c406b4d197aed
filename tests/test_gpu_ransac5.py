"""GPU tests of the five-point RANSAC (hv_ransac5*) and the hybrid RANSAC2 / RANSAC5 filter (hv_hybrid_ransac_lk_batch_dev)
against the numpy restatement tests/ransac5_restatement.py.

Corpus: 2016 synthetic two-view sets from 3-D points and known R, t on a pinhole, a radially distorted pinhole and a
fisheye camera; n in {5, 6, 7, 20, 200, 400}, 0-60 % outliers (>= 20 px off their epipolar line), 0-1 px noise, general,
planar and near pure-rotation scenes."""
import numpy as np
import pytest

import ransac5_restatement as R
from hybvio_amd import capi

pytestmark = pytest.mark.gpu
NS = [5, 6, 7, 20, 200, 400]
OUTLIERS = [0.0, 0.1, 0.2, 0.3, 0.45, 0.6]
NOISE = [0.0, 0.25, 0.5, 1.0]
N_SETS = 2016


def _cams(oracle, name):
    spec = R.CAMERAS[name]
    o = oracle.Camera(spec[0], *spec[1:5], coeffs=spec[5], max_valid_fov_deg=spec[6])
    g = capi.camera_model(spec[0], *spec[1:5], coeffs=spec[5], max_valid_fov_deg=spec[6])
    return o, g, (spec[1] + spec[2]) * 0.5, spec


def _run_batch(ctx, sets, gcam, max_points=400):
    import torch
    S = len(sets)
    c1 = np.zeros((S, max_points, 2), np.float32)
    c2 = np.zeros((S, max_points, 2), np.float32)
    cnt = np.zeros(S, np.int32)
    for s, st in enumerate(sets):
        n = len(st["c1"])
        c1[s, :n], c2[s, :n], cnt[s] = st["c1"], st["c2"], n
    dev = lambda x: torch.from_numpy(x).cuda()
    d_c1, d_c2, d_n = dev(c1), dev(c2), dev(cnt)
    d_st = torch.full((S, max_points), -9, dtype=torch.int32, device="cuda")
    d_E = torch.zeros((S, 9), dtype=torch.float64, device="cuda")
    d_sm = torch.zeros((S, 4), dtype=torch.int32, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.ransac5_batch_dev(S, max_points, d_n.data_ptr(), d_c1.data_ptr(), d_c2.data_ptr(), gcam, gcam, d_st.data_ptr(),
                          d_E.data_ptr(), d_sm.data_ptr())
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_E.cpu().numpy(), d_sm.cpu().numpy()


@pytest.fixture(scope="module")
def corpus(oracle):
    rng = np.random.default_rng(2024)
    out = []
    with capi.Context(width=752, height=480) as ctx:
        for ci, name in enumerate(R.CAMERAS):
            ocam, gcam, f, spec = _cams(oracle, name)
            sets = []
            for i in range(N_SETS // 3):
                n = NS[i % 6]
                outl = OUTLIERS[(i // 6) % 6]
                noise = NOISE[(i // 36) % 4]
                scene = ["general", "general", "general", "planar", "rotation"][(i // 144) % 5]
                c1, c2, truth, E = R.make_set(rng, (ocam, spec), n, outl, noise, scene)
                sets.append(dict(cam=name, n=n, outl=outl, noise=noise, scene=scene, c1=c1, c2=c2, truth=truth, E_true=E))
            st, E, sm = _run_batch(ctx, sets, gcam)
            norm = [R.normalize(s["c1"], s["c2"], ocam, ocam) for s in sets]
            runs = R.registrator_runs([(h1, h2, R.threshold(f, f)) for h1, h2, _ in norm])
            for s, d in enumerate(sets):
                done, st_r, E_r, sm_r, _ = R.do_ransac5(d["c1"], d["c2"], ocam, ocam, f, f, run=runs[s])
                d.update(gpu=(st[s, :d["n"]], E[s], sm[s].tolist()), ref=(st_r, E_r, sm_r))
                assert (st[s, d["n"]:] == -9).all()                                  # padding untouched
            out += sets
    return out


def _same(d):
    (sg, Eg, mg), (sr, Er, mr) = d["gpu"], d["ref"]
    return np.array_equal(sg, sr) and mg == mr


def test_corpus_against_the_restatement(corpus):
    assert len(corpus) >= 2000
    bad = [(i, d["cam"], d["n"], d["outl"], d["noise"], d["scene"], d["gpu"][2], d["ref"][2]) for i, d in enumerate(corpus) if not _same(d)]
    for b in bad:
        print("mismatch", b)
    assert len(bad) <= 0.01 * len(corpus), bad
    for i, *_ in bad:
        d = corpus[i]
        dn = abs(int((d["gpu"][0] == 0).sum()) - int((d["ref"][0] == 0).sum()))
        assert dn <= max(1, 0.01 * d["n"]), (i, dn)
    # the corpus reaches every branch of the registrator
    sm = np.array([d["ref"][2] for d in corpus])
    assert (sm[:, 3] == 5).any() and (sm[:, 1] == -1).any() and ((sm[:, 1] >= 0) & (sm[:, 2] < 75)).any() and (sm[:, 2] == 75).any()


def _well_separated(d):
    return d["n"] >= 20 and d["noise"] <= 0.5 and d["outl"] <= 0.3 and d["scene"] == "general"


def test_well_separated_sets_are_exact_and_near_the_truth(corpus):
    """Every well-separated set (all three cameras) is identical to the restatement (statuses, summary, E to 1e-7).
    Noise-free sets: the mask equals the ground truth on every set. E is the minimal solution of the winning 5-point sample
    (the reference does not refit) computed from binary32 pixels, so it meets the truth to ~1e-6 for a well spread sample and
    worse for a poorly spread one that still classifies every point correctly: >= 75 % of the sets within 1e-5, all within
    0.05. Noisy sets: the loop stops as soon as RANSACUpdateNumIters is satisfied at 0.999 (e.g. after 5 iterations with 376
    of 400 inliers), so the mask must agree with the truth on >= 98 % of their points."""
    ws = [d for d in corpus if _well_separated(d)]
    assert len(ws) >= 300 and {d["cam"] for d in ws} == set(R.CAMERAS)
    truth_err, agree, total = [], 0, 0
    for d in ws:
        (sg, Eg, mg), (sr, Er, mr) = d["gpu"], d["ref"]
        assert np.array_equal(sg, sr) and mg == mr, (d["cam"], d["n"], d["outl"], d["noise"], mg, mr)
        assert _e_dist(Eg, Er) <= 1e-7
        if d["noise"] == 0:
            assert np.array_equal(sg == 0, d["truth"]), (d["cam"], d["n"], d["outl"])
            truth_err.append(_e_dist(Eg, d["E_true"]))
        else:
            agree += int(((sg == 0) == d["truth"]).sum())
            total += d["n"]
    truth_err = np.array(truth_err)
    assert len(truth_err) >= 100 and (truth_err <= 1e-5).mean() >= 0.75 and truth_err.max() <= 0.05, np.sort(truth_err)
    assert agree >= 0.98 * total, (agree, total)


def _e_dist(a, b):
    a, b = np.asarray(a) / np.linalg.norm(a), np.asarray(b) / np.linalg.norm(b)
    return min(np.abs(a - b).max(), np.abs(a + b).max())


def test_synchronous_batched_and_graph_replayed_forms_agree(oracle):
    import torch
    ocam, gcam, f, spec = _cams(oracle, "pinhole_radial")
    rng = np.random.default_rng(5)
    sets = [dict(zip(("c1", "c2", "truth", "E"), R.make_set(rng, (ocam, spec), n, 0.3, 0.5))) for n in [5, 6, 7, 20, 80, 200, 400, 3] * 4]
    S, MP = len(sets), 400
    with capi.Context(width=752, height=480) as ctx:
        sync = [ctx.ransac5(d["c1"], d["c2"], gcam, gcam) for d in sets]
        st, E, sm = _run_batch(ctx, sets, gcam, MP)
        for s, d in enumerate(sets):
            n = len(d["c1"])
            assert np.array_equal(st[s, :n], sync[s][0]) and np.array_equal(E[s], sync[s][1]) and sm[s].tolist() == sync[s][2].tolist()
        c1 = np.zeros((S, MP, 2), np.float32); c2 = c1.copy(); cnt = np.array([len(d["c1"]) for d in sets], np.int32)
        for s, d in enumerate(sets):
            c1[s, :cnt[s]], c2[s, :cnt[s]] = d["c1"], d["c2"]
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        d_c1, d_c2, d_n = (torch.from_numpy(x).cuda() for x in (c1, c2, cnt))
        d_st = torch.zeros((S, MP), dtype=torch.int32, device="cuda")
        d_E = torch.zeros((S, 9), dtype=torch.float64, device="cuda"); d_sm = torch.zeros((S, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            ctx.ransac5_batch_dev(S, MP, d_n.data_ptr(), d_c1.data_ptr(), d_c2.data_ptr(), gcam, gcam, d_st.data_ptr(),
                                  d_E.data_ptr(), d_sm.data_ptr())
        for _ in range(2):
            with torch.cuda.stream(stream):
                d_st.fill_(-9); d_E.fill_(0); d_sm.fill_(0)
                g.replay()
            stream.synchronize()
            gst, gE, gsm = d_st.cpu().numpy(), d_E.cpu().numpy(), d_sm.cpu().numpy()
            for s in range(S):
                assert np.array_equal(gst[s, :cnt[s]], st[s, :cnt[s]])
            assert np.array_equal(gE, E) and np.array_equal(gsm, sm)
        del g


def test_hybrid_entry_on_the_device_lk_and_rotation_ransac_chain(oracle):
    """hv_klt_track_batch_dev -> hv_rot_ransac_lk_batch_dev -> hv_hybrid_ransac_lk_batch_dev, nothing through the host; the
    statuses, type, inlier count and score must equal the restatement's RansacPipeline::compute on the same device outputs."""
    import torch
    from hybvio_amd import synth
    w, h, npts, S = 376, 240, 150, 4
    cam_args = ("pinhole", 229.3, 228.6, 183.6, 124.2)
    radial = [-0.28, 0.07, 0.0]
    ocam, gcam = oracle.Camera(*cam_args, coeffs=radial), capi.camera_model(*cam_args, coeffs=radial)
    f = (cam_args[1] + cam_args[2]) * 0.5
    thr = float(np.float32((4.0 * min(w, h) / 720.0) ** 2))
    seqs = [synth.stereo_sequence(60 + s, w, h, 2)[0] for s in range(S)]
    pts = np.stack([synth.grid_points(w, h, npts, margin=12, seed=s) for s in range(S)]).astype(np.float32)
    draws = np.stack([oracle.mt19937_draws(4649 + s, 200) for s in range(S)])
    rng = np.random.default_rng(3)
    with capi.Context(width=w, height=h, pool_size=2 * S, max_tracks=npts) as ctx:
        prev = [ctx.acquire() for _ in range(S)]; cur = [ctx.acquire() for _ in range(S)]
        for s in range(S):
            ctx.build(prev[s], seqs[s][0]); ctx.build(cur[s], seqs[s][1])
        dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()
        d_prev, d_cur, d_pts = dev(prev, np.int32), dev(cur, np.int32), dev(pts, np.float32)
        d_next = torch.zeros_like(d_pts); d_lk = torch.zeros((S, npts), dtype=torch.uint8, device="cuda")
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.klt_track_batch_dev(S, d_prev.data_ptr(), d_cur.data_ptr(), npts, d_pts.data_ptr(), d_next.data_ptr(), d_lk.data_ptr(), 0,
                                use_initial_flow=False)
        # set 1: the current positions of a translating camera (0.4 sideways, points 1.5-6 deep, 10 % of them 12-30 px off):
        # the rotation-only model explains few tracks and RANSAC5 must win. Set 2: a quarter of the LK tracks moved off by
        # 12-30 px (RANSAC2 falls below the skip fraction, RANSAC5 runs). Set 3: a single tracked feature (SKIPPED clears every
        # entry). Set 0: the LK output as it is (RANSAC2 explains nearly everything and skips RANSAC5).
        Rm, t = R.rotation([0.01, -0.02, 0.005]), np.array([0.4, 0.05, 0.1])
        moved = np.zeros((npts, 2), np.float32)
        for i in range(npts):
            _, ray = ocam.pixel_to_ray(*pts[1, i])
            _, pix = ocam.ray_to_pixel(Rm @ (ray / ray[2] * rng.uniform(1.5, 6.0)) + t)
            moved[i] = pix
        off = rng.choice(npts, npts // 10, replace=False)
        moved[off] += rng.uniform(12, 30, (len(off), 2)).astype(np.float32) * rng.choice([-1, 1], (len(off), 2))
        d_next[1] = torch.from_numpy(moved).cuda()
        idx = torch.from_numpy(rng.choice(npts, npts // 4, replace=False)).cuda()
        d_next[2, idx] += torch.from_numpy(rng.uniform(12, 30, (npts // 4, 2)).astype(np.float32) * rng.choice([-1, 1], (npts // 4, 2))).cuda()
        first = int(torch.nonzero(d_lk[3] == 1)[0])
        d_lk[3].zero_(); d_lk[3, first] = 1
        d_ts = torch.where(d_lk == 1, 0, 2).to(torch.int32)
        d_n = dev(np.full(S, npts, np.int32), np.int32)
        d_r2 = torch.full((S, npts), -7, dtype=torch.int32, device="cuda")
        d_R = torch.zeros((S, 9), dtype=torch.float32, device="cuda"); d_r2s = torch.zeros((S, 2), dtype=torch.int32, device="cuda")
        ctx.rot_ransac_lk_batch_dev(S, npts, d_n.data_ptr(), d_pts.data_ptr(), d_next.data_ptr(), d_lk.data_ptr(), 1, gcam, gcam,
                                    dev(draws, np.uint32).data_ptr(), thr, d_r2.data_ptr(), d_R.data_ptr(), d_r2s.data_ptr())
        ts_in = d_ts.cpu().numpy()
        d_res = torch.zeros((S, 2), dtype=torch.int32, device="cuda"); d_score = torch.zeros(S, dtype=torch.float64, device="cuda")
        d_sm = torch.zeros((S, 4), dtype=torch.int32, device="cuda")
        ctx.hybrid_ransac_lk_batch_dev(S, npts, d_n.data_ptr(), d_pts.data_ptr(), d_next.data_ptr(), d_ts.data_ptr(), d_r2.data_ptr(),
                                       d_r2s.data_ptr(), gcam, gcam, d_res.data_ptr(), d_score.data_ptr(), 0, d_sm.data_ptr())
        torch.cuda.synchronize()
        ts, res, score, sm = d_ts.cpu().numpy(), d_res.cpu().numpy(), d_score.cpu().numpy(), d_sm.cpu().numpy()
        nxt, r2, r2s = d_next.cpu().numpy(), d_r2.cpu().numpy(), d_r2s.cpu().numpy()
    types = []
    for s in range(S):
        want_ts, typ, cnt, sc = R.hybrid_pipeline(ts_in[s], pts[s], nxt[s], r2[s], int(r2s[s, 0]), ocam, ocam, f, f)
        assert np.array_equal(ts[s], want_ts), s
        assert res[s].tolist() == [typ, cnt] and score[s] == sc, (s, res[s], typ, cnt, score[s], sc)
        types.append(typ)
    assert types[1] == R.TYPE_R5 and types[3] == R.TYPE_SKIPPED and (ts[3] == 3).all()
    assert {R.TYPE_SKIPPED, R.TYPE_R2, R.TYPE_R5} <= set(types), types
    assert (sm[1:3, 3] > 0).all()                                                          # RANSAC5 ran where R2 was weak
    # the RANSAC5 rewrite: exactly the tracked features RANSAC5 rejected became outliers, at their original numbers
    keep1 = np.nonzero(ts_in[1] == 0)[0]
    assert 0 < int((ts[1][keep1] == 3).sum()) < len(keep1) and (ts[1][ts_in[1] != 0] == ts_in[1][ts_in[1] != 0]).all()


def test_profile_class_counts_the_launches(oracle):
    ocam, gcam, f, spec = _cams(oracle, "pinhole")
    c1, c2, _, _ = R.make_set(np.random.default_rng(1), (ocam, spec), 50, 0.2, 0.3)
    with capi.Context(width=752, height=480) as ctx:
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(3):
            ctx.ransac5(c1, c2, gcam, gcam)
        ms, n = ctx.profile_read(capi.K_RANSAC5)
        assert n == 3 and ms > 0
        ms2, n2 = ctx.profile_read(capi.K_ROT_RANSAC)
        assert n2 == 0


EDGE_COUNTS = [0, 1, 4, 5, 6, 63, 64, 65, 128, 129, 769, 1023, 1024]


def _edge_masks(n):
    """All TRACKED; every second feature; feature 0 and the last feature of every 64-feature chunk."""
    i = np.arange(n)
    return [np.ones(n, bool), i % 2 == 0, (i % 64 == 63) | (i == 0)]


def test_compaction_and_gather_at_the_chunk_edges(oracle):
    """The ordered compaction (TRACKED features, then valid points) and the gather behind it at their edges: one launch of the
    hybrid entry with max_points = 1024, point counts around the 64-feature chunks and the 256-thread strides, three
    track-status masks per count. Noise-free general scenes with 20 % outliers, so the inlier counts are far from a tie and
    pow / log of the iteration update cannot fork: every set must equal the restatement (statuses, type, count, score,
    summary; E as in the well-separated test), none exempted. Counts from 63 up carry features whose second corner is outside
    the fisheye's valid field of view: normalizePixel fails there and the gather moves the points behind them."""
    import torch
    ocam, gcam, f, spec = _cams(oracle, "fisheye")
    rng = np.random.default_rng(77)
    MP = 1024
    sets = []
    for n in EDGE_COUNTS:
        c1, c2 = (R.make_set(rng, (ocam, spec), n, 0.2, 0.0)[:2]) if n else (np.zeros((0, 2), np.float32),) * 2
        if n >= 63:
            c2 = c2.copy()
            c2[[i for i in (2, 63, 2 * (n // 4)) if i < n]] = (-150.0, -120.0)
        for mask in _edge_masks(n):
            sel = np.nonzero(mask)[0]
            r2 = np.full(n, 3, np.int32)
            r2[sel[::2]] = 0                                                   # RANSAC2 "found" every second tracked feature
            sets.append(dict(n=n, c1=c1, c2=c2, sel=sel, ts=np.where(mask, 0, 2).astype(np.int32), r2=r2,
                             r2count=len(sel[::2]) if len(sel) >= 2 else 0))    # doRansac2 does not run below two tracks
    S = len(sets)
    c1 = np.zeros((S, MP, 2), np.float32); c2 = np.zeros((S, MP, 2), np.float32)
    ts = np.full((S, MP), -9, np.int32); r2 = np.full((S, MP), -7, np.int32)
    cnt = np.array([d["n"] for d in sets], np.int32); r2s = np.zeros((S, 2), np.int32)
    for s, d in enumerate(sets):
        n = d["n"]
        c1[s, :n], c2[s, :n], ts[s, :n], r2[s, :n], r2s[s, 0] = d["c1"], d["c2"], d["ts"], d["r2"], d["r2count"]
    with capi.Context(width=752, height=480) as ctx:
        d_c1, d_c2, d_ts, d_r2, d_n, d_r2s = (torch.from_numpy(x).cuda() for x in (c1, c2, ts, r2, cnt, r2s))
        d_res = torch.full((S, 2), -1, dtype=torch.int32, device="cuda"); d_score = torch.full((S,), -1.0, dtype=torch.float64, device="cuda")
        d_E = torch.full((S, 9), 7.0, dtype=torch.float64, device="cuda"); d_sm = torch.full((S, 4), -5, dtype=torch.int32, device="cuda")
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.hybrid_ransac_lk_batch_dev(S, MP, d_n.data_ptr(), d_c1.data_ptr(), d_c2.data_ptr(), d_ts.data_ptr(), d_r2.data_ptr(),
                                       d_r2s.data_ptr(), gcam, gcam, d_res.data_ptr(), d_score.data_ptr(), d_E.data_ptr(), d_sm.data_ptr())
        torch.cuda.synchronize()
        g_ts, g_res, g_score, g_E, g_sm = (t.cpu().numpy() for t in (d_ts, d_res, d_score, d_E, d_sm))
    norm = [R.normalize(d["c1"][d["sel"]], d["c2"][d["sel"]], ocam, ocam) for d in sets]
    runs = R.registrator_runs([(h1, h2, R.threshold(f, f)) for h1, h2, _ in norm])
    types, moved = [], 0
    for s, d in enumerate(sets):
        n, sel = d["n"], d["sel"]
        want_ts, typ, count, score = R.hybrid_pipeline(d["ts"], d["c1"], d["c2"], d["r2"], d["r2count"], ocam, ocam, f, f, run=runs[s])
        done, _, E_r, sm_r, _ = R.do_ransac5(d["c1"][sel], d["c2"][sel], ocam, ocam, f, f, run=runs[s])
        print("set", s, "n", n, "tracked", len(sel), "type", typ, "count", count, "summary", sm_r, "gpu", g_res[s], g_sm[s])
        assert np.array_equal(g_ts[s, :n], want_ts) and (g_ts[s, n:] == -9).all(), (s, n)
        assert g_res[s].tolist() == [typ, count] and g_score[s] == score and g_sm[s].tolist() == list(sm_r), (s, n, g_res[s], g_sm[s], typ, count, sm_r)
        assert (_e_dist(g_E[s], E_r) <= 1e-7) if E_r.any() else not g_E[s].any(), (s, n)
        types.append(typ)
        moved += 5 <= sm_r[3] < len(sel)
    assert {R.TYPE_SKIPPED, R.TYPE_R2, R.TYPE_R5} <= set(types), types          # (by the restatement: the batch reaches every outcome,
    assert moved >= 10                                                         # and sets where valid points < TRACKED features)
