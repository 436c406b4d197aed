"""GPU tests of the stereo track gate (hv_flow_status_batch_dev, hv_track_gate*, hv_detection_filter*) against the numpy
restatement tests/stereo_gate_restatement.py: a corpus of 2016 synthetic sets, the synchronous / batched / graph-replayed
forms, the device chains LK -> flow status -> gate -> RANSAC2 -> hybrid RANSAC and GFTT -> cornerSubPix -> stereo LK ->
detection filter, and a closed stereo tracker loop at 752x480 with the gate and the detection filter on."""
import math

import numpy as np
import pytest

import ransac5_restatement as R
import stereo_gate_restatement as G
import test_gpu_tracker_closed_loop as CL
from hybvio_amd import capi, synth

pytestmark = pytest.mark.gpu
W, H = 752, 480
MP = 24                                   # max_points of the corpus sets
SETS_PER_CONFIG = 126                     # 4 cameras x 2 transforms x 2 crops x 126 = 2016 sets


def _rot(v):
    return R.rotation(v)


CAMERAS = {
    "pinhole": (("pinhole", 400.0, 402.0, 376.0, 240.0), {}, {}),
    "radial": (("pinhole", 395.0, 398.0, 370.0, 236.0), dict(coeffs=(-0.25, 0.07, 0.0)), dict(coeffs=(-0.24, 0.06, 0.0))),
    "rectified": (("pinhole", 410.0, 410.0, 380.0, 245.0), dict(rotation=_rot([0.01, -0.02, 0.005])), dict(rotation=_rot([-0.01, 0.015, 0.0]))),
    "fisheye": (("fisheye", 300.0, 301.0, 376.0, 240.0), dict(coeffs=(0.02, -0.01, 0.003, -0.0005), max_valid_fov_deg=150.0),
                dict(coeffs=(0.02, -0.01, 0.003, -0.0005), max_valid_fov_deg=150.0)),
}


def _transforms():
    a = np.eye(4)
    a[0, 3] = -0.1                                                    # a baseline along x
    b = np.eye(4)
    b[:3, :3] = _rot([0.02, -0.03, 0.01])
    b[:3, 3] = (-0.08, 0.03, 0.01)                                    # rotation and a vertical component
    return {"baseline_x": a, "rotated_vertical": b}


def _cams(oracle, name):
    args, k0, k1 = CAMERAS[name]
    k1 = {**k0, **k1} if name != "rectified" else k1
    return (oracle.Camera(*args, **k0), oracle.Camera(*args, **k1), capi.camera_model(*args, **k0), capi.camera_model(*args, **k1))


def _dev(x, dt=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x if dt is None else np.asarray(x, dt))).cuda()


def _make_sets(rng, ocam0, ocam1, T, dist, n_sets, sizes=None):
    """n_sets sets of 1..MP points (or of the given sizes): right corners on, near (within +-2 px of dist), far from the
    left corner's curve, or outside the image; mixed flow statuses and blacklists."""
    sets = []
    for k in range(n_sets):
        n = int(rng.integers(1, MP + 1)) if sizes is None else sizes[k]
        left = rng.uniform([0, 0], [W, H], (n, 2))
        out_l = rng.random(n) < 0.03
        left[out_l] = rng.choice([-2.0, W + 1.0], out_l.sum())[:, None] * np.array([1, 0]) + left[out_l] * np.array([0, 1])
        left = left.astype(np.float32)
        right = np.zeros((n, 2), np.float32)
        for i in range(n):
            kind = rng.choice(4, p=[0.35, 0.35, 0.2, 0.1])
            ok, ray = ocam0.pixel_to_ray(float(left[i, 0]), float(left[i, 1]))
            on = None
            if ok:
                p3 = T[:3, :3] @ (rng.uniform(0.6, 50.0) * ray) + T[:3, 3]
                ok2, pix = ocam1.ray_to_pixel(p3)
                on = pix if ok2 else None
            if on is None:
                on = rng.uniform([0, 0], [W, H])
            ang = rng.uniform(0, 2 * math.pi)
            u = np.array([math.cos(ang), math.sin(ang)])
            if kind == 0:
                r = on
            elif kind == 1:
                r = on + u * (float(dist) + rng.uniform(-2, 2))
            elif kind == 2:
                r = on + u * rng.uniform(20, 60)
            else:
                r = np.array([rng.choice([-3.0, W + 2.0]), on[1]])
            right[i] = r
        ts = rng.choice([0, 0, 0, 0, 0, 0, 0, 2, 3, 4], n).astype(np.int32)
        ss = rng.choice([0, 0, 0, 0, 0, 0, 2, 4], n).astype(np.int32)
        bl = (rng.random(n) < 0.05).astype(np.uint8)
        sets.append(dict(left=left, right=right, ts=ts, ss=ss, bl=bl))
    return sets


def _pack(sets, key, shape_tail, dt, fill, mp=MP):
    out = np.full((len(sets), mp) + shape_tail, fill, dt)
    for s, d in enumerate(sets):
        out[s, :len(d[key])] = d[key]
    return out


def _run_corpus_config(ctx, sets, g0, g1, gp, mp=MP):
    import torch
    S, MP = len(sets), mp
    cnt = np.array([len(d["left"]) for d in sets], np.int32)
    d_n = _dev(cnt)
    d_l, d_r = _dev(_pack(sets, "left", (2,), np.float32, 0, mp)), _dev(_pack(sets, "right", (2,), np.float32, 0, mp))
    d_ts = _dev(_pack(sets, "ts", (), np.int32, -9, mp))
    d_ss = _dev(_pack(sets, "ss", (), np.int32, 0, mp))
    d_bl = _dev(_pack(sets, "bl", (), np.uint8, 0, mp))
    d_mask = torch.full((S, MP), 77, dtype=torch.uint8, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.track_gate_batch_dev(S, MP, d_n.data_ptr(), d_l.data_ptr(), d_r.data_ptr(), d_ss.data_ptr(), d_bl.data_ptr(), g0, g1,
                             d_ts.data_ptr(), d_mask.data_ptr(), params=gp)
    d_st = torch.full((S, MP), -9, dtype=torch.int32, device="cuda")
    d_ol = torch.full((S, MP, 2), float("nan"), dtype=torch.float32, device="cuda")
    d_or = torch.full((S, MP, 2), float("nan"), dtype=torch.float32, device="cuda")
    d_no = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    ctx.detection_filter_batch_dev(S, MP, d_n.data_ptr(), d_l.data_ptr(), d_r.data_ptr(), d_ss.data_ptr(), g0, g1, d_st.data_ptr(),
                                   d_ol.data_ptr(), d_or.data_ptr(), d_no.data_ptr(), params=gp)
    torch.cuda.synchronize()
    return (d_ts.cpu().numpy(), d_mask.cpu().numpy(), d_st.cpu().numpy(), d_ol.cpu().numpy(), d_or.cpu().numpy(), d_no.cpu().numpy())


@pytest.fixture(scope="module")
def corpus(oracle):
    rng = np.random.default_rng(2026)
    out = []
    with capi.Context(width=W, height=H) as ctx:
        for cname in CAMERAS:
            o0, o1, g0, g1 = _cams(oracle, cname)
            for tname, T in _transforms().items():
                for part in (1.0, 0.8):
                    prm = G.Params(partOfImageToDetectFeatures=part, fisheyeCamera=cname == "fisheye", cam0ToCam1=T)
                    gp = capi.stereo_gate_default_params(partOfImageToDetectFeatures=part, fisheyeCamera=int(cname == "fisheye"),
                                                         cam0ToCam1=T)
                    dist, _ = G.epipolar_dist(W, H, prm.maxStereoEpipolarDistance)
                    sets = _make_sets(rng, o0, o1, T, dist, SETS_PER_CONFIG)
                    ts, mask, st, ol, orr, no = _run_corpus_config(ctx, sets, g0, g1, gp)
                    mt = g1.max_theta if cname == "fisheye" else None
                    for s, d in enumerate(sets):
                        n = len(d["left"])
                        ginfo, finfo = [], []
                        want = G.track_gate(d["left"], d["right"], d["ss"], d["bl"], d["ts"], o0, o1, W, H, prm, mt, ginfo)
                        kl, kr, fst = G.detection_filter(d["left"], d["right"], d["ss"], o0, o1, W, H, prm, mt, finfo)
                        assert (ts[s, n:] == -9).all() and (mask[s, n:] == 77).all() and (st[s, n:] == -9).all()   # padding untouched
                        assert np.array_equal(mask[s, :n], (ts[s, :n] == 0).astype(np.uint8))
                        d.update(cam=cname, T=tname, part=part, want=want, gate=ts[s, :n], ginfo=ginfo, fwant=(kl, kr, fst),
                                 fgot=(ol[s, :no[s]], orr[s, :no[s]], st[s, :n]), finfo=finfo, no=int(no[s]))
                    out += sets
    return out


def _close(info, i):
    margin, theta_close = info[i]
    return margin < 1e-5 or theta_close


def test_corpus_against_the_restatement(corpus):
    assert len(corpus) >= 2000
    gate_bad, filt_bad, statuses = [], [], set()
    for k, d in enumerate(corpus):
        diff = np.nonzero(d["gate"] != d["want"])[0]
        fk, fr, fs = d["fwant"]
        gl, gr, gs = d["fgot"]
        fdiff = np.nonzero(gs != fs)[0]
        same_filter = d["no"] == len(fk) and np.array_equal(gl, fk) and np.array_equal(gr, fr) and len(fdiff) == 0
        statuses |= set(d["want"].tolist())
        if d["cam"] != "fisheye":
            assert len(diff) == 0, (k, d["cam"], d["T"], d["part"], d["gate"], d["want"])
            assert same_filter, (k, d["cam"], d["T"], d["part"], gs, fs)
            continue
        for i in diff:
            assert _close(d["ginfo"], i), (k, i, d["gate"][i], d["want"][i], d["ginfo"][i])
            gate_bad.append((k, int(i)))
        if not same_filter:
            assert all(_close(d["finfo"], i) for i in fdiff), (k, fdiff, d["finfo"])
            filt_bad.append(k)
    print(f"fisheye: {len(gate_bad)} gate statuses and {len(filt_bad)} filter sets differ within the tolerance")
    assert {G.TRACKED, G.FAILED_FLOW, G.FAILED_EPIPOLAR_CHECK, G.OUT_OF_RANGE, G.BLACKLISTED, 3, 4} <= statuses
    fe = [d for d in corpus if d["cam"] == "fisheye"]
    assert any((d["want"] == G.OUT_OF_RANGE).any() and d["part"] == 1.0 for d in fe)        # pixelToRay failures of the crop
    for name in CAMERAS:                                                                     # every camera reaches both outcomes
        sub = [d for d in corpus if d["cam"] == name]
        assert any((d["want"] == G.FAILED_EPIPOLAR_CHECK).any() for d in sub), name
        assert sum(int((d["want"] == G.TRACKED).sum()) for d in sub) > 100, name


def test_flow_status_and_the_synchronous_batched_and_graph_replayed_forms_agree(oracle):
    import torch
    o0, o1, g0, g1 = _cams(oracle, "radial")
    T = _transforms()["rotated_vertical"]
    prm = G.Params(partOfImageToDetectFeatures=0.8, cam0ToCam1=T)
    gp = capi.stereo_gate_default_params(partOfImageToDetectFeatures=0.8, cam0ToCam1=T)
    rng = np.random.default_rng(5)
    ns = [1, 7, 64, 65, 200, 1000, 1024, 0, 333]
    S, M = len(ns), 1024
    dist, _ = G.epipolar_dist(W, H, 10.0)
    sets = _make_sets(rng, o0, o1, T, dist, S, sizes=ns)
    cnt = np.array([len(d["left"]) for d in sets], np.int32)
    with capi.Context(width=W, height=H) as ctx:
        # flow status: NaN, the image edges and the LK status
        xy = np.array([[0, 0], [-1e-7, 5], [np.nextafter(np.float32(W), np.float32(0)), 4], [W, 10], [10, H], [np.nan, 3], [5, 5],
                       [760, 5], [3, np.nan], [100, 100]], np.float32)
        lk = np.array([1, 1, 1, 1, 1, 1, 0, 0, 1, 0], np.uint8)
        d_xy, d_lk = _dev(xy[None]), _dev(lk[None])
        d_fs = torch.full((1, 12), -9, dtype=torch.int32, device="cuda")
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.flow_status_batch_dev(1, 10, _dev(np.array([10], np.int32)).data_ptr(), d_xy.data_ptr(), d_lk.data_ptr(), d_fs.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_fs.cpu().numpy()[0, :10], G.flow_status(lk, xy, W, H))
        # synchronous forms vs the restatement
        sync_g = [ctx.track_gate(d["left"], d["right"], d["ss"], d["ts"], g0, g1, blacklist=d["bl"], params=gp) for d in sets]
        sync_f = [ctx.detection_filter(d["left"], d["right"], d["ss"], g0, g1, params=gp) for d in sets]
        for d, sg, sf in zip(sets, sync_g, sync_f):
            assert np.array_equal(sg, G.track_gate(d["left"], d["right"], d["ss"], d["bl"], d["ts"], o0, o1, W, H, prm))
            kl, kr, fs = G.detection_filter(d["left"], d["right"], d["ss"], o0, o1, W, H, prm)
            assert np.array_equal(sf[0], kl) and np.array_equal(sf[1], kr) and np.array_equal(sf[2], fs)
        # mono
        d = sets[4]
        mono = ctx.track_gate(d["left"], None, None, d["ts"], g0, None, blacklist=d["bl"], params=gp)
        assert np.array_equal(mono, G.track_gate(d["left"], None, None, d["bl"], d["ts"], o0, None, W, H, prm))
        mk, mr, ms = ctx.detection_filter(d["left"], None, None, g0, params=gp)
        wk, wr, ws = G.detection_filter(d["left"], None, None, o0, None, W, H, prm)
        assert mr is None and np.array_equal(mk, wk) and np.array_equal(ms, ws)
        # batched eager
        eager = _run_corpus_config(ctx, sets, g0, g1, gp, M)
        for s, d in enumerate(sets):
            n = cnt[s]
            assert np.array_equal(eager[0][s, :n], sync_g[s]) and eager[5][s] == len(sync_f[s][0])
            assert np.array_equal(eager[3][s, :eager[5][s]], sync_f[s][0]) and np.array_equal(eager[4][s, :eager[5][s]], sync_f[s][1])
        # graph-replayed (gate + filter in one capture); the in-place filter compacts its own inputs
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        d_n = _dev(cnt)
        l0, r0 = _pack(sets, "left", (2,), np.float32, 0, M), _pack(sets, "right", (2,), np.float32, 0, M)
        ts0 = _pack(sets, "ts", (), np.int32, -9, M)
        d_l, d_r, d_ts = _dev(l0), _dev(r0), _dev(ts0)
        d_ss, d_bl = _dev(_pack(sets, "ss", (), np.int32, 0, M)), _dev(_pack(sets, "bl", (), np.uint8, 0, M))
        d_mask = torch.zeros((S, M), dtype=torch.uint8, device="cuda")
        d_no = torch.zeros(S, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            ctx.track_gate_batch_dev(S, M, d_n.data_ptr(), d_l.data_ptr(), d_r.data_ptr(), d_ss.data_ptr(), d_bl.data_ptr(), g0, g1,
                                     d_ts.data_ptr(), d_mask.data_ptr(), params=gp)
            ctx.detection_filter_batch_dev(S, M, d_n.data_ptr(), d_l.data_ptr(), d_r.data_ptr(), d_ss.data_ptr(), g0, g1, 0,
                                           d_l.data_ptr(), d_r.data_ptr(), d_no.data_ptr(), params=gp)
        for _ in range(2):
            with torch.cuda.stream(stream):
                d_l.copy_(_dev(l0)); d_r.copy_(_dev(r0)); d_ts.copy_(_dev(ts0)); d_no.fill_(-1)
                g.replay()
            stream.synchronize()
            gts, gl, gr, gno = d_ts.cpu().numpy(), d_l.cpu().numpy(), d_r.cpu().numpy(), d_no.cpu().numpy()
            assert np.array_equal(gno, eager[5])
            for s in range(S):
                n, m = cnt[s], gno[s]
                assert np.array_equal(gts[s, :n], sync_g[s]) and np.array_equal(gl[s, :m], sync_f[s][0]) and np.array_equal(gr[s, :m], sync_f[s][1])
                assert np.array_equal(gl[s, m:n], l0[s, m:n])            # behind the kept pairs the inputs stay as they were
        del g


def test_device_chain_lk_gate_rotation_and_hybrid_ransac(oracle):
    """hv_klt_track_batch_dev (left) -> flow status -> hv_klt_track_batch_dev (stereo) -> flow status -> gate ->
    hv_rot_ransac_lk_batch_dev on the tracked mask -> hv_hybrid_ransac_lk_batch_dev, nothing through the host; every stage
    equals the restatement (and the oracle's RANSAC2) applied to the same device LK outputs."""
    import torch
    w, h, npts, S = 376, 240, 150, 4
    cam_args, radial = ("pinhole", 229.3, 228.6, 183.6, 124.2), [-0.28, 0.07, 0.0]
    ocam, gcam = oracle.Camera(*cam_args, coeffs=radial), capi.camera_model(*cam_args, coeffs=radial)
    f = (cam_args[1] + cam_args[2]) * 0.5
    thr = float(np.float32((4.0 * min(w, h) / 720.0) ** 2))
    T = np.eye(4)
    T[0, 3] = -0.1
    prm = G.Params(partOfImageToDetectFeatures=0.95, cam0ToCam1=T)
    gp = capi.stereo_gate_default_params(partOfImageToDetectFeatures=0.95, cam0ToCam1=T)
    seqs = [synth.stereo_sequence(60 + s, w, h, 2) for s in range(S)]
    pts = np.stack([synth.grid_points(w, h, npts, margin=12, seed=s) for s in range(S)]).astype(np.float32)
    draws = np.stack([oracle.mt19937_draws(4649 + s, 200) for s in range(S)])
    bl = (np.random.default_rng(4).random((S, npts)) < 0.03).astype(np.uint8)
    with capi.Context(width=w, height=h, pool_size=3 * S, max_tracks=npts) as ctx:
        prev = [ctx.acquire() for _ in range(S)]; cur = [ctx.acquire() for _ in range(S)]; rgt = [ctx.acquire() for _ in range(S)]
        for s in range(S):
            ctx.build(prev[s], seqs[s][0][0]); ctx.build(cur[s], seqs[s][0][1]); ctx.build(rgt[s], seqs[s][1][1])
        d_prev, d_cur, d_rgt = _dev(prev, np.int32), _dev(cur, np.int32), _dev(rgt, np.int32)
        d_pts, d_n, d_bl = _dev(pts), _dev(np.full(S, npts, np.int32)), _dev(bl)
        d_next = torch.zeros_like(d_pts); d_lk = torch.zeros((S, npts), dtype=torch.uint8, device="cuda")
        d_right = torch.zeros_like(d_pts); d_lk2 = torch.zeros((S, npts), dtype=torch.uint8, device="cuda")
        d_ts = torch.zeros((S, npts), dtype=torch.int32, device="cuda"); d_ss = torch.zeros_like(d_ts)
        d_mask = torch.zeros((S, npts), dtype=torch.uint8, device="cuda")
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.klt_track_batch_dev(S, d_prev.data_ptr(), d_cur.data_ptr(), npts, d_pts.data_ptr(), d_next.data_ptr(), d_lk.data_ptr(), 0,
                                use_initial_flow=False)
        ctx.flow_status_batch_dev(S, npts, d_n.data_ptr(), d_next.data_ptr(), d_lk.data_ptr(), d_ts.data_ptr())
        ctx.klt_track_batch_dev(S, d_cur.data_ptr(), d_rgt.data_ptr(), npts, d_next.data_ptr(), d_right.data_ptr(), d_lk2.data_ptr(), 0,
                                use_initial_flow=False)
        # set 1: a fifth of the right corners moved 15 px down, off their curves (FAILED_EPIPOLAR_CHECK)
        d_right[1, ::5, 1] += 15.0
        ctx.flow_status_batch_dev(S, npts, d_n.data_ptr(), d_right.data_ptr(), d_lk2.data_ptr(), d_ss.data_ptr())
        left_ts = d_ts.clone()
        ctx.track_gate_batch_dev(S, npts, d_n.data_ptr(), d_next.data_ptr(), d_right.data_ptr(), d_ss.data_ptr(), d_bl.data_ptr(), gcam,
                                 gcam, d_ts.data_ptr(), d_mask.data_ptr(), params=gp)
        gated = d_ts.clone()
        d_r2 = torch.full((S, npts), -7, dtype=torch.int32, device="cuda")
        d_R = torch.zeros((S, 9), dtype=torch.float32, device="cuda"); d_r2s = torch.zeros((S, 2), dtype=torch.int32, device="cuda")
        ctx.rot_ransac_lk_batch_dev(S, npts, d_n.data_ptr(), d_pts.data_ptr(), d_next.data_ptr(), d_mask.data_ptr(), 1, gcam, gcam,
                                    _dev(draws, np.uint32).data_ptr(), thr, d_r2.data_ptr(), d_R.data_ptr(), d_r2s.data_ptr())
        d_res = torch.zeros((S, 2), dtype=torch.int32, device="cuda"); d_score = torch.zeros(S, dtype=torch.float64, device="cuda")
        ctx.hybrid_ransac_lk_batch_dev(S, npts, d_n.data_ptr(), d_pts.data_ptr(), d_next.data_ptr(), d_ts.data_ptr(), d_r2.data_ptr(),
                                       d_r2s.data_ptr(), gcam, gcam, d_res.data_ptr(), d_score.data_ptr())
        torch.cuda.synchronize()
        host = lambda t: t.cpu().numpy()
        nxt, lk, rxy, lk2, lts, sst = host(d_next), host(d_lk), host(d_right), host(d_lk2), host(left_ts), host(d_ss)
        gts, mask, r2, r2s, ts, res, score = host(gated), host(d_mask), host(d_r2), host(d_r2s), host(d_ts), host(d_res), host(d_score)
    epi = 0
    for s in range(S):
        assert np.array_equal(lts[s], G.flow_status(lk[s], nxt[s], w, h)) and np.array_equal(sst[s], G.flow_status(lk2[s], rxy[s], w, h))
        want = G.track_gate(nxt[s], rxy[s], sst[s], bl[s], lts[s], ocam, ocam, w, h, prm)
        assert np.array_equal(gts[s], want), s
        assert np.array_equal(mask[s], (want == 0).astype(np.uint8))
        sel = np.nonzero(want == 0)[0]
        o_st, _, o_best, _ = oracle.rot_ransac_fit(pts[s][sel], nxt[s][sel], ocam, ocam, draws[s], thr)
        assert np.array_equal(r2[s][sel], o_st) and r2s[s, 0] == o_best, s                  # RANSAC2 ran on exactly compute()'s set
        want_ts, typ, cnt, sc = R.hybrid_pipeline(want, pts[s], nxt[s], r2[s], int(r2s[s, 0]), ocam, ocam, f, f)
        assert np.array_equal(ts[s], want_ts) and res[s].tolist() == [typ, cnt] and score[s] == sc, s
        epi += int((want == G.FAILED_EPIPOLAR_CHECK).sum())
    assert int((gts[1] == G.FAILED_EPIPOLAR_CHECK).sum()) >= npts // 10 and epi > 0
    assert (gts == G.BLACKLISTED).any() and (gts == G.TRACKED).sum() > S * npts // 2


def test_detection_chain_gftt_subpix_stereo_lk_and_filter(oracle):
    """hv_gftt_detect -> hv_corner_subpix_batch_dev -> stereo hv_klt_track_batch_ragged_dev -> flow status -> detection filter:
    the compacted pairs and counts equal the restatement on the same device outputs."""
    import torch
    S, M = 3, 400
    cam_args, radial = CL.cam_args(W, H)
    ocam, gcam = oracle.Camera(*cam_args, coeffs=radial), capi.camera_model(*cam_args, coeffs=radial)
    T = np.eye(4)
    T[:3, 3] = (-0.1, 0.01, 0.0)
    prm = G.Params(partOfImageToDetectFeatures=0.9, cam0ToCam1=T)
    gp = capi.stereo_gate_default_params(partOfImageToDetectFeatures=0.9, cam0ToCam1=T)
    seqs = [synth.stereo_sequence(90 + s, W, H, 1) for s in range(S)]
    with capi.Context(width=W, height=H, pool_size=2 * S, max_tracks=M) as ctx:
        ls = [ctx.acquire() for _ in range(S)]; rs = [ctx.acquire() for _ in range(S)]
        corners = np.zeros((S, M, 2), np.float32)
        cnt = np.zeros(S, np.int32)
        for s in range(S):
            ctx.build(ls[s], seqs[s][0][0]); ctx.build(rs[s], seqs[s][1][0])
            c = ctx.gftt_detect(ls[s], params=capi.gftt_default_params(maxTracks=M))[:M]
            corners[s, :len(c)], cnt[s] = c, len(c)
        assert (cnt > 50).all()
        d_l, d_r, d_c, d_n = _dev(np.array(ls, np.int32)), _dev(np.array(rs, np.int32)), _dev(corners), _dev(cnt)
        d_right = torch.zeros_like(d_c); d_lk = torch.zeros((S, M), dtype=torch.uint8, device="cuda")
        d_ss = torch.zeros((S, M), dtype=torch.int32, device="cuda"); d_st = torch.full((S, M), -9, dtype=torch.int32, device="cuda")
        d_ol = torch.zeros_like(d_c); d_or = torch.zeros_like(d_c); d_no = torch.zeros(S, dtype=torch.int32, device="cuda")
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.corner_subpix_batch_dev(S, d_l.data_ptr(), M, d_n.data_ptr(), d_c.data_ptr())
        ctx.klt_track_batch_ragged_dev(S, d_l.data_ptr(), d_r.data_ptr(), M, d_n.data_ptr(), d_c.data_ptr(), d_right.data_ptr(),
                                       d_lk.data_ptr(), 0, use_initial_flow=False)
        ctx.flow_status_batch_dev(S, M, d_n.data_ptr(), d_right.data_ptr(), d_lk.data_ptr(), d_ss.data_ptr())
        ctx.detection_filter_batch_dev(S, M, d_n.data_ptr(), d_c.data_ptr(), d_right.data_ptr(), d_ss.data_ptr(), gcam, gcam,
                                       d_st.data_ptr(), d_ol.data_ptr(), d_or.data_ptr(), d_no.data_ptr(), params=gp)
        torch.cuda.synchronize()
        sub, rxy, lk, ss, st, ol, orr, no = (t.cpu().numpy() for t in (d_c, d_right, d_lk, d_ss, d_st, d_ol, d_or, d_no))
    seen = set()
    for s in range(S):
        n = cnt[s]
        assert not np.array_equal(sub[s, :n], corners[s, :n])                               # cornerSubPix moved the corners
        assert np.array_equal(ss[s, :n], G.flow_status(lk[s, :n], rxy[s, :n], W, H))
        kl, kr, fs = G.detection_filter(sub[s, :n], rxy[s, :n], ss[s, :n], ocam, ocam, W, H, prm)
        assert no[s] == len(kl) and np.array_equal(ol[s, :no[s]], kl) and np.array_equal(orr[s, :no[s]], kr) and np.array_equal(st[s, :n], fs)
        seen |= set(fs.tolist())
        assert 0 < no[s] < n
    assert {G.TRACKED, G.OUT_OF_RANGE} <= seen, seen


# ---- closed stereo loop: TrackerImplementation's order (LK left, stereo LK, gate, RANSAC2 on TRACKED, detection + filter) ----
GATE_T = np.array([[1.0, 0.0, 0.0, -0.1], [0.0, 1.0, 0.0, 0.015], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
GATE_PART = 0.95


class HipStereo(CL.HipBackend):
    def __init__(self, w, h, max_tracks, min_dist):
        super().__init__(w, h, max_tracks, min_dist)
        self.gate_params = capi.stereo_gate_default_params(partOfImageToDetectFeatures=GATE_PART, cam0ToCam1=GATE_T)

    def gate(self, left, right, stereo_status, track_status):
        return self.ctx.track_gate(left, right, stereo_status, track_status, self.cam, self.cam, params=self.gate_params)

    def detection_filter(self, left, right, stereo_status):
        return self.ctx.detection_filter(left, right, stereo_status, self.cam, self.cam, params=self.gate_params)


class OracleStereo(CL.OracleBackend):
    def __init__(self, oracle, w, h, max_tracks, min_dist):
        super().__init__(oracle, w, h, max_tracks, min_dist)
        self.w, self.h = w, h
        self.prm = G.Params(partOfImageToDetectFeatures=GATE_PART, cam0ToCam1=GATE_T)

    def gate(self, left, right, stereo_status, track_status):
        return G.track_gate(left, right, stereo_status, None, track_status, self.cam, self.cam, self.w, self.h, self.prm)

    def detection_filter(self, left, right, stereo_status):
        return G.detection_filter(left, right, stereo_status, self.cam, self.cam, self.w, self.h, self.prm)


def run_stereo_tracker(be, oracle, left, right, w, h, max_tracks, min_dist):
    log, tracks = [], []
    prev_l = None
    thr = float(np.float32((1.0 * min(w, h) / 720.0) ** 2))
    epi = [0, 0]
    for frame in range(len(left)):
        cur_l, cur_r = be.build(left[frame]), be.build(right[frame])
        next_id = frame * max_tracks + 1
        status = np.zeros(0, np.int32)
        if frame > 0 and len(tracks) >= 5:
            p0 = np.array([t[1] for t in tracks], np.float32)
            vel = np.array([t[3] for t in tracks], np.float32)
            xy, st = be.flow(prev_l, cur_l, p0, guess=p0 + vel)
            xr, st2 = be.flow(cur_l, cur_r, xy, guess=np.array([t[2] for t in tracks], np.float32) + (xy - p0))
            status = np.asarray(be.gate(xy, xr, st2, st), np.int32)                    # tracker.cpp:441-478
            epi[0] += int((status == G.FAILED_EPIPOLAR_CHECK).sum())
            ok = np.flatnonzero(status == 0)
            if len(ok) >= 2:
                rs, _ = be.ransac(oracle, p0[ok], xy[ok], thr)
                status[ok] = np.where(rs == 3, 3, status[ok])
            tracks = [[t[0], tuple(xy[i]), tuple(xr[i]), tuple(xy[i] - p0[i])] for i, t in enumerate(tracks) if status[i] == 0]
        missing = max_tracks - len(tracks)
        if frame == 0 or missing >= max_tracks // 10:
            mask = np.array([t[1] for t in tracks], np.float32).reshape(-1, 2)
            corners = be.detect(cur_l, mask, min_dist)
            if len(corners):
                cr, sts = be.flow(cur_l, cur_r, corners)
                kl, kr, fst = be.detection_filter(corners, cr, sts)                     # tracker.cpp:266-311
                epi[1] += int((np.asarray(fst) == G.FAILED_EPIPOLAR_CHECK).sum())
                for i in range(min(len(kl), missing)):
                    tracks.append([next_id, tuple(kl[i]), tuple(kr[i]), (0.0, 0.0)]); next_id += 1
        log.append((np.array([t[0] for t in tracks]), np.array([t[1] for t in tracks], np.float32).reshape(-1, 2),
                    np.array([t[2] for t in tracks], np.float32).reshape(-1, 2), status.copy()))
        if prev_l is not None:
            be.release(prev_l)
            be.release(prev_r)
        prev_l, prev_r = cur_l, cur_r
    return log, be.pos, epi


def test_closed_stereo_loop_with_the_gate_identical_over_a_sequence(oracle):
    w, h, max_tracks, min_dist, unique, frames = 752, 480, 200, 30, 40, 60
    left, right = CL.moving_sequence(77, w, h, unique, frames, radius=0.5 * unique, rot=1.2)
    hip = HipStereo(w, h, max_tracks, min_dist)
    try:
        hip.ctx.profile_enable(True)
        got, pos_hip, epi_hip = run_stereo_tracker(hip, oracle, left, right, w, h, max_tracks, min_dist)
        _, launches = hip.ctx.profile_read(capi.K_STEREO_GATE)
    finally:
        hip.ctx.close()
    ref, pos_ref, epi_ref = run_stereo_tracker(OracleStereo(oracle, w, h, max_tracks, min_dist), oracle, left, right, w, h, max_tracks,
                                               min_dist)
    for f, ((gi, gl, gr, gs), (oi, ol, orr, os_)) in enumerate(zip(got, ref)):
        np.testing.assert_array_equal(gs, os_, err_msg=f"frame {f}: status")
        np.testing.assert_array_equal(gi, oi, err_msg=f"frame {f}: track ids")
        np.testing.assert_array_equal(gl, ol, err_msg=f"frame {f}: left positions")
        np.testing.assert_array_equal(gr, orr, err_msg=f"frame {f}: right positions")
    assert pos_hip == pos_ref > 0 and epi_hip == epi_ref
    assert epi_hip[0] > 0, epi_hip                                                     # the gate failed tracks on the epipolar check
    assert len(got[-1][0]) >= max_tracks // 2 and launches >= frames
    print("stereo loop: epipolar failures (gate, detection) =", epi_hip, "tracks at the end:", len(got[-1][0]))


def test_profile_class_counts_the_launches(oracle):
    o0, o1, g0, g1 = _cams(oracle, "pinhole")
    d = _make_sets(np.random.default_rng(1), o0, o1, _transforms()["baseline_x"], 6.7, 1)[0]
    with capi.Context(width=W, height=H) as ctx:
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(3):
            ctx.track_gate(d["left"], d["right"], d["ss"], d["ts"], g0, g1)
        ctx.detection_filter(d["left"], d["right"], d["ss"], g0, g1)
        ms, n = ctx.profile_read(capi.K_STEREO_GATE)
        assert n == 4 and ms > 0
        assert ctx.profile_read(capi.K_RANSAC5)[1] == 0 and ctx.profile_read(capi.K_KLT)[1] == 0


# ---- every synchronous host-pointer entry stages through one block per context ----
ARENA_W, ARENA_H, ARENA_B, ARENA_TRAIL = 64, 48, 8, 20
# (entry, point count) in call order. The counts rise from round to round; the order is chosen so that the context's staging block,
# reserved for ONE point, grows ten times, once under every entry, and every entry also runs directly behind another entry's growth:
# round 0 grows under subpix, gate, gftt, flow, ekf, ingest; round 1 under klt, r5; round 2 under rot, filt (16-byte sections, a block
# that at least doubles). ekf: poses of a stereo track on ARENA_B filters; ingest: channels of the image; gftt: always 48 key points
ARENA_ROUNDS = [
    [("subpix", 6), ("gate", 5), ("gftt", 0), ("flow", 60), ("klt", 30), ("rot", 12), ("filt", 12), ("ekf", 2), ("ingest", 1), ("r5", 12)],
    [("klt", 250), ("subpix", 100), ("r5", 510), ("rot", 300), ("filt", 100), ("gate", 100), ("flow", 120), ("ekf", 8), ("ingest", 3), ("gftt", 0)],
    [("rot", 1000), ("filt", 1024), ("ekf", 20), ("subpix", 1000), ("r5", 1000), ("gate", 1000), ("flow", 1000), ("klt", 1000), ("ingest", 4), ("gftt", 0)],
]


def _arena_setup(ctx, left, right):
    """three built slots (left frame 0, left frame 1, right frame 0), one acquired slot for ingest, one filter batch"""
    slots = [ctx.acquire() for _ in range(4)]
    for s, img in zip(slots, (left[0], left[1], right[0])):
        ctx.build(s, img)
    return slots, capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=ARENA_TRAIL), ARENA_B)


def _arena_call(ctx, g, slots, left, right, name, n):
    """one host-pointer call on inputs that depend on (name, n) alone -> its outputs as a list of arrays"""
    rng = np.random.default_rng([sorted(("klt", "flow", "gftt", "subpix", "rot", "r5", "gate", "filt", "ekf", "ingest")).index(name), n])
    cam0 = capi.camera_model("pinhole", 60.0, 61.0, 32.0, 24.0, coeffs=(-0.25, 0.07, 0.0))
    cam1 = capi.camera_model("pinhole", 60.0, 61.0, 32.0, 24.0, coeffs=(-0.24, 0.06, 0.0))
    pts = rng.uniform([2, 2], [ARENA_W - 3, ARENA_H - 3], (max(n, 1), 2)).astype(np.float32)
    moved = (pts + [-2.0, 0.3] + rng.normal(0, 0.7, pts.shape)).astype(np.float32)
    if name == "klt":
        return list(ctx.klt_track(slots[0], slots[1], pts))
    if name == "flow":
        return list(ctx.optical_flow_compute(slots[0], slots[2], pts, corners=moved))
    if name == "gftt":
        return [ctx.gftt_detect(slots[0], params=capi.gftt_default_params(gfttMinDistance=8.0))]
    if name == "subpix":
        return list(ctx.corner_subpix(slots[1], pts))
    if name == "rot":
        st, R, best, visited = ctx.rot_ransac(pts, moved, cam0, cam1, rng.integers(0, n, (100, 2)), 4e-4)
        return [st, R, np.array([best, visited])]
    if name == "r5":
        return list(ctx.ransac5(pts, moved, cam0, cam1))
    gp = capi.stereo_gate_default_params(partOfImageToDetectFeatures=0.9, cam0ToCam1=_transforms()["rotated_vertical"])
    if name == "gate":
        return [ctx.track_gate(pts, moved, rng.integers(0, 3, n), rng.choice([0, 2, 4], n), cam0, cam1, blacklist=rng.random(n) < 0.1, params=gp)]
    if name == "filt":
        kept, kept_second, st = ctx.detection_filter(pts, moved, rng.integers(0, 3, n), cam0, cam1, params=gp)
        return [kept, kept_second, st]
    if name == "ingest":
        planes = [left[0], right[0], left[1], right[1]][:n]
        ctx.ingest_build(slots[3], planes[0] if n == 1 else np.stack(planes, -1))
        return list(ctx.download(slots[3], 0))
    assert name == "ekf"
    T1, T2, means, idx, feat = synth.visual_tracks(rng, ARENA_B, ARENA_TRAIL, n, True)
    for b in range(ARENA_B):
        g.set_state(b, means[b], np.eye(g.n) * 1e-4)
    y = feat.reshape(ARENA_B, -1) + 1e-3 * rng.normal(size=(ARENA_B, feat.shape[1] * 2))
    out = list(g.visual_track(capi.vu_default_params(imu_to_camera=T1, second_imu_to_camera=T2), idx, feat, np.zeros_like(feat), y, 1.5, 0.05))
    return out + [a for b in range(ARENA_B) for a in g.get_state(b)]


def test_host_pointer_entries_share_one_growing_staging_block():
    """hv_ingest_build, hv_klt_track, hv_optical_flow_compute, hv_gftt_detect, hv_corner_subpix, hv_rot_ransac, hv_ransac5,
    hv_track_gate, hv_detection_filter and hv_ekf_visual_track carve their device staging out of ONE block of the context that
    grows under them. Interleaved on one context over three rounds of rising point counts (ARENA_ROUNDS), every call returns, bit
    for bit, what the same call returns on a fresh context that has made no other staging call: a section that is mis-sized,
    mis-aligned or reused too early would show here. No tolerance, nothing skipped."""
    left, right, _ = synth.stereo_sequence(31, ARENA_W, ARENA_H, 2)
    kw = dict(width=ARENA_W, height=ARENA_H, levels=1, pool_size=4, max_tracks=1)
    assert all(sorted(e for e, _ in rnd) == sorted(e for e, _ in ARENA_ROUNDS[0]) and len(rnd) == 10 for rnd in ARENA_ROUNDS)
    with capi.Context(**kw) as ctx:
        slots, g = _arena_setup(ctx, left, right)
        for r, rnd in enumerate(ARENA_ROUNDS):
            for name, n in rnd:
                got = _arena_call(ctx, g, slots, left, right, name, n)
                with capi.Context(**kw) as ctx2:
                    slots2, g2 = _arena_setup(ctx2, left, right)
                    want = _arena_call(ctx2, g2, slots2, left, right, name, n)
                    g2.close()
                assert len(got) == len(want) > 0
                for k, (a, b) in enumerate(zip(got, want)):
                    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
                    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (r, name, n, k)
        g.close()
