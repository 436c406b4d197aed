"""GPU tests of the stereo upright 2-point filter (hv_upright2p*) against the numpy restatement tests/upright2p_restatement.py.

Corpus: 422 synthetic stereo sets (the rig, points, noise and outliers of the RANSAC3 corpus) on a pinhole, a radially
distorted pinhole and a fisheye camera; n in {0, 1, 2, 3, 5, 20, 64, 65, 200, 257} and two sets of 1024, 0-75 % outliers,
0-0.5 px noise; sets of 20 or more features carry non-TRACKED entries, features whose triangulation is rejected and
(fisheye) features outside the valid field of view. The previous camera attitude cycles through general, optical axis
along +z / -z of the world and horizontal; the current rotation handed to the filter carries a yaw error drawn from
(-pi, pi) and, on every second set, a tilt error of 0.1 degree.

Figures of the restatement alone on this corpus (CPU, before any GPU run: branches reached, truth recovered, agreement,
sensitivity to one ulp on every normalised coordinate) are in profiles/upright2p/README.md.
"""
import math

import numpy as np
import pytest

import ransac5_restatement as R5
import upright2p_restatement as U
from hybvio_amd import capi

pytestmark = pytest.mark.gpu
NS = [0, 1, 2, 3, 5, 20, 64, 65, 200, 257]
CELLS = [(0.0, 0.0), (0.2, 0.0), (0.4, 0.0), (0.6, 0.0), (0.75, 0.0), (0.0, 0.25), (0.2, 0.25), (0.4, 0.25), (0.6, 0.25),
         (0.0, 0.5), (0.2, 0.5), (0.4, 0.5), (0.6, 0.5), (0.75, 0.5)]                    # (outliers, noise px), as the RANSAC3 test
T = U.SECOND_TO_FIRST
CAP = 98                                                                                 # the first iteration limit with the defaults


def _cams(oracle, name):
    spec = R5.CAMERAS[name]
    o = oracle.Camera(spec[0], *spec[1:5], coeffs=spec[5], max_valid_fov_deg=spec[6])
    g = capi.camera_model(spec[0], *spec[1:5], coeffs=spec[5], max_valid_fov_deg=spec[6])
    return o, g


def _make(rng, oracle, ocam, name, n, outl, noise, seed, kind="general", tilt=0.0):
    extra = (3, 2, 2 if name == "fisheye" else 0) if 20 <= n < 1024 else (0, 0, 0)
    d = U.make_set(rng, ocam, n - sum(extra), outl, noise, *extra, kind=kind, psi=rng.uniform(-math.pi, math.pi), tilt_deg=tilt)
    d.update(cam=name, n=n, outl=outl, noise=noise, kind=kind, tilt=tilt, draws=oracle.mt19937_draws(seed, 2 * U.MAX_ITERS))
    return d


def _reference(d, ocam, params=None, perturb=None):
    ts, done, cnt, model, summ = U.do_upright2p(d["status"], d["prev_left"], d["prev_right"], d["cur_left"], ocam, ocam, T, d["poses"],
                                                d["draws"], params, perturb)
    return ts, model, summ


def build_sets(oracle):
    """The corpus without its GPU results: [(camera name, max_points, sets)], every set with its restatement result `ref`."""
    rng = np.random.default_rng(2027)
    groups, count = [], 0
    for name in R5.CAMERAS:
        ocam, _ = _cams(oracle, name)
        sets = []
        for i, (outl, noise) in enumerate(CELLS):
            for k, n in enumerate(NS):
                q = len(sets)
                sets.append(_make(rng, oracle, ocam, name, n, outl, noise, 1000 + count + q, U.ATTITUDES[(i + k) % 4], 0.1 * ((i + k // 4) % 2)))
        count += len(sets)
        groups.append((name, 257, sets))
    ocam, _ = _cams(oracle, "pinhole_radial")
    groups.append(("pinhole_radial", 1024, [_make(rng, oracle, ocam, "pinhole_radial", 1024, outl, 0.25, 77 + i, "general", 0.1 * i)
                                            for i, outl in enumerate((0.2, 0.6))]))
    for name, _, sets in groups:
        ocam, _ = _cams(oracle, name)
        for d in sets:
            d["ref"] = _reference(d, ocam)
    return groups


def _pack(sets, max_points, max_iters=U.MAX_ITERS):
    S = len(sets)
    xy = np.zeros((3, S, max_points, 2), np.float32)
    st = np.full((S, max_points), -9, np.int32)
    cnt = np.zeros(S, np.int32)
    for s, d in enumerate(sets):
        n = len(d["status"])
        xy[0, s, :n], xy[1, s, :n], xy[2, s, :n], st[s, :n], cnt[s] = d["prev_left"], d["prev_right"], d["cur_left"], d["status"], n
    draws = np.stack([d["draws"][:2 * max_iters] for d in sets])           # [sets][2 * MaxIterations]
    poses = np.stack([d["poses"] for d in sets])
    return xy, st, cnt, draws, poses


def _run_batch(ctx, sets, gcam, max_points=257, params=None):
    import torch
    xy, st, cnt, draws, poses = _pack(sets, max_points, params.ransacStereoUpright2pMaxIterations if params is not None else U.MAX_ITERS)
    S = len(sets)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_xy, d_st, d_n, d_dr, d_po = dev(xy), dev(st), dev(cnt), dev(draws), dev(poses)
    d_model = torch.full((S, 12), 7.0, dtype=torch.float64, device="cuda")
    d_sm = torch.full((S, 4), -5, dtype=torch.int32, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.upright2p_batch_dev(S, max_points, d_n.data_ptr(), d_xy[0].data_ptr(), d_xy[1].data_ptr(), d_xy[2].data_ptr(), gcam, gcam, T,
                            d_po.data_ptr(), d_dr.data_ptr(), d_st.data_ptr(), d_model.data_ptr(), d_sm.data_ptr(), params=params)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_model.cpu().numpy(), d_sm.cpu().numpy()


@pytest.fixture(scope="module")
def corpus(oracle):
    out = []
    with capi.Context(width=752, height=480) as ctx:
        for name, mp, sets in build_sets(oracle):
            _, gcam = _cams(oracle, name)
            st, model, sm = _run_batch(ctx, sets, gcam, mp)
            for s, d in enumerate(sets):
                d["gpu"] = (st[s, :d["n"]], model[s], sm[s].tolist())
                assert (st[s, d["n"]:] == -9).all()                                  # padding untouched
            out += sets
    return out


def _same(d):
    (sg, pg, mg), (sr, pr, mr) = d["gpu"], d["ref"]
    return np.array_equal(sg, sr) and mg == list(mr)


def well_separated(d):
    return d["n"] >= 20 and d["noise"] <= 0.5 and d["outl"] <= 0.4


def truth_recoverable(d):
    """Noise-free sets without a tilt error, of 20 and more features, whose mask must equal the ground truth exactly: every
    outlier level up to 60 %, and 75 % from 64 features on. A 20-feature set carries 13 good features at most, so at 75 %
    outliers it has 3 true inliers, and a 2-point model that fits its own two points and one more by chance cannot be told
    from the truth."""
    return d["noise"] == 0 and d["tilt"] == 0 and d["n"] >= 20 and (d["outl"] <= 0.6 or d["n"] >= 64)


def branches(corpus):
    """not run / ended at minIterations / adaptively in between / at the cap, and the compaction, by the restatement"""
    sm = np.array([d["ref"][2] for d in corpus])
    assert (sm[:, 3] < 2).any() and (sm[:, 2] == 50).any() and ((sm[:, 2] > 50) & (sm[:, 2] < CAP)).any() and (sm[:, 2] == CAP).any()
    assert (sm[:, 2] <= CAP).all() and ((sm[:, 3] < 2) == (sm[:, 2] == 0)).all()
    assert any(d["ref"][2][3] < int((d["status"] == 0).sum()) < d["n"] for d in corpus)


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
    branches(corpus)


def test_well_separated_sets_are_exact_and_near_the_truth(corpus):
    """Well-separated sets (n >= 20, noise <= 0.5 px, <= 40 % outliers): on the pinhole cameras the result is identical to
    the restatement and the model matches to 1e-9; on the noisy ones the agreement with the ground truth is at least the
    restatement's own on the same sets less one percentage point. Noise-free sets without a tilt error
    (truth_recoverable) recover the ground truth exactly."""
    ws = [d for d in corpus if well_separated(d)]
    assert len(ws) >= 130 and {d["cam"] for d in ws} == set(R5.CAMERAS)
    agree = agree_ref = total = 0
    for d in ws:
        (sg, pg, mg), (sr, pr, mr) = d["gpu"], d["ref"]
        if d["cam"] != "fisheye":
            assert np.array_equal(sg, sr) and mg == list(mr), (d["cam"], d["n"], d["outl"], d["noise"], mg, mr)
            assert np.abs(pg - pr).max() <= 1e-9
        if d["noise"] > 0:
            agree += int(((sg == 0) == d["truth"]).sum())
            agree_ref += int(((sr == 0) == d["truth"]).sum())
            total += d["n"]
    nf = [d for d in corpus if truth_recoverable(d)]
    assert len(nf) >= 30 and {d["outl"] for d in nf} == {0.0, 0.2, 0.4, 0.6, 0.75} and {d["kind"] for d in nf} == set(U.ATTITUDES)
    for d in nf:
        assert np.array_equal(d["gpu"][0] == 0, d["truth"]), (d["cam"], d["n"], d["outl"], d["kind"])
    print("noise-free sets", len(nf), "noisy agreement", agree, total, agree / total, "restatement", agree_ref / total)
    assert agree / total >= agree_ref / total - 0.01, (agree, agree_ref, total)


def test_more_sets_than_compute_units(oracle):
    ocam, gcam = _cams(oracle, "pinhole")
    rng = np.random.default_rng(9)
    sets = [_make(rng, oracle, ocam, "pinhole", 20, [0.0, 0.2, 0.4][i % 3], [0.0, 0.25][i % 2], 5000 + i, U.ATTITUDES[i % 4], 0.1 * (i % 2))
            for i in range(600)]
    with capi.Context(width=752, height=480) as ctx:
        st, model, sm = _run_batch(ctx, sets, gcam, 32)
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
    sets = [_make(rng, oracle, ocam, "pinhole_radial", n, 0.3, 0.5, 300 + n, U.ATTITUDES[n % 4], 0.1) for n in (1, 2, 3, 5, 20, 65, 200, 64)]
    S, MP = len(sets), 200
    with capi.Context(width=752, height=480) as ctx:
        sync = [ctx.upright2p(d["status"], d["prev_left"], d["prev_right"], d["cur_left"], gcam, gcam, T, d["poses"], d["draws"]) for d in sets]
        st, model, sm = _run_batch(ctx, sets, gcam, MP)
        for s, d in enumerate(sets):
            n = d["n"]
            assert np.array_equal(st[s, :n], sync[s][0]) and np.array_equal(model[s], sync[s][1]) and sm[s].tolist() == sync[s][2].tolist()
        xy, st0, cnt, draws, poses = _pack(sets, MP)
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        d_xy, d_st0, d_n, d_dr, d_po = (torch.from_numpy(x).cuda() for x in (xy, st0, cnt, draws, poses))
        d_st = torch.zeros((S, MP), dtype=torch.int32, device="cuda")
        d_model = torch.zeros((S, 12), dtype=torch.float64, device="cuda"); d_sm = torch.zeros((S, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            ctx.upright2p_batch_dev(S, MP, d_n.data_ptr(), d_xy[0].data_ptr(), d_xy[1].data_ptr(), d_xy[2].data_ptr(), gcam, gcam, T,
                                    d_po.data_ptr(), d_dr.data_ptr(), d_st.data_ptr(), d_model.data_ptr(), d_sm.data_ptr())
        for _ in range(2):
            with torch.cuda.stream(stream):
                d_st.copy_(d_st0); d_model.fill_(0); d_sm.fill_(0)
                g.replay()
            stream.synchronize()
            assert np.array_equal(d_st.cpu().numpy(), st) and np.array_equal(d_model.cpu().numpy(), model)
            assert np.array_equal(d_sm.cpu().numpy(), sm)
        del g


def test_use_mle_off_and_other_parameters_follow_the_restatement(oracle):
    ocam, gcam = _cams(oracle, "pinhole")
    rng = np.random.default_rng(21)
    sets = [_make(rng, oracle, ocam, "pinhole", n, 0.3, 0.25, 900 + n, U.ATTITUDES[n % 4]) for n in (20, 65, 200)]
    with capi.Context(width=752, height=480) as ctx:
        for kw in (dict(ransacStereoUpright2pUseMle=0), dict(ransacStereoUpright2pMinIterations=10, ransacStereoUpright2pMaxIterations=100),
                   dict(ransacStereoUpright2pMinIterations=300, ransacStereoUpright2pMaxIterations=400),      # more than one round
                   dict(ransacStereoUpright2pErrorThresh=2.5e-5)):
            st, model, sm = _run_batch(ctx, sets, gcam, params=capi.upright2p_default_params(**kw))
            for s, d in enumerate(sets):
                ts, pr, mr = _reference(d, ocam, U.Params(**kw))
                assert np.array_equal(st[s, :d["n"]], ts) and sm[s].tolist() == list(mr), (kw, d["n"], sm[s], mr)
                assert np.abs(model[s] - pr).max() <= 1e-9


EDGE_COUNTS = [0, 1, 2, 3, 63, 64, 65, 128, 129, 769, 1023, 1024]


def build_edge_sets(oracle):
    """The sets of test_compaction_and_gather_at_the_chunk_edges, every one with its restatement result `ref`."""
    ocam, _ = _cams(oracle, "pinhole_radial")
    rng = np.random.default_rng(79)
    sets = []
    for k, n in enumerate(EDGE_COUNTS):
        extra = 6 if n >= 63 else 0
        base = U.make_set(rng, ocam, n - extra, 0.2, 0.0, n_diverging=extra, kind=U.ATTITUDES[k % 4], psi=rng.uniform(-math.pi, math.pi))
        i = np.arange(n)
        for j, mask in enumerate([np.ones(n, bool), i % 2 == 0, (i % 64 == 63) | (i == 0)]):
            d = dict(base, n=n, status=np.where(mask, 0, 2).astype(np.int32), draws=oracle.mt19937_draws(7000 + 3 * k + j, 2 * U.MAX_ITERS))
            d["ref"] = _reference(d, ocam)
            sets.append(d)
    return sets


def edge_conditions(sets):
    """By the restatement alone: both outcomes (run, not run) are reached, and sets where correspondences < TRACKED features."""
    ran = {d["ref"][2][3] >= 2 for d in sets}
    moved = sum(2 <= d["ref"][2][3] < int((d["status"] == 0).sum()) for d in sets)
    assert ran == {True, False} and moved >= 10, (ran, moved)


def test_compaction_and_gather_at_the_chunk_edges(oracle):
    """The ordered compaction (TRACKED features, then correspondences) and the gather behind it at their edges: one launch of
    hv_upright2p_batch_dev with max_points = 1024, point counts around the 64-feature chunks and the 256-thread strides, and
    per count three masks: all TRACKED, every second feature, feature 0 and the last feature of every 64-feature chunk.
    Noise-free sets with 20 % outliers; counts from 63 up carry six features whose triangulation is rejected, so the gather
    moves the correspondences behind them. Every set must equal the restatement's do_upright2p, none exempted."""
    _, gcam = _cams(oracle, "pinhole_radial")
    sets = build_edge_sets(oracle)
    edge_conditions(sets)
    with capi.Context(width=752, height=480) as ctx:
        st, model, sm = _run_batch(ctx, sets, gcam, 1024)
    for s, d in enumerate(sets):
        n, (ts, pr, mr) = d["n"], d["ref"]
        print("set", s, "n", n, "tracked", int((d["status"] == 0).sum()), "summary", list(mr), "gpu", sm[s])
        assert np.array_equal(st[s, :n], ts) and (st[s, n:] == -9).all(), (s, n)
        assert sm[s].tolist() == list(mr), (s, n, sm[s], mr)
        assert np.abs(model[s] - pr).max() <= 1e-9, (s, n)


def _chain_case(oracle):
    """12 filters with distinct states and a trail of 3 poses, one 60-feature set each (sets 3 and 7: one and no TRACKED feature)."""
    import flow_predict_restatement as F
    ocam, gcam = _cams(oracle, "pinhole_radial")
    rng = np.random.default_rng(33)
    S, MP = 12, 64
    sets = [_make(rng, oracle, ocam, "pinhole_radial", 60, [0.0, 0.2, 0.4][s % 3], [0.0, 0.25][s % 2], 40 + s, U.ATTITUDES[s % 4]) for s in range(S)]
    sets[3]["status"][np.nonzero(sets[3]["status"] == 0)[0][1:]] = 2
    sets[7]["status"][:] = 2
    i2c = np.eye(4)
    i2c[:3, :3], i2c[:3, 3] = U.rotation(np.array([0.3, -0.2, 1.1])), [0.05, -0.02, 0.01]
    par = capi.flow_predict_default_params(imu_to_camera=i2c)
    cam_to_imu = [float(x) for x in np.ctypeslib.as_array(par.cameraToImu)]

    def poses_of(m):
        return np.array(F.toCameraToWorld(np.float64, m[20:23], m[23:27], cam_to_imu) + F.toCameraToWorld(np.float64, m[0:3], m[6:10], cam_to_imu))
    return ocam, gcam, rng, S, MP, sets, par, poses_of


def _random_means(rng, S, n):
    means = rng.normal(size=(S, n)) * 0.3
    for b in range(S):
        for o in (6, 23, 30, 37):
            if o + 4 <= n:
                means[b, o:o + 4] /= np.linalg.norm(means[b, o:o + 4])
    return means


def test_chain_reads_the_poses_from_the_filter_mean(oracle):
    """hv_upright2p_lk_batch_dev on a filter batch against hv_upright2p_batch_dev fed with the poses that
    flow_predict_restatement.toCameraToWorld forms from the read-back mean: eagerly, then captured behind a predict; one set
    with a non-finite mean ends SKIPPED and touches no other."""
    import torch
    ocam, gcam, rng, S, MP, sets, par, poses_of = _chain_case(oracle)
    xy, st0, cnt, draws, _ = _pack(sets, MP)
    r2s = np.zeros((S, 2), np.int32); r2s[:, 0] = [int((d["status"] == 0).sum()) // 2 for d in sets]
    with capi.Context(width=752, height=480) as ctx:
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        ekf = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=3), batch=S)
        means = _random_means(rng, S, ekf.n)
        means[5, 7] = np.nan                                              # the current orientation of filter 5
        for b in range(S):
            ekf.set_state(b, m=means[b])
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        d_xy, d_st0, d_n, d_dr, d_r2s = dev(xy), dev(st0), dev(cnt), dev(draws), dev(r2s)
        d_dt, d_gy, d_ac = dev(np.full(S, 0.005)), dev(rng.normal(size=(S, 3)) * 0.2), dev(rng.normal(size=(S, 3)) + [0, 0, 9.8])
        new = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device="cuda")
        d_st, d_res, d_score = new((S, MP), torch.int32, 0), new((S, 2), torch.int32, -1), new((S,), torch.float64, -1.0)
        d_model, d_sm = new((S, 12), torch.float64, 7.0), new((S, 4), torch.int32, -5)
        d_po = new((S, 32), torch.float64, 0.0)
        d_st2, d_model2, d_sm2 = new((S, MP), torch.int32, 0), new((S, 12), torch.float64, 7.0), new((S, 4), torch.int32, -5)

        def chain():
            ekf.upright2p_lk_batch_dev(par, MP, d_n.data_ptr(), d_xy[0].data_ptr(), d_xy[1].data_ptr(), d_xy[2].data_ptr(), d_st.data_ptr(),
                                       d_r2s.data_ptr(), gcam, gcam, T, d_dr.data_ptr(), d_res.data_ptr(), d_score.data_ptr(),
                                       d_model.data_ptr(), d_sm.data_ptr())

        def check(what):
            stream.synchronize()
            m = ekf.get_means()
            poses = np.stack([poses_of(m[b]) for b in range(S)])
            with torch.cuda.stream(stream):
                d_st2.copy_(d_st0)
                d_po.copy_(torch.from_numpy(poses))
                ctx.upright2p_batch_dev(S, MP, d_n.data_ptr(), d_xy[0].data_ptr(), d_xy[1].data_ptr(), d_xy[2].data_ptr(), gcam, gcam, T,
                                        d_po.data_ptr(), d_dr.data_ptr(), d_st2.data_ptr(), d_model2.data_ptr(), d_sm2.data_ptr())
            stream.synchronize()
            g_st, g_res, g_score, g_model, g_sm, b_st, b_model, b_sm = (t.cpu().numpy() for t in (d_st, d_res, d_score, d_model, d_sm, d_st2, d_model2, d_sm2))
            types = []
            for s, d in enumerate(sets):
                n, tracked = d["n"], int((d["status"] == 0).sum())
                done = b_sm[s, 1] >= 0
                want_st = b_st[s, :n] if done else np.full(n, 3)
                assert np.array_equal(g_st[s, :n], want_st) and (g_st[s, n:] == -9).all(), (what, s)
                assert g_res[s].tolist() == [4 if done else 0, int(b_sm[s, 0])] and g_sm[s].tolist() == b_sm[s].tolist(), (what, s, g_res[s], b_sm[s])
                assert g_score[s] == ((r2s[s, 0] if tracked >= 2 else 0) / tracked if tracked else 0.0), (what, s)
                assert np.abs(g_model[s] - b_model[s]).max() <= 1e-9, (what, s)
                types.append(int(g_res[s, 0]))
                if done:                                                   # and the batched entry itself equals the restatement
                    ts, _, summ = _reference(dict(d, poses=poses[s]), ocam)
                    assert np.array_equal(b_st[s, :n], ts) and b_sm[s].tolist() == list(summ), (what, s)
            assert [types[s] for s in (3, 5, 7)] == [0, 0, 0] and all(t == 4 for s, t in enumerate(types) if s not in (3, 5, 7)), types
            assert g_sm[5].tolist() == [0, -1, CAP, int(b_sm[5, 3])] and b_sm[5, 3] >= 2 and g_sm[7].tolist() == [0, -1, 0, 0]

        with torch.cuda.stream(stream):
            d_st.copy_(d_st0)
            chain()
        check("eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            d_st.copy_(d_st0)
            ekf.predict_dev(d_dt.data_ptr(), d_gy.data_ptr(), d_ac.data_ptr())
            chain()
        before = ekf.get_means()
        with torch.cuda.stream(stream):
            g.replay()
        check("captured behind a predict")
        assert not np.array_equal(np.nan_to_num(before), np.nan_to_num(ekf.get_means()))     # the predict ran
        del g
        ekf.close()


def test_profile_class_counts_the_launches(oracle):
    ocam, gcam = _cams(oracle, "pinhole")
    d = _make(np.random.default_rng(1), oracle, ocam, "pinhole", 50, 0.2, 0.25, 3)
    with capi.Context(width=752, height=480) as ctx:
        ctx.profile_enable(True)
        ctx.profile_reset()
        for k in range(3):
            ctx.upright2p(d["status"], d["prev_left"], d["prev_right"], d["cur_left"], gcam, gcam, T, d["poses"], d["draws"])
            assert ctx.profile_read(capi.K_RANSAC3)[1] == k + 1
        ms, n = ctx.profile_read(capi.K_RANSAC3)
        assert n == 3 and ms > 0
        assert ctx.profile_read(capi.K_RANSAC5)[1] == 0 and ctx.profile_read(capi.K_ROT_RANSAC)[1] == 0
