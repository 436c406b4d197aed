"""GPU tests of the device detect() tail (hv_apply_min_distance_batch_dev, hv_gftt_corners_batch_dev, hv_gftt_detect_batch_dev).
Every comparison is np.array_equal against the CPU oracle (oracle.apply_min_distance / oracle.gftt_detect), per set: the same
points in the same order with the same count."""
import math

import numpy as np
import pytest

import test_gpu_tracker_closed_loop as CL
from hybvio_amd import capi, synth

pytestmark = pytest.mark.gpu

CORNER_COUNTS = (0, 1, 63, 64, 65, 129, 700)
PREV_COUNTS = (0, 1, 200)
RADII = (0, 2, 8, 20, 50)
MAX_CORNERS, MAX_PREV = 700, 200


def _dev(x, dt=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x if dt is None else np.asarray(x, dt))).cuda()


# ---- a. hv_apply_min_distance_batch_dev on ragged sets ----
def _make_list_sets():
    """One set per (corner count, live-track count, radius): sub-pixel coordinates at a density where the filter both keeps and
    rejects, a tenth of the corners duplicates of earlier ones, and boundary content: for a third of the corners either the
    corner itself sits at c_j + r (cos t, sin t) of an earlier corner j, or a live track sits at c + r (cos t, sin t), rounded to
    binary32. Returns the sets and the boundary pairs (a, b, r)."""
    rng = np.random.default_rng(20261017)
    sets, pairs = [], []
    for n in CORNER_COUNTS:
        for p in PREV_COUNTS:
            for r in RADII:
                side = max(24.0, 0.8 * max(r, 2) * math.sqrt(max(n, 1)))
                c = rng.uniform(0, side, (n, 2)).astype(np.float32)
                pv = rng.uniform(0, side, (p, 2)).astype(np.float32)
                free_prev = list(range(p))
                for k in range(1, n):
                    u = rng.random()
                    if u < 0.1:
                        c[k] = c[rng.integers(0, k)]
                    elif u < 0.43 and r > 0:
                        t = rng.uniform(0, 2 * math.pi)
                        off = np.array([r * math.cos(t), r * math.sin(t)])
                        if free_prev and rng.random() < 0.4:
                            i = free_prev.pop()
                            pv[i] = (c[k].astype(np.float64) + off).astype(np.float32)
                            pairs.append((pv[i].copy(), c[k].copy(), r))
                        else:
                            j = rng.integers(0, k)
                            c[k] = (c[j].astype(np.float64) + off).astype(np.float32)
                            pairs.append((c[j].copy(), c[k].copy(), r))
                sets.append(dict(c=c, pv=pv, r=r))
    return sets, pairs


def _d2(a, b, form):
    """squared distance of binary32 points in binary32: form 0 = two rounded products and one rounded sum (the reference),
    1 / 2 = fma(dx, dx, dy * dy) / fma(dy, dy, dx * dx), emulated in binary64 (a 24 x 24 bit product is exact there)"""
    d = (a.astype(np.float32) - b.astype(np.float32)).astype(np.float32)
    dx, dy = d[..., 0], d[..., 1]
    if form == 0:
        return ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32)
    if form == 2:
        dx, dy = dy, dx
    return (dx.astype(np.float64) * dx.astype(np.float64) + (dy * dy).astype(np.float32).astype(np.float64)).astype(np.float32)


def _greedy(c, pv, r, max_tracks, form):
    """applyMinDistance restated (feature_detector_legacy.cpp:177-213) with a selectable distance expression"""
    kept = np.zeros((0, 2), np.float32)
    r2 = np.float32(r * r)
    for k in range(len(c)):
        near = False
        if r > 0:
            near = bool((_d2(pv, c[k], form) < r2).any()) or bool((_d2(kept, c[k], form) < r2).any())
        if not near:
            kept = np.concatenate([kept, c[k:k + 1]])
        if len(kept) >= max_tracks:
            break
    return kept


@pytest.fixture(scope="module")
def list_sets():
    return _make_list_sets()


def test_list_sets_discriminate_contracted_distance_forms(oracle, list_sets):
    """Condition on the input of the next test, computed with numpy: the greedy evaluated with either contracted form of the
    distance gives a kept list different from the oracle's on at least 3 sets, and at least 20 boundary pairs have d2 == r2
    exactly (where `<` against `<=` decides)."""
    sets, pairs = list_sets
    a, b, r = (np.array([p[i] for p in pairs]) for i in range(3))
    exact = int((_d2(a, b, 0) == (r * r).astype(np.float32)).sum())
    flips = int(((_d2(a, b, 0) < (r * r).astype(np.float32)) != (_d2(a, b, 1) < (r * r).astype(np.float32))).sum())
    differ = [0, 0]
    for d in sets:
        want = oracle.apply_min_distance(d["c"], d["pv"], d["r"], 200)
        if d["r"] > 0 and len(d["c"]) <= 129:
            assert np.array_equal(_greedy(d["c"], d["pv"], d["r"], 200, 0), want)      # the restatement itself
        for f in (1, 2):
            differ[f - 1] += not np.array_equal(_greedy(d["c"], d["pv"], d["r"], 200, f), want)
    print(f"boundary pairs {len(pairs)}, d2 == r2 on {exact}, verdict flips under fma {flips}, sets differing {differ}")
    assert exact >= 20 and len(pairs) >= 2000
    assert min(differ) >= 3                                    # at least 3 sets under EITHER contracted form
    # a kept list can only change where a verdict flips, and "a few thousand boundary pairs" at a flip rate of about one in a
    # hundred (2 .. 3 in a hundred at r = 8 / 20 / 50, fewer at r = 2) must give some tens of flips: as many as the exact pairs asked for
    assert flips >= 20


@pytest.mark.parametrize("max_tracks", [1, 30, 200])
def test_apply_min_distance_batch_dev_equals_the_oracle(oracle, list_sets, max_tracks):
    import torch
    sets, _ = list_sets
    S = len(sets)
    corners = np.full((S, MAX_CORNERS, 2), -3.0, np.float32)
    prev = np.full((S, MAX_PREV, 2), 1e6, np.float32)
    nc, npv, rad = (np.array([len(d["c"]) for d in sets], np.int32), np.array([len(d["pv"]) for d in sets], np.int32),
                    np.array([d["r"] for d in sets], np.int32))
    for s, d in enumerate(sets):
        corners[s, :nc[s]], prev[s, :npv[s]] = d["c"], d["pv"]
    with capi.Context(width=64, height=64, pool_size=1) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        d_c, d_nc, d_p, d_np, d_r = _dev(corners), _dev(nc), _dev(prev), _dev(npv), _dev(rad)
        d_no = torch.full((S,), -9, dtype=torch.int32, device="cuda")
        ctx.apply_min_distance_batch_dev(S, MAX_CORNERS, d_nc.data_ptr(), d_c.data_ptr(), MAX_PREV, d_np.data_ptr(), d_p.data_ptr(),
                                         d_r.data_ptr(), max_tracks, d_no.data_ptr())
        torch.cuda.synchronize()
        got, no = d_c.cpu().numpy(), d_no.cpu().numpy()
        # no live tracks at all: NULL arrays with max_prev == 0
        sel = np.flatnonzero(npv == 0)
        d_c0, d_no0 = _dev(corners[sel]), torch.full((len(sel),), -9, dtype=torch.int32, device="cuda")
        d_nc0, d_r0 = _dev(nc[sel]), _dev(rad[sel])
        ctx.apply_min_distance_batch_dev(len(sel), MAX_CORNERS, d_nc0.data_ptr(), d_c0.data_ptr(), 0, 0, 0, d_r0.data_ptr(),
                                         max_tracks, d_no0.data_ptr())
        torch.cuda.synchronize()
        got0, no0 = d_c0.cpu().numpy(), d_no0.cpu().numpy()
    stopped_early = rejected = 0
    for s, d in enumerate(sets):
        want = oracle.apply_min_distance(d["c"], d["pv"], d["r"], max_tracks)
        assert no[s] == len(want) and np.array_equal(got[s, :no[s]], want), (s, nc[s], npv[s], rad[s])
        stopped_early += len(want) == max_tracks and nc[s] > max_tracks
        rejected += d["r"] > 0 and len(want) < min(nc[s], max_tracks)
    for k, s in enumerate(sel):
        want = oracle.apply_min_distance(sets[s]["c"], sets[s]["pv"], sets[s]["r"], max_tracks)
        assert no0[k] == len(want) and np.array_equal(got0[k, :no0[k]], want), s
    assert stopped_early >= 5 and rejected >= 10, (stopped_early, rejected)


# ---- b. hv_gftt_detect_batch_dev / hv_gftt_corners_batch_dev ----
def _periodic(h, w, bs, seed):
    tile = np.random.default_rng(seed).integers(0, 256, (bs, bs)).astype(np.uint8)
    return np.tile(tile, (h // bs + 1, w // bs + 1))[:h, :w].copy()


def _detect_cases(h, w, min_dist, many=False):
    """(image, live tracks, radius) per set"""
    rng = np.random.default_rng(h * 1000 + w)
    bs = 32 if min_dist >= 32 else 16 if min_dist >= 16 else 8
    tex = rng.integers(0, 256, (h, w)).astype(np.uint8)
    smooth = synth.render(synth.Texture.make(h + w), w, h, synth.Warp.make(3.0, 1.5, -2.0, w / 2, h / 2), noise_seed=5, noise_sigma=2.0)
    flat = np.full((h, w), 93, np.uint8)
    pts = lambda n: rng.uniform([0, 0], [w, h], (n, 2)).astype(np.float32)
    none = np.zeros((0, 2), np.float32)
    if many:
        base = [(tex, pts(9), 8), (smooth, none, 8), (_periodic(h, w, bs, 3), pts(3), 5), (flat, none, 8), (tex, pts(20), 0),
                (smooth, pts(30), 12), (flat, np.array([[3.0, 4.5]], np.float32), 8)]
        return [base[i % len(base)] for i in range(300)]
    n_live = 150 if h * w > 100000 else 25
    return [(tex, pts(n_live), min_dist), (smooth, pts(n_live), min_dist), (smooth, none, min_dist),
            (_periodic(h, w, bs, 1), none, min_dist), (_periodic(h, w, bs, 2), pts(4), max(min_dist // 2, 1)),
            (flat, none, min_dist), (flat, pts(5) * 0 + np.array([min_dist * 0.6, min_dist * 0.6], np.float32), min_dist),
            (flat, pts(5) * 0 + np.array([min_dist * 0.8, min_dist * 0.8], np.float32), min_dist),
            (tex, pts(n_live), 0), (smooth, pts(n_live), 1)]


def _run_detect(ctx, slots, cases, gp, max_corners=None, corners_only_from=None):
    """-> (corner lists per set, kp by-product as numpy, raw n_out)"""
    import torch
    S = len(cases)
    nk = ctx.gftt_keypoint_count(gp)
    mc = 2 * nk if max_corners is None else max_corners
    mp = max(max(len(c[1]) for c in cases), 1)
    prev = np.zeros((S, mp, 2), np.float32)
    for s, c in enumerate(cases):
        prev[s, :len(c[1])] = c[1]
    d_sl, d_p = _dev(np.array(slots, np.int32)), _dev(prev)
    d_np, d_r = _dev(np.array([len(c[1]) for c in cases], np.int32)), _dev(np.array([c[2] for c in cases], np.int32))
    d_c = torch.full((S, max(mc, 1), 2), -5.0, dtype=torch.float32, device="cuda")
    d_no = torch.full((S,), -9, dtype=torch.int32, device="cuda")
    if corners_only_from is None:
        d_kp = torch.full((S, nk, 3), -7.0, dtype=torch.float32, device="cuda")
        ctx.gftt_detect_batch_dev(S, d_sl.data_ptr(), d_kp.data_ptr(), mp, d_np.data_ptr(), d_p.data_ptr(), d_r.data_ptr(), mc,
                                  d_c.data_ptr(), d_no.data_ptr(), params=gp)
    else:
        d_kp = _dev(corners_only_from)
        ctx.gftt_corners_batch_dev(S, d_kp.data_ptr(), mp, d_np.data_ptr(), d_p.data_ptr(), d_r.data_ptr(), mc, d_c.data_ptr(),
                                   d_no.data_ptr(), params=gp)
    torch.cuda.synchronize()
    c, no = d_c.cpu().numpy(), d_no.cpu().numpy()
    return [c[s, :max(no[s], 0)].copy() for s in range(S)], d_kp.cpu().numpy(), no


def _oracle_detect(oracle, case, min_dist, max_tracks):
    img, pv, r = case
    return oracle.gftt_detect(img, prev=pv, mask_radius=r, min_distance=float(min_dist), max_tracks=max_tracks)


def _built(ctx, cases):
    import torch
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    slots, by_image = [], {}
    for img, _, _ in cases:
        if id(img) not in by_image:
            by_image[id(img)] = ctx.acquire()
            ctx.build(by_image[id(img)], img)
        slots.append(by_image[id(img)])
    return slots


# (256, 256) and (264, 256) at block edge 8: 1024 and 1056 key points, the two sides of the rank sort / bitonic network threshold
@pytest.mark.parametrize("h,w,min_dist", [(64, 64, 8), (97, 130, 20), (96, 160, 50), (480, 752, 8), (256, 256, 8), (264, 256, 8)])
def test_gftt_detect_batch_dev_equals_the_oracle(oracle, h, w, min_dist):
    cases = _detect_cases(h, w, min_dist)
    with capi.Context(width=w, height=h, pool_size=8) as ctx:
        slots = _built(ctx, cases)
        ctx.profile_enable(True)
        for max_tracks in (1, 30, 200):
            gp = capi.gftt_default_params(gfttMinDistance=float(min_dist), maxTracks=max_tracks)
            nk = ctx.gftt_keypoint_count(gp)
            ctx.profile_reset()
            got, kp, no = _run_detect(ctx, slots, cases, gp)
            again, kp2, no2 = _run_detect(ctx, slots, cases, gp)                           # e. repeatable bit for bit
            assert ctx.profile_read(capi.K_DETECT_TAIL)[1] == 2 and ctx.profile_read(capi.K_GFTT)[1] == 2
            only, _, no3 = _run_detect(ctx, slots, cases, gp, corners_only_from=kp)        # the tail alone on the by-product
            ms, launches = ctx.profile_read(capi.K_DETECT_TAIL)
            assert launches == 3 and ms > 0 and ctx.profile_read(capi.K_GFTT)[1] == 2
            assert np.array_equal(no, no2) and np.array_equal(no, no3) and kp.tobytes() == kp2.tobytes()
            for s, case in enumerate(cases):
                want = _oracle_detect(oracle, case, min_dist, max_tracks)
                assert no[s] == len(want) and np.array_equal(got[s], want), (s, max_tracks, no[s], len(want))
                assert got[s].tobytes() == again[s].tobytes() == only[s].tobytes()
            # what the cases are there for
            assert no[5] == 1 and np.array_equal(got[5], np.zeros((1, 2), np.float32))     # flat: the single (0, 0)
            assert no[6] == 0                                                              # ... rejected by a live track near the origin
            assert no[7] == (0 if 2 * (0.8 * min_dist) ** 2 < min_dist ** 2 else 1)
            assert no[8] == 2 * nk and not got[8][:nk].any()                               # radius 0: zero prefix, no cap (maxTracks 1 is below it)
            # periodic image: every block whose 5 x 5 neighbourhoods stay inside the image has the same response, so the stable
            # order decides among at least the interior blocks
            bs = capi.lib().hv_gftt_block_size(gp)
            ties = np.unique(kp[3, :, 2], return_counts=True)[1]
            assert ties.max() >= max((w // bs - 2) * (h // bs - 2), 3) and len(ties) < nk, ties
            assert (kp[5, :, 2] == np.float32(-1e10)).all()                                # flat: every block empty
            if max_tracks == 30 and nk > 40:
                assert (no[:5] == 30).any()                                                # the cap stopped a scan


def test_gftt_detect_batch_dev_more_workgroups_than_cus(oracle):
    """300 images of 64 x 64 in one call"""
    cases = _detect_cases(64, 64, 8, many=True)
    gp = capi.gftt_default_params(gfttMinDistance=8.0, maxTracks=30)
    with capi.Context(width=64, height=64, pool_size=8) as ctx:
        slots = _built(ctx, cases)
        got, kp, no = _run_detect(ctx, slots, cases, gp)
    want = [_oracle_detect(oracle, c, 8, 30) for c in cases[:7]]
    for s in range(300):
        assert no[s] == len(want[s % 7]) and np.array_equal(got[s], want[s % 7]), s


def test_gftt_corners_capacity_rule():
    """max_corners >= min(maxTracks, 2 nk) is required; below 2 nk a set with radius <= 0 reports n_out = -1 and writes nothing,
    the other sets of the launch are served."""
    import torch
    cases = _detect_cases(64, 64, 8)
    gp = capi.gftt_default_params(gfttMinDistance=8.0, maxTracks=30)
    with capi.Context(width=64, height=64, pool_size=8) as ctx:
        slots = _built(ctx, cases)
        full, kp, no_full = _run_detect(ctx, slots, cases, gp)
        small, _, no = _run_detect(ctx, slots, cases, gp, max_corners=30)
        assert no[8] == -1 and no_full[8] == 128
        for s in range(len(cases)):
            if s != 8:
                assert no[s] == no_full[s] and np.array_equal(small[s], full[s])
        d = torch.zeros(4096, dtype=torch.float32, device="cuda")
        i = torch.zeros(64, dtype=torch.int32, device="cuda")
        with pytest.raises(capi.HvError):
            ctx.gftt_corners_batch_dev(1, d.data_ptr(), 0, 0, 0, i.data_ptr(), 29, d.data_ptr(), i.data_ptr(), params=gp)


def test_more_key_points_than_the_limit_is_unsupported():
    """1280 x 1040 at block edge 8 is 20 800 key points, above HV_DETECT_TAIL_MAX_KEYPOINTS: both entries refuse with
    HV_ERR_UNSUPPORTED once they have the context, before anything is launched; block edge 32 on the same context is served."""
    import torch
    w, h = 1280, 1040
    gp8, gp32 = capi.gftt_default_params(gfttMinDistance=8.0), capi.gftt_default_params(gfttMinDistance=50.0)
    with capi.Context(width=w, height=h, pool_size=1, levels=1) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        nk8, nk32 = ctx.gftt_keypoint_count(gp8), ctx.gftt_keypoint_count(gp32)
        assert nk8 == 20800 > capi.DETECT_TAIL_MAX_KEYPOINTS >= nk32
        slot = ctx.acquire()
        ctx.build(slot, np.random.default_rng(1).integers(0, 256, (h, w)).astype(np.uint8))
        d_sl, d_r = _dev(np.array([slot], np.int32)), _dev(np.array([8], np.int32))
        d_kp = torch.zeros((1, nk8, 3), dtype=torch.float32, device="cuda")
        d_c = torch.full((1, 200, 2), -5.0, dtype=torch.float32, device="cuda")
        d_n = torch.full((1,), -9, dtype=torch.int32, device="cuda")
        L, P = capi.lib(), lambda t: t.data_ptr()
        assert L.hv_gftt_detect_batch_dev(ctx._h, gp8, 1, P(d_sl), P(d_kp), 0, None, None, P(d_r), 200, P(d_c), P(d_n)) == -2
        assert L.hv_gftt_corners_batch_dev(ctx._h, gp8, 1, P(d_kp), 0, None, None, P(d_r), 200, P(d_c), P(d_n)) == -2
        torch.cuda.synchronize()
        assert int(d_n.item()) == -9 and not d_kp.any() and (d_c == -5.0).all()           # nothing ran
        ctx.gftt_detect_batch_dev(1, P(d_sl), P(d_kp), 0, 0, 0, P(d_r), 200, P(d_c), P(d_n), params=gp32)
        torch.cuda.synchronize()
        assert 0 < int(d_n.item()) <= 200


# ---- c. the detection chain with no host step ----
def test_detection_chain_without_a_host_step_eager_and_graph(oracle):
    """hv_gftt_detect_batch_dev -> hv_corner_subpix_batch_dev -> stereo hv_klt_track_batch_ragged_dev -> hv_flow_status_batch_dev
    -> hv_detection_filter_batch_dev, eagerly and captured in a graph replayed twice: counts and compacted pairs equal the same
    chain started from per-image hv_gftt_detect."""
    import torch
    W, H, S, M, R = 752, 480, 3, 400, 50
    cam_args, radial = CL.cam_args(W, H)
    gcam = capi.camera_model(*cam_args, coeffs=radial)
    T = np.eye(4)
    T[:3, 3] = (-0.1, 0.01, 0.0)
    sg = capi.stereo_gate_default_params(partOfImageToDetectFeatures=0.9, cam0ToCam1=T)
    gp = capi.gftt_default_params(maxTracks=M)
    left, right, _ = synth.stereo_sequence(90, W, H, S)
    with capi.Context(width=W, height=H, pool_size=2 * S, max_tracks=M) as ctx:
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        ls = [ctx.acquire() for _ in range(S)]; rs = [ctx.acquire() for _ in range(S)]
        nk = ctx.gftt_keypoint_count(gp)
        masks, radii = [], [R, 30, 40]
        for s in range(S):
            ctx.build(ls[s], left[s]); ctx.build(rs[s], right[s])
            before = ctx.gftt_detect(ls[s], mask_radius=R, params=gp)                      # a previous detection
            masks.append((before[1:120:2] + np.float32([0.37, -0.21])).astype(np.float32))  # half of its corners are live tracks
        mp = max(len(m) for m in masks)
        prev = np.zeros((S, mp, 2), np.float32)
        host_c, host_n = np.zeros((S, M, 2), np.float32), np.zeros(S, np.int32)
        for s in range(S):
            prev[s, :len(masks[s])] = masks[s]
            c = ctx.gftt_detect(ls[s], prev=masks[s], mask_radius=radii[s], params=gp)
            host_c[s, :len(c)], host_n[s] = c, len(c)
        assert (host_n > 30).all() and (host_n < M).all()
        with torch.cuda.stream(stream):
            d_l, d_r = _dev(np.array(ls, np.int32)), _dev(np.array(rs, np.int32))
            d_p, d_np, d_rad = _dev(prev), _dev(np.array([len(m) for m in masks], np.int32)), _dev(np.array(radii, np.int32))
            d_kp = torch.zeros((S, nk, 3), dtype=torch.float32, device="cuda")
            d_c = torch.zeros((S, M, 2), dtype=torch.float32, device="cuda"); d_n = torch.zeros(S, dtype=torch.int32, device="cuda")
            d_right = torch.zeros_like(d_c); d_lk = torch.zeros((S, M), dtype=torch.uint8, device="cuda")
            d_ss = torch.zeros((S, M), dtype=torch.int32, device="cuda")
            d_ol = torch.zeros_like(d_c); d_or = torch.zeros_like(d_c); d_no = torch.zeros(S, dtype=torch.int32, device="cuda")
        outs = (d_c, d_n, d_right, d_lk, d_ss, d_ol, d_or, d_no)

        def tail_of_chain():
            ctx.corner_subpix_batch_dev(S, d_l.data_ptr(), M, d_n.data_ptr(), d_c.data_ptr())
            ctx.klt_track_batch_ragged_dev(S, d_l.data_ptr(), d_r.data_ptr(), M, d_n.data_ptr(), d_c.data_ptr(), d_right.data_ptr(),
                                           d_lk.data_ptr(), 0, use_initial_flow=False)
            ctx.flow_status_batch_dev(S, M, d_n.data_ptr(), d_right.data_ptr(), d_lk.data_ptr(), d_ss.data_ptr())
            ctx.detection_filter_batch_dev(S, M, d_n.data_ptr(), d_c.data_ptr(), d_right.data_ptr(), d_ss.data_ptr(), gcam, gcam, 0,
                                           d_ol.data_ptr(), d_or.data_ptr(), d_no.data_ptr(), params=sg)

        def chain():
            ctx.gftt_detect_batch_dev(S, d_l.data_ptr(), d_kp.data_ptr(), mp, d_np.data_ptr(), d_p.data_ptr(), d_rad.data_ptr(), M,
                                      d_c.data_ptr(), d_n.data_ptr(), params=gp)
            tail_of_chain()

        def clear():
            with torch.cuda.stream(stream):
                for t in outs:
                    t.zero_()

        def result():
            stream.synchronize()
            n, no = d_n.cpu().numpy(), d_no.cpu().numpy()
            ol, orr = d_ol.cpu().numpy(), d_or.cpu().numpy()
            return n.copy(), no.copy(), [ol[s, :no[s]].copy() for s in range(S)], [orr[s, :no[s]].copy() for s in range(S)]

        # the reference chain: per-image host detection, then the same device stages
        clear()
        with torch.cuda.stream(stream):
            d_c.copy_(_dev(host_c)); d_n.copy_(_dev(host_n))
        tail_of_chain()
        want = result()
        assert np.array_equal(want[0], host_n) and (want[1] > 0).all() and (want[1] < host_n).any()

        def check(got, what):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
            for s in range(S):
                assert np.array_equal(got[2][s], want[2][s]) and np.array_equal(got[3][s], want[3][s]), (what, s)

        clear(); chain(); check(result(), "eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            chain()
        for rep in range(2):
            clear()
            with torch.cuda.stream(stream):
                g.replay()
            check(result(), f"replay {rep}")


# ---- d. closed tracker loop with the device detection ----
class HipDeviceDetect(CL.HipBackend):
    def __init__(self, w, h, max_tracks, min_dist):
        import torch
        super().__init__(w, h, max_tracks, min_dist)
        self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        self.masked = 0

    def detect(self, handle, mask, r):
        import torch
        nk = self.ctx.gftt_keypoint_count(self.gp)
        mask = np.ascontiguousarray(mask, np.float32).reshape(-1, 2)
        self.masked += len(mask) > 0
        d_sl, d_r, d_np = _dev(np.array([handle], np.int32)), _dev(np.array([r], np.int32)), _dev(np.array([len(mask)], np.int32))
        d_p = _dev(mask if len(mask) else np.zeros((1, 2), np.float32))
        d_kp = torch.zeros((1, nk, 3), dtype=torch.float32, device="cuda")
        d_c = torch.zeros((1, 2 * nk, 2), dtype=torch.float32, device="cuda"); d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.ctx.gftt_detect_batch_dev(1, d_sl.data_ptr(), d_kp.data_ptr(), max(len(mask), 1), d_np.data_ptr(), d_p.data_ptr(),
                                       d_r.data_ptr(), 2 * nk, d_c.data_ptr(), d_n.data_ptr(), params=self.gp)
        torch.cuda.synchronize()
        return d_c[0, :int(d_n.item())].cpu().numpy()


def test_closed_loop_with_device_detection_identical_to_the_oracle(oracle):
    w, h, max_tracks, min_dist, unique, frames = 256, 192, 60, 16, 15, 30
    left, right = CL.moving_sequence(77, w, h, unique, frames, radius=0.5 * unique, rot=1.2)
    hip = HipDeviceDetect(w, h, max_tracks, min_dist)
    try:
        got, pos_hip = CL.run_tracker(hip, oracle, left, right, w, h, max_tracks, min_dist)
    finally:
        hip.ctx.close()
    ref, pos_ref = CL.run_tracker(CL.OracleBackend(oracle, w, h, max_tracks, min_dist), oracle, left, right, w, h, max_tracks, min_dist)
    for f, ((gi, gl, gr, gs), (oi, ol, orr, os_)) in enumerate(zip(got, ref)):
        np.testing.assert_array_equal(gs, os_, err_msg=f"frame {f}: status")
        np.testing.assert_array_equal(gi, oi, err_msg=f"frame {f}: track ids")
        np.testing.assert_array_equal(gl, ol, err_msg=f"frame {f}: left positions")
        np.testing.assert_array_equal(gr, orr, err_msg=f"frame {f}: right positions")
    assert pos_hip == pos_ref and len(got) == frames
    assert hip.masked >= 1 and len(got[-1][0]) >= max_tracks // 2, (hip.masked, len(got[-1][0]))
