"""GPU tests of the kernels that take caller-supplied coordinates -- klt_kernel through every LK entry point, rot_ransac_kernel
through every rotation-RANSAC entry point -- on NaN, infinite and out-of-int-range coordinates, against the CPU oracle.

The reference converts coordinates with cvFloor / cvRound, which give INT_MIN for NaN and for every value outside int's range
(oracle/pyrlk_oracle.c cv_floor_f): such a point fails LK's window tests, status 0, and its position is the input value carried
through the levels. The device's conversion saturates and turns NaN into 0, so the kernel has to state the NaN case itself
(klt.hip, nan_in). The rotation RANSAC has no conversion: NaN is never an inlier, on both sides.

Bars: LK statuses, Feature::Status, err and positions identical to the oracle's (bits where the oracle's position is not NaN, NaN
where it is); RANSAC statuses, counts and the bits of R identical for the pinhole models (NaN where the oracle's R is NaN), the
fisheye model as in test_gpu_rot_ransac.py. No point is skipped. Shapes are the smallest that hold the cases: a 101 x 70 image, 103
points per call (specials at indices 0, 63, 64 and the last: both ends of a wavefront's worth of workgroups), <= 7 RANSAC sets."""
import numpy as np
import pytest

import stereo_gate_restatement as G
import track_table_restatement as T
from hybvio_amd import capi, synth
from test_oracle_pyrlk import nonfinite_scene

pytestmark = pytest.mark.gpu
W, H = 101, 70
NAN, INF = float("nan"), float("inf")
U32 = np.uint32

# ---- corpus ---------------------------------------------------------------------------------------------------------------------
VALUES = [NAN, INF, -INF, 3e9, -3e9, 1e9, 2147483520.0, 2147483648.0, -2147483648.0, 1e38, 3.4e38, -0.0, 1e-40]
SPECIALS = np.array([(v, 35.0) for v in VALUES] + [(50.0, v) for v in VALUES] + [(v, v) for v in VALUES], np.float32)
CONTROLS = synth.grid_points(W, H, 64, margin=6, seed=2)            # the points of test_klt_parity_other_sizes at this size
N = len(SPECIALS) + len(CONTROLS)                                   # 103
_slots = [0, 63, 64, N - 1]
_slots += [i for i in range(2, N, 2) if i not in _slots][:len(SPECIALS) - 4]
IS_SPECIAL = np.zeros(N, bool)
IS_SPECIAL[_slots] = True
assert IS_SPECIAL.sum() == len(SPECIALS) and N <= 130

MIXED = np.zeros((N, 2), np.float32)                                # specials interleaved with the controls
MIXED[IS_SPECIAL], MIXED[~IS_SPECIAL] = SPECIALS, CONTROLS
FINITE = MIXED.copy()                                               # a control (cycled) wherever MIXED has a special
FINITE[IS_SPECIAL] = CONTROLS[np.arange(len(SPECIALS)) % len(CONTROLS)]
OFFSET = np.array([1.5, -1.0], np.float32)
# mode -> (previous points, initial guesses or None)
MODES = {"prev": (MIXED, None),                                     # specials as previous points (no guess: they start the search too)
         "guess": (FINITE, np.where(IS_SPECIAL[:, None], MIXED, FINITE + OFFSET).astype(np.float32)),   # ... as initial guesses
         "prev_under_guess": (MIXED, FINITE + OFFSET)}              # ... as previous points under a finite guess
GRAD_FROM = [None, "0"]                                             # HV_GRAD_FROM_LEVEL=0: every template from the stored gradient planes


def _same_lk(got, want, what):
    """Device (xy, status, err) against the oracle's: every point."""
    (gxy, gst, gerr), (oxy, ost, oerr) = got, want
    np.testing.assert_array_equal(gst, ost, err_msg=f"{what}: status")
    nan = np.isnan(oxy)
    assert np.isnan(gxy[nan]).all(), (what, "NaN positions", gxy[nan])
    bad = np.nonzero((np.ascontiguousarray(gxy).view(U32) != np.ascontiguousarray(oxy).view(U32)) & ~nan)[0]
    assert bad.size == 0, (what, "positions", bad[:8], gxy[bad[:8]], oxy[bad[:8]])
    if gerr is not None:
        np.testing.assert_array_equal(gerr, oerr, err_msg=f"{what}: err")


@pytest.fixture(scope="module")
def lk_ref(oracle):
    """The oracle's answers, computed once: images, pyramids and, per (direction, mode, max_count), (xy, status, err)."""
    a, b = nonfinite_scene()
    pyr = {"ab": (oracle.Pyramid(a), oracle.Pyramid(b)), "ba": (oracle.Pyramid(b), oracle.Pyramid(a))}
    ref = {"images": (a, b), "pyr": pyr}
    for d, (p, q) in pyr.items():
        for mode, (prev, guess) in MODES.items():
            for mc in (20, 1):
                ref[d, mode, mc] = oracle.klt_track(p, q, prev, next_pts=guess, max_count=mc)
            ref[d, mode, "flow"] = oracle.optical_flow_compute(p, q, prev, corners=guess)
    st = ref["ab", "prev", 20][1]
    # a kernel (or an oracle) that fails everything cannot pass: the controls are tracked
    assert st[~IS_SPECIAL].mean() >= 0.8 and ref["ab", "guess", 20][1][~IS_SPECIAL].mean() >= 0.8
    assert not st[IS_SPECIAL][np.isnan(SPECIALS).any(axis=1)].any()
    return ref


def _ctx(monkeypatch, grad_from, **kw):
    if grad_from is not None:
        monkeypatch.setenv("HV_GRAD_FROM_LEVEL", grad_from)
    return capi.Context(width=W, height=H, max_tracks=N, **kw)


# ---- LK: the synchronous entry points --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad_from", GRAD_FROM)
@pytest.mark.parametrize("klt_tile", [5, 1])
def test_klt_track_and_optical_flow_compute(lk_ref, klt_tile, grad_from, monkeypatch):
    a, b = lk_ref["images"]
    with _ctx(monkeypatch, grad_from) as ctx:
        ctx.set_knob("klt_tile", klt_tile)
        assert ctx.get_knob("klt_tile") == klt_tile
        sa, sb = ctx.acquire(), ctx.acquire()
        ctx.build(sa, a); ctx.build(sb, b)
        for mode, (prev, guess) in MODES.items():
            for mc, override in ((20, -1), (1, 1)):
                got = ctx.klt_track(sa, sb, prev, next_xy=guess, max_iter_override=override)
                _same_lk(got, lk_ref["ab", mode, mc], f"hv_klt_track {mode} max_iter {mc} tile {klt_tile}")
            o_xy, o_fs = lk_ref["ab", mode, "flow"]
            g_xy, g_fs = ctx.optical_flow_compute(sa, sb, prev, corners=guess)
            np.testing.assert_array_equal(g_fs, o_fs, err_msg=f"hv_optical_flow_compute {mode}")
            _same_lk((g_xy, g_fs, None), (o_xy, o_fs, None), f"hv_optical_flow_compute {mode}")
            # NaN is FAILED_FLOW (no comparison of the range test holds), everything else outside the image FLOW_OUT_OF_RANGE
            sp = g_fs[IS_SPECIAL]
            if mode != "prev_under_guess":
                assert (sp[np.isnan(SPECIALS).any(axis=1)] == G.FAILED_FLOW).all()
                assert (sp[(np.abs(SPECIALS) >= 1e9).any(axis=1)] == G.FLOW_OUT_OF_RANGE).all()


# ---- LK: the batched entry points, and the neighbours of a special ---------------------------------------------------------------
def _dev(x, dt=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x if dt is None else np.asarray(x, dt))).cuda()


def _batch(ctx, prev_slots, next_slots, per_pair, prev, guess, counts=None, max_iter_override=-1):
    """One hv_klt_track_batch_dev / _ragged_dev call on host arrays [pairs][per_pair][2] -> (xy, status, err) per pair."""
    import torch
    P = len(prev_slots)
    d_prev, d_next = _dev(prev_slots, np.int32), _dev(next_slots, np.int32)
    d_p = _dev(prev, np.float32)
    d_n = _dev(guess, np.float32) if guess is not None else torch.full_like(d_p, -5.0)
    d_s = torch.full((P, per_pair), 9, dtype=torch.uint8, device="cuda")
    d_e = torch.full((P, per_pair), -3.0, dtype=torch.float32, device="cuda")
    if counts is None:
        ctx.klt_track_batch_dev(P, d_prev.data_ptr(), d_next.data_ptr(), per_pair, d_p.data_ptr(), d_n.data_ptr(), d_s.data_ptr(),
                                d_e.data_ptr(), use_initial_flow=guess is not None, max_iter_override=max_iter_override)
    else:
        d_counts = _dev(counts, np.int32)
        ctx.klt_track_batch_ragged_dev(P, d_prev.data_ptr(), d_next.data_ptr(), per_pair, d_counts.data_ptr(),
                                       d_p.data_ptr(), d_n.data_ptr(), d_s.data_ptr(), d_e.data_ptr(),
                                       use_initial_flow=guess is not None, max_iter_override=max_iter_override)
    torch.cuda.synchronize()
    return d_n.cpu().numpy(), d_s.cpu().numpy(), d_e.cpu().numpy()


RAGGED_COUNTS = [N, 0, 37, 64, 1]


@pytest.mark.parametrize("grad_from", GRAD_FROM)
@pytest.mark.parametrize("mode", list(MODES))
def test_klt_batch_and_ragged_batch(lk_ref, mode, grad_from, monkeypatch):
    """hv_klt_track_batch_dev and hv_klt_track_batch_ragged_dev (its own instance of the kernel): every point equals the oracle,
    and the controls' results are, bit for bit, those of a call that holds the controls alone."""
    import torch
    a, b = lk_ref["images"]
    prev, guess = MODES[mode]
    with _ctx(monkeypatch, grad_from) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        sa, sb = ctx.acquire(), ctx.acquire()
        ctx.build(sa, a); ctx.build(sb, b)
        slot = {"ab": (sa, sb), "ba": (sb, sa)}
        tile = lambda x, k: None if x is None else np.tile(x[None], (k, 1, 1))
        # the controls alone, both directions
        ctl = ~IS_SPECIAL
        dirs = ["ab", "ba"]
        alone = _batch(ctx, [slot[d][0] for d in dirs], [slot[d][1] for d in dirs], int(ctl.sum()), tile(prev[ctl], 2),
                       tile(None if guess is None else guess[ctl], 2))
        for mc, override in ((20, -1), (1, 1)):
            got = _batch(ctx, [slot[d][0] for d in dirs], [slot[d][1] for d in dirs], N, tile(prev, 2), tile(guess, 2),
                         max_iter_override=override)
            for k, d in enumerate(dirs):
                _same_lk(tuple(x[k] for x in got), lk_ref[d, mode, mc], f"batch {mode} {d} max_iter {mc}")
                if mc == 20:
                    for x, y in zip(got, alone):
                        assert x[k][ctl].tobytes() == y[k].tobytes(), ("batch: a control next to a special", mode, d)
        dirs5 = ["ab", "ba", "ab", "ba", "ab"]
        got = _batch(ctx, [slot[d][0] for d in dirs5], [slot[d][1] for d in dirs5], N, tile(prev, 5), tile(guess, 5), counts=RAGGED_COUNTS)
        for k, (d, c) in enumerate(zip(dirs5, RAGGED_COUNTS)):
            want = lk_ref[d, mode, 20]                                   # points are independent: the first c of the full answer
            _same_lk(tuple(x[k][:c] for x in got), tuple(x[:c] for x in want), f"ragged {mode} pair {k} ({c} points)")
            assert not got[1][k][c:].any(), ("ragged: padding has status 0", k)
            nc = int(ctl[:c].sum())
            for x, y in zip(got, alone):
                assert x[k][:c][ctl[:c]].tobytes() == y[dirs.index(d)][:nc].tobytes(), ("ragged: a control next to a special", mode, k)


# ---- rotation RANSAC ----------------------------------------------------------------------------------------------------------------
def _same_R(R, R_o, exact=True):
    R, R_o = np.asarray(R, np.float32).reshape(-1), np.asarray(R_o, np.float32).reshape(-1)
    nan = np.isnan(R_o)
    assert np.array_equal(np.isnan(R), nan), (R, R_o)                  # NaN where the oracle's is (payloads are not compared)
    if exact:
        assert np.array_equal(R[~nan].view(U32), R_o[~nan].view(U32)), (R, R_o)
    else:
        assert nan.all() or np.abs(R[~nan] - R_o[~nan]).max() < 1e-6, (R, R_o)


def _ransac_scene(oracle, kind):
    """tests/test_oracle_rot_ransac.nonfinite_ransac_scene with the camera `kind` of test_gpu_rot_ransac.py."""
    import test_gpu_rot_ransac as RR
    from test_oracle_pyrlk import NONFINITE_PAIRS
    ocam, gcam = RR._cams(oracle, kind)
    c1, c2 = RR._scene(ocam, np.random.default_rng(3), 40, 0)
    c2[:7] = NONFINITE_PAIRS[:7]
    c1[7:10] = NONFINITE_PAIRS[[7, 8, 0]]
    return ocam, gcam, c1, c2


@pytest.mark.parametrize("threads", [0, 1024, 256])
@pytest.mark.parametrize("kind", ["pinhole", "plain", "rotated", "fisheye"])
def test_rot_ransac_with_non_finite_points(oracle, kind, threads):
    import test_gpu_rot_ransac as RR
    ocam, gcam, c1, c2 = _ransac_scene(oracle, kind)
    draws = oracle.mt19937_draws(4649, 200)
    st_o, R_o, best_o, used_o = oracle.rot_ransac_fit(c1, c2, ocam, ocam, draws, RR.THR)
    if kind == "pinhole":                                              # the numbers tests/test_oracle_rot_ransac.py pins
        assert st_o.tolist() == [3] * 10 + [0] * 30 and (best_o, used_o) == (30, 200) and np.isfinite(R_o).all()
    with capi.Context(width=752, height=480) as ctx:
        ctx.set_knob("rot_ransac_threads", threads)
        for rep in range(2 if threads == 0 else 1):                    # the split form's ticket counters are back at zero
            st, R, best, visited = ctx.rot_ransac(c1, c2, gcam, gcam, RR._pairs(draws, 40), RR.THR)
            assert np.array_equal(st, st_o) and best == best_o and 2 * visited == used_o, (rep, st, st_o, best, best_o, visited, used_o)
            _same_R(R, R_o, exact=kind != "fisheye")


def _hostile(n, k=0):
    """n pairs with a NaN, an infinity or a value beyond int's range in at least one coordinate."""
    h = SPECIALS[(np.abs(SPECIALS) >= 1e9).any(axis=1) | np.isnan(SPECIALS).any(axis=1)]
    return h[(np.arange(n) + k) % len(h)]


@pytest.mark.parametrize("threads", [0, 25, 1024])
def test_rot_ransac_batch_dev_with_non_finite_points(oracle, threads):
    """Ragged sets: the pinned scene, sets too small to fit, a clean set, a set whose c2 is non-finite throughout (no hypothesis
    has an inlier, bestInds stays {0, 1} and R itself is NaN) and a set with specials in both frames. Twice."""
    import torch
    import test_gpu_rot_ransac as RR
    ocam, gcam, a0, b0 = _ransac_scene(oracle, "pinhole")
    rng = np.random.default_rng(22)
    sizes = [40, 2, 0, 33, 40, 17, 1]
    S, M = len(sizes), 40
    c1 = np.zeros((S, M, 2), np.float32); c2 = np.zeros((S, M, 2), np.float32); pairs = np.zeros((S, 100, 2), np.int32)
    ref = []
    for s, n in enumerate(sizes):
        if n < 2:
            ref.append(None)
            continue
        a, b = (a0, b0) if s == 0 else RR._scene(ocam, rng, n, n // 5)
        if s == 1:
            b = _hostile(2)
        if s == 4:
            b = _hostile(n)
        if s == 5:
            a, b = a.copy(), b.copy()
            a[[0, 16]] = _hostile(2, 3); b[[5, 16]] = _hostile(2, 7)
        c1[s, :n], c2[s, :n] = a, b
        d = oracle.mt19937_draws(4649 + s, 200)
        pairs[s] = RR._pairs(d, n)
        ref.append(oracle.rot_ransac_fit(a, b, ocam, ocam, d, RR.THR))
    assert ref[4][2] == 0 and np.isnan(ref[4][1]).any() and np.isfinite(ref[3][1]).all() and ref[3][2] > 20
    with capi.Context(width=752, height=480) as ctx:
        d_n, d_c1, d_c2, d_pairs = _dev(sizes, np.int32), _dev(c1), _dev(c2), _dev(pairs)
        R = torch.zeros((S, 9), dtype=torch.float32, device="cuda")
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_knob("rot_ransac_threads", threads)
        for rep in range(2):
            st = torch.full((S, M), -5, dtype=torch.int32, device="cuda")
            summ = torch.full((S, 2), -1, dtype=torch.int32, device="cuda")
            ctx.rot_ransac_batch_dev(S, M, d_n.data_ptr(), d_c1.data_ptr(), d_c2.data_ptr(), gcam, gcam, d_pairs.data_ptr(), RR.THR,
                                     st.data_ptr(), R.data_ptr(), summ.data_ptr())
            torch.cuda.synchronize()
            h_st, h_R, h_sum = st.cpu().numpy(), R.cpu().numpy(), summ.cpu().numpy()
            for s, n in enumerate(sizes):
                if ref[s] is None:
                    assert h_sum[s].tolist() == [0, 0] and (h_st[s] == -5).all(), (rep, s)
                    continue
                st_o, R_o, best_o, used_o = ref[s]
                assert np.array_equal(h_st[s, :n], st_o) and (h_st[s, n:] == -5).all(), (rep, s, h_st[s], st_o)
                assert h_sum[s].tolist() == [best_o, used_o // 2], (rep, s, h_sum[s], best_o, used_o)
                _same_R(h_R[s], R_o)


def test_rot_ransac_lk_batch_dev_with_non_finite_tracked_features(oracle):
    """Non-finite features that carry lk_status == tracked (what LK handed on before it failed NaN guesses): they are compacted
    like any other, draws % n counts them, and the statuses return at the original feature numbers -- equal to the oracle run
    on the compacted arrays."""
    import torch
    import test_gpu_rot_ransac as RR
    ocam, gcam = RR._cams(oracle, "pinhole")
    rng = np.random.default_rng(23)
    S, M = 3, 70
    sizes = [70, 41, 64]
    c1 = np.zeros((S, M, 2), np.float32); c2 = np.zeros((S, M, 2), np.float32)
    lk = np.zeros((S, M), np.uint8)
    draws = np.stack([oracle.mt19937_draws(4649 + s, 200) for s in range(S)])
    for s, n in enumerate(sizes):
        c1[s, :n], c2[s, :n] = RR._scene(ocam, rng, n, n // 6)
        lk[s, :n] = rng.random(n) < 0.8
        where = sorted({0, min(63, n - 2), n - 1} | set(rng.choice(np.arange(1, n - 1), 5, replace=False).tolist()))
        c2[s, where] = _hostile(len(where), 5 * s)
        lk[s, where] = 1
        c1[s, 7] = (NAN, 200.0); lk[s, 7] = 1
        lk[s, n:] = 1                                                  # behind the set's count: never read
    with capi.Context(width=752, height=480) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        st = torch.full((S, M), -7, dtype=torch.int32, device="cuda")
        R = torch.zeros((S, 9), dtype=torch.float32, device="cuda"); summ = torch.zeros((S, 2), dtype=torch.int32, device="cuda")
        d_n, d_c1, d_c2, d_lk, d_draws = _dev(sizes, np.int32), _dev(c1), _dev(c2), _dev(lk), _dev(draws)
        ctx.rot_ransac_lk_batch_dev(S, M, d_n.data_ptr(), d_c1.data_ptr(), d_c2.data_ptr(), d_lk.data_ptr(), 1, gcam, gcam,
                                    d_draws.data_ptr(), RR.THR, st.data_ptr(), R.data_ptr(), summ.data_ptr())
        torch.cuda.synchronize()
        st, R, summ = st.cpu().numpy(), R.cpu().numpy(), summ.cpu().numpy()
    for s, n in enumerate(sizes):
        keep = np.nonzero(lk[s, :n] == 1)[0]
        assert 20 < len(keep) < n
        st_o, R_o, best_o, used_o = oracle.rot_ransac_fit(c1[s][keep], c2[s][keep], ocam, ocam, draws[s], RR.THR)
        assert np.array_equal(st[s][keep], st_o), (s, st[s][keep], st_o)
        rest = np.ones(M, bool); rest[keep] = False
        assert (st[s][rest] == -7).all(), s
        assert summ[s].tolist() == [best_o, used_o // 2], (s, summ[s], best_o, used_o)
        _same_R(R[s], R_o)


# ---- one chain ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad_from", GRAD_FROM)
def test_chain_lk_flow_status_rotation_ransac_and_track_table(oracle, lk_ref, grad_from, monkeypatch):
    """hv_klt_track_batch_ragged_dev with predicted corners, some of them NaN or infinite (what a NaN pose predicts) ->
    hv_flow_status_batch_dev -> hv_rot_ransac_lk_batch_dev -> hv_tracks_update_batch_dev, nothing through the host. Every stage
    equals the oracle / the restatements driven by the ORACLE's LK output, and no non-finite position reaches the table.
    The set that holds maxTracks tracks (the culling runs: a sort of all pair distances, whose order the reference leaves
    undefined once a distance is NaN) gets one infinite guess -- its distances are +inf, ordered; the NaN guesses go to the
    sets below maxTracks."""
    import torch
    import test_gpu_track_table as TT
    a, b = lk_ref["images"]
    S, M = 3, 21
    counts = [21, 17, 9]
    imgs = [(a, b), (b, a), (a, b)]
    cam_args = ("pinhole", 60.0, 60.0, 50.5, 35.0)
    ocam, gcam = oracle.Camera(*cam_args), capi.camera_model(*cam_args)
    thr = 1.0
    bad = [{20: (INF, 30.0)},
           {0: (NAN, NAN), 5: (-INF, -INF), 16: (50.0, NAN)},
           {0: (3e9, 20.0), 8: (NAN, 35.0)}]
    prm = T.Params(maxTracks=M)
    tables, prev, guess = [], np.zeros((S, M, 2), np.float32), np.full((S, M, 2), 7e5, np.float32)
    for s, n in enumerate(counts):
        t = T.TrackTable(prm, W, H, False)
        t.frameNum = 5 + s
        p = synth.grid_points(W, H, n, margin=8, seed=10 + s)
        for i in range(n):
            t.tracks.append(dict(id=100 * s + i + 1, status=T.TRACKED, p0=(p[i, 0], p[i, 1]), p1=None))
            if i % 4:
                t.lastKeyframeCornerByTrackId[100 * s + i + 1] = (p[i, 0] - np.float32(1), p[i, 1])
        tables.append(t)
        prev[s, :n], guess[s, :n] = p, p + OFFSET
        for i, v in bad[s].items():
            guess[s, i] = v
    draws = np.stack([oracle.mt19937_draws(4649 + s, 200) for s in range(S)])
    with _ctx(monkeypatch, grad_from) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        sa, sb = ctx.acquire(), ctx.acquire()
        ctx.build(sa, a); ctx.build(sb, b)
        slot = {id(a): sa, id(b): sb}
        dt = TT.DevTable(S, M, False, 4)
        TT._upload(dt, [t.arrays() for t in tables])
        dt.corners.copy_(_dev(guess))
        d_prev, d_cur = _dev([slot[id(p)] for p, _ in imgs], np.int32), _dev([slot[id(q)] for _, q in imgs], np.int32)
        d_lk = torch.full((S, M), 9, dtype=torch.uint8, device="cuda")
        d_r2 = torch.full((S, M), -7, dtype=torch.int32, device="cuda")
        d_R = torch.zeros((S, 9), dtype=torch.float32, device="cuda"); d_sum = torch.zeros((S, 2), dtype=torch.int32, device="cuda")
        P = lambda x: x.data_ptr()
        n_tracks = dt.m["n_tracks"].clone()                              # (the update rewrites the table's own count)
        ctx.klt_track_batch_ragged_dev(S, P(d_prev), P(d_cur), M, P(n_tracks), P(dt.m["xy"]), P(dt.corners), P(d_lk), 0, use_initial_flow=True)
        ctx.flow_status_batch_dev(S, M, P(n_tracks), P(dt.corners), P(d_lk), P(dt.ts))
        flow = dt.ts.clone()
        d_draws = _dev(draws)
        ctx.rot_ransac_lk_batch_dev(S, M, P(n_tracks), P(dt.m["xy"]), P(dt.corners), P(d_lk), 1, gcam, gcam, P(d_draws), thr,
                                    P(d_r2), P(d_R), P(d_sum))
        dt.ts.copy_(torch.where(d_r2 == 3, torch.full_like(dt.ts, T.RANSAC_OUTLIER), dt.ts))   # ransac_pipeline.cpp:121-126
        ts_in = dt.ts.clone()
        dt.update(ctx, capi.track_table_default_params(maxTracks=M))
        torch.cuda.synchronize()
        lk, nxt, flow, r2, R, summ, ts_in = (x.cpu().numpy() for x in (d_lk, dt.corners, flow, d_r2, d_R, d_sum, ts_in))
        up = dt.host()
        o_ts, o_kf, o_nm, o_mask, o_src = (x.cpu().numpy() for x in (dt.ts, dt.keyframe, dt.n_mask, dt.mask_xy, dt.src))
    for s, n in enumerate(counts):
        p, q = imgs[s]
        oxy, ost, _ = oracle.klt_track(oracle.Pyramid(p), oracle.Pyramid(q), prev[s, :n], next_pts=guess[s, :n])
        _same_lk((nxt[s, :n], lk[s, :n], None), (oxy, ost, None), f"chain LK set {s}")
        assert not lk[s, n:].any() and not ost[list(bad[s])].any() and ost.sum() >= 5
        o_flow = G.flow_status(ost, oxy, W, H)
        assert np.array_equal(flow[s, :n], o_flow), (s, flow[s, :n], o_flow)
        keep = np.nonzero(ost == 1)[0]
        st_o, R_o, best_o, used_o = oracle.rot_ransac_fit(prev[s][keep], oxy[keep], ocam, ocam, draws[s], thr)
        assert np.array_equal(r2[s][keep], st_o) and (np.delete(r2[s], keep) == -7).all(), (s, r2[s], st_o)
        assert summ[s].tolist() == [best_o, used_o // 2]
        _same_R(R[s], R_o)
        ts = o_flow.copy()
        ts[keep[st_o == 3]] = T.RANSAC_OUTLIER
        assert np.array_equal(ts_in[s, :n], ts), (s, ts_in[s, :n], ts)
        ts_out = list(ts)
        r = tables[s].update(oxy, None, ts_out, 0.0)
        assert not r["reset"] and o_kf[s] == int(r["keyframe"]) and o_nm[s] == len(r["mask"]), (s, o_kf[s], r["keyframe"], o_nm[s])
        assert TT._same(o_mask[s, :o_nm[s]], r["mask"]) and TT._same(o_ts[s, :n], np.array(ts_out, np.int32)), s
        assert o_src[s, :len(r["src_index"])].tolist() == r["src_index"], s
        TT._assert_table(up, s, tables[s].arrays(), f"chain update set {s}")
        live = up["n_tracks"][s]
        assert live >= 3 and np.isfinite(up["xy"][s, :live]).all() and np.isfinite(up["kf_xy"][s, :live][up["kf_valid"][s, :live] != 0]).all()
