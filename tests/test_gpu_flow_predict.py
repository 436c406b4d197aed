"""GPU tests of the device optical-flow predictor (hv_flow_predict_batch_dev) against the literal restatement
tests/flow_predict_restatement.py in binary64 (the restatement) and in np.longdouble (the truth). The index state is produced on
the device, by driving hv_trail_select / finish_batch_dev over the frames of a synthetic world; the means are the true poses plus
noise, set with hv_ekf_set_state.

Bars. A point is decided unless the restatement and the truth take different branches or the truth sits within 1e-9 relative of
a branch threshold (flow_predict_restatement.undecided); at most 1 % may be undecided. For decided points the decisions equal the
restatement's, |pred - float(truth)| <= 1 binary32 ulp at the coordinate + 8 x |restatement - truth|, and |distance - truth| <=
8 x |restatement - truth| + 64 eps x |truth|: the project's bar of 8 x the oracle's own error with floor 64 eps
(tests/test_gpu_ekf_accuracy.py), the ulp covering the final rounding to float."""
import ctypes as C
import functools

import numpy as np
import pytest

import flow_predict_restatement as F
import test_gpu_trail_index as TI
from hybvio_amd import capi

pytestmark = pytest.mark.gpu
W, H = 752, 480
EPS = float(np.finfo(np.float64).eps)
SENTINEL_XY, SENTINEL_D = -12345.5, -777.25


class Rig:
    """One case on the device: the index driven to the end of the case's frames, the final table, the filter batch with the
    case's means, and the buffers of the predictor calls."""

    def __init__(self, ctx, c, means=None):
        import torch
        self.ctx, self.c = ctx, c
        S, M = c["S"], c["M"]
        self.dt = dt = TI.DevTrail(S, c["gp"], c["stereo"])
        dt.init(ctx)
        for f in range(len(c["seqs"][0])):
            frs = [seq[f] for seq in c["seqs"]]
            dt.load_select_inputs(frs)
            dt.load_finish_inputs(frs)
            dt.select(ctx, *c["gcams"])
            dt.finish(ctx)
        for k in ("n_tracks", "ids", "xy", "second_xy"):
            if dt.t[k] is not None:
                dt.t[k].copy_(TI._dev(c["table"][k]))
        self.ekf = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=c["trail"]), batch=S)
        assert self.ekf.n == c["n_state"]
        self.set_means(c["means"] if means is None else means)
        self.c0 = {ty: TI._dev(c["c0"][ty]) for ty in c["types"]}
        self.pred = torch.full((S, M, 2), SENTINEL_XY, dtype=torch.float32, device="cuda")
        self.dist = torch.full((S, M), SENTINEL_D, dtype=torch.float64, device="cuda")

    def set_means(self, means):
        for b in range(self.c["S"]):
            self.ekf.set_state(b, m=means[b])

    def predict(self, ty, pred=None, dist=None, reuse=False, keep_distance=True):
        pred = self.pred if pred is None else pred
        dist = self.dist if dist is None else dist
        self.ekf.flow_predict_batch_dev(self.c["fpar"], ty, self.c["gp"], self.dt.trail.table, self.dt.table, self.c0[ty].data_ptr(),
                                        self.c["gcams"][0], self.c["gcams"][1], pred.data_ptr(), dist.data_ptr() if keep_distance else 0, reuse)

    def fetch(self, ty, **kw):
        import torch
        self.pred.fill_(SENTINEL_XY); self.dist.fill_(SENTINEL_D)
        self.predict(ty, **kw)
        torch.cuda.synchronize()
        return self.pred.cpu().numpy(), self.dist.cpu().numpy()


def _context():
    import torch
    ctx = capi.Context(width=W, height=H)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    return ctx


@functools.lru_cache(maxsize=None)
def _outputs(name):
    """pred and distance of every type of a case, computed once: {type: (pred, distance)}; and the device index against the
    restatement's: every track sits in as many keyframes."""
    import torch
    c = F.case(name)
    with _context() as ctx:
        rig = Rig(ctx, c)
        torch.cuda.synchronize()
        h = rig.dt.host()
        for s in range(c["S"]):
            idx = c["finals"][s]["session"].ekfStateIndex
            live = h["col_len"][s] > 0
            assert dict(zip(h["col_id"][s][live].tolist(), h["col_len"][s][live].tolist())) == idx.lengths(), (name, s)
            assert int(h["n_keyframes"][s]) == len(idx.keyframes)
        out = {ty: rig.fetch(ty) for ty in c["types"]}
        out["kf_row"] = h["kf_row"]
        rig.ekf.close()
    return out


def _points(name):
    c, out = F.case(name), _outputs(name)
    for ty in c["types"]:
        pred, dist = out[ty]
        for s in range(c["S"]):
            rest, truth = c["results"][ty][s]
            for i, (r, t) in enumerate(zip(rest, truth)):
                yield ty, s, i, r, t, pred[s, i], dist[s, i], c["c0"][ty][s, i]


@pytest.mark.parametrize("name", list(F.CASES))
def test_decisions_equal_the_restatement(name):
    c = F.case(name)
    m = c["par"].predictOpticalFlowMinTriangulationDistance
    n = skipped = 0
    for ty, s, i, r, t, pred, dist, c0 in _points(name):
        n += 1
        if F.undecided(r, t):
            skipped += 1
            continue
        what = (name, ty, s, i)
        # distance_dev discloses "triangulated" (in front of the camera) and "clamped"
        assert (dist == m) == r["clamped"], (what, dist, r["distance"])
        assert (dist > m) == (r["triangulated"] and r["in_front"] and not r["clamped"]), (what, dist)
        # the camera calls: c1 is c0 itself exactly when one of them failed
        if r["p2r"] and r["r2p"]:
            assert r["c1"] == (c0[0], c0[1]) or not np.array_equal(pred, c0), what
        else:
            assert np.array_equal(pred, c0), (what, pred, c0)
    print(name, "points", n, "undecided", skipped)
    assert skipped <= 0.01 * n
    if c["trail"] >= 20:
        assert any(not np.array_equal(row, np.arange(c["trail"] + 1)) for row in _outputs(name)["kf_row"])   # a rotated kf_row was read


@pytest.mark.parametrize("name", list(F.CASES))
def test_values_within_eight_times_the_restatements_own_error(name):
    n = equal_pred = equal_dist = 0
    worst_p = worst_d = 0.0
    for ty, s, i, r, t, pred, dist, c0 in _points(name):
        if F.undecided(r, t):
            continue
        what = (name, ty, s, i)
        n += 1
        equal_pred += r["c1"] == (pred[0], pred[1])
        equal_dist += float(r["distance"]) == dist
        own = abs(F.LD(r["distance"]) - t["distance"])
        err, bound = abs(F.LD(dist) - t["distance"]), 8 * own + 64 * F.LD(EPS) * abs(t["distance"])
        assert err <= bound, (what, "distance", float(err), float(bound))
        worst_d = max(worst_d, float(err / (F.LD(EPS) * abs(t["distance"]))))
        if t["pixel1"] is None:
            assert np.array_equal(pred, c0), what
            continue
        for a in range(2):
            want = np.float32(t["pixel1"][a])
            own = abs(F.LD(r["pixel1"][a]) - t["pixel1"][a])
            err, bound = abs(F.LD(pred[a]) - F.LD(want)), F.LD(np.spacing(np.abs(want))) + 8 * own
            assert err <= bound, (what, "pred", a, float(err), float(bound))
            worst_p = max(worst_p, float(err / F.LD(np.spacing(np.abs(want)))))
    print(f"{name}: {n} decided points, pred bit-equal to the restatement {equal_pred / n:.4f}, distance {equal_dist / n:.4f}; "
          f"worst pred error {worst_p:.3f} binary32 ulp, worst distance error {worst_d:.2f} eps")


def test_reused_distance_gives_the_bits_of_a_call_that_triangulates():
    import torch
    c = F.case("stereo")
    with _context() as ctx:
        rig = Rig(ctx, c)
        fresh_pred, fresh_dist = rig.fetch(F.STEREO)
        left_pred, left_dist = rig.fetch(F.LEFT)                           # leaves its distances in rig.dist ...
        rig.pred.fill_(SENTINEL_XY)
        rig.predict(F.STEREO, reuse=True)                                 # ... which the stereo call reads
        torch.cuda.synchronize()
        assert np.array_equal(rig.pred.cpu().numpy().view(np.uint32), fresh_pred.view(np.uint32))
        assert np.array_equal(rig.dist.cpu().numpy().view(np.uint64), left_dist.view(np.uint64))     # read, not written
        assert np.array_equal(left_dist.view(np.uint64), fresh_dist.view(np.uint64))                  # all types triangulate with the first camera
        # without distance_dev the call still predicts
        rig.pred.fill_(SENTINEL_XY)
        rig.predict(F.STEREO, keep_distance=False)
        torch.cuda.synchronize()
        assert np.array_equal(rig.pred.cpu().numpy().view(np.uint32), fresh_pred.view(np.uint32))
        rig.ekf.close()


def test_eager_and_one_graph_replayed_three_times_give_identical_bits():
    import torch
    c = F.case("stereo")
    with capi.Context(width=W, height=H) as ctx:
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            rig = Rig(ctx, c)
            eager = {ty: rig.fetch(ty) for ty in (F.LEFT, F.STEREO)}
            pred2 = torch.full_like(rig.pred, SENTINEL_XY)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                rig.predict(F.LEFT)
                rig.predict(F.STEREO, pred=pred2, reuse=True)
            for _ in range(3):
                rig.pred.fill_(SENTINEL_XY); pred2.fill_(SENTINEL_XY); rig.dist.fill_(SENTINEL_D)
                g.replay()
                stream.synchronize()
                assert np.array_equal(rig.pred.cpu().numpy().view(np.uint32), eager[F.LEFT][0].view(np.uint32))
                assert np.array_equal(pred2.cpu().numpy().view(np.uint32), eager[F.STEREO][0].view(np.uint32))
                assert np.array_equal(rig.dist.cpu().numpy().view(np.uint64), eager[F.LEFT][1].view(np.uint64))
            del g
            ctx.profile_enable(True)
            ctx.profile_reset()
            rig.predict(F.LEFT)
            assert ctx.profile_read(capi.K_TRAIL_INDEX)[1] == 1
            rig.predict(F.STEREO, reuse=True)
            ms, launches = ctx.profile_read(capi.K_TRAIL_INDEX)
            assert launches == 2 and ms > 0
            rig.ekf.close()


def test_padding_is_not_written_and_a_non_finite_mean_stays_in_its_set():
    import torch
    c = F.case("stereo")
    S, M, bad = c["S"], c["M"], 1
    clean = _outputs("stereo")
    n_tracks = c["table"]["n_tracks"]
    assert (n_tracks < M).any()                                            # there is padding to look at
    for ty in c["types"]:
        pred, dist = clean[ty]
        for s in range(S):
            assert (pred[s, n_tracks[s]:] == np.float32(SENTINEL_XY)).all() and (dist[s, n_tracks[s]:] == SENTINEL_D).all(), (ty, s)
            assert np.isfinite(pred[s, :n_tracks[s]]).all() and (dist[s, :n_tracks[s]] >= 3.0).all(), (ty, s)
    idx = c["finals"][bad]["session"].ekfStateIndex
    n = int(n_tracks[bad])
    poisons = {"NaN in the orientation of history pose 0": (F.CAM + 4, np.nan), "inf in the current position": (F.POS, np.inf),
               "NaN in the position of keyframe 12": (F.CAM + 7 * 11 + 1, np.nan), "-inf in the current orientation": (F.ORI + 2, -np.inf)}
    with _context() as ctx:
        rig = Rig(ctx, c)
        for what, (entry, value) in poisons.items():
            means = c["means"].copy()
            means[bad, entry] = value
            rig.set_means(means)
            seen_non_finite = False
            for ty in c["types"]:
                pred, dist = rig.fetch(ty)
                want = F.predict(np.float64, idx, means[bad], c["par"], c["rcams"], ty, c["c0"][ty][bad, :n], c["table"]["ids"][bad, :n].tolist())
                w_pred = np.array([r["c1"] for r in want], np.float32)
                w_dist = np.array([float(r["distance"]) for r in want])
                assert np.array_equal(np.isnan(pred[bad, :n]), np.isnan(w_pred)) and np.array_equal(np.isinf(pred[bad, :n]), np.isinf(w_pred)), (what, ty)
                assert np.array_equal(np.isnan(dist[bad, :n]), np.isnan(w_dist)) and np.array_equal(np.isinf(dist[bad, :n]), np.isinf(w_dist)), (what, ty)
                assert np.array_equal(dist[bad, :n] == 3.0, w_dist == 3.0), (what, ty)       # a NaN pf is "not in front": the minimum
                seen_non_finite |= bool((~np.isfinite(w_pred)).any())
                for s in range(S):
                    if s != bad:
                        assert np.array_equal(pred[s].view(np.uint32), clean[ty][0][s].view(np.uint32)), (what, ty, s)
                        assert np.array_equal(dist[s].view(np.uint64), clean[ty][1][s].view(np.uint64)), (what, ty, s)
                assert (pred[bad, n:] == np.float32(SENTINEL_XY)).all() and (dist[bad, n:] == SENTINEL_D).all(), (what, ty)
            assert seen_non_finite or "keyframe 12" in what, what
        rig.ekf.close()


def test_a_state_too_small_for_the_trail_is_unsupported_and_invalid_wins():
    c = F.case("trail5")
    with _context() as ctx:
        ekf = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=5), batch=c["S"])
        dt = TI.DevTrail(c["S"], c["gp"], True)
        longer = capi.trail_index_default_params(cameraTrailLength=6, maxTracks=c["M"])
        a = dt.t["xy"].data_ptr()

        def call(tp, kind=0, pred=a):
            return capi.lib().hv_flow_predict_batch_dev(ekf._h, C.byref(c["fpar"]), kind, C.byref(tp), C.byref(dt.trail.table), C.byref(dt.table),
                                                        C.c_void_p(a), C.addressof(c["gcams"][0]), C.addressof(c["gcams"][1]), C.c_void_p(pred), None, 0)

        assert call(longer) == -2 and call(longer, kind=3) == -1 and call(longer, pred=0) == -1
        ekf.close()


def test_predictions_start_the_lk_call_as_they_start_the_oracles(oracle, seq752):
    """The chain: pred_xy goes straight into hv_klt_track_batch_ragged_dev(use_initial_flow = 1); statuses and positions equal
    the oracle's LK started from the same (downloaded) guesses."""
    import torch
    left, _, _ = seq752
    c = F.case("stereo")
    S, M = c["S"], c["M"]
    with capi.Context(width=W, height=H, pool_size=8) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        rig = Rig(ctx, c)
        slots = [ctx.acquire() for _ in range(2)]
        d_imgs = torch.from_numpy(np.ascontiguousarray(left[:2])).cuda()
        d_slots = torch.tensor(slots, dtype=torch.int32, device="cuda")
        ctx.build_batch_dev(2, d_slots.data_ptr(), d_imgs.data_ptr(), W * H, W)
        prev = torch.full((S,), slots[0], dtype=torch.int32, device="cuda")
        nxt = torch.full((S,), slots[1], dtype=torch.int32, device="cuda")
        status = torch.full((S * M,), 9, dtype=torch.uint8, device="cuda")
        rig.predict(F.LEFT)
        guesses = rig.pred.clone()
        ctx.klt_track_batch_ragged_dev(S, prev.data_ptr(), nxt.data_ptr(), M, rig.dt.t["n_tracks"].data_ptr(), rig.dt.t["xy"].data_ptr(),
                                       rig.pred.data_ptr(), status.data_ptr(), 0, use_initial_flow=True)
        torch.cuda.synchronize()
        guesses, xy, st = guesses.cpu().numpy(), rig.pred.cpu().numpy(), status.cpu().numpy().reshape(S, M)
        refs = [oracle.Pyramid(im) for im in left[:2]]
        tracked = 0
        for s in range(S):
            n = int(c["table"]["n_tracks"][s])
            o_xy, o_st, _ = oracle.klt_track(refs[0], refs[1], c["table"]["xy"][s, :n], next_pts=guesses[s, :n])
            np.testing.assert_array_equal(st[s, :n], o_st)
            np.testing.assert_array_equal(xy[s, :n], o_xy)
            assert not st[s, n:].any()
            tracked += int(o_st.sum())
        assert tracked > 0
        rig.ekf.close()
