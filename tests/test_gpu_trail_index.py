"""GPU tests of the device pose-trail index (hv_trail_init / select / finish_batch_dev) against the literal restatement
tests/trail_index_restatement.py. Every rule is integer or single-rounded IEEE arithmetic, so every comparison is
np.array_equal: the state read back in logical order after each call and every output, over a 40-frame corpus at every
configuration, with a fisheye camera (integer outputs only), eagerly and replayed from one captured graph, and joined with the
filter (select -> hv_ekf_visual_frame_ragged_dev -> finish -> hv_tracks_delete_batch_dev -> hv_ekf_symmetrize_augment_dev)."""
import functools

import numpy as np
import pytest

import ransac3_restatement as R3
import trail_index_restatement as T
from hybvio_amd import capi

pytestmark = pytest.mark.gpu
W, H, FRAMES = 752, 480, 40
PLAIN = dict(kind="pinhole", fx=458.6, fy=457.3, ppx=367.2, ppy=248.4)
RADIAL = dict(PLAIN, coeffs=[-0.28, 0.07, 0.0])
_c, _s = np.cos(0.02), np.sin(0.02)
ROTATED = dict(PLAIN, rotation=[[_c, 0.0, _s], [0.0, 1.0, 0.0], [-_s, 0.0, _c]])
FISHEYE = dict(kind="fisheye", fx=190.9, fy=190.9, ppx=376.0, ppy=240.0, coeffs=[0.0034, 0.0007, -0.002, 0.0002], max_valid_fov_deg=150.0)
# (maxTracks, n_sets, trail, hanoi, stereo): one wavefront and less, several sets, the defaults (a thread loop over the tracks is
# not needed below 257 tracks: 200 is the reference's value), more sets than CUs
CORPUS = [(8, 1, 4, 2, False), (24, 3, 6, 2, True), (200, 2, 20, 3, True), (24, 300, 6, 2, True)]
CAMERAS = {8: (PLAIN, PLAIN), 24: (RADIAL, ROTATED), 200: (RADIAL, RADIAL), 300: (PLAIN, ROTATED)}
LIMITS = {8: (3, 2), 24: (6, 3), 200: (20, 5), 300: (6, 3)}        # maxVisualUpdates, maxSuccessfulVisualUpdates
# a trail of 20 only fills, and only sees a Hanoi removal, with tracks that live 21 frames and a run of keyframes
LONG_TRAIL = dict(warm=24, special=(2, 1), drop=0.015, p_key=0.85)
DISTINCT = 12                                                       # set s of a larger batch repeats sequence s % DISTINCT


def _dev(x, dt=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x if dt is None else np.asarray(x, dt))).cuda()


def _cams(spec):
    from oracle import orc
    kw = {k: v for k, v in spec.items() if k not in ("kind", "fx", "fy", "ppx", "ppy")}
    args = (spec["kind"], spec["fx"], spec["fy"], spec["ppx"], spec["ppy"])
    return orc.Camera(*args, **kw), capi.camera_model(*args, **kw)


def _params(M, trail, hanoi, stereo, sampling, **over):
    V, succ = LIMITS[M]
    kw = dict(cameraTrailLength=trail, cameraTrailHanoiLength=hanoi, useStereo=int(stereo), maxTracks=M, maxVisualUpdates=V,
              maxSuccessfulVisualUpdates=succ, trackSampling=sampling)
    kw.update(over)
    return T.Params(**{k: (bool(v) if k == "useStereo" else v) for k, v in kw.items()}), capi.trail_index_default_params(**kw)


def _pack(state, ncam):
    """Session.state() as arrays: per keyframe the sorted track IDs, [n][ncam][6] = imagePoint, normalizedImagePoint,
    normalizedVelocity, and the used flags."""
    ids, vals, used = [], [], []
    for feats in state["features"]:
        k = sorted(feats)
        ids.append(np.array(k, np.int32))
        vals.append(np.array([[feats[t][0][c] + feats[t][1][c] + feats[t][2][c] for c in range(ncam)] for t in k], np.float64).reshape(len(k), ncam, 6))
        used.append(np.array([feats[t][3] for t in k], np.uint8))
    return dict(n_keyframes=state["n_keyframes"], frame_counter=state["frame_counter"], frame_number=np.array(state["frame_number"], np.int32),
                timestamp=np.array(state["timestamp"], np.float64), ids=ids, vals=vals, used=used, blacklist=np.array(state["blacklist"], np.int32))


def _pack_dev(h, s, K, ncam, after_finish):
    """The device state of set s in logical order: kf_row maps keyframe -> row; a column of length L sits in the keyframes
    0 .. L - 1 after select and 1 .. L after finish."""
    n, rows, L, cid = int(h["n_keyframes"][s]), h["kf_row"][s], h["col_len"][s], h["col_id"][s]
    assert sorted(rows.tolist()) == list(range(K)) and 1 <= n <= K, (s, rows)
    assert (cid[L == 0] == -1).all() and (L >= 0).all()
    ids, vals, used = [], [], []
    off = 1 if after_finish else 0
    for i in range(n):
        cols = np.nonzero(L > i - off)[0] if i >= off else np.zeros(0, np.int64)
        cols = cols[np.argsort(cid[cols], kind="stable")]
        r = rows[i]
        ids.append(cid[cols].astype(np.int32))
        vals.append(np.concatenate([h["image_point"][s, r, cols].astype(np.float64), h["norm_point"][s, r, cols], h["norm_velocity"][s, r, cols]],
                                   axis=2).reshape(len(cols), ncam, 6))
        used.append(h["used"][s, r, cols])
    nb = int(h["n_blacklist"][s])
    return dict(n_keyframes=n, frame_counter=int(h["frame_counter"][s]), frame_number=h["frame_number"][s, rows[:n]],
                timestamp=h["timestamp"][s, rows[:n]], ids=ids, vals=vals, used=used, blacklist=h["blacklist_ids"][s, :nb])


def _assert_state(got, want, what, floats=True):
    assert got["n_keyframes"] == want["n_keyframes"] and got["frame_counter"] == want["frame_counter"], (what, got["n_keyframes"], want["n_keyframes"])
    for k in ("frame_number", "timestamp", "blacklist"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for i in range(want["n_keyframes"]):
        assert np.array_equal(got["ids"][i], want["ids"][i]), (what, "ids of keyframe", i, got["ids"][i], want["ids"][i])
        assert np.array_equal(got["used"][i], want["used"][i]), (what, "used flags of keyframe", i)
        g, w = (got["vals"][i], want["vals"][i]) if floats else (got["vals"][i][:, :, :2], want["vals"][i][:, :, :2])
        assert np.array_equal(g, w), (what, "observations of keyframe", i)


@functools.lru_cache(maxsize=None)
def _record(M, S, trail, hanoi, stereo, sampling, camera_key=None, frames=FRAMES):
    """The restatement run of min(S, DISTINCT) sequences, computed once: per frame and sequence the inputs, the outputs of
    select() and finish() and the packed states, and the counts of the cases the corpus is there for."""
    p, _ = _params(M, trail, hanoi, stereo, sampling)
    spec = CAMERAS[M] if camera_key is None else (FISHEYE, FISHEYE)
    ocams = (_cams(spec[0])[0], _cams(spec[1])[0])
    beyond = (lambda rng: rng.uniform([0, 0], [40, 30])) if camera_key == "fisheye" else None
    D, ncam = min(S, DISTINCT), 2 if stereo else 1
    seen = dict(popped=0, free_slot=0, short=0, score=0, carried=0, not_carried=0, closed=0, one_track=0, no_track=0, full_table=0,
                repeated_time=0, beyond=0)
    hanoi_seen = set()
    seqs = []
    for d in range(D):
        rec, last_t = [], None
        for fr in T.drive(p, R3.normalize_pixel, ocams, frames, 7000 + 100 * M + 10 * sampling + d, W, H, beyond=beyond,
                          **(LONG_TRAIL if trail >= 20 else {})):
            fr["after_select"], fr["after_finish"] = _pack(fr["after_select"], ncam), _pack(fr["after_finish"], ncam)
            kinds = [k for k, _ in fr["walk"]]
            new_bl, skipped = fr["finish"]["blacklist"], [t for _, t in fr["select"]["skipped"]]
            seen["popped"] += (not fr["keyframe"]) and fr["frame"] > 0
            if fr["n_kf_before_push"] == trail + 1:
                seen["free_slot"] += fr["empty_tail"]
                if not fr["empty_tail"]:
                    hanoi_seen.add(fr["finish"]["discarded"] + 1)
            seen["short"] += "short" in kinds; seen["score"] += "score" in kinds; seen["closed"] += "closed" in kinds
            seen["carried"] += any(t in new_bl for t in skipped); seen["not_carried"] += any(t not in new_bl for t in skipped)
            seen["one_track"] += len(fr["select"]["order"]) == 1; seen["no_track"] += len(fr["table"]) == 0
            seen["full_table"] += len(fr["table"]) == M
            seen["repeated_time"] += last_t == fr["time"]
            seen["beyond"] += len(fr["select"]["order"]) < len(fr["table"])
            last_t = fr["time"]
            rec.append(fr)
        seqs.append(rec)
    return seqs, seen, hanoi_seen


class DevTrail:
    """The state, the table arrays select reads, and the buffers of the select / finish calls for S sets."""

    def __init__(self, S, gp, stereo):
        import torch
        self.S, self.gp, self.stereo = S, gp, stereo
        self.M, self.K, self.V, self.ncam = gp.maxTracks, gp.cameraTrailLength + 1, gp.maxVisualUpdates, 2 if stereo else 1
        M, K, V, Cn = self.M, self.K, self.V, self.ncam
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        i32, f64, u8 = torch.int32, torch.float64, torch.uint8
        self.trail = capi.TrailIndex(S, gp)
        self.t = dict(n_tracks=z(S, i32), ids=z((S, M), i32), xy=z((S, M, 2), torch.float32), second_xy=z((S, M, 2), torch.float32) if stereo else None)
        self.table = capi.track_table(**{k: (v.data_ptr() if v is not None else 0) for k, v in self.t.items()})
        self.i = dict(keyframe=z(S, i32), full=z(S, u8), frame_num=z(S, i32), time=z(S, f64), draws=z((S, M), i32),
                      status=z((V, S, 2), i32), gate=z((V, S), i32), stationary=z(S, u8))
        self.o = dict(draws_used=z(S, i32), n_poses=z((V, S), i32), pose_index=z((V, S, K), i32), features=z((V, S, Cn * K, 2), f64),
                      velocities=z((V, S, Cn * K, 2), f64), y=z((V, S, 2 * Cn * K), f64), cand_id=z((V, S), i32), n_cand=z(S, i32),
                      delete_ids=z((S, M), i32), n_delete=z(S, i32), good=z(S, u8), attempts=z(S, i32), successes=z(S, i32), discarded=z(S, i32))

    def init(self, ctx):
        ctx.trail_init_batch_dev(self.S, self.trail.table, params=self.gp)

    def select(self, ctx, cam0, cam1):
        i, o = self.i, self.o
        P = lambda x: x.data_ptr()
        ctx.trail_select_batch_dev(self.S, self.trail.table, self.table, cam0, cam1, P(i["keyframe"]), P(i["full"]), P(i["frame_num"]),
                                   P(i["time"]), P(i["draws"]), P(o["draws_used"]), P(o["n_poses"]), P(o["pose_index"]), P(o["features"]),
                                   P(o["velocities"]), P(o["y"]), P(o["cand_id"]), P(o["n_cand"]), params=self.gp)

    def finish(self, ctx, status=None, gate=None):
        i, o = self.i, self.o
        P = lambda x: x.data_ptr()
        ctx.trail_finish_batch_dev(self.S, self.trail.table, P(o["cand_id"]), P(o["n_cand"]), P(i["status"] if status is None else status),
                                   P(i["gate"] if gate is None else gate), P(i["stationary"]), P(o["delete_ids"]), P(o["n_delete"]), P(o["good"]),
                                   P(o["attempts"]), P(o["successes"]), P(o["discarded"]), params=self.gp)

    def load_select_inputs(self, frs):
        """frs: the frame records of the DISTINCT sequences; set s takes sequence s % len(frs)."""
        S, M = self.S, self.M
        h = dict(n_tracks=np.zeros(S, np.int32), ids=np.full((S, M), -77, np.int32), xy=np.full((S, M, 2), -5e5, np.float32),
                 second_xy=np.full((S, M, 2), -5e5, np.float32), keyframe=np.zeros(S, np.int32), full=np.zeros(S, np.uint8),
                 frame_num=np.zeros(S, np.int32), time=np.zeros(S), draws=np.zeros((S, M), np.uint32))
        for d, fr in enumerate(frs):
            n = len(fr["table"])
            h["n_tracks"][d] = n
            if n:
                h["ids"][d, :n] = [t[0] for t in fr["table"]]
                h["xy"][d, :n] = [t[1] for t in fr["table"]]
                if self.stereo:
                    h["second_xy"][d, :n] = [t[2] for t in fr["table"]]
            h["keyframe"][d], h["full"][d], h["frame_num"][d], h["time"][d], h["draws"][d] = fr["keyframe"], fr["full"], fr["frame_num"], fr["time"], fr["draws"]
        rep = np.arange(S) % len(frs)
        for k in ("n_tracks", "ids", "xy", "second_xy"):
            if self.t[k] is not None:
                self.t[k].copy_(_dev(h[k][rep]))
        for k in ("keyframe", "full", "frame_num", "time"):
            self.i[k].copy_(_dev(h[k][rep]))
        self.i["draws"].copy_(_dev(h["draws"][rep].view(np.int32)))

    def load_finish_inputs(self, frs):
        S, V = self.S, self.V
        st, gt, sta = np.full((V, S, 2), T.TRI_NOT_VISITED, np.int32), np.full((V, S), T.NOT_COMPUTED, np.int32), np.zeros(S, np.uint8)
        for d, fr in enumerate(frs):
            n = len(fr["tri"])
            st[:n, d, 0], gt[:n, d], sta[d] = fr["tri"], fr["gate"], fr["stationary"]
            st[:n, d, 1] = [0 if t == T.TRI_OK else T.TRI_NOT_VISITED for t in fr["tri"]]
        rep = np.arange(S) % len(frs)
        self.i["status"].copy_(_dev(st[:, rep])); self.i["gate"].copy_(_dev(gt[:, rep])); self.i["stationary"].copy_(_dev(sta[rep]))

    def host(self):
        h = {k: v.cpu().numpy() for k, v in self.trail.m.items()}
        h.update({k: v.cpu().numpy() for k, v in self.o.items()})
        return h


def _assert_repeats(h, D, S, what):
    """Sets that were given the same sequence hold the same bytes in every array."""
    if S <= D:
        return
    rep = np.arange(S) % D
    for k, v in h.items():
        if v.shape[0] == S:
            assert np.array_equal(v, v[rep]), (what, k)
        else:
            assert np.array_equal(v, v[:, rep]), (what, k)


def _assert_select(h, d, fr, dt, what, floats=True):
    sel, K, Cn = fr["select"], dt.K, dt.ncam
    cands = sel["candidates"]
    assert h["draws_used"][d] == sel["draws_used"] == max(len(sel["order"]) - 1, 0) and h["n_order"][d] == len(sel["order"]), (what, "order")
    assert h["n_cand"][d] == len(cands), (what, h["n_cand"][d], len(cands))
    assert np.array_equal(h["cand_id"][:, d], np.array([c["id"] for c in cands] + [-1] * (dt.V - len(cands)), np.int32)), (what, "cand_id")
    assert np.array_equal(h["n_poses"][:, d], np.array([len(c["index"]) for c in cands] + [0] * (dt.V - len(cands)), np.int32)), (what, "n_poses")
    assert np.array_equal(h["cand_pos"][d, :len(cands)], np.array([c["pos"] for c in cands], np.int32)), (what, "cand_pos")
    for v, c in enumerate(cands):
        nv = len(c["index"])
        assert np.array_equal(h["pose_index"][v, d, :nv], np.array(c["index"], np.int32)), (what, v, "pose_index")
        if floats:
            assert np.array_equal(h["features"][v, d, :Cn * nv], np.array(c["features"])), (what, v, "features")
            assert np.array_equal(h["velocities"][v, d, :Cn * nv], np.array(c["velocities"])), (what, v, "velocities")
            assert np.array_equal(h["y"][v, d, :2 * Cn * nv], np.array(c["y"])), (what, v, "y")
    ns = len(sel["skipped"])
    assert h["n_skipped"][d] == ns, (what, "n_skipped")
    assert np.array_equal(h["skipped_pos"][d, :ns], np.array([q for q, _ in sel["skipped"]], np.int32).reshape(-1)), (what, "skipped_pos")
    assert np.array_equal(h["skipped_id"][d, :ns], np.array([t for _, t in sel["skipped"]], np.int32).reshape(-1)), (what, "skipped_id")


def _assert_finish(h, d, fr, what):
    fin = fr["finish"]
    nd = len(fin["delete_ids"])
    assert h["n_delete"][d] == nd and np.array_equal(h["delete_ids"][d, :nd], np.array(fin["delete_ids"], np.int32).reshape(-1)), (what, "delete_ids")
    assert (h["good"][d], h["attempts"][d], h["successes"][d], h["discarded"][d]) == (int(fin["good_frame"]), fin["attempts"], fin["successes"],
                                                                                      fin["discarded"]), (what, fin)


def _run_frames(ctx, dt, seqs, gcams, floats=True, replay=None):
    """Every frame: inputs up, select, compare, statuses up, finish, compare. replay: a captured graph of select + finish."""
    import torch
    D = len(seqs)
    for f in range(len(seqs[0])):
        frs = [seq[f] for seq in seqs]
        dt.load_select_inputs(frs)
        dt.load_finish_inputs(frs)
        if replay is not None:
            replay.replay()
        else:
            dt.select(ctx, *gcams)
            torch.cuda.synchronize()
            h = dt.host()
            _assert_repeats(h, D, dt.S, f"select frame {f}")
            for d, fr in enumerate(frs):
                what = f"select frame {f} sequence {d}"
                _assert_select(h, d, fr, dt, what, floats)
                _assert_state(_pack_dev(h, d, dt.K, dt.ncam, False), fr["after_select"], what, floats)
            dt.finish(ctx)
        torch.cuda.synchronize()
        h = dt.host()
        _assert_repeats(h, D, dt.S, f"finish frame {f}")
        for d, fr in enumerate(frs):
            what = f"finish frame {f} sequence {d}"
            if replay is not None:
                _assert_select(h, d, fr, dt, what, floats)
            _assert_finish(h, d, fr, what)
            _assert_state(_pack_dev(h, d, dt.K, dt.ncam, True), fr["after_finish"], what, floats)


@pytest.mark.parametrize("sampling", [T.GAP, T.ALL])
@pytest.mark.parametrize("M,S,trail,hanoi,stereo", CORPUS)
def test_forty_frames_of_select_and_finish_equal_the_restatement(M, S, trail, hanoi, stereo, sampling):
    import torch
    seqs, _, _ = _record(M, S, trail, hanoi, stereo, sampling)
    _, gp = _params(M, trail, hanoi, stereo, sampling)
    gcams = tuple(_cams(c)[1] for c in CAMERAS[M])
    with capi.Context(width=W, height=H) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        dt = DevTrail(S, gp, stereo)
        dt.init(ctx)
        torch.cuda.synchronize()
        h = dt.host()
        for d in range(len(seqs)):
            _assert_state(_pack_dev(h, d, dt.K, dt.ncam, True), _pack(T.Session(_params(M, trail, hanoi, stereo, sampling)[0], None).state(), dt.ncam), "init")
        _run_frames(ctx, dt, seqs, gcams)


def test_the_corpus_contains_the_cases_it_is_there_for():
    """A popped head, a free-slot removal, each Hanoi index, tracks below trackMinFrames and below the median, carried and
    not-carried blacklist entries, more passing tracks than maxVisualUpdates, n - 1 = 0 draws, a frame without tracks, one at
    capacity and repeated timestamps: a corpus without any of these would hide a failure."""
    total = {}
    for cfg in CORPUS:
        for sampling in (T.GAP, T.ALL):
            _, seen, hanoi_seen = _record(*cfg, sampling)
            for k, v in seen.items():
                total[k] = total.get(k, 0) + int(v)
            M, S, trail, hanoi, stereo = cfg
            assert {trail - hanoi + i for i in range(hanoi)} | {trail} <= hanoi_seen, (cfg, sampling, hanoi_seen)
            for k in ("popped", "short", "score", "no_track", "full_table", "repeated_time", "one_track"):
                assert seen[k] > 0, (cfg, sampling, k)
    total.pop("beyond")
    assert all(v > 0 for v in total.values()), total
    for cfg in CORPUS[1:]:
        seen = _record(*cfg, T.GAP)[1]
        assert seen["carried"] > 0 and seen["not_carried"] > 0 and seen["closed"] > 0 and seen["free_slot"] > 0, (cfg, seen)


def test_fisheye_integer_outputs_equal_the_restatement_and_points_beyond_the_field_of_view_stay_out():
    """sin and cos come from two maths libraries (as in test_gpu_rot_ransac.py), so the normalised points and velocities are not
    compared; the normalisation flags, the order, the candidates, the pose indices, the pixels and every integer output are."""
    import torch
    M, S, trail, hanoi, stereo = 24, 3, 6, 2, True
    seqs, seen, _ = _record(M, S, trail, hanoi, stereo, T.GAP, "fisheye")
    assert seen["beyond"] > 10 and seen["popped"] > 0
    _, gp = _params(M, trail, hanoi, stereo, T.GAP)
    gcam = _cams(FISHEYE)[1]
    with capi.Context(width=W, height=H) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        dt = DevTrail(S, gp, stereo)
        dt.init(ctx)
        _run_frames(ctx, dt, seqs, (gcam, gcam), floats=False)


def test_forty_frames_eager_and_one_graph_replayed_equal_the_restatement():
    """3 sets x 40 frames: once eagerly and once as ONE captured graph of select + finish replayed 40 times with only the input
    buffers rewritten; HV_K_TRAIL_INDEX counts one launch per entry."""
    import torch
    M, S, trail, hanoi, stereo = 24, 3, 6, 2, True
    seqs, _, _ = _record(M, S, trail, hanoi, stereo, T.GAP)
    _, gp = _params(M, trail, hanoi, stereo, T.GAP)
    gcams = tuple(_cams(c)[1] for c in CAMERAS[M])
    with capi.Context(width=W, height=H) as ctx:
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        for mode in ("eager", "graph"):
            with torch.cuda.stream(stream):
                dt = DevTrail(S, gp, stereo)
                dt.init(ctx)
                stream.synchronize()
                g = None
                if mode == "graph":
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=stream):
                        dt.select(ctx, *gcams)
                        dt.finish(ctx)
                _run_frames(ctx, dt, seqs, gcams, replay=g)
            del g
        ctx.profile_enable(True)
        with torch.cuda.stream(stream):
            dt = DevTrail(S, gp, stereo)
            ctx.profile_reset()
            dt.init(ctx)
            assert ctx.profile_read(capi.K_TRAIL_INDEX)[1] == 1
            dt.load_select_inputs([seq[0] for seq in seqs]); dt.load_finish_inputs([seq[0] for seq in seqs])
            dt.select(ctx, *gcams)
            assert ctx.profile_read(capi.K_TRAIL_INDEX)[1] == 2
            dt.finish(ctx)
            ms, launches = ctx.profile_read(capi.K_TRAIL_INDEX)
            assert launches == 3 and ms > 0
            assert ctx.profile_read(capi.K_TRACK_TABLE)[1] == 0


def test_more_tracks_than_threads():
    """maxTracks 300 > the 256 threads of a workgroup: every loop over the slots, the columns and the order takes a second turn."""
    import torch
    M, S, trail, hanoi, stereo = 300, 2, 4, 2, True
    seqs, _, _ = _record(M, S, trail, hanoi, stereo, T.GAP, None, 16)
    assert max(len(fr["select"]["order"]) for seq in seqs for fr in seq) > 256
    _, gp = _params(M, trail, hanoi, stereo, T.GAP)
    gcams = tuple(_cams(c)[1] for c in CAMERAS[M])
    with capi.Context(width=W, height=H) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        dt = DevTrail(S, gp, stereo)
        dt.init(ctx)
        _run_frames(ctx, dt, seqs, gcams)


# ---- joined with the filter ----------------------------------------------------------------------------------------------------------
def _rot(q):
    w, x, y, z = q
    return np.array([[w*w+x*x-y*y-z*z, 2*x*y-2*w*z, 2*x*z+2*w*y], [2*x*y+2*w*z, w*w-x*x+y*y-z*z, 2*y*z-2*w*x],
                     [2*x*z-2*w*y, 2*y*z+2*w*x, w*w-x*x-y*y+z*z]])


def test_select_joined_with_the_filter_equals_the_same_calls_fed_by_the_restatement():
    """3 sets, trail 6: the means are synth.visual_tracks' trajectories, the pixel tracks are world points projected through the plain
    pinhole from the pose that sits at each keyframe when the last frame arrives (frame g is seen from pose 6 - g), some tracks
    shorter than trackMinFrames and some with wrong pixels. Six frames build the index (no visits); on the seventh the device
    select feeds hv_ekf_visual_frame_ragged_dev directly, then finish, hv_tracks_delete_batch_dev and
    hv_ekf_symmetrize_augment_dev(discarded_dev). A second batch of the same filters runs the same calls on arrays built by the
    restatement and uploaded from the host: statuses, success counters, means, covariances and tables are bit-identical."""
    import torch
    from hybvio_amd import synth
    S, trail, M, n_tr = 3, 6, 24, 12
    K = trail + 1
    rng = np.random.default_rng(31)
    T1, T2, means, _, _ = synth.visual_tracks(rng, S, trail, K, True)
    p, gp = _params(M, trail, 2, True, T.GAP)
    V, quota = LIMITS[M]
    ocam, gcam = _cams(PLAIN)
    Ric, base2 = T1[:3, :3], T2[:3, 3]
    start = [0, 0, 0, 0, 0, 0, 0, 0, 2, 3, 4, 5]                                          # the last three stay below trackMinFrames
    px = np.zeros((S, K, n_tr, 2, 2), np.float32)                                        # [set][pose][track][camera]
    for s in range(S):
        m = means[s]
        cams = []
        for k in range(K):
            ip, io = (0, 6) if k == 0 else (20 + 7 * (k - 1), 20 + 7 * (k - 1) + 3)
            R = Ric @ _rot(m[io:io + 4])
            cams.append([(R, m[ip:ip + 3] - R.T @ (base2 if cam else np.zeros(3))) for cam in range(2)])
        for i in range(n_tr):
            pw = cams[0][0][1] + cams[0][0][0].T @ np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2, 12)])
            for k in range(K):
                for cam in range(2):
                    R, pos = cams[k][cam]
                    pc = R @ (pw - pos)
                    noise = rng.normal(size=2) * (25.0 if i % 4 == 3 else 0.2)           # every fourth track has wrong pixels
                    px[s, k, i, cam] = [PLAIN["fx"] * pc[0] / pc[2] + PLAIN["ppx"] + noise[0], PLAIN["fy"] * pc[1] / pc[2] + PLAIN["ppy"] + noise[1]]
    draws = rng.integers(0, 2 ** 32, (K, S, M), dtype=np.uint32)
    ses = [T.Session(p, R3.normalize_pixel) for _ in range(S)]
    vp = capi.vu_default_params(imu_to_camera=T1, second_imu_to_camera=T2)
    r_gate, r_update = 1.5, 0.05
    z = lambda shape, dtp: torch.zeros(shape, dtype=dtp, device="cuda")
    with capi.Context(width=W, height=H) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        filters = [capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=trail), S) for _ in range(2)]
        for g in filters:
            for s in range(S):
                g.set_state(s, means[s], np.eye(g.n) * 1e-4)
        dt = DevTrail(S, gp, True)
        tables = []
        for _ in range(2):                                                                # the device path's table and the host path's
            t = dict(dt.t, status=z((S, M), torch.int32), blacklist=z((S, M), torch.uint8), kf_xy=z((S, M, 2), torch.float32),
                     kf_valid=z((S, M), torch.uint8), frame_num=z(S, torch.int32), mask_steps=z(S, torch.int32), mask_radius=z(S, torch.int32),
                     frame_flags=z(S, torch.uint8))
            tables.append(t)
        tables[1] = {k: v.clone() for k, v in tables[1].items()}
        tt = [capi.track_table(**{k: v.data_ptr() for k, v in t.items()}) for t in tables]
        dt.t, dt.table = tables[0], tt[0]
        dt.init(ctx)
        frs = None
        for g in range(K):
            frs = []
            for s in range(S):
                table = [(100 * s + i + 1, tuple(px[s, trail - g, i, 0]), tuple(px[s, trail - g, i, 1])) for i in range(n_tr) if start[i] <= g]
                fr = dict(table=table, keyframe=True, full=True, frame_num=g + 1, time=0.05 * (g + 1), draws=draws[g, s])
                fr["select"] = ses[s].select(table, (ocam, ocam), True, True, g + 1, fr["time"], fr["draws"])
                fr["after_select"] = _pack(ses[s].state(), 2)
                if g < trail:
                    n = len(fr["select"]["candidates"])
                    fr.update(tri=[T.TRI_NOT_VISITED] * n, gate=[T.NOT_COMPUTED] * n, stationary=False)
                    fr["finish"] = ses[s].finish(fr["tri"], fr["gate"], False)
                frs.append(fr)
            dt.load_select_inputs(frs)
            dt.select(ctx, gcam, gcam)
            if g < trail:
                dt.load_finish_inputs(frs)
                dt.finish(ctx)
        for k in tables[1]:
            tables[1][k].copy_(tables[0][k])
        # ---- the device path: nothing crosses the host between select and the augmentation ----
        o = dt.o
        P = lambda x: x.data_ptr()
        st, gs, cnt = [z((V, S, 2), torch.int32) for _ in range(2)], [z((V, S), torch.int32) for _ in range(2)], [z(S, torch.int32) for _ in range(2)]
        filters[0].visual_frame_ragged_dev(vp, V, K, P(o["n_poses"]), P(o["pose_index"]), P(o["features"]), P(o["velocities"]), P(o["y"]), r_gate,
                                           r_update, P(st[0]), P(gs[0]), P(cnt[0]), quota)
        dt.finish(ctx, status=st[0], gate=gs[0])
        ctx.tracks_delete_batch_dev(S, tt[0], M, P(o["n_delete"]), P(o["delete_ids"]), params=capi.track_table_default_params(maxTracks=M))
        filters[0].symmetrize_augment_dev(P(o["discarded"]))
        torch.cuda.synchronize()
        h = dt.host()
        # ---- the host path: the restatement's arrays, uploaded ----
        Cn = 2
        a = dict(n_poses=np.zeros((V, S), np.int32), pose_index=np.zeros((V, S, K), np.int32), features=np.zeros((V, S, Cn * K, 2)),
                 velocities=np.zeros((V, S, Cn * K, 2)), y=np.zeros((V, S, 2 * Cn * K)))
        for s, fr in enumerate(frs):
            for v, c in enumerate(fr["select"]["candidates"]):
                nv = len(c["index"])
                a["n_poses"][v, s] = nv
                a["pose_index"][v, s, :nv] = c["index"]
                a["features"][v, s, :Cn * nv] = c["features"]; a["velocities"][v, s, :Cn * nv] = c["velocities"]; a["y"][v, s, :2 * Cn * nv] = c["y"]
        d = {k: _dev(v) for k, v in a.items()}
        filters[1].visual_frame_ragged_dev(vp, V, K, P(d["n_poses"]), P(d["pose_index"]), P(d["features"]), P(d["velocities"]), P(d["y"]), r_gate,
                                           r_update, P(st[1]), P(gs[1]), P(cnt[1]), quota)
        torch.cuda.synchronize()
        st_h, gs_h = st[1].cpu().numpy(), gs[1].cpu().numpy()
        del_ids, n_del, disc = np.zeros((S, M), np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
        for s, fr in enumerate(frs):
            n = len(fr["select"]["candidates"])
            fr.update(tri=list(st_h[:n, s, 0]), gate=list(gs_h[:n, s]), stationary=False)
            fr["finish"] = ses[s].finish(fr["tri"], fr["gate"], False)
            n_del[s], disc[s] = len(fr["finish"]["delete_ids"]), fr["finish"]["discarded"]
            del_ids[s, :n_del[s]] = fr["finish"]["delete_ids"]
        d_del, d_n, d_disc = _dev(del_ids), _dev(n_del), _dev(disc)
        ctx.tracks_delete_batch_dev(S, tt[1], M, P(d_n), P(d_del), params=capi.track_table_default_params(maxTracks=M))
        filters[1].symmetrize_augment_dev(P(d_disc))
        torch.cuda.synchronize()
        assert np.array_equal(st[0].cpu().numpy(), st_h) and np.array_equal(gs[0].cpu().numpy(), gs_h), "statuses"
        assert np.array_equal(cnt[0].cpu().numpy(), cnt[1].cpu().numpy()), "success counters"
        for s, fr in enumerate(frs):
            what = f"joined set {s}"
            _assert_select(h, s, fr, dt, what)
            _assert_finish(h, s, fr, what)
            _assert_state(_pack_dev(h, s, K, 2, True), _pack(ses[s].state(), 2), what)
            (m0, P0), (m1, P1) = filters[0].get_state(s), filters[1].get_state(s)
            assert np.array_equal(m0, m1) and np.array_equal(P0, P1), what
            assert not np.array_equal(m0, means[s]) or cnt[0][s].item() == 0, what
        for k in ("status", "blacklist", "ids", "n_tracks"):
            assert np.array_equal(tables[0][k].cpu().numpy(), tables[1][k].cpu().numpy()), k
        counts = cnt[0].cpu().numpy()
        visited = st_h[:, :, 0] != T.TRI_NOT_VISITED
        assert counts.max() > 0 and (gs_h[visited] != T.INLIER).any(), (counts, gs_h)       # an update was applied and a track rejected
        assert tables[0]["blacklist"].cpu().numpy().sum() == n_del.sum() > 0
        assert (np.array([len(fr["select"]["candidates"]) for fr in frs]) > 0).all()
        for g in filters:
            g.close()
