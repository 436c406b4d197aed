"""GPU tests of the device track table (hv_tracks_init / update / append / delete_batch_dev) against the literal restatement
tests/track_table_restatement.py. Every rule is integer or IEEE arithmetic, so every comparison is equality of bits: a corpus
of random sets at every maxTracks where the kernel takes another path, 40 frames of 64 sets eagerly and replayed from one
captured graph, the whole device frame (LK -> flow status -> gate -> RANSAC2 -> hybrid RANSAC -> table update -> GFTT ->
cornerSubPix -> stereo LK -> detection filter -> append) joined by the table, and the launch count of the timer class."""
import functools

import numpy as np
import pytest

import track_table_restatement as T
from hybvio_amd import capi

pytestmark = pytest.mark.gpu
W, H = 752, 480


def _dev(x, dt=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x if dt is None else np.asarray(x, dt))).cuda()


def _same(a, b):
    """Equality of bits (-0.0 is not 0.0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class DevTable:
    """The arrays of one hv_track_table for S sets of M slots, and the buffers of the update / append / delete calls."""

    def __init__(self, S, M, stereo, max_new, max_ids=4):
        import torch
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        self.S, self.M, self.stereo, self.max_new, self.max_ids = S, M, stereo, max_new, max_ids
        self.m = dict(n_tracks=z(S, torch.int32), ids=z((S, M), torch.int32), xy=z((S, M, 2), torch.float32),
                      second_xy=z((S, M, 2), torch.float32) if stereo else None, status=z((S, M), torch.int32),
                      blacklist=z((S, M), torch.uint8), kf_xy=z((S, M, 2), torch.float32), kf_valid=z((S, M), torch.uint8),
                      frame_num=z(S, torch.int32), mask_steps=z(S, torch.int32), mask_radius=z(S, torch.int32),
                      frame_flags=z(S, torch.uint8))
        self.table = capi.track_table(**{k: (v.data_ptr() if v is not None else 0) for k, v in self.m.items()})
        # inputs
        self.corners, self.second = z((S, M, 2), torch.float32), (z((S, M, 2), torch.float32) if stereo else None)
        self.ts, self.score = z((S, M), torch.int32), z(S, torch.float64)
        self.n_new, self.new_xy = z(S, torch.int32), z((S, max(max_new, 1), 2), torch.float32)
        self.new_second = z((S, max(max_new, 1), 2), torch.float32) if stereo else None
        self.n_ids, self.del_ids = z(S, torch.int32), z((S, max_ids), torch.int32)
        # outputs, filled with a value no call writes
        self.keyframe, self.n_mask = torch.full((S,), -9, dtype=torch.int32, device="cuda"), torch.full((S,), -9, dtype=torch.int32, device="cuda")
        self.mask_xy, self.src = z((S, M, 2), torch.float32), torch.full((S, M), -9, dtype=torch.int32, device="cuda")
        self.mm, self.n_added = z(S, torch.float64), torch.full((S,), -9, dtype=torch.int32, device="cuda")

    def init(self, ctx, prm):
        ctx.tracks_init_batch_dev(self.S, self.table, params=prm)

    def update(self, ctx, prm):
        ctx.tracks_update_batch_dev(self.S, self.table, self.corners.data_ptr(), self.second.data_ptr() if self.stereo else 0,
                                    self.ts.data_ptr(), self.score.data_ptr(), self.keyframe.data_ptr(), self.mask_xy.data_ptr(),
                                    self.n_mask.data_ptr(), self.src.data_ptr(), self.mm.data_ptr(), params=prm)

    def append(self, ctx, prm):
        ctx.tracks_append_batch_dev(self.S, self.table, self.max_new, self.n_new.data_ptr(), self.new_xy.data_ptr(),
                                    self.new_second.data_ptr() if self.stereo else 0, self.n_added.data_ptr(), params=prm)

    def delete(self, ctx, prm):
        ctx.tracks_delete_batch_dev(self.S, self.table, self.max_ids, self.n_ids.data_ptr(), self.del_ids.data_ptr(), params=prm)

    def host(self):
        return {k: (v.cpu().numpy() if v is not None else None) for k, v in self.m.items()}


def _assert_table(got, s, want, what):
    """Set s of the table arrays read back (DevTable.host()) against TrackTable.arrays()."""
    n = want["n_tracks"]
    assert got["n_tracks"][s] == n, (what, s, got["n_tracks"][s], n)
    for k in ("frame_num", "mask_steps", "mask_radius"):
        assert got[k][s] == want[k], (what, s, k, got[k][s], want[k])
    for k in ("ids", "xy", "status", "blacklist", "kf_valid"):
        assert _same(got[k][s, :n], want[k]), (what, s, k)
    if want["second_xy"] is not None:
        assert _same(got["second_xy"][s, :n], want["second_xy"]), (what, s, "second_xy")
    v = want["kf_valid"] != 0
    assert _same(got["kf_xy"][s, :n][v], want["kf_xy"][v]), (what, s, "kf_xy")
    assert not got["kf_valid"][s, n:].any() or what == "delete", (what, s, "kf_valid behind the tracks")


# ---- corpus --------------------------------------------------------------------------------------------------------------------
# maxTracks: the smallest value with one (5) and with two (20) culled tracks, a non-multiple of 20, one wavefront, the default
# and the cap; n_sets: 1, 7 and more sets than CUs. (maxTracks, n_sets, stereo)
CORPUS = [(5, 300, True), (20, 300, False), (21, 7, True), (64, 300, True), (200, 7, False), (200, 1, True), (200, 300, True),
          (1024, 7, True), (1024, 1, False)]


def _random_state(rng, prm, M, stereo, n, grid, clean):
    """A TrackTable in the middle of a run: n tracks with unique IDs, earlier statuses (blacklisted ones among them unless
    `clean`), keyframe entries for most, any frame number and mask scale."""
    t = T.TrackTable(prm, W, H, stereo)
    t.frameNum = int(rng.choice([0, 1, 2, 19, 20, 21, 22, 57]))
    t.maskScale = float(rng.integers(-10, 11)) / 2.0
    ids = rng.choice(np.arange(1, max(t.frameNum, 1) * M + 1), n, replace=False)   # earlier frames' IDs: below this frame's first
    side = int(rng.integers(2, 13))
    for i in range(n):
        p0 = rng.integers(0, side, 2).astype(np.float32) if grid else rng.uniform(0, [W, H]).astype(np.float32)
        st = int(rng.choice([T.TRACKED, T.NEW, T.BLACKLISTED], p=[0.7, 0.3, 0.0] if clean else [0.6, 0.3, 0.1]))
        trk = dict(id=int(ids[i]), status=st, p0=(p0[0], p0[1]), p1=(p0[0] - np.float32(3), p0[1]) if stereo else None)
        t.tracks.append(trk)
        if st != T.NEW and rng.random() < 0.8:
            t.lastKeyframeCornerByTrackId[trk["id"]] = trk["p0"]
    return t, side


def _upload(dt, arrays):
    """Writes TrackTable.arrays() of every set into the device table, slots behind the tracks filled with values no call may read."""
    S, M = dt.S, dt.M
    h = dict(n_tracks=np.zeros(S, np.int32), ids=np.full((S, M), -77, np.int32), xy=np.full((S, M, 2), -5e5, np.float32),
             second_xy=np.full((S, M, 2), -5e5, np.float32), status=np.full((S, M), -77, np.int32), blacklist=np.zeros((S, M), np.uint8),
             kf_xy=np.full((S, M, 2), -5e5, np.float32), kf_valid=np.zeros((S, M), np.uint8), frame_num=np.zeros(S, np.int32),
             mask_steps=np.zeros(S, np.int32), mask_radius=np.zeros(S, np.int32), frame_flags=np.zeros(S, np.uint8))
    for s, a in enumerate(arrays):
        n = a["n_tracks"]
        for k in ("n_tracks", "frame_num", "mask_steps", "mask_radius"):
            h[k][s] = a[k]
        for k in ("ids", "xy", "status", "blacklist", "kf_xy", "kf_valid"):
            h[k][s, :n] = a[k]
        if dt.stereo:
            h["second_xy"][s, :n] = a["second_xy"]
    for k, v in dt.m.items():
        if v is not None:
            v.copy_(_dev(h[k]))


@functools.lru_cache(maxsize=None)
def _corpus(M, S, stereo):
    """The sets of one configuration with what the restatement makes of them, computed once: per set the arrays before the
    frame, the inputs, the results of update / append / delete, and the counts of the cases the corpus is there for."""
    rng = np.random.default_rng(1000 * M + S)
    prm = T.Params(maxTracks=M)
    max_new, max_ids = M + 4, 4
    counts = [c for c in (M, M - 1, 5, 4, 0) if 0 <= c <= M]       # in this order, so that a single set is a full one
    sets = []
    seen = dict(culled=0, reset=0, stationary=0, moving=0, appended=0, skipped=0, first_frames=0, deleted=0)
    for s in range(S):
        grid, clean = s % 2 == 1, rng.random() < 0.3
        n = counts[s % len(counts)] if s < 2 * len(counts) or rng.random() < 0.6 else int(rng.integers(0, M + 1))
        t, side = _random_state(rng, prm, M, stereo, n, grid, clean)
        if s < len(counts) and t.frameNum == 0:
            t.frameNum = 57                                        # the first set of every count is past frame 0
        kind = rng.random()                                       # < 0.3: nothing moved since the last keyframe
        cur, ts = np.zeros((n, 2), np.float32), np.zeros(n, np.int32)
        for i, trk in enumerate(t.tracks):
            if kind < 0.3:
                cur[i] = trk["p0"]
            elif grid:
                cur[i] = rng.integers(0, side, 2)
            else:
                cur[i] = np.float32(trk["p0"]) + rng.uniform(-4, 4, 2).astype(np.float32)
            ts[i] = T.TRACKED if clean or rng.random() < 0.85 else int(rng.integers(0, 9))
            if trk["status"] == T.BLACKLISTED:
                ts[i] = T.BLACKLISTED                              # what hv_track_gate_batch_dev does with `blacklist`
        d = dict(before=t.arrays(), cur=cur, right=cur - np.float32(2.5), ts=ts, score=float(rng.choice([0.0, 0.9, 0.95, 0.96, 1.0])),
                 n_new=int(rng.choice([0, 1, M // 10, M, M + 3, M + 9])),                  # M + 9 > max_new: clamped
                 new=rng.uniform(0, [W, H], (max_new, 2)).astype(np.float32))
        f = t.frameNum
        ts_out = list(ts)
        r = t.update(cur, d["right"] if stereo else None, ts_out, d["score"])
        d.update(r=r, ts_out=np.array(ts_out, np.int32).reshape(-1), updated=t.arrays())
        seen["reset"] += r["reset"]
        if not r["reset"]:
            assert ts_out.count(T.CULLED) >= (M // 20 + 1 if n == M else 0)
            late = f + 1 >= prm.maxTrackLength
            seen["culled"] += n == M
            seen["first_frames"] += not late
            seen["stationary"] += late and not r["keyframe"]
            seen["moving"] += late and r["keyframe"]
        left = len(t.tracks)
        k = min(d["n_new"], max_new)
        d["added"] = t.append(d["new"][:k], (d["new"] - np.float32(2.5))[:k] if stereo else None)
        d["appended"] = t.arrays()
        seen["appended"] += d["added"] > 0
        seen["skipped"] += k > 0 and d["added"] == 0 and left < M
        # deleteTrack on the state the append left: a live ID, the same again, an unknown one, the last track's
        live, lst = [q["id"] for q in t.tracks], []
        if live and s % 4 != 3:
            a = int(rng.choice(live))
            lst = [a, a, 40 * M + 5000, live[-1]][:int(rng.integers(1, 5))]
        d["del_ids"] = lst
        d["n_ids"] = 9 if len(lst) == max_ids and s % 2 else len(lst)                       # 9 > max_ids: clamped
        for track_id in lst:
            t.deleteTrack(track_id)
        d["deleted"] = t.arrays()
        seen["deleted"] += len(set(lst) & set(live))
        sets.append(d)
    return sets, seen


@pytest.mark.parametrize("M,S,stereo", CORPUS)
def test_corpus_update_append_and_delete_equal_the_restatement(M, S, stereo):
    import torch
    sets, _ = _corpus(M, S, stereo)
    gp = capi.track_table_default_params(maxTracks=M)
    max_new = M + 4

    def pad(key, shape, dtp, fill):
        return np.stack([np.concatenate([np.asarray(d[key], dtp).reshape((-1,) + shape),
                                         np.full((M - len(d[key]),) + shape, fill, dtp)]) for d in sets])
    with capi.Context(width=W, height=H) as ctx:
        dt = DevTable(S, M, stereo, max_new)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        _upload(dt, [d["before"] for d in sets])
        dt.corners.copy_(_dev(pad("cur", (2,), np.float32, 7e5)))
        if stereo:
            dt.second.copy_(_dev(pad("right", (2,), np.float32, 7e5)))
            dt.new_second.copy_(_dev(np.stack([d["new"] - np.float32(2.5) for d in sets])))
        ts_in = pad("ts", (), np.int32, -5)
        dt.ts.copy_(_dev(ts_in))
        dt.score.copy_(_dev(np.array([d["score"] for d in sets], np.float64)))
        dt.n_new.copy_(_dev(np.array([d["n_new"] for d in sets], np.int32)))
        dt.new_xy.copy_(_dev(np.stack([d["new"] for d in sets])))
        del_ids = np.zeros((S, dt.max_ids), np.int32)
        for s, d in enumerate(sets):
            del_ids[s, :len(d["del_ids"])] = d["del_ids"]
        dt.del_ids.copy_(_dev(del_ids)); dt.n_ids.copy_(_dev(np.array([d["n_ids"] for d in sets], np.int32)))
        dt.update(ctx, gp)
        torch.cuda.synchronize()
        up = dt.host()
        o_ts, o_kf, o_nm, o_mask, o_src, o_mm = (x.cpu().numpy() for x in (dt.ts, dt.keyframe, dt.n_mask, dt.mask_xy, dt.src, dt.mm))
        dt.append(ctx, gp)
        torch.cuda.synchronize()
        ap, o_added = dt.host(), dt.n_added.cpu().numpy()
        dt.delete(ctx, gp)
        torch.cuda.synchronize()
        de = dt.host()
    for s, d in enumerate(sets):
        r, n_old, what = d["r"], len(d["ts"]), f"update M={M}"
        assert up["frame_flags"][s] == (1 if r["reset"] else 0), (what, s)
        assert o_kf[s] == int(r["keyframe"]) and o_nm[s] == len(r["mask"]), (what, s, o_kf[s], r["keyframe"], o_nm[s], len(r["mask"]))
        assert _same(o_mm[s], np.float64(r["max_movement"])), (what, s, o_mm[s], r["max_movement"])
        assert _same(o_mask[s, :o_nm[s]], r["mask"]), (what, s, "mask_xy")
        assert _same(o_ts[s, :n_old], d["ts_out"]) and _same(o_ts[s, n_old:], ts_in[s, n_old:]), (what, s, "track_status")
        assert o_src[s, :len(r["src_index"])].tolist() == r["src_index"], (what, s, "src_index")
        _assert_table(up, s, d["updated"], what)
        assert o_added[s] == d["added"], (f"append M={M}", s, o_added[s], d["added"])
        _assert_table(ap, s, d["appended"], f"append M={M}")
        assert ap["frame_flags"][s] == 0
        _assert_table(de, s, d["deleted"], "delete")


def test_the_corpus_contains_the_cases_it_is_there_for():
    """Culled, reset, stationary and non-stationary sets, appended and skipped detections, deleted tracks: a corpus without any
    of these would hide a failure."""
    total = {}
    for cfg in CORPUS:
        for k, v in _corpus(*cfg)[1].items():
            total[k] = total.get(k, 0) + int(v)
    assert all(v > 0 for v in total.values()), total
    for M in sorted({c[0] for c in CORPUS}):
        assert sum(_corpus(*c)[1]["culled"] for c in CORPUS if c[0] == M) > 0, M           # the culling ran at every maxTracks
        assert sum(_corpus(*c)[1]["reset"] for c in CORPUS if c[0] == M) > 0, M


# ---- frames: all state is on the device ------------------------------------------------------------------------------------------
def _record_frames(S, M, frames, prm):
    """The restatement run that drives both device runs: per frame the inputs (formed from the restatement's own state, never
    from the device) and the arrays every set must hold afterwards."""
    rng = np.random.default_rng(40)
    tabs = [T.TrackTable(prm, W, H, True) for _ in range(S)]
    rec = []
    for k in range(frames):
        fr = dict(del_ids=np.zeros((S, 4), np.int32), n_ids=np.zeros(S, np.int32), cur=np.zeros((S, M, 2), np.float32),
                  right=np.zeros((S, M, 2), np.float32), ts=np.full((S, M), -5, np.int32), score=np.zeros(S), n_new=np.zeros(S, np.int32),
                  new=rng.uniform(0, [W, H], (S, 12, 2)).astype(np.float32), want=[], keyframe=np.zeros(S, np.int32),
                  n_mask=np.zeros(S, np.int32), culled=0, reset=0)
        for s, t in enumerate(tabs):
            if k % 3 == 0 and t.tracks:                           # deleteTrack between the frames: two live IDs and an unknown one
                lst = [int(rng.choice([q["id"] for q in t.tracks])), int(rng.choice([q["id"] for q in t.tracks])), 99999][:int(rng.integers(1, 4))]
                fr["del_ids"][s, :len(lst)], fr["n_ids"][s] = lst, len(lst)
                for track_id in lst:
                    t.deleteTrack(track_id)
            n = len(t.tracks)
            still = s % 4 == 0 and k > 22 and k % 2 == 0           # nothing moves: not a keyframe once past maxTrackLength
            wipe = s % 16 == 5 and k == 17                         # everything fails: the next frame resets
            for i, q in enumerate(t.tracks):
                step = np.zeros(2, np.float32) if still else rng.uniform(-2.5, 2.5, 2).astype(np.float32)
                fr["cur"][s, i] = np.float32(q["p0"]) + step
                fr["right"][s, i] = fr["cur"][s, i] - np.float32(4)
                st = T.TRACKED if rng.random() < 0.93 else int(rng.choice([T.FAILED_FLOW, T.RANSAC_OUTLIER, T.OUT_OF_RANGE]))
                fr["ts"][s, i] = T.BLACKLISTED if q["status"] == T.BLACKLISTED else (T.FAILED_FLOW if wipe else st)
            fr["score"][s] = 0.99 if s % 2 == 0 else 0.5
            fr["n_new"][s] = 3 if wipe else (int(rng.integers(0, 13)) if k else 12)
            ts = list(fr["ts"][s, :n])
            r = t.update(fr["cur"][s, :n], fr["right"][s, :n], ts, fr["score"][s])
            fr["keyframe"][s], fr["n_mask"][s] = int(r["keyframe"]), len(r["mask"])
            fr["culled"] += ts.count(T.CULLED) > 0
            fr["reset"] += r["reset"]
            t.append(fr["new"][s, :fr["n_new"][s]], fr["new"][s, :fr["n_new"][s]] - np.float32(4))
            fr["want"].append(t.arrays())
        rec.append(fr)
    return rec


def test_forty_frames_eager_and_one_graph_replayed_equal_the_restatement():
    """64 sets x 40 frames of delete -> update -> append with synthetic statuses, maxTracks 40: once eagerly and once as ONE
    captured graph of the three calls replayed 40 times with only the input buffers rewritten. After every frame the table
    (IDs, frame_num, mask_steps / mask_radius, keyframe entries, ...) equals the restatement."""
    import torch
    S, M, frames = 64, 40, 40
    prm = T.Params(maxTracks=M)
    gp = capi.track_table_default_params(maxTracks=M)
    rec = _record_frames(S, M, frames, prm)
    assert sum(f["culled"] for f in rec) > 0 and sum(f["reset"] for f in rec) > S          # frame 0 and the wiped sets
    assert any((f["keyframe"] == 0).any() for f in rec) and len({w["mask_steps"] for f in rec for w in f["want"]}) > 3
    with capi.Context(width=W, height=H) as ctx:
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        for mode in ("eager", "graph"):
            with torch.cuda.stream(stream):
                dt = DevTable(S, M, True, 12)
                dt.init(ctx, gp)
            stream.synchronize()
            g = None
            if mode == "graph":
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=stream):
                    dt.delete(ctx, gp)
                    dt.update(ctx, gp)
                    dt.append(ctx, gp)
            for k, fr in enumerate(rec):
                with torch.cuda.stream(stream):
                    dt.del_ids.copy_(_dev(fr["del_ids"])); dt.n_ids.copy_(_dev(fr["n_ids"]))
                    dt.corners.copy_(_dev(fr["cur"])); dt.second.copy_(_dev(fr["right"])); dt.ts.copy_(_dev(fr["ts"]))
                    dt.score.copy_(_dev(fr["score"])); dt.n_new.copy_(_dev(fr["n_new"]))
                    dt.new_xy.copy_(_dev(fr["new"])); dt.new_second.copy_(_dev(fr["new"] - np.float32(4)))
                    if g is not None:
                        g.replay()
                    else:
                        if k % 3 == 0:
                            dt.delete(ctx, gp)
                        dt.update(ctx, gp)
                        dt.append(ctx, gp)
                stream.synchronize()
                got = dt.host()
                assert _same(dt.keyframe.cpu().numpy(), fr["keyframe"]) and _same(dt.n_mask.cpu().numpy(), fr["n_mask"]), (mode, k)
                for s in range(S):
                    _assert_table(got, s, fr["want"][s], f"{mode} frame {k}")
            del g


def test_profile_class_counts_one_launch_per_update_and_per_append():
    import torch
    S, M = 3, 64
    gp = capi.track_table_default_params(maxTracks=M)
    with capi.Context(width=W, height=H) as ctx:
        dt = DevTable(S, M, False, 8)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.profile_enable(True)
        dt.init(ctx, gp)
        ctx.profile_reset()
        dt.update(ctx, gp)
        assert ctx.profile_read(capi.K_TRACK_TABLE)[1] == 1
        dt.append(ctx, gp)
        ms, launches = ctx.profile_read(capi.K_TRACK_TABLE)
        assert launches == 2 and ms > 0
        for _ in range(3):
            dt.update(ctx, gp)
            dt.append(ctx, gp)
        assert ctx.profile_read(capi.K_TRACK_TABLE)[1] == 8
        assert dt.m["frame_num"].cpu().numpy().tolist() == [4] * S


# ---- the whole device frame ------------------------------------------------------------------------------------------------------
GATE_T = np.array([[1.0, 0.0, 0.0, -0.1], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])   # a baseline along x


# min_dist (gfttMinDistance) 8 / 10, the gate's defaults and a baseline along x: with OracleBackend's LK and detection, the gate's
# and the filter's restatements and this file's TrackTable on the CPU (no RANSAC), seed 77 fills the table at frames 1, 4 and 8
# (376x240, 120 tracks) and at frame 5 (752x480, 200 tracks) and culls 7 / 11 tracks on the frame after. (With a detection crop the
# table never fills on these sequences: the new corners appear at the image edges, where the crop rejects them.)
@pytest.mark.parametrize("w,h,M,min_dist,unique,frames,seeds", [(376, 240, 120, 8, 14, 14, (77, 78)), (752, 480, 200, 10, 40, 30, (77,))])
def test_whole_device_frame_joined_by_the_table(w, h, M, min_dist, unique, frames, seeds):
    """The chain of test_device_chain_lk_gate_rotation_and_hybrid_ransac and of
    test_detection_chain_gftt_subpix_stereo_lk_and_filter joined by the table, on moving_sequence frames: ragged LK from table.xy /
    n_tracks -> flow status -> stereo LK -> flow status -> gate (table.blacklist) -> RANSAC2 -> hybrid RANSAC -> table update ->
    GFTT detect (mask_xy / n_mask / table.mask_radius) -> cornerSubPix -> stereo LK -> flow status -> detection filter -> append.
    Every frame's stage outputs are kept on the device and read after the last frame; the table after every frame equals the
    restatement driven by the same stage outputs, and the table reaches maxTracks and culls on the way."""
    import torch
    import test_gpu_tracker_closed_loop as CL
    S = len(seeds)
    seqs = [CL.moving_sequence(seed, w, h, unique, frames, radius=0.5 * unique, rot=1.2) for seed in seeds]
    cam_args, radial = CL.cam_args(w, h)
    gcam = capi.camera_model(*cam_args, coeffs=radial)
    sg = capi.stereo_gate_default_params(cam0ToCam1=GATE_T)
    gp = capi.gftt_default_params(gfttMinDistance=float(min_dist), maxTracks=M)
    tp = capi.track_table_default_params(maxTracks=M)
    thr = float(np.float32((4.0 * min(w, h) / 720.0) ** 2))
    draws = np.random.default_rng(4649).integers(0, 2 ** 32, (frames, S, 200), dtype=np.uint32)
    snaps = []
    with capi.Context(width=w, height=h, pool_size=4 * S, max_tracks=M) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        dt = DevTable(S, M, True, M)
        t = dt.m
        z = lambda shape, dtp: torch.zeros(shape, dtype=dtp, device="cuda")
        nk = ctx.gftt_keypoint_count(gp)
        d_lk, d_lk2, d_lk3, d_mask = (z((S, M), torch.uint8) for _ in range(4))
        d_ss, d_ss3, d_r2 = (z((S, M), torch.int32) for _ in range(3))
        d_R, d_r2s, d_res = z((S, 9), torch.float32), z((S, 2), torch.int32), z((S, 2), torch.int32)
        d_kp, d_c, d_cr, d_nc = z((S, nk, 3), torch.float32), z((S, M, 2), torch.float32), z((S, M, 2), torch.float32), z(S, torch.int32)
        d_draws = _dev(draws)
        P = lambda x: x.data_ptr()
        dt.init(ctx, tp)
        prev = None
        for f in range(frames):
            cur = [(ctx.acquire(), ctx.acquire()) for _ in range(S)]
            for s in range(S):
                ctx.build(cur[s][0], seqs[s][0][f]); ctx.build(cur[s][1], seqs[s][1][f])
            d_cur, d_rgt = _dev([c[0] for c in cur], np.int32), _dev([c[1] for c in cur], np.int32)
            if f > 0:
                d_prev = _dev([c[0] for c in prev], np.int32)
                ctx.klt_track_batch_ragged_dev(S, P(d_prev), P(d_cur), M, P(t["n_tracks"]), P(t["xy"]), P(dt.corners), P(d_lk), 0,
                                               use_initial_flow=False)
                ctx.flow_status_batch_dev(S, M, P(t["n_tracks"]), P(dt.corners), P(d_lk), P(dt.ts))
                ctx.klt_track_batch_ragged_dev(S, P(d_cur), P(d_rgt), M, P(t["n_tracks"]), P(dt.corners), P(dt.second), P(d_lk2), 0,
                                               use_initial_flow=False)
                ctx.flow_status_batch_dev(S, M, P(t["n_tracks"]), P(dt.second), P(d_lk2), P(d_ss))
                ctx.track_gate_batch_dev(S, M, P(t["n_tracks"]), P(dt.corners), P(dt.second), P(d_ss), P(t["blacklist"]), gcam, gcam,
                                         P(dt.ts), P(d_mask), params=sg)
                ctx.rot_ransac_lk_batch_dev(S, M, P(t["n_tracks"]), P(t["xy"]), P(dt.corners), P(d_mask), 1, gcam, gcam, P(d_draws[f]), thr,
                                            P(d_r2), P(d_R), P(d_r2s))
                ctx.hybrid_ransac_lk_batch_dev(S, M, P(t["n_tracks"]), P(t["xy"]), P(dt.corners), P(dt.ts), P(d_r2), P(d_r2s), gcam, gcam,
                                               P(d_res), P(dt.score))
            snap = dict(n=t["n_tracks"].clone(), cur=dt.corners.clone(), right=dt.second.clone(), ts_in=dt.ts.clone(), score=dt.score.clone())
            dt.update(ctx, tp)
            ctx.gftt_detect_batch_dev(S, P(d_cur), P(d_kp), M, P(dt.n_mask), P(dt.mask_xy), P(t["mask_radius"]), M, P(d_c), P(d_nc), params=gp)
            ctx.corner_subpix_batch_dev(S, P(d_cur), M, P(d_nc), P(d_c))
            ctx.klt_track_batch_ragged_dev(S, P(d_cur), P(d_rgt), M, P(d_nc), P(d_c), P(d_cr), P(d_lk3), 0, use_initial_flow=False)
            ctx.flow_status_batch_dev(S, M, P(d_nc), P(d_cr), P(d_lk3), P(d_ss3))
            ctx.detection_filter_batch_dev(S, M, P(d_nc), P(d_c), P(d_cr), P(d_ss3), gcam, gcam, 0, P(dt.new_xy), P(dt.new_second), P(dt.n_new),
                                           params=sg)
            snap.update(ts_out=dt.ts.clone(), keyframe=dt.keyframe.clone(), n_mask=dt.n_mask.clone(), mask=dt.mask_xy.clone(),
                        src=dt.src.clone(), mm=dt.mm.clone(), radius=t["mask_radius"].clone(), n_new=dt.n_new.clone(),
                        new=dt.new_xy.clone(), new_second=dt.new_second.clone())
            dt.append(ctx, tp)
            snap.update(added=dt.n_added.clone(), table={k: v.clone() for k, v in t.items()})
            snaps.append(snap)
            if prev is not None:
                torch.cuda.synchronize()                            # the slots go back to the pool only after their last reader
                for c in prev:
                    ctx.release(c[0]); ctx.release(c[1])
            prev = cur
        torch.cuda.synchronize()
        snaps = [{k: ({a: b.cpu().numpy() for a, b in v.items()} if isinstance(v, dict) else v.cpu().numpy()) for k, v in sn.items()}
                 for sn in snaps]
    prm = T.Params(maxTracks=M)
    tabs = [T.TrackTable(prm, w, h, True) for _ in range(S)]
    culled = lost = full = detected = 0
    for f, sn in enumerate(snaps):
        for s, tab in enumerate(tabs):
            n, what = len(tab.tracks), f"frame {f}"
            assert sn["n"][s] == n, (what, s)
            radius = tab.maskRadius()
            ts = list(sn["ts_in"][s, :n])
            r = tab.update(sn["cur"][s, :n], sn["right"][s, :n], ts, sn["score"][s])
            assert sn["keyframe"][s] == int(r["keyframe"]) and sn["n_mask"][s] == len(r["mask"]), (what, s)
            assert _same(sn["mask"][s, :len(r["mask"])], r["mask"]) and _same(sn["mm"][s], np.float64(r["max_movement"])), (what, s)
            assert sn["src"][s, :len(r["src_index"])].tolist() == r["src_index"], (what, s)
            if not r["reset"]:
                assert _same(sn["ts_out"][s, :n], np.array(ts, np.int32)), (what, s)
                culled += ts.count(T.CULLED)
                lost += sum(1 for v in ts if v not in (T.TRACKED, T.CULLED))
                full += n == M
            assert sn["radius"][s] == radius                        # the radius the detection of this frame ran with
            k = sn["n_new"][s]
            assert 0 <= k <= M
            detected += k
            added = tab.append(sn["new"][s, :k], sn["new_second"][s, :k])
            assert sn["added"][s] == added, (what, s)
            _assert_table(sn["table"], s, tab.arrays(), what)
    last = snaps[-1]["table"]
    assert full > 0 and culled >= full * (M // 20 + 1), (full, culled)               # the table reached maxTracks and culled
    assert lost > 0 and detected > M and (last["n_tracks"] >= M // 2).all() and (last["frame_num"] == frames).all()
    assert (last["ids"][:, :5] > 0).all() and last["ids"].max() > M                    # tracks born after frame 0 are alive
