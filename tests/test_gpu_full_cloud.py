"""GPU tests of the device full point cloud (hv_full_point_cloud_dev) against the literal restatement
tests/full_cloud_restatement.py, on its generated corpus: every judged frame of every case runs select -> the entry -> finish on
the device, with the case's means and the synthetic outcomes of the visit loop uploaded in between. Every frame of the small cases
is judged; in the 200-track case the first 21 frames only fill the trail (select -> finish) and the last two are judged, the very
last one for the points.

Bars.
- Every integer and copied field (n_points, point_id, point_status, point_first_pixel, n_tail, tail_id, tail_col, tail_pose_mask,
  n_attempts, good_frame) is bit-equal to the restatement REPLAYED ON THE DEVICE'S OWN tail_status and points: the bookkeeping is
  judged apart from the floating point. Sentinels survive behind every count.
- tail_status equals the oracle's on every tail track on which the oracle's binary64 and long-double builds agree; the others
  (at most 1 % of the corpus, asserted on the CPU by test_full_cloud_restatement.py) are a decision within rounding of a
  threshold and are left out, judged by the reference alone.
- point_xyz of a tail track obeys the rule tests/test_gpu_vu_accuracy.py applies to the pf of hv_ekf_visual_prepare_dev:
  tests/vu_truth.py's Ensemble budget against the long-double oracle, FACTOR unchanged. With odometry_to_slam_dev the transform
  adds test_gpu_output.py's bound: 8 x the restatement's own error + 64 u x L."""
import functools

import numpy as np
import pytest

import full_cloud_restatement as F
import output_restatement as OR
import test_gpu_trail_index as TI
import trail_index_restatement as T
import vu_truth as vt
from flow_predict_restatement import LD
from hybvio_amd import capi

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
SENTINEL = {np.dtype(np.float64): -777.25, np.dtype(np.float32): -12345.5, np.dtype(np.int32): -99, np.dtype(np.uint8): 0xAB,
            np.dtype(np.int64): -99}
COUNTED = dict(point_id="n_points", point_status="n_points", point_first_pixel="n_points", point_xyz="n_points", tail_id="n_tail",
               tail_status="n_tail", tail_col="n_tail", tail_pose_mask="n_tail")


def dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def fill_sentinels(out):
    for t in out.m.values():
        t.fill_(SENTINEL[np.dtype(str(t.dtype).split(".")[1])])


def fetch(out):
    import torch
    torch.cuda.synchronize()
    return {k: t.cpu().numpy().copy() for k, t in out.m.items()}


def _gpu_params(c):
    p = c["p"]
    gp = capi.trail_index_default_params(cameraTrailLength=p.cameraTrailLength, cameraTrailHanoiLength=p.cameraTrailHanoiLength,
                                         useStereo=int(p.useStereo), maxTracks=p.maxTracks, maxVisualUpdates=p.maxVisualUpdates,
                                         maxSuccessfulVisualUpdates=p.maxSuccessfulVisualUpdates, trackSampling=p.trackSampling,
                                         trackMinFrames=p.trackMinFrames)
    vp = capi.vu_default_params(imu_to_camera=c["T1"], second_imu_to_camera=c["T2"], useStereo=int(p.useStereo), **c["over"])
    return gp, vp


class Rig:
    """The device side of one corpus case: the index driven by the device's own select and finish, the filter batch holding the
    frame's means, the visit arrays, and the entry's record filled with sentinels."""

    def __init__(self, ctx, c, counters=True):
        import torch
        self.ctx, self.c = ctx, c
        S, M, V = c["S"], c["M"], c["V"]
        self.gp, self.vp = _gpu_params(c)
        self.dt = TI.DevTrail(S, self.gp, c["stereo"])
        self.dt.init(ctx)
        self.gcam = TI._cams(F.PLAIN)[1]
        self.ekf = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=c["trail"]), batch=S)
        n = self.ekf.n
        for b in range(S):
            self.ekf.set_state(b, np.zeros(n), np.eye(n) * 1e-4)
        self.pf = torch.zeros((V, S, 3), dtype=torch.float64, device="cuda")
        self.ready = torch.ones(S, dtype=torch.uint8, device="cuda")
        self.o2s = torch.zeros((S, 16), dtype=torch.float64, device="cuda")
        self.out = capi.FullCloud(S, self.gp, counters=counters)

    def load(self, row, means=None, sync=False):
        """Everything a frame's entries read; then the device's own select. sync: the library runs on another stream than torch."""
        c, dt = self.c, self.dt
        S, V = c["S"], c["V"]
        dt.load_select_inputs(row)
        st, gt = np.full((V, S, 2), T.TRI_NOT_VISITED, np.int32), np.full((V, S), T.NOT_COMPUTED, np.int32)
        pf, sta, ready = np.zeros((V, S, 3)), np.zeros(S, np.uint8), np.zeros(S, np.uint8)
        for s, rec in enumerate(row):
            n = rec["n_cand"]
            st[:n, s, 0], st[:n, s, 1], gt[:n, s], pf[:n, s] = rec["tri"], rec["prep"], rec["gate"], rec["pf"]
            sta[s], ready[s] = rec["stationary"], rec["ready"]
            self.ekf.set_state(s, rec["mean"] if means is None else means[s])
        dt.i["status"].copy_(dev(st)); dt.i["gate"].copy_(dev(gt)); dt.i["stationary"].copy_(dev(sta))
        self.pf.copy_(dev(pf)); self.ready.copy_(dev(ready))
        if sync:
            import torch
            torch.cuda.synchronize()
        dt.select(self.ctx, self.gcam, self.gcam)
        if sync:
            self.ctx.synchronize()

    def frame(self, without=(), o2s=False):
        dt = self.dt
        ptr = dict(draws_dev=dt.i["draws"], full_update_dev=dt.i["full"], cand_id_dev=dt.o["cand_id"], n_candidates_dev=dt.o["n_cand"],
                   status_dev=dt.i["status"], gate_status_dev=dt.i["gate"], pf_dev=self.pf, stationary_dev=dt.i["stationary"],
                   odometry_to_slam_dev=self.o2s if o2s else None, ready_dev=self.ready)
        return capi.full_cloud_frame(**{k: (0 if (k in without or v is None) else v.data_ptr()) for k, v in ptr.items()})

    def run(self, without=(), o2s=False):
        self.ekf.full_point_cloud_dev(self.gp, self.vp, self.dt.trail.table, self.dt.table, self.frame(without, o2s), self.out)

    def everything_else(self):
        """What the entry may only read: means, covariances, the index, the table, the visit arrays."""
        import torch
        torch.cuda.synchronize()
        got = {("index", k): v.cpu().numpy().copy() for k, v in self.dt.trail.m.items()}
        got.update({("table", k): v.cpu().numpy().copy() for k, v in self.dt.t.items() if v is not None})
        got.update({("visit", k): self.dt.i[k].cpu().numpy().copy() for k in ("status", "gate", "draws", "full", "stationary")})
        got.update({("visit", k): self.dt.o[k].cpu().numpy().copy() for k in ("cand_id", "n_cand")})
        for b in range(self.c["S"]):
            got[("mean", b)], got[("cov", b)] = self.ekf.get_state(b)
        return got

    def close(self):
        self.ekf.close()


def _context():
    import torch
    ctx = capi.Context(width=64, height=64, levels=1, pool_size=1)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)     # the tests' torch tensors and the library share one stream
    return ctx


@functools.lru_cache(maxsize=None)
def _outputs(name):
    """The device's record of every judged frame of a case, computed once. Beside the record, for the tests that own them: "wrote" =
    what else differs in device memory after the call (means, covariances, index, table, visit arrays), and on the last frame
    "launches" = (launches, ms) of the two timer classes."""
    c = F.corpus(name)
    frames = []
    with _context() as ctx:
        rig = Rig(ctx, c)
        for f, row in enumerate(c["frames"]):
            rig.load(row)
            if not row[0]["judged"]:                             # a frame that only fills the trail
                frames.append(None)
                rig.dt.finish(ctx)
                continue
            fill_sentinels(rig.out)
            before = rig.everything_else()
            if f == len(c["frames"]) - 1:
                ctx.profile_enable(True)
                ctx.profile_reset()
            rig.run()
            if f == len(c["frames"]) - 1:
                launches = (ctx.profile_read(capi.K_TRAIL_INDEX), ctx.profile_read(capi.K_VU_TRI))
                ctx.profile_enable(False)
            got = fetch(rig.out)
            got["col_id"] = rig.dt.trail.m["col_id"].cpu().numpy().copy()
            got["col_len"] = rig.dt.trail.m["col_len"].cpu().numpy().copy()
            after = rig.everything_else()
            got["wrote"] = [k for k in before if not same_bits(np.asarray(before[k]), np.asarray(after[k]))]
            if f == len(c["frames"]) - 1:
                got["launches"] = launches
            frames.append(got)
            rig.dt.finish(ctx)
        rig.close()
    return frames


@pytest.mark.parametrize("name", list(F.CASES))
def test_the_entry_writes_nothing_but_its_record(name):
    """Means, covariances, every array of the index, the table and the visit arrays are bit-equal before and after the call."""
    judged = [g for g in _outputs(name) if g is not None]
    assert judged
    for g in judged:
        assert g["wrote"] == [], (name, "the entry wrote", g["wrote"])


@pytest.mark.parametrize("name", list(F.CASES))
def test_two_launches_under_the_index_and_the_triangulation_timers(name):
    (ms_i, n_i), (ms_t, n_t) = _outputs(name)[-1]["launches"]
    assert (n_i, n_t) == (1, 1) and ms_i > 0 and ms_t > 0, (name, n_i, ms_i, n_t, ms_t)     # HV_K_TRAIL_INDEX, HV_K_VU_TRI


def _replay(rec, got, s, ready=None, stationary=None):
    """The restatement on the device's own outcomes of the tail: its statuses, and as the point of an OK track what the device put
    into the cloud (the identity transform copies it)."""
    n_tail = int(got["n_tail"][s])
    st = got["tail_status"][s][:n_tail]
    n_ok = int((st == F.TRI_OK).sum())
    n_points = int(got["n_points"][s])
    pts = iter(got["point_xyz"][s][max(n_points - n_ok, 0):n_points]) if (rec["ready"] if ready is None else ready) else iter([np.zeros(3)] * n_ok)
    points = [next(pts) if x == F.TRI_OK else np.zeros(3) for x in st]
    return F.full_cloud(rec["ses"], rec["mean"], list(zip(rec["tri"], rec["prep"])), rec["gate"], rec["pf"],
                        rec["stationary"] if stationary is None else stationary, F.replayed(st, points),
                        ready=rec["ready"] if ready is None else ready)


def _assert_bookkeeping(got, s, rec, r, what, counters=True):
    cloud, tail = r["cloud"], r["tail"]
    assert got["n_points"][s] == len(cloud) and got["n_tail"][s] == len(tail), (what, got["n_points"][s], len(cloud), got["n_tail"][s], len(tail))
    n, nt = len(cloud), len(tail)
    assert np.array_equal(got["point_id"][s][:n], np.array([x[0] for x in cloud], np.int32).reshape(-1)), (what, "point_id")
    assert np.array_equal(got["point_status"][s][:n], np.array([x[1] for x in cloud], np.int32).reshape(-1)), (what, "point_status")
    assert same_bits(got["point_first_pixel"][s][:n], np.array([x[2] for x in cloud], np.float32).reshape(n, 2)), (what, "point_first_pixel")
    assert same_bits(got["point_xyz"][s][:n], np.array([x[3] for x in cloud], np.float64).reshape(n, 3)), (what, "point_xyz of the replay")
    assert np.array_equal(got["tail_id"][s][:nt], np.array([x[0] for x in tail], np.int32).reshape(-1)), (what, "tail_id")
    assert np.array_equal(got["tail_pose_mask"][s][:nt], np.array([F.pose_mask(x[2]) for x in tail], np.int64).reshape(-1)), (what, "tail_pose_mask")
    cols = got["tail_col"][s][:nt]
    assert ((cols >= 0) & (cols < got["col_id"].shape[1])).all() and np.array_equal(got["col_id"][s][cols], got["tail_id"][s][:nt]), (what, "tail_col")
    assert np.array_equal(got["col_len"][s][cols], np.array([x[2][-1] + 1 for x in tail], np.int32).reshape(-1)), (what, "the column's length")
    if counters:
        assert (got["n_attempts"][s], got["good_frame"][s]) == (r["n_attempts"], int(r["good_frame"])), (what, "attempts / goodFrame")
    for k, counter in COUNTED.items():
        behind = got[k][s][int(got[counter][s]):]
        assert (behind == SENTINEL[behind.dtype]).all(), (what, k, "written behind", counter)


@pytest.mark.parametrize("name", list(F.CASES))
def test_integer_and_copied_fields_equal_the_restatement_replayed_on_the_devices_statuses(name):
    c, frames = F.corpus(name), _outputs(name)
    tails = 0
    for f, row in enumerate(c["frames"]):
        for s, rec in enumerate(row):
            if frames[f] is None:
                continue
            _assert_bookkeeping(frames[f], s, rec, _replay(rec, frames[f], s), (name, f, s))
            tails += int(frames[f]["n_tail"][s])
            if not rec["ready"]:
                assert frames[f]["n_points"][s] == 0
    assert tails > 100


@pytest.mark.parametrize("name", list(F.CASES))
def test_tail_status_equals_the_oracle_where_its_two_precisions_agree(name):
    c, frames = F.corpus(name), _outputs(name)
    compared = excluded = 0
    seen = set()
    for f, row in enumerate(c["frames"]):
        for s, rec in enumerate(row):
            if frames[f] is None:
                continue
            got = frames[f]["tail_status"][s]
            assert frames[f]["n_tail"][s] == len(rec["rest"]["tail"]), (name, f, s)
            for k, ((tid, so, _), (_, sl, _)) in enumerate(zip(rec["rest"]["tail"], rec["truth"]["tail"])):
                if so != sl:
                    excluded += 1
                    continue
                assert got[k] == so, (name, f, s, k, tid, "device", int(got[k]), "oracle", so)
                compared += 1
                seen.add(so)
    print(f"{name}: {compared} tail statuses equal the oracle's, {excluded} left out; statuses seen {sorted(seen)}")
    assert compared > 100 and F.TRI_OK in seen and len(seen) >= 2


def _judged_frames(c):
    """Small cases: every frame; the 200-track case: the last frame (~270 tracks of up to 42 observations; an ensemble is 32
    oracle runs with derivatives per track)."""
    n = len(c["frames"])
    return range(n) if c["M"] <= 24 else range(n - 1, n)


@pytest.mark.parametrize("name", list(F.CASES))
def test_points_within_the_budget_of_the_visual_fronts_accuracy_rule(name):
    c, frames = F.corpus(name), _outputs(name)
    par, T1, T2 = c["par"], c["T1"], c["T2"]
    jobs = []
    for f in _judged_frames(c):
        for s, rec in enumerate(c["frames"][f]):
            if not rec["ready"]:
                continue
            got = frames[f]
            n_tail, n_points = int(got["n_tail"][s]), int(got["n_points"][s])
            st = got["tail_status"][s][:n_tail]
            first = n_points - int((st == F.TRI_OK).sum())
            # the prefix is a copy of pf_dev (the identity transform: x * 1 + y * 0 + z * 0 + 0)
            want = np.array([p for _, _, _, p in rec["rest"]["cloud"]][:first], np.float64).reshape(first, 3)
            assert same_bits(got["point_xyz"][s][:first], want), (name, f, s, "prefix")
            k_ok = 0
            for k, (index, feat, vel) in enumerate(rec["tail_inputs"]):
                if st[k] == F.TRI_OK:
                    jobs.append(((f, s, k), rec["mean"], index, feat, vel, got["point_xyz"][s][first + k_ok].copy(), rec["rest"]["tail"][k][1]))
                    k_ok += 1
    ens = vt.in_threads(lambda j: vt.Ensemble(par, j[1], j[2], T1, T2, j[3], j[4], [sum(name.encode()), *j[0]]), jobs)
    J = vt.Judge(f"full cloud {name}")
    compared = bit_equal = worst = 0
    for j, e in zip(jobs, ens):
        if not e.ok or e.excluded or j[6] != F.TRI_OK:
            continue
        r = e.ratio_pf(j[5])
        worst = max(worst, r)
        J.fail_if(not r <= vt.FACTOR, f"{name}{j[0]}: pf at {r:.3g} x the scale (bar {vt.FACTOR:g})")
        bit_equal += int(same_bits(j[5], np.asarray(e.o_pf, np.float64)))
        compared += 1
    print(f"ACC full cloud {name}: {compared} points compared of {len(jobs)} OK tail tracks, worst {worst:.3g} x the scale (bar {vt.FACTOR:g}); "
          f"{bit_equal} of {compared} points bit-equal to the binary64 oracle")
    J.fail_if(compared < len(jobs) // 2 or compared == 0, f"only {compared} of {len(jobs)} compared")
    J.done()


def test_odometry_to_slam_within_eight_times_the_restatements_own_error():
    """The same frames with a transform per set: every point is transformVec3ByMat4(odometryToSlam, the point without it)."""
    name = "stereo_gap"
    c, base = F.corpus(name), _outputs(name)
    _, _, o2s = OR.slam_transforms()
    S = c["S"]
    mats = np.stack([np.asarray(o2s[s % len(o2s)], np.float64).reshape(16) for s in range(S)])
    checked = 0
    with _context() as ctx:
        rig = Rig(ctx, c)
        rig.o2s.copy_(dev(mats))
        for f, row in enumerate(c["frames"]):
            rig.load(row)
            fill_sentinels(rig.out)
            rig.run(o2s=True)
            got = fetch(rig.out)
            rig.dt.finish(ctx)
            for k in ("n_points", "point_id", "point_status", "point_first_pixel", "n_tail", "tail_id", "tail_status", "tail_col",
                      "tail_pose_mask", "n_attempts", "good_frame"):
                assert same_bits(got[k], base[f][k]), (f, k)
            for s in range(S):
                for i in range(int(got["n_points"][s])):
                    pf = base[f]["point_xyz"][s][i]
                    rest = np.array(OR.transformVec3ByMat4([np.float64(x) for x in mats[s]], [np.float64(x) for x in pf]), np.float64)
                    truth = np.array(OR.transformVec3ByMat4([LD(x) for x in mats[s]], [LD(x) for x in pf]), LD)
                    L = np.abs(truth).max()
                    err, own = np.abs(got["point_xyz"][s][i].astype(LD) - truth), np.abs(rest.astype(LD) - truth)
                    assert (err <= 8 * own + 64 * LD(U) * L).all(), (f, s, i, err, own)
                    checked += 1
        rig.close()
    assert checked > 100


def test_optional_arrays_may_be_null():
    """full_update_dev NULL: every frame is full; stationary_dev NULL: 0; odometry_to_slam_dev NULL: the identity; ready_dev NULL:
    every set is ready; n_attempts / good_frame NULL: not written."""
    name = "mono_all"
    c = F.corpus(name)
    clouds = 0
    with _context() as ctx:
        rig = Rig(ctx, c, counters=False)
        for f, row in enumerate(c["frames"]):
            rig.load(row)
            fill_sentinels(rig.out)
            rig.run(without=("full_update_dev", "stationary_dev", "ready_dev"))
            got = fetch(rig.out)
            got["col_id"], got["col_len"] = rig.dt.trail.m["col_id"].cpu().numpy(), rig.dt.trail.m["col_len"].cpu().numpy()
            rig.dt.finish(ctx)
            for s, rec in enumerate(row):
                # (a frame that is not full has no candidate, hence no stop and no tail, whatever the entry is told)
                r = _replay(rec, got, s, ready=True, stationary=False)
                _assert_bookkeeping(got, s, rec, r, (f, s), counters=False)
                clouds += (not rec["ready"]) and got["n_points"][s] > 0
            assert (got["n_attempts"] == SENTINEL[np.dtype(np.int32)]).all() and (got["good_frame"] == SENTINEL[np.dtype(np.uint8)]).all()
        rig.close()
    assert clouds > 0                                            # the set that is not ready has a cloud now


def test_a_non_finite_mean_stays_in_its_set():
    name = "stereo_gap"
    c, clean = F.corpus(name), _outputs(name)
    f = len(c["frames"]) - 1
    bad = 0
    poisons = {"NaN in the current orientation": (F.ORI + 1, np.nan), "inf in the current position": (F.POS, np.inf),
               "NaN in the position of history pose 1": (F.CAM + 7 + 1, np.nan)}
    with _context() as ctx:
        rig = Rig(ctx, c)
        for g, row in enumerate(c["frames"][:f]):                # the index of the last frame: every frame before it, select and finish
            rig.dt.load_select_inputs(row)
            rig.dt.select(ctx, rig.gcam, rig.gcam)
            st = np.full((c["V"], c["S"], 2), T.TRI_NOT_VISITED, np.int32); gt = np.full((c["V"], c["S"]), T.NOT_COMPUTED, np.int32)
            sta = np.zeros(c["S"], np.uint8)
            for s, rec in enumerate(row):
                n = rec["n_cand"]
                st[:n, s, 0], st[:n, s, 1], gt[:n, s], sta[s] = rec["tri"], rec["prep"], rec["gate"], rec["stationary"]
            rig.dt.i["status"].copy_(dev(st)); rig.dt.i["gate"].copy_(dev(gt)); rig.dt.i["stationary"].copy_(dev(sta))
            rig.dt.finish(ctx)
        row = c["frames"][f]
        assert len(row[bad]["rest"]["tail"]) > 0
        saved = {k: v.clone() for k, v in rig.dt.trail.m.items()}
        for what, (entry, value) in poisons.items():
            for k, v in rig.dt.trail.m.items():                  # the index as finish left it: select runs again on the same state
                v.copy_(saved[k])
            means = [rec["mean"].copy() for rec in row]
            means[bad][entry] = value
            rig.load(row, means=means)
            fill_sentinels(rig.out)
            rig.run()
            got = fetch(rig.out)
            for s in range(c["S"]):
                if s != bad:
                    for k in got:
                        assert same_bits(got[k][s], clean[f][k][s]), (what, s, k)
            n_tail = int(got["n_tail"][bad])
            assert n_tail == len(row[bad]["rest"]["tail"]), what
            assert not same_bits(got["tail_status"][bad][:n_tail], clean[f]["tail_status"][bad][:n_tail]), (what, "no status changed")
            if "current" in what:                                # pose 0 is every track's
                assert (got["tail_status"][bad][:n_tail] != F.TRI_OK).all(), what
            for k in ("n_tail", "tail_id", "tail_col", "tail_pose_mask", "n_attempts", "good_frame"):    # the bookkeeping of the poisoned set holds
                assert same_bits(got[k][bad], clean[f][k][bad]), (what, k)
        rig.close()


def test_limits_that_need_the_handle():
    import ctypes as C
    c = F.corpus("stereo_gap")
    with _context() as ctx:
        rig = Rig(ctx, c)
        frame = rig.frame()
        longer = capi.trail_index_default_params(cameraTrailLength=c["trail"] + 1, cameraTrailHanoiLength=2, useStereo=1, maxTracks=c["M"],
                                                 maxVisualUpdates=c["V"])

        def call(tp, out=rig.out.table):
            return capi.lib().hv_full_point_cloud_dev(rig.ekf._h, C.byref(tp), C.byref(rig.vp), C.byref(rig.dt.trail.table), C.byref(rig.dt.table),
                                                      C.byref(frame), C.byref(out) if out is not None else None)

        assert call(longer) == -2 and call(longer, out=None) == -1           # a state shorter than the trail: unsupported; invalid wins
        rig.close()


# ---- chain -------------------------------------------------------------------------------------------------------------------

def test_chain_on_device_produced_state():
    """select -> hv_ekf_visual_frame_ragged_dev -> the entry -> finish -> augmentation -> hv_output_dev over four frames, the visits
    the filter's own. A host Session runs beside the device on the same tables and is fed the device's statuses, so the restatement
    sees the frame's device state: the mean as the updates left it, read back in front of the entry. The cloud of hv_output_dev is a
    prefix of the entry's, minus the stopping candidate."""
    import torch
    import test_gpu_output as GO
    trail, frames = 3, 4
    S, M, V = GO.S, GO.M, GO.V
    K = trail + 1
    T1, T2, poses, tables, draws = GO._chain_world(trail, frames)
    kw = dict(cameraTrailLength=trail, cameraTrailHanoiLength=min(3, trail - 2), maxTracks=M, maxVisualUpdates=V, maxSuccessfulVisualUpdates=2,
              trackMinFrames=2, scoreVisualUpdateTracks=0, useStereo=1)
    gp = capi.trail_index_default_params(**kw)
    hp = T.Params(**{k: (bool(v) if k in ("useStereo", "scoreVisualUpdateTracks") else v) for k, v in kw.items()})
    op = GO.gpu_params(OR.Params(trail, M, V, 2, True, T1))
    ocam, gcam = TI._cams(TI.PLAIN)
    vp = capi.vu_default_params(imu_to_camera=T1, second_imu_to_camera=T2)
    par = F.orc.tri_default_params()
    tri_rest, tri_truth = F.oracle_points(par, T1, T2), F.oracle_long_double(par, T1, T2)
    import ransac3_restatement as R3
    hosts = [T.Session(hp, R3.normalize_pixel) for _ in range(S)]
    z = lambda shape, dtp: torch.zeros(shape, dtype=dtp, device="cuda")
    P_ = lambda x: x.data_ptr()
    seen = dict(tail=0, points=0, stopped=0, stop_pushed=0, statuses=0)
    with _context() as ctx:
        g = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=trail), S)
        for b in range(S):
            m = np.zeros(g.n); m[16:19] = 1.0
            for k in range(trail):
                m[OR.CAM + 7 * k + 3] = 1.0
            m[OR.POS:OR.POS + 3], m[OR.ORI:OR.ORI + 4] = poses[b][0]
            g.set_state(b, m, np.eye(g.n) * 1e-4)
        dt = TI.DevTrail(S, gp, True)
        dt.init(ctx)
        ses = capi.session_state(S, 4)
        st, gs, cnt, pf = z((V, S, 2), torch.int32), z((V, S), torch.int32), z(S, torch.int32), z((V, S, 3), torch.float64)
        status = z(S, torch.int32)
        out, cloud = capi.Output(S, op), capi.FullCloud(S, gp)
        oframe = capi.output_frame(cand_id_dev=P_(dt.o["cand_id"]), n_candidates_dev=P_(dt.o["n_cand"]), status_dev=P_(st), gate_status_dev=P_(gs),
                                   pf_dev=P_(pf), tracking_status_dev=P_(status), stationary_dev=P_(dt.i["stationary"]))
        cframe = capi.full_cloud_frame(draws_dev=P_(dt.i["draws"]), full_update_dev=P_(dt.i["full"]), cand_id_dev=P_(dt.o["cand_id"]),
                                       n_candidates_dev=P_(dt.o["n_cand"]), status_dev=P_(st), gate_status_dev=P_(gs), pf_dev=P_(pf),
                                       stationary_dev=P_(dt.i["stationary"]))
        for f in range(frames):
            for b in range(S):                                   # the frame's IMU propagation, scripted: the true pose of the frame
                m, _ = g.get_state(b)
                m[OR.POS:OR.POS + 3], m[OR.ORI:OR.ORI + 4] = poses[b][f]
                g.set_state(b, m)
            frs = [dict(table=tables[s][f], keyframe=True, full=True, frame_num=f + 1, time=0.5 * f, draws=draws[f, s]) for s in range(S)]
            dt.load_select_inputs(frs)
            dt.select(ctx, gcam, gcam)
            o = dt.o
            g.visual_frame_ragged_dev(vp, V, K, P_(o["n_poses"]), P_(o["pose_index"]), P_(o["features"]), P_(o["velocities"]), P_(o["y"]), 1.5, 0.05,
                                      P_(st), P_(gs), P_(cnt), 2, pf_dev=P_(pf))
            torch.cuda.synchronize()
            means = [g.get_state(b)[0] for b in range(S)]        # as the frame's updates left it
            fill_sentinels(cloud)
            g.full_point_cloud_dev(gp, vp, dt.trail.table, dt.table, cframe, cloud)
            got = fetch(cloud)
            got["col_id"], got["col_len"] = dt.trail.m["col_id"].cpu().numpy(), dt.trail.m["col_len"].cpu().numpy()
            dt.finish(ctx, status=st, gate=gs)
            g.symmetrize_augment_dev(P_(o["discarded"]))
            g.output_dev(op, ses, dt.trail.table, oframe, out)
            small = GO.fetch(out)
            h_st, h_gs, h_pf, h_n = st.cpu().numpy(), gs.cpu().numpy(), pf.cpu().numpy(), o["n_cand"].cpu().numpy()
            for s in range(S):
                host = hosts[s]
                sel = host.select(tables[s][f], (ocam, ocam), True, True, f + 1, 0.5 * f, draws[f, s])
                n = int(h_n[s])
                assert n == len(sel["candidates"]), (f, s)
                stat = [tuple(int(x) for x in h_st[v, s]) for v in range(n)]
                gate = [int(h_gs[v, s]) for v in range(n)]
                rec = dict(ses=host, mean=means[s], tri=[x[0] for x in stat], prep=[x[1] for x in stat], gate=gate, pf=h_pf[:n, s],
                           stationary=False, ready=True)
                _assert_bookkeeping(got, s, rec, _replay(rec, got, s), ("chain", f, s))
                rest = F.full_cloud(host, means[s], stat, gate, h_pf[:n, s], False, tri_rest)
                truth = F.full_cloud(host, means[s], stat, gate, h_pf[:n, s], False, tri_truth)
                for k, ((_, so, _), (_, sl, _)) in enumerate(zip(rest["tail"], truth["tail"])):
                    if so == sl:
                        assert got["tail_status"][s][k] == so, ("chain", f, s, k)
                        seen["statuses"] += 1
                # hv_output_dev's cloud: the same prefix without the stopping candidate
                n_small, n_tail_ok = int(small["n_points"][s]), int((got["tail_status"][s][:len(rest["tail"])] == F.TRI_OK).sum())
                n_prefix = int(got["n_points"][s]) - n_tail_ok
                assert n_prefix - n_small in (0, 1) and (rest["stopped"] or n_prefix == n_small), ("chain", f, s, n_prefix, n_small)
                for k in ("point_id", "point_status", "point_first_pixel", "point_xyz"):
                    assert same_bits(got[k][s][:n_small], small[k][s][:n_small]), ("chain", f, s, k)
                seen["tail"] += len(rest["tail"]); seen["points"] += int(got["n_points"][s]); seen["stopped"] += rest["stopped"]
                seen["stop_pushed"] += n_prefix - n_small
                host.finish([x[0] for x in stat], gate, False)
        g.close()
    print("chain:", seen)
    assert seen["tail"] > 0 and seen["stopped"] > 0 and seen["stop_pushed"] > 0 and seen["statuses"] > 0


# ---- capture -----------------------------------------------------------------------------------------------------------------

def test_captured_entry_replays_bit_equal():
    """Only the entry inside torch.cuda.graph on a lane's stream; replayed twice from restored inputs and sentinels, bit-equal to
    the eager call."""
    import torch
    name = "stereo_gap"
    c = F.corpus(name)
    f = len(c["frames"]) - 1
    with capi.Lanes(1, width=64, height=64) as lanes:
        ctx = lanes.ctx[0]
        stream = torch.cuda.ExternalStream(ctx.get_stream())
        rig = Rig(ctx, c)
        for row in c["frames"][:f + 1]:                          # the index of the last frame, on the lane's stream
            rig.load(row, sync=True)
            if row is not c["frames"][f]:
                rig.dt.finish(ctx)
                ctx.synchronize()
        ctx.synchronize(); torch.cuda.synchronize()
        saved = {k: v.clone() for k, v in rig.dt.trail.m.items()}
        mean = [rec["mean"] for rec in c["frames"][f]]

        def restore():
            """The torch work runs on the default stream, the library's on the lane's: synchronised in between."""
            fill_sentinels(rig.out)
            for k, v in rig.dt.trail.m.items():
                v.copy_(saved[k])
            for s, m in enumerate(mean):
                rig.ekf.set_state(s, m)
            ctx.synchronize()
            torch.cuda.synchronize()

        restore()
        with torch.cuda.stream(stream):
            rig.run()
        ctx.synchronize()
        eager = fetch(rig.out)
        assert eager["n_tail"].max() > 0 and eager["n_points"].max() > 0
        restore()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            rig.run()
        for rep in range(2):
            restore()
            graph.replay()
            got = fetch(rig.out)
            for k in eager:
                assert same_bits(got[k], eager[k]), (rep, k)
        del graph
        rig.close()
