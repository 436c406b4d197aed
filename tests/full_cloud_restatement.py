"""Literal restatement of the visit loop of Session::trackerVisualUpdate (src/odometry/backend.cpp:1012-1252, 1269-1274) with
odometry.fullPointCloud on, the yardstick of hv_full_point_cloud_dev. It is built on trail_index_restatement.Session after its
select(): the walk, the candidates, createTrackIndex and buildTrackVectors are that file's; the visits themselves belong to the
filter and are replayed from their outcomes, as in Session.finish(). What is new here is what fullPointCloud changes: the loop
does not break at its limits (:1242-1247), the stopping candidate reaches the push at :1249-1251, and every later track of the
order that passes the filter of :1017-1038 is triangulated from the current mean (:1048-1099), counted (:1121) and appended when
OK (:1126-1132). The triangulation is a callable, so that the same text runs with the oracle in binary64 (with and without
derivatives), with its long-double build, and with a device's own statuses and points replayed.

corpus() at the end is the seeded, generated corpus the CPU and the GPU tests share. Nothing here reads the reference tree."""
import copy
import functools
import math

import numpy as np

import ransac3_restatement as R3
import trail_index_restatement as T
from oracle import orc
from output_restatement import transformVec3ByMat4

TRI_OK, TRI_BEHIND, TRI_BAD_COND, TRI_NO_CONVERGENCE, TRI_BAD_DEPTH, TRI_UNKNOWN_PROBLEM = 0, 2, 3, 4, 5, 6
PREPARE_VU_OK = 0
POINT_POSE_TRAIL, POINT_OUTLIER = 1, 4                                                  # PointFeature::Status
POS, ORI, CAM, POSE_DIM = 0, 6, 20, 7


# ---- the triangulation of one track: (mean, poseTrailIndex, imageFeatures, featureVelocities) -> (status, pf) ------------------------
def _depth_window(par, st, pf, p0):                                                     # backend.cpp:1096-1099
    dx, dy, dz = pf[0] - p0[0], pf[1] - p0[1], pf[2] - p0[2]
    depth = math.sqrt(dx * dx + dy * dy + dz * dz)
    if depth < par.triangulationMinDist or depth > par.triangulationMaxDist:
        st = TRI_BAD_DEPTH
    return st


def oracle_points(par, T1, T2):
    """Triangulator::triangulate WITHOUT derivatives, then the depth window: what the device's points-only kernel restates."""
    def tri(m, index, feat, vel):
        trail = orc.extract_camera_pose_trail(m, index, T1, T2)
        st, pf, _, _, _ = orc.triangulate(par, trail, feat, vel, stereo=T2 is not None, calc_derivatives=False)
        return _depth_window(par, st, pf, trail[0].p), pf
    return tri


def oracle_with_derivatives(par, T1, T2):
    """The per-track glue as the reference runs it, calculateDerivatives = true (backend.cpp:1084-1099)."""
    def tri(m, index, feat, vel):
        st, _, pf, _, _ = orc.visual_track_prepare(par, m, index, T1, T2, feat, vel)
        return st, pf
    return tri


def oracle_long_double(par, T1, T2):
    """The same source with real = long double: the truth."""
    def tri(m, index, feat, vel):
        st, _, pf, _, _ = orc.visual_track_prepare_as("ld", par, m, index, T1, T2, feat, vel)
        return st, pf
    return tri


def replayed(statuses, points):
    """The outcomes of the tail in tail order, from whoever computed them (a device): separates the bookkeeping from the arithmetic."""
    it = iter(zip(statuses, points))

    def tri(m, index, feat, vel):
        st, pf = next(it)
        return int(st), np.asarray(pf)
    return tri


# ---- the loop --------------------------------------------------------------------------------------------------------------------------
def full_cloud(ses, mean, status, gate, pf_visit, stationary, triangulate, ready=True, odometry_to_slam=None, real=np.float64):
    """backend.cpp:1012-1252 with fullPointCloud, over a Session whose select() has run and whose finish() has not. status [v] =
    (TriangulatorStatus, PrepareVuStatus), gate [v] = VuOutlierStatus and pf_visit [v] of the candidates, as the filter's visit
    loop left them (TRI_NOT_VISITED: the filter did not visit it). -> the cloud [(id, PointFeature::Status, firstPixel, point)],
    the tail [(id, TriangulatorStatus, poseTrailIndex)], updateAttemptCount, goodFrame."""
    p, idx = ses.p, ses.ekfStateIndex
    head = idx.headKeyFrame()
    o2s = None if odometry_to_slam is None else [real(x) for x in odometry_to_slam]
    cloud, tail = [], []
    updateAttemptCount = updateSuccessCount = 0                                         # :902-903
    needMoreVisualUpdates = True                                                        # :999

    def push(trackId, point_status, pf):
        firstPixel = np.asarray(head.features[trackId].frames[0].imagePoint, np.float32)   # track.points[0] (:1069)
        point = [real(x) for x in pf]
        if o2s is not None:
            with np.errstate(all="ignore"):
                point = transformVec3ByMat4(o2s, point)                                 # getPointCloud (:278)
        cloud.append((int(trackId), point_status, firstPixel, point))

    for pos, (kind, arg) in enumerate(ses.walk):                                        # :1012
        trackId = ses.track_ids[pos]
        if kind in ("score", "short", "lite"):                                          # :1022-1034: whatever the loop's state
            continue
        if kind == "blacklisted" and needMoreVisualUpdates:                             # :1039-1046
            continue
        if needMoreVisualUpdates:
            if kind != "candidate" or status[arg][0] == T.TRI_NOT_VISITED:
                continue
            point_status = POINT_POSE_TRAIL                                             # :1118
            updateAttemptCount += 1                                                     # :1121
            if status[arg][1] == PREPARE_VU_OK and status[arg][0] == TRI_OK:            # :1152-1153
                if gate[arg] == T.INLIER:
                    updateSuccessCount += 1                                             # :1188
                else:
                    point_status = POINT_OUTLIER                                        # :1191
            limitSuccessful = p.maxSuccessfulVisualUpdates > 0 and updateSuccessCount >= p.maxSuccessfulVisualUpdates   # :1240
            limitTotal = p.maxVisualUpdates > 0 and updateAttemptCount >= p.maxVisualUpdates                           # :1241
            if limitSuccessful or limitTotal:
                needMoreVisualUpdates = False                                           # :1243; fullPointCloud: no break
            if status[arg][0] == TRI_OK:                                                # :1249-1251
                push(trackId, point_status, pf_visit[arg])
            continue
        # ---- behind the stop: blacklisted or not, a candidate or not (:1048-1132) ----
        poseTrailIndex = idx.createTrackIndex(trackId, p.trackSampling)                 # :1017
        imageFeatures, featureVelocities, _ = idx.buildTrackVectors(trackId, poseTrailIndex, p.useStereo)   # :1051-1052
        triangulateStatus, pf = triangulate(mean, poseTrailIndex, imageFeatures, featureVelocities)        # :1055-1099
        updateAttemptCount += 1                                                         # :1121
        tail.append((int(trackId), int(triangulateStatus), list(poseTrailIndex)))
        if triangulateStatus == TRI_OK:                                                 # :1127-1129
            push(trackId, POINT_POSE_TRAIL, pf)
    tooManyFailures = updateAttemptCount - updateSuccessCount > T.FAILED_UPDATES_THRESHOLD   # :1273
    goodFrame = (bool(stationary) or not needMoreVisualUpdates) and not tooManyFailures      # :1274
    if not ready:                                                                       # getPointCloud (:255-280): empty until ready
        cloud = []
    return dict(cloud=cloud, tail=tail, n_attempts=updateAttemptCount, successes=updateSuccessCount, good_frame=goodFrame,
                stopped=not needMoreVisualUpdates)


def pose_mask(index):
    return sum(1 << int(k) for k in index)


# ---- the corpus ------------------------------------------------------------------------------------------------------------------------
PLAIN = dict(kind="pinhole", fx=458.6, fy=457.3, ppx=367.2, ppy=248.4)
RIC = np.array([[0.0, -1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])
BASE2 = np.array([0.11, 0.002, -0.001])
NOT_READY, NEVER_STOPS, NO_TRACKS, ONE_TRACK = 4, 3, 1, 2                                 # the roles of the sets of a five-set case
# name: n_sets, maxTracks, trail, V, successes, stereo, sampling, frames, triangulation overrides
CASES = {
    "stereo_gap": (5, 24, 6, 4, 2, True, T.GAP, 14, {}),
    "mono_all": (5, 24, 6, 4, 2, False, T.ALL, 14, {}),
    "defaults": (3, 200, 20, 20, 5, True, T.GAP, 23, {}),
    "trail24_depth": (2, 24, 24, 4, 2, True, T.ALL, 28, dict(triangulationMinDist=4.0, triangulationMaxDist=9.0)),
}
NOT_FULL_FRAME, JUMP_FRAMES = 9, (10, 11, 12, 13)
JUDGED_LAST = 2                                                                         # the 200-track case: the frames that are evaluated
STATIC = 1e-6                                                                           # the motion scale of the mono case's standing camera


def extrinsics(stereo):
    T1 = np.eye(4); T1[:3, :3] = RIC
    T2 = T1.copy(); T2[:3, 3] = BASE2
    return T1, (T2 if stereo else None)


def quat2rmat(q):
    return orc.quat2rmat_d(np.asarray(q, np.float64))[0]


def _quat_mul(a, b):
    w0, x0, y0, z0 = a; w1, x1, y1, z1 = b
    return np.array([w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1, w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1,
                     w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1, w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1])


def _trajectory(rng, frames, scale=1.0):
    """A smooth trajectory: a drifting position with a sideways sway (parallax) and a slowly turning orientation. scale: of the
    motion (a camera that all but stands still gives a mono track almost no baseline: BAD_COND)."""
    p0, vel = rng.uniform(-2, 2, 3), rng.normal(size=3) * 0.08
    q0 = rng.normal(size=4); q0 /= np.linalg.norm(q0)
    axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
    out = []
    for f in range(frames):
        a = 0.012 * f
        dq = np.concatenate([[math.cos(a / 2)], math.sin(a / 2) * axis])
        q = _quat_mul(q0, dq)
        q /= np.linalg.norm(q)
        Rf = RIC @ quat2rmat(q)
        sway = Rf.T @ np.array([0.25 * math.sin(0.7 * f), 0.2 * math.cos(0.5 * f), 0.0])
        out.append((p0 + scale * (f * vel + sway), q))
    return out


def _project(pose, pw, cam):
    p, q = pose
    Rf = RIC @ quat2rmat(q)
    pc = Rf @ (pw - (p - Rf.T @ (BASE2 if cam else np.zeros(3))))
    return PLAIN["fx"] * pc[0] / pc[2] + PLAIN["ppx"], PLAIN["fy"] * pc[1] / pc[2] + PLAIN["ppy"]


def _new_point(rng, pose, kind):
    """A world point in front of the camera at `pose`: near (most), far (almost no baseline: BAD_COND)."""
    p, q = pose
    Rf = RIC @ quat2rmat(q)
    depth = rng.uniform(3, 10) if kind != "far" else rng.uniform(2e4, 1e5)
    return p + Rf.T @ (np.array([rng.uniform(-0.45, 0.45), rng.uniform(-0.3, 0.3), 1.0]) * depth)


def mean_of(ses, trail, rng_noise=None):
    """The filter mean whose pose trail is the poses stamped on the index's keyframes: keyframe 0 is the current pose, keyframe k
    history pose k - 1 (ekf.cpp:544-554)."""
    m = np.zeros(CAM + POSE_DIM * trail)
    m[16:19] = 1.0
    for k in range(trail):
        m[CAM + POSE_DIM * k + 3] = 1.0
    for k, kf in enumerate(ses.ekfStateIndex.keyframes):
        if getattr(kf, "pose", None) is None:
            continue
        ip, io = (POS, ORI) if k == 0 else (CAM + POSE_DIM * (k - 1), CAM + POSE_DIM * (k - 1) + 3)
        m[ip:ip + 3], m[io:io + 4] = kf.pose
    return m


@functools.lru_cache(maxsize=None)
def corpus(name):
    """Per frame and set of the case: the inputs of select (table, keyframe, full, frame_num, time, draws), the mean, the synthetic
    outcomes of the visit loop (tri, prep, gate, pf, stationary), the Session as select left it ("ses"), and the restatement's result with the
    oracle without derivatives ("rest"), with them ("rest_d") and in long double ("truth") -- in the 200-track case on the last
    JUDGED_LAST frames only ("judged"), the earlier ones fill the trail. -> dict(par, vu, T1, T2, frames[f][s])."""
    S, M, trail, V, succ, stereo, sampling, frames, over = CASES[name]
    rng = np.random.default_rng([sum(name.encode()), 2026])
    p = T.Params(cameraTrailLength=trail, cameraTrailHanoiLength=min(3, trail - 2), useStereo=stereo, maxTracks=M, maxVisualUpdates=V,
                 maxSuccessfulVisualUpdates=succ, trackSampling=sampling, trackMinFrames=3)
    par = orc.tri_default_params(**over)
    T1, T2 = extrinsics(stereo)
    cam = orc.Camera(PLAIN["kind"], PLAIN["fx"], PLAIN["fy"], PLAIN["ppx"], PLAIN["ppy"])
    tris = dict(rest=oracle_points(par, T1, T2), rest_d=oracle_with_derivatives(par, T1, T2), truth=oracle_long_double(par, T1, T2))
    sessions = [T.Session(p, R3.normalize_pixel) for _ in range(S)]
    five = S == 5
    trajs = [_trajectory(rng, frames, STATIC if (five and not stereo and s == NOT_READY) else 1.0) for s in range(S)]
    tracks = [[] for _ in range(S)]                                                     # [id, world point, kind]
    next_id = [1000 * s + 1 for s in range(S)]
    out = []
    for f in range(frames):
        row = []
        for s, ses in enumerate(sessions):
            pose = trajs[s][f]
            full = not (five and s == 0 and f == NOT_FULL_FRAME)
            keyframe = full and not (f % 6 == 4 and trail < 20)                         # a popped head now and then (backend.cpp:790)
            # ---- the table: drop, append ----
            tracks[s] = [tr for tr in tracks[s] if rng.random() > (0.02 if trail >= 20 else 0.08)]
            target = 0 if (five and s == NO_TRACKS) else 1 if (five and s == ONE_TRACK) else M if f % 4 == 0 else int(rng.integers(M // 2, M + 1))
            while len(tracks[s]) < target:
                r = rng.random()
                kind = "far" if r < 0.08 else "wild" if r < 0.2 else "near"
                tracks[s].append([next_id[s], _new_point(rng, pose, kind), kind])
                next_id[s] += 1
            table = []
            for tid, pw, kind in tracks[s]:
                px = []
                for c in range(2 if stereo else 1):
                    x, y = _project(pose, pw, c)
                    sigma = 0.3 if kind != "wild" else 12.0                              # wild: pixels no point explains (BEHIND, NO_CONVERGENCE)
                    px.append((np.float32(x + rng.normal() * sigma), np.float32(y + rng.normal() * sigma)))
                table.append((tid, px[0], px[1] if stereo else None))
            draws = rng.integers(0, 2 ** 32, M, dtype=np.uint32)
            t = 0.05 * (f + 1)
            sel = ses.select(table, (cam, cam), keyframe, full, f + 1, t, draws)
            ses.ekfStateIndex.headKeyFrame().pose = (pose[0].copy(), pose[1].copy())
            mean = mean_of(ses, trail)
            if five and s == 0 and f in JUMP_FRAMES and len(ses.ekfStateIndex.keyframes) > 3:   # a trail with a jump (NO_CONVERGENCE)
                Rj = RIC @ quat2rmat(mean[CAM + 3:CAM + 7])                              # history pose 0 leaps 12 m along its own view
                mean[CAM:CAM + 3] += 12.0 * (Rj.T @ np.array([0.1, 0.0, 1.0]))
            # ---- the visit loop's outcomes, synthetic: the visits belong to the filter ----
            n_cand = len(sel["candidates"])
            mode = "early" if (five and s == NEVER_STOPS) or (not five and f % 7 == 3 and s == 0) else "limits"
            tri, gate = T.synthetic_outcomes(rng, p, n_cand, mode)
            if mode == "early" and n_cand:                                              # never stops: the last candidate stays unvisited
                tri[-1], gate[-1] = T.TRI_NOT_VISITED, T.NOT_COMPUTED
            prep = [PREPARE_VU_OK if x == TRI_OK else (T.TRI_NOT_VISITED if x == T.TRI_NOT_VISITED else int(rng.integers(0, 3))) for x in tri]
            status = list(zip(tri, prep))
            pf = rng.normal(size=(n_cand, 3)) * 5.0
            stationary = bool(rng.random() < 0.3)
            ready = not (five and s == NOT_READY)
            o2s = None
            rec = dict(table=table, keyframe=keyframe, full=full, frame_num=f + 1, time=t, draws=draws, mean=mean, tri=tri, prep=prep,
                       gate=gate, pf=pf, stationary=stationary, ready=ready, n_cand=n_cand, walk=list(ses.walk), ids=list(ses.track_ids),
                       blacklist_prev=list(ses.blacklistedPrev), cand_pos=[c["pos"] for c in sel["candidates"]])
            # the 200-track case needs 21 frames to grow tracks of full length: the earlier ones only drive the index
            rec["judged"] = M <= 24 or f >= frames - JUDGED_LAST
            for k, tri_fn in tris.items():
                if not rec["judged"]:
                    break
                rec[k] = full_cloud(ses, mean, status, gate, pf, stationary, tri_fn, ready=ready, odometry_to_slam=o2s,
                                    real=np.longdouble if k == "truth" else np.float64)
            # what the GPU test needs to judge a tail track's point: its inputs
            idx = ses.ekfStateIndex
            rec["tail_inputs"] = []
            for tid, _, index in (rec["rest"]["tail"] if rec["judged"] else []):
                ft, vl, _ = idx.buildTrackVectors(tid, index, p.useStereo)
                rec["tail_inputs"].append((list(index), np.array(ft), np.array(vl)))
            if rec["judged"]:
                rec["ses"] = copy.deepcopy(ses)                                          # as select left it: full_cloud() can run again on it
            fin = ses.finish(tri, gate, stationary)
            rec["finish"] = fin
            gone = set(fin["delete_ids"])
            tracks[s] = [tr for tr in tracks[s] if tr[0] not in gone or rng.random() < 0.6]
            row.append(rec)
        out.append(row)
    return dict(par=par, p=p, over=dict(over), T1=T1, T2=T2, frames=out, S=S, M=M, trail=trail, V=V, stereo=stereo)
