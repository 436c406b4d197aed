"""The call-by-call chain the resident VIO engine's sessions are compared against (tests/test_gpu_vio_sessions.py): every stage of
a frame issued one by one from Python on the chain's own buffers, in the order of INTEGRATION.md "One call per frame", for whichever
session hv_vio_create_session would build from the same parameters. What the engine keeps in device memory is kept here on the
host: the slot roles, the frame number, "has a previous frame", full_update (the literal rule of backend.cpp:765) and the choice of
filter and detector (ransac_pipeline.cpp:119-136, restated in session_of). Scenes, parameters and shapes are those of the default
session's test: 376 x 240, maxTracks 120, gfttMinDistance 8, two sets, ten IMU samples per frame."""
import ctypes as C
import functools

import numpy as np

from hybvio_amd import capi, scene

W_, H_, M, S, NS, FPS = 376, 240, 120, 2, 10, 20.0
RIG = scene.Rig(width=W_, height=H_)
TRAJ = [scene.Trajectory(amp=(0.12, 0.08, 0.05, 0.10), omega=(1.9, 2.3, 1.3, 1.1)),
        scene.Trajectory(amp=(0.07, 0.13, 0.06, 0.15), omega=(2.4, 1.6, 1.7, 0.9))]
ACC_BIAS = 0.025
# no rest phase and faster motion: inside 16 frames tracks leave the image, the table refills to maxTracks and culls
FAST_TRAJ = [scene.Trajectory(amp=(0.35, 0.25, 0.10, 0.30), omega=(3.0, 2.6, 2.0, 2.2), t_rest=0.0, ramp_seconds=0.3),
             scene.Trajectory(amp=(0.25, 0.35, 0.12, 0.40), omega=(2.7, 3.1, 2.3, 1.9), t_rest=0.0, ramp_seconds=0.3)]
# triangulationMaxDist 2.9 m with the plane 2.5 m away: tracks far from the image centre are beyond the depth window and are
# blacklisted when visited; trackMinFrames 2 and a good-frame window of 0.2 s: visits from the second frame, TRACKING within 0.25 s
FAST = dict(vu__triangulationMaxDist=2.9, trail__trackMinFrames=2, session__goodFramesTimeWindowSeconds=0.2, session__goodFramesToTracking=0.5)
FILTER_RANSAC3, FILTER_UPRIGHT2P, FILTER_HYBRID, FILTER_NONE = 0, 1, 2, 3
TRACKED = 0


def params(every_n=1, fast=True, stereo=True, **over):
    """The parameters of a session; `over` names members as capi.vio_default_params does (useRansac3=0, fast__maxTracks=M, ...)."""
    T1, T2 = scene.IMU_TO_CAMERA, RIG.second_imu_to_camera()
    cam = capi.camera_model("pinhole", RIG.focal, RIG.focal, RIG.pp[0], RIG.pp[1])
    kw = dict(
        gftt__maxTracks=M, gftt__gfttMinDistance=8.0, tracks__maxTracks=M, trail__maxTracks=M, output__maxTracks=M, fast__maxTracks=M,
        gftt_legacy__maxTracks=M, gftt_legacy__gfttMinDistance=8.0 * 720.0 / min(W_, H_),
        gate__cam0ToCam1=T2 @ np.linalg.inv(T1), flow__imuToCamera=T1, flow__secondImuToCamera=T2, flow__cameraToImu=np.linalg.inv(T1),
        flow__secondCameraToImu=np.linalg.inv(T2), vu__imuToCamera=T1, vu__secondImuToCamera=T2, output__imuToCamera=T1,
        session__targetFps=FPS, session__visualUpdateForEveryNFrame=every_n, imu_samples_max=NS,
        trail__useStereo=int(stereo), output__useStereo=int(stereo))
    kw.update(FAST if fast else {})
    kw.update(over)
    p = capi.vio_default_params(**kw)
    p.vu.useStereo = int(stereo)
    p.camera0, p.camera1 = cam, cam
    return p


def session_of(p):
    """(stereo, filter, detector): RansacPipeline::compute's choice (ransac_pipeline.cpp:121-136); RANSAC3 and the upright filter
    need cameras.size() >= 2."""
    stereo = bool(p.trail.useStereo)
    if p.useRansac3 and stereo:
        filt = FILTER_RANSAC3
    elif p.useStereoUpright2p and stereo:
        filt = FILTER_UPRIGHT2P
    else:
        filt = FILTER_HYBRID if p.useHybridRansac else FILTER_NONE
    return stereo, filt, p.featureDetector


@functools.lru_cache(maxsize=None)
def scenes(frames, kind):
    """Two sequences. kind "fast": the fast trajectories with exact IMU samples; "noisy": the trajectories with the rest phase, white
    IMU noise at the filter's process-noise levels and the constant accelerometer bias."""
    e = capi.ekf_default_params()
    noisy = kind == "noisy"
    kw = dict(noise_acc=e.noiseProcessAcc, noise_gyro=e.noiseProcessGyro, acc_bias=(ACC_BIAS, 0.0, 0.0)) if noisy else {}
    return tuple(scene.make(11 + s, (TRAJ if noisy else FAST_TRAJ)[s], frames, RIG, fps=FPS, imu_rate=FPS * NS, gravity=e.gravity,
                            noise_seed=(100 + s if noisy else None), **kw) for s in range(S))


def inputs(scs, frames, stereo=True, noise_set=None):
    """Device tensors: left / right [F][S][H][W] u8 (right: None for a mono session), t [F][NS][S], gyro / acc [F][NS][S][3].
    noise_set: that set sees unrelated noise, in its right images (stereo) or its only images (mono)."""
    import torch
    left = np.stack([sc.left[:frames] for sc in scs], 1)
    right = np.stack([sc.right[:frames] for sc in scs], 1) if stereo else None
    if noise_set is not None:
        img = right if stereo else left
        img[:, noise_set] = np.random.default_rng(9).integers(0, 256, img[:, noise_set].shape, dtype=np.uint8)
    t = np.stack([sc.imu_t[:frames * NS].reshape(frames, NS) for sc in scs], 2)
    gyro = np.stack([sc.gyro[:frames * NS].reshape(frames, NS, 3) for sc in scs], 2)
    acc = np.stack([sc.acc[:frames * NS].reshape(frames, NS, 3) for sc in scs], 2)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(left=dev(left), right=dev(right) if stereo else None, t=dev(t), gyro=dev(gyro), acc=dev(acc))


def host(x):
    if isinstance(x, dict):
        return {k: host(v) for k, v in x.items() if v is not None}
    return x.cpu().numpy().copy()


STAGES = ("full_update", "keyframe", "keyframe_out", "good_frame", "reset_kind", "tracking_status", "n_candidates", "cand_id", "status",
          "gate_status", "ransac_result", "ransac_score")


def groups_of(p):
    """The owned objects a session has: the second tracker generator only where the filter draws from it."""
    _, filt, _ = session_of(p)
    rng3 = ("rng_ransac3",) if filt in (FILTER_RANSAC3, FILTER_UPRIGHT2P) else ()
    return ("table", "trail", "session", "control", "record", "rng_pipeline", "rng_odometry") + rng3


def stages_of(p):
    return STAGES + (("r5_summary",) if session_of(p)[1] == FILTER_HYBRID else ())


def engine_snapshot(eng, view, p):
    import torch
    torch.cuda.synchronize()
    snap = {g: host(view[g]) for g in groups_of(p)}
    snap["stage"] = {k: host(view[k]) for k in stages_of(p)}
    snap["mean"], snap["cov"] = eng.state()
    return snap


def frame_args(inp, f):
    right = inp["right"][f].data_ptr() if inp["right"] is not None else 0
    return (inp["left"][f].data_ptr(), right, H_ * W_, W_, NS, inp["t"][f].data_ptr(), inp["gyro"][f].data_ptr(), inp["acc"][f].data_ptr())


def run_engine(p, inp, frames, session=True):
    """hv_vio_frame per frame, eagerly; a snapshot of everything the view exposes after every frame."""
    import torch
    snaps = []
    per_set = 3 if p.trail.useStereo else 2
    with capi.Context(width=W_, height=H_, pool_size=per_set * S, max_tracks=M) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        with capi.VioEngine(ctx, p, S, session=session) as eng:
            assert eng.replay_period() == 1
            view = eng.view()
            for f in range(frames):
                eng.frame(*frame_args(inp, f))
                snaps.append(engine_snapshot(eng, view, p))
    return snaps


class Chain:
    """The stages of a frame issued one by one on this object's own buffers."""

    def __init__(self, ctx, p):
        import torch
        self.ctx, self.p, self.L = ctx, p, capi.lib()
        self.stereo, self.filter, self.detector = session_of(p)
        self.K, self.V = p.trail.cameraTrailLength + 1, p.trail.maxVisualUpdates
        K, V, Cn = self.K, self.V, (2 if self.stereo else 1)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        i32, f32, f64, u8 = torch.int32, torch.float32, torch.float64, torch.uint8
        self.ekf = capi.EkfBatch(ctx, p.ekf, S)
        self.t = dict(n_tracks=z(S, i32), ids=z((S, M), i32), xy=z((S, M, 2), f32), status=z((S, M), i32),
                      blacklist=z((S, M), u8), kf_xy=z((S, M, 2), f32), kf_valid=z((S, M), u8), frame_num=z(S, i32), mask_steps=z(S, i32),
                      mask_radius=z(S, i32), frame_flags=z(S, u8))
        if self.stereo:
            self.t["second_xy"] = z((S, M, 2), f32)
        self.table = capi.track_table(**{k: v.data_ptr() for k, v in self.t.items()})
        self.trail = capi.TrailIndex(S, p.trail)
        self.ses = capi.session_state(S, capi.session_window(p.session))
        self.ctl = capi.EkfControl(S)
        self.rng2, self.rng_odo = capi.rng_state(S), capi.rng_state(S)
        self.n_draws = {FILTER_RANSAC3: 3 * p.ransac3.ransac3MaxIterations,
                        FILTER_UPRIGHT2P: 2 * p.upright2p.ransacStereoUpright2pMaxIterations}.get(self.filter, 0)
        self.rng3 = capi.rng_state(S) if self.n_draws else None
        self.rec = capi.Output(S, p.output)
        self.b = dict(
            dt=z((NS, S), f64), time=z((NS, S), f64), n_lk=z(S, i32), full_update=z(S, u8), frame_no=z(S, i32),
            cur_xy=z((S, M, 2), f32), distance=z((S, M), f64), lk=z((S, M), u8),
            tracked_mask=z((S, M), u8), track_status=z((S, M), i32), draws2=z((S, 200), i32),
            r2_status=z((S, M), i32), r2_R=z((S, 9), f32), r2_summary=z((S, 2), i32), ransac_result=z((S, 2), i32),
            ransac_score=z(S, f64), keyframe=z(S, i32), mask_xy=z((S, M, 2), f32), n_mask=z(S, i32), src_index=z((S, M), i32),
            corners=z((S, M, 2), f32), n_corners=z(S, i32), new_xy=z((S, M, 2), f32), n_new=z(S, i32), n_added=z(S, i32),
            keyframe_out=z(S, i32), undo_active=z(S, u8), stationary=z(S, u8), draws_odo=z((S, M), i32), draws_used=z(S, i32),
            n_poses=z((V, S), i32), pose_index=z((V, S, K), i32), features=z((V, S, Cn * K, 2), f64), velocities=z((V, S, Cn * K, 2), f64),
            y=z((V, S, 2 * Cn * K), f64), cand_id=z((V, S), i32), n_candidates=z(S, i32), status=z((V, S, 2), i32), gate_status=z((V, S), i32),
            pf=z((V, S, 3), f64), success=z(S, i32), delete_ids=z((S, M), i32), n_delete=z(S, i32), good_frame=z(S, u8), n_attempts=z(S, i32),
            n_success=z(S, i32), discarded=z(S, i32), tracking_status=z(S, i32), frozen=z(S, u8), reset_kind=z(S, i32))
        if self.stereo:
            self.b.update(right_xy=z((S, M, 2), f32), lk2=z((S, M), u8), lk3=z((S, M), u8), stereo_status=z((S, M), i32),
                          corners_right=z((S, M, 2), f32), detection_status=z((S, M), i32), new_right=z((S, M, 2), f32))
        if self.n_draws:
            self.b.update(draws3=z((S, self.n_draws), i32), summary=z((S, 4), i32))
        if self.filter == FILTER_HYBRID:
            self.b.update(r5_summary=z((S, 4), i32))
        if self.detector == capi.DETECTOR_GPU_GFTT:
            self.b.update(kp=z((S, ctx.gftt_keypoint_count(p.gftt), 3), f32))
        elif self.detector == capi.DETECTOR_FAST:
            self.max_kp = self.L.hv_fast_keypoint_bound(ctx._h)
            self.b.update(kp=z((S, self.max_kp, 3), f32), n_kp=z(S, i32), work=z(self.L.hv_fast_work_bytes(ctx._h, S), u8))
        else:
            self.max_kp = self.L.hv_gftt_legacy_keypoint_bound(ctx._h)
            self.b.update(n_kp=z(S, i32), work=z(self.L.hv_gftt_legacy_work_bytes(ctx._h, S, self.max_kp), u8))
        # host-side bookkeeping
        n_slots = 3 if self.stereo else 2
        self.slots = [[ctx.acquire() for _ in range(n_slots)] for _ in range(S)]   # per set: previous left, current left(, right)
        self.frame_no = [1] * S                                  # frame->num = ++frameCount (sample_sync.cpp:138)
        self.has_prev = [False] * S
        self.facts = dict(full=0, culled=0, inliers=0, blacklisted=0, resets=[0] * S, full_update=[], frames=[])
        focal = (p.camera0.fx + p.camera0.fy) * 0.5
        self.r_gate, self.r_update = p.trackChiTestOutlierR / focal, p.visualR / focal
        su = min(W_, H_) / 720.0
        self.thr = float(np.float32((p.ransac2Threshold * su) * (p.ransac2Threshold * su)))
        self.s2f = np.ascontiguousarray(np.array(p.flow.imuToCamera).reshape(4, 4) @ np.array(p.flow.secondCameraToImu).reshape(4, 4))
        self.vu = capi.VuParams.from_buffer_copy(p.vu)
        self.vu.useStereo = p.trail.useStereo
        self.ok(self.L.hv_tracks_init_batch_dev(ctx._h, C.byref(p.tracks), S, C.byref(self.table)))
        ctx.trail_init_batch_dev(S, self.trail.table, params=p.trail)
        self.ekf.session_init_dev(p.session, self.ses)
        self.ekf.control_init_dev(self.ctl)
        ctx.rng_seed_batch_dev(S, self.rng2.table, seed=p.ransacRngSeed)
        if self.rng3 is not None:
            ctx.rng_seed_batch_dev(S, self.rng3.table, seed=p.ransacRngSeed)
        ctx.rng_seed_batch_dev(S, self.rng_odo.table, seed=p.odometryRngSeed)

    @staticmethod
    def ok(rc):
        assert rc == 0, capi.lib().hv_status_string(rc).decode()

    def frame(self, left, right, t, gyro, acc):
        import torch
        p, L, ctx, b, ok = self.p, self.L, self.ctx._h, self.b, self.ok
        e = self.ekf._h
        P = lambda x: x.data_ptr()
        B = lambda name: b[name].data_ptr() if name in b else None          # an array the session does not have is NULL
        T = lambda name: self.t[name].data_ptr() if name in self.t else None
        tab, trail = C.byref(self.table), C.byref(self.trail.table)
        cam0, cam1 = C.addressof(p.camera0), C.addressof(p.camera1)
        cam1s = cam1 if self.stereo else None
        dev_i = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")
        fact = {}
        # ---- the host's per-frame state ----
        torch.cuda.synchronize()
        n_kf = self.trail.m["n_keyframes"].cpu().tolist()
        full = [int(self.frame_no[s] % p.session.visualUpdateForEveryNFrame == 0 or n_kf[s] < 2) for s in range(S)]
        self.facts["full_update"].append(full)
        b["full_update"].copy_(torch.tensor(full, dtype=torch.uint8))
        b["frame_no"].copy_(torch.tensor(self.frame_no, dtype=torch.int32))
        n_tracks = self.t["n_tracks"].cpu().tolist()
        b["n_lk"].copy_(torch.tensor([n_tracks[s] if self.has_prev[s] else 0 for s in range(S)], dtype=torch.int32))
        for k in ("success", "n_candidates", "n_delete"):
            b[k].zero_()
        roles = [dev_i([sl[r] for sl in self.slots]) for r in range(len(self.slots[0]))]
        prev, cur = roles[0], roles[1]
        self.facts["full"] += sum(n == M for n in n_tracks)
        # 1. pyramids
        ok(L.hv_ingest_build_batch_dev(ctx, S, P(cur), P(left), H_ * W_, W_, 1, -1))
        if self.stereo:
            rgt = roles[2]
            ok(L.hv_ingest_build_batch_dev(ctx, S, P(rgt), P(right), H_ * W_, W_, 1, -1))
        # 2. IMU
        ok(L.hv_session_imu_dev(e, C.byref(self.ses.table), NS, P(t), P(acc), None, B("dt"), B("time")))
        ok(L.hv_ekf_predict_n_dev(e, NS, B("dt"), P(gyro), P(acc)))
        ok(L.hv_ekf_normalize_quaternions(e, 1))
        time = P(b["time"][NS - 1])
        ok(L.hv_ekf_imu_control_dev(e, C.byref(p.control), C.byref(self.ctl.table), time, None))
        # 3. temporal LK   4. stereo LK (a set without a previous frame has n_lk = 0)
        ok(L.hv_flow_predict_batch_dev(e, C.byref(p.flow), capi.FLOW_PREDICT_LEFT, C.byref(p.trail), trail, tab, T("xy"), cam0, cam1,
                                       B("cur_xy"), B("distance"), 0))
        ok(L.hv_klt_track_batch_ragged_dev(ctx, S, P(prev), P(cur), M, B("n_lk"), T("xy"), B("cur_xy"), B("lk"), None, 1, -1))
        ok(L.hv_flow_status_batch_dev(ctx, S, M, B("n_lk"), B("cur_xy"), B("lk"), B("track_status")))
        if self.stereo:
            ok(L.hv_flow_predict_batch_dev(e, C.byref(p.flow), capi.FLOW_PREDICT_STEREO, C.byref(p.trail), trail, tab, B("cur_xy"), cam0, cam1,
                                           B("right_xy"), B("distance"), 1))
            ok(L.hv_klt_track_batch_ragged_dev(ctx, S, P(cur), P(rgt), M, B("n_lk"), B("cur_xy"), B("right_xy"), B("lk2"), None, 1, -1))
            ok(L.hv_flow_status_batch_dev(ctx, S, M, B("n_lk"), B("right_xy"), B("lk2"), B("stereo_status")))
        # 5. gate, RANSAC2, the filter
        ok(L.hv_track_gate_batch_dev(ctx, C.byref(p.gate), S, M, B("n_lk"), B("cur_xy"), B("right_xy"), B("stereo_status"), T("blacklist"),
                                     cam0, cam1s, B("track_status"), B("tracked_mask")))
        ok(L.hv_rng_draw_batch_dev(ctx, S, C.byref(self.rng2.table), 200, B("draws2")))
        ok(L.hv_rot_ransac_lk_batch_dev(ctx, S, M, B("n_lk"), T("xy"), B("cur_xy"), B("tracked_mask"), 1, cam0, cam0, B("draws2"), self.thr,
                                        B("r2_status"), B("r2_R"), B("r2_summary")))
        ok(L.hv_rng_advance_batch_dev(ctx, S, C.byref(self.rng2.table), P(b["r2_summary"].view(-1)[1:]), 2, 2, 200))
        gated = b["track_status"].clone()
        if self.filter == FILTER_RANSAC3:
            ok(L.hv_rng_draw_batch_dev(ctx, S, C.byref(self.rng3.table), self.n_draws, B("draws3")))
            ok(L.hv_ransac3_lk_batch_dev(ctx, C.byref(p.ransac3), S, M, B("n_lk"), T("xy"), T("second_xy"), B("cur_xy"), B("track_status"),
                                         B("r2_summary"), cam0, cam1, self.s2f.ctypes.data, B("draws3"), B("ransac_result"), B("ransac_score"),
                                         None, B("summary")))
            ok(L.hv_rng_advance_batch_dev(ctx, S, C.byref(self.rng3.table), P(b["summary"].view(-1)[2:]), 4, 3, self.n_draws))
        elif self.filter == FILTER_UPRIGHT2P:
            ok(L.hv_rng_draw_batch_dev(ctx, S, C.byref(self.rng3.table), self.n_draws, B("draws3")))
            ok(L.hv_upright2p_lk_batch_dev(e, C.byref(p.upright2p), C.byref(p.flow), M, B("n_lk"), T("xy"), T("second_xy"), B("cur_xy"),
                                           B("track_status"), B("r2_summary"), cam0, cam1, self.s2f.ctypes.data, B("draws3"),
                                           B("ransac_result"), B("ransac_score"), None, B("summary")))
            ok(L.hv_rng_advance_batch_dev(ctx, S, C.byref(self.rng3.table), P(b["summary"].view(-1)[2:]), 4, 2, self.n_draws))
        elif self.filter == FILTER_HYBRID:
            ok(L.hv_hybrid_ransac_lk_batch_dev(ctx, C.byref(p.ransac5), S, M, B("n_lk"), T("xy"), B("cur_xy"), B("track_status"), B("r2_status"),
                                               B("r2_summary"), cam0, cam0, B("ransac_result"), B("ransac_score"), None, B("r5_summary")))
        else:
            # ransac_pipeline.cpp:135 in numpy: ransac2Result.inlierCount / static_cast<double>(nTrackedFeatures), no guard
            torch.cuda.synchronize()
            n_lk = b["n_lk"].cpu().numpy()
            st = gated.cpu().numpy()
            tracked = np.array([(st[s, :n_lk[s]] == TRACKED).sum() for s in range(S)], np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                score = b["r2_summary"].cpu().numpy()[:, 0].astype(np.float64) / tracked
            b["ransac_score"].copy_(torch.from_numpy(score))
            b["ransac_result"].zero_()
            fact["tracked"], fact["score"] = tracked.tolist(), score.tolist()
        fact["filter_changed"] = int((gated != b["track_status"]).sum().item())
        fact["n_tracked_in"] = [(gated[s, :n] == TRACKED).sum().item() for s, n in enumerate(b["n_lk"].cpu().tolist())]
        # 6. table, detection, append
        ok(L.hv_tracks_update_batch_dev(ctx, C.byref(p.tracks), S, tab, B("cur_xy"), B("right_xy"), B("track_status"), B("ransac_score"),
                                        B("keyframe"), B("mask_xy"), B("n_mask"), B("src_index"), None))
        ts_after = b["track_status"].clone()
        if self.detector == capi.DETECTOR_GPU_GFTT:
            ok(L.hv_gftt_detect_batch_dev(ctx, C.byref(p.gftt), S, P(cur), B("kp"), M, B("n_mask"), B("mask_xy"), T("mask_radius"), M,
                                          B("corners"), B("n_corners")))
        elif self.detector == capi.DETECTOR_FAST:
            ok(L.hv_fast_detect_batch_dev(ctx, C.byref(p.fast), S, P(cur), B("work"), self.max_kp, B("kp"), B("n_kp"), M, B("n_mask"),
                                          B("mask_xy"), T("mask_radius"), M, B("corners"), B("n_corners")))
        else:
            ok(L.hv_gftt_legacy_detect_batch_dev(ctx, C.byref(p.gftt_legacy), S, P(cur), B("work"), self.max_kp, B("n_kp"), M, B("n_mask"),
                                                 B("mask_xy"), T("mask_radius"), M, B("corners"), None, B("n_corners")))
        ok(L.hv_corner_subpix_batch_dev(ctx, C.byref(p.subpix), S, P(cur), M, B("n_corners"), B("corners"), None))
        if self.stereo:
            ok(L.hv_klt_track_batch_ragged_dev(ctx, S, P(cur), P(rgt), M, B("n_corners"), B("corners"), B("corners_right"), B("lk3"), None, 0, -1))
            ok(L.hv_flow_status_batch_dev(ctx, S, M, B("n_corners"), B("corners_right"), B("lk3"), B("detection_status")))
        ok(L.hv_detection_filter_batch_dev(ctx, C.byref(p.gate), S, M, B("n_corners"), B("corners"), B("corners_right"), B("detection_status"),
                                           cam0, cam1s, None, B("new_xy"), B("new_right"), B("n_new")))
        ok(L.hv_tracks_append_batch_dev(ctx, C.byref(p.tracks), S, tab, M, B("n_new"), B("new_xy"), B("new_right"), B("n_added")))
        # 7. frame control, undo-augment
        ok(L.hv_ekf_frame_control_dev(e, C.byref(p.control), C.byref(self.ctl.table), time, B("keyframe"), B("full_update"), B("keyframe_out"),
                                      B("undo_active"), B("stationary"), None))
        ok(L.hv_ekf_undo_augment_dev(e, B("undo_active")))
        # 8. select, the visit loop, finish
        ok(L.hv_rng_draw_batch_dev(ctx, S, C.byref(self.rng_odo.table), M, B("draws_odo")))
        ok(L.hv_trail_select_batch_dev(ctx, C.byref(p.trail), S, trail, tab, cam0, cam1, B("keyframe_out"), B("full_update"), B("frame_no"), time,
                                       B("draws_odo"), B("draws_used"), B("n_poses"), B("pose_index"), B("features"), B("velocities"), B("y"),
                                       B("cand_id"), B("n_candidates")))
        ok(L.hv_ekf_visual_frame_ragged_dev(e, C.addressof(self.vu), self.V, self.K, B("n_poses"), B("pose_index"), B("features"),
                                            B("velocities"), B("y"), self.r_gate, self.r_update, B("status"), B("gate_status"), None, B("pf"),
                                            B("success"), p.trail.maxSuccessfulVisualUpdates))
        ok(L.hv_rng_advance_batch_dev(ctx, S, C.byref(self.rng_odo.table), B("draws_used"), 1, 1, M))
        ok(L.hv_trail_finish_batch_dev(ctx, C.byref(p.trail), S, trail, B("cand_id"), B("n_candidates"), B("status"), B("gate_status"),
                                       B("stationary"), B("delete_ids"), B("n_delete"), B("good_frame"), B("n_attempts"), B("n_success"),
                                       B("discarded")))
        # 9. delete, augmentation
        ok(L.hv_tracks_delete_batch_dev(ctx, C.byref(p.tracks), S, tab, M, B("n_delete"), B("delete_ids")))
        ok(L.hv_ekf_symmetrize_augment_dev(e, B("discarded"), None))
        # 10. status, record, reset
        ok(L.hv_session_status_dev(e, C.byref(p.session), C.byref(self.ses.table), B("good_frame"), B("full_update"), B("tracking_status"),
                                   B("frozen"), B("reset_kind")))
        of = capi.output_frame(cand_id_dev=B("cand_id"), n_candidates_dev=B("n_candidates"), status_dev=B("status"),
                               gate_status_dev=B("gate_status"), pf_dev=B("pf"), tracking_status_dev=B("tracking_status"),
                               frozen_dev=B("frozen"), stationary_dev=B("stationary"))
        ok(L.hv_output_dev(e, C.byref(p.output), C.byref(self.ses.table), trail, C.byref(of), C.byref(self.rec.table)))
        ok(L.hv_session_reset_dev(e, C.byref(p.session), C.byref(self.ses.table), C.byref(self.ctl.table), C.byref(p.tracks), tab,
                                  C.byref(p.trail), trail, B("reset_kind")))
        ok(L.hv_rng_seed_batch_dev(ctx, S, C.byref(self.rng2.table), p.ransacRngSeed, None, B("reset_kind")))
        if self.rng3 is not None:
            ok(L.hv_rng_seed_batch_dev(ctx, S, C.byref(self.rng3.table), p.ransacRngSeed, None, B("reset_kind")))
        # ---- the host's bookkeeping behind the frame ----
        torch.cuda.synchronize()
        kinds = b["reset_kind"].cpu().tolist()
        for s in range(S):
            self.slots[s][0], self.slots[s][1] = self.slots[s][1], self.slots[s][0]
            self.frame_no[s] += 1
            self.has_prev[s] = kinds[s] == 0
            self.facts["resets"][s] += kinds[s] != 0
        self.facts["culled"] += int((ts_after == capi.ST_CULLED).sum().item())
        st, gs = b["status"].cpu().numpy(), b["gate_status"].cpu().numpy()
        self.facts["inliers"] += int(((st[:, :, 0] != -1) & (gs == 0)).sum())
        self.facts["blacklisted"] += int(b["n_delete"].sum().item())
        fact["n_corners"] = b["n_corners"].cpu().tolist()
        fact["result"] = b["ransac_result"].cpu().tolist()
        for k in ("summary", "r5_summary"):
            if k in b:
                fact[k] = b[k].cpu().tolist()
        self.facts["frames"].append(fact)

    def snapshot(self):
        import torch
        torch.cuda.synchronize()
        rng = lambda r: dict(mt=host(r.mt), pos=host(r.pos))
        snap = dict(table=host(self.t), trail=host(self.trail.m), session=host(self.ses.m),
                    control={k: host(getattr(self.ctl, k)) for k, _ in capi.EkfControlTable._fields_}, record=host(self.rec.m),
                    rng_pipeline=rng(self.rng2), rng_odometry=rng(self.rng_odo))
        if self.rng3 is not None:
            snap["rng_ransac3"] = rng(self.rng3)
        snap["stage"] = {k: host(self.b[k]) for k in stages_of(self.p)}
        snap["mean"] = np.stack([self.ekf.get_state(s)[0] for s in range(S)])
        snap["cov"] = np.stack([self.ekf.get_state(s)[1] for s in range(S)])
        return snap


def run_chain(p, inp, frames):
    import torch
    snaps = []
    per_set = 3 if p.trail.useStereo else 2
    with capi.Context(width=W_, height=H_, pool_size=per_set * S, max_tracks=M) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ch = Chain(ctx, p)
        for f in range(frames):
            ch.frame(inp["left"][f], inp["right"][f] if inp["right"] is not None else None, inp["t"][f], inp["gyro"][f], inp["acc"][f])
            snaps.append(ch.snapshot())
        facts = ch.facts
        ch.ekf.close()
    return snaps, facts


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def assert_equal(got, want, what, sets=None):
    """Equality of bits, member by member (sets: only these sets of every [S]-leading array; the visit arrays are [V][S])."""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for g in got:
        pairs = got[g].items() if isinstance(got[g], dict) else [(None, got[g])]
        if isinstance(got[g], dict):
            assert set(got[g]) == set(want[g]), (what, g, sorted(got[g]), sorted(want[g]))
        for k, a in pairs:
            w = want[g][k] if k is not None else want[g]
            assert a.shape == w.shape and a.dtype == w.dtype, (what, g, k, a.shape, w.shape, a.dtype, w.dtype)
            if sets is not None:
                ax = 1 if (g == "stage" and k in ("cand_id", "status", "gate_status")) else 0
                a, w = np.take(a, sets, ax), np.take(w, sets, ax)
            if a.dtype.kind == "f" and k == "ransac_score":       # 0 / 0: IEEE leaves the sign and payload of the NaN open
                assert (np.isnan(a) == np.isnan(w)).all(), (what, g, k)
                a, w = np.where(np.isnan(a), 0.0, a), np.where(np.isnan(w), 0.0, w)
            assert bits(a) == bits(w), (what, g, k)
