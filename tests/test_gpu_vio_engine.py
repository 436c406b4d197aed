"""GPU tests of the resident VIO engine (hv_vio_create / hv_vio_frame / hv_vio_view_get / hv_vio_replay_period; csrc/vio_engine.hip)
on scenes with ground truth (hybvio_amd/scene.py): the engine against the same stages issued call by call from Python with the
test's own buffers and host-side bookkeeping, through in-place resets, replayed from one captured graph, and against the true
trajectory. 376 x 240, maxTracks 120, gfttMinDistance 8, two sets, ten IMU samples per frame."""
import ctypes as C
import functools

import numpy as np
import pytest

from hybvio_amd import capi, scene

pytestmark = pytest.mark.gpu
W_, H_, M, S, NS, FPS = 376, 240, 120, 2, 10, 20.0
RIG = scene.Rig(width=W_, height=H_)
TRAJ = [scene.Trajectory(amp=(0.12, 0.08, 0.05, 0.10), omega=(1.9, 2.3, 1.3, 1.1)),
        scene.Trajectory(amp=(0.07, 0.13, 0.06, 0.15), omega=(2.4, 1.6, 1.7, 0.9))]
ACC_BIAS = 0.025
# tests (a) to (c): no rest phase and faster motion, so that inside 16 frames tracks leave the image, the table refills to
# maxTracks and culls; FAST below completes the session these tests run
FAST_TRAJ = [scene.Trajectory(amp=(0.35, 0.25, 0.10, 0.30), omega=(3.0, 2.6, 2.0, 2.2), t_rest=0.0, ramp_seconds=0.3),
             scene.Trajectory(amp=(0.25, 0.35, 0.12, 0.40), omega=(2.7, 3.1, 2.3, 1.9), t_rest=0.0, ramp_seconds=0.3)]
# - triangulationMaxDist 2.9 m: the plane is 2.5 m away, so a track more than about 135 px from the image centre lies beyond the
#   depth window (backend.cpp:1096-1099, BAD_DEPTH) and is blacklisted when it is visited, while central tracks are inliers;
# - trackMinFrames 2 and a good-frame window of 0.2 s (four frames): the visits start at the second frame and a session is
#   TRACKING once three of them have come in with more than half of them good (goodFramesToTracking 0.5): at 0.15 s to 0.25 s, in
#   front of test (b)'s reset timer of 0.3 s.
FAST = dict(vu__triangulationMaxDist=2.9, trail__trackMinFrames=2, session__goodFramesTimeWindowSeconds=0.2, session__goodFramesToTracking=0.5)


def _params(every_n=1, fast=True, **session):
    T1, T2 = scene.IMU_TO_CAMERA, RIG.second_imu_to_camera()
    cam = capi.camera_model("pinhole", RIG.focal, RIG.focal, RIG.pp[0], RIG.pp[1])
    p = capi.vio_default_params(
        gftt__maxTracks=M, gftt__gfttMinDistance=8.0, tracks__maxTracks=M, trail__maxTracks=M, output__maxTracks=M,
        gate__cam0ToCam1=T2 @ np.linalg.inv(T1), flow__imuToCamera=T1, flow__secondImuToCamera=T2, flow__cameraToImu=np.linalg.inv(T1),
        flow__secondCameraToImu=np.linalg.inv(T2), vu__imuToCamera=T1, vu__secondImuToCamera=T2, output__imuToCamera=T1,
        session__targetFps=FPS, session__visualUpdateForEveryNFrame=every_n, imu_samples_max=NS,
        **(FAST if fast else {}), **{"session__" + k: v for k, v in session.items()})
    p.vu.useStereo = 1
    p.camera0, p.camera1 = cam, cam
    return p


@functools.lru_cache(maxsize=None)
def _scenes(frames, noisy):
    """Two sequences. noisy (test (d)): the trajectories with the rest phase, white IMU noise at the filter's process-noise levels
    and the constant accelerometer bias; otherwise the fast trajectories with exact IMU samples."""
    e = capi.ekf_default_params()
    kw = dict(noise_acc=e.noiseProcessAcc, noise_gyro=e.noiseProcessGyro, acc_bias=(ACC_BIAS, 0.0, 0.0)) if noisy else {}
    return tuple(scene.make(11 + s, (TRAJ if noisy else FAST_TRAJ)[s], frames, RIG, fps=FPS, imu_rate=FPS * NS, gravity=e.gravity,
                            noise_seed=(100 + s if noisy else None), **kw) for s in range(S))


def _inputs(scs, frames, right_noise_set=None):
    """Device tensors: left / right [F][S][H][W] u8, t [F][NS][S], gyro / acc [F][NS][S][3]."""
    import torch
    left = np.stack([sc.left[:frames] for sc in scs], 1)
    right = np.stack([sc.right[:frames] for sc in scs], 1)
    if right_noise_set is not None:
        right[:, right_noise_set] = np.random.default_rng(9).integers(0, 256, right[:, right_noise_set].shape, dtype=np.uint8)
    t = np.stack([sc.imu_t[:frames * NS].reshape(frames, NS) for sc in scs], 2)
    gyro = np.stack([sc.gyro[:frames * NS].reshape(frames, NS, 3) for sc in scs], 2)
    acc = np.stack([sc.acc[:frames * NS].reshape(frames, NS, 3) for sc in scs], 2)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(left=dev(left), right=dev(right), t=dev(t), gyro=dev(gyro), acc=dev(acc))


def _host(x):
    return {k: _host(v) for k, v in x.items()} if isinstance(x, dict) else x.cpu().numpy().copy()


STAGES = ("full_update", "keyframe", "keyframe_out", "good_frame", "reset_kind", "tracking_status", "n_candidates", "cand_id", "status",
          "gate_status")
GROUPS = ("table", "trail", "session", "control", "record", "rng_pipeline", "rng_ransac3", "rng_odometry")


def _engine_snapshot(eng, view):
    import torch
    torch.cuda.synchronize()
    snap = {g: _host(view[g]) for g in GROUPS}
    snap["stage"] = {k: _host(view[k]) for k in STAGES}
    snap["mean"], snap["cov"] = eng.state()
    return snap


def _run_engine(p, inp, frames):
    """hv_vio_frame per frame, eagerly; a snapshot of everything the view exposes after every frame."""
    import torch
    snaps = []
    with capi.Context(width=W_, height=H_, pool_size=3 * S, max_tracks=M) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        with capi.VioEngine(ctx, p, S) as eng:
            assert eng.replay_period() == 1
            view = eng.view()
            for f in range(frames):
                eng.frame(inp["left"][f].data_ptr(), inp["right"][f].data_ptr(), H_ * W_, W_, NS, inp["t"][f].data_ptr(),
                          inp["gyro"][f].data_ptr(), inp["acc"][f].data_ptr())
                snaps.append(_engine_snapshot(eng, view))
    return snaps


@functools.lru_cache(maxsize=None)
def _engine_run(every_n, frames, reset):
    scs = _scenes(24, False)
    p = _params(every_n, **(dict(resetUntilInitSucceeds=1, resetAfterTrackingFailsToInitialize=0.3) if reset else {}))
    return _run_engine(p, _inputs(scs, frames, 1 if reset else None), frames)


class Chain:
    """The stages of a frame issued one by one, in the order of INTEGRATION.md, on this object's own buffers. The slot roles, the
    frame number, "has a previous frame" and full_update (the literal rule of backend.cpp:765) are kept on the host."""

    def __init__(self, ctx, p):
        import torch
        self.ctx, self.p, self.L = ctx, p, capi.lib()
        self.K, self.V = p.trail.cameraTrailLength + 1, p.trail.maxVisualUpdates
        K, V = self.K, self.V
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        i32, f32, f64, u8 = torch.int32, torch.float32, torch.float64, torch.uint8
        self.ekf = capi.EkfBatch(ctx, p.ekf, S)
        self.t = dict(n_tracks=z(S, i32), ids=z((S, M), i32), xy=z((S, M, 2), f32), second_xy=z((S, M, 2), f32), status=z((S, M), i32),
                      blacklist=z((S, M), u8), kf_xy=z((S, M, 2), f32), kf_valid=z((S, M), u8), frame_num=z(S, i32), mask_steps=z(S, i32),
                      mask_radius=z(S, i32), frame_flags=z(S, u8))
        self.table = capi.track_table(**{k: v.data_ptr() for k, v in self.t.items()})
        self.trail = capi.TrailIndex(S, p.trail)
        self.ses = capi.session_state(S, capi.session_window(p.session))
        self.ctl = capi.EkfControl(S)
        self.rng2, self.rng3, self.rng_odo = capi.rng_state(S), capi.rng_state(S), capi.rng_state(S)
        self.rec = capi.Output(S, p.output)
        nk = ctx.gftt_keypoint_count(p.gftt)
        n3 = 3 * p.ransac3.ransac3MaxIterations
        self.b = dict(
            dt=z((NS, S), f64), time=z((NS, S), f64), n_lk=z(S, i32), full_update=z(S, u8), frame_no=z(S, i32),
            cur_xy=z((S, M, 2), f32), right_xy=z((S, M, 2), f32), distance=z((S, M), f64), lk=z((S, M), u8), lk2=z((S, M), u8), lk3=z((S, M), u8),
            tracked_mask=z((S, M), u8), track_status=z((S, M), i32), stereo_status=z((S, M), i32), draws2=z((S, 200), i32),
            r2_status=z((S, M), i32), r2_R=z((S, 9), f32), r2_summary=z((S, 2), i32), draws3=z((S, n3), i32), r3_result=z((S, 2), i32),
            score=z(S, f64), r3_summary=z((S, 4), i32), keyframe=z(S, i32), mask_xy=z((S, M, 2), f32), n_mask=z(S, i32), src_index=z((S, M), i32),
            kp=z((S, nk, 3), f32), corners=z((S, M, 2), f32), n_corners=z(S, i32), corners_right=z((S, M, 2), f32), detection_status=z((S, M), i32),
            new_xy=z((S, M, 2), f32), new_right=z((S, M, 2), f32), n_new=z(S, i32), n_added=z(S, i32),
            keyframe_out=z(S, i32), undo_active=z(S, u8), stationary=z(S, u8), draws_odo=z((S, M), i32), draws_used=z(S, i32),
            n_poses=z((V, S), i32), pose_index=z((V, S, K), i32), features=z((V, S, 2 * K, 2), f64), velocities=z((V, S, 2 * K, 2), f64),
            y=z((V, S, 4 * K), f64), cand_id=z((V, S), i32), n_candidates=z(S, i32), status=z((V, S, 2), i32), gate_status=z((V, S), i32),
            pf=z((V, S, 3), f64), success=z(S, i32), delete_ids=z((S, M), i32), n_delete=z(S, i32), good_frame=z(S, u8), n_attempts=z(S, i32),
            n_success=z(S, i32), discarded=z(S, i32), tracking_status=z(S, i32), frozen=z(S, u8), reset_kind=z(S, i32))
        # host-side bookkeeping
        self.slots = [[ctx.acquire() for _ in range(3)] for _ in range(S)]     # per set: previous left, current left, right
        self.frame_no = [1] * S                                  # frame->num = ++frameCount (sample_sync.cpp:138)
        self.has_prev = [False] * S
        self.facts = dict(full=0, culled=0, inliers=0, blacklisted=0, resets=[0] * S, full_update=[])
        focal = (p.camera0.fx + p.camera0.fy) * 0.5
        self.r_gate, self.r_update = p.trackChiTestOutlierR / focal, p.visualR / focal
        su = min(W_, H_) / 720.0
        self.thr = float(np.float32((p.ransac2Threshold * su) * (p.ransac2Threshold * su)))
        self.s2f = np.ascontiguousarray(np.array(p.flow.imuToCamera).reshape(4, 4) @ np.array(p.flow.secondCameraToImu).reshape(4, 4))
        self.ok(self.L.hv_tracks_init_batch_dev(ctx._h, C.byref(p.tracks), S, C.byref(self.table)))
        ctx.trail_init_batch_dev(S, self.trail.table, params=p.trail)
        self.ekf.session_init_dev(p.session, self.ses)
        self.ekf.control_init_dev(self.ctl)
        ctx.rng_seed_batch_dev(S, self.rng2.table, seed=p.ransacRngSeed)
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
        B = lambda name: b[name].data_ptr()
        T = lambda name: self.t[name].data_ptr()
        tab, trail = C.byref(self.table), C.byref(self.trail.table)
        cam0, cam1 = C.addressof(p.camera0), C.addressof(p.camera1)
        dev_i = lambda xs: torch.tensor(xs, dtype=torch.int32, device="cuda")
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
        prev, cur, rgt = (dev_i([sl[r] for sl in self.slots]) for r in range(3))
        self.facts["full"] += sum(n == M for n in n_tracks)
        # 1. pyramids
        ok(L.hv_ingest_build_batch_dev(ctx, S, P(cur), P(left), H_ * W_, W_, 1, -1))
        ok(L.hv_ingest_build_batch_dev(ctx, S, P(rgt), P(right), H_ * W_, W_, 1, -1))
        # 2. IMU
        ok(L.hv_session_imu_dev(e, C.byref(self.ses.table), NS, P(t), P(acc), None, B("dt"), B("time")))
        ok(L.hv_ekf_predict_n_dev(e, NS, B("dt"), P(gyro), P(acc)))
        ok(L.hv_ekf_normalize_quaternions(e, 1))
        time = P(b["time"][NS - 1])
        ok(L.hv_ekf_imu_control_dev(e, C.byref(p.control), C.byref(self.ctl.table), time, None))
        if any(self.has_prev):                                    # no set has a previous frame: the detection-only path
            # 3. temporal LK   4. stereo LK
            ok(L.hv_flow_predict_batch_dev(e, C.byref(p.flow), capi.FLOW_PREDICT_LEFT, C.byref(p.trail), trail, tab, T("xy"), cam0, cam1,
                                           B("cur_xy"), B("distance"), 0))
            ok(L.hv_klt_track_batch_ragged_dev(ctx, S, P(prev), P(cur), M, B("n_lk"), T("xy"), B("cur_xy"), B("lk"), None, 1, -1))
            ok(L.hv_flow_status_batch_dev(ctx, S, M, B("n_lk"), B("cur_xy"), B("lk"), B("track_status")))
            ok(L.hv_flow_predict_batch_dev(e, C.byref(p.flow), capi.FLOW_PREDICT_STEREO, C.byref(p.trail), trail, tab, B("cur_xy"), cam0, cam1,
                                           B("right_xy"), B("distance"), 1))
            ok(L.hv_klt_track_batch_ragged_dev(ctx, S, P(cur), P(rgt), M, B("n_lk"), B("cur_xy"), B("right_xy"), B("lk2"), None, 1, -1))
            ok(L.hv_flow_status_batch_dev(ctx, S, M, B("n_lk"), B("right_xy"), B("lk2"), B("stereo_status")))
            # 5. gate, RANSAC2, RANSAC3
            ok(L.hv_track_gate_batch_dev(ctx, C.byref(p.gate), S, M, B("n_lk"), B("cur_xy"), B("right_xy"), B("stereo_status"), T("blacklist"),
                                         cam0, cam1, B("track_status"), B("tracked_mask")))
            ok(L.hv_rng_draw_batch_dev(ctx, S, C.byref(self.rng2.table), 200, B("draws2")))
            ok(L.hv_rot_ransac_lk_batch_dev(ctx, S, M, B("n_lk"), T("xy"), B("cur_xy"), B("tracked_mask"), 1, cam0, cam0, B("draws2"), self.thr,
                                            B("r2_status"), B("r2_R"), B("r2_summary")))
            ok(L.hv_rng_advance_batch_dev(ctx, S, C.byref(self.rng2.table), P(b["r2_summary"].view(-1)[1:]), 2, 2, 200))
            n3 = 3 * p.ransac3.ransac3MaxIterations
            ok(L.hv_rng_draw_batch_dev(ctx, S, C.byref(self.rng3.table), n3, B("draws3")))
            ok(L.hv_ransac3_lk_batch_dev(ctx, C.byref(p.ransac3), S, M, B("n_lk"), T("xy"), T("second_xy"), B("cur_xy"), B("track_status"),
                                         B("r2_summary"), cam0, cam1, self.s2f.ctypes.data, B("draws3"), B("r3_result"), B("score"), None,
                                         B("r3_summary")))
            ok(L.hv_rng_advance_batch_dev(ctx, S, C.byref(self.rng3.table), P(b["r3_summary"].view(-1)[2:]), 4, 3, n3))
        # 6. table, detection, append
        ok(L.hv_tracks_update_batch_dev(ctx, C.byref(p.tracks), S, tab, B("cur_xy"), B("right_xy"), B("track_status"), B("score"), B("keyframe"),
                                        B("mask_xy"), B("n_mask"), B("src_index"), None))
        ts_after = b["track_status"].clone()
        ok(L.hv_gftt_detect_batch_dev(ctx, C.byref(p.gftt), S, P(cur), B("kp"), M, B("n_mask"), B("mask_xy"), T("mask_radius"), M, B("corners"),
                                      B("n_corners")))
        ok(L.hv_corner_subpix_batch_dev(ctx, C.byref(p.subpix), S, P(cur), M, B("n_corners"), B("corners"), None))
        ok(L.hv_klt_track_batch_ragged_dev(ctx, S, P(cur), P(rgt), M, B("n_corners"), B("corners"), B("corners_right"), B("lk3"), None, 0, -1))
        ok(L.hv_flow_status_batch_dev(ctx, S, M, B("n_corners"), B("corners_right"), B("lk3"), B("detection_status")))
        ok(L.hv_detection_filter_batch_dev(ctx, C.byref(p.gate), S, M, B("n_corners"), B("corners"), B("corners_right"), B("detection_status"),
                                           cam0, cam1, None, B("new_xy"), B("new_right"), B("n_new")))
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
        ok(L.hv_ekf_visual_frame_ragged_dev(e, C.addressof(p.vu), self.V, self.K, B("n_poses"), B("pose_index"), B("features"), B("velocities"),
                                            B("y"), self.r_gate, self.r_update, B("status"), B("gate_status"), None, B("pf"), B("success"),
                                            p.trail.maxSuccessfulVisualUpdates))
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

    def snapshot(self):
        import torch
        torch.cuda.synchronize()
        rng = lambda r: dict(mt=_host(r.mt), pos=_host(r.pos))
        snap = dict(table=_host(self.t), trail=_host(self.trail.m), session=_host(self.ses.m),
                    control={k: _host(getattr(self.ctl, k)) for k, _ in capi.EkfControlTable._fields_}, record=_host(self.rec.m),
                    rng_pipeline=rng(self.rng2), rng_ransac3=rng(self.rng3), rng_odometry=rng(self.rng_odo))
        snap["stage"] = {k: _host(self.b[k]) for k in STAGES}
        snap["mean"] = np.stack([self.ekf.get_state(s)[0] for s in range(S)])
        snap["cov"] = np.stack([self.ekf.get_state(s)[1] for s in range(S)])
        return snap


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _assert_equal(got, want, what, sets=None):
    """Equality of bits, member by member (sets: only these sets of every [S]-leading array; the visit arrays are [V][S])."""
    for g in got:
        pairs = got[g].items() if isinstance(got[g], dict) else [(None, got[g])]
        for k, a in pairs:
            w = want[g][k] if k is not None else want[g]
            assert a.shape == w.shape and a.dtype == w.dtype, (what, g, k)
            if sets is not None:
                ax = 1 if (g == "stage" and k in ("cand_id", "status", "gate_status")) else 0
                a, w = np.take(a, sets, ax), np.take(w, sets, ax)
            assert _bits(a) == _bits(w), (what, g, k)


def _run_chain(p, inp, frames):
    import torch
    snaps = []
    with capi.Context(width=W_, height=H_, pool_size=3 * S, max_tracks=M) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ch = Chain(ctx, p)
        for f in range(frames):
            ch.frame(inp["left"][f], inp["right"][f], inp["t"][f], inp["gyro"][f], inp["acc"][f])
            snaps.append(ch.snapshot())
        facts = ch.facts
        ch.ekf.close()
    return snaps, facts


@pytest.mark.parametrize("every_n", [1, 2])
def test_the_engine_is_the_chain(every_n):
    """(a) 16 frames of two scene sequences: after every frame the table, the index, the session, the control block, the three
    generators, the mean and covariance, every stage output of the view and the record are bit-equal between hv_vio_frame and the
    call-by-call chain. The chain asserts what makes the comparison worth something: the table filled and culled, a visit was an
    inlier, a track was blacklisted; and, with visualUpdateForEveryNFrame = 2, what the literal rule gave."""
    frames = 16
    eng = _engine_run(every_n, frames, False)
    chain, facts = _run_chain(_params(every_n), _inputs(_scenes(24, False), frames), frames)
    print("chain facts", every_n, {k: v for k, v in facts.items() if k != "full_update"}, "full_update", facts["full_update"])
    for f in range(frames):
        _assert_equal(eng[f], chain[f], ("frame", f))
    assert facts["full"] > 0 and facts["culled"] > 0, facts
    assert facts["inliers"] > 0 and facts["blacklisted"] > 0, facts
    assert facts["resets"] == [0, 0]
    fu = np.array(facts["full_update"])
    assert (np.array([e["stage"]["full_update"] for e in eng]) == fu).all()
    if every_n == 1:
        assert fu.all()
    else:
        assert fu[:2].all()                                       # the first two frames: n_keyframes < 2
        assert (fu[2:, 0] == (np.arange(3, frames + 1) % 2 == 0)).all() and (fu[2:, 1] == fu[2:, 0]).all()   # frame->num is 1-based


def test_reset_in_place():
    """(b) 24 frames with resetUntilInitSucceeds and resetAfterTrackingFailsToInitialize = 0.3 s; set 1's right images are unrelated
    noise, so it never has a good frame: it resets at least twice, set 0 never; engine and chain stay bit-equal through the resets,
    and set 0 is bit-equal to its run without them."""
    frames = 24
    eng = _engine_run(1, frames, True)
    p = _params(1, resetUntilInitSucceeds=1, resetAfterTrackingFailsToInitialize=0.3)
    chain, facts = _run_chain(p, _inputs(_scenes(24, False), frames, 1), frames)
    print("reset facts", {k: v for k, v in facts.items() if k != "full_update"}, "good", [e["stage"]["good_frame"].tolist() for e in eng],
          "status", [e["stage"]["tracking_status"].tolist() for e in eng], "kind", [e["stage"]["reset_kind"].tolist() for e in eng])
    for f in range(frames):
        _assert_equal(eng[f], chain[f], ("frame", f))
    assert facts["resets"][1] >= 2 and facts["resets"][0] == 0, facts
    kinds = np.array([e["stage"]["reset_kind"] for e in eng])
    assert (kinds[:, 1] != 0).sum() == facts["resets"][1] and (kinds[:, 0] == 0).all()
    plain = _engine_run(1, 16, False)
    for f in range(16):
        _assert_equal(eng[f], plain[f], ("set 0, frame", f), sets=[0])


def test_replay_from_one_graph():
    """(c) One eager frame, then hv_vio_replay_period() frames captured and replayed for the remaining frames with the inputs copied
    into fixed buffers in front of each replay: every record is bit-equal to the eager run."""
    import torch
    frames = 16
    eager = _engine_run(1, frames, False)
    inp = _inputs(_scenes(24, False), frames)
    p = _params(1)
    with capi.Context(width=W_, height=H_, pool_size=3 * S, max_tracks=M) as ctx:
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            fixed = {k: torch.empty_like(v[0]) for k, v in inp.items()}
            eng = capi.VioEngine(ctx, p, S)
            view = eng.view()
            period = eng.replay_period()
            assert period == 1
            call = lambda: eng.frame(fixed["left"].data_ptr(), fixed["right"].data_ptr(), H_ * W_, W_, NS, fixed["t"].data_ptr(),
                                     fixed["gyro"].data_ptr(), fixed["acc"].data_ptr())
            for k in fixed:
                fixed[k].copy_(inp[k][0])
            call()
        stream.synchronize()
        _assert_equal({"record": _host(view["record"])}, {"record": eager[0]["record"]}, "eager frame 0")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(period):
                call()
        for f in range(1, frames):
            with torch.cuda.stream(stream):
                for k in fixed:
                    fixed[k].copy_(inp[k][f])
                g.replay()
            stream.synchronize()
            _assert_equal({"record": _host(view["record"])}, {"record": eager[f]["record"]}, ("replayed frame", f))
        del g
        eng.close()


def test_create_refuses_a_context_that_is_too_small():
    """The two refusals of hv_vio_create that need a context: fewer than 3 * n_sets free pyramid slots, max_tracks below maxTracks;
    neither grows the pool nor leaves anything behind."""
    import torch
    p = _params(1)
    with capi.Context(width=W_, height=H_, pool_size=3 * S - 1, max_tracks=M) as ctx:
        with pytest.raises(capi.HvError, match="hv_vio_create"):
            capi.VioEngine(ctx, p, S)
        assert len([ctx.acquire() for _ in range(3 * S - 1)]) == 3 * S - 1        # every slot is still free
    with capi.Context(width=W_, height=H_, pool_size=3 * S, max_tracks=M - 1) as ctx:
        with pytest.raises(capi.HvError, match="hv_vio_create"):
            capi.VioEngine(ctx, p, S)
    with capi.Context(width=W_, height=H_, pool_size=3 * S, max_tracks=M) as ctx:
        with capi.VioEngine(ctx, p, S) as eng:
            with pytest.raises(capi.HvError, match="hv_vio_frame"):               # more samples than imu_samples_max
                eng.frame(16, 16, H_ * W_, W_, NS + 1, 16, 16, 16)
        torch.cuda.synchronize()


def _quat_rot(q):
    w, x, y, z = q
    return np.array([[w*w+x*x-y*y-z*z, 2*x*y-2*w*z, 2*x*z+2*w*y], [2*x*y+2*w*z, w*w-x*x+y*y-z*z, 2*y*z-2*w*x],
                     [2*x*z-2*w*y, 2*y*z+2*w*x, w*w-x*x-y*y+z*z]])


def _dead_reckoning(sc, frames):
    """Strapdown integration of the same samples in numpy from the true initial state, independent of the library: the roll from
    the gyro's z rate, the specific force turned into the world and gravity removed, semi-implicit Euler at the sample rate."""
    pos, vel, th = sc.pos[0] * 0.0, np.zeros(3), 0.0
    h = sc.imu_t[1] - sc.imu_t[0]
    for k in range(1, frames * NS):
        th += sc.gyro[k, 2] * h
        R_wi = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
        pos = pos + vel * h
        vel = vel + (R_wi @ sc.acc[k] - np.array([0, 0, sc.gravity])) * h
    return pos


def test_ground_truth():
    """(d) 80 frames (4 s at 20 Hz) of two trajectories of about 1 m, Z0 2.5 m, baseline 0.1 m, IMU white noise at the process-noise
    levels and a constant accelerometer bias of 0.025 m/s^2. e_dr: the position error at 4 s of a strapdown integration of the same
    samples (analytic size b T^2 / 2 = 0.2 m); e_vio: the error of the record's position after the first record's pose is aligned
    rigidly to the truth. Every record finite, both sets TRACKING at the end without a reset, e_vio < e_dr / 2: vision helps."""
    frames = 80
    scs = _scenes(frames, True)
    snaps = _run_engine(_params(1, fast=False), _inputs(scs, frames), frames)
    for s, sc in enumerate(scs):
        e_dr = np.linalg.norm(_dead_reckoning(sc, frames) - sc.pos[frames - 1])
        pose = np.array([sn["record"]["inertial_mean"][s] for sn in snaps])
        status = np.array([sn["record"]["tracking_status"][s] for sn in snaps])
        kinds = np.array([sn["stage"]["reset_kind"][s] for sn in snaps])
        assert all(np.isfinite(v).all() for sn in snaps for v in sn["record"].values() if v.dtype.kind == "f")
        # rigid alignment of the first record's pose to the truth: world_true = Ra (x - p_0) + pos_true_0
        Ra = _quat_rot(sc.quat[0]).T @ _quat_rot(pose[0, 6:10] / np.linalg.norm(pose[0, 6:10]))
        est = (pose[:, 0:3] - pose[0, 0:3]) @ Ra.T + sc.pos[0]
        e_vio = np.linalg.norm(est[-1] - sc.pos[frames - 1])
        first = int(np.argmax(status == capi.TRACKING_TRACKING)) if (status == capi.TRACKING_TRACKING).any() else -1
        print(f"set {s}: e_vio {e_vio:.4f} m, e_dr {e_dr:.4f} m, TRACKING from frame {first}, max error on the way "
              f"{np.linalg.norm(est - sc.pos[:frames], axis=1).max():.4f} m")
        assert (kinds == 0).all() and status[-1] == capi.TRACKING_TRACKING, (s, first, kinds.tolist())
        assert e_vio < 0.5 * e_dr, (s, e_vio, e_dr)
