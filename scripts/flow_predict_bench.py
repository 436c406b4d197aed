#!/usr/bin/env python3
"""Microbenchmark of the device optical-flow predictor: HV_K_TRAIL_INDEX event milliseconds per launch of
hv_flow_predict_batch_dev for 1024 stereo sets x 200 tracks, trail 20 (the reference's defaults), every prediction type with
and without reuse_distance. The index is brought to the steady state of scripts/trail_index_bench.py first (a full trail of 21
keyframes, tracks that drift by a few pixels, 2 % of them replaced per frame, so that most tracks are longer than ten keyframes
and are triangulated); the means are a camera that moves 0.1 m per keyframe, so that the triangulations are healthy. Nothing
changes between the repetitions of a call: the predictor reads the state and writes only its outputs. For reference the same
event pair is put around hv_trail_select_batch_dev of the next frame (once: it advances the state) and around a one-set
hv_trail_init_batch_dev launch, the floor of the method.
usage: scripts/flow_predict_bench.py [--reps N] [--sets N] [--warm N] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from hybvio_amd import capi  # noqa: E402

W, H = 752, 480
TRI_NOT_VISITED, INLIER, NOT_COMPUTED, CHI2 = -1, 0, 1, 3
TYPES = {"left": capi.FLOW_PREDICT_LEFT, "right": capi.FLOW_PREDICT_RIGHT, "stereo": capi.FLOW_PREDICT_STEREO}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sets", type=int, default=1024)
    ap.add_argument("--warm", type=int, default=45)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import platform

    import torch
    S, M = a.sets, 200
    gp = capi.trail_index_default_params()
    K, V = gp.cameraTrailLength + 1, gp.maxVisualUpdates
    res = {"params": {"image": [W, H], "sets": S, "maxTracks": M, "trail": gp.cameraTrailLength, "stereo": True, "warm_frames": a.warm},
           "box": {"host": platform.node(), "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d")}}
    rng = np.random.default_rng(5)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    cam = capi.camera_model("pinhole", 458.6, 457.3, 367.2, 248.4, coeffs=[-0.28, 0.07, 0.0])
    T0, T1 = np.eye(4), np.eye(4)
    T0[:3, 3], T1[:3, 3] = [0.05, -0.02, 0.01], [-0.06, -0.02, 0.01]
    fp = capi.flow_predict_default_params(T0, T1)
    with capi.Context(width=W, height=H) as ctx:
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
            trail, one = capi.TrailIndex(S, gp), capi.TrailIndex(1, gp)
            xy = rng.uniform([40, 40], [W - 40, H - 40], (S, M, 2)).astype(np.float32)
            ids = np.tile(np.arange(1, M + 1, dtype=np.int32), (S, 1))
            t = dict(n_tracks=dev(np.full(S, M, np.int32)), ids=dev(ids), xy=dev(xy), second_xy=dev(xy - np.float32(20)))
            table = capi.track_table(**{k: v.data_ptr() for k, v in t.items()})
            keyframe, frame_num, tm = dev(np.ones(S, np.int32)), z(S, torch.int32), z(S, torch.float64)
            draws = z((S, M), torch.int32)
            o = dict(draws_used=z(S, torch.int32), n_poses=z((V, S), torch.int32), pose_index=z((V, S, K), torch.int32),
                     features=z((V, S, 2 * K, 2), torch.float64), velocities=z((V, S, 2 * K, 2), torch.float64), y=z((V, S, 4 * K), torch.float64),
                     cand_id=z((V, S), torch.int32), n_cand=z(S, torch.int32), delete_ids=z((S, M), torch.int32), n_delete=z(S, torch.int32),
                     good=z(S, torch.uint8), attempts=z(S, torch.int32), successes=z(S, torch.int32), discarded=z(S, torch.int32))
            st_h, gs_h = np.full((V, S, 2), TRI_NOT_VISITED, np.int32), np.full((V, S), NOT_COMPUTED, np.int32)
            st_h[:6], gs_h[0], gs_h[1:6] = 0, CHI2, INLIER
            status, gate = dev(st_h), dev(gs_h)
            pred, dist = z((S, M, 2), torch.float32), z((S, M), torch.float64)
            ctx.trail_init_batch_dev(S, trail.table, params=gp)
            ekf = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=gp.cameraTrailLength), batch=S)
            # the current pose and the history poses: 0.1 m apart along x, orientations close to the identity
            m = rng.normal(0.0, 1.0, (S, ekf.n))
            for k in range(K):
                ip, io = (0, 6) if k == 0 else (20 + 7 * (k - 1), 20 + 7 * (k - 1) + 3)
                q = np.array([1.0, 0.0, 0.0, 0.0]) + rng.normal(0.0, 5e-3, (S, 4))
                m[:, ip:ip + 3] = np.array([-0.1 * k, 0.0, 0.0]) + rng.normal(0.0, 2e-3, (S, 3))
                m[:, io:io + 4] = q / np.linalg.norm(q, axis=1, keepdims=True)
            for b in range(S):
                ekf.set_state(b, m=m[b])
        P = lambda x: x.data_ptr()
        select = lambda: ctx.trail_select_batch_dev(S, trail.table, table, cam, cam, P(keyframe), 0, P(frame_num), P(tm), P(draws),
                                                    P(o["draws_used"]), P(o["n_poses"]), P(o["pose_index"]), P(o["features"]), P(o["velocities"]),
                                                    P(o["y"]), P(o["cand_id"]), P(o["n_cand"]), params=gp)
        finish = lambda: ctx.trail_finish_batch_dev(S, trail.table, P(o["cand_id"]), P(o["n_cand"]), P(status), P(gate), 0, P(o["delete_ids"]),
                                                    P(o["n_delete"]), P(o["good"]), P(o["attempts"]), P(o["successes"]), P(o["discarded"]), params=gp)
        floor = lambda: ctx.trail_init_batch_dev(1, one.table, params=gp)
        predict = lambda ty, reuse: ekf.flow_predict_batch_dev(fp, ty, gp, trail.table, table, P(t["xy"]), cam, cam, P(pred), P(dist), reuse)

        def load_frame(f):
            nonlocal xy, ids, next_id
            xy += rng.uniform(-2.5, 2.5, xy.shape).astype(np.float32)
            new = rng.random((S, M)) < 0.02
            xy[new] = rng.uniform([40, 40], [W - 40, H - 40], (int(new.sum()), 2)).astype(np.float32)
            ids[new] = np.arange(next_id, next_id + int(new.sum()), dtype=np.int32)
            next_id += int(new.sum())
            with torch.cuda.stream(stream):
                t["ids"].copy_(dev(ids)); t["xy"].copy_(dev(xy)); t["second_xy"].copy_(dev(xy - np.float32(20)))
                frame_num.fill_(f + 1); tm.fill_(0.05 * (f + 1))
                draws.copy_(dev(rng.integers(0, 2 ** 32, (S, M), dtype=np.uint32).view(np.int32)))

        def timed(call):
            stream.synchronize()
            ctx.profile_enable(True)
            ctx.profile_reset()
            call()
            ms, launches = ctx.profile_read(capi.K_TRAIL_INDEX)
            ctx.profile_enable(False)
            assert launches == 1
            return ms

        next_id = M + 1
        for f in range(a.warm):
            load_frame(f)
            select(); finish()
        load_frame(a.warm)                                       # the table of the frame the predictor runs on: 2 % of its tracks have no column
        stream.synchronize()
        L = trail.m["col_len"].cpu().numpy()
        assert int(trail.m["n_keyframes"].min().item()) == K
        out = {"reps": a.reps, "live_columns_mean": float((L > 0).sum(1).mean()), "columns_longer_than_10_mean": float((L > 10).sum(1).mean())}
        for name, ty in TYPES.items():
            for reuse in (False, True):
                if reuse:
                    predict(ty, False)                           # the distances a reusing call reads
                ts = [timed(lambda: predict(ty, reuse)) for _ in range(a.reps + 3)][3:]
                key = f"{name}_{'reuse' if reuse else 'triangulate'}"
                out[key + "_us_median"], out[key + "_us_min"] = 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts))
        stream.synchronize()
        d = dist.cpu().numpy()
        out["triangulated_in_front_share"] = float((d > fp.predictOpticalFlowMinTriangulationDistance).mean())
        out["pred_moved_share"] = float((pred.cpu().numpy() != xy).any(axis=2).mean())
        ts = [timed(floor) for _ in range(a.reps)]
        out["floor_us_median"], out["floor_us_min"] = 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts))
        out["select_next_frame_us"] = 1e3 * timed(select)        # one launch: it advances the state
        res[f"{S}x{M}_trail{gp.cameraTrailLength}"] = out
        ekf.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
