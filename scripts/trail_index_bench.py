#!/usr/bin/env python3
"""Microbenchmark of the device pose-trail index: HV_K_TRAIL_INDEX event milliseconds per launch of hv_trail_select_batch_dev and
hv_trail_finish_batch_dev for 1024 stereo sets x 200 tracks, trail 20 (the reference's defaults), in steady state: a full trail
(21 keyframes), every frame a full keyframe, tracks that drift by a few pixels, 2 % of them replaced by new IDs every frame,
and visit outcomes that reach the success limit (a rejected track, then five inliers), so that every frame marks tracks,
carries a blacklist and removes a keyframe by the Hanoi rule. The state is not restored between repetitions: every timed frame
is the next frame of the same run. The same event pair around hv_trail_init_batch_dev on ONE set (a kernel that writes a few
hundred bytes) is reported as the floor of the method: event overhead plus an almost empty launch.
usage: scripts/trail_index_bench.py [--reps N] [--sets N] [--warm N] [--out file.json]"""
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


def frame_bytes(M, K, C, V, live, mean_len, n_cand, cand_len):
    """Bytes one set moves per frame, from the shapes: select reads the table, the column directory, the draws and,
    per live track, the older image points and used flags (score) and two older normalised points (velocity); it writes one
    observation row, the second row's velocities, the directory and the candidates' records. finish reads the records' outcomes and
    rewrites the directory, the used flags of the successes and kf_row."""
    table = live * (4 + 4 * 2 * C)
    directory = 2 * M * 4
    select_read = table + directory + live * 4 + live * (mean_len - 1) * (8 + 1) + live * 2 * C * 16
    select_write = live * C * (8 + 16 + 16) + live + live * C * 16 + directory + n_cand * cand_len * (4 + C * 3 * 16) + 4 * V * 4
    finish = V * 3 * 4 + 2 * directory + 5 * cand_len + 2 * K * 4 + M * 4
    return {"select_read": select_read, "select_write": select_write, "finish": finish}


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
            st_h[:6], gs_h[0], gs_h[1:6] = 0, CHI2, INLIER              # a candidate the set does not have is ignored
            status, gate = dev(st_h), dev(gs_h)
            ctx.trail_init_batch_dev(S, trail.table, params=gp)
        P = lambda x: x.data_ptr()
        select = lambda: ctx.trail_select_batch_dev(S, trail.table, table, cam, cam, P(keyframe), 0, P(frame_num), P(tm), P(draws),
                                                    P(o["draws_used"]), P(o["n_poses"]), P(o["pose_index"]), P(o["features"]), P(o["velocities"]),
                                                    P(o["y"]), P(o["cand_id"]), P(o["n_cand"]), params=gp)
        finish = lambda: ctx.trail_finish_batch_dev(S, trail.table, P(o["cand_id"]), P(o["n_cand"]), P(status), P(gate), 0, P(o["delete_ids"]),
                                                    P(o["n_delete"]), P(o["good"]), P(o["attempts"]), P(o["successes"]), P(o["discarded"]), params=gp)
        floor = lambda: ctx.trail_init_batch_dev(1, one.table, params=gp)
        next_id = M + 1
        times = {"select": [], "finish": [], "floor": []}
        stats = {"n_cand": [], "mean_len": [], "cand_len": [], "live": [], "discarded": set()}
        for f in range(a.warm + a.reps):
            xy += rng.uniform(-2.5, 2.5, xy.shape).astype(np.float32)
            new = rng.random((S, M)) < 0.02
            xy[new] = rng.uniform([40, 40], [W - 40, H - 40], (int(new.sum()), 2)).astype(np.float32)
            ids[new] = np.arange(next_id, next_id + int(new.sum()), dtype=np.int32)
            next_id += int(new.sum())
            with torch.cuda.stream(stream):
                t["ids"].copy_(dev(ids)); t["xy"].copy_(dev(xy)); t["second_xy"].copy_(dev(xy - np.float32(20)))
                frame_num.fill_(f + 1); tm.fill_(0.05 * (f + 1))
                draws.copy_(dev(rng.integers(0, 2 ** 32, (S, M), dtype=np.uint32).view(np.int32)))
            for name, call in (("select", select), ("finish", finish), ("floor", floor)):
                stream.synchronize()
                ctx.profile_enable(True)
                ctx.profile_reset()
                call()
                ms, launches = ctx.profile_read(capi.K_TRAIL_INDEX)
                ctx.profile_enable(False)
                assert launches == 1
                if f >= a.warm:
                    times[name].append(ms)
                if name == "select" and f >= a.warm:
                    L = trail.m["col_len"].cpu().numpy()
                    nc, npz = o["n_cand"].cpu().numpy(), o["n_poses"].cpu().numpy()
                    stats["n_cand"].append(float(nc.mean())); stats["live"].append(float((L > 0).sum(1).mean()))
                    stats["mean_len"].append(float(L[L > 0].mean())); stats["cand_len"].append(float(npz[npz > 0].mean()))
                if name == "finish" and f >= a.warm:
                    stats["discarded"] |= set(o["discarded"].cpu().numpy().tolist())
                    assert int(trail.m["n_keyframes"].min().item()) == K
        mean = lambda k: float(np.mean(stats[k]))
        res[f"{S}x{M}_trail{gp.cameraTrailLength}"] = {
            "select_us_median": 1e3 * float(np.median(times["select"])), "select_us_min": 1e3 * float(np.min(times["select"])),
            "finish_us_median": 1e3 * float(np.median(times["finish"])), "finish_us_min": 1e3 * float(np.min(times["finish"])),
            "floor_us_median": 1e3 * float(np.median(times["floor"])), "floor_us_min": 1e3 * float(np.min(times["floor"])),
            "reps": a.reps, "live_tracks_mean": mean("live"), "track_length_mean": mean("mean_len"), "candidates_mean": mean("n_cand"),
            "candidate_poses_mean": mean("cand_len"), "discarded_seen": sorted(int(x) for x in stats["discarded"]),
            "bytes_per_set": frame_bytes(M, K, 2, V, mean("live"), mean("mean_len"), mean("n_cand"), mean("cand_len"))}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
