#!/usr/bin/env python3
"""Host clock around the synchronous host-pointer entries a drop-in integrator calls per frame: hv_klt_track, hv_rot_ransac and
hv_track_gate at 200 points on a warmed 752x480 context, and the single-filter chain hv_ekf_predict_n (10 samples) + hv_ekf_update
(2 rows) + hv_ekf_visual_track (10 stereo poses) at trail 20. Each call ends in a stream synchronise, so the figure is upload +
kernel + download + the library's host work (the staging of hv::Stage among it). --memory adds the change of the device's free
memory across hv_ekf_create for trail 20 x 1024 filters (a device-wide reading: other processes move it). For an A/B against
another build of the library set HV_LIB_OVERRIDE and alternate the two in one job.
usage: scripts/host_stage_bench.py [--reps N] [--memory] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from hybvio_amd import capi, synth  # noqa: E402


def clock(run, reps, before=None):
    host = []
    for _ in range(reps):
        if before:
            before()
        t0 = time.perf_counter()
        run()
        host.append(time.perf_counter() - t0)
    return {"host_us_median": 1e6 * float(np.median(host)), "host_us_mean": 1e6 * float(np.mean(host)), "host_us_min": 1e6 * float(np.min(host))}


def ekf_chain(res, reps):
    rng = np.random.default_rng(5)
    trail, npose, ns = 20, 10, 10
    T1, T2, means, idx, feat = synth.visual_tracks(rng, 1, trail, npose, True)
    n = means.shape[1]
    A = rng.normal(size=(n, n)) * 1e-3
    P = np.eye(n) * 1e-4 + A @ A.T
    vel, ys = 0.2 * rng.normal(size=feat.shape), feat.reshape(1, -1) + 2e-3 * rng.normal(size=(1, feat.shape[1] * 2))
    vp = capi.vu_default_params(imu_to_camera=T1, second_imu_to_camera=T2)
    dt, gyro, acc = np.full((ns, 1), 0.005), 0.05 * rng.normal(size=(ns, 1, 3)), np.array([0, 0, 9.8]) + 0.05 * rng.normal(size=(ns, 1, 3))
    H, y, r = rng.normal(size=(1, 2, n)), 0.01 * rng.normal(size=(1, 2)), np.full(1, 1e-2)
    f64 = lambda a: a.ctypes.data_as(capi.f64p)
    with capi.Context(width=64, height=64, levels=1, pool_size=1) as ctx:
        g = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=trail), 1)

        def chain():
            rc = capi.lib().hv_ekf_predict_n(g._h, ns, f64(dt), f64(gyro), f64(acc))
            assert rc == 0, rc
            g.update(H, y, r)
            g.visual_track(vp, idx, feat, vel, ys, 1.5, 0.05)
        reset = lambda: g.set_state(0, means[0], P)                   # (outside the clock)
        for _ in range(20):
            reset(); chain()
        res["ekf_chain"] = clock(chain, reps, before=reset)
        g.close()


def ekf_create_memory(res):
    import torch
    with capi.Context(width=64, height=64, levels=1, pool_size=1) as ctx:
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        g = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=20), 1024)
        free1 = torch.cuda.mem_get_info()[0]
        res["ekf_create_1024x_trail20_bytes"] = int(free0 - free1)
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--memory", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h, M = 752, 480, 200
    cam = capi.camera_model("pinhole", 458.7, 457.3, 367.2, 248.4, coeffs=[-0.2834, 0.0740, 0.0])
    T = np.eye(4)
    T[:3, 3] = (-0.1, 0.002, 0.0)
    gp = capi.stereo_gate_default_params(cam0ToCam1=T)
    rng = np.random.default_rng(3)
    left, _, _ = synth.stereo_sequence(7, w, h, 2)
    pts = synth.grid_points(w, h, M)
    moved = (pts + [-20.0, 0.0] + rng.normal(0, 1, pts.shape)).astype(np.float32)
    pairs, ss, ts = rng.integers(0, M, (100, 2)), np.zeros(M, np.int32), np.zeros(M, np.int32)
    res = {"library": os.environ.get("HV_LIB_OVERRIDE", "default"), "points": M, "image": [w, h], "reps": a.reps}
    with capi.Context(width=w, height=h, max_tracks=M) as ctx:
        s0, s1 = ctx.acquire(), ctx.acquire()
        ctx.build(s0, left[0]); ctx.build(s1, left[1])
        runs = {
            "klt_track": lambda: ctx.klt_track(s0, s1, pts),
            "rot_ransac": lambda: ctx.rot_ransac(pts, moved, cam, cam, pairs, 4e-4),
            "track_gate": lambda: ctx.track_gate(pts, moved, ss, ts, cam, cam, params=gp),
        }
        for run in runs.values():                                 # every entry has grown the staging it needs
            for _ in range(10):
                run()
        for name, run in runs.items():
            for _ in range(10):
                run()
            res[name] = clock(run, a.reps)
    ekf_chain(res, a.reps)
    if a.memory:
        ekf_create_memory(res)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
