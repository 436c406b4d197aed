#!/usr/bin/env python3
"""Host clock around the synchronous host-pointer entries a drop-in integrator calls per frame: hv_klt_track, hv_rot_ransac and
hv_track_gate at 200 points on a warmed 752x480 context. Each call ends in the entry's own stream synchronise, so the figure is
upload + kernel + download + the library's host work (the staging carve of hv::Stage among it). For an A/B against another build of
the library set HV_LIB_OVERRIDE and alternate the two in one job.
usage: scripts/host_stage_bench.py [--reps N] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from hybvio_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
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
            host = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                run()
                host.append(time.perf_counter() - t0)
            res[name] = {"host_us_median": 1e6 * float(np.median(host)), "host_us_mean": 1e6 * float(np.mean(host)),
                         "host_us_min": 1e6 * float(np.min(host))}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
