#!/usr/bin/env python3
"""Microbenchmark of the stereo track gate (HV_K_STEREO_GATE events + a host clock around synchronised launches): default
parameters (maxStereoEpipolarDistance 10, so every TRACKED stereo feature takes the epipolar check), a radially distorted
pinhole camera pair at 752x480, cam0ToCam1 = a 0.1 baseline with a small rotation, right corners 20 px left of the left ones
with 1 px noise and 10 % moved off their curves:
  (a) track_gate_kernel, 1 set x 200 and 1024 sets x 200 features (hv_track_gate_batch_dev)
  (b) detection_filter_kernel, 1 set x 200 and 1024 sets x 200 corners (hv_detection_filter_batch_dev)
  (c) flow_status_kernel, 1024 sets x 200 (hv_flow_status_batch_dev)
usage: scripts/stereo_gate_bench.py [--reps N] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from hybvio_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    w, h, M = 752, 480, 200
    cam = capi.camera_model("pinhole", 458.7, 457.3, 367.2, 248.4, coeffs=[-0.2834, 0.0740, 0.0])
    T = np.eye(4)
    T[:3, 3] = (-0.1, 0.002, 0.0)
    gp = capi.stereo_gate_default_params(cam0ToCam1=T)
    rng = np.random.default_rng(3)
    res = {"params": {"maxStereoEpipolarDistance": 10.0, "points_per_set": M, "image": [w, h], "camera": "pinhole k1 -0.2834"}}
    with capi.Context(width=w, height=h) as ctx:
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        for B in (1, 1024):
            left = rng.uniform([8, 8], [w - 8, h - 8], (B, M, 2)).astype(np.float32)
            right = (left - np.array([20, 0], np.float32) + rng.normal(0, 1, left.shape)).astype(np.float32)
            off = rng.random((B, M)) < 0.1
            right[off, 1] += 25
            lk = (rng.random((B, M)) < 0.95).astype(np.uint8)
            dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
            d_n, d_l, d_r, d_lk = dev(np.full(B, M, np.int32)), dev(left), dev(right), dev(lk)
            d_fs, d_ss = torch.zeros((B, M), dtype=torch.int32, device="cuda"), torch.zeros((B, M), dtype=torch.int32, device="cuda")
            d_ts, d_mask = torch.zeros_like(d_fs), torch.zeros((B, M), dtype=torch.uint8, device="cuda")
            d_ol, d_or, d_no = torch.zeros_like(d_l), torch.zeros_like(d_r), torch.zeros(B, dtype=torch.int32, device="cuda")
            ctx.flow_status_batch_dev(B, M, d_n.data_ptr(), d_r.data_ptr(), d_lk.data_ptr(), d_ss.data_ptr())
            ctx.flow_status_batch_dev(B, M, d_n.data_ptr(), d_l.data_ptr(), d_lk.data_ptr(), d_fs.data_ptr())
            stream.synchronize()
            runs = {
                "gate": lambda: ctx.track_gate_batch_dev(B, M, d_n.data_ptr(), d_l.data_ptr(), d_r.data_ptr(), d_ss.data_ptr(), 0, cam, cam,
                                                         d_ts.data_ptr(), d_mask.data_ptr(), params=gp),
                "detection_filter": lambda: ctx.detection_filter_batch_dev(B, M, d_n.data_ptr(), d_l.data_ptr(), d_r.data_ptr(),
                                                                           d_ss.data_ptr(), cam, cam, 0, d_ol.data_ptr(), d_or.data_ptr(),
                                                                           d_no.data_ptr(), params=gp),
                "flow_status": lambda: ctx.flow_status_batch_dev(B, M, d_n.data_ptr(), d_l.data_ptr(), d_lk.data_ptr(), d_fs.data_ptr()),
            }
            for name, run in runs.items():
                if name == "flow_status" and B == 1:
                    continue
                for _ in range(3):
                    if name == "gate":
                        d_ts.copy_(d_fs)
                    run()
                stream.synchronize()
                ctx.profile_enable(True)
                ctx.profile_reset()
                host = []
                for _ in range(a.reps):
                    if name == "gate":
                        with torch.cuda.stream(stream):
                            d_ts.copy_(d_fs)
                        stream.synchronize()
                    t0 = time.perf_counter()
                    run()
                    stream.synchronize()
                    host.append(time.perf_counter() - t0)
                ms, n = ctx.profile_read(capi.K_STEREO_GATE)
                ctx.profile_enable(False)
                r = {"sets": B, "kernel_us_mean": 1e3 * ms / n, "host_us_median": 1e6 * float(np.median(host)),
                     "features_per_s": B * M / (ms / n * 1e-3), "launches": n}
                if name == "gate":
                    ts = d_ts.cpu().numpy()
                    r["status_counts"] = {int(k): int(v) for k, v in zip(*np.unique(ts, return_counts=True))}
                if name == "detection_filter":
                    r["kept_mean"] = float(d_no.cpu().numpy().mean())
                res[f"{name}_{B}x{M}"] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
