#!/usr/bin/env python3
"""Microbenchmark of the five-point RANSAC (hv_ransac5*, HV_K_RANSAC5 events + a host clock around synchronised calls),
default parameters (prob 0.999, threshold 2 px, 75 iterations), synthetic two-view sets on a radially distorted pinhole
camera (752x480, 30 % outliers, 0.5 px noise):
  (a) latency: one 200-point set, hv_ransac5
  (b) throughput: 1024 sets x 200 points, one hv_ransac5_batch_dev launch
  (c) Durand-Kerner sweeps per hypothesis (from the numpy restatement, which runs the same iteration): the share of
      hypotheses and of sets that reach the 300-sweep cap
usage: scripts/ransac5_bench.py [--reps N] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hybvio_amd import capi  # noqa: E402
from oracle import orc  # noqa: E402
import ransac5_restatement as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    spec = R.CAMERAS["pinhole_radial"]
    ocam = orc.Camera(spec[0], *spec[1:5], coeffs=spec[5])
    gcam = capi.camera_model(spec[0], *spec[1:5], coeffs=spec[5])
    rng = np.random.default_rng(11)
    B, M = 1024, 200
    n_distinct = 64
    sets = [R.make_set(rng, (ocam, spec), M, 0.3, 0.5) for _ in range(n_distinct)]
    res = {"params": {"ransac5Prob": 0.999, "ransac5Threshold": 2.0, "ransacMaxIters": 75, "outliers": 0.3, "noise_px": 0.5}}
    with capi.Context(width=752, height=480) as ctx:
        c1, c2 = sets[0][0], sets[0][1]
        for _ in range(5):
            ctx.ransac5(c1, c2, gcam, gcam)
        ctx.profile_enable(True)
        ctx.profile_reset()
        host = []
        for k in range(a.reps):
            d = sets[k % n_distinct]
            t0 = time.perf_counter()
            st, E, sm = ctx.ransac5(d[0], d[1], gcam, gcam)
            host.append(time.perf_counter() - t0)
        ms, n = ctx.profile_read(capi.K_RANSAC5)
        res["a_latency"] = {"points": M, "kernel_us_mean": 1e3 * ms / n, "host_call_us_median": 1e6 * float(np.median(host)),
                            "host_call_us_p10": 1e6 * float(np.percentile(host, 10)), "host_call_us_p90": 1e6 * float(np.percentile(host, 90)),
                            "launches": n}
        ctx.profile_enable(False)
        cc1 = np.stack([sets[i % n_distinct][0] for i in range(B)])
        cc2 = np.stack([sets[i % n_distinct][1] for i in range(B)])
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        d_c1, d_c2 = torch.from_numpy(cc1).cuda(), torch.from_numpy(cc2).cuda()
        d_n = torch.full((B,), M, dtype=torch.int32, device="cuda")
        d_st = torch.zeros((B, M), dtype=torch.int32, device="cuda")
        d_sm = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        run = lambda: ctx.ransac5_batch_dev(B, M, d_n.data_ptr(), d_c1.data_ptr(), d_c2.data_ptr(), gcam, gcam, d_st.data_ptr(), 0,
                                            d_sm.data_ptr())
        for _ in range(2):
            run()
        stream.synchronize()
        ctx.profile_enable(True)
        ctx.profile_reset()
        host = []
        for _ in range(max(5, a.reps // 20)):
            t0 = time.perf_counter()
            run()
            stream.synchronize()
            host.append(time.perf_counter() - t0)
        ms, n = ctx.profile_read(capi.K_RANSAC5)
        sm = d_sm.cpu().numpy()
        res["b_throughput"] = {"sets": B, "points_per_set": M, "kernel_ms_mean": ms / n, "host_ms_median": 1e3 * float(np.median(host)),
                               "sets_per_s": B / (ms / n * 1e-3), "mean_iterations_run": float(sm[:, 2].mean()), "launches": n}
        ctx.profile_enable(False)
    # (c) Durand-Kerner sweeps: the same 75 hypotheses per set as the kernel solves
    f = (spec[1] + spec[2]) * 0.5
    runs = R.registrator_runs([(*R.normalize(s[0], s[1], ocam, ocam)[:2], R.threshold(f, f)) for s in sets])
    capped = np.array([r.dk_capped for r in runs])
    res["c_durand_kerner"] = {"sets": n_distinct, "hypotheses": 75 * n_distinct, "hypotheses_at_cap_share": float(capped.sum() / (75 * n_distinct)),
                              "sets_with_a_capped_hypothesis_share": float((capped > 0).mean())}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
