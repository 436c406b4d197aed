#!/usr/bin/env python3
"""Microbenchmark of the stereo RANSAC3 filter (hv_ransac3*, HV_K_RANSAC3 events + a host clock around synchronised calls),
default parameters (error threshold 1e-4, failure probability 1e-4, 50..500 iterations, MLE cost), synthetic stereo sets on
a radially distorted pinhole rig (752x480, baseline 0.11, 30 % outliers, 0.5 px noise):
  (a) latency: one 200-feature set, hv_ransac3
  (b) throughput: 1024 sets x 200 features, one hv_ransac3_batch_dev launch
  (c) where the time of (b) goes: the same launch with one iteration (ransac3MinIterations = ransac3MaxIterations = 1: the gather,
      one P3P, four cost sums), with the default parameters at 200 features, and at 400 features (the cost sums double, the P3Ps
      and the sampler do not)
(a) and (b) record the mean number of iterations the loop ran (the kernel solves hypotheses in rounds of 64 and stops with it).
usage: scripts/ransac3_bench.py [--reps N] [--out file.json]"""
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
import ransac3_restatement as R  # noqa: E402
import ransac5_restatement as R5  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    spec = R5.CAMERAS["pinhole_radial"]
    ocam = orc.Camera(spec[0], *spec[1:5], coeffs=spec[5])
    gcam = capi.camera_model(spec[0], *spec[1:5], coeffs=spec[5])
    rng = np.random.default_rng(11)
    B, M = 1024, 200
    n_distinct = 64
    T = R.SECOND_TO_FIRST
    sets = [R.make_set(rng, ocam, M, 0.3, 0.5) for _ in range(n_distinct)]
    draws = [orc.mt19937_draws(4649 + i, 3 * R.MAX_ITERS) for i in range(n_distinct)]
    res = {"params": {"ransac3ErrorThresh": 1e-4, "ransac3FailureProbability": 1e-4, "ransac3MaxIterations": 500,
                      "ransac3MinIterations": 50, "ransac3UseMle": 1, "outliers": 0.3, "noise_px": 0.5}}
    call = lambda d, dr: ctx.ransac3(d["status"], d["prev_left"], d["prev_right"], d["cur_left"], gcam, gcam, T, dr)
    with capi.Context(width=752, height=480) as ctx:
        for _ in range(5):
            call(sets[0], draws[0])
        ctx.profile_enable(True)
        ctx.profile_reset()
        host, iters = [], []
        for k in range(a.reps):
            t0 = time.perf_counter()
            st, pose, sm = call(sets[k % n_distinct], draws[k % n_distinct])
            host.append(time.perf_counter() - t0)
            iters.append(int(sm[2]))
        ms, n = ctx.profile_read(capi.K_RANSAC3)
        res["a_latency"] = {"points": M, "kernel_us_mean": 1e3 * ms / n, "host_call_us_median": 1e6 * float(np.median(host)),
                            "host_call_us_p10": 1e6 * float(np.percentile(host, 10)), "host_call_us_p90": 1e6 * float(np.percentile(host, 90)),
                            "mean_iterations_run": float(np.mean(iters)), "launches": n}
        ctx.profile_enable(False)
        stack = lambda key: np.stack([sets[i % n_distinct][key] for i in range(B)])
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        d_pl, d_pr, d_cl = (torch.from_numpy(stack(k)).cuda() for k in ("prev_left", "prev_right", "cur_left"))
        d_dr = torch.from_numpy(np.stack([draws[i % n_distinct] for i in range(B)])).cuda()
        d_n = torch.full((B,), M, dtype=torch.int32, device="cuda")
        d_st0 = torch.from_numpy(stack("status")).cuda()
        d_st = d_st0.clone()
        d_sm = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def run():
            with torch.cuda.stream(stream):
                d_st.copy_(d_st0)                                       # the statuses are in/out
            ctx.ransac3_batch_dev(B, M, d_n.data_ptr(), d_pl.data_ptr(), d_pr.data_ptr(), d_cl.data_ptr(), gcam, gcam, T,
                                  d_dr.data_ptr(), d_st.data_ptr(), 0, d_sm.data_ptr())
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
        ms, n = ctx.profile_read(capi.K_RANSAC3)
        sm = d_sm.cpu().numpy()
        res["b_throughput"] = {"sets": B, "points_per_set": M, "kernel_ms_mean": ms / n, "host_ms_median": 1e3 * float(np.median(host)),
                               "sets_per_s": B / (ms / n * 1e-3), "mean_iterations_run": float(sm[:, 2].mean()),
                               "mean_inliers": float(sm[:, 0].mean()), "launches": n}
        ctx.profile_enable(False)

        # (c) the gather alone, and the slope of the cost phase in the number of correspondences
        def timed(M2, sets2, params):
            stack2 = lambda key: np.stack([sets2[i % len(sets2)][key] for i in range(B)])
            t_pl, t_pr, t_cl = (torch.from_numpy(stack2(k)).cuda() for k in ("prev_left", "prev_right", "cur_left"))
            t_n = torch.full((B,), M2, dtype=torch.int32, device="cuda")
            t_st0 = torch.from_numpy(stack2("status")).cuda()
            t_st, t_sm = t_st0.clone(), torch.zeros((B, 4), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def go():
                with torch.cuda.stream(stream):
                    t_st.copy_(t_st0)
                ctx.ransac3_batch_dev(B, M2, t_n.data_ptr(), t_pl.data_ptr(), t_pr.data_ptr(), t_cl.data_ptr(), gcam, gcam, T,
                                      d_dr.data_ptr(), t_st.data_ptr(), 0, t_sm.data_ptr(), params=params)
            go()
            stream.synchronize()
            ctx.profile_enable(True)
            ctx.profile_reset()
            for _ in range(5):
                go()
            ms, n = ctx.profile_read(capi.K_RANSAC3)
            ctx.profile_enable(False)
            return {"points_per_set": M2, "kernel_ms_mean": ms / n, "mean_iterations_run": float(t_sm.cpu().numpy()[:, 2].mean())}
        sets400 = [R.make_set(rng, ocam, 400, 0.3, 0.5) for _ in range(16)]
        res["c_breakdown"] = {
            "one_iteration_200": timed(M, sets, capi.ransac3_default_params(ransac3MinIterations=1, ransac3MaxIterations=1)),
            "default_200": timed(M, sets, None),
            "default_400": timed(400, sets400, None)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
