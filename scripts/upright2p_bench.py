#!/usr/bin/env python3
"""Microbenchmark of the stereo upright 2-point filter (hv_upright2p*, HV_K_RANSAC3 events), default parameters, synthetic stereo
sets on a radially distorted pinhole rig (752x480, baseline 0.11, 30 % outliers, 0.5 px noise, general attitude, yaw error drawn
from (-pi, pi), tilt error 0.1 degree), with hv_ransac3_batch_dev on the same sets beside it in the same process:
  (a) latency: one 200-feature set, hv_upright2p
  (b) throughput: 1024 sets x 200 features, one hv_upright2p_batch_dev launch; the same sets through hv_ransac3_batch_dev
  (c) where the time of (b) goes: both launches with one iteration (MinIterations = MaxIterations = 1: the gather, one solve, the
      cost sums of one hypothesis), and the upright launch at 400 features (the cost sums double, the sampler does not)
usage: scripts/upright2p_bench.py [--reps N] [--out file.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hybvio_amd import capi  # noqa: E402
from oracle import orc  # noqa: E402
import ransac3_restatement as R3  # noqa: E402
import ransac5_restatement as R5  # noqa: E402
import upright2p_restatement as U  # noqa: E402


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
    B, n_distinct, T = 1024, 64, U.SECOND_TO_FIRST
    make = lambda M: [U.make_set(rng, ocam, M, 0.3, 0.5, psi=rng.uniform(-math.pi, math.pi), tilt_deg=0.1) for _ in range(n_distinct)]
    draws = np.stack([orc.mt19937_draws(4649 + i, 3 * R3.MAX_ITERS) for i in range(n_distinct)])
    res = {"params": {"defaults": True, "outliers": 0.3, "noise_px": 0.5, "tilt_deg": 0.1}}
    with capi.Context(width=752, height=480) as ctx:
        sets = make(200)
        call = lambda k: ctx.upright2p(sets[k]["status"], sets[k]["prev_left"], sets[k]["prev_right"], sets[k]["cur_left"], gcam, gcam, T,
                                       sets[k]["poses"], draws[k])
        for _ in range(5):
            call(0)
        ctx.profile_enable(True)
        ctx.profile_reset()
        iters = [int(call(k % n_distinct)[2][2]) for k in range(a.reps)]
        ms, n = ctx.profile_read(capi.K_RANSAC3)
        res["a_latency"] = {"points": 200, "kernel_us_mean": 1e3 * ms / n, "mean_iterations_run": float(np.mean(iters)), "launches": n}
        ctx.profile_enable(False)
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        d_dr = torch.from_numpy(np.stack([draws[i % n_distinct] for i in range(B)])).cuda()

        def timed(M, sets2, which, params=None, reps=5):
            stack = lambda key: torch.from_numpy(np.stack([sets2[i % n_distinct][key] for i in range(B)])).cuda()
            t_pl, t_pr, t_cl, t_st0, t_po = stack("prev_left"), stack("prev_right"), stack("cur_left"), stack("status"), stack("poses")
            t_n = torch.full((B,), M, dtype=torch.int32, device="cuda")
            t_st, t_sm = t_st0.clone(), torch.zeros((B, 4), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def go():
                with torch.cuda.stream(stream):
                    t_st.copy_(t_st0)                                   # the statuses are in/out
                if which == "upright2p":
                    ctx.upright2p_batch_dev(B, M, t_n.data_ptr(), t_pl.data_ptr(), t_pr.data_ptr(), t_cl.data_ptr(), gcam, gcam, T,
                                            t_po.data_ptr(), d_dr.data_ptr(), t_st.data_ptr(), 0, t_sm.data_ptr(), params=params)
                else:                                                   # (the draws are laid out [sets][3 * 500] for both)
                    ctx.ransac3_batch_dev(B, M, t_n.data_ptr(), t_pl.data_ptr(), t_pr.data_ptr(), t_cl.data_ptr(), gcam, gcam, T,
                                          d_dr.data_ptr(), t_st.data_ptr(), 0, t_sm.data_ptr(), params=params)
            for _ in range(2):
                go()
            stream.synchronize()
            ctx.profile_enable(True)
            ctx.profile_reset()
            for _ in range(reps):
                go()
            stream.synchronize()
            ms, n = ctx.profile_read(capi.K_RANSAC3)
            ctx.profile_enable(False)
            sm = t_sm.cpu().numpy()
            return {"sets": B, "points_per_set": M, "kernel_ms_mean": ms / n, "mean_iterations_run": float(sm[:, 2].mean()),
                    "mean_inliers": float(sm[:, 0].mean()), "launches": n}
        reps = max(5, a.reps // 10)
        one_u = capi.upright2p_default_params(ransacStereoUpright2pMinIterations=1, ransacStereoUpright2pMaxIterations=1)
        one_3 = capi.ransac3_default_params(ransac3MinIterations=1, ransac3MaxIterations=1)
        res["b_throughput"] = {"upright2p": timed(200, sets, "upright2p", reps=reps), "ransac3": timed(200, sets, "ransac3", reps=reps)}
        res["c_breakdown"] = {"upright2p_one_iteration_200": timed(200, sets, "upright2p", one_u),
                              "ransac3_one_iteration_200": timed(200, sets, "ransac3", one_3),
                              "upright2p_default_400": timed(400, make(400), "upright2p")}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
