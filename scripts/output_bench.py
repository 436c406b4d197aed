#!/usr/bin/env python3
"""Launch time of the output entry (hv_output_dev, csrc/output.hip; HV_K_EKF_CONTROL events) at the shape a lane runs: 1024 resident
sequences, cameraTrailLength 20 (n = 160), maxVisualUpdates 20, maxTracks 200, stereo.
  full_trail        every set with 20 historical poses and 20 visited candidates, per-set SLAM transforms
  short_trail       every set with one historical pose and no candidate (the first frames of a sequence)
  full_trail_no_candidates, short_trail_20_candidates: the two mixed shapes, to tell the trail's share from the point cloud's
  all_frozen        every set frozen: the launch floor
Per figure: `rounds` rounds of `calls` launches; a round's figure is the mean event time of its launches; reported are the median,
minimum and maximum over the rounds, as scripts/session_bench.py does for the session entries.
usage: scripts/output_bench.py [--rounds N] [--calls N] [--reverse] [--out file.json]
       --reverse measures the figures in the opposite order, to tell an effect of the order from a difference between them"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from hybvio_amd import capi  # noqa: E402

B, TRAIL, M, V = 1024, 20, 200, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reverse", action="store_true")
    a = ap.parse_args()
    import torch
    rng = np.random.default_rng(1)
    K, n = TRAIL + 1, 20 + 7 * TRAIL
    res = {"sets": B, "n": n, "maxVisualUpdates": V, "maxTracks": M, "reverse": a.reverse, "rounds": a.rounds, "calls_per_round": a.calls, "us": {}}
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    with capi.Context(width=752, height=480, levels=1, pool_size=1) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        g = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=TRAIL), B)
        means = rng.normal(size=(B, n))
        for k in range(-1, TRAIL):
            o = 6 if k < 0 else 20 + 7 * k + 3
            means[:, o:o + 4] /= np.linalg.norm(means[:, o:o + 4], axis=1, keepdims=True)
        A = rng.normal(size=(n, n))
        P = 1e-2 * (A @ A.T / n + 0.1 * np.eye(n))
        for b in range(B):
            g.set_state(b, means[b], P)
        ses = capi.session_state(B, 60)
        ses.m["first_sample_t"].fill_(100.0); ses.m["time"].fill_(12.5)
        ip = capi.trail_index_default_params(cameraTrailLength=TRAIL, maxTracks=M, maxVisualUpdates=V)
        trail = capi.TrailIndex(B, ip)
        ctx.trail_init_batch_dev(B, trail.table, params=ip)
        trail.m["timestamp"].copy_(dev(rng.uniform(1, 100, (B, K))))
        trail.m["image_point"].copy_(dev(rng.uniform(0, 700, (B, K, M, 2, 2)).astype(np.float32)))
        trail.m["cand_col"].copy_(dev(rng.integers(0, M, (B, V)).astype(np.int32)))
        op = capi.output_default_params(maxSuccessfulVisualUpdates=0)      # no success limit: every visited candidate is walked
        out = capi.Output(B, op)
        status = np.zeros((V, B, 2), np.int32)
        gate = rng.integers(0, 2, (V, B)).astype(np.int32) * 3             # INLIER or CHI2
        W = np.tile(np.eye(4), (B, 1, 1))
        for b in range(B):
            ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
            Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
            ang = rng.uniform(0, 3)
            W[b, :3, :3] = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)
            W[b, :3, 3] = rng.uniform(-5, 5, 3)
        arrays = dict(cand_id_dev=dev(rng.integers(1, 10 ** 6, (V, B)).astype(np.int32)), n_candidates_dev=dev(np.full(B, V, np.int32)),
                      status_dev=dev(status), gate_status_dev=dev(gate), pf_dev=dev(rng.uniform(-8, 8, (V, B, 3))),
                      tracking_status_dev=dev(np.ones(B, np.int32)), frozen_dev=dev(np.zeros(B, np.uint8)),
                      stationary_dev=dev(np.zeros(B, np.uint8)), slam_to_odometry_dev=dev(W.reshape(B, 16)),
                      odometry_to_slam_dev=dev(np.linalg.inv(W).reshape(B, 16)), ready_dev=dev(np.ones(B, np.uint8)))
        frame = capi.output_frame(**{k: v.data_ptr() for k, v in arrays.items()})
        call = lambda: g.output_dev(op, ses, trail.table, frame, out)

        def full_trail():
            trail.m["n_keyframes"].fill_(K); arrays["n_candidates_dev"].fill_(V); arrays["frozen_dev"].fill_(0)

        def short_trail():
            trail.m["n_keyframes"].fill_(2); arrays["n_candidates_dev"].fill_(0); arrays["frozen_dev"].fill_(0)

        def full_trail_no_candidates():
            trail.m["n_keyframes"].fill_(K); arrays["n_candidates_dev"].fill_(0); arrays["frozen_dev"].fill_(0)

        def short_trail_20_candidates():
            trail.m["n_keyframes"].fill_(2); arrays["n_candidates_dev"].fill_(V); arrays["frozen_dev"].fill_(0)

        def all_frozen():
            arrays["frozen_dev"].fill_(1)

        ctx.profile_enable(True)
        figures = [("full_trail", full_trail), ("short_trail", short_trail), ("full_trail_no_candidates", full_trail_no_candidates),
                   ("short_trail_20_candidates", short_trail_20_candidates), ("all_frozen", all_frozen)]
        for name, prepare in (figures[::-1] if a.reverse else figures):
            prepare()                                                      # (outside the event pairs: the timer brackets the launch alone)
            for _ in range(3):                                             # warm-up: code object, first touch
                call()
            ctx.synchronize()
            per_round = []
            for _ in range(a.rounds):
                ctx.profile_reset()
                for _ in range(a.calls):
                    call()
                ms, n_launch = ctx.profile_read(capi.K_EKF_CONTROL)
                assert n_launch == a.calls, (name, n_launch)
                per_round.append(1e3 * ms / a.calls)
            res["us"][name] = {"median": float(np.median(per_round)), "min": float(np.min(per_round)), "max": float(np.max(per_round))}
        ctx.profile_enable(False)
        g.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
