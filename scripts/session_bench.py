#!/usr/bin/env python3
"""Launch times of the session lifecycle entries (hv_session_*_dev, csrc/session.hip; HV_K_EKF_CONTROL events) at the shape a lane
runs: 1024 resident sequences, cameraTrailLength 20 (n = 160), maxTracks 200, stereo, the default ring of 60 flags.
  init      hv_session_init_dev
  imu       hv_session_imu_dev, 7 samples (200 Hz IMU, 30 Hz frames): every filter past its first sample / every filter on its first
            sample (initializeOrientation written)
  status    hv_session_status_dev, rings half full
  reset     hv_session_reset_dev with no set, with 16 sets (8 of each kind, spread over the batch; the same 16 all fresh and all
            keep-pose) and with all 1024 resetting
Per figure: `rounds` rounds of `calls` launches; a round's figure is the mean event time of its launches; reported are the median,
minimum and maximum over the rounds. The entries are a few scalar rules per set, so the figures are launch floors except for the
reset, which writes 8 n^2 bytes of covariance and the table and index slices of each set that resets.
usage: scripts/session_bench.py [--rounds N] [--calls N] [--out file.json]
       rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python scripts/session_bench.py --rounds 3 --calls 20, then
       scripts/session_bench.py --rounds 3 --calls 20 --trace-summary DIR/.../t_kernel_trace.csv: the kernels' traced durations"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from hybvio_amd import capi  # noqa: E402

B, TRAIL, M, NS = 1024, 20, 200, 7
# kernel -> (launches in front of the timed ones: set-up and warm-up, the figures it serves in launch order); W = the ring size
TRACE_PLAN = {"session_init_kernel": (lambda W: 1 + 3, ["init"]),
              "session_imu_kernel": (lambda W: 3 + 3, ["imu_7_samples", "imu_7_samples_first_sample"]),
              "session_status_kernel": (lambda W: W // 2 + 3, ["status"]),
              "session_reset_kernel": (lambda W: 5 * 3, ["reset_0_of_1024", "reset_16_of_1024", "reset_1024_of_1024", "reset_16_fresh_of_1024",
                                                         "reset_16_keep_pose_of_1024"])}


def trace_summary(path, rounds, calls, W=60):
    """Kernel durations of a `rocprofv3 --kernel-trace --output-format csv` run of this script with the same --rounds and --calls,
    attributed to the figures by launch order."""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    out, n = {}, rounds * calls
    for kernel, (skip, names) in TRACE_PLAN.items():
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        assert len(d) == skip(W) + n * len(names), (kernel, len(d))
        for i, name in enumerate(names):
            chunk = d[skip(W) + i * n: skip(W) + (i + 1) * n]
            out[name] = {"median": float(np.median(chunk)), "min": float(np.min(chunk)), "max": float(np.max(chunk))}
    return {"source": "kernel trace", "launches_per_figure": n, "us": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-summary", metavar="CSV", default=None, help="summarise the kernel_trace.csv of a traced run instead of measuring")
    a = ap.parse_args()
    if a.trace_summary:
        line = json.dumps(trace_summary(a.trace_summary, a.rounds, a.calls))
        print(line)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return
    import torch
    rng = np.random.default_rng(1)
    res = {"sets": B, "n": 20 + 7 * TRAIL, "maxTracks": M, "imu_samples": NS, "rounds": a.rounds, "calls_per_round": a.calls, "us": {}}
    with capi.Context(width=752, height=480, levels=1, pool_size=1) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        g = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=TRAIL), B)
        sp = capi.session_default_params()
        W = capi.session_window(sp)
        res["window"] = W
        ses, ctl = capi.session_state(B, W), capi.EkfControl(B)
        tp, ip = capi.track_table_default_params(maxTracks=M), capi.trail_index_default_params(cameraTrailLength=TRAIL, maxTracks=M)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        tm = dict(n_tracks=z(B, torch.int32), ids=z((B, M), torch.int32), xy=z((B, M, 2), torch.float32), second_xy=z((B, M, 2), torch.float32),
                  status=z((B, M), torch.int32), blacklist=z((B, M), torch.uint8), kf_xy=z((B, M, 2), torch.float32),
                  kf_valid=z((B, M), torch.uint8), frame_num=z(B, torch.int32), mask_steps=z(B, torch.int32), mask_radius=z(B, torch.int32),
                  frame_flags=z(B, torch.uint8))
        table, trail = capi.track_table(**{k: v.data_ptr() for k, v in tm.items()}), capi.TrailIndex(B, ip)
        ctx.tracks_init_batch_dev(B, table, params=tp); ctx.trail_init_batch_dev(B, trail.table, params=ip)
        g.control_init_dev(ctl); g.session_init_dev(sp, ses)
        t = torch.from_numpy(100.0 + 0.005 * np.arange(NS)[:, None] + np.zeros((NS, B))).cuda()
        acc = torch.from_numpy(np.array([0.2, -0.1, 9.8]) + rng.normal(0, 0.05, (NS, B, 3))).cuda()
        dt_out, time_out = z((NS, B), torch.float64), z((NS, B), torch.float64)
        good = torch.from_numpy(rng.integers(0, 2, B).astype(np.uint8)).cuda()
        status, frozen, kind_out = z(B, torch.int32), z(B, torch.uint8), z(B, torch.int32)
        kinds = {"reset_0_of_1024": np.zeros(B, np.int32), "reset_16_of_1024": np.zeros(B, np.int32), "reset_1024_of_1024": 1 + (np.arange(B, dtype=np.int32) % 2)}
        which = rng.choice(B, 16, replace=False)
        kinds["reset_16_of_1024"][which] = np.tile(np.array([1, 2], np.int32), 8)
        for name, k in (("reset_16_fresh_of_1024", 1), ("reset_16_keep_pose_of_1024", 2)):
            kinds[name] = np.zeros(B, np.int32)
            kinds[name][which] = k
        kinds = {k: torch.from_numpy(v).cuda() for k, v in kinds.items()}

        def imu():
            g.session_imu_dev(ses, NS, t.data_ptr(), acc.data_ptr(), dt_out.data_ptr(), time_out.data_ptr())

        def first_imu():
            ses.m["initialized_orientation"].zero_()           # (outside the event pair: the timer brackets the launch alone)
            imu()

        def reset(k):
            return lambda: g.session_reset_dev(sp, ses, ctl, tp, table, ip, trail.table, kinds[k].data_ptr())

        entries = {"init": lambda: g.session_init_dev(sp, ses), "imu_7_samples": imu, "imu_7_samples_first_sample": first_imu,
                   "status": lambda: g.session_status_dev(sp, ses, good.data_ptr(), kind_out.data_ptr(), status_dev=status.data_ptr(),
                                                          frozen_dev=frozen.data_ptr())}
        entries.update({k: reset(k) for k in kinds})
        for _ in range(W // 2):                                # rings half full: the mean is consulted from here on
            entries["status"]()
        for fn in entries.values():                            # warm-up: code objects, first touch
            for _ in range(3):
                fn()
        ctx.synchronize()
        ctx.profile_enable(True)
        for name, fn in entries.items():
            per_round = []
            for _ in range(a.rounds):
                ctx.profile_reset()
                for _ in range(a.calls):
                    fn()
                ms, n = ctx.profile_read(capi.K_EKF_CONTROL)
                assert n == a.calls, (name, n)
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
