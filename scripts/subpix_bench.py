#!/usr/bin/env python3
"""Microbenchmark of the sub-pixel corner refinement (hv_corner_subpix*, HV_K_SUBPIX events + a host clock around synchronised
calls), default parameters (window 10, 20 iterations, epsilon 0.03):
  (a) latency: one 752x480 image, its GFTT corners (mask radius 20, at most 200 incl. the (0, 0) prefix), hv_corner_subpix
  (b) throughput: 1024 images x 200 corners, one hv_corner_subpix_batch_dev launch
  (c) the histogram of position updates per corner on synth stereo frames (left and right images)
usage: scripts/subpix_bench.py [--reps N] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from hybvio_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    w, h = 752, 480
    left, right, _ = synth.stereo_sequence(7, w, h, 8)
    res = {"params": {"subPixWindowSize": 10, "subPixMaxIter": 20, "subPixEpsilon": 0.03}}
    with capi.Context(width=w, height=h, pool_size=16) as ctx:
        s = ctx.acquire()
        ctx.build(s, left[0])
        corners = ctx.gftt_detect(s, mask_radius=20)
        for _ in range(20):
            ctx.corner_subpix(s, corners)
        ctx.profile_enable(True)
        ctx.profile_reset()
        host = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.corner_subpix(s, corners)                     # H2D points, kernel, D2H points + counts, stream synchronise
            host.append(time.perf_counter() - t0)
        ms, n = ctx.profile_read(capi.K_SUBPIX)
        _, it = ctx.corner_subpix(s, corners)
        res["a_latency"] = {"corners": int(len(corners)), "kernel_us_mean": 1e3 * ms / n, "host_call_us_median": 1e6 * float(np.median(host)),
                            "host_call_us_p10": 1e6 * float(np.percentile(host, 10)), "host_call_us_p90": 1e6 * float(np.percentile(host, 90)),
                            "max_updates": int(it.max()), "mean_updates": float(it.mean()), "launches": n}
        ctx.profile_enable(False)

        # (b) 1024 images x 200 corners: 16 distinct frames in 16 slots, every set refines the corners of its frame
        frames = [left[k] for k in range(8)] + [right[k] for k in range(8)]
        ctx.release(s)
        slots = [ctx.acquire() for _ in frames]
        lists = []
        for sl, f in zip(slots, frames):
            ctx.build(sl, f)
            c = ctx.gftt_detect(sl, mask_radius=20)
            lists.append(np.pad(c, ((0, 200 - len(c)), (0, 0))) if len(c) < 200 else c[:200])
        B, M = 1024, 200
        set_slot = np.array([slots[i % len(slots)] for i in range(B)], np.int32)
        xy = np.stack([lists[i % len(slots)] for i in range(B)]).astype(np.float32)
        counts = np.full(B, M, np.int32)
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        d_slots, d_n = torch.from_numpy(set_slot).cuda(), torch.from_numpy(counts).cuda()
        d_in = torch.from_numpy(xy).cuda()
        d_xy = d_in.clone()
        d_it = torch.zeros((B, M), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(3):
            d_xy.copy_(d_in)
            ctx.corner_subpix_batch_dev(B, d_slots.data_ptr(), M, d_n.data_ptr(), d_xy.data_ptr(), d_it.data_ptr())
        stream.synchronize()
        ctx.profile_enable(True)
        ctx.profile_reset()
        reps_b = max(5, a.reps // 20)
        host = []
        for _ in range(reps_b):
            with torch.cuda.stream(stream):
                d_xy.copy_(d_in)
            stream.synchronize()
            t0 = time.perf_counter()
            ctx.corner_subpix_batch_dev(B, d_slots.data_ptr(), M, d_n.data_ptr(), d_xy.data_ptr(), d_it.data_ptr())
            stream.synchronize()
            host.append(time.perf_counter() - t0)
        ms, n = ctx.profile_read(capi.K_SUBPIX)
        itb = d_it.cpu().numpy()
        res["b_throughput"] = {"sets": B, "corners_per_set": M, "kernel_ms_mean": ms / n, "host_ms_median": 1e3 * float(np.median(host)),
                               "corners_per_s": B * M / (ms / n * 1e-3), "mean_updates": float(itb.mean()), "launches": n}
        ctx.profile_enable(False)

        # (c) position updates per corner, default parameters, every left and right frame of the sequence
        hist = np.zeros(21, np.int64)
        for sl in slots:
            c = ctx.gftt_detect(sl, mask_radius=20)
            _, it = ctx.corner_subpix(sl, c)
            hist += np.bincount(it, minlength=21)[:21]
        res["c_update_histogram"] = {"frames": len(slots), "corners": int(hist.sum()), "counts_by_updates_0_to_20": hist.tolist()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
