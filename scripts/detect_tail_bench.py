#!/usr/bin/env python3
"""Microbenchmark of the device detect() tail (HV_K_DETECT_TAIL events + a host clock around synchronised calls) at 752x480,
150 live tracks per image, mask radius = gfttMinDistance, maxTracks 200, for block edges 32 (gfttMinDistance 50, 345 key points)
and 8 (gfttMinDistance 8, 5 640 key points), 1 and 1024 images:
  (a) detect_tail_kernel per launch, from the HV_K_DETECT_TAIL events (hv_gftt_corners_batch_dev on resident key points)
  (b) wall time of the full hv_gftt_detect_batch_dev call (key points + tail), synchronised
  (c) the library's own one-image path for the same lists, hv_gftt_detect (key points, synchronous copy, std::stable_sort and
      hv_apply_min_distance in C++): wall time per call, median over up to 64 of the images -- the only form there was before the
      device tail; a batch of B images costs B of these calls
  (d) a batched host tail driven from Python: hv_gftt_keypoints_batch_dev, ONE device-to-host copy, and per image numpy's stable
      argsort, the zero prefix and the library's C hv_apply_min_distance through ctypes. At 1024 images this mostly measures the
      interpreter's per-image loop; (c) is the C cost
The device lists are compared with those of (c) and (d) on every run.
usage: scripts/detect_tail_bench.py [--reps N] [--images N] [--out file.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from hybvio_amd import capi, synth  # noqa: E402


def host_tail(kp, prev, r, max_tracks):
    """the tail of hv_gftt_detect for one image"""
    L = capi.lib()
    nk = len(kp)
    order = np.argsort(-kp[:, 2], kind="stable")
    c = np.zeros((2 * nk, 2), np.float32)
    c[nk:] = kp[order, :2]
    n = C.c_int(2 * nk)
    L.hv_apply_min_distance(c.ctypes.data_as(capi.f32p), C.byref(n), prev.ctypes.data_as(capi.f32p), len(prev), int(r), int(max_tracks))
    return c[:n.value]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    w, h, live, max_tracks, distinct = 752, 480, 150, 200, 8
    left, _, _ = synth.stereo_sequence(11, w, h, distinct)
    rng = np.random.default_rng(5)
    import platform
    res = {"params": {"image": [w, h], "live_tracks": live, "maxTracks": max_tracks, "distinct_images": distinct},
           "box": {"host": platform.node(), "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d")}}
    with capi.Context(width=w, height=h, pool_size=distinct) as ctx:
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        slots = [ctx.acquire() for _ in range(distinct)]
        for s, img in zip(slots, left):
            ctx.build(s, img)
        for min_dist in (50, 8):
            gp = capi.gftt_default_params(gfttMinDistance=float(min_dist), maxTracks=max_tracks)
            nk = ctx.gftt_keypoint_count(gp)
            for B in sorted({1, a.images}):
                prev = rng.uniform([0, 0], [w, h], (B, live, 2)).astype(np.float32)
                with torch.cuda.stream(stream):
                    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
                    d_sl = dev(np.array([slots[i % distinct] for i in range(B)], np.int32))
                    d_p, d_np, d_r = dev(prev), dev(np.full(B, live, np.int32)), dev(np.full(B, min_dist, np.int32))
                    d_kp = torch.zeros((B, nk, 3), dtype=torch.float32, device="cuda")
                    d_c = torch.zeros((B, max_tracks, 2), dtype=torch.float32, device="cuda")
                    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
                full = lambda: ctx.gftt_detect_batch_dev(B, d_sl.data_ptr(), d_kp.data_ptr(), live, d_np.data_ptr(), d_p.data_ptr(),
                                                         d_r.data_ptr(), max_tracks, d_c.data_ptr(), d_n.data_ptr(), params=gp)
                tail = lambda: ctx.gftt_corners_batch_dev(B, d_kp.data_ptr(), live, d_np.data_ptr(), d_p.data_ptr(), d_r.data_ptr(),
                                                          max_tracks, d_c.data_ptr(), d_n.data_ptr(), params=gp)
                for _ in range(3):
                    full()
                stream.synchronize()
                ctx.profile_enable(True)
                ctx.profile_reset()
                for _ in range(a.reps):
                    tail()
                ms, n = ctx.profile_read(capi.K_DETECT_TAIL)
                ctx.profile_enable(False)
                wall = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    full()
                    stream.synchronize()
                    wall.append(time.perf_counter() - t0)
                got_c, got_n = d_c.cpu().numpy(), d_n.cpu().numpy()
                host, same = [], True
                for rep in range(max(1, min(a.reps, 3))):
                    t0 = time.perf_counter()
                    ctx.gftt_keypoints_batch_dev(B, d_sl.data_ptr(), d_kp.data_ptr(), gp)
                    with torch.cuda.stream(stream):
                        kp = d_kp.cpu().numpy()
                    lists = [host_tail(kp[s], prev[s], min_dist, max_tracks) for s in range(B)]
                    host.append(time.perf_counter() - t0)
                    same = same and all(got_n[s] == len(lists[s]) and np.array_equal(got_c[s, :got_n[s]], lists[s]) for s in range(B))
                one = []
                for s in range(min(B, 64)):
                    t0 = time.perf_counter()
                    c1 = ctx.gftt_detect(slots[s % distinct], prev=prev[s], mask_radius=min_dist, params=gp)
                    one.append(time.perf_counter() - t0)
                    same = same and got_n[s] == len(c1) and np.array_equal(got_c[s, :got_n[s]], c1)
                res[f"bs{32 if min_dist >= 32 else 8}_{B}x{nk}"] = {
                    "images": B, "key_points": nk, "tail_kernel_us_mean": 1e3 * ms / n, "tail_launches": n,
                    "detect_batch_dev_wall_us_median": 1e6 * float(np.median(wall)),
                    "hv_gftt_detect_wall_us_per_image_median": 1e6 * float(np.median(one)),
                    "keypoints_d2h_host_tail_wall_us_median": 1e6 * float(np.median(host)),
                    "corners_mean": float(got_n.mean()), "device_equals_host": bool(same)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
