#!/usr/bin/env python3
"""Time of the dense stereo entries (csrc/stereo_bm.hip) at 752 x 480, numDisparities 96, 64 resident pairs of synthetic frames.
Event times through hv_profile_read, per pair:
  match      hv_stereo_disparity_batch_dev with speckleWindowSize 0 and no count: bm_prefilter_kernel + bm_match_kernel (HV_K_INGEST)
  speckles   hv_filter_speckles_batch_dev on the maps that call left: the four labelling kernels (HV_K_INGEST)
  full       hv_stereo_disparity_batch_dev with the defaults and n_valid_dev (prefilter, matching, labelling, count)
  depth, cloud   hv_stereo_track_depth_batch_dev (200 tracks per pair) and hv_stereo_point_cloud_batch_dev, stride 5 (HV_K_STEREO_GATE)
A round's figure is the mean over its calls; reported are the median, minimum and maximum over the rounds, and a host clock
around the full calls. usage: scripts/stereo_bm_bench.py --out profiles/stereo_bm/stereo_bm_bench.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
W, H = 752, 480


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from hybvio_amd import capi, synth
    n = a.pairs
    left, right, _ = synth.stereo_sequence(11, W, H, 4)
    params = capi.stereo_bm_default_params(W)
    raw = capi.stereo_bm_default_params(W, speckleWindowSize=0)
    res = {"pairs": n, "size": [W, H], "numDisparities": params.numDisparities, "rounds": a.rounds, "calls_per_round": a.calls}
    with capi.Context(width=W, height=H, levels=1, pool_size=2 * n) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        sl, sr = [], []
        for i in range(n):
            l, r = ctx.acquire(), ctx.acquire()
            ctx.build(l, left[i % len(left)]); ctx.build(r, right[i % len(right)])
            sl.append(l); sr.append(r)
        d_l = torch.tensor(sl, dtype=torch.int32, device="cuda"); d_r = torch.tensor(sr, dtype=torch.int32, device="cuda")
        work = torch.empty(ctx.stereo_work_bytes(n, params), dtype=torch.uint8, device="cuda")
        disp = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
        scratch = torch.empty_like(disp)
        n_valid = torch.zeros(n, dtype=torch.int32, device="cuda")
        spk_work = torch.empty(capi.filter_speckles_work_bytes(W, H, n), dtype=torch.uint8, device="cuda")
        q = np.array([[1, 0, 0, -W / 2], [0, 1, 0, -H / 2], [0, 0, 0, 458.0], [0, 0, 1 / 0.11, 0]], np.float64)
        rng = np.random.default_rng(1)
        xy = torch.from_numpy(np.stack([rng.uniform(0, W, (n, 200)), rng.uniform(0, H, (n, 200))], -1).astype(np.float32)).cuda()
        n_pts = torch.full((n,), 200, dtype=torch.int32, device="cuda")
        depth = torch.empty((n, 200), dtype=torch.float32, device="cuda")
        bound = ctx.stereo_cloud_bound(5)
        xyz = torch.empty((n, bound, 3), dtype=torch.float32, device="cuda")
        n_cloud = torch.zeros(n, dtype=torch.int32, device="cuda")
        P = lambda t: t.data_ptr()
        calls = {
            "match": (capi.K_INGEST, lambda: ctx.stereo_disparity_batch_dev(n, P(d_l), P(d_r), P(work), P(disp), W * H, 0, raw)),
            "speckles": (capi.K_INGEST, lambda: (scratch.copy_(disp),
                                                 ctx.filter_speckles_batch_dev(n, W, H, P(scratch), W * H, -16, 500, 10, P(spk_work)))),
            "full": (capi.K_INGEST, lambda: ctx.stereo_disparity_batch_dev(n, P(d_l), P(d_r), P(work), P(disp), W * H, P(n_valid), params)),
            "depth": (capi.K_STEREO_GATE, lambda: ctx.stereo_track_depth_batch_dev(n, 200, P(n_pts), P(xy), P(disp), W * H, q, P(depth))),
            "cloud": (capi.K_STEREO_GATE, lambda: ctx.stereo_point_cloud_batch_dev(n, P(disp), W * H, q, 5, bound, P(xyz), P(n_cloud))),
        }
        for name in ("match", "speckles", "full", "depth", "cloud"):           # warm-up, in an order that leaves `disp` unfiltered for "speckles"
            calls[name][1]()
        ctx.synchronize()
        res["unfiltered_pixels_per_pair_mean"] = float(n_valid.cpu().numpy().mean())
        res["cloud_points_per_pair_mean"] = float(n_cloud.cpu().numpy().mean())
        stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
        host = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                calls["full"][1]()
            ctx.synchronize()
            host.append(1e6 * (time.perf_counter() - t0) / a.calls / n)
        ctx.profile_enable(True)
        us = {"full_host_clock": stat(host)}
        for name in ("match", "speckles", "full", "depth", "cloud"):
            if name == "speckles":
                calls["match"][1]()                                            # unfiltered maps to label
            k, fn = calls[name]
            v = []
            for _ in range(a.rounds):
                ctx.synchronize()
                ctx.profile_reset()
                for _ in range(a.calls):
                    fn()
                ms, launches = ctx.profile_read(k)
                assert launches == a.calls, (name, launches)
                v.append(1e3 * ms / a.calls / n)
            us[name] = stat(v)
        ctx.profile_enable(False)
        res["us_per_pair"] = us
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
