#!/usr/bin/env python3
"""Microbenchmark of the device std::mt19937 entries (hv_rng_*_batch_dev, HV_K_TRAIL_INDEX events) at 1024 and 4096 sets, with
hv_rot_ransac_lk_batch_dev (HV_K_ROT_RANSAC events) on the device's own draws beside them in the same process for scale:
  seed                per-set seeds
  draw 200 / 1500     the RANSAC2 and the RANSAC3 offer
  advance 200         every set by 2 x 100 hypotheses (a twist in one launch out of three)
  advance mixed       per-set counts drawn from 0 .. 100 hypotheses
  advance 1500        every set by 3 x 500 iterations (two or three twists)
  rot_ransac          200 features, 40 outliers: all 100 hypotheses
Per entry: the event time per launch (it contains the event pair's own floor, which this script does not separate) and the host's
wall time per launch around the same loop, ending in a synchronise. The whole list is measured --rounds times: the spread.
usage: scripts/rng_bench.py [--reps N] [--rounds N] [--out file.json]"""
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
from test_gpu_rot_ransac import THR, _cams, _scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": []}

    def timed(ctx, kid, fn, warm, reps):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ctx.profile_reset()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / reps * 1e6
        ms, n = ctx.profile_read(kid)
        assert n == reps, (n, reps)
        return {"event_us_per_launch": round(ms / n * 1e3, 3), "wall_us_per_launch": round(wall, 3), "launches": n}

    with capi.Context(width=64, height=64) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.profile_enable(True)
        ocam, gcam = _cams(orc, "pinhole")
        rng = np.random.default_rng(1)
        M = n = 200
        scenes = [_scene(ocam, rng, n, 40) for _ in range(8)]
        P = lambda x: x.data_ptr()
        for rnd in range(a.rounds):
            for S in (1024, 4096):
                st = capi.rng_state(S)
                seeds = torch.arange(4649, 4649 + S, dtype=torch.int32, device="cuda")
                ctx.rng_seed_batch_dev(S, st.table, seed_dev=P(seeds))
                d200 = torch.zeros((S, 200), dtype=torch.int32, device="cuda")
                d1500 = torch.zeros((S, 1500), dtype=torch.int32, device="cuda")
                c200 = torch.full((S, 2), 100, dtype=torch.int32, device="cuda")
                c1500 = torch.full((S, 4), 500, dtype=torch.int32, device="cuda")
                c_mixed = torch.from_numpy(np.random.default_rng(2).integers(0, 101, (S, 2)).astype(np.int32)).cuda()
                K = capi.K_TRAIL_INDEX
                row = {"round": rnd, "n_sets": S}
                row["seed"] = timed(ctx, K, lambda: ctx.rng_seed_batch_dev(S, st.table, seed_dev=P(seeds)), 20, a.reps)
                row["draw_200"] = timed(ctx, K, lambda: ctx.rng_draw_batch_dev(S, st.table, 200, P(d200)), 20, a.reps)
                row["draw_1500"] = timed(ctx, K, lambda: ctx.rng_draw_batch_dev(S, st.table, 1500, P(d1500)), 20, a.reps)
                row["advance_200"] = timed(ctx, K, lambda: ctx.rng_advance_batch_dev(S, st.table, P(c200) + 4, 2, 2, 200), 20, a.reps)
                row["advance_mixed_0_200"] = timed(ctx, K, lambda: ctx.rng_advance_batch_dev(S, st.table, P(c_mixed) + 4, 2, 2, 200), 20, a.reps)
                row["advance_1500"] = timed(ctx, K, lambda: ctx.rng_advance_batch_dev(S, st.table, P(c1500) + 8, 4, 3, 1500), 20, a.reps)
                rep = np.arange(S) % len(scenes)
                c1 = torch.from_numpy(np.stack([scenes[i][0] for i in rep])).cuda()
                c2 = torch.from_numpy(np.stack([scenes[i][1] for i in rep])).cuda()
                cnt = torch.full((S,), n, dtype=torch.int32, device="cuda")
                lk = torch.ones((S, M), dtype=torch.uint8, device="cuda")
                stt = torch.zeros((S, M), dtype=torch.int32, device="cuda")
                Rm = torch.zeros((S, 9), dtype=torch.float32, device="cuda")
                summ = torch.zeros((S, 2), dtype=torch.int32, device="cuda")
                ctx.rng_draw_batch_dev(S, st.table, 200, P(d200))
                row["rot_ransac"] = timed(ctx, capi.K_ROT_RANSAC,
                                          lambda: ctx.rot_ransac_lk_batch_dev(S, M, P(cnt), P(c1), P(c2), P(lk), 1, gcam, gcam, P(d200), THR,
                                                                              P(stt), P(Rm), P(summ)), 5, max(a.reps // 5, 1))
                row["rot_ransac_hypotheses_mean"] = float(summ[:, 1].float().mean().item())
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
