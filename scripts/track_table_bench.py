#!/usr/bin/env python3
"""Microbenchmark of the device track table: HV_K_TRACK_TABLE event milliseconds per launch of hv_tracks_update_batch_dev and
hv_tracks_append_batch_dev on FULL tables (n_tracks == maxTracks on entry to every update, so the culling runs), for
1024 sets x 200 tracks and 1024 sets x 1024 tracks, stereo. Every repetition starts from the same uploaded table; each
update culls maxTracks / 20 + 1 tracks and drops the 2 % the synthetic statuses fail; the append then adds tracks only in the
sets where at least maxTracks / 10 are missing (few of them here; its kernel does the same work either way).
A set not at capacity (one track fewer) is timed beside it to show what the culling costs.
usage: scripts/track_table_bench.py [--reps N] [--sets N] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from hybvio_amd import capi  # noqa: E402

W, H = 752, 480


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import platform

    import torch
    S = a.sets
    res = {"params": {"image": [W, H], "sets": S, "stereo": True},
           "box": {"host": platform.node(), "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d")}}
    rng = np.random.default_rng(3)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    with capi.Context(width=W, height=H) as ctx:
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        for M in (200, 1024):
            tp = capi.track_table_default_params(maxTracks=M)
            for n in (M, M - 1):
                with torch.cuda.stream(stream):
                    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
                    xy = rng.uniform([0, 0], [W, H], (S, M, 2)).astype(np.float32)
                    m = dict(n_tracks=dev(np.full(S, n, np.int32)), ids=dev(np.tile(np.arange(1, M + 1, dtype=np.int32), (S, 1))),
                             xy=dev(xy), second_xy=dev(xy - np.float32(20)), status=z((S, M), torch.int32), blacklist=z((S, M), torch.uint8),
                             kf_xy=dev(xy), kf_valid=dev(np.ones((S, M), np.uint8)), frame_num=dev(np.full(S, 30, np.int32)),
                             mask_steps=z(S, torch.int32), mask_radius=dev(np.full(S, 32, np.int32)), frame_flags=z(S, torch.uint8))
                    start = {k: v.clone() for k, v in m.items()}
                    table = capi.track_table(**{k: v.data_ptr() for k, v in m.items()})
                    cur = dev(xy + rng.uniform(-2, 2, xy.shape).astype(np.float32))
                    right = cur - 20
                    ts0 = dev(np.where(rng.random((S, M)) < 0.02, 2, 0).astype(np.int32))
                    ts = ts0.clone()
                    score = dev(np.full(S, 0.5))
                    kf, n_mask, n_added = z(S, torch.int32), z(S, torch.int32), z(S, torch.int32)
                    mask_xy, src, mm = z((S, M, 2), torch.float32), z((S, M), torch.int32), z(S, torch.float64)
                    n_new = dev(np.full(S, M, np.int32))
                    new = dev(rng.uniform([0, 0], [W, H], (S, M, 2)).astype(np.float32))
                    new2 = new - 20
                P = lambda x: x.data_ptr()
                update = lambda: ctx.tracks_update_batch_dev(S, table, P(cur), P(right), P(ts), P(score), P(kf), P(mask_xy), P(n_mask),
                                                             P(src), P(mm), params=tp)
                append = lambda: ctx.tracks_append_batch_dev(S, table, M, P(n_new), P(new), P(new2), P(n_added), params=tp)

                def restore():
                    with torch.cuda.stream(stream):
                        for k, v in m.items():
                            v.copy_(start[k])
                        ts.copy_(ts0)
                times = {"update": [], "append": []}
                kept = added = 0
                for rep in range(a.reps + 2):                       # two warm-up repetitions
                    for name, call in (("update", update), ("append", append)):
                        if name == "update":
                            restore()
                        stream.synchronize()
                        ctx.profile_enable(True)
                        ctx.profile_reset()
                        call()
                        ms, launches = ctx.profile_read(capi.K_TRACK_TABLE)
                        ctx.profile_enable(False)
                        assert launches == 1
                        if rep >= 2:
                            times[name].append(ms)
                        if name == "update":
                            kept = float(m["n_tracks"].float().mean().item())
                        else:
                            added = float(n_added.float().mean().item())
                res[f"{S}x{M}_{'full' if n == M else 'one_below_capacity'}"] = {
                    "sets": S, "maxTracks": M, "tracks_on_entry": n,
                    "update_us_median": 1e3 * float(np.median(times["update"])), "update_us_min": 1e3 * float(np.min(times["update"])),
                    "append_us_median": 1e3 * float(np.median(times["append"])), "append_us_min": 1e3 * float(np.min(times["append"])),
                    "tracks_after_update_mean": kept, "appended_mean": added, "reps": a.reps}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
