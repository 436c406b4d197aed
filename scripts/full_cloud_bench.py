#!/usr/bin/env python3
"""Launch time of the full point cloud entry (hv_full_point_cloud_dev, csrc/full_cloud.hip) at the shape a lane runs: 1024 resident
sequences, maxTracks 200, stereo, cameraTrailLength 20 (n = 160), track lengths as in the bench's realistic frame (5 + Geometric(0.2),
at most 21), observations that are projections of world points along a moving trail, so the Gauss-Newton loops converge as they do
in a sequence. The visit loop of every set stopped at its fifth success; the tail is what lies behind it in the shuffled order.

In the same run, alternating with it, what a caller of the previous commit has to launch for the same cloud: the tail of every set
gathered into visit-shaped records and run through hv_ekf_visual_prepare_dev, one launch of 1024 filters per tail element. The
emulation is given every advantage: its gather and its read-back of the index are not counted, every element runs at the MEAN track
length (hv_ekf_visual_prepare_dev takes one length per launch), and only as many elements are launched as the largest tail holds.

Per round: `calls` entry launches between one pair of device events, then one emulation pass between another; the two kernels of
the entry are reported separately from the library's own event pairs (HV_K_TRAIL_INDEX, HV_K_VU_TRI) in a pass of their own.
usage: scripts/full_cloud_bench.py [--rounds N] [--calls N] [--sets N] [--out file.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from hybvio_amd import capi  # noqa: E402

TRAIL, M, V, SUCC = 20, 200, 20, 5
RIC = np.array([[0.0, -1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])
BASE2 = np.array([0.11, 0.002, -0.001])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--sets", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    B, K, n = a.sets, TRAIL + 1, 20 + 7 * TRAIL
    rng = np.random.default_rng(3)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    T1 = np.eye(4); T1[:3, :3] = RIC
    T2 = T1.copy(); T2[:3, 3] = BASE2
    # ---- the world: per set a straight trail (keyframe 0 the newest), identity orientation, 200 points in front ----
    step = rng.normal(size=(B, 1, 3)) * 0.05 + np.array([0.12, 0.0, 0.0])
    pos = rng.uniform(-2, 2, (B, 1, 3)) - np.arange(K).reshape(1, K, 1) * step                  # [B][K][3]
    means = np.zeros((B, n)); means[:, 16:19] = 1.0
    means[:, 0:3], means[:, 6] = pos[:, 0], 1.0
    for k in range(TRAIL):
        means[:, 20 + 7 * k:20 + 7 * k + 3], means[:, 20 + 7 * k + 3] = pos[:, k + 1], 1.0
    cam_pts = np.stack([rng.uniform(-0.45, 0.45, (B, M)), rng.uniform(-0.3, 0.3, (B, M)), np.ones((B, M))], axis=2) * rng.uniform(3, 10, (B, M, 1))
    pw = pos[:, :1] + cam_pts @ RIC                                                                # R' x = x R for R = RIC
    norm = np.zeros((B, K, M, 2, 2))
    for cam in range(2):
        pcam = pos - (BASE2 @ RIC if cam else 0.0)                                                 # p - R' baseline
        pc = (pw[:, None] - pcam[:, :, None]) @ RIC.T                                              # [B][K][M][3]
        norm[:, :, :, cam] = pc[..., :2] / pc[..., 2:] + rng.normal(size=(B, K, M, 2)) * 7e-4
    length = np.minimum(5 + rng.geometric(0.2, (B, M)) - 1, K).astype(np.int32)
    with capi.Context(width=752, height=480, levels=1, pool_size=1) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        g = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=TRAIL), B)
        for b in range(B):
            g.set_state(b, means[b], np.eye(n) * 1e-4 if b == 0 else None)
        tp = capi.trail_index_default_params(cameraTrailLength=TRAIL, maxTracks=M, maxVisualUpdates=V, maxSuccessfulVisualUpdates=SUCC)
        vp = capi.vu_default_params(imu_to_camera=T1, second_imu_to_camera=T2)
        trail = capi.TrailIndex(B, tp)
        ctx.trail_init_batch_dev(B, trail.table, params=tp)
        torch.cuda.synchronize()
        trail.m["n_keyframes"].fill_(K)
        trail.m["col_id"].copy_(dev(np.tile(np.arange(1, M + 1, dtype=np.int32), (B, 1))))
        trail.m["col_len"].copy_(dev(length))
        trail.m["norm_point"].copy_(dev(norm))
        trail.m["image_point"].copy_(dev((norm * 458.0 + 300.0).astype(np.float32)))
        trail.m["cand_pos"].copy_(dev(np.tile(np.arange(V, dtype=np.int32), (B, 1))))           # the stop: position 4 of the order
        trail.m["cand_col"].copy_(dev(rng.integers(0, M, (B, V)).astype(np.int32)))
        table = dict(n_tracks=dev(np.full(B, M, np.int32)), ids=dev(np.tile(np.arange(1, M + 1, dtype=np.int32), (B, 1))))
        tt = capi.track_table(**{k: v.data_ptr() for k, v in table.items()})
        status = np.full((V, B, 2), -1, np.int32); status[:SUCC] = 0                             # five visits, five successes: stopped
        gate = np.ones((V, B), np.int32); gate[:SUCC] = 0
        arrays = dict(draws_dev=dev(rng.integers(0, 2 ** 31, (B, M)).astype(np.int32)), cand_id_dev=dev(rng.integers(1, M + 1, (V, B)).astype(np.int32)),
                      n_candidates_dev=dev(np.full(B, V, np.int32)), status_dev=dev(status), gate_status_dev=dev(gate),
                      pf_dev=dev(rng.uniform(-8, 8, (V, B, 3))))
        frame = capi.full_cloud_frame(**{k: v.data_ptr() for k, v in arrays.items()})
        out = capi.FullCloud(B, tp)
        entry = lambda: g.full_point_cloud_dev(tp, vp, trail.table, tt, frame, out)
        entry()
        torch.cuda.synchronize()
        n_tail, n_points = out.m["n_tail"].cpu().numpy(), out.m["n_points"].cpu().numpy()
        st = out.m["tail_status"].cpu().numpy()
        ok = sum(int((st[b, :n_tail[b]] == 0).sum()) for b in range(B))
        # ---- the emulation: max(n_tail) launches of hv_ekf_visual_prepare_dev over the B filters at the mean track length ----
        n_elem, np_mean = int(n_tail.max()), int(round(float(length.mean())))
        idx = dev(np.tile(np.arange(np_mean, dtype=np.int32), (B, 1)))
        feat = dev(np.ascontiguousarray(norm[:, :np_mean, 0].transpose(0, 2, 1, 3).reshape(B, 2 * np_mean, 2)))
        vel = torch.zeros_like(feat)
        z = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device="cuda")
        H, v_, f_, pf_, st_ = z(B, 4 * np_mean * n), z(B, 4 * np_mean), z(B, 4 * np_mean), z(B, 3), z(B, 2, dt=torch.int32)
        P_ = lambda x: x.data_ptr()

        def emulation():
            for _ in range(n_elem):
                g.visual_prepare_dev(vp, np_mean, P_(idx), P_(feat), P_(vel), 0, P_(H), P_(v_), P_(f_), P_(pf_), P_(st_))

        def timed(fn, reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps

        for _ in range(3):
            entry()
        emulation()
        torch.cuda.synchronize()
        rounds = []
        for _ in range(a.rounds):
            rounds.append(dict(entry_ms=timed(entry, a.calls), emulation_ms=timed(emulation, 1)))
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(a.calls):
            entry()
        (ms_i, n_i), (ms_t, n_t) = ctx.profile_read(capi.K_TRAIL_INDEX), ctx.profile_read(capi.K_VU_TRI)
        assert n_i == a.calls and n_t == a.calls
        ctx.profile_enable(False)
        g.close()
    e, m = [r["entry_ms"] for r in rounds], [r["emulation_ms"] for r in rounds]
    res = dict(sets=B, maxTracks=M, cameraTrailLength=TRAIL, stereo=1, mean_track_length=float(length.mean()),
               tail_tracks=int(n_tail.sum()), tail_per_set=float(n_tail.mean()), tail_max=int(n_tail.max()), tail_ok=ok,
               points=int(n_points.sum()), calls_per_round=a.calls, emulation_launches=n_elem, emulation_n_poses=np_mean, rounds=rounds,
               entry_ms=dict(median=float(np.median(e)), min=float(min(e)), max=float(max(e))),
               emulation_ms=dict(median=float(np.median(m)), min=float(min(m)), max=float(max(m))),
               index_kernel_ms=ms_i / a.calls, tri_kernel_ms=ms_t / a.calls,
               entry_faster_on_every_alternation=bool(all(r["entry_ms"] < r["emulation_ms"] for r in rounds)))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
