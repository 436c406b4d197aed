#!/usr/bin/env python3
"""Microbenchmark of the device ZUPT (hv_ekf_block_update_dev at VEL, 3 rows: ekf_block_update_kernel, HV_K_EKF_CONTROL events)
against the same ZUPT through hv_ekf_update (a host-built 3 x 6 H, four host-to-device copies, the general ekf_update_kernel:
HV_K_EKF_UPDATE events), n = 160 (cameraTrailLength 20):
  batch 1 and batch 1024; all filters active, and at batch 1024 one in eight: a seeded random eighth (an unpredictable subset, the
  case the launch is built for) and every eighth filter (workgroup b runs on XCD b % 8, so this mask puts all its work on one XCD:
  the worst subset there is for one workgroup per filter in filter order).
The two paths alternate inside one process: `rounds` rounds, each `calls` calls of one path and then of the other. Per path and
round: the mean event time of the round's launches (the kernel alone) and the median of a host clock around call + synchronise
(what a caller waits for: hv_ekf_update's copies are in it). Reported: median, min and max over the rounds, and the algorithm's
bytes (2 * 8 n^2 + 8 k n per active filter) over the kernel time -- not an HBM share: 1024 covariances are 210 MB and can sit
in the 256 MiB Infinity Cache. Before the timing both paths run once on equal states and their results are compared.
usage: scripts/ekf_control_bench.py [--rounds N] [--calls N] [--out file.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from hybvio_amd import capi  # noqa: E402

VEL, ROWS, TRAIL = 3, 3, 20
R_ZUPT = 1e-7


def spd_state(rng, n):
    m = rng.normal(size=n)
    m[6:10] /= np.linalg.norm(m[6:10])
    A = rng.normal(size=(n, n))
    return m, 1e2 * (A @ A.T / n + 0.1 * np.eye(n))


def fill(g, m, P):
    for b in range(g.batch):
        g.set_state(b, m, P)


class Paths:
    """The two ways to apply one ZUPT to the filters `active` marks (None: all), arguments packed once."""

    def __init__(self, ctx, g, active):
        import torch
        self.ctx, self.g, self.L = ctx, g, capi.lib()
        B, l = g.batch, VEL + ROWS
        H = np.zeros((ROWS, l))
        H[np.arange(ROWS), VEL + np.arange(ROWS)] = 1.0
        self.H = np.ascontiguousarray(np.broadcast_to(H.T, (B, l, ROWS)))           # column-major per filter
        self.y, self.rd = np.zeros((B, ROWS)), np.full(B, R_ZUPT)
        self.act = np.ascontiguousarray(active, np.uint8) if active is not None else None
        self.act_dev = torch.from_numpy(self.act).cuda() if active is not None else None
        torch.cuda.synchronize()
        self.p = lambda a, t: a.ctypes.data_as(t) if a is not None else None

    def old(self):
        rc = self.L.hv_ekf_update(self.g._h, ROWS, VEL + ROWS, self.p(self.H, capi.f64p), self.p(self.y, capi.f64p),
                                  self.p(self.rd, capi.f64p), self.p(self.act, capi.u8p), 0)
        assert rc == 0, rc

    def new(self):
        rc = self.L.hv_ekf_block_update_dev(self.g._h, VEL, ROWS, None, None, R_ZUPT,
                                            C.c_void_p(self.act_dev.data_ptr()) if self.act_dev is not None else None, 0, None)
        assert rc == 0, rc


def measure(ctx, paths, rounds, calls):
    out = {"old": {"kernel_us": [], "host_us": []}, "new": {"kernel_us": [], "host_us": []}}
    for name, fn in (("old", paths.old), ("new", paths.new)):                      # warm-up: code objects, first-touch
        for _ in range(3):
            fn()
        ctx.synchronize()
    ctx.profile_enable(True)
    for _ in range(rounds):
        for name, fn, kid in (("old", paths.old, capi.K_EKF_UPDATE), ("new", paths.new, capi.K_EKF_CONTROL)):
            ctx.profile_reset()
            host = []
            for _ in range(calls):
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                host.append(time.perf_counter() - t0)
            ms, n = ctx.profile_read(kid)
            out[name]["launches_per_call"] = n / calls
            out[name]["kernel_us"].append(1e3 * ms / calls)
            out[name]["host_us"].append(1e6 * float(np.median(host)))
    ctx.profile_enable(False)
    return out


def summary(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(3)
    params = capi.ekf_default_params(cameraTrailLength=TRAIL)
    res = {"n": 20 + 7 * TRAIL, "rows": ROWS, "rounds": a.rounds, "calls_per_round": a.calls, "cases": []}
    with capi.Context(width=64, height=64, levels=1, pool_size=1) as ctx:
        # the two paths on equal states, one filter in two masked out
        g1, g2 = capi.EkfBatch(ctx, params, 8), capi.EkfBatch(ctx, params, 8)
        m, P = spd_state(rng, g1.n)
        fill(g1, m, P); fill(g2, m, P)
        mask = np.arange(8) % 2 == 0
        Paths(ctx, g1, mask).old(); Paths(ctx, g2, mask).new()
        ctx.synchronize()
        worst = 0.0
        for b in range(8):
            (m1, P1), (m2, P2) = g1.get_state(b), g2.get_state(b)
            assert mask[b] or (np.array_equal(P1, P) and np.array_equal(P2, P))
            worst = max(worst, float(np.linalg.norm(m1 - m2) / np.linalg.norm(m1)), float(np.linalg.norm(P1 - P2) / np.linalg.norm(P1)))
        assert worst <= 1e-9, worst
        res["old_vs_new_max_rel_diff"] = worst
        g1.close(); g2.close()
        for batch, subset in ((1, "all"), (1024, "all"), (1024, "random eighth"), (1024, "every eighth")):
            g = capi.EkfBatch(ctx, params, batch)
            n = g.n
            fill(g, m, P)
            active = None
            if subset == "random eighth":
                active = np.zeros(batch, bool)
                active[np.random.default_rng(8).choice(batch, batch // 8, replace=False)] = True
            elif subset == "every eighth":
                active = np.arange(batch) % 8 == 0
            n_active = int(active.sum()) if active is not None else batch
            t = measure(ctx, Paths(ctx, g, active), a.rounds, a.calls)
            algo_bytes = n_active * (2 * 8 * n * n + 8 * ROWS * n)
            case = {"batch": batch, "subset": subset, "active": n_active, "algorithm_bytes": algo_bytes}
            for name in ("old", "new"):
                k, h = summary(t[name]["kernel_us"]), summary(t[name]["host_us"])
                case[name] = {"kernel_us": k, "host_call_and_sync_us": h, "timed_launches_per_call": t[name]["launches_per_call"],
                              "algorithm_bytes_over_kernel_time_GBps": algo_bytes / (k["median"] * 1e-6) / 1e9}
            res["cases"].append(case)
            g.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
