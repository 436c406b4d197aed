#!/usr/bin/env python3
"""How often the early exit of the chi2 gates (ekf_device.hpp gate_factor_chi2, `exit_above`) fires on the benchmark's realistic frame,
and how much of the Cholesky it saves. CPU only: the visit loop of bench.verify_c3 (make_visual_frame_realistic, seed 300, the
bench's covariances) replayed with the oracle for the first F filters.

Nothing of the gate is restated here. The prefix of chi2 behind the first m rows of the blocked Cholesky, noise_scale z[:m]' z[:m]
with z = L^-1 v, equals the quadratic form of the LEADING m x m problem, v[:m]' S[:m, :m]^-1 v[:m]: the oracle's own gate
(orc_ekf_visual_track_outlier_check: its S = H P H' + R, its factorisation, its noise scale) run on the first m rows of (H, f, y)
returns it, and the threshold is the oracle's table entry for the WHOLE track (oracle/chi2inv95.h). The device checks the prefix behind
every 16-column block but the last, with the margin 1 + 2^-20.

usage: python scripts/gate_prefix_replay.py [F ...]      (default: 48 256; prints one table per F)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench                                                             # noqa: E402
import ekf_truth as tr                                                   # noqa: E402
from oracle import orc                                                   # noqa: E402

MARGIN = 1.0 + 2.0 ** -20
SHORT_NP = 12                                                            # the split form's short class: up to 12 stereo poses (48 rows)


def replay(F, seed=0):
    rng = np.random.default_rng(300 + seed)
    T1, T2, means, lens, idx, feat, vel, y = bench.make_visual_frame_realistic(rng, F)
    table, par = tr.chi2inv95(), orc.tri_default_params()
    base = orc.Ekf(orc.ekf_default_params(cameraTrailLength=20)).P.copy() * 1e-6
    base += np.eye(len(base)) * 1e-4
    prng = np.random.default_rng(7000 + seed)                            # VisualEkfBench.P0_host
    P0 = np.empty((F,) + base.shape)
    for b0 in range(0, F, 64):
        A = prng.normal(size=(min(64, F - b0),) + base.shape) * 0.01
        P0[b0:b0 + len(A)] = base + (A @ A.transpose(0, 2, 1)) * 1e-3
    cls = {c: {"gated": 0, "rejected": 0, "decided": {}, "blocks_run": 0, "blocks": 0, "pivots_run": 0, "pivots": 0,
               "accepted": 0, "accepted_crossing": 0, "max_accepted_prefix": 0.0} for c in ("short", "long")}
    for s in range(F):
        o = orc.Ekf(orc.ekf_default_params(cameraTrailLength=20))
        o.set_state(means[s]); o.set_cov(P0[s]); o.set_first_sample_time(0.0)
        done = 0
        for v in range(bench.VISITS):
            if done >= bench.QUOTA:
                break
            n = int(lens[v, s])
            ots, ops, _, oH, of = orc.visual_track_prepare(par, o.m.copy(), idx[v, s, :n], T1, T2, feat[v, s, :2 * n], vel[v, s, :2 * n])
            if (ots, ops) != (0, 0):
                continue
            yy, rows = y[v, s, :4 * n], 4 * n
            status, chi2 = o.visual_track_outlier_check(oH, of, yy, bench.R_GATE)
            thr, nblocks = table[rows], (rows + 15) // 16
            c = cls["short" if n <= SHORT_NP else "long"]
            c["gated"] += 1
            decided = None
            for k in range(1, nblocks):                                  # behind every block column but the last
                m = 16 * k
                prefix = o.visual_track_outlier_check(oH[:m], of[:m], yy[:m], bench.R_GATE)[1]
                assert prefix <= chi2 * (1 + 1e-9), (s, v, k, prefix, chi2)
                if status == 0:
                    c["max_accepted_prefix"] = max(c["max_accepted_prefix"], prefix / thr)
                if prefix > thr * MARGIN:
                    decided = k
                    break
            if status == 0:
                c["accepted"] += 1
                c["accepted_crossing"] += int(decided is not None)
                o.update_visual_track(oH, of, yy, bench.R_UPDATE); done += 1
                continue
            c["rejected"] += 1
            c["decided"][decided or "full"] = c["decided"].get(decided or "full", 0) + 1
            c["blocks"] += nblocks; c["blocks_run"] += decided or nblocks
            c["pivots"] += rows; c["pivots_run"] += 16 * decided if decided else rows
    return cls


def main():
    for F in [int(a) for a in sys.argv[1:]] or [48, 256]:
        cls = replay(F)
        print(f"# {F} filters, make_visual_frame_realistic seed 300, visit loop of verify_c3 ({bench.VISITS} visits, quota {bench.QUOTA}), margin 1 + 2^-20")
        print("class  gated  rejected  decided behind block 1 / 2 / 3 / 4 / 5 / never (whole factor)  blocks run / all (rejected)  pivots run / all (rejected)"
              "  accepted  accepted that cross  largest prefix / threshold of an accepted record")
        tot = {"r": 0, "br": 0, "b": 0, "pr": 0, "p": 0}
        for name in ("short", "long"):
            c = cls[name]
            d = " / ".join(str(c["decided"].get(k, 0)) for k in (1, 2, 3, 4, 5, "full"))
            print(f"{name:5s}  {c['gated']:5d}  {c['rejected']:8d}  {d:40s}  {c['blocks_run']:5d} / {c['blocks']:5d}  "
                  f"{c['pivots_run']:6d} / {c['pivots']:6d} ({c['pivots_run'] / max(c['pivots'], 1):.2f})  {c['accepted']:5d}  {c['accepted_crossing']:3d}  "
                  f"{c['max_accepted_prefix']:.4f}")
            tot["r"] += c["rejected"]; tot["br"] += c["blocks_run"]; tot["b"] += c["blocks"]; tot["pr"] += c["pivots_run"]; tot["p"] += c["pivots"]
            assert c["accepted_crossing"] == 0
        print(f"all    rejected {tot['r']}: diagonal blocks run {tot['br']} of {tot['b']}, pivots {tot['pr']} of {tot['p']} ({tot['pr'] / max(tot['p'], 1):.2f})")
        print()


if __name__ == "__main__":
    main()
