#!/usr/bin/env python3
"""CPU-only companion of tests/test_gpu_ekf_accuracy.py (profiles/ekf_accuracy/README.md): binary64 numpy emulations of the two
augmentation algebras -- the expanded rank-14 form P = sym(P1 - K HP - G K') the kernel used, and the form it uses now (those
14 columns from W = P1 - K HP and the rows of T = I - K H) -- and of the update's P -= Y'Y, fed through the accuracy test's
own assertions on the snapshots of tests/ekf_truth.realistic_filters. The negative control: the expanded form must FAIL the
budget, or the tests would not catch the defect they were written for. numpy's summation order is not the device's; these are
emulations of the algebra, not of the kernels.

    python scripts/ekf_accuracy_emulation.py [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ekf_truth as tr                                                # noqa: E402
from oracle import orc                                                # noqa: E402

CAM, POSE = tr.CAM, tr.POSE


def _shifted(m, P, k, params):
    n, trail = len(m), params.cameraTrailLength
    ns = params.noiseScale ** 2
    m1, P1 = tr.shift(m, P, tr.aug_src(n, trail - 1 if k == -1 else k))
    P1 = P1.astype(np.float64).copy()
    for i in range(POSE):
        P1[CAM + i, CAM + i] += (params.noiseInitialPosTrail ** 2 if i < 3 else params.noiseInitialOriTrail ** 2) * ns
    H = np.asarray(tr.aug_H(n), np.float64)
    HP = H @ P1
    S0 = HP @ H.T
    rd = params.augmentR * ns
    L = np.linalg.cholesky(0.5 * (S0 + S0.T) + rd * np.eye(POSE))
    K = np.linalg.solve(L.T, np.linalg.solve(L, HP)).T
    return m1, P1, H, HP, S0, K, rd


def augment_expanded(m, P, k, params):
    """ekf_augment_kernel steps 3-4 as they were: G = P1 H' - K S0 - rd K, P = sym(P1 - K HP - G K')."""
    m1, P1, H, HP, S0, K, rd = _shifted(m, P, k, params)
    G = P1 @ H.T - K @ S0 - rd * K
    X = P1 - K @ HP - G @ K.T
    return 0.5 * (X + X.T)


def augment_columns(m, P, k, params):
    """The same, but the 14 columns visAugH touches (and their rows) come from W T(j, :)' + rd K K(j, :)'."""
    m1, P1, H, HP, S0, K, rd = _shifted(m, P, k, params)
    G = P1 @ H.T - K @ S0 - rd * K
    X = P1 - K @ HP - G @ K.T
    W = P1 - K @ HP
    cols = np.flatnonzero(np.abs(H).sum(0))
    T = -(K[cols] @ H)
    T[np.arange(len(cols)), cols] += 1.0
    X[:, cols] = W @ T.T + rd * K @ K[cols].T
    X[cols, :] = X[:, cols].T
    return 0.5 * (X + X.T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    a = ap.parse_args()
    out = []
    for trail in (20, 5):
        params, snaps = tr.realistic_filters(orc, np.random.default_rng(2024), trail=trail)
        for regime in tr.REGIMES:
            for frame, m, P in snaps[regime]:
                k = tr.discard_index(frame, trail)
                _, T = tr.augment(m, P, k, params)
                o = orc.Ekf(params); o.set_state(m); o.set_cov(P)
                o.update_visual_pose_augmentation(k)
                row = {"trail": trail, "regime": regime, "frame": frame, "corr_min_eig": tr.corr_min_eig(T),
                       "oracle": tr.scaled_err(o.P, T)}
                for name, fn in (("expanded", augment_expanded), ("columns", augment_columns)):
                    X = fn(m, P, k, params)
                    row[name], row[name + "_frobenius"] = tr.scaled_err(X, T), tr.frob_err(X, T)
                    row[name + "_passes"] = bool(row[name] <= max(8 * row["oracle"], 64 * tr.EPS64))
                    row[name + "_corr_min_eig"] = tr.corr_min_eig(X)
                out.append(row)
                print(" ".join(f"{k_}={v:.2e}" if isinstance(v, float) else f"{k_}={v}" for k_, v in row.items()))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
