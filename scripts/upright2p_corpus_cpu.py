#!/usr/bin/env python3
"""CPU figures of tests/upright2p_restatement.py alone on the corpus of tests/test_gpu_upright2p.py (no GPU): the branches it
reaches, the truth-recoverable sets, the agreement with the ground truth per camera / noise / tilt cell, and how many sets change
when every normalised coordinate and ray component moves by one ulp (the size of a device-libm difference inside the camera calls).
usage: scripts/upright2p_corpus_cpu.py > profiles/upright2p/cpu_corpus.txt"""
import os
import sys
ROOT =os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from oracle import orc
orc.build()
import test_gpu_upright2p as G
import upright2p_restatement as U
groups = G.build_sets(orc)
corpus = [d for _, _, sets in groups for d in sets]
print("sets", len(corpus))
G.branches(corpus)
sm = np.array([d["ref"][2] for d in corpus])
print("not run", int((sm[:, 3] < 2).sum()), "at min", int((sm[:, 2] == 50).sum()), "between", int(((sm[:, 2] > 50) & (sm[:, 2] < 98)).sum()),
      "at cap", int((sm[:, 2] == 98).sum()), "no model", int(((sm[:, 3] >= 2) & (sm[:, 1] < 0)).sum()))
nf = [d for d in corpus if G.truth_recoverable(d)]
badnf = [(d["cam"], d["n"], d["outl"], d["kind"]) for d in nf if not np.array_equal(d["ref"][0] == 0, d["truth"])]
print("truth-recoverable sets", len(nf), "not recovering", badnf)
rows = {}
for d in corpus:
    if G.well_separated(d) and d["noise"] > 0:
        k = (d["cam"], d["noise"], d["tilt"])
        a = rows.setdefault(k, [0, 0])
        a[0] += int(((d["ref"][0] == 0) == d["truth"]).sum()); a[1] += d["n"]
tot = [0, 0]
for k in sorted(rows):
    print("agreement", k, "%d / %d = %.4f" % (rows[k][0], rows[k][1], rows[k][0] / rows[k][1])); tot[0] += rows[k][0]; tot[1] += rows[k][1]
print("agreement all noisy well-separated %d / %d = %.4f" % (tot[0], tot[1], tot[0] / tot[1]))
rng = np.random.default_rng(0)
def ulp(a):
    return np.nextafter(a, np.where(rng.integers(0, 2, a.shape) > 0, np.inf, -np.inf))
changed, changed_ws, worst = 0, 0, 0
for name, _, sets in groups:
    ocam, _ = G._cams(orc, name)
    for d in sets:
        ts, model, summ = G._reference(d, ocam, perturb=ulp)
        if not (np.array_equal(ts, d["ref"][0]) and list(summ) == list(d["ref"][2])):
            changed += 1
            dn = abs(int((ts == 0).sum()) - int((d["ref"][0] == 0).sum()))
            worst = max(worst, dn / max(1, d["n"]))
            ws = G.well_separated(d) and d["cam"] != "fisheye"
            changed_ws += ws
            print("  one ulp changes", d["cam"], d["n"], d["outl"], d["noise"], d["kind"], list(d["ref"][2]), list(summ), "inliers differ by", dn, "well-separated pinhole" if ws else "")
print("one-ulp: %d of %d sets change (%.2f %%), %d among the well-separated pinhole sets" % (changed, len(corpus), 100.0 * changed / len(corpus), changed_ws))
