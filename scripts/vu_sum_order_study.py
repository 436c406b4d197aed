#!/usr/bin/env python3
"""The order of the Gauss-Newton derivative sums and what it costs in accuracy (profiles/vu_accuracy/README.md), without a device.

vu_sum_order_study.patch turns oracle/triangulation_oracle.c into a copy whose derivative-column sums can be taken in the orders
the kernels use (csrc/vu_prepare.hip, "derivative columns"), chosen with -DSUM_ORDER=n:
  0  the reference's: one sum per column, pose by pose (bit-identical to the oracle)
  1  the plain part (the point moves) and the motion part (a pose moves) in separate sums
  2  the plain part as (sum_i L_i) d_j through the summed linear maps, the motion part separate: the kernels' form
  3  as 2, but the seven pose-0 columns in the reference's order
  5  as 3, the maps summed and contracted in long double
  7  as 3, with the term X E'E d_j = d_j cancelled by hand
  8  as 2 in every iteration but the converging one, which keeps the reference's order
Each build is judged like the device (tests/vu_truth.py) on the tracks given, default: the five the device fails on.

    python scripts/vu_sum_order_study.py [case:track ...]
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
ORDERS = {0: "reference", 1: "plain | motion", 2: "summed maps (kernel)", 3: "maps, pose-0 columns per pose", 5: "... long-double maps",
          7: "... X E'E d cancelled by hand", 8: "kernel form, last pass in reference order"}
FAILING = ("s20_np10:19", "s20_np21:0", "m20_np4:19", "m20_np21:17", "m20_np21:18")


def build(order, out_dir):
    """The patched source compiled like liboracle.so with -DSUM_ORDER=order; returns its visual_track_prepare."""
    from oracle import orc
    src = os.path.join(out_dir, "triangulation_sum_order_study.c")
    if not os.path.exists(src):
        subprocess.check_call(["patch", "-s", "-o", src, os.path.join(ROOT, "oracle", "triangulation_oracle.c"),
                               os.path.join(ROOT, "scripts", "vu_sum_order_study.patch")])
    so = os.path.join(out_dir, f"libsum_order_{order}.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-std=c11", "-ffp-contract=off", "-fno-fast-math", f"-DSUM_ORDER={order}", "-shared",
                           "-o", so, src, "-lm"])
    fn = C.CDLL(so).orc_visual_track_prepare
    fn.argtypes = [C.c_void_p, orc.f64p, C.c_int, orc.i32p, C.c_int] + [orc.f64p] * 7 + [orc.i32p]

    def prepare(par, m, idx, T1, T2, feat, vel):
        m, idx = np.ascontiguousarray(m, np.float64), np.ascontiguousarray(idx, np.int32)
        nt = len(idx) * (2 if T2 is not None else 1)
        H, f, pf, ps = np.zeros((len(m), 2 * nt)), np.zeros(2 * nt), np.zeros(3), np.zeros(1, np.int32)
        a = [np.ascontiguousarray(x, np.float64) for x in (T1, T1 if T2 is None else T2, feat, vel)]
        p = lambda x: orc._p(x, orc.f64p)
        st = fn(C.byref(par), p(m), len(m), orc._p(idx, orc.i32p), len(idx), p(a[0]), None if T2 is None else p(a[1]), p(a[2]), p(a[3]),
                p(pf), p(H), p(f), orc._p(ps, orc.i32p))
        return st, int(ps[0]), pf, H.T.copy(), f
    return prepare


def ratios(prepare, name, b):
    """(worst ratio to the scale over all blocks, over the POS / ORI blocks, median over the non-zero blocks, bits equal the oracle's)."""
    import vu_truth as vt
    T1, T2, means, idx, feat, vel, over = vt.corpus(name)
    e = vt.case_ensembles(name)[b]
    st, ps, pf, H, f = prepare(vt.params_of(over), means[b], idx[b], T1, T2, feat[b], vel[b])
    assert (st, ps) == e.status == (0, 0)
    r = e.ratio_H(H)
    return float(r.max()), float(r[:, :2].max()), float(np.median(r[e.magH > 0])), bool(np.array_equal(H, e.o_H))


def main(argv):
    tracks = [(s.split(":")[0], int(s.split(":")[1])) for s in (argv or FAILING)]
    with tempfile.TemporaryDirectory() as tmp:
        for order, what in ORDERS.items():
            prepare = build(order, tmp)
            row = [ratios(prepare, name, b) for name, b in tracks]
            print(f"SUM_ORDER {order} ({what}): " + "; ".join(f"{n}[{b}] {r[0]:.3g} / {r[1]:.3g} / {r[2]:.3g}" for (n, b), r in zip(tracks, row)))


if __name__ == "__main__":
    main(sys.argv[1:])
