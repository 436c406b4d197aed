"""Block-wise accuracy of per-track triangulation + prepareVisualUpdate: the truth, the scale and the bar.

Test infrastructure only (not collected, imported by test_vu_truth.py and test_gpu_vu_accuracy.py; nothing under hybvio_amd/ uses it).

THE TRUTH is oracle/triangulation_oracle.c compiled a second time with real = long double (oracle/Makefile: liboracle_ld.so, bound by
orc.visual_track_prepare_as("ld", ...)): one statement of the algorithm at two precisions, so the oracle and the truth differ by
rounding only. The inputs (mean, feature coordinates, velocities, extrinsics, parameters) stay binary64 values.

THE METRIC looks at every row of H and every column block of the state on its own,

    err(X)[row, block] = max |X - T| over the block,

the blocks being POS (3), ORI (4), SFT (1) and per trail pose its position (3) and its quaternion (4): a whole-matrix Frobenius
norm sees the large entries only, and a defect confined to one small block (the time-shift column, one pose's quaternion) hides behind
them. Velocity and bias columns are exactly zero and asserted so.

THE SCALE is the oracle's own distance from the truth -- but not one realisation of it. A track's errors come from a few
cancellations, all fed by the same triangulated point, so two correct binary64 evaluations differ from the truth by amounts whose ratio
reaches 10 .. 20 per track. The scale is therefore taken over an ENSEMBLE: the unperturbed inputs plus K - 1 copies in which the mean and
the feature coordinates are multiplied by 1 + 2^-52 u, u uniform in [-1, 1] from a fixed seed; on every member the plain oracle and the
truth are evaluated ON THE SAME perturbed inputs, and the scale per (row, block) of H, for pf and for every entry of f is the largest
oracle-minus-truth distance over the members. The bar is

    err <= FACTOR x (scale + FLOOR x max |T| over the block)          FLOOR = 64 eps (the project's figure, test_gpu_ekf_accuracy.py)

with max |T| = max |pf_T| for pf and 1 for f (normalised image coordinates). A track is left out of the comparison (and still compared
by status) if any member's triangulation status, prepare status or Gauss-Newton iteration count differs from the unperturbed truth's,
in either precision: its result is then not a smooth function of its inputs at rounding level.

FACTOR is measured, before any device has been seen, from a second CORRECT binary64 build of the oracle (oracle/Makefile `standin`:
-O3 -march=native -ffp-contract=fast -ffast-math) that stands in for the device: its worst ratio to the scale over the whole corpus
below, times four (the device restructures more than a compiler does: parallel derivative columns, 11 nt - 7 motion pairs per
iteration, the factor form), rounded up to a power of two. tests/test_vu_truth.py re-measures the ratio and asserts the stand-in passes.
"""
from __future__ import annotations

import copy
import functools
import hashlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import ekf_truth as tr
from hybvio_amd import synth
from oracle import orc

LD = tr.LD                                            # (ekf_truth refuses to import where np.longdouble is no wider than binary64)
EPS64 = tr.EPS64
FLOOR = 64 * EPS64
K = 16
# The stand-in's worst ratio to the scale over the corpus (K = 16, every compared track, every row and block):
#   H 2.03 (case s20_np21, track 0, row 67, quaternion of pose 17), pf 1.46, f 0.49; re-measured by
#   test_vu_truth.py::test_stand_in_differs_in_bits_and_passes. Fixed before the first device run.
STANDIN_WORST = 2.03
FACTOR = 16.0                                         # 4 x 2.03 = 8.1, rounded up to a power of two
POS, ORI, SFT, CAM, POSE = tr.POS, tr.ORI, tr.SFT, tr.CAM, tr.POSE
ZERO_COLS = np.r_[3:6, 10:19]                         # velocity and biases never enter a visual Jacobian
B = 48

# name: (trail, poses, stereo, triangulation parameter overrides, feature-velocity factor)
CASES = {
    "s20_np10": (20, 10, True, {}, 1.0),
    "s20_np21": (20, 21, True, {}, 1.0),
    "s20_np12": (20, 12, True, {}, 1.0),              # the last short shape (48 rows) ...
    "s20_np13": (20, 13, True, {}, 1.0),              # ... and the first long one
    "m20_np4": (20, 4, False, {}, 1.0),
    "m20_np21": (20, 21, False, {}, 1.0),
    "s12_np2": (12, 2, True, {}, 1.0),
    "m5_np6": (5, 6, False, {}, 1.0),
    "s20_np10_linear": (20, 10, True, {"useLinearTriangulation": 1}, 1.0),
    "m20_np5_linear": (20, 5, False, {"useLinearTriangulation": 1}, 1.0),
    "s20_np13_vel5": (20, 13, True, {}, 5.0),         # the SFT column carries weight
    "s20_np13_vel5_noshift": (20, 13, True, {"estimateImuCameraTimeShift": 0}, 5.0),     # ... and must be exactly zero
}


def _seed(name):
    return [int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little"), 2025]


@functools.lru_cache(maxsize=None)
def corpus(name, count=B):
    """The case's inputs: (T1, T2, means, idx, feat, vel, parameter overrides), `count` tracks from synth.visual_tracks."""
    trail, npose, stereo, over, velx = CASES[name]
    rng = np.random.default_rng(_seed(name))
    T1, T2, means, idx, feat = synth.visual_tracks(rng, count, trail, npose, stereo)
    vel = 0.1 * velx * rng.normal(size=feat.shape)                    # (0.1: the size the reference's own fixtures use)
    return T1, T2, means, idx, feat, vel, dict(over)


def blocks(n):
    """[(name, columns)] of a state of dimension n = 20 + 7 trail: the column blocks a visual Jacobian can touch."""
    out = [("POS", np.arange(POS, POS + 3)), ("ORI", np.arange(ORI, ORI + 4)), ("SFT", np.arange(SFT, SFT + 1))]
    for k in range((n - CAM) // POSE):
        out.append((f"p{k}", np.arange(CAM + POSE * k, CAM + POSE * k + 3)))
        out.append((f"q{k}", np.arange(CAM + POSE * k + 3, CAM + POSE * k + 7)))
    return out


def block_max(X, n):
    """max |X| over each block: (rows, blocks)."""
    X = np.abs(np.asarray(X, LD))
    return np.stack([X[:, c].max(axis=1) for _, c in blocks(n)], axis=1)


def evaluate(kind, par, m, idx, T1, T2, feat, vel):
    """(triangulation status, prepare status, iterations, pf, H, f) from the plain oracle ('oracle'), the truth ('ld') or the
    stand-in ('standin')."""
    if kind == "oracle":
        st, ps, pf, H, f = orc.visual_track_prepare(par, m, idx, T1, T2, feat, vel)
        it = orc.tri_last_diag()[2]
    else:
        st, ps, pf, H, f = orc.visual_track_prepare_as(kind, par, m, idx, T1, T2, feat, vel)
        it = orc.tri_last_diag_as(kind)[2]
    return st, ps, (0 if par.useLinearTriangulation else int(it)), pf, H, f


def gate_chi2(P, H, f, y, r, ns):
    """The gate statistic of (H, f) against covariance P in long double (ekf_truth.gate_chi2 on the columns H touches)."""
    H = np.asarray(H, LD)
    v = np.asarray(y, LD) - np.asarray(f, LD)
    return tr.gate_chi2(P, H, v, (float(r) * float(r)) * float(ns), ns)      # rd: a binary64 product in the oracle and on the device


class Ensemble:
    """One track's truth, the oracle's result and the scale (see the module docstring). keep: the members' (H, f) of both precisions are
    kept, for with_gate."""

    def __init__(self, par, m, idx, T1, T2, feat, vel, seed, k=K, keep=False):
        n = len(m)
        rng = np.random.default_rng(seed)
        self.n, self.excluded = n, False
        self.sH = self.spf = self.sf = None
        self.members = []
        for member in range(k):
            mm, ff = np.array(m, np.float64), np.array(feat, np.float64)
            if member:
                mm = mm * (1.0 + 2.0 ** -52 * rng.uniform(-1, 1, mm.shape))
                ff = ff * (1.0 + 2.0 ** -52 * rng.uniform(-1, 1, ff.shape))
            o = evaluate("oracle", par, mm, idx, T1, T2, ff, vel)
            t = evaluate("ld", par, mm, idx, T1, T2, ff, vel)
            if member == 0:
                self.status, self.iters = (t[0], t[1]), t[2]
                self.ok = self.status == (0, 0)
                self.oracle_status = (o[0], o[1])
                self.pf, self.H, self.f = t[3], t[4], t[5]
                self.o_pf, self.o_H, self.o_f = o[3], o[4], o[5]
            if (o[0], o[1], o[2]) != (*self.status, self.iters) or (t[0], t[1], t[2]) != (*self.status, self.iters):
                self.excluded = True
            if not self.ok:
                break                                                  # a non-OK track is compared by status alone
            if (o[0], o[1]) != (0, 0) or (t[0], t[1]) != (0, 0):
                continue                                               # (excluded above; its H is not a Jacobian)
            dH, dpf, df = block_max(o[4] - t[4], n), np.abs(o[3] - t[3]).max(), np.abs(o[5] - t[5])
            self.sH = dH if self.sH is None else np.maximum(self.sH, dH)
            self.spf = dpf if self.spf is None else max(self.spf, dpf)
            self.sf = df if self.sf is None else np.maximum(self.sf, df)
            if keep:
                self.members.append((o[4], o[5], t[4], t[5]))
        if self.ok:
            self.magH = block_max(self.H, n)
            self.bH = self.sH + FLOOR * self.magH                      # the budget is FACTOR x these
            self.bpf = self.spf + FLOOR * np.abs(self.pf).max()
            self.bf = self.sf + FLOOR

    def with_gate(self, ekf, P, y, r, ns):
        """A copy that also holds the gate's chi2 against covariance P at gate noise r: the truth's, v' S^-1 v in long double from the
        long-double (H, f); the oracle's, from its prepare + outlier check (ekf: an oracle filter holding P); and the scale, the largest
        distance between the two over the members."""
        g = copy.copy(self)
        if not self.ok:
            return g
        g.schi = 0.0
        for k, (oH, of, tH, tf) in enumerate(self.members):
            co, ct = ekf.visual_track_outlier_check(oH, of, y, r)[1], gate_chi2(P, tH, tf, y, r, ns)
            if k == 0:
                g.chi2, g.o_chi2 = ct, co
            g.schi = max(g.schi, float(abs(LD(co) - ct)))
        g.bchi = g.schi + FLOOR * max(LD(1), g.chi2)
        return g

    # ratios to the budget's base: a result passes with ratio <= FACTOR
    def ratio_H(self, H):
        assert not np.asarray(H)[:, ZERO_COLS].any(), "velocity / bias columns of H must be exactly zero"
        return _ratio(block_max(np.asarray(H, LD) - self.H, self.n), self.bH)

    def ratio_pf(self, pf):
        return float(_ratio(np.abs(np.asarray(pf, LD) - self.pf).max(), self.bpf))

    def ratio_f(self, f):
        return _ratio(np.abs(np.asarray(f, LD) - self.f), self.bf)

    def ratio_chi2(self, chi2):
        return float(_ratio(abs(LD(chi2) - self.chi2), self.bchi))


def _ratio(num, den):
    return np.asarray(tr._ratio(num, den), np.float64)


def frob(X, O):
    """The figure the parity tests see: ||X - O||_F / ||O||_F against the ORACLE."""
    X, O = np.asarray(X, np.float64), np.asarray(O, np.float64)
    return float(np.linalg.norm(X - O) / max(np.linalg.norm(O), 1e-300))


def params_of(over):
    return orc.tri_default_params(**over)


@functools.lru_cache(maxsize=None)
def case_ensembles(name):
    """The case's 48 ensembles, computed once per process."""
    T1, T2, means, idx, feat, vel, over = corpus(name)
    par = params_of(over)
    return in_threads(lambda b: Ensemble(par, means[b], idx[b], T1, T2, feat[b], vel[b], _seed(name) + [b]), range(len(means)))


def in_threads(fn, items):
    """[fn(x) for x in items] on up to 8 threads: the time goes to the C evaluations, which run without the interpreter lock, and
    the oracle's per-call diagnostics are thread-local."""
    orc.tri_last_diag(), orc.tri_last_diag_as("ld")                   # both libraries loaded (in a fresh tree: built) before any thread asks
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return list(pool.map(fn, items))


def corpus_hash(prepare=None):
    """sha256 over the plain double build's statuses, pf, H and f on every track of every case (prepare: another build's
    visual_track_prepare): equal hashes = bit-identical oracles."""
    prepare = prepare or orc.visual_track_prepare
    h = hashlib.sha256()
    for name in CASES:
        T1, T2, means, idx, feat, vel, over = corpus(name)
        par = params_of(over)
        for b in range(len(means)):
            st, ps, pf, H, f = prepare(par, means[b], idx[b], T1, T2, feat[b], vel[b])
            h.update(np.array([st, ps], np.int32).tobytes() + pf.tobytes() + np.ascontiguousarray(H).tobytes() + f.tobytes())
    return h.hexdigest()


class Judge:
    """Prints every comparison before anything is asserted, then fails with the whole list (as test_gpu_ekf_accuracy.Judge)."""

    def __init__(self, what):
        self.what, self.failures, self.worst = what, [], {}

    def fail_if(self, cond, msg):
        if cond:
            self.failures.append(msg)

    def track(self, tag, ens, pf, H, f):
        """One compared track: the result's ratios, the oracle's own, the Frobenius figure. Returns the line's figures."""
        names = [nm for nm, _ in blocks(ens.n)]
        rH, rO = ens.ratio_H(H), ens.ratio_H(ens.o_H)
        i, j = np.unravel_index(np.argmax(rH), rH.shape)
        rpf, rf = ens.ratio_pf(pf), float(ens.ratio_f(f).max())
        fig = dict(H=float(rH.max()), H_oracle=float(rO.max()), where=f"row {i} {names[j]}", pf=rpf, pf_oracle=ens.ratio_pf(ens.o_pf),
                   f=rf, f_oracle=float(ens.ratio_f(ens.o_f).max()), frob=frob(H, ens.o_H), frob_pf=frob(pf, ens.o_pf))
        self.fail_if(not fig["H"] <= FACTOR, f"{tag}: H {fig['where']} at {fig['H']:.3g} x the scale (bar {FACTOR:g}; Frobenius {fig['frob']:.2e})")
        self.fail_if(not rpf <= FACTOR, f"{tag}: pf at {rpf:.3g} x the scale")
        self.fail_if(not rf <= FACTOR, f"{tag}: f at {rf:.3g} x the scale")
        for k_ in ("H", "H_oracle", "pf", "pf_oracle", "f", "f_oracle", "frob", "frob_pf"):
            if fig[k_] >= self.worst.get(k_, -1.0):
                self.worst[k_] = fig[k_]
                if k_ == "H":
                    self.worst["where"] = f"{tag} {fig['where']}"
        return fig

    def summary(self, extra=""):
        w = self.worst
        if w:
            print(f"ACC {self.what}: worst ratio to the scale (bar {FACTOR:g}) H {w['H']:.3g} [{w['where']}] oracle {w['H_oracle']:.3g}; "
                  f"pf {w['pf']:.3g} oracle {w['pf_oracle']:.3g}; f {w['f']:.3g} oracle {w['f_oracle']:.3g}; "
                  f"Frobenius vs oracle H {w['frob']:.2e} pf {w['frob_pf']:.2e}{extra}")
        else:
            print(f"ACC {self.what}: nothing compared{extra}")

    def done(self):
        assert not self.failures, f"{self.what}: " + " | ".join(self.failures[:12]) + (f" | ... {len(self.failures)} in all" if len(self.failures) > 12 else "")


def judge_case(J, name, ens, results, min_ok=0.75, max_excluded=0.10):
    """results[b] = (triangulation status, prepare status, pf, H, f) of track b from the implementation under test. Statuses are
    compared on every track, values on every OK track that is not excluded; the case's own conditions are checked too."""
    n_ok = sum(e.ok for e in ens)
    n_exc = sum(e.ok and e.excluded for e in ens)
    compared = 0
    for b, (e, (st, ps, pf, H, f)) in enumerate(zip(ens, results)):
        J.fail_if((st, ps) != e.status, f"{name}[{b}]: status {(st, ps)} vs the truth's {e.status}")
        if e.ok and not e.excluded and (st, ps) == (0, 0):
            J.track(f"{name}[{b}]", e, pf, H, f)
            compared += 1
    J.fail_if(n_ok < min_ok * len(ens), f"{name}: only {n_ok} of {len(ens)} tracks OK")
    J.fail_if(n_exc > max_excluded * n_ok, f"{name}: {n_exc} of {n_ok} OK tracks excluded")
    J.summary(f"; {compared} compared, {n_ok} OK, {n_exc} excluded of {len(ens)}")
    return compared


# ---- the gate: chi2 of hv_ekf_visual_track_dev, whose Jacobian no entry point returns ----

GATE_B, GATE_TRAIL, GATE_POSES = 16, 20, (9, 21)
GATE_COVS = ("dense", "c", "d", "e")
# trackChiTestOutlierR = 1.5 as the product runs it: rd = r^2 noiseScale^2 = 22500 beside diag(H P H') of 3e-4 (regime e) .. 3 (dense), so
# S is nearly a multiple of the identity and chi2 feels H through a 1e-4 correction only. 0.01: rd = 1, where S is made of H P H'.
GATE_R = (1.5, 0.01)
R_UPDATE = 0.05                                                       # visualR


@functools.lru_cache(maxsize=None)
def gate_corpus(npose):
    """16 stereo tracks on the 20-pose trail and their measurements: (T1, T2, means, idx, feat, vel, y)."""
    rng = np.random.default_rng([npose, 77, 2025])
    T1, T2, means, idx, feat = synth.visual_tracks(rng, GATE_B, GATE_TRAIL, npose, True)
    vel = 0.1 * rng.normal(size=feat.shape)
    y = feat.reshape(GATE_B, -1) + 2e-3 * rng.normal(size=(GATE_B, feat.shape[1] * 2))
    return T1, T2, means, idx, feat, vel, y


@functools.lru_cache(maxsize=None)
def gate_covariances():
    """{name: [P per filter]}: `dense` is the parity test's well-conditioned random covariance (one per filter); c, d, e are the
    first trail-20 snapshot with a filled trail of ekf_truth.realistic_filters' regimes (the trail just filled, the first visual updates,
    steady state), symmetrised, the same for every filter. The snapshots are paired with the SYNTHETIC means of gate_corpus: the
    snapshot's own trail is a standing sensor and cannot be triangulated. That pairing is unphysical -- the covariance does not
    describe the uncertainty of these poses -- but numerically it is what a gate sees: H from one state, P with a running filter's
    scales (1e-8 .. 1e4 on the diagonal) and near-singular correlations."""
    params, snaps = tr.realistic_filters(orc, np.random.default_rng(2024), trail=GATE_TRAIL)
    n = 20 + 7 * GATE_TRAIL
    rng = np.random.default_rng(4242)
    P0 = orc.Ekf(params).P.copy()
    out = {"dense": []}
    for _ in range(GATE_B):
        A = rng.normal(size=(n, n)) * 0.02
        P = P0 * 1e-6 + A @ A.T * 1e-3 + np.eye(n) * 1e-4
        out["dense"].append(0.5 * (P + P.T))
    for r in ("c", "d", "e"):
        P = tr.filled(snaps[r], GATE_TRAIL)[0][2]
        out[r] = [0.5 * (P + P.T)] * GATE_B
    return params, out


@functools.lru_cache(maxsize=None)
def _gate_base(npose):
    """The 16 ensembles of gate_corpus(npose), members kept: the prepare side does not depend on the covariance."""
    T1, T2, means, idx, feat, vel, y = gate_corpus(npose)
    par = params_of({})
    return in_threads(lambda b: Ensemble(par, means[b], idx[b], T1, T2, feat[b], vel[b], [npose, 77, b], keep=True), range(GATE_B))


@functools.lru_cache(maxsize=None)
def gate_ensembles(npose, cov, r_gate):
    """The 16 ensembles of gate_corpus(npose) against covariance `cov` at gate noise r_gate, with the gate's chi2 and its scale."""
    y = gate_corpus(npose)[6]
    params, covs = gate_covariances()
    ns, base = params.noiseScale * params.noiseScale, _gate_base(npose)

    def one(b):
        ekf = orc.Ekf(params)                                         # its own: the outlier check works in the filter's buffers
        ekf.set_cov(covs[cov][b])
        return base[b].with_gate(ekf, covs[cov][b], y[b], r_gate, ns)
    return in_threads(one, range(GATE_B))


def gate_status(chi2, nr):
    return tr.CHI2 if chi2 > tr.chi2inv95()[nr] else tr.INLIER


def judge_gate(J, tag, ens, st, gs, chi, pf):
    """The device's (statuses [B, 2], gate status [B], chi2 [B], pf [B, 3]) of one visit against the ensembles. Returns (compared, worst
    chi2 ratio, the oracle's worst, worst relative chi2 distance to the oracle)."""
    worst = worst_o = worst_rel = worst_pf = 0.0
    compared = 0
    for b, e in enumerate(ens):
        J.fail_if(tuple(int(x) for x in st[b]) != e.status, f"{tag}[{b}]: status {st[b]} vs the truth's {e.status}")
        if not e.ok:
            J.fail_if(gs[b] != 1, f"{tag}[{b}]: gate status {gs[b]} on a track that was not prepared")
            continue
        if e.excluded or tuple(int(x) for x in st[b]) != (0, 0):
            continue
        nr = len(e.f)
        r, ro, rp = e.ratio_chi2(chi[b]), e.ratio_chi2(e.o_chi2), e.ratio_pf(pf[b])
        worst, worst_o, worst_pf = max(worst, r), max(worst_o, ro), max(worst_pf, rp)
        worst_rel = max(worst_rel, abs(chi[b] - e.o_chi2) / max(1.0, abs(e.o_chi2)))
        J.fail_if(not r <= FACTOR, f"{tag}[{b}]: chi2 {chi[b]!r} vs the truth's {float(e.chi2)!r}: {r:.3g} x the scale (bar {FACTOR:g})")
        J.fail_if(not rp <= FACTOR, f"{tag}[{b}]: pf at {rp:.3g} x the scale")
        if abs(e.chi2 - tr.chi2inv95()[nr]) > FACTOR * e.bchi:
            J.fail_if(gs[b] != gate_status(e.chi2, nr), f"{tag}[{b}]: gate status {gs[b]} vs the truth's {gate_status(e.chi2, nr)}")
        compared += 1
    print(f"ACC {J.what} {tag}: chi2 worst ratio to the scale (bar {FACTOR:g}) device {worst:.3g} oracle {worst_o:.3g}; pf {worst_pf:.3g}; "
          f"relative distance to the oracle's chi2 {worst_rel:.2e}; {compared} compared of {len(ens)}")
    return compared, worst, worst_o, worst_rel
