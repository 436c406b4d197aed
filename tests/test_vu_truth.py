"""CPU side of the block-wise accuracy tests of triangulation + prepareVisualUpdate (tests/vu_truth.py): the truth is pinned to the
oracle, the scale's ensemble excludes nothing on the reference alone, FACTOR is re-measured on the stand-in build, and two planted
defects that the parity tests' Frobenius bar (test_gpu_visual_prepare.py: _rel < 1e-9) lets through fail the new bar.
No device takes part in any figure here."""
import math

import numpy as np
import pytest

import ekf_truth as tr
import vu_truth as vt

TOL_PARITY = 1e-9                                                     # test_gpu_visual_prepare.TOL


def _rel(a, b):                                                       # test_gpu_visual_prepare._rel
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def test_blocks_are_the_support_of_a_visual_jacobian():
    for n in (20 + 7 * 20, 20 + 7 * 5):
        cols = np.concatenate([c for _, c in vt.blocks(n)])
        assert len(cols) == len(set(cols)) and sorted(list(cols) + list(vt.ZERO_COLS)) == list(range(n))
    assert [len(c) for _, c in vt.blocks(27)] == [3, 4, 1, 3, 4]
    e = vt.case_ensembles("m5_np6")[0]
    H = np.array(e.o_H)
    H[0, 4] = 1e-300                                                  # a velocity column that is not exactly zero
    with pytest.raises(AssertionError):
        e.ratio_H(H)


def test_gate_chi2_is_visual_updates_statistic():
    rng = np.random.default_rng(5)
    n, nr = 20 + 7 * 5, 12
    A = rng.normal(size=(n, n))
    P, H, v = A @ A.T * 1e-3 + np.eye(n) * 1e-4, tr.structured_H(rng, nr, n, 5), rng.normal(size=nr)
    want = tr.visual_update(np.zeros(n), P, H, v, 0.3, 5, ns=7.0)[2]
    assert abs(float(tr.gate_chi2(P, H, v, 0.3, 7.0)) - want) <= 1e-15 * want


@pytest.mark.parametrize("name", list(vt.CASES))
def test_oracle_lies_within_rounding_of_the_truth(name):
    """Per case: the table row of profiles/vu_accuracy/README.md (oracle against truth: Frobenius, worst block relative to the block's
    own size, pf, f). The reference alone excludes no track; three quarters of the tracks are OK; both precisions agree on every
    status and iteration count; the time-shift column is exactly zero where the shift is not estimated."""
    ens = vt.case_ensembles(name)
    ok = [e for e in ens if e.ok]
    assert all(e.oracle_status == e.status for e in ens)
    assert len(ok) >= 0.75 * len(ens), (name, len(ok))
    assert not any(e.excluded for e in ens), [b for b, e in enumerate(ens) if e.excluded]
    fro = max(vt.frob(e.o_H, e.H) for e in ok)
    blk = max(float(vt._ratio(vt.block_max(np.asarray(e.o_H, vt.LD) - e.H, e.n), e.magH).max()) for e in ok)
    pf = max(float(np.abs(e.o_pf - e.pf).max() / np.abs(e.pf).max()) for e in ok)
    f = max(float(np.abs(e.o_f - e.f).max()) for e in ok)
    print(f"TRUTH {name}: {len(ok)} OK of {len(ens)}; oracle against truth: Frobenius {fro:.1e}, worst block {blk:.1e}, pf {pf:.1e}, f {f:.1e}")
    # one source at two precisions: a few cancellations' worth of binary64 rounding, nothing like the parity tolerance
    assert fro < TOL_PARITY and pf < TOL_PARITY and f < TOL_PARITY
    for e in ok:                                                      # the unperturbed oracle is a member of its own ensemble
        assert e.ratio_H(e.o_H).max() <= 1.0 and e.ratio_pf(e.o_pf) <= 1.0 and e.ratio_f(e.o_f).max() <= 1.0
        assert not np.asarray(e.H)[:, vt.ZERO_COLS].any()
        if not vt.params_of(vt.CASES[name][3]).estimateImuCameraTimeShift:
            assert not np.asarray(e.H)[:, vt.SFT].any() and not e.o_H[:, vt.SFT].any()
    if name == "s20_np13_vel5":                                       # the SFT column carries weight: as large as a pose block
        assert np.median([float(e.magH[:, 2].max() / e.magH.max()) for e in ok]) > 0.1


def test_stand_in_differs_in_bits_and_passes():
    """The -O3 -march=native -ffp-contract=fast -ffast-math build of the same source: a different binary64 evaluation (bits differ on
    most tracks), and within FACTOR of the scale on every row and block of every compared track of the corpus."""
    worst = {"H": 0.0, "pf": 0.0, "f": 0.0}
    failures = []
    for name in vt.CASES:
        T1, T2, means, idx, feat, vel, over = vt.corpus(name)
        par, ens = vt.params_of(over), vt.case_ensembles(name)
        res = [vt.evaluate("standin", par, means[b], idx[b], T1, T2, feat[b], vel[b]) for b in range(len(ens))]
        ok = [b for b, e in enumerate(ens) if e.ok]
        differ = sum(not np.array_equal(res[b][4], ens[b].o_H) for b in ok)
        assert differ > len(ok) // 2, (name, differ, len(ok))
        J = vt.Judge(f"stand-in {name}")
        vt.judge_case(J, name, ens, [(r[0], r[1], r[3], r[4], r[5]) for r in res])
        failures += J.failures
        for k in worst:
            worst[k] = max(worst[k], J.worst[k])
    rule = 2.0 ** math.ceil(math.log2(4 * worst["H"]))
    print(f"STANDIN worst ratio to the scale: H {worst['H']:.3g} pf {worst['pf']:.3g} f {worst['f']:.3g}; recorded {vt.STANDIN_WORST:g}; "
          f"4 x {max(worst.values()):.3g} rounded up to a power of two = {rule:g}; FACTOR = {vt.FACTOR:g}")
    assert not failures, failures                                     # (-march=native: the figure above belongs to the machine that prints it)


def _controls(e, idx):
    """The two planted defects on the oracle's own output: (name, H)."""
    names = [nm for nm, _ in vt.blocks(e.n)]
    k = int(idx[0])
    q = dict(vt.blocks(e.n))["ORI" if k == 0 else f"q{k - 1}"]       # the quaternion of the track's first pose
    Hq = np.array(e.o_H)
    Hq[0, q] *= 1 + 1e-10
    Hs = np.array(e.o_H)
    Hs[:, vt.SFT] *= 1 + 1e-8
    assert names[2] == "SFT"
    return ("quaternion block of row 0 x (1 + 1e-10)", Hq), ("SFT column x (1 + 1e-8)", Hs)


@pytest.mark.parametrize("name", ["s20_np10", "s20_np21", "m20_np4"])
def test_negative_controls_pass_the_frobenius_bar_and_fail_the_block_bar(name):
    """One quaternion block of one row scaled by 1 + 1e-10, and the time-shift column scaled by 1 + 1e-8, applied to the ORACLE's
    output in the device's place: every track passes the parity tests' _rel < 1e-9, and the case fails the block-wise bar (on how many
    of its tracks is printed: a track whose own rounding error in that block exceeds the planted one cannot show it)."""
    _, _, _, idx, _, _, _ = vt.corpus(name)
    ens = vt.case_ensembles(name)
    for c in (0, 1):
        caught = total = 0
        for b, e in enumerate(ens):
            if not e.ok or e.excluded:
                continue
            what, H = _controls(e, idx[b])[c]
            assert not np.array_equal(H, e.o_H) and _rel(H, e.o_H) < TOL_PARITY
            J = vt.Judge(what)
            J.track(f"{name}[{b}]", e, e.o_pf, H, e.o_f)
            total += 1
            caught += bool(J.failures)
        print(f"CONTROL {name}: {what}: passes _rel < 1e-9 on {total} of {total} tracks, fails the block bar on {caught}")
        assert caught >= 0.9 * total, (name, what, caught, total)


@pytest.mark.parametrize("npose", vt.GATE_POSES)
def test_gate_chi2_scale_and_a_second_binary64_evaluation(oracle, npose):
    """The gate's ensembles (16 tracks x 4 covariances x 2 gate noises): the oracle in the device's place passes judge_gate with a ratio
    of at most 1 and the truth's decision everywhere; a second binary64 evaluation of the statistic -- the stand-in's H and f, S from
    numpy's products, LAPACK's solve -- stays within FACTOR of the scale (measured: 0.88 and 0.41, below the stand-in's Jacobian)."""
    T1, T2, means, idx, feat, vel, y = vt.gate_corpus(npose)
    params, covs = vt.gate_covariances()
    ns, par = params.noiseScale ** 2, vt.params_of({})
    standin = [vt.evaluate("standin", par, means[b], idx[b], T1, T2, feat[b], vel[b]) for b in range(vt.GATE_B)]
    J = vt.Judge(f"oracle in the device's place np={npose}")
    worst = 0.0
    for cov in vt.GATE_COVS:
        for r in vt.GATE_R:
            ens = vt.gate_ensembles(npose, cov, r)
            assert sum(e.ok for e in ens) >= 0.75 * len(ens) and not any(e.excluded for e in ens)
            st = np.array([e.oracle_status for e in ens])
            chi = np.array([e.o_chi2 if e.ok else -1.0 for e in ens])
            gs = np.array([vt.gate_status(e.o_chi2, len(e.f)) if e.ok else 1 for e in ens])
            pf = np.array([e.o_pf if e.ok else np.zeros(3) for e in ens])
            compared, w, wo, _ = vt.judge_gate(J, f"P={cov} r_gate={r:g}", ens, st, gs, chi, pf)
            assert compared == sum(e.ok for e in ens) and w <= 1.0 and w == wo
            for b, e in enumerate(ens):
                if e.ok:
                    H, f = standin[b][4], standin[b][5]
                    v = y[b] - f
                    S = H @ covs[cov][b] @ H.T + np.eye(len(v)) * ((r * r) * ns)
                    worst = max(worst, e.ratio_chi2(ns * (v @ np.linalg.solve(S, v))))
    J.done()
    print(f"STANDIN gate np={npose}: chi2 worst ratio to the scale {worst:.3g} (FACTOR {vt.FACTOR:g})")
    assert worst <= vt.FACTOR


def test_corpus_hash_is_stable_within_a_process():
    """The figure profiles/vu_accuracy/README.md records for the parent's and this tree's double build (equal = bit-identical)."""
    h = vt.corpus_hash()
    print(f"HASH double build over the corpus: {h}")
    assert h == vt.corpus_hash() and len(h) == 64


def test_kernel_summation_order_reproduces_the_device_finding(tmp_path):
    """scripts/vu_sum_order_study.py: the oracle's source with the derivative sums in the kernels' order (plain part through the summed
    linear maps, motion part separate) leaves the bar on the five tracks the device fails on (test_gpu_vu_accuracy.py), the reference's
    order is the oracle to the bit, and the kernels' order with the converging iteration alone in the reference's order is back inside."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("vu_sum_order_study", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                      "scripts", "vu_sum_order_study.py"))
    study = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(study)
    tracks = [(s.split(":")[0], int(s.split(":")[1])) for s in study.FAILING]
    res = {order: [study.ratios(prepare, n, b) for n, b in tracks] for order in (0, 2, 8) for prepare in [study.build(order, str(tmp_path))]}
    for order, rows in res.items():
        print(f"SUM_ORDER {order} ({study.ORDERS[order]}): " + "; ".join(f"{n}[{b}] {r[0]:.3g}" for (n, b), r in zip(tracks, rows)))
    assert all(r[3] and r[0] <= 1.0 for r in res[0])
    assert all(r[0] > vt.FACTOR for r in res[2])
    assert all(r[0] <= vt.FACTOR for r in res[8])
