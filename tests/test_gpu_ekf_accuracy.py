"""Scale-aware accuracy tests of the EKF covariance kernels. The parity tests (test_gpu_ekf.py) judge a covariance by
||P_gpu - P_oracle||_F / ||P_oracle||_F on dense, well-conditioned random matrices; a running filter's covariance has a diagonal
from 1e-8 (accelerometer bias) to 1e8 (a trail slot still at its prior) and is near-singular along "new trail pose = current
pose", and there a Frobenius norm sees the largest entries only. Here every kernel runs on covariances taken from the oracle's
closed loop (tests/ekf_truth.realistic_filters: regimes (a) every trail slot at the 1e8 prior, (b) half-filled trail, (c) the
trail just filled, smallest correlation eigenvalue ~1e-9, (d) the first visual updates, (e) steady state) and is judged by

    scaled_err(P, T) = max_ij |P_ij - T_ij| / sqrt(T_ii T_jj)

against T, the reference's expressions evaluated in extended precision (tests/ekf_truth.py, pinned to the oracle by
test_ekf_truth.py). The device restructures the algebra (unpivoted Cholesky and P -= Y'Y; a rank-14 expansion of the Joseph
form), which is equal in exact arithmetic and need not be equally accurate, so the bar is the reference's own error:

    scaled_err(P_gpu, T) <= max(8 * scaled_err(P_oracle, T), 64 eps)      and the same for the mean (in standard deviations)

8: two correct binary64 evaluations of one formula in different summation orders differ by a small constant (a numpy emulation
of the update measured 1.3 x); the defect these tests exist for -- cancellation of 1e8 against 1e8 to leave 1e-6 -- is 1e6 to
1e8 x. 64 eps: a few dozen roundings of an entry that is at most 1 in this metric, for where the oracle happens to be exact.
Further: corr_min_eig(P_gpu) >= 0.5 corr_min_eig(T) wherever the truth's is >= 1e-10 (by Weyl's inequality an error within
the budget moves it by n x budget ~ 1e-12 at most), P == P' bitwise after the augmentation, no variance grown by a measurement.
Every comparison prints the device's and the oracle's scaled error and the Frobenius figure the parity tests would have seen.
"""
import numpy as np
import pytest

import ekf_truth as tr
import test_gpu_ekf as E
from hybvio_amd import capi

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 8.0, 64 * tr.EPS64
CASES = [(r, t, 0) for r in tr.REGIMES for t in (20, 5)] + [("e", 20, 15)]      # (regime, trail, hybridMapSize): n = 160, 55, 205
UPDATE_CASES = [(r, t, nr, l) for r in tr.UPDATE_REGIMES for t in (20, 5) for nr, l in tr.UPDATE_SHAPES[t]]


@pytest.fixture(scope="module")
def filters(oracle):
    """The oracle's closed loops, run once: {(trail, hybridMapSize): (params, {regime: [(frame, m, P)]})}."""
    return {(trail, hyb): tr.realistic_filters(oracle, np.random.default_rng(2024 + hyb), trail=trail, hybrid_map=hyb)
            for trail, hyb in ((20, 0), (5, 0), (20, 15))}


@pytest.fixture()
def ctx():
    c = capi.Context(width=64, height=64, levels=1, pool_size=1)
    yield c
    c.close()


def budget(oracle_err):
    return max(FACTOR * oracle_err, FLOOR)


class Judge:
    """Prints every comparison before anything is asserted, then fails with the whole list."""

    def __init__(self, what):
        self.what, self.failures = what, []

    def fail_if(self, cond, msg):
        if cond:
            self.failures.append(msg)

    def compare(self, case, Pg, Po, T, mg=None, mo=None, mT=None, definite=True):
        eg, eo, fg = tr.scaled_err(Pg, T), tr.scaled_err(Po, T), tr.frob_err(Pg, T)
        line = f"ACC {self.what} {case}: P scaled error device {eg:.2e} oracle {eo:.2e}; Frobenius device {fg:.2e}"
        self.fail_if(not eg <= budget(eo), f"{case}: P scaled error {eg:.2e} > budget {budget(eo):.2e} (oracle {eo:.2e})")
        if mg is not None:
            gm, om = tr.scaled_err_m(mg, mT, T), tr.scaled_err_m(mo, mT, T)
            line += f"; m device {gm:.2e} oracle {om:.2e}"
            self.fail_if(not gm <= budget(om), f"{case}: m scaled error {gm:.2e} > budget {budget(om):.2e} (oracle {om:.2e})")
        if definite:
            lt = tr.corr_min_eig(T)
            if lt >= 1e-10:
                lg = tr.corr_min_eig(Pg)
                line += f"; corr min eig device {lg:.3e} truth {lt:.3e}"
                self.fail_if(not lg >= 0.5 * lt, f"{case}: smallest correlation eigenvalue {lg:.3e} < half the truth's {lt:.3e}")
        print(line)

    def done(self):
        assert not self.failures, f"{self.what}: " + " | ".join(self.failures)


def load(oracle, ctx, params, snaps):
    """One EkfBatch holding the snapshots, with the oracle's parameters."""
    po, pg = E.same_params(oracle, cameraTrailLength=params.cameraTrailLength, hybridMapSize=params.hybridMapSize)
    g = capi.EkfBatch(ctx, pg, len(snaps))
    for b, (_, m, P) in enumerate(snaps):
        g.set_state(b, m, P)
    return g


def _knob(ctx, name, value):
    old = ctx.get_knob(name)
    ctx.set_knob(name, value)
    assert ctx.get_knob(name) == value
    return old


@pytest.mark.parametrize("regime,trail,hyb", CASES)
def test_augmentation_accuracy(oracle, ctx, filters, regime, trail, hyb):
    """hv_ekf_augment with k = -1, the last and the fourth-last slot (19 and 16 of the Hanoi pattern at trail 20), the undo shift
    after each, and hv_ekf_symmetrize_augment_dev on an asymmetric covariance with per-filter k."""
    import torch
    params, snaps = filters[(trail, hyb)]
    snaps = snaps[regime]
    B, J = len(snaps), Judge(f"augment regime={regime} trail={trail} n={20 + 7 * trail + 3 * hyb}")
    for k in (-1, trail - 1, trail - 4):
        g = load(oracle, ctx, params, snaps)
        g.augment([k] * B)
        after = [g.get_state(b) for b in range(B)]
        g.undo_augment()
        for b, (frame, m, P) in enumerate(snaps):
            mT, T = tr.augment(m, P, k, params)
            o = tr.oracle_filter(oracle, params, m, P)
            o.update_visual_pose_augmentation(k)
            mg, Pg = after[b]
            J.compare(f"k={k} frame={frame}", Pg, o.P, T, mg, o.m, mT)
            J.fail_if(not np.array_equal(Pg, Pg.T), f"k={k} frame={frame}: P != P' after the augmentation")
            o.update_undo_augmentation()
            mU, U = tr.undo_augment(mT, T, params)
            mg, Pg = g.get_state(b)
            J.compare(f"k={k} frame={frame} undo", Pg, o.P, U, mg, o.m, mU, definite=False)     # (a zero slot: no correlation matrix)
        g.close()
    if hyb:                                                             # (the device-pointer entries decline states above 64 KB of LDS)
        return J.done()
    rng = np.random.default_rng([ord(regime), trail, hyb])
    ks = np.array([(trail - 1, trail - 4, -1)[b % 3] for b in range(B)], np.int32)
    g = load(oracle, ctx, params, snaps)
    sym = []
    for b, (frame, m, P) in enumerate(snaps):
        Pa = P * (1 + 1e-13 * np.triu(rng.normal(size=P.shape), 1))     # asymmetric in the last three digits, as updates leave it
        assert not np.array_equal(Pa, Pa.T)
        g.set_state(b, m, Pa)
        sym.append(0.5 * (Pa + Pa.T))                                   # what the kernel reads, bit for bit
    kd = torch.from_numpy(ks).cuda()
    g.symmetrize_augment_dev(kd.data_ptr(), 0)
    ctx.synchronize()
    for b, (frame, m, P) in enumerate(snaps):
        mT, T = tr.augment(m, sym[b], int(ks[b]), params)
        o = tr.oracle_filter(oracle, params, m, sym[b])
        o.update_visual_pose_augmentation(int(ks[b]))
        mg, Pg = g.get_state(b)
        J.compare(f"symmetrize_augment_dev k={ks[b]} frame={frame}", Pg, o.P, T, mg, o.m, mT)
        J.fail_if(not np.array_equal(Pg, Pg.T), f"symmetrize_augment_dev frame={frame}: P != P'")
    g.close()
    J.done()


def _device_inputs(g, H, v):
    import torch
    g.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    dH = torch.from_numpy(np.ascontiguousarray(np.transpose(H, (0, 2, 1)))).cuda()      # column-major per filter
    return dH, torch.from_numpy(np.ascontiguousarray(v)).cuda()


@pytest.mark.parametrize("regime,trail,nr,l", UPDATE_CASES)
def test_visual_gate_and_update_accuracy(oracle, ctx, filters, regime, trail, nr, l):
    """Structured H (velocity and bias columns exactly zero) at 16 x 76, 40 x 160 and 84 x 160 -- the one- and three-row-tile
    builds and the global-workspace kernel -- and 16 x 55 on the 5-pose trail. The gate on the host-pointer path, on
    hv_ekf_visual_dev mode 0 and under both forced gate kernels: chi2 within 1e-9 relative of the truth, the truth's status, the
    filter untouched. The update on the host-pointer path and fused with the gate (mode 2): the budget, no variance grown."""
    import torch
    params, snaps = filters[(trail, 0)]
    snaps = tr.filled(snaps[regime], trail)
    B, J = len(snaps), Judge(f"update regime={regime} trail={trail} H={nr}x{l}")
    inputs = tr.update_inputs(regime, trail, nr, l, B)
    H, v = np.stack([h for h, _ in inputs]), np.stack([x for _, x in inputs])
    assert not H[:, :, 3:6].any() and not H[:, :, 10:19].any()
    rd, ns, table = tr.visual_rd(params), params.noiseScale ** 2, tr.chi2inv95()
    g = load(oracle, ctx, params, snaps)
    for scale in (1.0, 40.0):                                           # inliers, then gross outliers
        chi_t = np.array([tr.visual_update(m, P, H[b], scale * v[b], rd, trail, ns=ns)[2] for b, (_, m, P) in enumerate(snaps)])
        st_t = np.where(chi_t > table[nr], tr.CHI2, tr.INLIER)
        assert (st_t == (tr.CHI2 if scale > 1 else tr.INLIER)).all()
        gates = [("host gate", lambda: g.visual_gate(H, scale * v, tr.R_VISUAL), None),
                 ("host gate, ekf_gate_kmode 1", lambda: g.visual_gate(H, scale * v, tr.R_VISUAL), ("ekf_gate_kmode", 1)),
                 ("visual_dev mode 0", lambda: E._gate_dev(g, H, scale * v, tr.R_VISUAL), None)]
        if E._stream_gate_serves(nr, l):
            gates.append(("visual_dev mode 0, ekf_stream_gate 1", lambda: E._gate_dev(g, H, scale * v, tr.R_VISUAL), ("ekf_stream_gate", 1)))
        for name, run, knob in gates:
            old = _knob(ctx, *knob) if knob else None
            chi2, st = run()
            if knob:
                _knob(ctx, knob[0], old)
            rel = np.abs(chi2 - chi_t) / np.maximum(1.0, np.abs(chi_t))
            print(f"ACC gate regime={regime} trail={trail} H={nr}x{l} {name} scale={scale:g}: chi2 relative error {rel.max():.2e}, status {[int(x) for x in st]}")
            J.fail_if(not (rel <= 1e-9).all(), f"{name} scale={scale:g}: chi2 {chi2} vs truth {chi_t}")
            J.fail_if(not np.array_equal(st, st_t), f"{name} scale={scale:g}: status {st} vs truth {st_t}")
    for b, (_, m, P) in enumerate(snaps):
        mg, Pg = g.get_state(b)
        J.fail_if(not (np.array_equal(mg, m) and np.array_equal(Pg, P)), f"filter {b} changed by a gate")
    truth = [tr.visual_update(m, P, H[b], v[b], rd, trail) for b, (_, m, P) in enumerate(snaps)]
    orc_ = []
    for b, (_, m, P) in enumerate(snaps):
        o = tr.oracle_filter(oracle, params, m, P)
        o.update_visual_track(H[b], np.zeros(nr), v[b], tr.R_VISUAL)
        orc_.append(o)
    g.visual_update(H, v, tr.R_VISUAL)
    g2 = load(oracle, ctx, params, snaps)
    dH, dv = _device_inputs(g2, H, v)
    chi2 = torch.zeros(B, dtype=torch.float64, device="cuda")
    st = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    g2.visual_dev(nr, l, dH.data_ptr(), dv.data_ptr(), tr.R_VISUAL, 2, chi2.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    J.fail_if(st.cpu().tolist() != [tr.INLIER] * B, f"mode 2 status {st.cpu().tolist()}")
    for name, gg in (("visual_update", g), ("visual_dev mode 2", g2)):
        for b, (frame, m, P) in enumerate(snaps):
            mg, Pg = gg.get_state(b)
            J.compare(f"{name} frame={frame}", Pg, orc_[b].P, truth[b][1], mg, orc_[b].m, truth[b][0])
            growth = float((np.diag(Pg) / np.diag(P)).max() - 1)
            J.fail_if(not growth <= FLOOR, f"{name} frame={frame}: a variance grew by {growth:.2e} relative")
    g.close(); g2.close()
    J.done()


@pytest.mark.parametrize("regime,trail", [(r, t) for r in tr.REGIMES for t in (20, 5)])
def test_predict_covariance_accuracy(oracle, ctx, filters, regime, trail):
    """Five samples through hv_ekf_predict (one launch each) and through hv_ekf_predict_n_dev in both kernel forms
    (ekf_predict_chain 2: the chain kernel; 0: nine stages per sample). The truth is F P F' + Qd per sample with the oracle's own
    dydx and process-noise term (ekf_truth.predict_cov), so no second restatement of the process model is involved."""
    import torch
    params, snaps = filters[(trail, 0)]
    snaps = snaps[regime]
    B, nS, dt = len(snaps), 5, 0.005
    gyro, acc = tr.predict_inputs(regime, trail, B, nS)
    ref = [tr.predict_truth(oracle, params, m, P, gyro[:, b], acc[:, b], dt) for b, (_, m, P) in enumerate(snaps)]
    J = Judge(f"predict regime={regime} trail={trail}")
    results = {}
    g = load(oracle, ctx, params, snaps)
    for s in range(nS):
        g.predict(np.full(B, dt), gyro[s], acc[s])
    results["predict x 5"] = [g.get_state(b) for b in range(B)]
    d_dt, d_gy, d_ac = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (np.full((nS, B), dt), gyro, acc))
    for form in E.PREDICT_CHAIN_FORMS:
        for b, (_, m, P) in enumerate(snaps):
            g.set_state(b, m, P)
        old = _knob(ctx, "ekf_predict_chain", form)
        g.predict_n_dev(nS, d_dt.data_ptr(), d_gy.data_ptr(), d_ac.data_ptr())
        ctx.synchronize()
        _knob(ctx, "ekf_predict_chain", old)
        results[f"predict_n_dev, ekf_predict_chain {form}"] = [g.get_state(b) for b in range(B)]
    for name, states in results.items():
        for b, (frame, m, P) in enumerate(snaps):
            J.compare(f"{name} frame={frame}", states[b][1], ref[b][0].P, ref[b][1])
    g.close()
    J.done()


def test_closed_loop_40_frames_against_the_carried_truth(oracle, ctx):
    """40 frames from the constructor state: 10 predicts, from frame 24 four gated structured visual updates and a symmetrisation,
    the augmentation with the Hanoi discard pattern. The device, the oracle and the extended-precision covariance are carried side
    by side on the same inputs; the oracle and the truth apply the updates the DEVICE's gate accepted. At the end the device's
    scaled error must be within 8 x the oracle's. (dt = 1/256: the oracle's time stamps then accumulate without rounding, so all
    three see the same dt.)"""
    trail, dt = 20, 1.0 / 256
    rng = np.random.default_rng(40)
    po, pg = E.same_params(oracle)
    o, g = oracle.Ekf(po), capi.EkfBatch(ctx, pg, 1)
    acc0 = np.array([0.2, -0.1, 9.8])
    o.initialize_orientation(acc0)
    g.set_state(0, o.m.copy(), o.P.copy())
    o.set_first_sample_time(0.0)
    T = np.asarray(o.P.copy(), tr.LD)
    rd = tr.visual_rd(po)
    step = applied = rejected = 0
    for frame in range(40):
        for _ in range(10):
            gy, ac = tr.closed_loop_inputs(rng, acc0)
            _, F, Qd = tr.oracle_predict_terms(oracle, po, o.m.copy(), step * dt, (step + 1) * dt, gy, ac)
            step += 1
            o.predict(step * dt, gy, ac)
            assert np.array_equal(F, o.dydx)
            g.predict(dt, gy, ac)
            T = tr.predict_cov(T, F, Qd)
        if frame >= trail + 4:
            for _ in range(4):
                poses = int(rng.integers(4, 11))
                nr, l = 4 * poses, tr.CAM + tr.POSE * int(rng.integers(poses, trail + 1))
                H = tr.structured_H(rng, nr, l, trail)
                v = rng.normal(size=nr) * (0.5 if rng.random() < 0.25 else 0.02)
                if g.visual_gate(H, v, tr.R_VISUAL)[1][0] == tr.INLIER:
                    g.visual_update(H, v, tr.R_VISUAL)
                    o.update_visual_track(H, np.zeros(nr), v, tr.R_VISUAL)
                    T = tr.visual_update(o.m, T, H, v, rd, trail)[1]
                    applied += 1
                else:
                    rejected += 1
            g.symmetrize(); o.maintain_psd()
            T = (T + T.T) / 2
        k = tr.discard_index(frame, trail)
        T = tr.augment(o.m, T, k, po)[1]
        g.augment([k]); o.update_visual_pose_augmentation(k)
    assert applied >= 10 and rejected >= 3, (applied, rejected)
    J = Judge(f"closed loop 40 frames ({applied} updates, {rejected} rejected)")
    mg, Pg = g.get_state(0)
    J.compare("end", Pg, o.P, T)
    print(f"    mean: ||m_gpu - m_oracle|| / ||m_oracle|| = {E.rel(mg, o.m):.2e}")
    J.done()
