"""CPU tests of the EKF oracle (oracle/ekf_oracle.c).

Part 1 re-expresses the reference's own EKF tests (test/ekf.cpp, test/util.cpp) against the
oracle using the reference's fixture DATA (tests/golden/ekf_reference_fixtures.npz, extracted by
tests/golden/make_ekf_fixtures.py). Part 2 cross-checks every covariance operation against an
independent numpy/scipy f64 implementation (scipy.linalg.expm, np.linalg.solve, plain @) because
the reference holds no golden posterior (m, P) for predict / updates / augmentation.
"""
import os
import re

import numpy as np
import pytest
import scipy.linalg

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ekf_reference_fixtures.npz")
POS, VEL, ORI, BGA, BAA, BAT, SFT, CAM = 0, 3, 6, 10, 13, 16, 19, 20


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLD)


# ---------------------------------------------------------------------------------------------
# Part 1: the reference's tests
# ---------------------------------------------------------------------------------------------

def test_chi_squared_innovation(oracle, fx):
    """test/ekf.cpp:19-71 -- t = v' * (M \\ v) via LDLT equals Matlab's 1.7626 (+- 0.1)."""
    t = oracle.ldlt_quadratic_form(fx["chi2_M"], fx["chi2_v"])
    assert abs(t - float(fx["chi2_matlab"])) < 1e-1
    assert abs(t - fx["chi2_v"] @ np.linalg.solve(fx["chi2_M"], fx["chi2_v"])) < 1e-9


def _der_check(x0, numeric, analytic, h=1e-7):
    """test/helpers.cpp:34-63 -- forward differences vs analytic Jacobian."""
    f0 = numeric(x0)
    D = np.zeros((len(f0), len(x0)))
    for i in range(len(x0)):
        x = x0.copy()
        x[i] += h
        D[:, i] = (numeric(x) - f0) / h
    return D - analytic(x0)


def test_der_predict(oracle, fx):
    """test/ekf.cpp:73-117 -- dydx of predict() vs numeric derivative, max abs diff < 1e-3."""
    poses, gyro, acc = fx["poses"], fx["gyro"], fx["acc"]
    m = np.zeros(20 + 20 * 7)
    m[POS:POS + 3] = poses[0:3]
    m[ORI:ORI + 4] = poses[3:7]
    t = dt = 0.01
    e0 = oracle.Ekf(oracle.ekf_default_params(cameraTrailLength=5, hybridMapSize=0))
    e0.set_first_sample_time(t)

    def run(x):
        e = e0.clone()
        mm = e.m.copy()
        mm[:20] = x
        e.set_state(mm)
        e.predict(t + dt, gyro, acc)
        return e

    D = _der_check(m[:20].copy(), lambda x: run(x).m[:20].copy(), lambda x: run(x).dydx.copy())
    assert np.abs(D).max() < 1e-3


def test_transform_to_round_trip(oracle, fx):
    """test/ekf.cpp:119-145 -- transformTo to a target pose and back on the 55-dim fixtures."""
    P0, m0 = fx["P55"], fx["m55"]
    o = oracle.Ekf(oracle.ekf_default_params(cameraTrailLength=5, hybridMapSize=0))
    assert o.n == 55
    o.set_state(m0)
    o.set_cov(P0)
    A = 2
    pos0 = o.m[CAM + 7 * A: CAM + 7 * A + 3].copy()
    rot0 = o.m[CAM + 7 * A + 3: CAM + 7 * A + 7].copy()
    to_pos, to_rot = np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0, 0.0])
    o.transform_to(to_pos, to_rot, A)
    assert np.linalg.norm(o.m[CAM + 7 * A: CAM + 7 * A + 3] - to_pos) < 1e-6
    assert np.linalg.norm(o.m[CAM + 7 * A + 3: CAM + 7 * A + 7] - to_rot) < 1e-6
    o.transform_to(pos0, rot0, A)
    assert np.linalg.norm(o.m - m0) < 1e-3
    assert np.linalg.norm(o.P - P0) < 1e-3


def test_quat2rmat_goldens(oracle, fx):
    """test/util.cpp:9-60 -- Matlab goldens, sum |diff| < 1e-5."""
    R, dR = oracle.quat2rmat_d(fx["q"])
    assert np.abs(R - fx["rmat_e"]).sum() < 1e-5
    for k in range(4):
        assert np.abs(dR[k] - fx["dR_e"][k]).sum() < 1e-5


def test_chi2_table_matches_reference_constants():
    """The generated chi2inv95 table equals the reference's (src/odometry/util.hpp:23), stored as
    tests/golden/chi2inv95_reference.npy by tests/golden/make_chi2_fixture.py."""
    vals = np.load(os.path.join(os.path.dirname(__file__), "golden", "chi2inv95_reference.npy")).tolist()
    here = open(os.path.join(os.path.dirname(__file__), "..", "oracle", "chi2inv95.h")).read()
    body = re.search(r"#define HV_CHI2INV95_VALUES(.*?)\nstatic", here, re.S).group(1).replace("\\", " ")
    mine = [float(x) for x in body.split(",")]
    assert len(mine) == len(vals) == 201
    np.testing.assert_allclose(mine, vals, rtol=1e-13)
    prod = open(os.path.join(os.path.dirname(__file__), "..", "hybvio_amd", "csrc", "chi2inv95.h")).read()
    assert prod == here


# ---------------------------------------------------------------------------------------------
# Part 2: independent numpy/scipy implementation
# ---------------------------------------------------------------------------------------------

def np_quat2rmat(q):
    w, x, y, z = q
    return np.array([[w*w+x*x-y*y-z*z, 2*x*y-2*w*z, 2*x*z+2*w*y],
                     [2*x*y+2*w*z, w*w-x*x+y*y-z*z, 2*y*z-2*w*x],
                     [2*x*z-2*w*y, 2*y*z+2*w*x, w*w-x*x-y*y+z*z]])


def np_predict(m, P, Q, dt, xg, xa, par):
    """Mean + covariance of ekf.cpp:320-514 with a NUMERIC Jacobian-free covariance check:
    returns (m_new, F, L) where F, L come from central differences of the mean map."""
    ns = par.noiseScale ** 2

    def f(state, noise):
        s = state.copy()
        ea, eg = noise[0:3], noise[3:6]
        w = xg - s[BGA:BGA + 3] + eg
        Om = np.array([[0, -w[0], -w[1], -w[2]], [w[0], 0, -w[2], w[1]], [w[1], w[2], 0, -w[0]], [w[2], -w[1], w[0], 0]])
        A = scipy.linalg.expm(-dt / 2 * Om)
        qn = A @ s[ORI:ORI + 4]
        R = np_quat2rmat(qn)
        out = s.copy()
        out[POS:POS + 3] = s[POS:POS + 3] + s[VEL:VEL + 3] * dt
        out[VEL:VEL + 3] = s[VEL:VEL + 3] + (R.T @ (s[BAT:BAT + 3] * xa - s[BAA:BAA + 3] + ea) + np.array([0, 0, -par.gravity])) * dt
        out[ORI:ORI + 4] = qn
        out[BAA:BAA + 3] = s[BAA:BAA + 3] * np.exp(-dt * par.noiseProcessBAARev) + noise[9:12]
        out[BGA:BGA + 3] = s[BGA:BGA + 3] + noise[6:9]
        return out

    return f(m[:20], np.zeros(12)), f


def _random_spd(rng, n, scale=1.0):
    A = rng.normal(size=(n, n))
    return scale * (A @ A.T / n + 0.1 * np.eye(n))


def _random_filter(oracle, rng, trail=20):
    e = oracle.Ekf(oracle.ekf_default_params(cameraTrailLength=trail))
    n = e.n
    m = rng.normal(size=n)
    m[ORI:ORI + 4] /= np.linalg.norm(m[ORI:ORI + 4])
    m[BAT:BAT + 3] = 1 + 0.01 * rng.normal(size=3)
    for c in range(trail):
        m[CAM + 7 * c + 3: CAM + 7 * c + 7] /= np.linalg.norm(m[CAM + 7 * c + 3: CAM + 7 * c + 7])
    e.set_state(m)
    e.set_cov(_random_spd(rng, n, 1e2))
    return e


def test_predict_mean_and_covariance_vs_numpy(oracle):
    rng = np.random.default_rng(0)
    e = _random_filter(oracle, rng)
    par = e.params
    e.set_first_sample_time(1.0)
    m0, P0 = e.m.copy(), e.P.copy()
    xg, xa, dt = np.array([0.19, -0.31, -0.03]), np.array([0.18, 7.46, 2.25]), 0.005
    e.predict(1.0 + dt, xg, xa)
    m1, f = np_predict(m0, P0, None, dt, xg, xa, par)
    np.testing.assert_allclose(e.m[:20], m1, rtol=0, atol=1e-12)          # closed-form exp == expm
    np.testing.assert_array_equal(e.m[20:], m0[20:])
    # covariance: the filter's own F (dydx) and L must reproduce its P, and F must be the Jacobian
    F = e.dydx.copy()
    h = 1e-6
    Fnum = np.stack([(f(m0[:20] + h * np.eye(20)[i], np.zeros(12)) - f(m0[:20] - h * np.eye(20)[i], np.zeros(12))) / (2 * h)
                     for i in range(20)], 1)
    # Upstream's analytic Jacobian is knowingly approximate in the gyro-driven entries (ekf.cpp:478-483:
    # "A is multiplied twice"; d exp(S(w)) q / dw is taken as A dS q, exact only to O(dt^2)) and keeps
    # identity for the BAA block although the mean reverts by exp(-dt*rev) (ekf.cpp:450-455). The
    # reference test der_predict accepts 1e-3; the exact entries agree to 1e-9 and the rest to 1e-4.
    exact = np.ones((20, 20), bool)
    exact[VEL:VEL + 3, BGA:BGA + 3] = False
    exact[ORI:ORI + 4, BGA:BGA + 3] = False
    exact[BAA:BAA + 3, BAA:BAA + 3] = False
    assert np.allclose(np.diag(Fnum)[BAA:BAA + 3], np.exp(-dt * par.noiseProcessBAARev))
    assert np.abs((F - Fnum)[exact]).max() < 1e-8
    assert np.abs(F - Fnum).max() < 1e-3
    Q = e.Q.copy()
    Lnum = np.stack([(f(m0[:20], h * np.eye(12)[i]) - f(m0[:20], -h * np.eye(12)[i])) / (2 * h) for i in range(12)], 1)
    LQL = e.P[:20, :20] - F @ P0[:20, :20] @ F.T                           # what the filter added as L Q L'
    assert np.allclose(LQL, LQL.T, atol=1e-6 * np.abs(P0).max())
    ref = Lnum @ Q @ Lnum.T
    assert np.abs(LQL - ref).max() <= 1e-3 * np.abs(ref).max() + 1e-9 * np.abs(P0).max()
    np.testing.assert_allclose(e.P[20:, :20], P0[20:, :20] @ F.T, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(e.P[:20, 20:], F @ P0[:20, 20:], rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(e.P[20:, 20:], P0[20:, 20:])


def test_predict_time_bookkeeping(oracle):
    e = oracle.Ekf()
    m0 = e.m.copy()
    e.predict(5.0, np.zeros(3), np.array([0, 0, 9.819]))      # first sample only latches the time
    np.testing.assert_array_equal(e.m, m0)
    e.predict(5.0, np.zeros(3), np.array([0, 0, 9.819]))      # dt == 0 -> skipped
    np.testing.assert_array_equal(e.m, m0)
    e.predict(5.01, np.array([0.1, 0.0, 0.0]), np.array([0.5, 0, 9.819]))
    assert abs(e.platform_time() - 5.01) < 1e-12 and not np.array_equal(e.m, m0)


def _np_update(m, P, H, v, Rm):
    l = H.shape[1]
    HP = H @ P[:l, :]
    S = HP[:, :l] @ H.T + Rm
    K = np.linalg.solve(S, HP).T
    return m + K @ v, P - K @ HP, S


@pytest.mark.parametrize("nr,l", [(40, 160), (84, 160), (16, 76), (8, 41)])
def test_visual_update_and_gate_vs_numpy(oracle, nr, l):
    rng = np.random.default_rng(nr * 1000 + l)
    e = _random_filter(oracle, rng)
    ns = e.params.noiseScale ** 2
    H = rng.normal(size=(nr, l))
    f, y = rng.normal(size=nr), rng.normal(size=nr)
    y = f + 0.05 * rng.normal(size=nr)
    r = 0.05
    m0, P0 = e.m.copy(), e.P.copy()
    st, chi2 = e.visual_track_outlier_check(H, f, y, r)
    _, _, S = _np_update(m0, P0, H, y - f, r * r * ns * np.eye(nr))
    chi2_np = ns * (y - f) @ np.linalg.solve(S, y - f)
    assert abs(chi2 - chi2_np) <= 1e-9 * max(1.0, abs(chi2_np))
    assert st in (oracle.Ekf.INLIER, oracle.Ekf.CHI2)
    np.testing.assert_array_equal(e.P, P0)                    # the gate must not touch the state
    e.update_visual_track(H, f, y, r)
    m1, P1, _ = _np_update(m0, P0, H, y - f, r * r * ns * np.eye(nr))
    for q0 in [ORI] + [CAM + 7 * c + 3 for c in range(20)]:
        m1[q0:q0 + 4] /= np.linalg.norm(m1[q0:q0 + 4])
    assert np.linalg.norm(e.m - m1) <= 1e-10 * np.linalg.norm(m1)
    assert np.linalg.norm(e.P - P1) <= 1e-10 * np.linalg.norm(P1)
    # RMSE pre-gate and the "no chi2" shortcut (ekf.cpp:796-802)
    assert e.visual_track_outlier_check(H, f, f + 10.0, r, rmse_threshold=1.0)[0] == oracle.Ekf.RMSE
    assert e.visual_track_outlier_check(H, f, y, -1.0)[0] == oracle.Ekf.INLIER


def test_small_updates_vs_numpy(oracle):
    rng = np.random.default_rng(5)
    e = _random_filter(oracle, rng)
    ns = e.params.noiseScale ** 2
    e.set_first_sample_time(10.0)

    def expect(H, y, rd):
        m0, P0 = e.m.copy(), e.P.copy()
        l = H.shape[1]
        m1, P1, _ = _np_update(m0, P0, H, y - H @ m0[:l], rd * np.eye(H.shape[0]))
        m1[ORI:ORI + 4] /= np.linalg.norm(m1[ORI:ORI + 4])
        return m1, P1

    H = np.zeros((3, 6)); H[:, 3:6] = np.eye(3)
    m1, P1 = expect(H, np.zeros(3), 1e-3 * ns)
    e.update_zupt(1e-3)
    np.testing.assert_allclose(e.m, m1, rtol=1e-11, atol=1e-11); np.testing.assert_allclose(e.P, P1, rtol=1e-10, atol=1e-9)
    assert e.was_stationary()
    P_before = e.P.copy(); e.update_zupt(1e-3); np.testing.assert_array_equal(e.P, P_before)   # < 0.25 s rate limit
    H = np.zeros((3, 13)); H[:, 10:13] = np.eye(3)
    xg = np.array([0.01, -0.02, 0.005])
    m1, P1 = expect(H, xg, e.params.rotationZuptR * ns)
    e.update_zrupt(xg)
    np.testing.assert_allclose(e.m, m1, rtol=1e-11, atol=1e-11); np.testing.assert_allclose(e.P, P1, rtol=1e-10, atol=1e-9)
    H = np.zeros((3, 3)); H[:, 0:3] = np.eye(3)
    pos = np.array([1.0, 2.0, 3.0])
    m1, P1 = expect(H, pos, 0.1 * ns)
    e.update_position(pos, 0.1)
    np.testing.assert_allclose(e.m, m1, rtol=1e-11, atol=1e-11); np.testing.assert_allclose(e.P, 0.5 * (P1 + P1.T), rtol=1e-10, atol=1e-9)
    H = np.zeros((1, 3)); H[0, 2] = 1
    m1, P1 = expect(H, np.zeros(1), 0.2 * ns)
    e.update_zero_height(0.2)
    np.testing.assert_allclose(e.m, m1, rtol=1e-11, atol=1e-11); np.testing.assert_allclose(e.P, 0.5 * (P1 + P1.T), rtol=1e-10, atol=1e-9)
    # pseudo velocity (scalar update on the horizontal speed)
    m0, P0 = e.m.copy(), e.P.copy()
    hn = np.linalg.norm(m0[3:5]); Hs = np.zeros(5); Hs[3:5] = m0[3:5] / hn
    HP = Hs @ P0[:5, :]; s = HP[:5] @ Hs + 0.3 * ns; K = HP / s
    m1 = m0 + K * (0.7 - hn); m1[ORI:ORI + 4] /= np.linalg.norm(m1[ORI:ORI + 4])
    e.update_pseudo_velocity(0.7, 0.3)
    np.testing.assert_allclose(e.m, m1, rtol=1e-11, atol=1e-11); np.testing.assert_allclose(e.P, P0 - np.outer(K, HP), rtol=1e-10, atol=1e-9)


@pytest.mark.parametrize("k", [19, 18, 17, 16, 0, -1])
def test_pose_augmentation_vs_numpy(oracle, k):
    rng = np.random.default_rng(100 + k)
    e = _random_filter(oracle, rng)
    n, par = e.n, e.params
    ns = par.noiseScale ** 2
    m0, P0 = e.m.copy(), e.P.copy()
    kk = 19 if k == -1 else k
    A = np.zeros((n, n))
    A[:CAM, :CAM] = np.eye(CAM)
    for i in range(CAM, CAM + kk * 7):
        A[i + 7, i] = 1
    for i in range(CAM + (kk + 1) * 7, n):
        A[i, i] = 1
    Qa = np.zeros((n, n))
    Qa[CAM:CAM + 3, CAM:CAM + 3] = np.eye(3) * par.noiseInitialPosTrail ** 2 * ns
    Qa[CAM + 3:CAM + 7, CAM + 3:CAM + 7] = np.eye(4) * par.noiseInitialOriTrail ** 2 * ns
    m1, P1 = A @ m0, A @ P0 @ A.T + Qa
    H = np.zeros((7, n))
    for i in range(3):
        H[i, POS + i], H[i, CAM + i] = 1, -1
    for i in range(4):
        H[3 + i, ORI + i], H[3 + i, CAM + 3 + i] = 1, -1
    Rm = np.eye(7) * par.augmentR * ns
    S = H @ P1 @ H.T + Rm
    K = np.linalg.solve(S, H @ P1).T
    m2 = m1 + K @ (-H @ m1)
    T = np.eye(n) - K @ H
    P2 = T @ P1 @ T.T + K @ Rm @ K.T
    P2 = 0.5 * (P2 + P2.T)
    for q0 in [ORI] + [CAM + 7 * c + 3 for c in range(20)]:
        nn = np.linalg.norm(m2[q0:q0 + 4])
        if nn > 0:
            m2[q0:q0 + 4] /= nn
    e.update_visual_pose_augmentation(k)
    assert np.linalg.norm(e.m - m2) <= 1e-9 * np.linalg.norm(m2)
    assert np.linalg.norm(e.P - P2) <= 1e-9 * np.linalg.norm(P2)
    np.testing.assert_allclose(e.m[CAM:CAM + 7], e.m[[0, 1, 2, 6, 7, 8, 9]], atol=1e-6)   # slot 0 clones the current pose
    assert e.pose_count() == 2
    # undo: drops slot 0 again, shifting the trail back
    m3, P3 = e.m.copy(), e.P.copy()
    e.update_undo_augmentation()
    U = np.zeros((n, n)); U[:CAM, :CAM] = np.eye(CAM)
    for i in range(CAM, n - 7):
        U[i, i + 7] = 1
    np.testing.assert_allclose(e.m, U @ m3, rtol=0, atol=0)
    np.testing.assert_allclose(e.P, U @ P3 @ U.T, rtol=0, atol=0)
    assert e.pose_count() == 1


def test_augment_times_ring(oracle):
    e = oracle.Ekf(oracle.ekf_default_params(cameraTrailLength=3))
    e.set_first_sample_time(1.0)
    e.initialize_orientation(np.array([0.1, 0.2, 9.8]))
    for i in range(6):
        e.predict(1.0 + 0.1 * (i + 1), np.zeros(3), np.array([0.0, 0.0, 9.819]))
        e.update_visual_pose_augmentation(-1)
        assert e.pose_count() == min(i + 1, 3) + 1
        assert abs(e.history_time(0) - e.platform_time()) < 1e-12          # newest slot = now
    assert abs(e.history_time(2) - (e.platform_time() - 0.2)) < 1e-9


def test_housekeeping_ops(oracle):
    rng = np.random.default_rng(9)
    e = _random_filter(oracle, rng, trail=4)
    n = e.n
    P0 = e.P.copy() + rng.normal(size=(n, n)) * 1e-3
    e.set_cov(P0)
    e.maintain_psd()
    np.testing.assert_allclose(e.P, 0.5 * (P0 + P0.T), rtol=0, atol=0)
    m0 = e.m.copy()
    e.translate_to(np.array([5.0, 6.0, 7.0]))
    d = np.array([5.0, 6.0, 7.0]) - m0[:3]
    np.testing.assert_allclose(e.m[:3], [5, 6, 7])
    for c in range(4):
        np.testing.assert_allclose(e.m[CAM + 7 * c: CAM + 7 * c + 3], m0[CAM + 7 * c: CAM + 7 * c + 3] + d)
    e.lock_biases()
    assert not e.P[BGA:BGA + 9, :].any() and not e.P[:, BGA:BGA + 9].any()
    mean, cov = e.get_inertial_state()
    np.testing.assert_array_equal(mean, e.m[:20]); np.testing.assert_array_equal(cov, e.P[:20, :20])
    e2 = _random_filter(oracle, rng, trail=4)
    e2.set_inertial_state(mean, cov)
    np.testing.assert_array_equal(e2.m[:20], mean); np.testing.assert_array_equal(e2.P[:20, :20], cov)
    assert e2.pose_count() == 1
    # conditionOnLastPose == Schur complement on the last 7 states
    e3 = _random_filter(oracle, rng, trail=4)
    P = e3.P.copy(); mm = n - 7
    schur = P[:mm, :mm] - P[:mm, mm:] @ np.linalg.solve(P[mm:, mm:], P[mm:, :mm])
    e3.condition_on_last_pose()
    np.testing.assert_allclose(e3.P[:mm, :mm], schur, rtol=1e-10, atol=1e-9)
    assert not e3.P[:mm, mm:].any() and np.allclose(e3.P[mm:, mm:], 1e6 * np.eye(7))
    # initializeOrientation: rotates -gravity onto the measured acceleration, yaw component fixed
    e4 = oracle.Ekf()
    xa = np.array([0.3, -0.2, 9.7])
    e4.initialize_orientation(xa)
    q = e4.m[ORI:ORI + 4]
    assert abs(np.linalg.norm(q) - 1) < 1e-12 and q[3] == 0
    R = np_quat2rmat(q)
    np.testing.assert_allclose(R @ np.array([0, 0, 1.0]), xa / np.linalg.norm(xa), atol=1e-12)
    ns = e4.params.noiseScale ** 2
    np.testing.assert_allclose(np.diag(e4.P[ORI:ORI + 4, ORI:ORI + 4]), np.array([1, 1, 1, 0]) * e4.params.noiseInitialOri ** 2 * ns)
