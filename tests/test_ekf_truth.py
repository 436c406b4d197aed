"""Pins tests/ekf_truth.py (the extended-precision restatement the GPU accuracy tests judge the kernels by) to the CPU oracle, so
that a wrong restatement cannot pass itself off as the truth: on covariances as a running filter holds them -- diagonal from
1e-8 to 1e8, near-singular along "new trail pose = current pose" -- the oracle's binary64 result of every operation must lie
within a scaled distance of the truth that only rounding explains. The bounds are 16 x the worst distance measured with this
file's own cases (recorded next to each); the defect of a wrong restatement is of order 1, of a cancelling algebra 1e-8.
"""
import numpy as np
import pytest

import ekf_truth as tr

# worst scaled distance oracle <-> truth per (operation, regime) over both trail lengths, every snapshot, every case below
MEASURED = {
    ("augment", "a"): 3.68e-16, ("augment", "b"): 3.35e-16, ("augment", "c"): 4.70e-16, ("augment", "d"): 3.97e-16,
    ("augment", "e"): 4.45e-16,
    # the mean in standard deviations: a bias of 1.0 with a deviation of 1e-3 rounds to 1e-13 of it
    ("augment_m", "a"): 3.25e-16, ("augment_m", "b"): 9.48e-14, ("augment_m", "c"): 8.92e-14, ("augment_m", "d"): 6.16e-14,
    ("augment_m", "e"): 9.47e-14,
    # the subtractive update P -= K HP right after the trail has filled (correlation condition ~1e10) loses digits in the
    # reference's own expression; in the steady state it does not
    ("update", "c"): 9.00e-12, ("update", "d"): 1.56e-11, ("update", "e"): 3.92e-16,
    ("update_m", "c"): 1.08e-13, ("update_m", "d"): 1.26e-13, ("update_m", "e"): 1.10e-13,
    ("predict", "a"): 1.63e-15, ("predict", "b"): 8.47e-16, ("predict", "c"): 1.88e-15, ("predict", "d"): 1.30e-15,
    ("predict", "e"): 1.30e-15,
}
MARGIN = 16
CHI2_RTOL = 1e-9                                                      # the suite's bar for the gate statistic (measured: 1.0e-12)


@pytest.fixture(scope="module")
def filters(oracle):
    return {(trail, hyb): tr.realistic_filters(oracle, np.random.default_rng(2024 + hyb), trail=trail, hybrid_map=hyb)
            for trail, hyb in ((20, 0), (5, 0), (20, 15))}


def _cases(filters, regime):
    for (trail, hyb), (params, snaps) in filters.items():
        if not hyb or regime == "e":
            yield trail, params, snaps[regime]


def _check(worst, key):
    print(f"{key}: measured {worst:.2e}, recorded {MEASURED[key]:.2e}, bound {MARGIN * MEASURED[key]:.2e}")
    assert worst <= MARGIN * MEASURED[key], (key, worst)


def test_extended_precision_is_available():
    assert np.finfo(tr.LD).eps < 2e-19


def test_helpers_against_binary64_lapack():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(12, 12))
    S = A @ A.T + 12 * np.eye(12)
    B = rng.normal(size=(12, 5))
    L = tr.chol(S)
    assert np.abs(np.asarray(L, np.float64) - np.linalg.cholesky(S)).max() < 1e-13
    assert np.abs(np.asarray(tr.spd_solve(L, B), np.float64) - np.linalg.solve(S, B)).max() < 1e-13
    assert float(np.abs(L @ L.T - S).max()) < 1e-17
    T = np.diag([4.0, 1e-8, 0.0])
    P = T.copy(); P[0, 1] = P[1, 0] = 2e-4 * 1e-3                   # an error of 1e-3 of sqrt(4 * 1e-8)
    assert tr.scaled_err(P, T) == pytest.approx(1e-3, rel=1e-12) and tr.scaled_err(T, T) == 0.0
    P[2, 2] = 1e-300
    assert tr.scaled_err(P, T) == np.inf                             # an entry the truth holds at exactly zero
    assert tr.scaled_err_m([1, 1e-4, 0], [1, 0, 0], T) == pytest.approx(1.0)
    assert tr.corr_min_eig(np.array([[4.0, 1.0], [1.0, 1.0]])) == pytest.approx(0.5)
    assert len(tr.chi2inv95()) == 201 and tr.chi2inv95()[16] == pytest.approx(26.296227604864232)


def test_snapshots_have_the_regimes_properties(filters):
    """(a) every trail slot still at its 1e8 prior next to 1e-6 variances; (c) the trail just filled, the correlation matrix
    within 1e-8 of singular (trail 20; the 5-pose trail has had less time to correlate: 1e-7); (e) no prior left anywhere."""
    for (trail, hyb), (params, snaps) in filters.items():
        for frame, m, P in snaps["a"]:
            d = np.diag(P)
            assert d.max() / d[d > 0].min() >= 1e10 and d.max() >= 1e8
        for frame, m, P in snaps["c"]:
            assert tr.corr_min_eig(P) <= (1e-8 if trail == 20 else 1e-7), (trail, frame, tr.corr_min_eig(P))
        for frame, m, P in snaps["e"]:
            assert np.diag(P)[:20 + 7 * trail].max() < 1e4
        assert [len(snaps[r]) for r in tr.REGIMES] == [3, 1, 3, 1, 2]


def test_structured_jacobian_support():
    rng = np.random.default_rng(0)
    for nr, l in [s for shapes in tr.UPDATE_SHAPES.values() for s in shapes]:
        H = tr.structured_H(rng, nr, l, (l - 20) // 7 if l < 160 else 20)
        assert not H[:, 3:6].any() and not H[:, 10:19].any()         # velocity and bias columns stay exactly zero
        assert np.abs(H[:, :3]).min() > 0 and np.abs(H[:, 6:10]).min() > 0 and np.abs(H[:, 19]).min() > 0
        assert np.linalg.matrix_rank(H) == min(nr, np.count_nonzero(np.abs(H).sum(0)))


def test_sparse_joseph_form_equals_the_dense_products(filters):
    params, snaps = filters[(20, 0)]
    for regime in ("a", "c", "e"):
        frame, m, P = snaps[regime][0]
        (ms, Ts), (md, Td) = tr.augment(m, P, -1, params), tr.augment(m, P, -1, params, dense=True)
        assert tr.scaled_err(Ts, Td) < 1e-18 and tr.scaled_err_m(ms, md, Td) == 0.0      # measured 2.2e-19


@pytest.mark.parametrize("regime", tr.REGIMES)
def test_oracle_augmentation_lies_within_rounding_of_the_truth(oracle, filters, regime):
    worst = worst_m = 0.0
    for trail, params, snaps in _cases(filters, regime):
        for frame, m, P in snaps:
            for k in (-1, trail - 1, trail - 4):
                mT, T = tr.augment(m, P, k, params)
                o = tr.oracle_filter(oracle, params, m, P)
                o.update_visual_pose_augmentation(k)
                worst, worst_m = max(worst, tr.scaled_err(o.P, T)), max(worst_m, tr.scaled_err_m(o.m, mT, T))
                o.update_undo_augmentation()                                            # a pure shift: exact on both sides
                mU, U = tr.undo_augment(mT, T, params)
                assert tr.scaled_err(o.P, U) <= worst and tr.scaled_err_m(o.m, mU, T) <= worst_m
    _check(worst, ("augment", regime))
    _check(worst_m, ("augment_m", regime))


@pytest.mark.parametrize("regime", tr.UPDATE_REGIMES)
def test_oracle_update_and_gate_lie_within_rounding_of_the_truth(oracle, filters, regime):
    table = tr.chi2inv95()
    worst = worst_m = worst_chi = 0.0
    for trail, params, snaps in _cases(filters, regime):
        if params.hybridMapSize:
            continue
        snaps = tr.filled(snaps, trail)
        for nr, l in tr.UPDATE_SHAPES[trail]:
            for (frame, m, P), (H, v) in zip(snaps, tr.update_inputs(regime, trail, nr, l, len(snaps))):
                assert not H[:, 3:6].any() and not H[:, 10:19].any()
                o = tr.oracle_filter(oracle, params, m, P)
                for scale in (1.0, 40.0):                                               # an inlier and a gross outlier
                    _, _, chi2 = tr.visual_update(m, P, H, scale * v, tr.visual_rd(params), trail, ns=params.noiseScale ** 2)
                    st, co = o.visual_track_outlier_check(H, np.zeros(nr), scale * v, tr.R_VISUAL)
                    assert st == (tr.CHI2 if chi2 > table[nr] else tr.INLIER) == (tr.CHI2 if scale > 1 else tr.INLIER)
                    worst_chi = max(worst_chi, abs(co - chi2) / max(1.0, abs(chi2)))
                mT, T, _ = tr.visual_update(m, P, H, v, tr.visual_rd(params), trail)
                o.update_visual_track(H, np.zeros(nr), v, tr.R_VISUAL)
                worst, worst_m = max(worst, tr.scaled_err(o.P, T)), max(worst_m, tr.scaled_err_m(o.m, mT, T))
    print(f"chi2 relative distance {worst_chi:.2e}")
    assert worst_chi <= CHI2_RTOL
    _check(worst, ("update", regime))
    _check(worst_m, ("update_m", regime))


@pytest.mark.parametrize("regime", tr.REGIMES)
def test_oracle_predict_covariance_lies_within_rounding_of_the_truth(oracle, filters, regime):
    worst = 0.0
    for trail, params, snaps in _cases(filters, regime):
        gyro, acc = tr.predict_inputs(regime, trail, len(snaps))
        for b, (frame, m, P) in enumerate(snaps):
            o, T = tr.predict_truth(oracle, params, m, P, gyro[:, b], acc[:, b])
            worst = max(worst, tr.scaled_err(o.P, T))
    _check(worst, ("predict", regime))
