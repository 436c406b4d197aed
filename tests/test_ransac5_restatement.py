"""CPU checks of tests/ransac5_restatement.py, the numpy statement of the five-point RANSAC and the hybrid selection that the
device kernel (hybvio_amd/csrc/ransac5.hip) is compared with."""
import math

import numpy as np
import pytest

import ransac5_restatement as R


def _minimal(rng, H):
    X = [np.zeros((H, 5)) for _ in range(4)]
    truth = []
    for h in range(H):
        Rm = R.rotation(rng.normal(size=3) * 0.2)
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        P = np.c_[rng.uniform(-1, 1, (5, 2)), rng.uniform(3, 8, 5)]
        Q = P @ Rm.T + t
        X[0][h], X[1][h], X[2][h], X[3][h] = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2], Q[:, 0] / Q[:, 2], Q[:, 1] / Q[:, 2]
        truth.append(R.essential_truth(Rm, t))
    return X, truth


def test_minimal_problems_return_the_true_essential_matrix():
    X, truth = _minimal(np.random.default_rng(0), 300)
    E, V, _ = R.essential_kernel(*X)
    best = []
    for h in range(300):
        assert V[h].any()
        best.append(min(np.abs(R.canonical(e) - R.canonical(truth[h])).max() for e in E[h][V[h]]))
    best = np.array(best)
    # one model is [t]x R to 1e-8 on (almost) every problem; a rare ill-conditioned draw (two close roots) still within 1e-6
    assert np.median(best) <= 1e-12 and (best <= 1e-8).mean() >= 0.99 and best.max() <= 1e-6, np.sort(best)[-5:]
    # every returned model satisfies the epipolar constraint and the cubic constraints
    for h in range(20):
        for e in E[h][V[h]]:
            Em = e.reshape(3, 3)
            assert abs(np.linalg.det(Em)) < 1e-8
            assert np.abs(2 * Em @ Em.T @ Em - np.trace(Em @ Em.T) * Em).max() < 1e-8
            x1 = np.c_[X[0][h], X[1][h], np.ones(5)]
            x2 = np.c_[X[2][h], X[3][h], np.ones(5)]
            assert np.abs(np.einsum("ij,jk,ik->i", x2, Em, x1)).max() < 1e-9


def test_solve_poly_finds_known_roots():
    rng = np.random.default_rng(1)
    roots = [np.sort(rng.uniform(-3, 3, 10)) for _ in range(8)]
    roots.append(np.array([1, 2, 3, -1, -2, 0.5, 0.25, 4, -4, 1.5]))
    c = np.stack([np.polynomial.polynomial.polyfromroots(r) * 0.7 for r in roots])
    re, im, n, _ = R.solve_poly(c)
    for k, r in enumerate(roots):
        assert n[k] == 10
        assert np.abs(im[k]).max() < 1e-8
        assert np.allclose(np.sort(re[k]), np.sort(r), atol=1e-8)
    # complex pair + trimmed leading coefficient: x^2 + 1 (degree 2 after dropping zeros)
    c2 = np.zeros((1, 11)); c2[0, 0] = 1; c2[0, 2] = 1
    re, im, n, _ = R.solve_poly(c2)
    assert n[0] == 2 and np.allclose(sorted(im[0, :2]), [-1, 1]) and np.allclose(re[0, :2], 0, atol=1e-12)


@pytest.mark.parametrize("ep,niters,want", [
    (0.0, 75, 0),      # every point an inlier: 1 - (1 - 0)^5 = 0 < DBL_MIN
    (0.1, 75, 8),      # log(0.001) / log(1 - 0.9^5) = 7.74
    (0.2, 75, 17),     # 17.39
    (0.3, 75, 38),     # 37.54
    (0.3, 30, 30),     # capped by the current niters
    (0.5, 75, 75),     # 217.6 > 75
    (1.0, 75, 75),     # log(1) = 0: denom >= 0
])
def test_update_num_iters(ep, niters, want):
    assert R.update_num_iters(0.999, ep, 5, niters) == want


def test_rng_subsets_are_distinct_and_deterministic():
    a, b = R.rng_subsets(6, 75), R.rng_subsets(6, 75)
    assert np.array_equal(a, b) and a.min() >= 0 and a.max() < 6
    assert all(len(set(r)) == 5 for r in a.tolist())
    assert not np.array_equal(R.rng_subsets(200, 5), R.rng_subsets(201, 5))


@pytest.mark.parametrize("case", [
    # n, r2_done, r2, r5_done, r5, use_r2 -> type
    (100, True, 95, False, 0, True, R.TYPE_R2),        # skip rule: R5 not run
    (100, True, 60, True, 80, False, R.TYPE_R5),       # R5 clearly better
    (100, True, 75, True, 80, False, R.TYPE_R2),       # R2 > 0.9 x R5
    (100, True, 72, True, 80, False, R.TYPE_R5),       # R2 == 0.9 x R5 is not enough
    (100, True, 20, True, 80, False, R.TYPE_R5),       # R2 below the minimum fraction
    (100, True, 50, True, 10, False, R.TYPE_R2),       # R5 below the minimum fraction
    (100, True, 20, True, 10, False, R.TYPE_SKIPPED),  # both below
    (3, True, 3, False, 0, True, R.TYPE_R2),
    (1, False, 0, False, 0, False, R.TYPE_SKIPPED),
    (0, False, 0, False, 0, False, R.TYPE_SKIPPED),
])
def test_hybrid_selection_branches(case):
    n, d2, c2, d5, c5, use2, want = case
    assert R.hybrid_select(n, d2, c2, d5, c5, use2) == want


class _IdCam:
    """A camera whose rays are (x, y, 1) of the pixel / 100 (normalizePixel = pixel / 100); rays with y > 1e4 fail."""

    def pixel_to_ray(self, x, y):
        return y < 1e4, np.array([x / 100.0, y / 100.0, 1.0])


def test_hybrid_pipeline_skipped_clears_every_entry():
    ts = np.array([0, 2, 0, 4], np.int32)
    c = np.zeros((4, 2), np.float32)
    out, typ, cnt, score = R.hybrid_pipeline(ts, c, c, np.zeros(4, np.int32), 0, _IdCam(), _IdCam(), 100.0, 100.0)
    assert typ == R.TYPE_SKIPPED and cnt == 0 and (out == 3).all() and score == 0.0


def test_r2_choice_rewrites_only_tracked_entries():
    ts = np.array([0, 2, 0, 0, 4, 0], np.int32)
    r2 = np.array([0, 9, 3, 0, 9, 0], np.int32)
    c = np.zeros((6, 2), np.float32)
    out, typ, cnt, score = R.hybrid_pipeline(ts, c, c, r2, 4, _IdCam(), _IdCam(), 100.0, 100.0)
    assert typ == R.TYPE_R2 and cnt == 4 and out.tolist() == [0, 2, 3, 0, 4, 0] and score == 1.0


def test_exactly_five_valid_points_keep_the_all_one_mask_and_invalid_points_are_outliers():
    rng = np.random.default_rng(3)
    c1 = rng.uniform(0, 300, (6, 2)).astype(np.float32)
    c2 = c1 + rng.uniform(-40, 40, (6, 2)).astype(np.float32)
    c2[2, 1] = 2e4                                                     # normalizePixel fails: not passed on
    done, st, E, summ, _ = R.do_ransac5(c1, c2, _IdCam(), _IdCam(), 100.0, 100.0)
    assert done and st.tolist() == [0, 0, 3, 0, 0, 0] and summ == [5, -1, 0, 5]
    # four valid points: not done, everything an outlier
    c2[3, 1] = 2e4
    done, st, E, summ, _ = R.do_ransac5(c1, c2, _IdCam(), _IdCam(), 100.0, 100.0)
    assert not done and (st == 3).all() and summ[3] == 4 and not E.any()


def test_no_qualifying_model_keeps_every_valid_point():
    # threshold 0: (float)(thr^2) == 0, so not even a model's own five points (Sampson error ~1e-30, not 0) count, no model
    # ever qualifies, and the pre-filled all-1 mask survives
    rng = np.random.default_rng(4)
    h1, h2 = rng.normal(size=(40, 2)), rng.normal(size=(40, 2))
    run = R.registrator_runs([(h1, h2, 0.0)])[0]
    assert run.max_good == 0 and run.best_iter == -1 and run.iters == 75 and (run.mask == 1).all() and not run.E.any()


def test_sampson_error_is_zero_on_exact_correspondences():
    X, truth = _minimal(np.random.default_rng(5), 1)
    h1 = np.c_[X[0][0], X[1][0]]
    h2 = np.c_[X[2][0], X[3][0]]
    err = R.sampson_err(truth[0][None], h1, h2)
    assert err.dtype == np.float32 and err.max() < 1e-20
