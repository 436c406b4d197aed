"""CPU checks of tests/upright2p_restatement.py, the numpy statement of the stereo upright 2-point filter (the gather, the
two-point solver, the sample-consensus loop) that the device kernel (hybvio_amd/csrc/upright2p.hip) is compared with."""
import math

import numpy as np
import pytest

import ransac5_restatement as R5
import upright2p_restatement as U

T = U.SECOND_TO_FIRST


def _cam(oracle, name="pinhole"):
    spec = R5.CAMERAS[name]
    return oracle.Camera(spec[0], *spec[1:5], coeffs=spec[5], max_valid_fov_deg=spec[6])


def _problems(rng, H):
    """Random two-point problems with rays of any direction and length: X [H, 2, 3], r [H, 2, 3], theta [H], t [H, 3]."""
    th, t = rng.uniform(-math.pi, math.pi, H), rng.normal(size=(H, 3))
    X = rng.normal(size=(H, 2, 3)) * 2 + np.array([0, 0, 5.0])
    Y = np.stack([X[h] @ U.rz(th[h]).T + t[h] for h in range(H)])
    r = Y / np.linalg.norm(Y, axis=2, keepdims=True) * rng.uniform(0.5, 2.0, (H, 2, 1))
    return X, r, th, t


def test_solver_contains_the_true_pose_and_every_model_reprojects_its_sample():
    X, r, th, t = _problems(np.random.default_rng(3), 2000)
    mod, valid = U.solve(X, r)
    assert valid.all()                                                        # both roots are real on exact data
    for h in range(len(X)):
        want = np.concatenate([U.rz(th[h]).reshape(9), t[h]])
        err = [np.abs(U.model12(mod[h, s]) - want).max() for s in range(2)]
        assert min(err) <= 1e-9, (h, err)
        for s in range(2):
            M = U.model12(mod[h, s])
            Y = X[h] @ M[:9].reshape(3, 3).T + M[9:]
            cr = np.linalg.norm(np.cross(Y, r[h]), axis=1) / (np.linalg.norm(Y, axis=1) * np.linalg.norm(r[h], axis=1))
            assert cr.max() <= 1e-9, (h, s, cr)                              # on the ray's line (either sign: no cheirality test)
    # the order of the pair does not matter to t and R
    mod2, valid2 = U.solve(X[:, ::-1], r[:, ::-1])
    assert valid2.all() and np.abs(mod2 - mod).max() <= 1e-9


def test_solver_rejects_degenerate_samples():
    X, r, _, _ = _problems(np.random.default_rng(4), 8)
    Xv = X.copy(); Xv[:, 1, :2] = Xv[:, 0, :2]                                # vertically aligned points: n2 == 0
    assert not U.solve(Xv, r)[1].any()
    rh = r.copy(); rh[:, :, 2] = 0.0                                          # both rays horizontal: r1.z == 0
    assert not U.solve(X, rh)[1].any()
    rn = r.copy(); rn[:, 0, 1] = np.nan
    assert not U.solve(X, rn)[1].any()
    rp = r.copy(); rp[:, 1] = rp[:, 0] * 2.0                                  # parallel rays: b == 0, A == 0
    assert not U.solve(X, rp)[1].any()


def test_compute_max_iterations():
    logp = math.log(1e-4)
    assert U.compute_max_iterations(2, 0.3, logp, 50, 500) == 98
    assert U.compute_max_iterations(2, 1.0, logp, 50, 500) == 50 and U.compute_max_iterations(2, 0.0, logp, 50, 500) == 500
    assert U.compute_max_iterations(3, 0.3, logp, 50, 500) == 337             # the sample-size argument: RANSAC3's figure
    assert U.iteration_cap(U.Params()) == 98
    assert U.iteration_cap(U.Params(ransacStereoUpright2pMaxIterations=60)) == 60


def test_sampler_is_the_ransac3_sampler_with_two_draws():
    import ransac3_restatement as R3
    draws = np.arange(1, 61, dtype=np.uint32) * np.uint32(2654435761)
    a, b = U.Sampler(9, draws, 3), R3.Sampler(9, draws)
    assert [a.sample() for _ in range(10)] == [b.sample() for _ in range(10)]
    s = U.Sampler(2, draws)
    assert all(sorted(s.sample()) == [0, 1] for _ in range(5)) and s.pos == 10


@pytest.fixture(scope="module")
def runs(oracle):
    """Noise-free sets per attitude and outlier level, run once."""
    cam = _cam(oracle, "pinhole_radial")
    rng = np.random.default_rng(11)
    out = []
    for k, (outl, kind) in enumerate((o, a) for o in (0.0, 0.2, 0.6, 0.75) for a in U.ATTITUDES):
        d = U.make_set(rng, cam, 100, outl, 0.0, 4, 3, 0, kind=kind, psi=rng.uniform(-math.pi, math.pi))
        d["draws"] = oracle.mt19937_draws(50 + k, 2 * U.MAX_ITERS)
        d["outl"] = outl
        d["res"] = U.do_upright2p(d["status"], d["prev_left"], d["prev_right"], d["cur_left"], cam, cam, T, d["poses"], d["draws"])
        out.append(d)
    return cam, out


def test_noise_free_sets_recover_the_truth_and_the_loop_ends_where_it_should(runs):
    cam, sets = runs
    ended = set()
    for d in sets:
        ts, done, cnt, model, summ = d["res"]
        assert done and np.array_equal(ts == 0, d["truth"]), (d["outl"], summ)
        assert cnt == int(d["truth"].sum()) == summ[0] and summ[3] == 100
        assert np.abs(model - d["model_true"]).max() <= 1e-5                 # binary32 corners
        ended.add(summ[2])
        assert summ[2] == {0.0: 50, 0.2: 50, 0.6: 53, 0.75: 98}[d["outl"]], (d["outl"], summ)   # minimum, adaptive, cap
    assert ended == {50, 53, 98}                                             # 53 = ceil(log 1e-4 / log(1 - 0.4^2))


def test_a_yaw_error_of_any_size_leaves_the_mask_unchanged(runs):
    cam, sets = runs
    d = sets[5]
    P = d["poses"].reshape(2, 4, 4)
    for psi in (-math.pi, -2.0, -0.3, 1e-3, 1.0, 3.0, math.pi):
        Q = P.copy()
        Q[1, :3, :3] = U.rz(psi) @ P[1, :3, :3]
        ts, done, cnt, model, summ = U.do_upright2p(d["status"], d["prev_left"], d["prev_right"], d["cur_left"], cam, cam, T, Q.reshape(32), d["draws"])
        assert done and np.array_equal(ts, d["res"][0]) and summ == d["res"][4], psi
        want = U.rz(psi) @ d["res"][3][:9].reshape(3, 3)
        assert np.abs(model[:9].reshape(3, 3) - want).max() <= 1e-9 and np.abs(model[9:] - U.rz(psi) @ d["res"][3][9:]).max() <= 1e-9


def test_fewer_than_two_correspondences_is_skipped_and_the_tail_clears_every_track(oracle):
    cam = _cam(oracle)
    rng = np.random.default_rng(2)
    d = U.make_set(rng, cam, 1, 0.0, 0.0, 3, 2, 0)                            # one good feature, two rejected triangulations
    draws = oracle.mt19937_draws(1, 2 * U.MAX_ITERS)
    ts, done, cnt, model, summ = U.do_upright2p(d["status"], d["prev_left"], d["prev_right"], d["cur_left"], cam, cam, T, d["poses"], draws)
    assert not done and summ == [0, -1, 0, 1] and not model.any()
    assert (ts[d["status"] == 0] == 3).all() and np.array_equal(ts[d["status"] != 0], d["status"][d["status"] != 0])
    ts, typ, cnt, score, summ = U.compute(d["status"], d["prev_left"], d["prev_right"], d["cur_left"], cam, cam, T, d["poses"], draws, 2)
    assert typ == U.TYPE_SKIPPED and (ts == 3).all() and score == 2 / 3
    d = U.make_set(rng, cam, 30, 0.2, 0.0, 2, 0, 0)
    ts, typ, cnt, score, summ = U.compute(d["status"], d["prev_left"], d["prev_right"], d["cur_left"], cam, cam, T, d["poses"], draws, 21)
    assert typ == U.TYPE_UPRIGHT_2P == 4 and cnt == int((ts == 0).sum()) == 24 and score == 21 / 30
    # non-finite poses: the correspondences are gathered, no sample has a model
    P = d["poses"].copy(); P[16] = np.nan
    ts, done, cnt, model, summ = U.do_upright2p(d["status"], d["prev_left"], d["prev_right"], d["cur_left"], cam, cam, T, P, draws)
    assert not done and summ == [0, -1, 98, 30]
