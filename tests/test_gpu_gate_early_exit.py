"""The chi2 gates stop their Cholesky once a track is certainly rejected (ekf_device.hpp gate_factor_chi2, `exit_above`): the early path is
taken only when nobody reads chi2, so a visit WITH a chi2 buffer runs the whole factorisation and a visit WITHOUT one may stop after
any block column but the last. Both must give the same verdicts, apply the same updates, and agree with the oracle's sequence.

The prefix of chi2 after the first m rows, noise_scale * z[:m]' z[:m] with z = L^-1 v, is the quadratic form of the LEADING m x m
problem v[:m]' S[:m, :m]^-1 v[:m]: the oracle's own gate on the first m rows of (H, f, y) computes it, and that is how the inputs below
are checked ("late" outliers: below the threshold until the final block)."""
import numpy as np
import pytest

from hybvio_amd import capi
from ekf_truth import chi2inv95
from test_gpu_visual_prepare import VARIANTS, _apply, _ragged_frame, _random_tracks, _rel, _well_conditioned

pytestmark = pytest.mark.gpu

B, TRAIL = 12, 20
# residuals of a few 1e-3 .. 1e-2 (normalised image coordinates) against R = (r_gate^2 noiseScale) I = I and a covariance of the same
# order as R in the measurement space: neither term of S = H P H' + R is negligible, the factor is not nearly diagonal
R_GATE, R_UPDATE = 0.01, 0.05
KINDS = ["inlier"] * 3 + ["gross"] * 3 + ["late"] * 3 + ["marginal"] * 3
MARGINAL = (0.98, 1.02, 1.10)
LATE = (1.5, 3.0, 10.0)                   # chi2 / threshold of the three late outliers


def _covariance(rng, n):
    A = rng.normal(size=(n, n)) * 0.02
    return (A @ A.T * 1e-3 + np.eye(n) * 1e-4) * 1e3


def _scale_to(ratio_of, v_fixed, v_dir, target):
    """Bisection (in the logarithm of the scale s) until chi2(v_fixed + s v_dir) / threshold = target, on the oracle."""
    lo, hi = 1e-8, 1e8
    assert ratio_of(v_fixed + lo * v_dir) < target < ratio_of(v_fixed + hi * v_dir)
    for _ in range(200):
        mid = np.sqrt(lo * hi)
        r = ratio_of(v_fixed + mid * v_dir)
        if abs(r - target) <= 1e-9 * target:
            break
        lo, hi = (mid, hi) if r < target else (lo, mid)
    assert abs(r - target) <= 1e-6 * target, (r, target)
    return v_fixed + mid * v_dir


def _triangulable_tracks(oracle, rng, count, npose):
    """`count` random stereo tracks that the oracle triangulates and prepares, well conditioned (the device then reports the same status)."""
    T1, T2, means, idx, feat, vel = _random_tracks(oracle, rng, 4 * count, TRAIL, npose, True, bad_fraction=0.0)
    par, keep = oracle.tri_default_params(), []
    for b in range(4 * count):
        ost, ops = oracle.visual_track_prepare(par, means[b], idx[b], T1, T2, feat[b], vel[b])[:2]
        if (ost, ops) == (0, 0) and _well_conditioned(oracle.tri_last_diag()) and idx[b][2] >= 1:
            keep.append(b)
    keep = keep[:count]
    assert len(keep) == count
    return T1, T2, means[keep], idx[keep], feat[keep], vel[keep]


_PROBLEMS = {}


def _problem(oracle, npose):
    """Twelve records of `npose` stereo poses, every kind present; computed once per pose count and shared by the variants (read-only)."""
    if npose in _PROBLEMS:
        return _PROBLEMS[npose]
    rng = np.random.default_rng(7000 + npose)
    par, table = oracle.tri_default_params(), chi2inv95()
    T1, T2, means, idx, feat, vel = _triangulable_tracks(oracle, rng, B, npose)
    rows = 4 * npose
    thr = table[rows]
    nblocks = (rows + 15) // 16
    Ps, ys, ratios, expect = [], [], [], []
    for b in range(B):
        o = oracle.Ekf(oracle.ekf_default_params(cameraTrailLength=TRAIL))
        P = _covariance(rng, o.n)
        o.set_state(means[b]); o.set_cov(P)
        ost, ops, opf, oH, of = oracle.visual_track_prepare(par, means[b], idx[b], T1, T2, feat[b], vel[b])
        assert (ost, ops) == (0, 0), (b, ost, ops)
        ratio_of = lambda v, m=rows: o.visual_track_outlier_check(oH[:m], of[:m], of[:m] + v[:m], R_GATE)[1] / thr
        kind, j = KINDS[b], b % 3
        noise = 1e-4 * rng.normal(size=rows)
        if kind == "inlier":
            v = noise
        elif kind == "gross":
            v = 0.05 * rng.choice([-1.0, 1.0], size=rows)
        elif kind == "late":                                  # the error sits in the rows of the last pose of the second camera only
            d = np.zeros(rows); d[-2:] = rng.choice([-1.0, 1.0], size=2)
            v = _scale_to(ratio_of, noise, d, LATE[j])
            for k in range(1, nblocks):                       # ... so every prefix in front of the final block is far below the threshold
                assert ratio_of(v, 16 * k) < 0.01, (b, k, ratio_of(v, 16 * k))
        else:
            v = _scale_to(ratio_of, np.zeros(rows), 0.01 * rng.normal(size=rows), MARGINAL[j])
        y = of + v
        status, chi2 = o.visual_track_outlier_check(oH, of, y, R_GATE)
        assert abs(chi2 / thr - 1.0) > 1e-6, (b, kind, chi2 / thr)                       # no verdict hangs on the last bits
        assert status == {"inlier": 0, "gross": 3, "late": 3}.get(kind, 3 if MARGINAL[j] > 1 else 0), (b, kind, chi2 / thr)
        m0, P0 = o.m.copy(), o.P.copy()
        if status == 0:
            o.update_visual_track(oH, of, y, R_UPDATE)
        Ps.append(P0); ys.append(y); ratios.append(chi2 / thr)
        expect.append((status, m0, P0, o.m.copy(), o.P.copy()))
    _PROBLEMS[npose] = (T1, T2, means, idx, feat, vel, np.array(ys), Ps, expect, ratios)
    return _PROBLEMS[npose]


def _visit(g, ctx, vp, npose, means, Ps, idx, feat, vel, y, with_chi2):
    """One visual_track_dev from the saved (m, P): (status, gate_status, chi2 or None, [(m, P)])."""
    import torch
    nb = len(means)
    for b in range(nb):
        g.set_state(b, means[b], Ps[b])
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    d_idx, d_feat, d_vel, d_y = dev(idx, np.int32), dev(feat, np.float64), dev(vel, np.float64), dev(y, np.float64)
    st = torch.full((nb, 2), -1, dtype=torch.int32, device="cuda")
    gs = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    chi = torch.zeros((nb,), dtype=torch.float64, device="cuda")
    g.visual_track_dev(vp, npose, d_idx.data_ptr(), d_feat.data_ptr(), d_vel.data_ptr(), d_y.data_ptr(), R_GATE, R_UPDATE,
                       st.data_ptr(), gs.data_ptr(), chi.data_ptr() if with_chi2 else 0, 0)
    torch.cuda.synchronize()
    return st.cpu().numpy(), gs.cpu().numpy(), chi.cpu().numpy() if with_chi2 else None, [g.get_state(b) for b in range(nb)]


@pytest.mark.parametrize("npose", [4, 5, 9, 12, 13, 21])      # 16 / 20 / 36 / 48 / 52 / 84 rows: 1 / 2 (ragged, w = 4) / 3 / 3 / 4 / 6 blocks
@pytest.mark.parametrize("variant", ["default", "split_tri", "split_tri_one_stream", "fused_front", "gate_own_launch", "long_two_launches"])
def test_same_verdicts_with_and_without_a_reader_of_chi2(oracle, variant, npose):
    """visual_track_dev twice from one saved (m, P), with a chi2 buffer (whole factorisation) and without (early exit allowed): identical
    status and gate status, byte-identical (m, P) afterwards, every status the oracle's (prepare -> outlier check -> update). Twelve
    records per batch: three inliers, three gross outliers, three whose error sits in the final block only, three at 0.98 / 1.02 / 1.10
    of the threshold."""
    import torch
    T1, T2, means, idx, feat, vel, y, Ps, expect, ratios = _problem(oracle, npose)
    vp = capi.vu_default_params(imu_to_camera=T1, second_imu_to_camera=T2)
    with capi.Context(width=64, height=64) as ctx:
        _apply(ctx, variant)
        g = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=TRAIL), B)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        full = _visit(g, ctx, vp, npose, means, Ps, idx, feat, vel, y, True)
        early = _visit(g, ctx, vp, npose, means, Ps, idx, feat, vel, y, False)
        g.close()
    print(f"{variant} np={npose}: chi2 / threshold of the oracle {np.round(ratios, 4).tolist()}, gate status {early[1].tolist()}")
    assert np.array_equal(full[0], early[0]) and np.array_equal(full[1], early[1])
    for b in range(B):                                          # the same updates were applied: the same bytes
        assert full[3][b][0].tobytes() == early[3][b][0].tobytes() and full[3][b][1].tobytes() == early[3][b][1].tobytes(), b
    thr = chi2inv95()[4 * npose]
    for b, (status, m0, P0, m1, P1) in enumerate(expect):
        assert early[0][b].tolist() == [0, 0] and early[1][b] == status, (b, KINDS[b], early[1][b], status)
        assert abs(full[2][b] / thr - ratios[b]) <= 1e-7 * max(1.0, ratios[b]), (b, full[2][b] / thr, ratios[b])
        mg, Pg = early[3][b]
        if status == 0:
            assert _rel(mg, m1) < 1e-8 and _rel(Pg, P1) < 1e-8 and not np.array_equal(mg, m0), (b, _rel(mg, m1), _rel(Pg, P1))
        else:
            assert np.array_equal(mg, m0) and np.array_equal(Pg, P0), b


def _first_bad_pivot(S):
    """Index of the first non-positive pivot of the unpivoted Cholesky of S (the device's elimination order), or -1."""
    S = S.copy()
    for k in range(len(S)):
        if not S[k, k] > 0.0:
            return k
        S[k + 1:, k] /= S[k, k]
        S[k + 1:, k + 1:] -= np.outer(S[k + 1:, k], S[k, k + 1:])
    return -1


@pytest.mark.parametrize("npose", [9, 17])
def test_non_positive_pivot_behind_the_first_block(oracle, npose):
    """A covariance with a negative diagonal entry in a column of the track's third pose: S = S0 - |p| h h' keeps a positive definite
    leading 16 x 16 block for |p| < 1 / (h1' S0_11^-1 h1) and is indefinite for |p| > 1 / (h' S0^-1 h), h = that column of H. In
    between, the first block factors (its prefix, an inlier's, is far below the threshold) and a later block meets the pivot: status 3
    (CHI2, as a broken factorisation is reported) with or without a chi2 buffer, the filter untouched, and the call returns."""
    import torch
    rng = np.random.default_rng(8100 + npose)
    nb, rows = 4, 4 * npose
    T1, T2, means, idx, feat, vel = _triangulable_tracks(oracle, rng, nb, npose)
    par, thr = oracle.tri_default_params(), chi2inv95()[rows]
    ns = oracle.ekf_default_params().noiseScale ** 2
    rd = R_GATE ** 2 * ns
    Ps, ys = [], []
    for b in range(nb):
        ost, ops, opf, oH, of = oracle.visual_track_prepare(par, means[b], idx[b], T1, T2, feat[b], vel[b])
        assert (ost, ops) == (0, 0)
        P = _covariance(rng, len(means[b]))
        c = 20 + 7 * (int(idx[b][2]) - 1) + 3 + b % 4           # an orientation column of the third pose (idx > 0: a trail pose)
        assert idx[b][2] >= 1
        P[c, c] = 0.0
        S0 = oH @ P @ oH.T + rd * np.eye(rows)
        h = oH[:, c]
        p_lead, p_full = 1.0 / (h[:16] @ np.linalg.solve(S0[:16, :16], h[:16])), 1.0 / (h @ np.linalg.solve(S0, h))
        assert p_full < 0.8 * p_lead, (p_full, p_lead)                  # room on both sides of the geometric mean
        P[c, c] = -np.sqrt(p_full * p_lead)
        v = 1e-4 * rng.normal(size=rows)
        S = oH @ P @ oH.T + rd * np.eye(rows)
        bad = _first_bad_pivot(S)
        assert bad >= 16, bad                                   # the first block column factors, a later one meets the pivot
        z = np.linalg.solve(np.linalg.cholesky(S[:16, :16]), v[:16])
        assert ns * (z @ z) < 0.01 * thr                        # ... and its prefix is far below the threshold
        Ps.append(P); ys.append(of + v)
    vp = capi.vu_default_params(imu_to_camera=T1, second_imu_to_camera=T2)
    with capi.Context(width=64, height=64) as ctx:
        g = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=TRAIL), nb)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        for with_chi2 in (True, False):
            st, gs, _, states = _visit(g, ctx, vp, npose, means, Ps, idx, feat, vel, np.array(ys), with_chi2)
            assert st.tolist() == [[0, 0]] * nb and gs.tolist() == [3] * nb, (with_chi2, st.tolist(), gs.tolist())
            for b in range(nb):
                assert np.array_equal(states[b][0], means[b]) and np.array_equal(states[b][1], Ps[b]), (with_chi2, b)
        g.close()


@pytest.mark.parametrize("variant", ["split_tri", "default"])
def test_frame_loop_without_a_chi2_buffer(oracle, variant):
    """hv_ekf_visual_frame_ragged_dev without a chi2 buffer (every gate of the loop may stop early) against the oracle's sequential loop:
    every visit status, the applied count and the final (m, P), within the tolerances of test_whole_frame_loop_with_ragged_track_lengths."""
    import torch
    rng = np.random.default_rng(77 + B)
    K, quota, np_max = 8, 3, 21
    T1, T2, means, _, _, _ = _random_tracks(oracle, rng, B, TRAIL, 6, True, bad_fraction=0.0)
    lens, idx, feat, vel, ys, per = _ragged_frame(oracle, rng, means, TRAIL, K, np_max, True)
    vp = capi.vu_default_params(imu_to_camera=T1, second_imu_to_camera=T2)
    par = oracle.tri_default_params()
    r_gate, r_update = 1.5, 0.05
    with capi.Context(width=64, height=64) as ctx:
        _apply(ctx, variant)
        g = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=TRAIL), B)
        filters = []
        for b in range(B):
            o = oracle.Ekf(oracle.ekf_default_params(cameraTrailLength=TRAIL))
            P = o.P.copy() * 1e-6 + np.eye(o.n) * 1e-4
            o.set_state(means[b]); o.set_cov(P)
            g.set_state(b, means[b], P)
            filters.append(o)
        dev = lambda a, dt: torch.from_numpy(np.array(a, dt, order="C")).cuda()
        d = [dev(lens, np.int32), dev(idx, np.int32), dev(feat, np.float64), dev(vel, np.float64), dev(ys, np.float64)]
        st = torch.full((K, B, 2), -9, dtype=torch.int32, device="cuda"); gs = torch.full((K, B), -9, dtype=torch.int32, device="cuda")
        counter = torch.zeros((B,), dtype=torch.int32, device="cuda")
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        g.visual_frame_ragged_dev(vp, K, np_max, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                  r_gate, r_update, st.data_ptr(), gs.data_ptr(), counter.data_ptr(), quota)
        torch.cuda.synchronize()
        st, gs, counts = st.cpu().numpy(), gs.cpu().numpy(), counter.cpu().numpy()
        applied, rejected, ties = 0, 0, 0
        for b, o in enumerate(filters):
            done = 0
            for k in range(K):
                if done >= quota or lens[k, b] == 0:
                    assert st[k, b].tolist() == [-1, -1] and gs[k, b] == 1, (b, k)
                    continue
                i_, f_, v_, yy = per[(k, b)]
                ost, ops, opf, oH, of = oracle.visual_track_prepare(par, o.m.copy(), i_, T1, T2, f_, v_)
                if st[k, b].tolist() != [ost, ops]:            # (a degenerate triangulation: the class of the status, as in the ragged test)
                    assert not _well_conditioned(oracle.tri_last_diag()) and ost != 0 and st[k, b, 0] != 0, (b, k, st[k, b].tolist(), [ost, ops])
                    ties += 1
                if (ost, ops) != (0, 0):
                    assert gs[k, b] == 1
                    continue
                status, _ = o.visual_track_outlier_check(oH, of, yy, r_gate)
                assert gs[k, b] == status, (b, k, lens[k, b])
                if status == 0:
                    o.update_visual_track(oH, of, yy, r_update); done += 1
                else:
                    rejected += 1
            assert counts[b] == done
            applied += done
            mg, Pg = g.get_state(b)
            assert _rel(mg, o.m) < 1e-8 and _rel(Pg, o.P) < 1e-7, (b, _rel(mg, o.m), _rel(Pg, o.P))
        assert applied > B // 2 and rejected > 0 and ties <= 1, (applied, rejected, ties)
        g.close()
