"""The restatement of the output stage (tests/output_restatement.py) against what exists on the CPU: its inertial part in binary64
against the oracle's filter (set_inertial_state + transform_to + get_state on a filter with cameraTrailLength = 1, the reference's
coordinate filter), rmat2quat on one scripted orientation per branch, the 4 x 4 inverse against numpy.linalg.inv in long double,
the point-cloud rules on a scripted table, and the preconditions of the corpus the GPU test runs."""
import numpy as np
import pytest

import output_restatement as R
from flow_predict_restatement import LD, quat2rmat

U = 2.0 ** -53


@pytest.mark.parametrize("trail", [3, 20])
def test_inertial_part_equals_the_oracles_coordinate_filter(oracle, trail):
    """transformTo on the oracle forms the dense products; the restatement forms the three diagonal blocks that are not the
    identity. Both are binary64 sums of the same three or four products per entry, in another order at most: 64 u of the block's
    largest magnitude covers it (the project's floor)."""
    c = R.case(trail)
    checked = 0
    for s in range(R.S):
        if c["frozen"][s]:
            continue
        m, P, session, index, visit, slam = R.set_inputs(c, s)
        branches = []
        given = slam["ready"]
        pos, ori = R.slamPose(np.float64, R._vec(np.float64, m[R.POS:R.POS + 3]), R._vec(np.float64, m[R.ORI:R.ORI + 4]),
                              R._vec(np.float64, c["par"].imuToCamera),
                              R._vec(np.float64, slam["slam_to_odometry"] if given else R.IDENTITY), branches)
        o = oracle.Ekf(oracle.ekf_default_params(cameraTrailLength=1))
        o.set_inertial_state(m[:R.INER], P[:R.INER, :R.INER])
        o.transform_to(np.array(pos, np.float64), np.array(ori, np.float64))
        want_m, want_P = np.array(o.m)[:R.INER], np.array(o.P)[:R.INER, :R.INER]
        r = c["rest"][s]
        got_m, diag = np.array(r["inertial_mean"], np.float64), np.array(r["inertial_cov_diag"], np.float64)
        for s0, k in ((R.POS, 3), (R.VEL, 3), (R.ORI, 4), (R.BGA, 10)):
            L = np.abs(want_m[s0:s0 + k]).max()
            assert np.abs(got_m[s0:s0 + k] - want_m[s0:s0 + k]).max() <= 64 * U * L, (trail, s, "mean", s0)
        assert np.abs(diag - np.diag(want_P)).max() <= 64 * U * np.abs(np.diag(want_P)).max(), (trail, s, "diagonal")
        assert np.array_equal(diag[R.BGA:], np.diag(want_P)[R.BGA:]) and np.array_equal(got_m[R.BGA:], m[R.BGA:R.INER])      # identity blocks: copies
        for key, s0 in (("position_cov", R.POS), ("velocity_cov", R.VEL)):
            blk, want = np.array(r[key], np.float64).reshape(3, 3), want_P[s0:s0 + 3, s0:s0 + 3]
            assert np.abs(blk - want).max() <= 64 * U * np.abs(want).max(), (trail, s, key)
        # the transformed pose is the target pose: transformTo moves the filter there
        assert np.abs(got_m[R.POS:R.POS + 3] - np.array(pos, np.float64)).max() <= 64 * U * np.abs(pos).max()
        assert min(np.abs(got_m[R.ORI:R.ORI + 4] - ori).max(), np.abs(got_m[R.ORI:R.ORI + 4] + ori).max()) <= 64 * U
        checked += 1
    assert checked == R.S - 1


@pytest.mark.parametrize("T", [np.float64, LD])
def test_rmat2quat_inverts_quat2rmat_up_to_sign_in_every_branch(T):
    for want_branch, q in enumerate(R.BRANCH_QUATS):
        q = R._vec(T, q)
        norm = np.sqrt(sum(x * x for x in q))                              # a unit quaternion in T: quat2rmat is a rotation only for those
        q = [x / norm for x in q]
        got, branch = R.rmat2quat(T, quat2rmat(T, q))
        assert branch == want_branch, (q, branch)
        sign = 1 if got[branch] * q[branch] > 0 else -1
        err = max(abs(float(sign * g - x)) for g, x in zip(got, q))
        assert err <= 16 * float(np.finfo(T).eps), (branch, err)
        assert got[branch] > 0                                             # the branch's component is the positive root: the sign convention


def test_inverse_equals_numpy_in_long_double():
    rng = np.random.default_rng(4)
    worst = 0.0
    for k in range(40):
        A = R.rigid(rng.normal(size=3), rng.uniform(0, 3), rng.uniform(-5, 5, 3)) if k % 2 else rng.normal(size=(4, 4)) + 2 * np.eye(4)
        want = np.linalg.inv(A)                                            # binary64 LAPACK: the yardstick's own error is cond * u
        got = np.array(R.inv4(LD, R._vec(LD, A)), LD).reshape(4, 4)
        cond = np.linalg.cond(A)
        err = float(np.abs(got - want).max() / np.abs(want).max())
        assert err <= 16 * cond * U, (k, err, cond)
        # and it is an inverse, in long double
        res = float(np.abs(got @ A.astype(LD) - np.eye(4)).max())
        assert res <= 64 * cond * float(np.finfo(LD).eps), (k, res)
        got64 = np.array(R.inv4(np.float64, R._vec(np.float64, A)), np.float64).reshape(4, 4)
        assert float(np.abs(got64 - got).max() / np.abs(want).max()) <= 16 * cond * U
        worst = max(worst, err / (cond * U))
    print("worst error against numpy in units of cond * u:", worst)


ROWS = dict(nv=R.NOT_VISITED_ROW, tri=R.TRI_FAILED_ROW, prep=R.PREPARE_FAILED_ROW, out=R.OUTLIER_ROW, inl=R.INLIER_ROW)
TABLE = [
    # (rows in visit order, maxVisualUpdates, maxSuccessfulVisualUpdates) -> [(candidate, status)]
    ("not visited", ["nv", "nv"], 4, 5, []),
    ("triangulation failed", ["tri", "inl", "nv"], 4, 5, [(1, 1)]),
    ("prepare failed stays POSE_TRAIL", ["prep", "inl"], 4, 5, [(0, 1), (1, 1)]),
    ("gate outlier", ["out", "inl"], 4, 5, [(0, 4), (1, 1)]),
    ("inlier", ["inl"], 4, 5, [(0, 1)]),
    ("stopped by the success limit: the stopping candidate is left out", ["inl", "out", "inl", "inl"], 6, 2, [(0, 1), (1, 4)]),
    ("stopped by the attempt limit", ["out", "tri", "inl", "inl"], 3, 5, [(0, 4)]),
    ("attempt limit reached by a failed triangulation", ["inl", "prep", "tri", "inl"], 3, 5, [(0, 1), (1, 1)]),
    ("no stop", ["inl", "out", "prep", "tri", "nv"], 6, 5, [(0, 1), (1, 4), (2, 1)]),
    ("no success limit", ["inl", "inl", "inl", "nv"], 6, 0, [(0, 1), (1, 1), (2, 1)]),
    ("a gap in the visits is not an attempt", ["nv", "inl", "nv", "out", "inl"], 3, 5, [(1, 1), (3, 4)]),
]


@pytest.mark.parametrize("name,rows,V,succ,want", TABLE, ids=[t[0] for t in TABLE])
def test_point_cloud_rules(name, rows, V, succ, want):
    status = [ROWS[k][:2] for k in rows]
    gate = [ROWS[k][2] for k in rows]
    assert R.pointCloud(status, gate, len(rows), V, succ) == want


def branch_lists(c):
    return [(r["branches"], t["branches"]) for r, t in zip(c["rest"], c["truth"]) if r is not None]


@pytest.mark.parametrize("trail,passthrough", [(3, False), (20, False), (3, True)])
def test_corpus_preconditions(trail, passthrough):
    """What the GPU test relies on, checked here first: both precisions take the same rmat2quat branch in every conversion of every
    set, every branch occurs, and the scripted sets are what they are meant to be."""
    c = R.case(trail, passthrough)
    seen = set()
    for rest, truth in branch_lists(c):
        assert rest == truth
        seen |= set(rest)
    assert seen == {0, 1, 2, 3}
    assert c["rest"][R.FROZEN] is None and c["frozen"].sum() == 1
    nr = c["rest"][R.NOT_READY]
    assert nr["n_points"] == 0 and nr["n_trail"] > 0 and not np.any(np.array(nr["trail_pose"], np.float64))
    if not passthrough:
        assert np.isnan(np.array(nr["api_trail_pose"], np.float64)).all()  # the zero pose through the inverse of a singular matrix
    else:
        for r in c["rest"]:
            if r is not None:
                assert r["api_trail_pose"] == r["trail_pose"] and r["api_pose"] == r["inertial_mean"][:3] + r["inertial_mean"][R.ORI:R.ORI + 4]
    assert [r["n_points"] for r in c["rest"] if r is not None] == [3, 2, 0, 2]
    assert c["rest"][0]["point_status"] == [1, 4, 1] and c["rest"][2]["point_status"] == [4, 1] and c["rest"][4]["point_status"] == [1, 1]
    assert sorted(r["n_trail"] for r in c["rest"] if r is not None) == sorted([trail, 1, trail if trail == 3 else trail - 2, 0])
    for s in R.TRANSFORMED:
        assert not np.allclose(c["s2o"][s].reshape(4, 4), np.eye(4)) and abs(np.linalg.norm(c["s2o"][s].reshape(4, 4)[:3, 3])) > 2
        assert np.allclose(c["s2o"][s].reshape(4, 4) @ c["o2s"][s].reshape(4, 4), np.eye(4))
    # the truth is closer to the binary64 restatement than the test's floor is wide: the bound discriminates
    for r, t in zip(c["rest"], c["truth"]):
        if r is not None:
            a, b = np.array(r["inertial_mean"], LD), np.array(t["inertial_mean"], LD)
            assert float(np.abs(a - b).max()) <= 64 * U * float(np.abs(b).max())
