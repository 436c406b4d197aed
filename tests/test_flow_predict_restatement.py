"""CPU checks of tests/flow_predict_restatement.py, the yardstick of hv_flow_predict_batch_dev: its binary64 pieces against the
oracle's primitives on random inputs (pinhole and every algebraic piece bit for bit, fisheye within 4 binary64 ulp: libm's atan /
sin / cos / acos are not correctly rounded and differ between the C oracle and numpy), and the shared corpus: it contains what it
is there for, and the restatement and the truth leave at most 1 % of its points undecided."""
import numpy as np
import pytest

import flow_predict_restatement as F
from hybvio_amd import capi

F64, LD = np.float64, F.LD
N = 300


def _ulps(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), np.finfo(np.float64).tiny)


def _camera_pair(spec):
    from oracle import orc
    kw = {k: v for k, v in spec.items() if k not in ("kind", "fx", "fy", "ppx", "ppy")}
    args = (spec["kind"], spec["fx"], spec["fy"], spec["ppx"], spec["ppy"])
    return orc.Camera(*args, **kw), F.Camera(capi.camera_model(*args, **kw))


def test_pose_trail_pinv_and_two_camera_triangulation_equal_the_oracle(oracle):
    rng = np.random.default_rng(11)
    A, B = F.imu_to_camera_pair()
    for it in range(N):
        m = rng.normal(0.0, 2.0, 20 + 7 * 6)
        for k in range(7):
            io = F.historyIndices(k - 1)[1]
            m[io:io + 4] /= np.linalg.norm(m[io:io + 4]) * (1.0 if it % 3 else 1.0 + 1e-3 * rng.normal())   # some not quite normalised
        index = list(range(7))
        want = oracle.extract_camera_pose_trail(m, index, A, B)
        for cam, T in enumerate((A, B)):
            got = F.extractCameraPoseTrail(F64, F._vec(F64, m), index, F._vec(F64, T))
            for k in index:
                assert np.array_equal(np.array(got[k][0]), np.array(want[cam * 7 + k].p[:])), (it, cam, k)
                assert np.array_equal(np.array(got[k][1]), np.array(want[cam * 7 + k].R[:])), (it, cam, k)
        M32 = rng.normal(0.0, 1.0, (3, 2))
        assert np.array_equal(np.array(F.pinv32(F64, F._vec(F64, M32))).reshape(2, 3), oracle.pinv32(M32)), it
        ip0, ip1 = rng.uniform(-0.8, 0.8, 2), rng.uniform(-0.8, 0.8, 2)
        got = F.extractCameraPoseTrail(F64, F._vec(F64, m), index, F._vec(F64, A))
        pf = F.triangulateWithTwoCameras(F64, got[1], got[5], F._vec(F64, ip0), F._vec(F64, ip1))
        assert np.array_equal(np.array(pf), oracle.triangulate_with_two_cameras(want[1], want[5], ip0, ip1)[0]), it


@pytest.mark.parametrize("name", ["PLAIN", "RADIAL", "ROTATED"])
def test_pinhole_camera_calls_equal_the_oracle_bit_for_bit(oracle, name):
    ocam, rcam = _camera_pair(getattr(F, name))
    rng = np.random.default_rng(21)
    for it in range(N):
        x, y = rng.uniform(-50, 800), rng.uniform(-50, 530)
        ok, ray = ocam.pixel_to_ray(x, y)
        got_ok, got, _ = rcam.pixelToRay(F64, x, y)
        assert got_ok == ok and np.array_equal(np.array(got), ray), (it, x, y)
        v = rng.normal(0.0, 1.0, 3) * rng.uniform(0.5, 20.0)
        v[2] = abs(v[2]) if it % 4 else -abs(v[2])                                    # a quarter behind the camera
        ok, pix = ocam.ray_to_pixel(v)
        got_ok, got, _ = rcam.rayToPixel(F64, F._vec(F64, v))
        assert got_ok == ok and (not ok or np.array_equal(np.array(got), pix)), (it, v)


def test_fisheye_camera_calls_equal_the_oracle_within_4_ulp(oracle):
    ocam, rcam = _camera_pair(F.FISHEYE)
    rng = np.random.default_rng(31)
    fails = 0
    for it in range(N):
        x, y = rng.uniform(0, 752), rng.uniform(0, 480)
        ok, ray = ocam.pixel_to_ray(x, y)
        got_ok, got, _ = rcam.pixelToRay(F64, x, y)
        fails += not ok
        assert got_ok == ok and (_ulps(got, ray) <= 4).all(), (it, x, y, _ulps(got, ray))
        v = rng.normal(0.0, 1.0, 3) * rng.uniform(0.5, 20.0)
        v[2] = abs(v[2]) * (0.2 if it % 2 else 1.0) if it % 4 else -abs(v[2])
        ok, pix = ocam.ray_to_pixel(v)
        got_ok, got, _ = rcam.rayToPixel(F64, F._vec(F64, v))
        assert got_ok == ok and (not ok or (_ulps(got, pix) <= 4).all()), (it, v)
    assert fails > N // 50                                                            # pixels beyond max_valid_fov occur


def _points():
    for name in F.CASES:
        c = F.case(name)
        for ty in c["types"]:
            for s in range(c["S"]):
                for i, (r, t) in enumerate(zip(*c["results"][ty][s])):
                    yield c, ty, s, i, r, t


def test_corpus_contains_what_it_is_there_for():
    n = 0
    seen = dict(triangulated=0, span9=0, span10=0, behind=0, clamped=0, no_column=0, pixel_to_ray_failed=0, ray_to_pixel_failed=0,
                removed_keyframe=0)
    for c, ty, s, i, r, t in _points():
        n += 1
        kfs = c["finals"][s]["session"].ekfStateIndex.keyframes
        numbers = [k.frameNumber for k in kfs[1:]]
        seen["triangulated"] += r["triangulated"]
        seen["span9"] += r["span"] == 9
        seen["span10"] += r["span"] == 10
        seen["behind"] += r["triangulated"] and not r["in_front"]
        seen["clamped"] += r["clamped"]
        seen["no_column"] += r["span"] is None
        seen["pixel_to_ray_failed"] += not r["p2r"]
        seen["ray_to_pixel_failed"] += r["r2p"] is False
        # a removal out of the middle of a full trail: the frame numbers of the keyframes are no longer consecutive, and on the
        # device kf_row is no longer the identity
        seen["removed_keyframe"] += len(kfs) == c["trail"] + 1 and any(a - b > 1 for a, b in zip(numbers, numbers[1:]))
    print(n, seen)
    for k, v in seen.items():
        assert v >= 0.01 * n, (k, v, n)
    # span 9 is never triangulated and span 10 always is: the threshold sits between them
    for c, ty, s, i, r, t in _points():
        if r["span"] in (9, 10):
            assert r["triangulated"] == (r["span"] == 10)
        if c["trail"] < 10:
            assert not r["triangulated"]


def test_restatement_and_truth_leave_at_most_one_percent_undecided():
    per_case = {}
    for c, ty, s, i, r, t in _points():
        a = per_case.setdefault(c["name"], [0, 0])
        a[0] += 1
        a[1] += F.undecided(r, t)
    print(per_case)
    for name, (n, und) in per_case.items():
        assert und <= 0.01 * n, (name, und, n)


def test_reused_distance_gives_the_same_record():
    """predict(distances = the distances of an earlier call) is what the device's reuse_distance = 1 is compared with."""
    c = F.case("stereo")
    s = 0
    n = int(c["table"]["n_tracks"][s])
    left = c["results"][F.LEFT][s][0]
    a = (c["finals"][s]["session"].ekfStateIndex, c["means"][s], c["par"], c["rcams"], F.STEREO, c["c0"][F.STEREO][s, :n], c["table"]["ids"][s, :n].tolist())
    again = F.predict(F64, *a, distances=[r["distance"] for r in left])
    for r, q in zip(c["results"][F.STEREO][s][0], again):
        assert r["c1"] == q["c1"] and r["distance"] == q["distance"]
