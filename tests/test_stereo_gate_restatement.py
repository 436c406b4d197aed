"""CPU checks that pin the numpy restatement of the stereo track gate (tests/stereo_gate_restatement.py) on hand-built cases:
the strict distance tests of withinDistanceFromCurve, empty curves, the merge / crop / blacklist order of
TrackerImplementation::track and the detection filter of detectFeatures."""
import numpy as np

import stereo_gate_restatement as G

f32 = np.float32
W, H = 752, 480


def _curve(*pts):
    return [(f32(x), f32(y)) for x, y in pts]


def _baseline(bx=-0.1, by=0.0):
    T = np.eye(4)
    T[0, 3], T[1, 3] = bx, by
    return T


def _pinhole(oracle):
    return oracle.Camera("pinhole", 400.0, 400.0, 376.0, 240.0)


def test_epipolar_distance_and_flow_status():
    dist, dist2 = G.epipolar_dist(W, H, 10.0)
    assert dist == f32(f32(10 * 480) / f32(720)) == f32(6.6666665) and dist2 == dist * dist and dist2.dtype == np.float32
    xy = np.array([[0, 0], [-1e-7, 5], [751.99994, 479.99997], [752, 10], [10, 480], [np.nan, 3], [5, 5], [760, 5]], np.float32)
    lk = np.array([1, 1, 1, 1, 1, 1, 0, 0], np.uint8)
    assert G.flow_status(lk, xy, W, H).tolist() == [0, 4, 0, 4, 4, 0, 2, 4]           # NaN: no comparison holds


def test_vertex_and_segment_interior():
    curve = _curve((0, 0), (10, 0), (100, 0))
    assert G.within_distance_from_curve((10, 0), curve, f32(1))[0]                   # on a vertex
    assert G.within_distance_from_curve((55, 3), curve, f32(16))[0]                  # on the interior of the (10, 0)-(100, 0) segment
    assert not G.within_distance_from_curve((55, 5), curve, f32(16))[0]


def test_the_comparison_is_strict_at_dist2():
    curve = _curve((0, 0), (-200, 0))
    p = (3, 4)                                                                        # squared distance 25 exactly, t < 0 on the segment
    assert not G.within_distance_from_curve(p, curve, f32(25))[0]
    assert G.within_distance_from_curve(p, curve, np.nextafter(f32(25), f32(np.inf)))[0]
    assert not G.within_distance_from_curve(p, curve, np.nextafter(f32(25), f32(0)))[0]
    # the segment residual: (50, 3) against (0, 0)-(100, 0) leaves exactly 9
    seg = _curve((0, 0), (100, 0))
    assert not G.within_distance_from_curve((50, 3), seg, f32(9))[0]
    assert G.within_distance_from_curve((50, 3), seg, np.nextafter(f32(9), f32(np.inf)))[0]


def test_segment_ends_t_zero_and_one_take_the_vertex_answer():
    seg = _curve((0, 0), (100, 0))
    for p in ((0, 2), (100, 2)):                                                    # t == 0 and t == 1 exactly: not a segment hit
        assert not G.within_distance_from_curve(p, seg, f32(4))[0]
        assert G.within_distance_from_curve(p, seg, np.nextafter(f32(4), f32(np.inf)))[0]   # the vertex test decides


def test_zero_length_segment_fails_quietly():
    curve = _curve((5, 5), (5, 5), (5, 5))
    within, margin = G.within_distance_from_curve((5, 7), curve, f32(1))
    assert not within and margin > 0
    assert G.within_distance_from_curve((5, 5.5), curve, f32(1))[0]


def test_the_curve_of_a_horizontal_baseline(oracle):
    cam = _pinhole(oracle)
    curve, _ = G.epipolar_curve((300.5, 200.25), cam, cam, _baseline())
    assert len(curve) == 8
    ys = [float(y) for _, y in curve]
    xs = [float(x) for x, _ in curve]
    assert max(abs(y - 200.25) for y in ys) < 1e-3 and all(a < b for a, b in zip(xs, xs[1:]))   # disparity falls with depth
    assert abs(xs[0] - (300.5 - 400 * 0.1 / (0.5 * _ray_z(cam, 300.5, 200.25)))) < 1e-3


def _ray_z(cam, x, y):
    return cam.pixel_to_ray(x, y)[1][2]


def test_empty_curves_keep_the_track(oracle):
    cam = _pinhole(oracle)
    behind = np.diag([-1.0, 1.0, -1.0, 1.0])                                           # camera 1 looks the other way
    prm = G.Params(cam0ToCam1=behind)
    far = np.array([[100.0, 100.0]], np.float32)
    assert G.track_gate([[300, 200]], far, [0], None, [0], cam, cam, W, H, prm).tolist() == [G.TRACKED]
    # fisheye pixelToRay fails beyond the valid field of view (fisheyeCamera off: no crop mark)
    fish = oracle.Camera("fisheye", 300.0, 301.0, 376.0, 240.0, coeffs=(0.02, -0.01, 0.003, -0.0005), max_valid_fov_deg=100.0)
    assert not fish.pixel_to_ray(2.0, 2.0)[0]
    assert G.track_gate([[2, 2]], far, [0], None, [0], fish, fish, W, H, G.Params(cam0ToCam1=_baseline())).tolist() == [G.TRACKED]
    assert G.track_gate([[2, 2]], far, [0], None, [0], fish, fish, W, H,
                        G.Params(cam0ToCam1=_baseline(), fisheyeCamera=True)).tolist() == [G.OUT_OF_RANGE]


def test_merge_epipolar_crop_and_blacklist_order(oracle):
    cam = _pinhole(oracle)
    prm = G.Params(cam0ToCam1=_baseline(), partOfImageToDetectFeatures=0.8)
    left = np.array([[300, 200], [300, 200], [300, 200], [30, 200], [30, 200], [300, 200], [300, 200]], np.float32)
    right = left - np.array([20, 0], np.float32)                                      # on the curve (20 px disparity)
    right[2, 1] += 30                                                                 # off the curve
    track = [0, 0, 0, 2, 0, 0, 0]
    stereo = [4, 2, 0, 0, 0, 0, 0]
    black = [0, 0, 0, 0, 1, 0, 0]
    right[5, 0] = 700                                                                 # right corner outside the crop
    right[6] = [280, 235]                                                             # 35 px below the curve
    out = G.track_gate(left, right, stereo, black, track, cam, cam, W, H, prm)
    assert out.tolist()[:6] == [G.TRACKED,                 # a stereo FLOW_OUT_OF_RANGE is not merged
                                G.FAILED_FLOW,             # a stereo FAILED_FLOW is
                                G.FAILED_EPIPOLAR_CHECK,
                                G.OUT_OF_RANGE,            # the crop overwrites FAILED_FLOW
                                G.BLACKLISTED,             # the blacklist comes last
                                G.OUT_OF_RANGE]            # the right crop
    assert out[6] == G.FAILED_EPIPOLAR_CHECK
    # only TRACKED features take the epipolar check: an already failed one keeps its status
    assert G.track_gate(left[2:3], right[2:3], [0], None, [3], cam, cam, W, H, prm).tolist() == [3]


def test_independent_stereo_flow_skips_the_check_in_the_gate_only(oracle):
    cam = _pinhole(oracle)
    prm = G.Params(cam0ToCam1=_baseline(), independentStereoOpticalFlow=True)
    left = np.array([[300, 200]], np.float32)
    right = np.array([[280, 260]], np.float32)
    assert G.track_gate(left, right, [0], None, [0], cam, cam, W, H, prm).tolist() == [G.TRACKED]
    kept, kept_r, st = G.detection_filter(left, right, [0], cam, cam, W, H, prm)
    assert st.tolist() == [G.FAILED_EPIPOLAR_CHECK] and len(kept) == 0 and len(kept_r) == 0
    off = G.Params(cam0ToCam1=_baseline(), maxStereoEpipolarDistance=0.0)             # <= 0 switches the check off everywhere
    assert G.track_gate(left, right, [0], None, [0], cam, cam, W, H, off).tolist() == [G.TRACKED]
    assert G.detection_filter(left, right, [0], cam, cam, W, H, off)[2].tolist() == [G.TRACKED]


def test_detection_filter_keeps_the_input_order(oracle):
    cam = _pinhole(oracle)
    prm = G.Params(cam0ToCam1=_baseline(), partOfImageToDetectFeatures=0.9)
    rng = np.random.default_rng(3)
    left = rng.uniform([0, 0], [W, H], (60, 2)).astype(np.float32)
    right = left - np.array([20, 0], np.float32)
    right[::7, 1] += 40                                                               # epipolar failures
    stereo = rng.choice([0, 0, 0, 2, 4], 60).astype(np.int32)
    kept, kept_r, st = G.detection_filter(left, right, stereo, cam, cam, W, H, prm)
    idx = np.nonzero(st == G.TRACKED)[0]
    assert np.array_equal(kept, left[idx]) and np.array_equal(kept_r, right[idx]) and list(idx) == sorted(idx)
    assert {G.TRACKED, G.FAILED_FLOW, G.FLOW_OUT_OF_RANGE, G.OUT_OF_RANGE, G.FAILED_EPIPOLAR_CHECK} <= set(st.tolist())
    # mono: every status starts TRACKED, only the left crop applies
    kept_m, none, st_m = G.detection_filter(left, None, None, cam, None, W, H, prm)
    assert none is None and set(st_m.tolist()) <= {G.TRACKED, G.OUT_OF_RANGE}
    assert np.array_equal(kept_m, left[st_m == G.TRACKED])
