"""CPU checks of the dense-stereo restatement (tests/stereo_bm_restatement.py), the spec of hybvio_amd/csrc/stereo_bm.hip: known
answers of the prefilter, the box-sum SAD against a brute-force window, a noise-free shift, the per-pixel decision on crafted sad
vectors, the speckle rules, the depth and cloud rules, and the conditions the shared scenes (tests/stereo_bm_cases.py) must meet
so that the GPU tests exercise every rule. The restatement is not pinned against an OpenCV build; the fixture test at the end
skips until tests/golden/make_stereo_bm_golden_opencv.py has been run on a machine that has cv2."""
import os

import numpy as np
import pytest

import stereo_bm_cases as K
import stereo_bm_restatement as R

F = R.FILTERED
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stereo_bm_golden_opencv.npz")


def test_num_disparities_in_binary32():
    assert [R.num_disparities(w) for w in (752, 1280, 320, 160)] == [96, 128, 32, 32]


def test_prefilter_known_answers():
    c = 31
    assert (R.prefilter(np.full((12, 20), 93, np.uint8), c) == c).all()
    for s in (1, 2, 3):
        ramp = np.tile((10 + s * np.arange(20)).astype(np.uint8), (12, 1))
        out = R.prefilter(ramp, c)
        assert (out[:, 1:-1] == c + 8 * s).all() and (out[:, 0] == c).all() and (out[:, -1] == c).all()
    steep = np.tile((5 * np.arange(20)).astype(np.uint8), (12, 1))              # 8 * 5 > 31: saturates
    assert (R.prefilter(steep, c)[:, 1:-1] == 2 * c).all() and (R.prefilter(steep[:, ::-1], c)[:, 1:-1] == 0).all()
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (11, 16)).astype(np.uint8)                        # odd height
    out = R.prefilter(img, c)
    assert (out[10] == c).all() and (out[:, 0] == c).all() and (out[:, 15] == c).all()
    a = img.astype(int)
    # row 0 mirrors to row 1 (not to itself): S = 2 * (row 1) + 2 * (row 0)
    s0 = 2 * (a[1, 6] - a[1, 4]) + 2 * (a[0, 6] - a[0, 4])
    assert out[0, 5] == np.clip(s0, -c, c) + c
    even = R.prefilter(img[:10], c)                                              # even height: the last row mirrors to row H - 2
    s9 = 2 * (a[8, 6] - a[8, 4]) + 2 * (a[9, 6] - a[9, 4])
    assert even[9, 5] == np.clip(s9, -c, c) + c
    s4 = (a[3, 6] - a[3, 4]) + 2 * (a[4, 6] - a[4, 4]) + (a[5, 6] - a[5, 4])
    assert out[4, 5] == even[4, 5] == np.clip(s4, -c, c) + c


def test_box_sum_sad_equals_a_brute_force_window():
    w, h, nd = K.SHAPES[0]
    l, r = K.scenes(w, h, nd)[0]
    lp, rp = R.prefilter(l), R.prefilter(r)
    sad = R.sad_volume(lp, rp, nd)
    x0, x1, y0, y1 = R.valid_rect(w, h, nd)
    assert sad.shape == (nd, y1 - y0, x1 - x0) and (x0, x1, y0, y1) == (41, 150, 10, 86)
    rng = np.random.default_rng(1)
    L, Rr = lp.astype(int), rp.astype(int)
    for _ in range(40):
        x, y, d = rng.integers(x0, x1), rng.integers(y0, y1), rng.integers(0, nd)
        brute = np.abs(L[y - 10:y + 11, x - 10:x + 11] - Rr[y - 10:y + 11, x - 10 - d:x + 11 - d]).sum()
        assert sad[d, y - y0, x - x0] == brute
    assert R.valid_rect(64, 64, 64)[0] >= R.valid_rect(64, 64, 64)[1]            # empty
    assert (R.block_match(l[:64, :64], r[:64, :64], K.params_for(64, 64)) == F).all()


def test_a_noise_free_integer_shift_is_found_within_half_a_pixel():
    # with a perfect match m = 0, so dd = p + n + |p - n| = 2 max(p, n) and |(p - n) * 256 / dd| <= 128: |D - 16 d0| <= 8
    rng = np.random.default_rng(2)
    w, h, nd, d0 = 160, 64, 32, 9
    tex = (K._smooth(rng, h, w + 2 * nd) * 255).astype(np.uint8)
    left, right = tex[:, nd:nd + w], tex[:, nd + d0:nd + d0 + w]                 # right(x) = left(x + d0)
    d = R.block_match(left, right, K.params_for(w, nd))
    keep = d != F
    assert keep.sum() > 500 and (np.abs(d[keep].astype(int) - 16 * d0) <= 8).all()


def _decide(sad_by_k, text=100, **kw):
    sk = np.asarray(sad_by_k)
    return int(R.decide(sk[::-1].reshape(-1, 1), np.array([text]), len(sk), **kw)[0])


def test_the_decision_on_crafted_sad_vectors():
    nd = 16
    base = np.full(nd, 1000)
    v = base.copy(); v[5] = v[6] = 100                     # a tie of neighbours: the first k wins, so the larger disparity d = nd - 1 - 5
    # mink = 5, p = sad[6] = 100, n = sad[4] = 1000: dd = 900 + 900, quotient -900 * 256 / 1800 = -128
    assert _decide(v) == ((nd - 5 - 1) * 256 - 128 + 15) >> 4
    v = base.copy(); v[0] = 100; v[1] = 400                # mink = 0: sad[-1] = sad[1], so p = n and the quotient is 0
    assert _decide(v) == ((nd - 1) * 256 + 15) >> 4
    v = base.copy(); v[nd - 1] = 100; v[nd - 2] = 400      # mink = nd - 1: sad[nd] = sad[nd - 2]; disparity 0
    assert _decide(v) == (0 * 256 + 15) >> 4 == 0
    assert _decide(np.full(nd, 50)) == F                   # every value equal: rivals everywhere
    v = base.copy(); v[0] = v[1] = 10                      # dd = 0: mink = 0, p = n = sad[1] = m, no sub-pixel term
    assert _decide(v) == ((nd - 0 - 1) * 256 + 0 + 15) >> 4
    # (p - n) * 256 / dd is C's division, toward zero. dd = 2 max(p, n) - 2 m is even, so -256 / 3 itself cannot occur in a sad
    # vector; the rule is stated on the division, and on a vector with -1792 / 38 = -47 (floor would give -48, and another value)
    num, den = -256, 3
    assert int(np.sign(num) * (abs(num) // den)) == -85 and num // den == -86
    v = base.copy(); v[8] = 10; v[9] = 22; v[7] = 29       # m = 10, p = 22, n = 29: dd = 51 - 20 + 7 = 38
    assert _decide(v) == ((nd - 8 - 1) * 256 - 47 + 15) >> 4 == 110 and ((nd - 8 - 1) * 256 - 48 + 15) >> 4 == 109
    v = base.copy(); v[8] = 10; v[9] = 29; v[7] = 22       # the positive quotient: +47
    assert _decide(v) == ((nd - 8 - 1) * 256 + 47 + 15) >> 4
    # thresh for m = 7 is 7 + 7 * 15 / 100 = 8
    v = base.copy(); v[4] = 7; v[10] = 8
    assert _decide(v) == F                                 # a rival at 8 <= thresh
    v[10] = 9
    assert _decide(v) != F
    v = base.copy(); v[4] = 7; v[5] = 7                    # a rival at distance 1 is ignored ...
    assert _decide(v) != F
    v = base.copy(); v[4] = 7; v[6] = 7                    # ... one at distance 2 is not
    assert _decide(v) == F
    v = base.copy(); v[4] = 7
    assert _decide(v, text=9) == F and _decide(v, text=10) != F                  # textsum < textureThreshold


def test_speckle_rules():
    m = np.full((48, 64), F, np.int16)
    m[1:11, 2:52] = 200                                    # 500 pixels: removed
    m[20:30, 2:52] = 300; m[30, 2] = 300                   # 501: kept
    out = R.filter_speckles(m, F, 500, 10)
    assert (out == 200).sum() == 0 and (out == 300).sum() == 501
    b = np.full((48, 64), F, np.int16)
    b[0:10, 0:30] = 50; b[0:10, 30:60] = 60                # a difference of 10 joins: 600
    b[20:30, 0:30] = 50; b[20:30, 30:60] = 61              # 11 does not: 300 + 300
    out = R.filter_speckles(b, F, 500, 10)
    assert (out[0:10] != F).sum() == 600 and (out[20:30] != F).sum() == 0
    c = np.full((48, 64), F, np.int16)                     # a - b and b - c join, a - c would not: still one component
    c[5:15, 0:20] = 0; c[5:15, 20:40] = 10; c[5:15, 40:60] = 20
    labels, sizes = R.components(c, F, 10)
    assert len(sizes) == 1 and sizes[0] == 600 and (R.filter_speckles(c, F, 500, 10) == c).all()
    s = np.full((30, 40), F, np.int16)                     # a serpentine: one component however it is visited
    for i, y in enumerate(range(0, 30, 2)):
        s[y, :] = 100
        if y + 2 < 30:
            s[y + 1, 39 if i % 2 == 0 else 0] = 100
    labels, sizes = R.components(s, F, 10)
    assert len(sizes) == 1 and sizes[0] == (s != F).sum() > 500
    assert (R.filter_speckles(s, F, 500, 10) == s).all() and (R.filter_speckles(s, F, int(sizes[0]), 10) == F).all()
    assert (R.filter_speckles(np.full((5, 5), F, np.int16)) == F).all()


def test_depth_and_cloud_rules():
    w, h = 40, 30
    q = K.q_matrix(w, h, angle=0.0)
    disp = np.full((h, w), F, np.int16)
    disp[10, 7] = 64; disp[0, 0] = 32; disp[5, 5] = 15; disp[5, 6] = 16
    assert R.get_depth(q, disp, 7.9, 10.9) > 0 and R.get_depth(q, disp, 8.0, 10.0) == -1       # int(): toward zero
    assert R.get_depth(q, disp, -0.5, -0.9) > 0 and R.get_depth(q, disp, -1.0, 0) == -1
    assert R.get_depth(q, disp, 5, 5) == -1 and R.get_depth(q, disp, 6, 5) > 0                 # val = 15 / 16 rejected, 1 accepted
    assert R.get_depth(q, disp, w, 5) == -1 and R.get_depth(q, disp, 5, h) == -1
    for bad in (np.nan, np.inf, -np.inf, 3e9):
        assert R.get_depth(q, disp, bad, 5) == -1 and R.get_depth(q, disp, 5, bad) == -1
    # the value: z = f Tx' / d with this Q (w = -val / Tx), depth = the norm of the reprojected point
    f32 = np.float32
    qf = q.astype(np.float32)
    val = f32(4.0)
    pos = np.array([f32(7) + qf[0, 3], f32(10) + qf[1, 3], qf[2, 3]], np.float32) / f32(qf[3, 2] * val)
    assert np.isclose(R.get_depth(q, disp, 7.5, 10.5), np.linalg.norm(pos.astype(np.float64)), rtol=1e-6)
    # the cloud: row-major order, the disparity test, the squared-norm-below-1 skip
    disp = np.full((h, w), F, np.int16)
    disp[0, 5] = 64; disp[0, 35] = 48; disp[10, 0] = 32; disp[10, 10] = 15; disp[10, 11] = 4000; disp[25, 20] = 16 * 30
    cloud = R.point_cloud(q, disp, 5)
    near = R._project(qf, 20, 25, f32(30))
    assert (near ** 2).sum() < 1                           # closer than MIN_DEPTH: skipped
    assert len(cloud) == 3                                  # (10, 11) is off the stride-5 grid, (10, 10) fails the disparity test
    assert np.array_equal(cloud[0], R._project(qf, 5, 0, f32(4))) and np.array_equal(cloud[1], R._project(qf, 35, 0, f32(3)))
    assert np.array_equal(cloud[2], R._project(qf, 0, 10, f32(2)))
    assert R.cloud_bound(w, h, 5) == 8 * 6 and R.cloud_bound(161, 97, 5) == 33 * 20


@pytest.mark.parametrize("shape", K.SHAPES, ids=K.IDS)
def test_the_shared_scenes_fire_every_rule(shape):
    w, h, nd = shape
    x0, x1, y0, y1 = R.valid_rect(w, h, nd)
    for k in range(len(K.SEEDS)):
        d0, _ = K.expected(w, h, nd, k, False)
        d1, st = K.expected(w, h, nd, k, True)
        assert st["texture"] > 0 and st["uniqueness"] > 0 and st["tie"] > 0 and st["negative_quotient"] > 0, st
        assert st["small_components"] > 0 and st["speckle_pixels"] > 0 and st["large_components"] >= 1, st
        assert (d0 != F).sum() - (d1 != F).sum() == st["speckle_pixels"]
        assert (d1 != F).sum() >= 0.25 * (x1 - x0) * (y1 - y0)
        assert (d1[:y0] == F).all() and (d1[y1:] == F).all() and (d1[:, :x0] == F).all() and (d1[:, x1:] == F).all()
    assert not np.array_equal(K.scenes(w, h, nd)[0][0], K.scenes(w, h, nd)[1][0])


def test_the_restatement_equals_the_opencv_fixture():
    if not os.path.exists(GOLDEN):
        pytest.skip("no OpenCV fixture: run tests/golden/make_stereo_bm_golden_opencv.py where cv2 is installed")
    g = np.load(GOLDEN)
    for i in range(len(g["nd"])):
        p = K.params_for(g[f"left_{i}"].shape[1], int(g["nd"][i]))
        assert np.array_equal(R.compute_disparity(g[f"left_{i}"], g[f"right_{i}"], p), g[f"disp_{i}"]), i
