"""The numpy restatement of the FAST detector path (tests/fast_restatement.py) against hand-built images: the segment test at its
arc-length and threshold boundaries, both signs, the wrapped arc, the score's extremes, the 3-pixel border, the suppression of equal
neighbours, the asymmetric mask box, previous corners that draw nothing, images too small for a circle, and the tail's order."""
import os

import numpy as np
import pytest

import fast_cases as K
import fast_restatement as R


def _centre(img, t=10):
    return int(R.corner_scores(img, t)[K.C0, K.C0])


def test_segment_test_boundaries_and_scores():
    for name, (img, _, want) in K.hand_images(10).items():
        assert _centre(img) == want, name
    # an arc of exactly 9 is a corner and an arc of 8 is not, wherever it starts, for both signs
    for start in range(16):
        for val in (60, 140):
            assert _centre(K.arc(100, start, 9, val)) == 39 and _centre(K.arc(100, start, 8, val)) == 0
    # the score is the largest threshold that still passes
    img = K.arc(100, 2, 11, 77)
    assert _centre(img, 22) == 22 and _centre(img, 23) == 0 and _centre(img, 0) == 22
    assert _centre(K.patch(0, [255] * 16, bg=255), 254) == 254 and _centre(K.patch(0, [255] * 16, bg=255), 255) == 0


def test_keypoints_of_the_hand_images():
    imgs = K.hand_images(10)
    assert np.array_equal(R.keypoints(imgs["single_dot"][0]), [[K.C0, K.C0, 254]])
    assert len(R.keypoints(imgs["adjacent_equal"][0])) == 0          # two adjacent corners of equal score: both dropped
    assert len(R.keypoints(imgs["diagonal_equal"][0])) == 0
    kp = R.keypoints(imgs["arc9_dark"][0])
    assert kp.dtype == np.float32 and [K.C0, K.C0, 19] in kp.tolist()
    # unequal neighbours: the higher one stays
    img = K.dots(K.P, K.P, [(K.C0, K.C0)])
    img[K.C0, K.C0 + 1] = 200
    assert np.array_equal(R.keypoints(img), [[K.C0, K.C0, 254]])


def test_border_rows_and_columns():
    w, h = 20, 14
    inside = [(3, 3), (w - 4, 3), (3, h - 4), (w - 4, h - 4)]
    img = K.dots(w, h, inside + [(10, 2), (2, 7), (10, h - 3), (w - 3, 7)])      # the last four lie in the 3-pixel border
    kp = R.keypoints(img)
    assert np.array_equal(kp, [[3, 3, 254], [w - 4, 3, 254], [3, h - 4, 254], [w - 4, h - 4, 254]])      # row-major
    assert len(R.keypoints(np.random.default_rng(0).integers(0, 256, (40, 6), dtype=np.uint8))) == 0       # 6 x 40: no circle fits
    assert len(R.keypoints(np.random.default_rng(0).integers(0, 256, (6, 40), dtype=np.uint8))) == 0
    assert len(R.keypoints(np.random.default_rng(0).integers(0, 256, (7, 7), dtype=np.uint8), 0)) <= 1


def test_mask_box_is_asymmetric_and_out_of_range_corners_draw_nothing():
    w, h, r = 32, 32, 5
    img = K.dots(w, h, [(10, 10), (20, 10), (15, 5), (15, 15), (27, 27)])
    kp = R.keypoints(img)
    assert len(kp) == 5
    left = R.masked_sorted(kp, [[15.9, 10.2]], r, w, h)              # columns [10, 20), rows [5, 15)
    assert sorted(map(tuple, left[:, :2].tolist())) == [(15.0, 15.0), (20.0, 10.0), (27.0, 27.0)]
    m = R.draw_mask([[15.9, 10.2]], r, w, h)
    assert m[5:15, 10:20].all() and m.sum() == 100
    # clipped at the image: [max(ix - r, 0), min(ix + r, w - 1))
    m = R.draw_mask([[0.5, 30.5]], r, w, h)
    assert m[25:31, 0:5].all() and m.sum() == 30 and not m[31].any()
    assert not R.draw_mask(K.OUT_OF_RANGE_PREV(w, h), r, w, h).any()
    assert len(R.masked_sorted(kp, K.OUT_OF_RANGE_PREV(w, h), r, w, h)) == 5


def test_tail_is_a_stable_sort_and_a_greedy_walk():
    kp = np.array([[5, 1, 20], [9, 1, 30], [30, 2, 20], [5, 3, 30], [50, 9, 20], [7, 9, 30]], np.float32)
    srt = R.masked_sorted(kp, [], 3, 64, 64)
    assert srt[:, :2].tolist() == [[9, 1], [5, 3], [7, 9], [5, 1], [30, 2], [50, 9]]       # equal scores keep row-major order
    # dx*dx + dy*dy < r*r, strict: (9, 1) - (5, 3) is 20 < 25 apart, (9, 1) - (5, 1) is 16, (9, 1) - (9, 6) is exactly 25
    assert R.min_distance(srt[:, :2], 5, 200).tolist() == [[9, 1], [7, 9], [30, 2], [50, 9]]
    assert R.min_distance(np.array([[9, 1], [9, 6], [9, 5]], np.float32), 5, 200).tolist() == [[9, 1], [9, 6]]
    assert R.min_distance(srt[:, :2], 5, 2).tolist() == [[9, 1], [7, 9]]                    # stops at maxTracks
    corners, by = R.detect(K.dots(32, 32, [(10, 10), (20, 10)]), [[10.5, 10.5]], 2, 10, 200)
    assert corners.tolist() == [[20, 10]] and by.tolist() == [[20, 10, 254]]


def test_counts_on_a_seeded_noise_image_are_reproducible():
    # ties and key points at every scale: the properties the GPU comparison relies on, on an input small enough for every run
    img = np.random.default_rng(97 * 7 + 130).integers(0, 256, (130, 97), dtype=np.uint8)
    kp = R.keypoints(img)
    assert len(kp) > 300 and len(np.unique(kp[:, 2])) < len(kp)
    order = kp[:, 1] * 97 + kp[:, 0]
    assert (np.diff(order) > 0).all()
    xs, ys = kp[:, 0].astype(int), kp[:, 1].astype(int)
    occ = np.zeros((132, 99), bool)
    occ[ys + 1, xs + 1] = True
    nb = sum(occ[ys + 1 + dy, xs + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy)
    assert (nb == 0).all()                                           # suppressed key points are never 8-adjacent
    assert len(kp) <= ((97 - 6 + 1) // 2) * ((130 - 6 + 1) // 2)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fast_golden_opencv.npz")


def test_restatement_equals_the_opencv_fixture_when_there_is_one():
    """tests/golden/make_fast_golden_opencv.py writes the fixture where a cv2 exists; none has been available so far."""
    if not os.path.exists(GOLDEN):
        pytest.skip("no OpenCV fixture: the restatement is not pinned against OpenCV")
    g = np.load(GOLDEN)
    for name in g.files:
        if not name.startswith("img_"):
            continue
        tag = name[4:]
        img = g[name]
        h, w = img.shape
        for t in (10, 0, 40, 255):
            assert np.array_equal(R.keypoints(img, t), g[f"kp_{tag}_t{t}"]), (tag, t)
        if f"prev_{tag}" in g.files:
            kp = R.keypoints(img, 10)
            for r in (2, 7, 30):
                m = R.draw_mask(g[f"prev_{tag}"], r, w, h)
                assert np.array_equal(kp[~m[kp[:, 1].astype(int), kp[:, 0].astype(int)]], g[f"masked_{tag}_r{r}"]), (tag, r)
