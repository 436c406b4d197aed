"""The numpy restatement of the legacy GFTT detector (tests/gftt_legacy_restatement.py) on hand-built images: every rule of the
header's legacy GFTT section once, where its outcome can be read off the image; and OpenCV's grid walk against a brute-force walk on
the seeded images. No GPU. The restatement is written from the algorithm and is not pinned against an OpenCV build (none exists
here); what these tests pin is that it states the rules the device code is compared with."""
import numpy as np
import pytest

import gftt_legacy_cases as K
import gftt_legacy_restatement as R

f32 = np.float32
W, H = 96, 64


def _xy(c):
    return [(int(x), int(y)) for x, y in np.asarray(c)[:, :2]]


@pytest.mark.parametrize("name", sorted(K.hand_patches()))
def test_patches_give_their_candidates_in_order(name):
    patch, offs = K.hand_patches()[name]
    cand = R.candidates(K.embed(patch, 0, W, H, 40, 30))
    assert _xy(cand) == [(40 + dx, 30 + dy) for dx, dy in offs]
    if name.endswith("_equal"):                          # two equal adjacent maxima: both candidates, the later one first
        assert cand[0, 2] == cand[1, 2] and cand[0, 1] * W + cand[0, 0] > cand[1, 1] * W + cand[1, 0]


@pytest.mark.parametrize("name", sorted(K.border_images(W, H)))
def test_candidates_lie_inside_the_one_pixel_border(name):
    img, pts = K.border_images(W, H)[name]
    eig = R.response(img)
    cand = R.candidates(img, eig=eig)
    assert _xy(cand) == pts
    if not pts:
        # the maximum sits in the border row or column: it is no candidate, it sets the threshold and it suppresses its inner neighbour
        y, x = np.unravel_index(np.argmax(eig), eig.shape)
        assert x in (0, W - 1) or y in (0, H - 1)
        t, tv = R.threshold(eig, np.ones_like(eig, bool), 0.01)
        assert t == f32(np.float64(eig[y, x]) * 0.01)
        inner = (min(max(x, 1), W - 2), min(max(y, 1), H - 2))
        assert tv[inner[1], inner[0]] > 0 and tv[inner[1], inner[0]] < tv[y, x]


def test_mask_boxes_are_half_open_and_clipped_at_every_edge():
    w, h, r = 20, 16, 3
    inside = R.mask([[10.7, 8.2]], r, w, h)
    want = np.ones((h, w), bool)
    want[5:11, 7:13] = False                              # columns [7, 13), rows [5, 11): the upper ends are exclusive
    assert np.array_equal(inside, want)
    assert R.mask([[10.7, 8.2]], 1, w, h).sum() == w * h - 4
    lo = R.mask([[1.5, 1.5]], r, w, h)
    assert not lo[:4, :4].any() and lo.sum() == w * h - 16
    hi = R.mask([[18.5, 14.5]], r, w, h)                  # clipped at w - 1 and h - 1, exclusive: the last column and row stay unmasked
    assert not hi[11:15, 15:19].any() and hi.sum() == w * h - 16 and hi[:, 19].all() and hi[15, :].all()
    everything = R.mask([[10.0, 8.0]], 1000, w, h)
    assert not everything[:h - 1, :w - 1].any() and everything[h - 1, :].all() and everything[:, w - 1].all()
    # a track on px = 0 or py = h (or beyond, or NaN) draws nothing
    assert R.mask([[0.0, 5.0], [5.0, float(h)], [float(w), 5.0], [5.0, 0.0]], r, w, h).all()
    assert R.mask(K.OUT_OF_RANGE_PREV(w, h), r, w, h).all()
    with pytest.raises(AssertionError):
        R.mask([[5.0, 5.0]], 0, w, h)                     # the reference asserts maskRadius >= 1


def test_the_threshold_comes_from_the_unmasked_maximum_and_masked_pixels_still_suppress():
    ax, ay = 30, 20
    img, prev, r, q = K.masked_maximum(W, H, ax, ay)
    eig = R.response(img)
    m = R.mask(prev, r, W, H)
    y, x = np.unravel_index(np.argmax(eig), eig.shape)
    assert (x, y) == (ax, ay) and not m[ay, ax]          # the global maximum is masked
    t, tv = R.threshold(eig, m, q)
    assert t == f32(np.float64(eig[m].max()) * q) and eig[m].max() < eig[ay, ax]
    assert tv[ay, ax] == eig[ay, ax]                     # thresholding keeps the masked pixel
    weak = eig[ay + 10, ax + 15]
    assert t < weak < f32(np.float64(eig[ay, ax]) * q)   # a candidate only under the unmasked maximum's threshold
    assert m[ay, ax + 1] and tv[ay, ax + 1] > 0          # an unmasked neighbour above the threshold, suppressed by the masked pixel
    assert _xy(R.candidates(img, prev, r, 3, q, eig=eig)) == [(ax + 15, ay + 10)]
    assert _xy(R.candidates(img, (), 1, 3, q, eig=eig)) == [(ax, ay)]


def test_an_all_masked_image_has_threshold_zero_and_no_candidate():
    img = K.seeded_images(33, 33)[1]
    eig = R.response(img)
    t, tv = R.threshold(eig, np.zeros_like(eig, bool), 0.01)
    assert t == 0 and np.array_equal(tv, np.where(eig > 0, eig, 0))
    assert len(R.candidates_of(eig, np.zeros_like(eig, bool))) == 0
    # through drawMask the last row and column stay unmasked, and they hold no candidate
    c, v, cand = R.detect(img, [[16.0, 16.0]], 1000)
    assert len(cand) == 0 and len(c) == 0 and len(v) == 0


def test_negative_responses_above_a_negative_threshold_are_candidates():
    eig = np.full((7, 9), -4.0, f32)
    eig[3, 3], eig[3, 6], eig[0, 0] = -1.0, -1.5, -0.5
    m = np.ones_like(eig, bool)
    t, tv = R.threshold(eig, m, 3.0)                      # maxVal = -0.5, t = -1.5: -1 passes, -1.5 and -4 become 0
    assert t == f32(-1.5) and tv[3, 3] == -1 and tv[3, 6] == 0 and tv[1, 1] == 0
    assert len(R.candidates_of(eig, m, 3.0)) == 0         # the zeros around it are larger: it is no local maximum
    eig[2:5, 2:5] = -1.0
    assert _xy(R.candidates_of(eig, m, 3.0)) == [(3, 3)]  # ... but inside a plateau of its own value it is


def test_the_distance_test_is_strict_against_the_binary64_square():
    img, md, pts = K.distance_pairs(W, H, 20, 20)
    assert R.scaled_min_distance(W, H, md) == 6.5
    c, v, cand = R.detect(img, gftt_min_distance=md)
    assert len(cand) == 4 and _xy(c) == list(pts)        # 41 < 42.25 rejected, 45 accepted
    assert list(v) == [cand[i, 2] for i in (0, 2, 3)]
    two = np.array([[10, 10, 2.0], [13, 14, 1.0]], f32)  # squared distance 25
    assert list(R.walk_grid(two, W, H, 5.0, 10)) == [0, 1] and list(R.walk_brute(two, 5.0, 10)) == [0, 1]         # 25 < 25 is false
    assert list(R.walk_grid(two, W, H, 5.000001, 10)) == [0] and list(R.walk_brute(two, 5.000001, 10)) == [0]
    # minDistance < 1: every candidate in order; the cap cuts either branch
    assert list(R.walk_grid(two, W, H, 0.99, 10)) == [0, 1] and list(R.walk_grid(two, W, H, 0.0, 1)) == [0]
    assert _xy(R.detect(img, gftt_min_distance=0.0)[0]) == _xy(cand)
    assert _xy(R.detect(img, gftt_min_distance=md, max_tracks=2)[0]) == list(pts[:2])
    assert _xy(R.detect(img, gftt_min_distance=0.0, max_tracks=3)[0]) == _xy(cand[:3])


@pytest.mark.parametrize("size", [(33, 33), (97, 130), (752, 480)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_grid_walk_equals_the_brute_force_walk_on_the_seeded_images(size):
    w, h = size
    counts = {(752, 480): (19575, 23936, 24201)}.get(size)
    for k, img in enumerate(K.seeded_images(w, h)):
        cand = R.candidates(img)
        if counts:
            assert len(cand) == counts[k]
        else:
            assert (57 <= len(cand) <= 68) if w == 33 else (658 <= len(cand) <= 853)
        assert (np.diff(cand[:, 2]) <= 0).all()
        ties = np.nonzero(np.diff(cand[:, 2]) == 0)[0]
        idx = cand[:, 1] * w + cand[:, 0]
        assert (idx[ties] > idx[ties + 1]).all()
        if size == (752, 480) and k == 2:
            assert len(ties) > 1000                      # the seeded inputs exercise the tie rule themselves
        for md, cap in ((50.0, 200), (7.3, 4096), (0.0, 4096), (50.0, 4096)):
            if size == (752, 480) and k != (0 if md == 50.0 else 1):
                continue
            d = R.scaled_min_distance(w, h, md)
            assert np.array_equal(R.walk_grid(cand, w, h, d, cap), R.walk_brute(cand, d, cap)), (k, md, cap)
