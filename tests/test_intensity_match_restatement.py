"""tests/intensity_match_restatement.py against hand computation, Python big integers and the rules of
src/tracker/util.cpp:16-52,173-179 and src/commandline/main.cpp:763-777 -- and the condition the GPU tests rest on: on every fixture
they use, every in-range entry of every reference table keeps at least 1e-9 from a rounding boundary, so that a last-bit difference
of the device's k (4 ulp move an entry by at most 255 * 4 * 2^-52 ~ 2e-13) cannot flip a pixel. No GPU."""
import math

import numpy as np
import pytest

import intensity_match_cases as K
import intensity_match_restatement as R


def test_hand_computed_2x3_example():
    img = np.array([[10, 20, 30], [40, 50, 60]], np.uint8)
    s, sq = R.sums(img)
    assert (s, sq) == (210, 9100)
    mean, std0 = R.mean_std_dev(s, sq, 6)
    assert abs(mean - 35.0) < 1e-13 and abs(std0 - math.sqrt(9100 / 6 - 35 * 35)) < 1e-13
    # target: mean 100, twice the deviation: k = 2 exactly, mean0 = 210 * 2 / 6 = 70, v = 2 x + 100 - 70
    out, (T, k, mean0, m, v) = R.set_intensities(img, 100.0, 2 * std0, 1.0)
    assert k == 2.0 and mean0 == 70.0 and m == 100.0
    assert np.array_equal(out, [[50, 70, 90], [110, 130, 150]])
    assert np.array_equal(v[:3], [30.0, 32.0, 34.0]) and T[0] == 30 and T[112] == 254 and T[113] == 255 and T[255] == 255
    # weight 0.5: stddev = 1.5 std0, k = 1.5, mean0 = 52.5, mean = 52.5 + 0.5 (100 - 52.5) = 76.25, v = 1.5 x + 23.75
    out, (T, k, mean0, m, v) = R.set_intensities(img, 100.0, 2 * std0, 0.5)
    assert k == 1.5 and mean0 == 52.5 and m == 76.25
    assert np.array_equal(out, [[39, 54, 69], [84, 99, 114]])                # 38.75, 53.75, 68.75, 83.75, 98.75, 113.75
    # matchIntensities: r takes l's statistics
    l = (2 * img.astype(np.int32) + 30).astype(np.uint8)
    assert np.array_equal(R.match_intensities(l, img), l)


def test_round_is_half_away_from_zero():
    assert [R.c_round(x) for x in (0.5, 1.5, 2.5, -0.5, -1.5, 0.49999999999999994, 254.5, -0.4)] == [1, 2, 3, -1, -2, 0, 255, 0]
    # k = 0.5 and mean = mean0 = 1 exactly: v = x / 2, odd bytes sit on a boundary and go up (rint would send 2.5 to 2)
    img = np.array([[0, 4]], np.uint8)
    std0 = R.mean_std_dev(4, 16, 2)[1]
    T, k, mean0, m, v = R.table(4, 16, 2, 1.0, 0.5 * std0, 1.0)
    assert k == 0.5 and mean0 == 1.0 and m == 1.0 and v[5] == 2.5
    assert list(T[:8]) == [0, 1, 1, 2, 2, 3, 3, 4]
    assert R.boundary_distance(v) == 0.0


def test_statistics_against_python_big_integers():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (61, 83), dtype=np.uint8)
    flat = [int(x) for x in img.ravel()]
    assert R.sums(img) == (sum(flat), sum(x * x for x in flat))
    white = np.full((300, 300), 255, np.uint8)                                # sums beyond 32 bits
    assert R.sums(white) == (255 * 90000, 255 * 255 * 90000) and R.sums(white)[1] > 2 ** 32
    # the sums of a matched image follow from the histogram and the table
    T = R.table(*R.sums(img), img.size, 100.0, 30.0, 1.0)[0]
    hist = np.bincount(img.ravel(), minlength=256)
    assert R.sums(T[img]) == (sum(int(hist[v]) * int(T[v]) for v in range(256)), sum(int(hist[v]) * int(T[v]) ** 2 for v in range(256)))
    mean, std = R.mean_std_dev(*R.sums(img), img.size)
    f = img.astype(np.float64)
    assert abs(mean - f.mean()) < 1e-10 and abs(std - f.std()) < 1e-10


def _pair(name="97x131_both", f=0, s=0):
    L, Rt = K.frames(name)[f]
    return L[s], Rt[s]


def test_first_frame_is_the_identity_and_prev_is_the_matched_frame():
    frames = [K.frames("recursion_w025")[f][0][0] for f in range(3)]
    seq = R.Sequence()
    out, _, rec = seq.frame(frames[0], None, 0.25, False)
    assert np.array_equal(out, frames[0]) and rec.k[0] == 1.0 and rec.flags == R.MATCHED_LEFT     # main.cpp:766: prev = the frame itself
    assert (seq.prev_sum, seq.prev_sqsum, seq.has_prev) == (*R.sums(frames[0]), 1)
    out1, _, rec1 = seq.frame(frames[1], None, 0.25, False)
    assert not np.array_equal(out1, frames[1])
    assert (seq.prev_sum, seq.prev_sqsum) == R.sums(out1) != R.sums(frames[1])                    # :768: the MATCHED frame
    assert (rec1.out_sum[0], rec1.out_sqsum[0]) == R.sums(out1) and (rec1.in_sum[0], rec1.in_sqsum[0]) == R.sums(frames[1])
    # the third frame is matched against the matched second one
    want = R.set_intensities(frames[2], *R.mean_std_dev(*R.sums(out1), out1.size), 0.25)[0]
    raw = R.set_intensities(frames[2], *R.mean_std_dev(*R.sums(frames[1]), out1.size), 0.25)[0]
    out2 = seq.frame(frames[2], None, 0.25, False)[0]
    assert np.array_equal(out2, want) and not np.array_equal(out2, raw)


@pytest.mark.parametrize("w", [0.25, 1.0])
def test_weights_quarter_and_one(w):
    l, r = _pair("97x131_stereo", 0, 2)                                       # gain 0.55, offset 40
    ml, sl = R.mean_std_dev(*R.sums(l), l.size)
    mr, sr = R.mean_std_dev(*R.sums(r), r.size)
    out, (_, k, mean0, _, _) = R.set_intensities(r, ml, sl, w)
    mo, so = R.mean_std_dev(*R.sums(out), out.size)
    # the deviation moves the share w of the way; the mean is blended from mean0 = k * (the input's mean) (util.cpp:41-42), not
    # from the input's mean -- the reference's arithmetic, restated as it is. Up to the rounding to bytes:
    assert abs(k - (sr + w * (sl - sr)) / sr) < 1e-12 and abs(mean0 - k * mr) < 1e-9
    assert abs(so - (sr + w * (sl - sr))) < 0.5 and abs(mo - ((1 - w) * k * mr + w * ml)) < 0.5
    assert abs(ml - mr) > 5 and abs(sl - sr) > 5
    if w == 1.0:
        assert np.array_equal(out, R.match_intensities(l, r))


def test_stereo_step_sees_the_matched_left_frame():
    seq = R.Sequence()
    l0, r0 = _pair(f=0)
    l1, r1 = _pair(f=1)
    seq.frame(l0, r0, 0.5, True)
    ol, or_, rec = seq.frame(l1, r1, 0.5, True)
    assert rec.flags == R.MATCHED_LEFT | R.MATCHED_RIGHT and not np.array_equal(ol, l1)
    assert np.array_equal(or_, R.match_intensities(ol, r1)) and not np.array_equal(or_, R.match_intensities(l1, r1))
    # options off: nothing happens, nothing is remembered
    seq = R.Sequence()
    ol, or_, rec = seq.frame(l1, r1, 0.0, False)
    assert ol is l1 and or_ is r1 and rec.flags == 0 and seq.has_prev == 0
    ol, or_, rec = seq.frame(l1, None, 0.0, True)                             # mono: useStereo is false
    assert rec.flags == 0


def test_constant_image_rule():
    flat = np.full((5, 7), 93, np.uint8)
    l, r = _pair("5x7_both")
    out, info = R.set_intensities(flat, 100.0, 20.0)
    assert info is None and np.array_equal(out, flat)
    seq = R.Sequence()
    ol, or_, rec = seq.frame(flat, r, 0.5, True)
    assert rec.flags == R.CONSTANT_LEFT | R.MATCHED_RIGHT and np.array_equal(ol, flat)
    assert (seq.prev_sum, seq.prev_sqsum, seq.has_prev) == (93 * 35, 93 * 93 * 35, 1)             # still the prev statistics
    assert np.array_equal(or_, flat)                                          # target deviation 0: k = 0, every pixel round(mean)
    ol, or_, rec = seq.frame(l, flat, 0.5, True)
    assert rec.flags == R.MATCHED_LEFT | R.CONSTANT_RIGHT and np.array_equal(or_, flat) and rec.k[1] == 1.0
    flags = [[r.flags for r in e.records] for e in K.expected("special")]
    assert flags[0] == [R.CONSTANT_LEFT | R.MATCHED_RIGHT, R.MATCHED_LEFT | R.CONSTANT_RIGHT, R.MATCHED_LEFT | R.MATCHED_RIGHT]
    assert all(r.flags == R.CONSTANT_LEFT | R.CONSTANT_RIGHT for e in K.expected("one_pixel") for r in e.records)


def test_clamping_at_both_ends():
    (L, Rt), e = K.frames("clamp")[0], K.expected("clamp")[0]
    low = high = 0
    for s in range(3):
        v = e.records[s].v[1][Rt[s]]                                          # the value in front of round(), per pixel
        assert np.array_equal(e.right[s], np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8))
        low += int((v < -0.5).sum())
        high += int((v > 255.5).sum())
        assert e.right[s][v < -0.5].max(initial=0) == 0 and e.right[s][v > 255.5].min(initial=255) == 255
    assert low > 50 and high > 50


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_fixture_tables_keep_their_distance_from_rounding_boundaries(name):
    assert K.min_boundary_distance(name) >= 1e-9, "replace the fixture"


def test_host_pair_fixtures_keep_their_distance_too():
    for l, r, w in K.host_pairs():
        info = R.set_intensities(r, *R.mean_std_dev(*R.sums(l), l.size), w)[1]
        assert R.boundary_distance(info[4]) >= 1e-9, "replace the fixture"
