"""CPU checks that pin the cornerSubPix restatement (tests/subpix_restatement.py) where no OpenCV can: geometry it must
recover, the termination and revert branches it must take, and the sampler it must pick."""
from math import erf

import numpy as np
import pytest

import subpix_restatement as R


def xjunction(w, h, vx, vy, sigma=1.0, lo=40, hi=200, ss=8):
    """Checkerboard corner with its vertex at (vx, vy) (pixel centres on integers), edges blurred by a Gaussian of `sigma`
    px and every pixel area-sampled on an ss x ss grid."""
    o = (np.arange(ss) + 0.5) / ss - 0.5
    X = (np.arange(w)[:, None] + o[None, :]).reshape(-1)
    Y = (np.arange(h)[:, None] + o[None, :]).reshape(-1)
    cdf = np.vectorize(lambda t: 0.5 * (1.0 + erf(t / (sigma * np.sqrt(2.0)))))
    px, py = cdf(X - vx), cdf(Y - vy)
    f = py[:, None] * px[None, :] + (1 - py[:, None]) * (1 - px[None, :])
    f = f.reshape(h, ss, w, ss).mean(axis=(1, 3))
    return np.round(lo + (hi - lo) * f).astype(np.uint8)


@pytest.mark.parametrize("win", [10, 5])
def test_x_junction_vertex_is_recovered(win):
    rng = np.random.default_rng(100 + win)
    for _ in range(20):
        vx, vy = 32 + rng.uniform(-0.5, 0.5), 30 + rng.uniform(-0.5, 0.5)
        img = xjunction(64, 60, vx, vy)
        out, it = R.corner_subpix(img, np.array([[round(vx), round(vy)]], np.float32), win=win)
        assert np.hypot(out[0, 0] - vx, out[0, 1] - vy) <= 0.05, (vx, vy, out)
        assert it[0] >= 1


def test_flat_patch_breaks_on_det_and_returns_the_input():
    img = np.full((40, 50), 77, np.uint8)
    xy = np.array([[20.25, 17.5], [0, 0], [49.5, 39.75]], np.float32)
    out, it = R.corner_subpix(img, xy)
    assert np.array_equal(out, xy) and it.tolist() == [0, 0, 0]


def test_border_points_take_the_generic_sampler():
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (60, 80), dtype=np.uint8)
    for win in (10, 5, 3):
        w, h = 80, 60
        edge = [[0, 0], [win, 30], [w - win - 2, 30], [40, win], [40, h - win - 2], [w - 1, h - 1]]
        inner = [[win + 2, win + 2], [w - win - 3, h - win - 3], [40, 30]]
        trace = []
        R.corner_subpix(img, np.array(edge + inner, np.float32), win=win, max_iter=1, trace=trace)
        idx, fast = trace[0]
        assert idx.tolist() == list(range(len(edge) + len(inner)))
        assert not fast[:len(edge)].any() and fast[len(edge):].all()


def test_generic_and_fast_samplers_agree_away_from_the_border():
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    cx = rng.uniform(20, 44, 50).astype(np.float32)
    cy = rng.uniform(20, 44, 50).astype(np.float32)
    pf, _ = R.rect_subpix(img, cx, cy, 23, force="fast")
    pg, _ = R.rect_subpix(img, cx, cy, 23, force="generic")
    assert np.abs(pf.astype(np.float64) - pg).max() <= 1e-3


def wedge(w, h, vx, vy, k, lo=40, hi=200, ss=8):
    """Bright wedge |y - vy| < k (x - vx) with its apex at (vx, vy), area-sampled on an ss x ss grid per pixel."""
    o = (np.arange(ss) + 0.5) / ss - 0.5
    X = (np.arange(w)[:, None] + o[None, :]).reshape(-1)
    Y = (np.arange(h)[:, None] + o[None, :]).reshape(-1)
    f = (np.abs(Y[:, None] - vy) < k * (X[None, :] - vx)).astype(np.float64)
    return np.round(lo + (hi - lo) * f.reshape(h, ss, w, ss).mean(axis=(1, 3))).astype(np.uint8)


def test_iterate_leaving_the_image_is_reverted():
    # the two edges of a wedge whose apex lies left of the image: the first step goes towards the apex, out of the image
    img = wedge(64, 60, -4.0, 30.3, 0.6)
    xy = np.array([[0.5, 30.0], [2.0, 30.0], [3.0, 30.0]], np.float32)
    raw, it_raw = R.corner_subpix(img, xy, adjust=False)
    assert (raw[:, 0] < 0).all() and (it_raw == 1).all()
    out, it = R.corner_subpix(img, xy)
    assert np.array_equal(out, xy) and np.array_equal(it, it_raw)


def test_inputs_outside_the_image_come_back_unchanged():
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (40, 40), dtype=np.uint8)
    xy = np.array([[-0.5, 3], [40, 3], [3, 40.0], [np.nan, 2]], np.float32)
    out, it = R.corner_subpix(img, xy)
    assert np.array_equal(out, xy, equal_nan=True) and not it.any()


def test_serial_sum_is_the_left_to_right_chain():
    rng = np.random.default_rng(10)
    t = rng.normal(size=(6, 441)) * np.exp(rng.uniform(-20, 20, (6, 441)))
    ref = np.zeros(6)
    for k in range(441):
        ref = ref + t[:, k]
    assert np.array_equal(R._serial_sum(t), ref)


def test_gauss_table_is_the_binary32_formula():
    g = R.gauss_table(10)
    assert g.dtype == np.float32 and g[10] == 1.0 and g[0] == g[20]
    assert abs(float(g[0]) - np.exp(-1.0)) < 1e-7
