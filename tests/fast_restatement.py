"""numpy restatement of the reference's FAST detector path: CustomFastFeatureDetector (src/tracker/feature_detector_legacy.cpp:141-174,
cv::FastFeatureDetector, FAST-9 on the 16-pixel circle, non-max suppression on), MaskedFeatureDetector::detect / setMask / drawMask
(:20-51, :70-83) and the tail of FeatureDetector::detect with applyMinDistance (:177-213).

Test infrastructure only (not collected, imported by the tests; nothing under hybvio_amd/ uses it). No OpenCV exists here, so this is
written from the algorithm as the project's header states it (include/hybvio_hip.h, the FAST section), step by step, and has NOT been
pinned against an OpenCV build: tests/golden/make_fast_golden_opencv.py writes the fixture that would do so.

  1. segment test   pixel v at 3 <= x <= w - 4, 3 <= y <= h - 4 is a corner when 9 consecutive circle pixels (indices modulo 16) are
                    all > v + t or all < v - t (strict); no corners when w < 7 or h < 7
  2. score          max over the 16 arcs and both signs of the min over the arc of +-(v - circle_k), minus 1: the largest threshold
                    at which the pixel still passes (t .. 254 for a corner); a non-corner scores 0
  3. suppression    kept when strictly greater than the scores of all 8 neighbours; key points in row-major order
  4. mask           every previous corner with 0 < px < w and 0 < py < h (binary32) masks columns [max(ix - r, 0), min(ix + r, w - 1))
                    and the like rows, ix = (int)px
  5. tail           stable sort by descending score, then the greedy min-distance filter against the corners kept so far with the
                    binary32 test dx*dx + dy*dy < (float)(r*r), stopped at maxTracks
Vectorised over the image; the greedy walk is a plain loop over the candidates.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32

# (dx, dy) of circle pixel k = 0 .. 15
CIRCLE = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
          (-2, 2), (-1, 3))


def corner_scores(img: np.ndarray, t: int) -> np.ndarray:
    """Steps 1 and 2: int32 [h, w], the score of every corner and 0 elsewhere (a corner of score 0, possible at t = 0, reads as 0:
    it can never be strictly above a neighbour)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    h, w = img.shape
    out = np.zeros((h, w), np.int32)
    if w < 7 or h < 7:
        return out
    v = img[3:h - 3, 3:w - 3].astype(np.int32)
    d = np.stack([v - img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx].astype(np.int32) for dx, dy in CIRCLE])     # d_k = v - circle_k
    d = np.concatenate([d, d[:8]])
    darker, brighter = d > t, -d > t                        # circle_k < v - t, circle_k > v + t
    corner = np.zeros(v.shape, bool)
    best = np.full(v.shape, -256, np.int32)
    for s in range(16):
        arc = d[s:s + 9]
        corner |= darker[s:s + 9].all(0) | brighter[s:s + 9].all(0)
        best = np.maximum(best, np.maximum(arc.min(0), (-arc).min(0)))
    score = best - 1
    assert (score[corner] >= t).all() and (score[corner] <= 254).all() and (score[~corner] < t).all()
    out[3:h - 3, 3:w - 3] = np.where(corner, score, 0)
    return out


def keypoints(img: np.ndarray, t: int = 10) -> np.ndarray:
    """Steps 1 - 3: float32 [n, 3] = (x, y, score) in row-major order."""
    sc = corner_scores(img, t)
    h, w = sc.shape
    p = np.zeros((h + 2, w + 2), np.int32)
    p[1:-1, 1:-1] = sc
    keep = sc > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= sc > p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    ys, xs = np.nonzero(keep)                               # row-major
    return np.stack([xs.astype(f32), ys.astype(f32), sc[ys, xs].astype(f32)], axis=1).reshape(-1, 3)


def draw_mask(prev, r: int, w: int, h: int) -> np.ndarray:
    """Step 4, drawMask: bool [h, w], True where a key point is removed."""
    assert r >= 1                                           # the reference asserts maskRadius >= 1
    m = np.zeros((h, w), bool)
    for px, py in np.asarray(prev, f32).reshape(-1, 2):
        if not (f32(0) < px < f32(w) and f32(0) < py < f32(h)):          # NaN compares false
            continue
        ix, iy = int(px), int(py)
        x0, x1 = max(ix - r, 0), min(ix + r, w - 1)
        y0, y1 = max(iy - r, 0), min(iy + r, h - 1)
        if x1 > x0 and y1 > y0:
            m[y0:y1, x0:x1] = True                          # the upper ends are exclusive
    return m


def masked_sorted(kp: np.ndarray, prev, r: int, w: int, h: int) -> np.ndarray:
    """Step 4 and the sort of step 5: the key points outside every box, stable-sorted by descending score."""
    m = draw_mask(prev, r, w, h)
    kp = kp[~m[kp[:, 1].astype(int), kp[:, 0].astype(int)]]
    return kp[np.argsort(-kp[:, 2], kind="stable")]


def min_distance(xy: np.ndarray, r: int, max_tracks: int) -> np.ndarray:
    """applyMinDistance(corners, {}, r): greedy, in order, against the corners kept so far; stops at max_tracks."""
    r2 = f32(r * r)
    acc = np.zeros((max_tracks, 2), f32)
    n = 0
    for c in np.asarray(xy, f32).reshape(-1, 2):
        dx, dy = acc[:n, 0] - c[0], acc[:n, 1] - c[1]
        if not (dx * dx + dy * dy < r2).any():
            acc[n] = c
            n += 1
        if n >= max_tracks:
            break
    return acc[:n].copy()


def detect(img: np.ndarray, prev=(), r: int = 30, t: int = 10, max_tracks: int = 200, kp: np.ndarray | None = None):
    """FeatureDetector::detect of the FAST detector -> (corners float32 [n, 2], the masked and sorted key points float32 [m, 3]).
    kp: the result of keypoints(img, t) when the caller already has it."""
    h, w = img.shape
    srt = masked_sorted(keypoints(img, t) if kp is None else kp, prev, r, w, h)
    return min_distance(srt[:, :2], r, max_tracks), srt
