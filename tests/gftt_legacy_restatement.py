"""numpy restatement of the reference's legacy GFTT detector path: GFTTFeatureDetector (src/tracker/feature_detector_legacy.cpp:53-139,
cv::GFTTDetector = cv::goodFeaturesToTrack) behind MaskedFeatureDetector::detect / setMask / drawMask (:20-51), on top of the oracle's
cv::cornerMinEigenVal (oracle.corner_min_eigen_val).

Test infrastructure only (not collected, imported by the tests; nothing under hybvio_amd/ uses it). No OpenCV exists here, so this is
written from the algorithm of OpenCV 4.x's goodFeaturesToTrack as the project's header states it (include/hybvio_hip.h, the legacy
GFTT section), step by step, and has NOT been pinned against an OpenCV build. The one rule an older OpenCV does not share is the
order among equal responses (step 6: 4.x's greaterThanPtr compares the pointers, so the larger raster index comes first).

  1. mask        all ones; every live track (px, py) with 0 < px < w and 0 < py < h (binary32) zeroes columns [max(ix - r, 0),
                 min(ix + r, w - 1)) and the like rows, ix = (int)px (fast_restatement.draw_mask: the same drawMask)
  2. response    eig = cornerMinEigenVal(gray, blockSize, 3), binary32
  3. maximum     maxVal = the maximum of eig over the unmasked pixels, border rows and columns included; 0 when there is none
  4. threshold   t = (float)((double)maxVal * qualityLevel); eig[p] = eig[p] > t ? eig[p] : 0 at every pixel, masked or not
  5. candidates  1 <= x <= w - 2, 1 <= y <= h - 2, value v != 0, v == the maximum of the thresholded 3 x 3 neighbourhood, unmasked
  6. order       descending v, among equal v the larger raster index y * w + x first
  7. walk        minDistance >= 1: OpenCV's grid of cells of cvRound(minDistance) pixels; a candidate is accepted unless a corner
                 in the 3 x 3 cells around its own lies at dx*dx + dy*dy < minDistance * minDistance (binary64 right-hand side);
                 minDistance < 1: every candidate is accepted; both stop at maxCorners
  8. output      (float)x, (float)y in acceptance order
"""
from __future__ import annotations

import numpy as np

from fast_restatement import draw_mask

f32 = np.float32


def scaled_min_distance(w: int, h: int, gftt_min_distance: float = 50.0) -> float:
    """GFTTFeatureDetector's minDistance: gfttMinDistance * (min(w, h) / 720.0), binary64."""
    return float(gftt_min_distance) * (min(w, h) / 720.0)


def mask(prev, r: int, w: int, h: int) -> np.ndarray:
    """Step 1: bool [h, w], True where the pixel is unmasked."""
    return ~draw_mask(prev, r, w, h)


def response(img: np.ndarray, block_size: int = 3) -> np.ndarray:
    from oracle import orc
    return orc.corner_min_eigen_val(np.ascontiguousarray(img, np.uint8), block_size)


def threshold(eig: np.ndarray, m: np.ndarray, quality: float):
    """Steps 3 and 4 -> (t, the thresholded response)."""
    max_val = eig[m].max() if m.any() else f32(0)
    t = f32(np.float64(max_val) * np.float64(quality))
    return t, np.where(eig > t, eig, f32(0)).astype(f32)


def candidates_of(eig: np.ndarray, m: np.ndarray, quality: float = 0.01) -> np.ndarray:
    """Steps 3 - 6 on a response map: float32 [n, 3] = (x, y, v) in sorted order."""
    eig = np.asarray(eig, f32)
    h, w = eig.shape
    _, tv = threshold(eig, m, quality)
    p = np.full((h + 2, w + 2), -np.inf, f32)
    p[1:-1, 1:-1] = tv
    dil = tv.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            dil = np.maximum(dil, p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w])
    keep = (tv != 0) & (tv == dil) & m
    keep[0, :] = keep[-1, :] = False
    keep[:, 0] = keep[:, -1] = False
    ys, xs = np.nonzero(keep)
    v = tv[ys, xs]
    order = np.lexsort((-(ys * w + xs), -v.astype(np.float64)))       # descending v, then descending raster index
    return np.stack([xs[order].astype(f32), ys[order].astype(f32), v[order]], axis=1).reshape(-1, 3)


def candidates(img: np.ndarray, prev=(), r: int = 1, block_size: int = 3, quality: float = 0.01, eig: np.ndarray | None = None):
    """Steps 1 - 6: float32 [n, 3] = (x, y, v) in sorted order. eig: response(img, block_size) when the caller already has it."""
    h, w = img.shape
    return candidates_of(response(img, block_size) if eig is None else eig, mask(prev, r, w, h), quality)


def walk_grid(cand: np.ndarray, w: int, h: int, min_distance: float, max_corners: int) -> np.ndarray:
    """Step 7 as OpenCV writes it -> the indices of the accepted candidates."""
    out = []
    if min_distance >= 1:
        cell = int(round(min_distance))                      # cvRound: half to even
        gw, gh = (w + cell - 1) // cell, (h + cell - 1) // cell
        grid = [[] for _ in range(gw * gh)]
        md2 = float(min_distance) * float(min_distance)
        for i, (x, y) in enumerate(cand[:, :2].astype(int).tolist()):
            xc, yc = x // cell, y // cell
            x1, y1, x2, y2 = max(0, xc - 1), max(0, yc - 1), min(gw - 1, xc + 1), min(gh - 1, yc + 1)
            good = True
            for yy in range(y1, y2 + 1):
                for xx in range(x1, x2 + 1):
                    for qx, qy in grid[yy * gw + xx]:
                        dx, dy = x - qx, y - qy
                        if dx * dx + dy * dy < md2:
                            good = False
                            break
                    if not good:
                        break
                if not good:
                    break
            if good:
                grid[yc * gw + xc].append((x, y))
                out.append(i)
                if max_corners > 0 and len(out) == max_corners:
                    break
    else:
        out = list(range(min(len(cand), max_corners) if max_corners > 0 else len(cand)))
    return np.asarray(out, np.int64)


def walk_brute(cand: np.ndarray, min_distance: float, max_corners: int) -> np.ndarray:
    """Step 7 against every accepted corner (what the grid is a shortcut for)."""
    if min_distance < 1:
        return np.arange(min(len(cand), max_corners))
    md2 = float(min_distance) * float(min_distance)
    xy = cand[:, :2].astype(np.int64)
    acc = np.zeros((max_corners, 2), np.int64)
    out = []
    for i, c in enumerate(xy):
        d = acc[:len(out)] - c
        if not ((d * d).sum(1) < md2).any():
            acc[len(out)] = c
            out.append(i)
            if len(out) == max_corners:
                break
    return np.asarray(out, np.int64)


def detect(img: np.ndarray, prev=(), r: int = 1, block_size: int = 3, quality: float = 0.01, gftt_min_distance: float = 50.0,
           max_tracks: int = 200, cand: np.ndarray | None = None):
    """MaskedFeatureDetector::detect of the GFTT detector -> (corners float32 [n, 2], their responses float32 [n], the sorted
    candidates float32 [m, 3]). cand: candidates(img, prev, r, block_size, quality) when the caller already has it."""
    h, w = img.shape
    if cand is None:
        cand = candidates(img, prev, r, block_size, quality)
    idx = walk_grid(cand, w, h, scaled_min_distance(w, h, gftt_min_distance), max_tracks)
    return cand[idx, :2].copy().reshape(-1, 2), cand[idx, 2].copy(), cand
