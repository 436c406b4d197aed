"""Scenes for the dense-stereo tests, shared by the CPU and the GPU tests: a rectified pair whose left pixel x matches the right
pixel x - d. Each scene holds
  - a band-limited texture under a disparity plane (left part) and a disparity ramp (right part),
  - a flat patch in both images (the texture rule),
  - a band of 4 x 4 binary blocks shifted by 7 (the prefilter saturates: equal sad values, so ties),
  - a patch of the right image replaced by unrelated noise (wrong matches, and the speckles they leave).
SHAPES are the three the GPU tests run: (width, height, numDisparities)."""
import functools

import numpy as np

import stereo_bm_restatement as R

SHAPES = [(160, 96, 32), (161, 97, 32), (352, 64, 64)]
IDS = [f"{w}x{h}_nd{nd}" for w, h, nd in SHAPES]
BAND = 24                                             # rows of the binary band: windows of rows 22 .. 25 see nothing else
SEEDS = (12, 16, 19)                                  # three distinct scenes per shape


def _smooth(rng, h, w, passes=2, k=5):
    a = rng.uniform(0, 1, (h, w + 2 * k * passes + 8))
    ker = np.ones(k) / k
    for _ in range(passes):
        a = np.apply_along_axis(lambda r: np.convolve(r, ker, "same"), 1, a)
        a = np.apply_along_axis(lambda c: np.convolve(c, ker, "same"), 0, a)
    a = a[:, k * passes + 4:k * passes + 4 + w]
    a = (a - a.min()) / (a.max() - a.min())
    return a


def scene(w, h, nd, seed):
    """(left, right) uint8 [h, w]."""
    rng = np.random.default_rng(seed)
    tw = w + 2 * nd + 8
    tex = _smooth(rng, h, tw) * 200 + 25 + rng.uniform(-6, 6, (h, tw))
    xs = np.arange(w, dtype=np.float64)
    d_plane = 0.35 * nd
    ramp = d_plane + (xs - 0.55 * w) * (0.3 * nd / (0.45 * w))
    disp = np.where(xs < 0.55 * w, d_plane, ramp)                       # per column, every row alike
    left = tex[:, nd:nd + w]
    # right(x) = left(x + d(x)): sample the texture at nd + x + d by linear interpolation
    pos = nd + xs + disp
    i0 = np.floor(pos).astype(int); fr = pos - i0
    right = tex[:, i0] * (1 - fr) + tex[:, i0 + 1] * fr
    left, right = left.copy(), right.copy()
    # the flat patch
    fy, fx = int(0.55 * h), int(0.3 * w) + nd // 2
    left[fy:fy + 28, fx:fx + 30] = 128
    right[fy:fy + 28, fx - int(d_plane) - 4:fx + 30] = 128
    # the band of binary blocks, shifted by 7
    by = 12
    blocks = rng.integers(0, 2, (BAND // 4, (w + 16) // 4 + 4)) * 255
    band = np.kron(blocks, np.ones((4, 4)))[:, :w + 16]
    left[by:by + BAND] = band[:, :w]
    right[by:by + BAND, :w - 7] = band[:, 7:w]
    for r0 in range(4, BAND, 8):                                       # every other block row by 8: sad[7] and sad[8] compete
        right[by + r0:by + r0 + 4, :w - 8] = band[r0:r0 + 4, 8:w]
    # unrelated noise in the right image
    ny, nx = int(0.25 * h), int(0.62 * w)
    right[ny:ny + 30, nx - nd // 2:nx - nd // 2 + 40] = rng.uniform(0, 255, (30, 40))
    return np.clip(np.rint(left), 0, 255).astype(np.uint8), np.clip(np.rint(right), 0, 255).astype(np.uint8)


def params_for(w, nd, **over):
    p = R.default_params(w)
    p["numDisparities"] = nd
    p.update(over)
    return p


@functools.lru_cache(maxsize=None)
def scenes(w, h, nd):
    out = tuple(scene(w, h, nd, s) for s in SEEDS)
    for l, r in out:
        l.setflags(write=False); r.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(w, h, nd, k, speckles):
    """(disparity, stats) of scene k by the restatement; computed once, read-only."""
    l, r = scenes(w, h, nd)[k]
    stats = {}
    d = R.compute_disparity(l, r, params_for(w, nd, speckleWindowSize=500 if speckles else 0), stats)
    d.setflags(write=False)
    return d, stats


def q_matrix(w, h, angle=0.02):
    """disparityToDepthQ of a made-up rig: a small rotation times [[1,0,0,-cx],[0,1,0,-cy],[0,0,0,f],[0,0,-1/Tx,0]]."""
    cx, cy, f, tx = 0.5 * w - 3.25, 0.5 * h + 1.5, 0.8 * w, -0.11
    q = np.array([[1, 0, 0, -cx], [0, 1, 0, -cy], [0, 0, 0, f], [0, 0, -1 / tx, 0]], np.float64)
    c, s = np.cos(angle), np.sin(angle)
    rot = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], np.float64)
    return rot @ q
