"""numpy restatement of SubPixelAdjuster::adjust (src/tracker/subpixel_adjuster.cpp:18-42): cv::cornerSubPix followed by the
revert of refined points that left the image.

Test infrastructure only (not collected, imported by the tests; nothing under hybvio_amd/ uses it). No OpenCV exists here, so
this follows OpenCV 4.x from the upstream source, step by step:
  imgproc/src/cornersubpix.cpp   cv::cornerSubPix: criteria, mask, the iteration loop, the final distance check
  imgproc/src/samplers.cpp       getRectSubPix(u8 -> CV_32F): getRectSubPix_8u32f (patch and its +1 row / column inside the
                                 image) and getRectSubPix_Cn_<uchar, float, float> with adjustRect (replicated borders)
binary32 wherever OpenCV computes in float, binary64 wherever it uses double, in the same operation order; vectorised across
corners, serial over the W^2 terms of each sum (np.cumsum is a sequential accumulation, checked in test_subpix_restatement.py).
Where OpenCV's IPP build routes getRectSubPix to ippiCopySubpixIntersect, results may differ in the last bits: the non-IPP code
is the one restated.
"""
from __future__ import annotations

import ctypes
import ctypes.util

import numpy as np

f32, f64 = np.float32, np.float64
DBL_EPSILON = float(np.finfo(np.float64).eps)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]


def gauss_table(win: int) -> np.ndarray:
    """exp(-t^2), t = (float)(i - win) / win, with the platform expf (cornersubpix.cpp: float y = (float)(i - win.height) /
    win.height; float vy = std::exp(-y*y)). mask[i][j] = (float)(vy * std::exp(-x*x)) = g[i] * g[j] in binary32."""
    g = np.empty(2 * win + 1, f32)
    for i in range(2 * win + 1):
        y = f32(f32(i - win) / f32(win))
        g[i] = _libm.expf(float(-y * y))
    return g


def _px(img, r, c):
    h, w = img.shape
    return img[np.clip(r, 0, h - 1), np.clip(c, 0, w - 1)].astype(f32)


def rect_subpix(img: np.ndarray, cx: np.ndarray, cy: np.ndarray, pw: int, force: str | None = None):
    """getRectSubPix(img, Size(pw, pw), (cx, cy), patch, CV_32F) for n centres -> (patches [n, pw, pw] f32, fast [n] bool).
    force "generic" / "fast" (tests only): that sampler's formula for every centre (the fast one only where it is in range)."""
    h, w = img.shape
    cx = np.asarray(cx, f32)
    cy = np.asarray(cy, f32)
    half = f32((pw - 1) * 0.5)                                   # center.x -= (win_size.width-1)*0.5f
    hx, hy = cx - half, cy - half
    ipx = np.floor(hx).astype(np.int64)                          # cvFloor
    ipy = np.floor(hy).astype(np.int64)
    fa = hx - ipx.astype(f32)
    fb = hy - ipy.astype(f32)
    one = f32(1)
    I = np.arange(pw)[None, :, None]
    J = np.arange(pw)[None, None, :]
    col = lambda v: v[:, None, None]
    # getRectSubPix_8u32f (cn == 1 && 0 <= ip.x && ip.x + win.width < cols && same in y)
    fast = (ipx >= 0) & (ipx + pw < w) & (ipy >= 0) & (ipy + pw < h)
    if force is not None:
        assert force == "generic" or fast.all()
        fast = np.full_like(fast, force == "fast")
    a = np.maximum(fa, f32(0.0001))                              # a = MAX(a, 0.0001f)
    a12, a22, b1, b2 = a * (one - fb), a * fb, one - fb, fb
    s = (1.0 - a.astype(f64)) / a.astype(f64)                    # double s = (1. - a)/a
    R, C = col(ipy) + I, col(ipx) + J
    tj = col(a12) * _px(img, R, C + 1) + col(a22) * _px(img, R + 1, C + 1)     # t = a12*src[j+1] + a22*src[j+1+step]
    tp = col(a12) * _px(img, R, C) + col(a22) * _px(img, R + 1, C)             # the previous column's t
    prev = (tp.astype(f64) * col(s)).astype(f32)                                # prev = (float)(t*s)
    prev[:, :, 0] = ((one - a)[:, None] * (b1[:, None] * _px(img, R[:, :, 0], C[:, :, 0])
                                           + b2[:, None] * _px(img, R[:, :, 0] + 1, C[:, :, 0])))   # (1 - a)*(b1*src[0] + b2*src[step])
    patch_fast = prev + tj
    # getRectSubPix_Cn_ (its own inside test is the same as the one above, so only the adjustRect branch is reached)
    a11, a12g, a21, a22g = (one - fa) * (one - fb), fa * (one - fb), (one - fa) * fb, fa * fb
    rx = np.where(ipx >= 0, 0, np.minimum(-ipx, pw))
    col0 = np.where(ipx >= 0, ipx, 0)
    rw = np.where(ipx < w - pw, pw, w - ipx - 1)
    col0 = np.where(rw < 0, col0 + rw, col0)
    rw = np.maximum(rw, 0)
    col0 = col0 - rx                                             # return src - rect.x*pix_size
    ry = np.where(ipy >= 0, 0, -ipy)
    row0 = np.where(ipy >= 0, ipy, 0)
    rh = np.where(ipy < h - pw, pw, h - ipy - 1)
    row0 = np.where(rh < 0, row0 + rh, row0)
    rh = np.maximum(rh, 0)
    # rows: src advances after row i when i < r.height; src2 = src + step unless i < r.y or i >= r.height
    rt = col(row0) + np.maximum(0, np.minimum(I, col(rh)) - col(ry))
    rb = rt + ((I >= col(ry)) & (I < col(rh)))
    right, left = J >= col(rw), J < col(rx)                     # the right-border loop runs after the left one
    cb = col(col0) + np.where(right, col(rw), col(rx))
    border = _px(img, rt, cb) * col(b1) + _px(img, rb, cb) * col(b2)           # src[r.x]*b1 + src2[r.x]*b2
    c = col(col0) + J
    inner = ((_px(img, rt, c) * col(a11) + _px(img, rt, c + 1) * col(a12g)) + _px(img, rb, c) * col(a21)) \
        + _px(img, rb, c + 1) * col(a22g)
    patch_gen = np.where(right | left, border, inner)
    return np.where(col(fast), patch_fast, patch_gen).astype(f32), fast


def _serial_sum(terms: np.ndarray) -> np.ndarray:
    """acc = 0; for k: acc += terms[:, k] (sequential, starting from +0 like the reference)."""
    z = np.zeros((terms.shape[0], 1), f64)
    return np.cumsum(np.concatenate([z, terms], axis=1), axis=1)[:, -1]


def corner_subpix(img: np.ndarray, xy, win: int = 10, max_iter: int = 20, epsilon: float = 0.03, trace=None, adjust: bool = True):
    """SubPixelAdjuster::adjust -> (xy [n, 2] f32, position updates [n] i32). Inputs outside [0, w) x [0, h) (where OpenCV
    asserts) are returned unchanged with 0 updates, as the library does. trace: optional list, receives (idx, fast) per
    iteration (which corners were sampled and whether on the 8u32f path). adjust=False: cv::cornerSubPix alone (no revert of
    refined points outside the image)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    xy = np.ascontiguousarray(xy, f32).reshape(-1, 2)
    n = len(xy)
    assert win >= 1 and w >= 2 * win + 5 and h >= 2 * win + 5
    max_iters = min(max(int(max_iter), 1), 100)
    eps = max(float(epsilon), 0.0)
    eps *= eps
    ww, pw = 2 * win + 1, 2 * win + 3
    g = gauss_table(win)
    mask = (g[:, None] * g[None, :]).astype(f64).reshape(-1)
    px = np.tile((np.arange(ww) - win).astype(f64), ww)
    py = np.repeat((np.arange(ww) - win).astype(f64), ww)
    tx, ty = xy[:, 0].copy(), xy[:, 1].copy()
    cx, cy = tx.copy(), ty.copy()
    updates = np.zeros(n, np.int32)
    iters = np.zeros(n, np.int64)
    active = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
    inside0 = active.copy()
    while active.any():
        idx = np.nonzero(active)[0]
        P, fast = rect_subpix(img, cx[idx], cy[idx], pw)
        if trace is not None:
            trace.append((idx, fast))
        tgx = (P[:, 1:-1, 2:] - P[:, 1:-1, :-2]).reshape(len(idx), -1).astype(f64)     # subpix[j+1] - subpix[j-1] in float
        tgy = (P[:, 2:, 1:-1] - P[:, :-2, 1:-1]).reshape(len(idx), -1).astype(f64)     # subpix[j+win_w+2] - subpix[j-win_w-2]
        gxx, gxy, gyy = tgx * tgx * mask, tgx * tgy * mask, tgy * tgy * mask
        a, b, c = _serial_sum(gxx), _serial_sum(gxy), _serial_sum(gyy)
        bb1 = _serial_sum(gxx * px + gxy * py)
        bb2 = _serial_sum(gxy * px + gyy * py)
        det = a * c - b * b
        ok = ~(np.abs(det) <= DBL_EPSILON * DBL_EPSILON)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            scale = 1.0 / det
            x0, y0 = cx[idx].astype(f64), cy[idx].astype(f64)
            x2 = (x0 + c * scale * bb1 - b * scale * bb2).astype(f32)
            y2 = (y0 - b * scale * bb1 + a * scale * bb2).astype(f32)
            dx, dy = x2 - cx[idx], y2 - cy[idx]
            err = dx * dx + dy * dy                                                     # float
        u = idx[ok]
        cx[u], cy[u] = x2[ok], y2[ok]
        updates[u] += 1
        out = (cx[idx] < 0) | (cx[idx] >= w) | (cy[idx] < 0) | (cy[idx] >= h)
        iters[idx] += 1
        cont = ok & ~out & (iters[idx] < max_iters) & (err.astype(f64) > eps)          # while (++iter < max_iters && err > eps)
        active[idx] = cont
    far = (np.abs(cx - tx) > f32(win)) | (np.abs(cy - ty) > f32(win))
    cx[far], cy[far] = tx[far], ty[far]
    outside = ((cx < 0) | (cx >= w) | (cy < 0) | (cy >= h)) & adjust
    cx[outside], cy[outside] = tx[outside], ty[outside]
    cx[~inside0], cy[~inside0] = tx[~inside0], ty[~inside0]
    return np.stack([cx, cy], 1).astype(f32), updates
