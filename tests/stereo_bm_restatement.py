"""Numpy restatement of the reference's dense stereo depth (src/tracker/stereo_disparity.cpp, tracker.cpp:784-796, image.cpp:108-139):
cv::StereoBM::create(nd) with speckle window 500 and range 10, getDepth and computePointCloud. This file is the spec the kernels of
hybvio_amd/csrc/stereo_bm.hip follow, bit for bit.

NOT PINNED against an OpenCV build: none is installed where this was written. The rules are written from the algorithm of OpenCV 4.x
modules/calib3d/src/stereobm.cpp (prefilterXSobel, findStereoCorrespondenceBM_, filterSpeckles) as the maintainers and the author
remember it; tests/golden/make_stereo_bm_golden_opencv.py writes the fixture that would pin them. The doubts, each decided as
written below:
  1. prefilter edge rows: row -1 reads row 1 and row H reads row H - 2 (no repeated edge row); an odd height leaves the last row
     at the cap (the two-rows-at-a-time loop). The author's memory of prefilterXSobel agrees with both.
  2. tie order: the scalar loop keeps the FIRST strictly smallest sad in OpenCV's index k = nd - 1 - d, so a tie goes to the
     larger disparity. A SIMD path of a given build might scan in another order; the scalar rule is the one stated here.
  3. the speckle range: StereoBM hands speckleRange to filterSpeckles unscaled, so maxDiff = 10 compares values that carry four
     fraction bits (10 / 16 of a pixel). Some OpenCV versions are remembered to scale by 16 (DISPARITY_SHIFT); unscaled is stated.
  4. the valid rectangle's left edge nd - 1 + w2 and the texture sum |L' - c| over the left window only.
  5. getDepth / computePointCloud: Eigen's 4 x 4 by 4 product is taken as summed left to right, and squaredNorm as (x^2 + y^2) + z^2.
"""
import collections

import numpy as np

FILTERED = -16
MIN_DISPARITY_FILTER = np.float32(1.0)
MIN_DEPTH = np.float32(1.0)


def num_disparities(width):
    """std::ceil(width * REL_MAX_DISPARITY / 32) * 32 in binary32 (stereo_disparity.cpp:39)."""
    v = np.float32(np.float32(width) * np.float32(0.1))
    v = np.float32(v / np.float32(32))
    return int(np.ceil(v)) * 32


def default_params(width):
    """cv::StereoBM::create(nd) as OpenCvStereoDisparity::computeDisparity sets it up (stereo_disparity.cpp:52-57)."""
    return dict(numDisparities=num_disparities(width), blockSize=21, preFilterCap=31, textureThreshold=10, uniquenessRatio=15,
                speckleWindowSize=500, speckleRange=10)


def prefilter(img, cap=31):
    """Rule 1: XSOBEL, clamp(S, -c, c) + c; mirrored rows, edge columns c, the last row of an odd height c."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    out = np.full((h, w), cap, np.uint8)
    if w < 3 or h < 2:
        return out
    a = img.astype(np.int32)
    rows = np.arange(h)
    up, dn = np.where(rows - 1 < 0, 1, rows - 1), np.where(rows + 1 >= h, h - 2, rows + 1)
    dx = a[:, 2:] - a[:, :-2]
    s = dx[up] + 2 * dx + dx[dn]
    out[:, 1:-1] = (np.clip(s, -cap, cap) + cap).astype(np.uint8)
    if h % 2 == 1:
        out[h - 1, :] = cap
    return out


def valid_rect(w, h, nd, block=21):
    """Rule 2: (x0, x1, y0, y1), half open; x1 <= x0 or y1 <= y0: empty."""
    w2 = block // 2
    return nd - 1 + w2, w - w2, w2, h - w2


def _box(a, w2):
    """Sums over (2 w2 + 1)^2 windows centred on every pixel that has a whole window: [H - 2 w2, W - 2 w2]."""
    n = 2 * w2 + 1
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
    c[1:, 1:] = a.cumsum(0).cumsum(1)
    return c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]


def sad_volume(lp, rp, nd, block=21):
    """Rule 3, first line: sad [nd, Hv, Wv] over the valid rectangle; None when it is empty."""
    h, w = lp.shape
    w2 = block // 2
    x0, x1, y0, y1 = valid_rect(w, h, nd, block)
    if x1 <= x0 or y1 <= y0:
        return None
    L, R = lp.astype(np.int32), rp.astype(np.int32)
    sad = np.zeros((nd, y1 - y0, x1 - x0), np.int32)
    for d in range(nd):
        ad = np.zeros((h, w), np.int32)
        ad[:, d:] = np.abs(L[:, d:] - R[:, :w - d])
        sad[d] = _box(ad, w2)[:, x0 - w2:x1 - w2]
    return sad


def decide(sad, textsum, nd, texture_threshold=10, uniqueness_ratio=15, stats=None):
    """Rule 3 from the texture test on: sad [nd, ...] (index d) and textsum [...] -> int16 values (disparity x 16 or FILTERED)."""
    sad = np.asarray(sad, np.int64)
    sk = sad[::-1]                                            # OpenCV's index k = nd - 1 - d
    mink = np.argmin(sk, 0)                                   # the first k with the strictly smallest value
    m = np.take_along_axis(sk, mink[None], 0)[0]
    thresh = m + m * uniqueness_ratio // 100
    k = np.arange(nd).reshape((nd,) + (1,) * (sad.ndim - 1))
    rival = ((np.abs(k - mink[None]) > 1) & (sk <= thresh[None])).any(0)
    kp = np.where(mink + 1 >= nd, nd - 2, mink + 1)           # sad[nd] = sad[nd - 2]
    kn = np.where(mink - 1 < 0, 1, mink - 1)                  # sad[-1] = sad[1]
    p = np.take_along_axis(sk, kp[None], 0)[0]
    n = np.take_along_axis(sk, kn[None], 0)[0]
    dd = p + n - 2 * m + np.abs(p - n)
    num = (p - n) * 256
    q = np.where(dd != 0, np.sign(num) * (np.abs(num) // np.where(dd != 0, dd, 1)), 0)      # C's division: toward zero
    value = ((nd - mink - 1) * 256 + q + 15) >> 4             # arithmetic shift
    flat = np.asarray(textsum) < texture_threshold
    out = np.where(flat | rival, FILTERED, value).astype(np.int16)
    if stats is not None:
        keep = ~(flat | rival)
        stats["texture"] = int(flat.sum())
        stats["uniqueness"] = int((rival & ~flat).sum())
        stats["tie"] = int((((sk == m[None]).sum(0) > 1) & keep).sum())
        stats["negative_quotient"] = int(((q < 0) & keep).sum())
    return out


def block_match(left, right, params, stats=None):
    """Rules 1 - 3: the int16 disparity x 16 image before the speckle filter."""
    nd, block, cap = params["numDisparities"], params["blockSize"], params["preFilterCap"]
    lp, rp = prefilter(left, cap), prefilter(right, cap)
    h, w = lp.shape
    out = np.full((h, w), FILTERED, np.int16)
    sad = sad_volume(lp, rp, nd, block)
    if sad is None:
        return out
    x0, x1, y0, y1 = valid_rect(w, h, nd, block)
    w2 = block // 2
    text = _box(np.abs(lp.astype(np.int32) - cap), w2)[y0 - w2:y1 - w2, x0 - w2:x1 - w2]
    out[y0:y1, x0:x1] = decide(sad, text, nd, params["textureThreshold"], params["uniquenessRatio"], stats)
    return out


def components(disp, new_val, max_diff):
    """Rule 4's graph: (labels [H, W] int32, -1 on new_val pixels; sizes per label)."""
    d = np.asarray(disp, np.int32)
    h, w = d.shape
    ok = d != new_val
    right = np.zeros((h, w), bool); down = np.zeros((h, w), bool)
    right[:, :-1] = ok[:, :-1] & ok[:, 1:] & (np.abs(d[:, :-1] - d[:, 1:]) <= max_diff)
    down[:-1] = ok[:-1] & ok[1:] & (np.abs(d[:-1] - d[1:]) <= max_diff)
    labels = np.full((h, w), -1, np.int32)
    sizes = []
    okl, rl, dl = ok.tolist(), right.tolist(), down.tolist()
    lab = [[-1] * w for _ in range(h)]
    for sy in range(h):
        for sx in range(w):
            if not okl[sy][sx] or lab[sy][sx] >= 0:
                continue
            cur = len(sizes)
            lab[sy][sx] = cur
            q = collections.deque([(sy, sx)])
            cnt = 0
            while q:
                y, x = q.popleft()
                cnt += 1
                if rl[y][x] and lab[y][x + 1] < 0:
                    lab[y][x + 1] = cur; q.append((y, x + 1))
                if x > 0 and rl[y][x - 1] and lab[y][x - 1] < 0:
                    lab[y][x - 1] = cur; q.append((y, x - 1))
                if dl[y][x] and lab[y + 1][x] < 0:
                    lab[y + 1][x] = cur; q.append((y + 1, x))
                if y > 0 and dl[y - 1][x] and lab[y - 1][x] < 0:
                    lab[y - 1][x] = cur; q.append((y - 1, x))
            sizes.append(cnt)
    labels[:] = np.asarray(lab, np.int32)
    return labels, np.asarray(sizes, np.int64)


def filter_speckles(disp, new_val=FILTERED, max_size=500, max_diff=10, stats=None):
    """Rule 4: cv::filterSpeckles(disp, new_val, max_size, max_diff) on int16; returns a new array."""
    out = np.array(disp, np.int16, copy=True)
    labels, sizes = components(out, new_val, max_diff)
    if len(sizes):
        small = sizes <= max_size
        out[(labels >= 0) & small[np.maximum(labels, 0)]] = new_val
        if stats is not None:
            stats["small_components"] = int(small.sum())
            stats["large_components"] = int((~small).sum())
            stats["speckle_pixels"] = int(sizes[small].sum())
    elif stats is not None:
        stats.update(small_components=0, large_components=0, speckle_pixels=0)
    return out


def compute_disparity(left, right, params, stats=None):
    """OpenCvStereoDisparity::computeDisparity: rules 1 - 4."""
    d = block_match(left, right, params, stats)
    if params["speckleWindowSize"] > 0 and params["speckleRange"] >= 0:
        d = filter_speckles(d, FILTERED, params["speckleWindowSize"], params["speckleRange"], stats)
    return d


def _project(qf, x, y, val):
    """Qf . (x, y, val, 1) in binary32, summed left to right, then hnormalized: (pos [3], finite?)."""
    f = np.float32
    with np.errstate(all="ignore"):
        v = [f(f(f(f(qf[r, 0] * f(x)) + f(qf[r, 1] * f(y))) + f(qf[r, 2] * val)) + f(qf[r, 3] * f(1))) for r in range(4)]
        return np.array([f(v[0] / v[3]), f(v[1] / v[3]), f(v[2] / v[3])], np.float32)


def _val_of(v):
    val = np.float32(np.float32(v) / np.float32(16))
    return None if (val <= 0 or val < MIN_DISPARITY_FILTER) else val


def get_depth(q, disp, px, py):
    """Rule 5 (stereo_disparity.cpp:66-77), one point -> float32."""
    h, w = disp.shape
    px, py = np.float32(px), np.float32(py)
    if not (np.isfinite(px) and np.isfinite(py)) or abs(px) >= 2.0 ** 31 or abs(py) >= 2.0 ** 31:
        return np.float32(-1)                                 # the library's choice: the reference's cast is undefined there
    x, y = int(px), int(py)                                   # toward zero
    if x < 0 or y < 0 or x >= w or y >= h:
        return np.float32(-1)
    val = _val_of(disp[y, x])
    if val is None:
        return np.float32(-1)
    pos = _project(np.asarray(q, np.float64).reshape(4, 4).astype(np.float32), x, y, val)
    f = np.float32
    with np.errstate(all="ignore"):
        return np.sqrt(f(f(f(pos[0] * pos[0]) + f(pos[1] * pos[1])) + f(pos[2] * pos[2])))


def track_depths(q, disp, xy):
    return np.array([get_depth(q, disp, x, y) for x, y in np.asarray(xy, np.float32).reshape(-1, 2)], np.float32)


def point_cloud(q, disp, stride=5):
    """Rule 6 (stereo_disparity.cpp:79-94): [n, 3] float32 in row-major visiting order."""
    h, w = disp.shape
    qf = np.asarray(q, np.float64).reshape(4, 4).astype(np.float32)
    f = np.float32
    out = []
    for y in range(0, h, stride):
        for x in range(0, w, stride):
            val = _val_of(disp[y, x])
            if val is None:
                continue
            pos = _project(qf, x, y, val)
            with np.errstate(all="ignore"):
                n2 = f(f(f(pos[0] * pos[0]) + f(pos[1] * pos[1])) + f(pos[2] * pos[2]))
            if n2 < f(MIN_DEPTH * MIN_DEPTH):
                continue
            out.append(pos)
    return np.array(out, np.float32).reshape(-1, 3)


def cloud_bound(w, h, stride):
    return -(-w // stride) * -(-h // stride)
