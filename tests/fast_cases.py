"""Hand-built images for the FAST detector, shared by test_fast_restatement.py (CPU) and test_gpu_fast.py (the same images embedded
across the kernel's tile seams). Test infrastructure only (not collected)."""
import numpy as np

from fast_restatement import CIRCLE

P = 15          # patch edge; the pixel under test is the centre
C0 = P // 2


def patch(v, circle, bg=None):
    """A P x P patch of value bg (default v) whose centre is v and whose circle pixel k is circle[k] (a dict or 16 values)."""
    img = np.full((P, P), v if bg is None else bg, np.uint8)
    img[C0, C0] = v
    items = circle.items() if isinstance(circle, dict) else enumerate(circle)
    for k, val in items:
        dx, dy = CIRCLE[k % 16]
        img[C0 + dy, C0 + dx] = val
    return img


def arc(v, start, length, val):
    return patch(v, {k: val for k in range(start, start + length)})


def dots(w, h, pts, bg=0, val=255):
    img = np.full((h, w), bg, np.uint8)
    for x, y in pts:
        img[y, x] = val
    return img


def hand_images(t=10):
    """name -> (image, background value, expected corner score of the patch centre before suppression). Threshold t."""
    out = {}
    for sign, name in ((-1, "dark"), (1, "bright")):
        out[f"arc9_{name}"] = (arc(100, 3, 9, 100 + sign * 20), 100, 19)
        out[f"arc8_{name}"] = (arc(100, 3, 8, 100 + sign * 20), 100, 0)
        out[f"wrap_{name}"] = (arc(100, 12, 9, 100 + sign * 30), 100, 29)                     # k = 12 .. 15, 0 .. 4
        out[f"at_t_{name}"] = (arc(100, 0, 16, 100 + sign * t), 100, 0)
        out[f"at_t1_{name}"] = (arc(100, 0, 16, 100 + sign * (t + 1)), 100, t)
    out["zero_in_255"] = (patch(0, [255] * 16, bg=255), 255, 254)
    out["255_in_zero"] = (patch(255, [0] * 16, bg=0), 0, 254)
    out["single_dot"] = (dots(P, P, [(C0, C0)]), 0, 254)
    out["adjacent_equal"] = (dots(P, P, [(C0, C0), (C0 + 1, C0)]), 0, 254)        # both suppressed: no key point
    out["diagonal_equal"] = (dots(P, P, [(C0, C0), (C0 + 1, C0 + 1)]), 0, 254)
    return out


def embed(img, bg, w, h, cx, cy):
    """The patch in a w x h image of value bg, its centre at (cx, cy)."""
    out = np.full((h, w), bg, np.uint8)
    ph, pw = img.shape
    x0, y0 = cx - pw // 2, cy - ph // 2
    assert 0 <= x0 and x0 + pw <= w and 0 <= y0 and y0 + ph <= h
    out[y0:y0 + ph, x0:x0 + pw] = img
    return out


OUT_OF_RANGE_PREV = lambda w, h: np.array([[0.0, 5.0], [5.0, 0.0], [-3.0, 5.0], [5.0, -0.5], [w, 5.0], [5.0, h], [w + 7.5, 5.0],
                                           [np.nan, 5.0], [5.0, np.nan], [np.nan, np.nan], [-np.inf, 4.0], [np.inf, 4.0]], np.float32)


def seeded_images(w, h):
    """The seeded inputs of the GPU comparison and of the OpenCV fixture: the synthetic frame, uniform noise, and noise quantised to
    four gray levels (ties and equal neighbours everywhere)."""
    from hybvio_amd import synth
    rng = np.random.default_rng(w * 7 + h)
    frame = synth.stereo_sequence(11, w, h, 1)[0][0]
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    four = (rng.integers(0, 4, (h, w)) * 60 + 20).astype(np.uint8)
    return frame, noise, four


def golden_prev(w, h, kp, seed):
    """Live tracks near key points (fractional, so (int) matters): up to 150."""
    rng = np.random.default_rng(seed)
    m = min(150, len(kp))
    return (kp[rng.choice(len(kp), m, replace=False), :2] + rng.uniform(-1.5, 1.5, (m, 2))).astype(np.float32)
