"""Hand-built images and live tracks for the legacy GFTT detector, shared by test_gftt_legacy_restatement.py (CPU) and
test_gpu_gftt_legacy.py (the same patches embedded across the kernels' tile seams). Test infrastructure only (not collected).

A single bright pixel on black has its largest response at itself and falling responses around it, so it is exactly one candidate;
two equal bright pixels side by side are mirror images and give two equal adjacent maxima."""
import numpy as np

from fast_cases import embed, seeded_images, OUT_OF_RANGE_PREV     # noqa: F401  (re-exported: one set of seeded inputs)

P = 15          # patch edge; offsets below are relative to the centre (C0, C0)
C0 = P // 2


def dots(w, h, pts):
    """A black w x h image with the pixels (x, y, value)."""
    img = np.zeros((h, w), np.uint8)
    for x, y, v in pts:
        img[y, x] = v
    return img


def hand_patches():
    """name -> (P x P patch on black, the candidates it must give as (dx, dy) from the patch centre, in sorted order)."""
    return {
        "single_dot": (dots(P, P, [(C0, C0, 255)]), [(0, 0)]),
        "weak_dot": (dots(P, P, [(C0, C0, 90)]), [(0, 0)]),
        # two equal adjacent maxima: both are candidates, the later one (larger raster index) first
        "adjacent_equal": (dots(P, P, [(C0, C0, 255), (C0 + 1, C0, 255)]), [(1, 0), (0, 0)]),
        "stacked_equal": (dots(P, P, [(C0, C0, 255), (C0, C0 + 1, 255)]), [(0, 1), (0, 0)]),
    }


def border_images(w, h):
    """name -> (w x h image, the candidates it must give as (x, y)): a candidate in row 1 / column 1 / the last inner row and column,
    and maxima in row 0, column 0 and the last column, which are no candidates but suppress their inner neighbours."""
    return {
        "row1_col1": (dots(w, h, [(1, 1, 255)]), [(1, 1)]),
        "last_inner": (dots(w, h, [(w - 2, h - 2, 255)]), [(w - 2, h - 2)]),
        "col0": (dots(w, h, [(0, 5, 255)]), []),
        "row0": (dots(w, h, [(5, 0, 255)]), []),
        "last_col": (dots(w, h, [(w - 1, 6, 255)]), []),
        "last_row": (dots(w, h, [(6, h - 1, 255)]), []),
    }


def masked_maximum(w, h, ax, ay):
    """(image, live tracks, radius, quality): a strong dot at (ax, ay) whose pixel a radius-1 box masks, and a weak dot that passes
    the threshold of the unmasked maximum (0.3 of half the strong response) but not that of the masked one."""
    img = dots(w, h, [(ax, ay, 255), (ax + 15, ay + 10, 120)])
    return img, np.array([[ax + 0.5, ay + 0.5]], np.float32), 1, 0.3


def distance_pairs(w, h, x0, y0):
    """(image, gfttMinDistance for a scaled distance of 6.5, the accepted dots): four dots of falling brightness; the second lies at
    squared distance 41 < 42.25 from the first (rejected), the fourth at 45 >= 42.25 from the third (accepted)."""
    pts = [(x0, y0, 255), (x0 + 4, y0 + 5, 200), (x0 + 20, y0, 150), (x0 + 23, y0 + 6, 100)]
    return dots(w, h, pts), 6.5 * 720.0 / min(w, h), [pts[0][:2], pts[2][:2], pts[3][:2]]


def live_tracks(cand, seed, count=100):
    """Live tracks near the strongest candidates (fractional, so (int) matters)."""
    rng = np.random.default_rng(seed)
    m = min(count, len(cand))
    pick = rng.choice(min(len(cand), 4 * m), m, replace=False)
    return (cand[pick, :2] + rng.uniform(-1.5, 1.5, (m, 2))).astype(np.float32)


def edge_tracks(w, h):
    """A box clipped at each edge of the image and one inside."""
    return np.array([[w - 10.5, h * 0.4], [9.25, h * 0.6], [w * 0.5, 3.5], [w * 0.3, h - 2.5], [w * 0.7, h * 0.5]], np.float32)
