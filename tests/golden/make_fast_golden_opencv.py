"""Writes tests/golden/fast_golden_opencv.npz from a REAL OpenCV (cv2), when one is importable.

Not runnable where the project is built (no cv2 there): tests/fast_restatement.py was written from the algorithm and has not been
pinned against OpenCV; this fixture is what pins it (tests/test_fast_restatement.py picks the file up when it exists). Same seeded
inputs as tests/test_gpu_fast.py (tests/fast_cases.py: seeded_images, golden_prev), at the two small sizes so that the file stays far
below the size limit of a committed file. The calls are the reference's (src/tracker/feature_detector_legacy.cpp:141-174, :20-83):
    cv::FastFeatureDetector::create()  (threshold 10, TYPE_9_16)  with setNonmaxSuppression(true)
    detector->detect(image, keypoints, mask)    mask: 255, with a zero box per live track drawn as drawMask does
"""
import os
import sys

import numpy as np

try:
    import cv2
except ImportError:
    sys.exit("cv2 is not importable here: nothing written")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                   # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository root (hybvio_amd.synth)
import fast_cases as K  # noqa: E402


def draw_mask(prev, r, w, h):
    """MaskedFeatureDetector::drawMask: cv::Mat(h, w, CV_8U, 255) with mask(Rect(x0, y0, x1 - x0, y1 - y0)) = 0 per corner."""
    mask = np.full((h, w), 255, np.uint8)
    for px, py in prev:
        if not (0 < px < w and 0 < py < h):
            continue
        ix, iy = int(px), int(py)
        x0, x1 = (ix - r if ix - r > 0 else 0), (ix + r if ix + r < w - 1 else w - 1)
        y0, y1 = (iy - r if iy - r > 0 else 0), (iy + r if iy + r < h - 1 else h - 1)
        if x1 > x0 and y1 > y0:
            mask[y0:y1, x0:x1] = 0
    return mask


def as_rows(kps):
    return np.array([[k.pt[0], k.pt[1], k.response] for k in kps], np.float32).reshape(-1, 3)


out = dict(cv_version=cv2.__version__)
for w, h in ((33, 33), (97, 130)):
    for k, img in enumerate(K.seeded_images(w, h)):
        tag = f"{w}x{h}_{k}"
        out[f"img_{tag}"] = img
        for t in (10, 0, 40, 255):
            det = cv2.FastFeatureDetector_create(threshold=t, nonmaxSuppression=True, type=cv2.FAST_FEATURE_DETECTOR_TYPE_9_16)
            det.setNonmaxSuppression(True)
            kp = as_rows(det.detect(img, None))
            out[f"kp_{tag}_t{t}"] = kp                      # in OpenCV's order (row-major)
            if t == 10 and len(kp):
                prev = K.golden_prev(w, h, kp, k)
                out[f"prev_{tag}"] = prev
                for r in (2, 7, 30):
                    out[f"masked_{tag}_r{r}"] = as_rows(det.detect(img, draw_mask(prev, r, w, h)))
path = os.path.join(HERE, "fast_golden_opencv.npz")
np.savez_compressed(path, **out)
print(path, "written with OpenCV", cv2.__version__)
