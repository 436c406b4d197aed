"""Writes tests/golden/stereo_bm_golden_opencv.npz from a REAL OpenCV (cv2), when one is importable.

Not runnable where the project is built (no cv2 there): tests/stereo_bm_restatement.py was written from the algorithm and has not
been pinned against OpenCV; this fixture is what pins it (tests/test_stereo_bm_restatement.py picks the file up when it exists and
skips until then). Same seeded scenes as tests/test_gpu_stereo_bm.py (tests/stereo_bm_cases.py), at its three small shapes, so the
file stays far below the size limit of a committed file. The calls are the reference's (src/tracker/stereo_disparity.cpp:52-63):
    cv::StereoBM::create(nd)  with setSpeckleWindowSize(500) and setSpeckleRange(10)
    stereoMatcher->compute(left, right, disparity)      disparity: CV_16S, disparity x 16
The fixture also keeps the prefiltered-free intermediate that settles the doubts one at a time: the result without the speckle
filter (speckle window 0), and cv::filterSpeckles applied on it with maxDiff 10 and with maxDiff 160, to tell the unscaled range
from a scaled one.
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
import stereo_bm_cases as K  # noqa: E402

out = dict(cv_version=cv2.__version__)
nds = []
i = 0
for w, h, nd in K.SHAPES:
    for left, right in K.scenes(w, h, nd):
        bm = cv2.StereoBM_create(numDisparities=nd)
        bm.setSpeckleWindowSize(500)
        bm.setSpeckleRange(10)
        out[f"left_{i}"], out[f"right_{i}"] = left, right
        out[f"disp_{i}"] = bm.compute(left, right)
        raw = cv2.StereoBM_create(numDisparities=nd)
        raw.setSpeckleWindowSize(0)
        out[f"raw_{i}"] = raw.compute(left, right)
        for diff in (10, 160):
            m = out[f"raw_{i}"].copy()
            cv2.filterSpeckles(m, -16, 500, diff)
            out[f"speckles{diff}_{i}"] = m
        nds.append(nd)
        i += 1
out["nd"] = np.array(nds, np.int32)
path = os.path.join(HERE, "stereo_bm_golden_opencv.npz")
np.savez_compressed(path, **out)
print(path, "written with OpenCV", cv2.__version__)
