"""numpy restatement of the reference's stereo track gate and detection filter (src/tracker/tracker.cpp:441-478, 266-311,
with computeEpipolarCurve :81-106, withinDistanceFromCurve :128-151, isPointInCrop :315-320,
markOutOfDetectionCropCornersAsFailed :322-346, markCornersFailedByEpipolarConstraint :348-376) and of OpticalFlow's status
mapping (src/tracker/optical_flow.cpp:52-58).

Test infrastructure only (imported by the tests, never by the product). It states what the device kernels
(hybvio_amd/csrc/stereo_gate.hip) compute, operation by operation: the camera math in binary64 through the CPU oracle's
tracker::Camera (oracle.orc.Camera), the curve points rounded to binary32, the distance tests on np.float32 scalars (each
operation rounds once, as the kernel built without FMA contraction does), the crop test in binary64.
"""
from __future__ import annotations

import math

import numpy as np

f32 = np.float32
TRACKED, FAILED_FLOW, FLOW_OUT_OF_RANGE, OUT_OF_RANGE, FAILED_EPIPOLAR_CHECK, BLACKLISTED = 0, 2, 4, 5, 6, 8
CURVE_POINTS = 8


class Params:
    """tracker.* parameters of the gate (codegen/parameter_definitions.c:210, 217, 246, 353) and cam0ToCam1 (4 x 4)."""

    def __init__(self, maxStereoEpipolarDistance=10.0, partOfImageToDetectFeatures=1.0, fisheyeCamera=False,
                 independentStereoOpticalFlow=False, cam0ToCam1=None):
        self.maxStereoEpipolarDistance = float(f32(maxStereoEpipolarDistance))
        self.partOfImageToDetectFeatures = float(partOfImageToDetectFeatures)
        self.fisheyeCamera = bool(fisheyeCamera)
        self.independentStereoOpticalFlow = bool(independentStereoOpticalFlow)
        self.cam0ToCam1 = np.eye(4) if cam0ToCam1 is None else np.asarray(cam0ToCam1, np.float64).reshape(4, 4)


def flow_status(lk_status, xy, w: int, h: int) -> np.ndarray:
    """optical_flow.cpp:52-58: FAILED_FLOW / TRACKED from the LK status, FLOW_OUT_OF_RANGE outside [0, w) x [0, h) (binary32;
    a NaN coordinate fails every comparison)."""
    xy = np.asarray(xy, f32).reshape(-1, 2)
    x, y = xy[:, 0], xy[:, 1]
    st = np.where(np.asarray(lk_status) == 0, FAILED_FLOW, TRACKED).astype(np.int32)
    with np.errstate(invalid="ignore"):
        out = (x < f32(0)) | (x >= f32(w)) | (y < f32(0)) | (y >= f32(h))
    st[out] = FLOW_OUT_OF_RANGE
    return st


def epipolar_dist(w: int, h: int, max_dist: float):
    """markCornersFailedByEpipolarConstraint's dist (a float product, a double division, a float) and dist2 = dist * dist in
    binary32 (std::pow(float, 2) is exact in double, so its rounding to float is the same value)."""
    prod = f32(max_dist) * f32(min(w, h))
    dist = f32(float(prod) / 720.0)
    return dist, dist * dist


def epipolar_curve(p, cam0, cam1, T):
    """computeEpipolarCurve: 8 binary32 points, or [] when pixelToRay or any rayToPixel fails. Also returns the angles of the
    camera-1 rays (for fisheye tolerance bookkeeping: theta against max_theta)."""
    ok, ray = cam0.pixel_to_ray(float(f32(p[0])), float(f32(p[1])))
    if not ok:
        return [], []
    curve, rays = [], []
    s = f32(0.5)
    for _ in range(CURVE_POINTS):
        r0 = [float(s) * ray[0], float(s) * ray[1], float(s) * ray[2]]
        r1 = np.array([((T[i, 0] * r0[0] + T[i, 1] * r0[1]) + T[i, 2] * r0[2]) + T[i, 3] for i in range(3)])
        rays.append(r1)
        ok, pix = cam1.ray_to_pixel(r1)
        if not ok:
            return [], rays
        curve.append((f32(pix[0]), f32(pix[1])))
        s = s * f32(2)
    return curve, rays


def within_distance_from_curve(p, curve, dist2):
    """withinDistanceFromCurve in binary32 -> (within, margin): margin = the smallest relative distance to dist2 of any
    squared distance the reference compares, or |t| / |t - 1| of a segment projection (how close the decision was)."""
    assert len(curve) > 0
    px, py = f32(p[0]), f32(p[1])
    d2 = float(dist2)
    margin = math.inf
    found = False
    with np.errstate(all="ignore"):
        for cx, cy in reversed(curve):
            dx, dy = cx - px, cy - py
            q = dx * dx + dy * dy
            margin = min(margin, abs(float(q) - d2) / d2)
            if q < dist2:
                found = True
                break
        if not found:
            for i in range(len(curve) - 1):
                c0x, c0y = curve[i]
                c1x, c1y = curve[i + 1]
                ex, ey = c1x - c0x, c1y - c0y
                s2 = ex * ex + ey * ey
                qx, qy = px - c0x, py - c0y
                t = (qx * ex + qy * ey) / s2
                if np.isfinite(t):
                    margin = min(margin, abs(float(t)), abs(float(t) - 1.0))
                if t > 0 and t < 1:
                    rx, ry = px - (c0x + t * ex), py - (c0y + t * ey)
                    q = rx * rx + ry * ry
                    margin = min(margin, abs(float(q) - d2) / d2)
                    if q < dist2:
                        found = True
                        break
    return found, margin


def epipolar_fails(p0, p1, cam0, cam1, T, dist2, max_theta1=None):
    """True when the curve of p0 is non-empty and p1 is not within dist of it. -> (fails, margin, theta_close)."""
    curve, rays = epipolar_curve(p0, cam0, cam1, T)
    theta_close = False
    if max_theta1 is not None:
        for r in rays:
            n = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
            if r[2] > 0 and abs(math.acos(r[2] / n) - max_theta1) < 1e-9:
                theta_close = True
    if not curve:
        return False, math.inf, theta_close
    within, margin = within_distance_from_curve(p1, curve, dist2)
    return not within, margin, theta_close


def in_crop(p, w: int, h: int, part: float) -> bool:
    """isPointInCrop: binary64 bounds, the point promoted to double."""
    xd = w * (1 - part) / 2
    yd = h * (1 - part) / 2
    x, y = float(f32(p[0])), float(f32(p[1]))
    return x >= xd and x < w - xd and y >= yd and y < h - yd


def out_of_detection_crop(p, cam, w: int, h: int, prm: Params) -> bool:
    """markOutOfDetectionCropCornersAsFailed for one corner."""
    if prm.fisheyeCamera and not cam.pixel_to_ray(float(f32(p[0])), float(f32(p[1])))[0]:
        return True
    if prm.partOfImageToDetectFeatures < 1.0 and not in_crop(p, w, h, prm.partOfImageToDetectFeatures):
        return True
    return False


def track_gate(corners, second_corners, stereo_status, blacklist, track_status, cam0, cam1, w, h, prm: Params,
               max_theta1=None, info=None):
    """tracker.cpp:441-478 -> new track statuses. second_corners None = mono. info (a list, optional) receives per feature
    (margin, theta_close) of the epipolar decision (inf / False where none was taken)."""
    ts = np.array(track_status, np.int32).copy()
    a = np.asarray(corners, f32).reshape(-1, 2)
    stereo = second_corners is not None
    b = np.asarray(second_corners, f32).reshape(-1, 2) if stereo else None
    _, dist2 = epipolar_dist(w, h, prm.maxStereoEpipolarDistance)
    epi = stereo and prm.maxStereoEpipolarDistance > 0 and not prm.independentStereoOpticalFlow
    for i in range(len(ts)):
        margin, close = math.inf, False
        if stereo:
            if stereo_status[i] == FAILED_FLOW:
                ts[i] = FAILED_FLOW
            if epi and ts[i] == TRACKED:
                fails, margin, close = epipolar_fails(a[i], b[i], cam0, cam1, prm.cam0ToCam1, dist2, max_theta1)
                if fails:
                    ts[i] = FAILED_EPIPOLAR_CHECK
        if out_of_detection_crop(a[i], cam0, w, h, prm):
            ts[i] = OUT_OF_RANGE
        if stereo and out_of_detection_crop(b[i], cam1, w, h, prm):
            ts[i] = OUT_OF_RANGE
        if blacklist is not None and blacklist[i]:
            ts[i] = BLACKLISTED
        if info is not None:
            info.append((margin, close))
    return ts


def detection_filter(corners, second_corners, stereo_status, cam0, cam1, w, h, prm: Params, max_theta1=None, info=None):
    """tracker.cpp:266-311 after the stereo LK of the new corners -> (kept corners, kept right corners or None, statuses)."""
    a = np.asarray(corners, f32).reshape(-1, 2)
    stereo = second_corners is not None
    b = np.asarray(second_corners, f32).reshape(-1, 2) if stereo else None
    st = np.array(stereo_status, np.int32).copy() if stereo else np.full(len(a), TRACKED, np.int32)
    _, dist2 = epipolar_dist(w, h, prm.maxStereoEpipolarDistance)
    for i in range(len(a)):
        margin, close = math.inf, False
        if stereo and prm.maxStereoEpipolarDistance > 0 and st[i] == TRACKED:
            fails, margin, close = epipolar_fails(a[i], b[i], cam0, cam1, prm.cam0ToCam1, dist2, max_theta1)
            if fails:
                st[i] = FAILED_EPIPOLAR_CHECK
        if out_of_detection_crop(a[i], cam0, w, h, prm):
            st[i] = OUT_OF_RANGE
        if stereo and out_of_detection_crop(b[i], cam1, w, h, prm):
            st[i] = OUT_OF_RANGE
        if info is not None:
            info.append((margin, close))
    keep = st == TRACKED
    return a[keep].copy(), (b[keep].copy() if stereo else None), st
