"""Literal restatement of the reference's optical-flow predictor, the yardstick of hv_flow_predict_batch_dev: the
OpticalFlowPredictor lambda of Session::applyTracker (src/odometry/backend.cpp:548-664), EKFStateIndex::widestBaseline
(src/odometry/ekf_state_index.cpp:312-339), extractCameraPoseTrail (src/odometry/triangulation.cpp:65-103),
triangulateWithTwoCameras without derivatives (:610-646), pinv (:1000-1002), util::toWorldToCamera / toCameraToWorld
(src/odometry/util.cpp:132-158), util::transformVec3ByMat4 (util.hpp:77-85), quat2rmat (util.cpp:10-26) and pixelToRay /
rayToPixel of the pinhole and the fisheye camera (src/tracker/camera.cpp:93-221, 264-398).

Test infrastructure only (not collected; nothing under hybvio_amd/ uses it). Pure numpy scalars, written ONCE over the scalar
type T: with T = np.float64 the text is the restatement (the operation order the device kernel follows), with T = np.longdouble
the truth both are judged by. Same expressions in the same order, so the two differ by rounding only. Literals are exact in both
types or binary64 parameter values both share (1e-5, the camera's derived constants). The index is
trail_index_restatement.Session's, the mean a plain vector in the filter's layout (POS 0, ORI 6, CAM 20, 7 per pose).

Two calls have no in-tree definition and are restated by their meaning, as oracle/triangulation_oracle.c does: pinv(A) of the
full-rank 3x2 A = (A'A)^-1 A', and imuToCamera.inverse(), which the caller supplies (hv_flow_predict_params.cameraToImu). A 4x4
product sums every entry in the order of the inner index.

world() at the end is the synthetic corpus the CPU and the GPU tests share. Nothing here reads the reference tree."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, (
    "tests/flow_predict_restatement.py needs an extended-precision np.longdouble (eps < 2e-19, x87 80-bit or wider); on this host "
    f"it has eps = {np.finfo(LD).eps}, no wider than binary64, so it cannot serve as the truth for binary64 kernels")

LEFT, RIGHT, STEREO = 0, 1, 2                                                           # OpticalFlowPredictor::Type
POS, ORI, CAM, POSE_DIM = 0, 6, 20, 7
MIN_TWO_CAMERA_FLOW_TRIANGULATION_BASELINE = 10                                        # backend.cpp:627
MIN_TRIANGULATION_DISTANCE = 3.0                                                        # parameter_definitions.c:213


def _vec(T, a):
    return [T(x) for x in np.asarray(a).reshape(-1)]


# ---- util.cpp, util.hpp -------------------------------------------------------------------------------------------------------------
def quat2rmat(T, q):                                                                    # util.cpp:10-26 -> row-major [9]
    two = T(2)
    return [q[0] * q[0] + q[1] * q[1] - q[2] * q[2] - q[3] * q[3], two * q[1] * q[2] - two * q[0] * q[3], two * q[1] * q[3] + two * q[0] * q[2],
            two * q[1] * q[2] + two * q[0] * q[3], q[0] * q[0] - q[1] * q[1] + q[2] * q[2] - q[3] * q[3], two * q[2] * q[3] - two * q[0] * q[1],
            two * q[1] * q[3] - two * q[0] * q[2], two * q[2] * q[3] + two * q[0] * q[1], q[0] * q[0] - q[1] * q[1] - q[2] * q[2] + q[3] * q[3]]


def mm4(A, B):
    return [((A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]) + A[4 * r + 3] * B[12 + c] for r in range(4) for c in range(4)]


def toWorldToCamera(T, position, orientation, imuToCamera):                             # util.cpp:132-142
    R, p = quat2rmat(T, orientation), position
    t = [((-R[3 * r]) * p[0] + (-R[3 * r + 1]) * p[1]) + (-R[3 * r + 2]) * p[2] for r in range(3)]
    worldToImu = [R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], T(0), T(0), T(0), T(1)]
    return mm4(imuToCamera, worldToImu)


def toCameraToWorld(T, position, orientation, cameraToImu):                             # util.cpp:144-158, the inverse supplied
    R, p = quat2rmat(T, orientation), position
    imuToWorld = [R[0], R[3], R[6], p[0], R[1], R[4], R[7], p[1], R[2], R[5], R[8], p[2], T(0), T(0), T(0), T(1)]
    return mm4(imuToWorld, cameraToImu)


def transformVec3ByMat4(M, v):                                                          # util.hpp:77-85
    return [((M[4 * i] * v[0] + M[4 * i + 1] * v[1]) + M[4 * i + 2] * v[2]) + M[4 * i + 3] for i in range(3)]


# ---- triangulation.cpp --------------------------------------------------------------------------------------------------------------
def _mm3(A, B):
    return [A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c] for r in range(3) for c in range(3)]


def _mmT3(A, B):
    return [A[3 * r] * B[3 * c] + A[3 * r + 1] * B[3 * c + 1] + A[3 * r + 2] * B[3 * c + 2] for r in range(3) for c in range(3)]


def _mv3(A, x):
    return [A[3 * r] * x[0] + A[3 * r + 1] * x[1] + A[3 * r + 2] * x[2] for r in range(3)]


def _mTv3(A, x):
    return [A[c] * x[0] + A[3 + c] * x[1] + A[6 + c] * x[2] for c in range(3)]


def historyIndices(i):                                                                  # ekf.cpp:544-554: historyPosition(i), -1 = current
    return (POS, ORI) if i == -1 else (CAM + POSE_DIM * i, CAM + POSE_DIM * i + 3)


def extractCameraPoseTrail(T, m, poseTrailIndex, imuToCam):                             # :65-103, one camera -> [(p, R)]
    Ric = [imuToCam[0], imuToCam[1], imuToCam[2], imuToCam[4], imuToCam[5], imuToCam[6], imuToCam[8], imuToCam[9], imuToCam[10]]
    baseline = [imuToCam[3], imuToCam[7], imuToCam[11]]
    trail = []
    for i in poseTrailIndex:                                                            # :83
        ip, io = historyIndices(i - 1)                                                  # :84-85
        R = _mm3(Ric, quat2rmat(T, m[io:io + 4]))                                       # :88
        t = _mTv3(R, baseline)
        trail.append(([m[ip + a] - t[a] for a in range(3)], R))                         # :89-93
    return trail


def pinv32(T, A):                                                                       # :1000-1002; A row-major 3x2 -> row-major 2x3
    a = A[0] * A[0] + A[2] * A[2] + A[4] * A[4]
    b = A[0] * A[1] + A[2] * A[3] + A[4] * A[5]
    d = A[1] * A[1] + A[3] * A[3] + A[5] * A[5]
    det = a * d - b * b
    return [(d * A[2 * c] - b * A[2 * c + 1]) / det for c in range(3)] + [(-b * A[2 * c] + a * A[2 * c + 1]) / det for c in range(3)]


def triangulateWithTwoCameras(T, pose0, pose1, ip0, ip1):                               # :610-646
    (p0, R0), (p1, R1) = pose0, pose1
    C = _mmT3(R0, R1)                                                                   # :624
    d01 = [p1[a] - p0[a] for a in range(3)]
    b = _mv3(R0, d01)                                                                   # :625
    v0, v1 = [ip0[0], ip0[1], T(1)], [ip1[0], ip1[1], T(1)]                             # :627-628
    n0 = np.sqrt(v0[0] * v0[0] + v0[1] * v0[1] + v0[2] * v0[2])
    n1 = np.sqrt(v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2])
    vn0, vn1 = [x / n0 for x in v0], [x / n1 for x in v1]                               # :633-636
    Cvn1 = _mv3(C, vn1)
    A = [vn0[0], -Cvn1[0], vn0[1], -Cvn1[1], vn0[2], -Cvn1[2]]                          # :638-640
    iA = pinv32(T, A)                                                                   # :642
    s0 = iA[0] * b[0] + iA[1] * b[1] + iA[2] * b[2]                                     # :643
    return [s0 * vn0[a] for a in range(3)]                                              # :644


# ---- camera.cpp ---------------------------------------------------------------------------------------------------------------------
class Camera:
    """tracker::Camera over the fields of an initialised hv_camera_model (capi.camera_model): the intrinsic parameters and the
    constants the constructors derive (kinv, max_theta, max_r, the Newton start table), all binary64 values that both precisions
    share. pixelToRay / rayToPixel return (success, value, tests): tests = (quantity, threshold, scale) of every validity
    comparison made, for the tests' "undecided" rule (|quantity - threshold| against the scale: the ray's length for a sign test)."""

    def __init__(self, model):
        g = lambda k: getattr(model, k)
        self.kind, self.fx, self.fy, self.ppx, self.ppy = g("kind"), g("fx"), g("fy"), g("ppx"), g("ppy")
        self.coeffs = list(g("coeffs"))
        self.distortion_enabled, self.rotation_enabled = bool(g("distortion_enabled")), bool(g("rotation_enabled"))
        self.rotation, self.kinv = list(g("rotation")), list(g("kinv"))
        self.max_theta, self.max_r, self.table = g("max_theta"), g("max_r"), list(g("table"))[:g("n_table")]

    def _pin_distort(self, T, x, y):                                                    # camera.cpp:93-106 -> x, y, J
        if not self.distortion_enabled:
            return x, y, [T(1), T(0), T(0), T(1)]
        k = _vec(T, self.coeffs)
        r2 = x * x + y * y
        theta = T(1) + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))
        dth = k[0] + r2 * (k[1] * T(2) + r2 * k[2] * T(3))
        J = [theta + x * dth * T(2) * x, x * dth * T(2) * y, y * dth * T(2) * x, theta + y * dth * T(2) * y]
        return x * theta, y * theta, J

    def _fish_distort(self, T, theta):                                                  # :264-281 -> r, dr/dtheta
        if not self.distortion_enabled:
            return theta, T(1)
        k, t = _vec(T, self.coeffs), theta
        t2 = t * t
        der = T(1) + T(3) * t2 * (k[0] + T(5) / T(3) * t2 * (k[1] + T(7) / T(5) * t2 * (k[2] + T(9) / T(7) * t2 * k[3])))
        return t * (T(1) + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3])))), der

    def _fish_newton(self, T, r, theta0):                                               # :283-300
        eps = T(0.01) / ((T(self.fx) + T(self.fy)) * T(0.5))
        theta = theta0
        for _ in range(20):
            v, d = self._fish_distort(T, theta)
            dt = (v - r) / d
            theta = theta - dt
            if abs(dt) < eps:
                return theta if theta > T(0) else T(0)
        return T(-1)

    def pixelToRay(self, T, px, py):
        px, py = T(px), T(py)
        if self.kind == 0:                                                              # :169-180
            x, y = (px - T(self.ppx)) / T(self.fx), (py - T(self.ppy)) / T(self.fy)
            if self.distortion_enabled:                                                 # :108-123 Newton
                dx, dy, it = x, y, 0
                while True:
                    qx, qy, J = self._pin_distort(T, x, y)
                    idet = T(1) / (J[0] * J[3] - J[1] * J[2])
                    ex, ey = dx - qx, dy - qy
                    sx = (J[3] * idet) * ex + (-J[1] * idet) * ey
                    sy = (-J[2] * idet) * ex + (J[0] * idet) * ey
                    x, y = x + sx, y + sy
                    nrm = np.sqrt(sx * sx + sy * sy)
                    it += 1
                    if not (nrm > T(1e-5) and it < 100):
                        break
            n = np.sqrt(x * x + y * y + T(1))
            r = [x / n, y / n, T(1) / n]
            if self.rotation_enabled:
                r = _mv3(_vec(T, self.rotation), r)
            return True, r, []
        Ki = _vec(T, self.kinv)                                                         # :353-375
        u, v = Ki[0] * px + Ki[1] * py + Ki[2], Ki[3] * px + Ki[4] * py + Ki[5]
        r = np.sqrt(u * u + v * v)
        dxn, dyn = u / r, v / r
        theta = r
        if r > T(self.max_r):
            theta = T(self.max_theta)
        elif self.distortion_enabled:
            n = len(self.table)
            f = r / T(self.max_r)
            if not f > T(0):
                f = T(0)
            th = self._fish_newton(T, r, T(self.table[min(int(f * T(n)), n - 1)]))
            theta = r if th < T(0) else th
        s = np.sin(theta)
        return bool(r <= T(self.max_r)), [s * dxn, s * dyn, np.cos(theta)], [(r, T(self.max_r), T(self.max_r))]

    def rayToPixel(self, T, ray):
        if self.kind == 0:                                                              # :182-205
            r = list(ray)
            if self.rotation_enabled:
                r = _mTv3(_vec(T, self.rotation), r)
            scale = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
            if r[2] <= T(0):
                return False, None, [(r[2], T(0), scale)]
            iz = T(1) / r[2]
            x, y, _ = self._pin_distort(T, r[0] * iz, r[1] * iz)
            return True, [T(self.fx) * x + T(0) * y + T(self.ppx) * (r[2] * iz), T(0) * x + T(self.fy) * y + T(self.ppy) * (r[2] * iz)], [(r[2], T(0), scale)]
        scale = np.sqrt(ray[0] * ray[0] + ray[1] * ray[1] + ray[2] * ray[2])
        if ray[2] <= T(0):                                                              # :377-398
            return False, None, [(ray[2], T(0), scale)]
        inv = T(1) / np.sqrt(ray[0] * ray[0] + ray[1] * ray[1] + ray[2] * ray[2])
        theta = np.arccos(ray[2] * inv)
        tests = [(ray[2], T(0), scale), (theta, T(self.max_theta), T(self.max_theta))]
        if theta > T(self.max_theta):
            return False, None, tests
        r, _ = self._fish_distort(T, theta)
        n2 = ray[0] * ray[0] + ray[1] * ray[1]
        dx, dy = ray[0], ray[1]
        if n2 > T(0):
            n = np.sqrt(n2)
            dx, dy = dx / n, dy / n
        u, v = r * dx, r * dy
        return True, [T(self.fx) * u + T(0) * v + T(self.ppx), T(0) * u + T(self.fy) * v + T(self.ppy)], tests


# ---- ekf_state_index.cpp ------------------------------------------------------------------------------------------------------------
def widestBaseline(T, index, trackId):                                                  # :312-339 -> ok, keyframe0, keyframe1, ip0, ip1
    keyframes = index.keyframes
    poseCount = len(keyframes)
    if poseCount < 2:                                                                   # :319
        return False, 0, 0, None, None
    ok, keyframe0, imagePoint0 = False, 0, None
    for keyframe0 in range(poseCount):                                                  # :322-328
        if trackId in keyframes[keyframe0].features:
            imagePoint0 = _vec(T, keyframes[keyframe0].features[trackId].frames[0].normalizedImagePoint)
            ok = True
            break
    if not ok:                                                                          # :329
        return False, 0, 0, None, None
    keyframe1, imagePoint1 = poseCount - 1, None
    while True:                                                                         # :330-336
        if trackId in keyframes[keyframe1].features:
            imagePoint1 = _vec(T, keyframes[keyframe1].features[trackId].frames[0].normalizedImagePoint)
            break
        if keyframe1 == 0:
            break
        keyframe1 -= 1
    assert keyframe1 >= keyframe0                                                       # :337
    return keyframe0 != keyframe1, keyframe0, keyframe1, imagePoint0, imagePoint1


# ---- backend.cpp:548-664 ------------------------------------------------------------------------------------------------------------
class Params:
    def __init__(self, imuToCamera=None, secondImuToCamera=None, minDistance=MIN_TRIANGULATION_DISTANCE,
                 minBaselinePoses=MIN_TWO_CAMERA_FLOW_TRIANGULATION_BASELINE):
        eye = np.eye(4)
        self.imuToCamera = np.asarray(eye if imuToCamera is None else imuToCamera, np.float64).reshape(4, 4)
        self.secondImuToCamera = np.asarray(eye if secondImuToCamera is None else secondImuToCamera, np.float64).reshape(4, 4)
        self.cameraToImu, self.secondCameraToImu = np.linalg.inv(self.imuToCamera), np.linalg.inv(self.secondImuToCamera)   # binary64 parameters
        self.predictOpticalFlowMinTriangulationDistance, self.minBaselinePoses = minDistance, minBaselinePoses


def predict(T, index, mean, par, cameras, predictionType, c0, trackIds, distances=None):
    """The lambda: c0 [n][2] binary32 corners, trackIds [n] -> one dict per track: c1 (two np.float32), distance, triangulated
    (the two-camera triangulation ran), pf2 (its pf(2), else None), in_front, clamped, p2r / r2p (the camera calls' outcomes; r2p
    None when pixelToRay failed: && does not evaluate it), tests (the validity comparisons made), pixel1 (unrounded, or None).
    cameras: (first, second) Camera. distances: reuse these instead of triangulating (the device's reuse_distance)."""
    with np.errstate(all="ignore"):                                                     # non-finite means are allowed: the arithmetic runs
        return _predict(T, index, mean, par, cameras, predictionType, c0, trackIds, distances)


def _predict(T, index, mean, par, cameras, predictionType, c0, trackIds, distances):
    m = _vec(T, mean)
    poseTrailIndex = list(range(len(index.keyframes)))                                  # createFullIndex, :557
    trail = extractCameraPoseTrail(T, m, poseTrailIndex, _vec(T, par.imuToCamera))      # :559-560, the first camera's part
    hist0, cur = historyIndices(0), historyIndices(-1)
    pos = lambda ix: (m[ix[0]:ix[0] + 3], m[ix[1]:ix[1] + 4])
    if predictionType == LEFT:                                                          # :575-586
        camera0 = camera1 = cameras[0]
        camToWorld0 = toCameraToWorld(T, *pos(hist0), _vec(T, par.cameraToImu))
        worldToCam1 = toWorldToCamera(T, *pos(cur), _vec(T, par.imuToCamera))
    elif predictionType == RIGHT:                                                       # :587-598
        camera0 = camera1 = cameras[1]
        camToWorld0 = toCameraToWorld(T, *pos(hist0), _vec(T, par.secondCameraToImu))
        worldToCam1 = toWorldToCamera(T, *pos(cur), _vec(T, par.secondImuToCamera))
    else:                                                                               # :599-612
        assert predictionType == STEREO
        camera0, camera1 = cameras
        camToWorld0 = toCameraToWorld(T, *pos(cur), _vec(T, par.cameraToImu))
        worldToCam1 = toWorldToCamera(T, *pos(cur), _vec(T, par.secondImuToCamera))
    out = []
    for i in range(len(c0)):                                                            # :613
        rec = dict(triangulated=False, pf2=None, in_front=False)
        distance = T(-1)                                                                # :615
        if distances is not None:
            distance = T(distances[i])
        else:
            ok, keyframe0, keyframe1, imagePoint0, imagePoint1 = widestBaseline(T, index, trackIds[i])   # :619-620
            rec["span"] = keyframe1 - keyframe0 if ok else None
            if ok and keyframe1 - keyframe0 >= par.minBaselinePoses:                    # :628
                pf = triangulateWithTwoCameras(T, trail[keyframe0], trail[keyframe1], imagePoint0, imagePoint1)   # :629-635
                rec.update(triangulated=True, pf2=pf[2], pf_scale=np.sqrt(pf[0] * pf[0] + pf[1] * pf[1] + pf[2] * pf[2]))
                if pf[2] > T(0):                                                        # :638-640
                    distance = np.sqrt(pf[0] * pf[0] + pf[1] * pf[1] + pf[2] * pf[2])
                    rec["in_front"] = True
            rec["raw_distance"] = distance
            mn = T(par.predictOpticalFlowMinTriangulationDistance)                      # :644-645
            rec["clamped"] = bool(distance < mn)
            if distance < mn:
                distance = mn
        rec["distance"] = distance
        pixel0 = [T(np.float32(c0[i][0])), T(np.float32(c0[i][1]))]                     # :648-649
        success, ray0, tests = camera0.pixelToRay(T, pixel0[0], pixel0[1])              # :651
        ray0 = [x * distance for x in ray0]                                             # :652
        p = transformVec3ByMat4(camToWorld0, ray0)                                      # :654
        ray1 = transformVec3ByMat4(worldToCam1, p)                                      # :655
        rec["p2r"], rec["r2p"], rec["pixel1"] = success, None, None
        if success:                                                                     # :657
            rec["r2p"], pixel1, t2 = camera1.rayToPixel(T, ray1)
            tests = tests + t2
            if rec["r2p"]:
                rec["pixel1"] = pixel1
        chosen = rec["pixel1"] if rec["pixel1"] is not None else pixel0                 # :658-662
        rec["c1"] = (np.float32(chosen[0]), np.float32(chosen[1]))
        rec["tests"] = tests
        out.append(rec)
    return out


# ---- the synthetic corpus -------------------------------------------------------------------------------------------------------------
def _quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a])


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def world_pose(f, seed):
    """The true pose of frame f of sequence `seed`: the IMU position in the world and the quaternion whose quat2rmat is the
    world-to-IMU rotation. 0.12 m per frame mostly sideways (1.2 m across ten keyframes), a slow yaw."""
    ph = 0.7 * seed
    p = np.array([0.12 * f, 0.25 * np.sin(0.15 * f + ph), 0.02 * f + 0.1 * np.cos(0.1 * f + ph)])
    q = _qmul(_quat([0.1, 1.0, 0.05], 0.004 * f + 0.01 * np.sin(0.2 * f + ph)), _quat([1.0, 0.2, 0.1], 0.03 * np.sin(ph)))
    return p, q / np.linalg.norm(q)


def camera_frame(pose, imuToCam):
    """(R, c): x_cam = R (X - c), as extractCameraPoseTrail forms them."""
    p, q = pose
    R = np.asarray(imuToCam)[:3, :3] @ np.array(quat2rmat(np.float64, [np.float64(x) for x in q])).reshape(3, 3)
    return R, p - R.T @ np.asarray(imuToCam)[:3, 3]


def world(trail_params, normalize, ocams, par, frames, seed, M, width=752, height=480, beyond=None, p_swap=0.15, p_near=0.2,
          p_nonkey=0.08):
    """One sequence of `frames` frames of 3-D points (depths 1 .. 15 m, a fifth of them nearer than 3 m) seen from world_pose()
    through the oracle cameras `ocams` and driven through trail_index_restatement.Session with synthetic visit outcomes, as
    trail_index_restatement.drive does with random pixels. A track is born with a planned life, and some are replaced 10, 11 and 12 frames
    before the end, so that the spans 9, 10 and 11 are common when the sequence ends; a share p_swap of the tracks shows its observations in reverse order (the point
    triangulates behind the camera, from healthy rays). Yields per frame the dict trail_index_restatement.drive yields (the
    members the device driver reads) and, after the last frame, dict(final=True, session, table, poses): the table of the
    frame that follows -- the survivors at their last corners plus new tracks that have no column -- and the true pose of
    every frame number. beyond: callable (rng) -> a pixel outside the valid field of view, given to some of the new tracks."""
    import trail_index_restatement as TR
    rng = np.random.default_rng(seed)
    p = trail_params
    ses = TR.Session(p, normalize)
    stereo = p.useStereo
    imu2cam = (par.imuToCamera, par.secondImuToCamera)
    frames_cam = lambda f: [camera_frame(world_pose(f, seed), imu2cam[c]) for c in range(2 if stereo else 1)]

    def project(X, f):
        out = []
        for c, (R, ctr) in enumerate(frames_cam(f)):
            x = R @ (X - ctr)
            if x[2] <= 0.3:
                return None
            ok, pix = ocams[c].ray_to_pixel(x)
            if not ok or not (15 <= pix[0] <= width - 15 and 15 <= pix[1] <= height - 15):
                return None
            out.append((np.float32(pix[0]), np.float32(pix[1])))
        return out

    def shown(tr, f):                                                                   # the frame whose projection the track shows at frame f
        return tr["born"] + tr["dies"] - f if tr["swap"] else f

    def born(f, life, swap):
        dies = min(f + life, frames)                                                   # `frames` itself is the frame the predictor runs on
        for _ in range(200):
            R, ctr = frames_cam((f + dies) // 2)[0]
            depth = rng.uniform(1.0, 3.0) if rng.random() < p_near else rng.uniform(3.0, 15.0)
            ok, ray = ocams[0].pixel_to_ray(rng.uniform(40, width - 40), rng.uniform(40, height - 40))
            if not ok or ray[2] <= 0:
                continue
            X = ctr + R.T @ (ray / ray[2] * depth)
            tr = dict(X=X, born=f, dies=dies, swap=swap and dies - f >= 4)
            if all(project(X, g) is not None for g in range(f, dies + 1)):
                return tr
        raise AssertionError("no visible point found")

    lives = [3, 5, 7, 9, 10, 11, 12, 13, 15, 18, 22, 30]
    tracks, next_id, t = [], 1, 0.0
    for f in range(frames + 1):
        tracks = [tr for tr in tracks if tr["dies"] >= f and not tr.get("gone")]
        fill = M if f % 5 == 0 else int(rng.integers(max(3 * M // 4, 1), M + 1))
        turnover = frames - f in (10, 11, 12)                                           # tracks born here end the sequence with span 9, 10, 11
        if turnover and tracks:
            keep = rng.permutation(len(tracks))[:max(len(tracks) - max(M // 8, 2), 0)]
            tracks, fill = [tracks[i] for i in sorted(keep)], M
        if f == frames and tracks:                                                      # the predictor's table: some tracks lost, some new, padding left
            keep = rng.permutation(len(tracks))[:max(len(tracks) - max(M // 8, 2), 0)]
            tracks, fill = [tracks[i] for i in sorted(keep)], M - 2 - seed % 3
        while len(tracks) < fill:
            swap = bool(rng.random() < p_swap)
            life = frames - f + int(rng.integers(0, 3)) if turnover else int(rng.choice(lives))
            tr = born(f, max(life, 13) if swap else life, swap)
            tr["id"], next_id = next_id, next_id + 1
            if beyond is not None and rng.random() < 0.12:
                tr["beyond"] = np.asarray(beyond(rng), np.float32)
            tracks.append(tr)
        table = []
        for tr in tracks:
            px = project(tr["X"], shown(tr, f))
            if "beyond" in tr:
                px[0] = (tr["beyond"][0], tr["beyond"][1])
            table.append((tr["id"], px[0], px[1] if stereo else None))
        if f == frames:
            poses = {g + 1: world_pose(g, seed) for g in range(frames + 1)}
            yield dict(final=True, session=ses, table=table, poses=poses, frame_num=f + 1,
                       swapped={tr["id"] for tr in tracks if tr["swap"]})
            return
        keyframe = f < p.cameraTrailLength + 3 or rng.random() >= p_nonkey
        t += 0.05
        draws = rng.integers(0, 2 ** 32, M, dtype=np.uint32)
        sel = ses.select(table, ocams, keyframe, True, f + 1, t, draws)
        tri, gate = TR.synthetic_outcomes(rng, p, len(sel["candidates"]), "limits" if rng.random() < 0.6 else "early")
        stationary = bool(rng.random() < 0.3)
        fin = ses.finish(tri, gate, stationary)
        yield dict(frame=f, table=table, keyframe=keyframe, full=True, frame_num=f + 1, time=t, draws=draws, select=sel, tri=tri, gate=gate,
                   stationary=stationary, finish=fin)
        gone = set(fin["delete_ids"])
        for tr in tracks:
            if tr["id"] in gone and rng.random() < 0.5:
                tr["gone"] = True


def mean_of(session, poses, frame_num, n_state, rng, noise=1e-3):
    """The filter mean at the time of the prediction: the current pose = the true pose of frame `frame_num`, history pose k - 1
    = the true pose of the frame keyframe k was stamped with, plus noise; every other entry random."""
    m = rng.normal(0.0, 1.0, n_state)
    kfs = session.ekfStateIndex.keyframes
    for k in range(len(kfs)):
        pose = poses[frame_num] if k == 0 else poses[kfs[k].frameNumber]
        ip, io = historyIndices(k - 1)
        q = pose[1] + rng.normal(0.0, noise, 4)
        m[ip:ip + 3], m[io:io + 4] = pose[0] + rng.normal(0.0, noise, 3), q / np.linalg.norm(q)
    return m


# ---- the cases the CPU and the GPU tests share -----------------------------------------------------------------------------------------
PLAIN = dict(kind="pinhole", fx=458.6, fy=457.3, ppx=367.2, ppy=248.4)
RADIAL = dict(PLAIN, coeffs=[-0.28, 0.07, 0.0])
_c, _s = np.cos(0.02), np.sin(0.02)
ROTATED = dict(PLAIN, rotation=[[_c, 0.0, _s], [0.0, 1.0, 0.0], [-_s, 0.0, _c]])
FISHEYE = dict(kind="fisheye", fx=190.9, fy=190.9, ppx=376.0, ppy=240.0, coeffs=[0.0034, 0.0007, -0.002, 0.0002], max_valid_fov_deg=150.0)
# name -> (maxTracks, n_sets, trail, stereo, cameras, types): three sets at 32 tracks, mono and stereo, a fisheye pair, a trail too
# short for any triangulation, and once more tracks than the workgroup has threads
CASES = {
    "stereo": (32, 3, 20, True, (RADIAL, ROTATED), (LEFT, RIGHT, STEREO)),
    "mono": (32, 3, 20, False, (PLAIN, PLAIN), (LEFT,)),
    "fisheye": (32, 3, 20, True, (FISHEYE, FISHEYE), (LEFT, STEREO)),
    "trail5": (32, 3, 5, True, (RADIAL, RADIAL), (LEFT, RIGHT, STEREO)),
    "many": (300, 1, 20, True, (PLAIN, ROTATED), (LEFT, STEREO)),
}
TURNED_SET = 2                                                                          # its current pose is yawed by 1.2 rad: rayToPixel failures
_CACHE = {}


def _rot(axis, angle):
    return np.array(quat2rmat(np.float64, [np.float64(x) for x in _quat(axis, angle)])).reshape(3, 3)


def imu_to_camera_pair():
    A, B = np.eye(4), np.eye(4)
    A[:3, :3], A[:3, 3] = _rot([1.0, 0.3, -0.2], 0.11), [0.05, -0.02, 0.01]
    B[:3, :3], B[:3, 3] = _rot([1.0, 0.3, -0.2], 0.11) @ _rot([0.0, 1.0, 0.0], 0.015), [-0.06, -0.021, 0.012]
    return A, B


def stereo_c0(xy):
    """The c0 of the STEREO call in these tests: the table corners moved a little, as the temporal LK would have."""
    return (np.asarray(xy, np.float32) + np.array([1.5, -0.75], np.float32)).astype(np.float32)


def undecided(rest, truth):
    """The issue's rule for one point: the restatement and the truth disagree on a branch, or the truth's pf(2), distance - m
    or a camera validity quantity lies within 1e-9 relative of its threshold."""
    tol = LD(1e-9)
    for k in ("triangulated", "in_front", "clamped", "p2r", "r2p"):
        if rest.get(k) != truth.get(k):
            return True
    if truth["triangulated"] and abs(truth["pf2"]) <= tol * truth["pf_scale"]:
        return True
    if "raw_distance" in truth and abs(truth["raw_distance"] - LD(MIN_TRIANGULATION_DISTANCE)) <= tol * LD(MIN_TRIANGULATION_DISTANCE):
        return True
    return any(abs(q - thr) <= tol * scale for q, thr, scale in truth["tests"])


def case(name):
    """Everything about one case, computed once: the frames that drive the device index (per set), the final tables and means,
    and per type and set the restatement's and the truth's records."""
    if name in _CACHE:
        return _CACHE[name]
    import ransac3_restatement as R3
    import trail_index_restatement as TR
    from hybvio_amd import capi
    from oracle import orc
    M, S, trail, stereo, specs, types = CASES[name]
    frames = 25 if trail >= 20 else 12
    kw = dict(cameraTrailLength=trail, cameraTrailHanoiLength=3 if trail >= 20 else 2, useStereo=stereo, maxTracks=M)
    p = TR.Params(**kw)
    gp = capi.trail_index_default_params(**{k: int(v) for k, v in kw.items()})
    args = lambda s: ((s["kind"], s["fx"], s["fy"], s["ppx"], s["ppy"]), {k: v for k, v in s.items() if k not in ("kind", "fx", "fy", "ppx", "ppy")})
    ocams = tuple(orc.Camera(*args(s)[0], **args(s)[1]) for s in specs)
    gcams = tuple(capi.camera_model(*args(s)[0], **args(s)[1]) for s in specs)
    rcams = tuple(Camera(g) for g in gcams)
    A, B = imu_to_camera_pair()
    par = Params(A, B)
    fpar = capi.flow_predict_default_params(A, B)
    assert np.array_equal(np.array(fpar.cameraToImu[:]).reshape(4, 4), par.cameraToImu)
    beyond = (lambda rng: rng.uniform([0, 0], [40, 30])) if specs[0]["kind"] == "fisheye" else None
    n_state = CAM + POSE_DIM * trail
    seed0 = 4100 + 37 * sum(map(ord, name))
    seqs, finals, means = [], [], np.zeros((S, n_state))
    tab = dict(n_tracks=np.zeros(S, np.int32), ids=np.full((S, M), -77, np.int32), xy=np.full((S, M, 2), -5e5, np.float32),
               second_xy=np.full((S, M, 2), -5e5, np.float32))
    for s in range(S):
        recs = list(world(p, R3.normalize_pixel, ocams, par, frames, seed0 + s, M, beyond=beyond))
        fin = recs.pop()
        assert fin.get("final")
        rng = np.random.default_rng(seed0 + 1000 + s)
        m = mean_of(fin["session"], fin["poses"], fin["frame_num"], n_state, rng)
        if s == TURNED_SET:
            q = _qmul(m[ORI:ORI + 4], _quat([0.0, 1.0, 0.0], 1.2))
            m[ORI:ORI + 4] = q / np.linalg.norm(q)
        means[s] = m
        n = len(fin["table"])
        tab["n_tracks"][s] = n
        tab["ids"][s, :n] = [t[0] for t in fin["table"]]
        tab["xy"][s, :n] = [t[1] for t in fin["table"]]
        if stereo:
            tab["second_xy"][s, :n] = [t[2] for t in fin["table"]]
        seqs.append(recs); finals.append(fin)
    c0 = {LEFT: tab["xy"], RIGHT: tab["second_xy"], STEREO: stereo_c0(tab["xy"])}
    results = {}
    for ty in types:
        results[ty] = []
        for s in range(S):
            n = int(tab["n_tracks"][s])
            a = (finals[s]["session"].ekfStateIndex, means[s], par, rcams, ty, c0[ty][s, :n], tab["ids"][s, :n].tolist())
            results[ty].append((predict(np.float64, *a), predict(LD, *a)))
    out = dict(name=name, M=M, S=S, trail=trail, stereo=stereo, types=types, p=p, gp=gp, par=par, fpar=fpar, ocams=ocams, gcams=gcams,
               rcams=rcams, n_state=n_state, seqs=seqs, finals=finals, means=means, table=tab, c0=c0, results=results)
    _CACHE[name] = out
    return out
