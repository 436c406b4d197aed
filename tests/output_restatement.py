"""Literal restatement of what a session hands back at the end of a frame, the yardstick of hv_output_dev: Session::process's output
block (src/odometry/backend.cpp:840-860), SlamOdometryCoordinateTransformer (:42-96), EKF::transformTo / translateTo
(src/odometry/ekf.cpp:696-758), Output::setFromEKF (src/odometry/output.cpp:50-77), computePose (backend.cpp:1368-1386),
getPointCloud (:255-280) over the point-cloud lines of the visit loop (:905, 1066-1070, 1118, 1124, 1191, 1239-1251), Control's
overwrite of t and trackingStatus (src/odometry/control.cpp:117-128), convertOutputPose (src/api/api.cpp:726-742) and
util::toOdometryPose / toWorldToCamera (src/odometry/util.cpp:121-142).

Test infrastructure only (not collected; nothing under hybvio_amd/ uses it). Pure numpy scalars, written ONCE over the scalar type
T like tests/flow_predict_restatement.py, whose quat2rmat, mm4, toWorldToCamera and transformVec3ByMat4 it shares: with
T = np.float64 the text is the restatement (the operation order the device kernel follows), with T = np.longdouble the truth both
are judged by.

Three calls have no in-tree definition and are restated by their meaning:
- rmat2quat = Eigen::Quaterniond(Matrix3d): the trace branch and the three largest-diagonal branches, in Eigen's order;
- Matrix4d::inverse(): the cofactor expansion over the 2 x 2 minors of the upper and the lower row pair, the determinant inverted
  once (the convention of the project's 3 x 3 inverses);
- the dense products of transformTo, tmp = P * A' and P = A * tmp: A is block diagonal, so entry (i, j) of a diagonal block is
  sum_k A(i, k) * (sum_l P(k, l) * A(j, l)) over the block, every other term an exact zero, every identity block a copy.

One deliberate deviation (hybvio_hip.h): with exactly one historical pose the reference leaves trail element 0 as setFromEKF of
its coordinate filter wrote it; here it is computePose(0) like every other element.

The index and the visit arrays enter in the layout the device entries write (hv_trail_index, hv_ekf_visual_frame_ragged_dev), one
set at a time. case() at the end is the scripted corpus the CPU and the GPU tests share. Nothing here reads the reference tree."""
import functools

import numpy as np

from flow_predict_restatement import LD, mm4, quat2rmat, toWorldToCamera, transformVec3ByMat4

POS, VEL, ORI, BGA, INER, CAM, POSE_DIM = 0, 3, 6, 10, 20, 20, 7
TRI_OK, TRI_BEHIND, TRI_NOT_VISITED = 0, 2, -1
PREPARE_VU_OK, PREPARE_VU_BEHIND = 0, 2
INLIER, NOT_COMPUTED, CHI2 = 0, 1, 3                                                   # VuOutlierStatus
POINT_POSE_TRAIL, POINT_OUTLIER = 1, 4                                                 # PointFeature::Status
IDENTITY = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]


def _vec(T, a):
    return [T(x) for x in np.asarray(a).reshape(-1)]


# ---- Eigen ------------------------------------------------------------------------------------------------------------------------
def rmat2quat(T, R):
    """Eigen::Quaterniond(Matrix3d), R row-major [9] -> ((w, x, y, z), branch); branch 0: trace > 0, 1 + i: diagonal entry i."""
    t = (R[0] + R[4]) + R[8]
    q = [T(0)] * 4
    if t > T(0):
        t = np.sqrt(t + T(1))
        q[0] = T(0.5) * t
        t = T(0.5) / t
        q[1], q[2], q[3] = (R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t
        return q, 0
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[4 * i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = np.sqrt(((R[4 * i] - R[4 * j]) - R[4 * k]) + T(1))
    q[1 + i] = T(0.5) * t
    t = T(0.5) / t
    q[0] = (R[3 * k + j] - R[3 * j + k]) * t
    q[1 + j] = (R[3 * j + i] + R[3 * i + j]) * t
    q[1 + k] = (R[3 * k + i] + R[3 * i + k]) * t
    return q, 1 + i


def inv4(T, a):
    """Matrix4d::inverse() through the cofactors, row-major [16]."""
    s0, s1, s2 = a[0] * a[5] - a[4] * a[1], a[0] * a[6] - a[4] * a[2], a[0] * a[7] - a[4] * a[3]
    s3, s4, s5 = a[1] * a[6] - a[5] * a[2], a[1] * a[7] - a[5] * a[3], a[2] * a[7] - a[6] * a[3]
    c5, c4, c3 = a[10] * a[15] - a[14] * a[11], a[9] * a[15] - a[13] * a[11], a[9] * a[14] - a[13] * a[10]
    c2, c1, c0 = a[8] * a[15] - a[12] * a[11], a[8] * a[14] - a[12] * a[10], a[8] * a[13] - a[12] * a[9]
    with np.errstate(all="ignore"):
        d = T(1) / (s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0)
        return [(a[5] * c5 - a[6] * c4 + a[7] * c3) * d, (-a[1] * c5 + a[2] * c4 - a[3] * c3) * d,
                (a[13] * s5 - a[14] * s4 + a[15] * s3) * d, (-a[9] * s5 + a[10] * s4 - a[11] * s3) * d,
                (-a[4] * c5 + a[6] * c2 - a[7] * c1) * d, (a[0] * c5 - a[2] * c2 + a[3] * c1) * d,
                (-a[12] * s5 + a[14] * s2 - a[15] * s1) * d, (a[8] * s5 - a[10] * s2 + a[11] * s1) * d,
                (a[4] * c4 - a[5] * c2 + a[7] * c0) * d, (-a[0] * c4 + a[1] * c2 - a[3] * c0) * d,
                (a[12] * s4 - a[13] * s2 + a[15] * s0) * d, (-a[8] * s4 + a[9] * s2 - a[11] * s0) * d,
                (-a[4] * c3 + a[5] * c1 - a[6] * c0) * d, (a[0] * c3 - a[1] * c1 + a[2] * c0) * d,
                (-a[12] * s3 + a[13] * s1 - a[14] * s0) * d, (a[8] * s3 - a[9] * s1 + a[10] * s0) * d]


# ---- util.cpp ---------------------------------------------------------------------------------------------------------------------
def toOdometryPose(T, worldToCamera, imuToCamera, branches):                            # util.cpp:121-130
    with np.errstate(all="ignore"):
        imuToWorld = mm4(inv4(T, worldToCamera), imuToCamera)
        position = [imuToWorld[3], imuToWorld[7], imuToWorld[11]]
        Rt = [imuToWorld[0], imuToWorld[4], imuToWorld[8], imuToWorld[1], imuToWorld[5], imuToWorld[9], imuToWorld[2], imuToWorld[6], imuToWorld[10]]
        orientation, branch = rmat2quat(T, Rt)
    branches.append(branch)
    return position, orientation


# ---- backend.cpp ------------------------------------------------------------------------------------------------------------------
def slamPose(T, position, orientation, imuToCamera, slamToOdometry, branches):
    """backend.cpp:73-77 and the ready branch of computePose (:1374-1375): worldToCameraPoseOdometryToSlam is P -> P * slamToOdometry (:93-95)."""
    with np.errstate(all="ignore"):
        wToCOdo = toWorldToCamera(T, position, orientation, imuToCamera)
        wToCSlam = mm4(wToCOdo, slamToOdometry)
    return toOdometryPose(T, wToCSlam, imuToCamera, branches)


def convertOutputPose(T, position, orientation, imuToOutput, branches):                # api.cpp:726-742
    if [float(x) for x in imuToOutput] != IDENTITY:                                     # :730, the inverted test
        return list(position), list(orientation)
    with np.errstate(all="ignore"):
        worldToOutput = toWorldToCamera(T, position, orientation, imuToOutput)
    return toOdometryPose(T, worldToOutput, _vec(T, IDENTITY), branches)


# ---- ekf.cpp ----------------------------------------------------------------------------------------------------------------------
def changeMatrices(T, q0, q1):
    """ekf.cpp:715-733: qChange = conj(q0) * q1 (Eigen's quaternion product), qChangeMat and pChangeMat = toRotationMatrix()', row-major."""
    c0 = [q0[0], -q0[1], -q0[2], -q0[3]]
    p1 = c0[0] * q1[0] - c0[1] * q1[1] - c0[2] * q1[2] - c0[3] * q1[3]
    p2 = c0[0] * q1[1] + c0[1] * q1[0] + c0[2] * q1[3] - c0[3] * q1[2]
    p3 = c0[0] * q1[2] - c0[1] * q1[3] + c0[2] * q1[0] + c0[3] * q1[1]
    p4 = c0[0] * q1[3] + c0[1] * q1[2] - c0[2] * q1[1] + c0[3] * q1[0]
    qC = [p1, -p2, -p3, -p4, p2, p1, p4, -p3, p3, -p4, p1, p2, p4, p3, -p2, p1]
    w, x, y, z, two, one = p1, p2, p3, p4, T(2), T(1)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    pC = [one - (tyy + tzz), txy + twz, txz - twy, txy - twz, one - (txx + tzz), tyz + twx, txz + twy, tyz - twx, one - (txx + tyy)]
    return qC, pC


def _block(A, sz, P, s0, i, j):
    """Entry (i, j) of A P_bb A' for the sz x sz diagonal block at s0: A * (P * A')."""
    s = None
    for k in range(sz):
        tmp = P[s0 + k][s0] * A[sz * j]
        for l in range(1, sz):
            tmp = tmp + P[s0 + k][s0 + l] * A[sz * j + l]
        s = A[sz * i] * tmp if k == 0 else s + A[sz * i + k] * tmp
    return s


def transformTo(T, mean, P, pos, q):
    """ekf.cpp:704-757 on the inertial part: (mean', the diagonal of P', P'[POS block], P'[VEL block]); P indexed [row][column]."""
    qC, pC = changeMatrices(T, mean[ORI:ORI + 4], q)
    out = list(mean[:INER])
    for s0 in (POS, VEL):
        for r in range(3):
            out[s0 + r] = (pC[3 * r] * mean[s0] + pC[3 * r + 1] * mean[s0 + 1]) + pC[3 * r + 2] * mean[s0 + 2]
    for r in range(4):
        out[ORI + r] = ((qC[4 * r] * mean[ORI] + qC[4 * r + 1] * mean[ORI + 1]) + qC[4 * r + 2] * mean[ORI + 2]) + qC[4 * r + 3] * mean[ORI + 3]
    for r in range(3):                                                                  # :736, 757 and translateTo (:696-702)
        translation = pos[r] - out[POS + r]                                             # pChangeMat * refPos is the new position
        target = out[POS + r] + translation
        deltaX = target - out[POS + r]
        out[POS + r] = out[POS + r] + deltaX
    diag = [P[i][i] for i in range(INER)]
    cov = {}
    for s0 in (POS, VEL):
        cov[s0] = [_block(pC, 3, P, s0, i, j) for i in range(3) for j in range(3)]
        for i in range(3):
            diag[s0 + i] = cov[s0][4 * i]
    for i in range(4):
        diag[ORI + i] = _block(qC, 4, P, ORI, i, i)
    return out, diag, cov[POS], cov[VEL]


# ---- the visit loop's point cloud ---------------------------------------------------------------------------------------------------
def pointCloud(status, gate, n_cand, max_visual_updates, max_successful):
    """backend.cpp:1066-1251 with fullPointCloud off: [(candidate, PointFeature::Status)] in visit order. status [V][2] =
    (TriangulatorStatus, PrepareVuStatus), gate [V] = VuOutlierStatus as hv_ekf_visual_frame_ragged_dev writes them."""
    cloud, updateAttemptCount, updateSuccessCount = [], 0, 0
    for v in range(n_cand):
        if status[v][0] == TRI_NOT_VISITED:
            continue
        point_status = POINT_POSE_TRAIL                                                 # :1118
        updateAttemptCount += 1                                                         # :1121
        doVisualUpdate = status[v][1] == PREPARE_VU_OK and status[v][0] == TRI_OK       # :1152-1153
        if doVisualUpdate:
            if gate[v] == INLIER:
                updateSuccessCount += 1                                                 # :1188
            else:
                point_status = POINT_OUTLIER                                            # :1191
        limitSuccessful = max_successful > 0 and updateSuccessCount >= max_successful   # :1240
        limitTotal = max_visual_updates > 0 and updateAttemptCount >= max_visual_updates
        if limitSuccessful or limitTotal:
            break                                                                       # :1244, in front of the push
        if status[v][0] == TRI_OK:                                                      # :1249-1250
            cloud.append((v, point_status))
    return cloud


# ---- one set ------------------------------------------------------------------------------------------------------------------------
class Params:
    def __init__(self, trail, max_tracks=8, max_visual_updates=4, max_successful=5, stereo=True, imu_to_camera=None, imu_to_output=None):
        self.cameraTrailLength, self.maxTracks, self.maxVisualUpdates, self.maxSuccessfulVisualUpdates = trail, max_tracks, max_visual_updates, max_successful
        self.useStereo = stereo
        self.imuToCamera = list(IDENTITY) if imu_to_camera is None else [float(x) for x in np.asarray(imu_to_camera).reshape(16)]
        self.imuToOutput = list(IDENTITY) if imu_to_output is None else [float(x) for x in np.asarray(imu_to_output).reshape(16)]


def output(T, par, m, P, session, index, visit, slam):
    """The record of one set that is not frozen (a frozen set keeps its previous record, control.cpp:128), as a dict of lists by the
    member names of hv_output, plus "branches": the rmat2quat branch of every conversion, in a fixed order.
    m [n], P [n][n] (row, column); session: first_sample_t, time, tracking_status, stationary; index: n_keyframes, kf_row [K],
    timestamp [K], image_point [K][M][C][2], cand_col [V]; visit: cand_id [V], n_candidates, status [V][2], gate_status [V],
    pf [V][3]; slam: ready, slam_to_odometry [16], odometry_to_slam [16] (row-major; None: identity)."""
    K, V = par.cameraTrailLength + 1, par.maxVisualUpdates
    ready = bool(slam["ready"])
    given = ready and slam["slam_to_odometry"] is not None                              # until setCoordinates: the identity (:44-46)
    s2o = _vec(T, slam["slam_to_odometry"] if given else IDENTITY)
    o2s = _vec(T, slam["odometry_to_slam"] if given else IDENTITY)
    i2c, i2o = _vec(T, par.imuToCamera), _vec(T, par.imuToOutput)
    mean = _vec(T, m)
    Pm = [[T(P[i][j]) for j in range(INER)] for i in range(INER)]
    branches = []
    r = {}
    r["t"] = np.float64(session["first_sample_t"]) + np.float64(session["time"])        # control.cpp:118-119
    r["tracking_status"] = int(session["tracking_status"])                              # :122
    r["stationary_visual"] = int(bool(session["stationary"]))                           # backend.cpp:857
    # transformInertialState (:69-79), setFromEKF (output.cpp:56-62)
    pos, ori = slamPose(T, mean[POS:POS + 3], mean[ORI:ORI + 4], i2c, s2o, branches)
    with np.errstate(all="ignore"):
        r["inertial_mean"], r["inertial_cov_diag"], r["position_cov"], r["velocity_cov"] = transformTo(T, mean, Pm, pos, ori)
    # the pose trail (:844-855, 1368-1386)
    n_kf = min(max(int(index["n_keyframes"]), 1), K)
    r["n_trail"] = n_kf - 1
    r["trail_time"], r["trail_pose"], r["api_trail_pose"] = [], [], []
    for i in range(r["n_trail"]):
        r["trail_time"].append(np.float64(index["timestamp"][index["kf_row"][i + 1]]))
        if ready:
            ip = CAM + POSE_DIM * i
            p, q = slamPose(T, mean[ip:ip + 3], mean[ip + 3:ip + 7], i2c, s2o, branches)
        else:
            p, q = [T(0)] * 3, [T(0)] * 4
        r["trail_pose"].append(p + q)
        ap, aq = convertOutputPose(T, p, q, i2o, branches)                              # api.cpp:775-780
        r["api_trail_pose"].append(ap + aq)
    ap, aq = convertOutputPose(T, r["inertial_mean"][POS:POS + 3], r["inertial_mean"][ORI:ORI + 4], i2o, branches)   # :797
    r["api_pose"] = ap + aq
    # the point cloud (:255-280)
    r["point_id"], r["point_status"], r["point_first_pixel"], r["point_xyz"] = [], [], [], []
    if ready:
        n_cand = min(max(int(visit["n_candidates"]), 0), V)
        frame_row = index["kf_row"][1 % K]                                              # the frame's keyframe, keyframe 1 since the push
        for v, st in pointCloud(visit["status"], visit["gate_status"], n_cand, V, par.maxSuccessfulVisualUpdates):
            r["point_id"].append(int(visit["cand_id"][v]))
            r["point_status"].append(st)
            r["point_first_pixel"].append(np.asarray(index["image_point"][frame_row][index["cand_col"][v]][0], np.float32))   # track.points[0] (:1069)
            with np.errstate(all="ignore"):
                r["point_xyz"].append(transformVec3ByMat4(o2s, _vec(T, visit["pf"][v])))   # :278
    r["n_points"] = len(r["point_id"])
    r["branches"] = branches
    return r


# ---- the scripted corpus -------------------------------------------------------------------------------------------------------------
S, M, V = 5, 8, 4
FROZEN, NOT_READY, TRANSFORMED = 1, 3, (2, 4)
_C, _S = np.cos(0.3), np.sin(0.3)
IMU_TO_CAMERA = np.array([[0.0, -1.0, 0.0, 0.05], [-_C, 0.0, _S, -0.02], [-_S, 0.0, -_C, 0.01], [0.0, 0.0, 0.0, 1.0]])
IMU_TO_OUTPUT = np.array([[1.0, 0.0, 0.0, 0.1], [0.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, -0.2], [0.0, 0.0, 0.0, 1.0]])
# one orientation per rmat2quat branch: w, x, y, z dominant (the identity transforms leave them in that branch)
BRANCH_QUATS = [(0.9, 0.2, -0.3, 0.1), (0.15, 0.9, 0.25, -0.2), (-0.1, 0.3, 0.9, 0.2), (0.2, -0.15, 0.3, 0.9)]


def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def rigid(axis, angle, t):
    W = np.eye(4)
    W[:3, :3], W[:3, 3] = rotation(axis, angle), t
    return W


def slam_transforms():
    """Per set: ready, slamToOdometry, odometryToSlam (backend.cpp:59-63); sets 2 and 4 a rotation about a skew axis plus a
    translation of a few metres, the others the identity."""
    s2o, o2s = np.tile(np.eye(4).reshape(16), (S, 1)), np.tile(np.eye(4).reshape(16), (S, 1))
    for s, (axis, angle, t) in zip(TRANSFORMED, (((1.0, 2.0, -0.5), 0.7, (3.0, -2.0, 1.5)), ((-0.3, 0.4, 1.0), 2.1, (-4.0, 1.0, 2.5)))):
        odo, slam = rigid((0.2, -1.0, 0.4), 0.25, (0.5, 0.1, -0.3)), rigid(axis, angle, t)
        s2o[s] = (np.linalg.inv(odo) @ slam).reshape(16)
        o2s[s] = (np.linalg.inv(slam) @ odo).reshape(16)
    ready = np.ones(S, np.uint8)
    ready[NOT_READY] = 0
    return ready, s2o, o2s


# status rows of the point-cloud table: (triangulation, prepare, gate)
NOT_VISITED_ROW = (TRI_NOT_VISITED, TRI_NOT_VISITED, NOT_COMPUTED)
TRI_FAILED_ROW = (TRI_BEHIND, PREPARE_VU_OK, NOT_COMPUTED)
PREPARE_FAILED_ROW = (TRI_OK, PREPARE_VU_BEHIND, NOT_COMPUTED)
OUTLIER_ROW = (TRI_OK, PREPARE_VU_OK, CHI2)
INLIER_ROW = (TRI_OK, PREPARE_VU_OK, INLIER)


@functools.lru_cache(maxsize=None)
def case(trail, passthrough=False, max_successful=2):
    """The direct corpus of one trail length: S sets of scripted inputs in the device layouts, and the restatement in binary64 and
    in np.longdouble of every set that is not frozen."""
    rng = np.random.default_rng([trail, 2024])
    K, n = trail + 1, CAM + POSE_DIM * trail
    par = Params(trail, M, V, max_successful, True, IMU_TO_CAMERA, IMU_TO_OUTPUT if passthrough else None)
    means, covs = np.zeros((S, n)), np.zeros((S, n, n))
    for s in range(S):
        m = rng.normal(size=n)
        m[POS:POS + 3] = rng.uniform(-3, 3, 3)
        for c in range(-1, trail):
            ip, io = (POS, ORI) if c < 0 else (CAM + POSE_DIM * c, CAM + POSE_DIM * c + 3)
            q = np.array(BRANCH_QUATS[(s + c + 1) % 4]) + 0.03 * rng.normal(size=4)
            m[io:io + 4] = q / np.linalg.norm(q)
            if c >= 0:
                m[ip:ip + 3] = m[POS:POS + 3] + 0.2 * (c + 1) * rng.normal(size=3)
        A = rng.normal(size=(n, n))
        means[s], covs[s] = m, 1e-2 * (A @ A.T / n + 0.1 * np.eye(n))
    ready, s2o, o2s = slam_transforms()
    n_kf = np.array([K, min(3, K), 2, K, 1], np.int32)                                   # full, partial, one historical pose, none
    if trail > 3:
        n_kf[0], n_kf[3] = K, K - 2
    index = dict(n_keyframes=n_kf, kf_row=np.stack([rng.permutation(K) for _ in range(S)]).astype(np.int32),
                 timestamp=rng.uniform(1, 100, (S, K)), image_point=rng.uniform(0, 700, (S, K, M, 2, 2)).astype(np.float32),
                 cand_col=np.stack([rng.permutation(M)[:V] for _ in range(S)]).astype(np.int32))
    rows = [[INLIER_ROW, OUTLIER_ROW, PREPARE_FAILED_ROW, TRI_FAILED_ROW],             # attempts reach V at the last: it is left out anyway
            [INLIER_ROW, INLIER_ROW, INLIER_ROW, INLIER_ROW],                           # frozen
            [OUTLIER_ROW, INLIER_ROW, INLIER_ROW, INLIER_ROW],                          # the second success stops the loop: v = 2 left out
            [INLIER_ROW, OUTLIER_ROW, NOT_VISITED_ROW, NOT_VISITED_ROW],                # not ready: no cloud
            [PREPARE_FAILED_ROW, NOT_VISITED_ROW, INLIER_ROW, NOT_VISITED_ROW]]         # no stop; a gap in the visits
    n_cand = np.array([4, 4, 4, 2, 3], np.int32)
    status = np.zeros((V, S, 2), np.int32)
    gate = np.zeros((V, S), np.int32)
    for s in range(S):
        for v in range(V):
            status[v, s], gate[v, s] = rows[s][v][:2], rows[s][v][2]
    visit = dict(cand_id=rng.integers(1, 10 ** 6, (V, S)).astype(np.int32), n_candidates=n_cand, status=status, gate_status=gate,
                 pf=rng.uniform(-8, 8, (V, S, 3)))
    session = dict(first_sample_t=rng.uniform(1e3, 2e3, S), time=rng.uniform(0, 50, S), tracking_status=np.array([1, 2, 1, 0, 1], np.int32),
                   stationary=np.array([0, 1, 1, 0, 1], np.uint8))
    frozen = np.zeros(S, np.uint8)
    frozen[FROZEN] = 1
    c = dict(trail=trail, K=K, n=n, par=par, means=means, covs=covs, ready=ready, s2o=s2o, o2s=o2s, frozen=frozen, index=index, visit=visit,
             session=session)
    c["rest"], c["truth"] = restate_all(np.float64, c), restate_all(LD, c)
    return c


def set_inputs(c, s, means=None, covs=None):
    """The arguments of output() for set s of a case's arrays."""
    ix, vi, se = c["index"], c["visit"], c["session"]
    index = dict(n_keyframes=ix["n_keyframes"][s], kf_row=ix["kf_row"][s], timestamp=ix["timestamp"][s], image_point=ix["image_point"][s],
                 cand_col=ix["cand_col"][s])
    visit = dict(cand_id=vi["cand_id"][:, s], n_candidates=vi["n_candidates"][s], status=vi["status"][:, s], gate_status=vi["gate_status"][:, s],
                 pf=vi["pf"][:, s])
    session = {k: v[s] for k, v in se.items()}
    slam = dict(ready=c["ready"][s], slam_to_odometry=c["s2o"][s], odometry_to_slam=c["o2s"][s])
    return ((c["means"] if means is None else means)[s], (c["covs"] if covs is None else covs)[s], session, index, visit, slam)


def restate_all(T, c, means=None, covs=None):
    return [None if c["frozen"][s] else output(T, c["par"], *set_inputs(c, s, means, covs)) for s in range(S)]
