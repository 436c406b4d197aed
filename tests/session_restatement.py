"""Literal restatement of the session lifecycle of the reference, one sequence at a time, in numpy scalars:

- the ring size and trackingStatus (src/odometry/backend.cpp:195-198, 807-819) with CircularBuffer (src/odometry/util.hpp:111-149),
- initializeOrientation on the first IMU sample (backend.cpp:728-731; ekf.cpp:299-317 through oracle/ekf_oracle.c:285-311) with the
  zero-vector rule: Eigen's normalized() leaves a zero vector zero, FromTwoVectors then returns (sqrt(2) / 2, 0, 0, 0),
- the filter's sample clock (ekf.cpp:357-366),
- Control's status, freeze flag and reset rules (src/odometry/control.cpp:117-149) and reset() (control.cpp:49-65) with
  initializeAtPose (backend.cpp:224-229).

It is what the device entries hv_session_*_dev (csrc/session.hip) are compared with, array for array. The module needs numpy only; the
keep-pose filter is built from the CPU oracle (oracle/orc.py), which is passed in by the caller.
"""
import dataclasses

import numpy as np

INIT, TRACKING, LOST_TRACKING = 0, 1, 2                  # api::TrackingStatus (src/api/types.hpp:34-38)
RESET_NONE, RESET_FRESH, RESET_KEEP_POSE = 0, 1, 2       # none, reset(false), reset(true)
POS, VEL, ORI, BGA, BAA, BAT, SFT, CAM, POSE_DIM = 0, 3, 6, 10, 13, 16, 19, 20, 7
f32, f64 = np.float32, np.float64


@dataclasses.dataclass
class Params:
    """codegen/parameter_definitions.c:4, 193-204, 220"""
    targetFps: float = 30.0
    visualUpdateForEveryNFrame: int = 1
    goodFramesTimeWindowSeconds: float = 2.0
    goodFramesToTracking: float = 0.75
    goodFramesToTrackingFailed: float = 0.05
    resetUntilInitSucceeds: int = 0
    resetOnFailedTracking: int = 0
    resetAfterTrackingFailsToInitialize: float = 3.0
    freezeOnFailedTracking: int = 0


def window(p) -> int:
    """backend.cpp:195-197: (size_t)((double)targetFps / (double)visualUpdateForEveryNFrame * goodFramesTimeWindowSeconds)"""
    return int(f64(p.targetFps) / f64(p.visualUpdateForEveryNFrame) * f64(p.goodFramesTimeWindowSeconds))


class CircularBuffer:
    """util.hpp:111-149 with T = float"""

    def __init__(self, size):
        self.buffer = np.zeros(size, f32)
        self.size, self.head, self.entries = size, 0, 0

    def put(self, value):
        self.buffer[self.head] = f32(value)
        self.head = (self.head + 1) % self.size
        if self.entries != self.size:
            self.entries += 1

    def mean(self):
        if self.entries == 0:
            return f32(0)
        total = f32(0)
        for i in range(self.entries):
            total = f32(total + self.buffer[i])
        return f32(total / f32(self.entries))


def initialize_orientation(gravity, xa):
    """FromTwoVectors(-gravity, xa), gravity = (0, 0, -g), as oracle/ekf_oracle.c:285-306, plus the zero-vector rule."""
    a = np.array([-0.0, -0.0, gravity], f64)
    b = np.array(xa, f64)
    na, nb = np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), np.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
    a = a / na
    if nb > 0.0:                                         # Eigen >= 3.3 normalized(): a zero vector stays zero
        b = b / nb
    c = a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    q = np.zeros(4, f64)
    if c < -1.0 + 1e-12:
        ax = np.array([1.0, 0.0, 0.0])
        if abs(a[0]) > 0.9:
            ax = np.array([0.0, 1.0, 0.0])
        d = ax[0] * a[0] + ax[1] * a[1] + ax[2] * a[2]
        ax = ax - d * a
        nn = np.sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2])
        q[0] = 0.0
        q[1:] = ax / nn
    else:
        ax = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        s = np.sqrt((1.0 + c) * 2.0)
        invs = 1.0 / s
        q[0] = s * 0.5
        q[1:] = ax * invs
    return q


def orientation_block(ekf_params):
    """ekf.cpp:311-316: diag(1, 1, 1, 0) * noiseInitialOri^2 * noiseScale^2"""
    v = (ekf_params.noiseInitialOri * ekf_params.noiseInitialOri) * (ekf_params.noiseScale * ekf_params.noiseScale)
    return np.diag([v, v, v, 0.0])


class Clock:
    """The clock members of odometry::EKF (ekf.cpp:357-366)."""

    def __init__(self):
        self.first_sample, self.first_sample_t, self.prev_sample_t, self.time = True, f64(-1.0), f64(-1.0), f64(0.0)

    def sample(self, t):
        t = f64(t)
        dt = f64(0.0)
        if not self.first_sample:
            dt = t - self.prev_sample_t
            self.time = t - self.first_sample_t
        else:
            self.first_sample_t = t
            self.first_sample = False
        self.prev_sample_t = t
        return dt

    def platform_time(self):
        return self.first_sample_t + self.time


class Session:
    """What the lifecycle reads of Session: the ring, trackingStatus, initializedOrientation and the filter's clock."""

    def __init__(self, p):
        self.counter = CircularBuffer(window(p))
        self.tracking_status = INIT
        self.initialized_orientation = False
        self.clock = Clock()

    def imu(self, t, acc, gravity):
        """backend.cpp:728-734 up to the predict: returns (q or None, dt)."""
        q = None
        if not self.initialized_orientation:
            q = initialize_orientation(gravity, acc)
            self.initialized_orientation = True
        return q, self.clock.sample(t)

    def frame(self, p, good_frame, full_update=True):
        """backend.cpp:807-819"""
        if full_update:
            self.counter.put(1.0 if good_frame else 0.0)
            if self.counter.entries > self.counter.size // 2:
                mean = f64(self.counter.mean())
                if self.tracking_status != TRACKING and mean > p.goodFramesToTracking:
                    self.tracking_status = TRACKING
                elif self.tracking_status == TRACKING and mean < p.goodFramesToTrackingFailed:
                    self.tracking_status = LOST_TRACKING


class Control:
    """control.cpp:40-65, 117-149"""

    def __init__(self, p):
        self.p = p
        self.control_status = INIT
        self.last_reset_time = f64(0.0)
        self.session = Session(p)

    def frame(self, good_frame, full_update=True):
        """One processed frame: returns (output.trackingStatus, frozen, reset kind). The reset is decided, not performed."""
        p, s = self.p, self.session
        s.frame(p, good_frame, full_update)
        t = s.clock.platform_time()
        status = self.control_status
        frozen = bool(p.freezeOnFailedTracking) and self.control_status != INIT and s.tracking_status != TRACKING
        if self.control_status == INIT or s.tracking_status != INIT:
            self.control_status = s.tracking_status
        expired = self.last_reset_time + f64(p.resetAfterTrackingFailsToInitialize) < t
        kind = RESET_NONE
        if self.control_status == INIT and expired and p.resetUntilInitSucceeds:
            kind = RESET_FRESH
        elif p.resetOnFailedTracking and s.tracking_status == LOST_TRACKING:
            kind = RESET_KEEP_POSE
        elif self.control_status != INIT and s.tracking_status == INIT and expired:
            kind = RESET_KEEP_POSE
        return status, frozen, kind

    def reset(self, keep_pose):
        """control.cpp:49-65 without the filter (reset_filter below)."""
        self.last_reset_time = self.session.clock.platform_time()
        self.session = Session(self.p)
        if keep_pose:
            self.session.initialized_orientation = True       # initializeAtPose, backend.cpp:227


def reset_filter(orc, ekf_params, keep_pose, pos=None, q=None):
    """The filter of a new Session: a fresh oracle Ekf; with keep_pose, initializeAtPose(pos, q) (backend.cpp:224-229):
    initializeOrientation(0) set by hand under the zero-vector rule (the oracle divides by zero there), then transform_to."""
    e = orc.Ekf(ekf_params)
    if keep_pose:
        e.m[ORI:ORI + 4] = initialize_orientation(ekf_params.gravity, np.zeros(3))
        e.P[ORI:ORI + 4, ORI:ORI + 4] = orientation_block(ekf_params)
        e.transform_to(np.asarray(pos, f64), np.asarray(q, f64))
    return e


def transform_blockwise(m, P, trail, pos, q):
    """transformTo(pos, q) (ekf.cpp:704-758) on a filter whose P is block diagonal, formed per diagonal block of
    A = diag(pC, pC, qC, I_10, {pC, qC} x trail): what the device reset does. Returns (m, P)."""
    m, P = np.array(m, f64), np.array(P, f64)
    q0 = m[ORI:ORI + 4]
    a = np.array([q0[0], -q0[1], -q0[2], -q0[3]])
    p1 = a[0] * q[0] - a[1] * q[1] - a[2] * q[2] - a[3] * q[3]
    p2 = a[0] * q[1] + a[1] * q[0] + a[2] * q[3] - a[3] * q[2]
    p3 = a[0] * q[2] - a[1] * q[3] + a[2] * q[0] + a[3] * q[1]
    p4 = a[0] * q[3] + a[1] * q[2] - a[2] * q[1] + a[3] * q[0]
    qC = np.array([[p1, -p2, -p3, -p4], [p2, p1, p4, -p3], [p3, -p4, p1, p2], [p4, p3, -p2, p1]])
    w, x, y, z = p1, p2, p3, p4
    R = np.array([[1 - (2 * y * y + 2 * z * z), 2 * y * x - 2 * z * w, 2 * z * x + 2 * y * w],
                  [2 * y * x + 2 * z * w, 1 - (2 * x * x + 2 * z * z), 2 * z * y - 2 * x * w],
                  [2 * z * x - 2 * y * w, 2 * z * y + 2 * x * w, 1 - (2 * x * x + 2 * y * y)]])
    pC = R.T
    translation = np.asarray(pos, f64) - pC @ m[POS:POS + 3]
    blocks = [(POS, pC), (VEL, pC), (ORI, qC)]
    for c in range(trail):
        blocks += [(CAM + POSE_DIM * c, pC), (CAM + POSE_DIM * c + 3, qC)]
    for s, A in blocks:
        k = len(A)
        m[s:s + k] = A @ m[s:s + k]
        P[s:s + k, s:s + k] = A @ (P[s:s + k, s:s + k] @ A.T)
    target = m[POS:POS + 3] + translation
    d = target - m[POS:POS + 3]
    m[POS:POS + 3] += d
    for c in range(trail):
        m[CAM + POSE_DIM * c:CAM + POSE_DIM * c + 3] += d
    return m, P
