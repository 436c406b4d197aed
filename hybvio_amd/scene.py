"""A stereo + IMU scene with ground truth for the resident VIO engine (numpy only; the renderer is synth.render).

Geometry. A fronto-parallel textured plane at depth Z0 in front of a pinhole stereo rig without distortion. In the SCENE frame
the optical axis is +z and the plane is z = Z0; the rig translates in x, y and z and rolls about its optical axis by theta, so
the camera-to-scene rotation is Rz(theta). A plane point X projects to pixel pp + f Rz(theta)' (X_xy - c_xy) / d with
d = Z0 - c_z, which inverted is X_xy = c_xy + (d / f) Rz(theta) (pixel - pp): an affine map of the pixel. With s texture pixels
per metre the frame is synth.render under

    Warp(A = s (d / f) Rz(theta),  t = s (c_xy - (d / f) Rz(theta) pp)),

exactly, for the left camera at c and for the right one at c + Rz(theta) (b, 0, 0).

World and IMU. The filter's world has z up and gravity (0, 0, -g) (oracle/ekf_oracle.c:183); the rig looks DOWN at the plane, so
the roll axis is the gravity axis: world = RWS scene with RWS = diag(1, -1, -1), a half turn about x. The IMU sits at the left
camera's centre (no lever arm) with IMU_TO_CAMERA = diag(1, -1, -1): at theta = 0 the IMU axes are the world axes.
The filter's orientation q is world-to-IMU: the oracle's predict forms vel += (R(q)' (acc - bias) + gravity) dt and
q <- exp(-dt / 2 Omega(gyro)) q (oracle/ekf_oracle.c:347-371), so the samples are

    acc  = R_wi' (p_world'' + (0, 0, g))         specific force in the IMU frame, R_wi = RWS Rz(theta) IMU_TO_CAMERA (IMU to world)
    gyro = (0, 0, -theta')                       R_wi = Rz_world(-theta): the body rate of a turn about the common z axis

and the true state of a frame is pos = RWS c, vel = RWS c', q = quaternion of R_wi'.

Trajectory. Per axis i (x, y, z, roll): ramp(tau) A_i (1 - cos(w_i tau)), tau = t - t_rest, zero for tau <= 0: the rig is at
rest for `rest_frames` frames. ramp is the C3 smooth step s^4 (35 - 84 s + 70 s^2 - 20 s^3) over `ramp_seconds`, so position,
velocity, acceleration, jerk and snap are continuous everywhere and all start at zero. derivatives() returns them analytically.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import synth

RWS = np.diag([1.0, -1.0, -1.0])                 # scene -> world
IMU_TO_CAMERA = np.diag([1.0, -1.0, -1.0, 1.0])  # 4 x 4 homogeneous, row-major like Parameters::imuToCamera


def rot2(theta: float) -> np.ndarray:
    c, s = math.cos(theta), math.sin(theta)
    return np.array([[c, -s], [s, c]])


def rotz(theta: float) -> np.ndarray:
    R = np.eye(3)
    R[:2, :2] = rot2(theta)
    return R


def rmat2quat(R: np.ndarray) -> np.ndarray:
    """(w, x, y, z) of a rotation matrix, w >= 0 (Shepperd's branches)."""
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    return q if q[0] >= 0 else -q


_RAMP = np.polynomial.Polynomial([0, 0, 0, 0, 35.0, -84.0, 70.0, -20.0])


@dataclasses.dataclass
class Trajectory:
    """amp / omega: (x, y, z, roll) amplitudes (m, m, m, rad) and angular frequencies (rad/s)."""
    amp: tuple
    omega: tuple
    t_rest: float = 0.5
    ramp_seconds: float = 1.0

    def derivatives(self, t, order: int = 4) -> np.ndarray:
        """[order + 1][len(t)][4]: the four coordinates and their first `order` time derivatives at the times t (Leibniz rule on
        ramp * A (1 - cos))."""
        tau = np.atleast_1d(np.asarray(t, np.float64)) - self.t_rest
        s = np.clip(tau / self.ramp_seconds, 0.0, 1.0)
        r = [_RAMP.deriv(k)(s) / self.ramp_seconds ** k if k else _RAMP(s) for k in range(order + 1)]
        for k in range(1, order + 1):
            r[k] = np.where((tau > 0) & (tau < self.ramp_seconds), r[k], 0.0)
        out = np.zeros((order + 1, tau.size, 4))
        for i, (A, w) in enumerate(zip(self.amp, self.omega)):
            ph = w * np.maximum(tau, 0.0)
            g = [A * (1 - np.cos(ph)), A * w * np.sin(ph), A * w ** 2 * np.cos(ph), -A * w ** 3 * np.sin(ph), -A * w ** 4 * np.cos(ph),
                 A * w ** 5 * np.sin(ph), A * w ** 6 * np.cos(ph)]
            for n in range(order + 1):
                out[n, :, i] = sum(math.comb(n, k) * r[k] * g[n - k] for k in range(n + 1))
        out[:, tau <= 0, :] = 0.0
        return out


@dataclasses.dataclass
class Rig:
    width: int = 376
    height: int = 240
    focal: float = 230.0
    Z0: float = 2.5
    baseline: float = 0.1
    tex_per_metre: float = 120.0       # texture pixels per metre on the plane

    @property
    def pp(self) -> np.ndarray:
        return np.array([0.5 * (self.width - 1), 0.5 * (self.height - 1)])

    def second_imu_to_camera(self) -> np.ndarray:
        """x_cam1 = x_cam0 - (b, 0, 0): the right camera sits at +b along the left camera's x axis."""
        T = IMU_TO_CAMERA.copy()
        T[0, 3] = -self.baseline
        return T


def camera_centres(rig: Rig, c: np.ndarray, theta: float):
    """Left and right camera centres in the scene frame."""
    right = np.array(c, np.float64)
    right[:2] += rot2(theta) @ np.array([rig.baseline, 0.0])
    return np.asarray(c, np.float64), right


def warp_of(rig: Rig, centre: np.ndarray, theta: float) -> synth.Warp:
    """The affine map pixel -> texture coordinate of a camera at `centre` (scene frame) with roll theta."""
    d = rig.Z0 - centre[2]
    A = rig.tex_per_metre * (d / rig.focal) * rot2(theta)
    return synth.Warp(A, rig.tex_per_metre * centre[:2] - A @ rig.pp)


def project(rig: Rig, centre: np.ndarray, theta: float, X: np.ndarray) -> np.ndarray:
    """Pinhole projection of scene points X [n][3] from a camera at `centre` with roll theta (camera-to-scene rotation Rz(theta))."""
    pc = (X - centre) @ rotz(theta)              # rows: Rz(theta)' (X - c)
    return rig.pp + rig.focal * pc[:, :2] / pc[:, 2:3]


@dataclasses.dataclass
class Scene:
    rig: Rig
    traj: Trajectory
    frame_t: np.ndarray          # [F]
    left: np.ndarray             # [F][H][W] u8
    right: np.ndarray
    warps: list                  # [F] (left Warp, right Warp)
    centre: np.ndarray           # [F][3] left camera centre, scene frame
    theta: np.ndarray            # [F]
    pos: np.ndarray              # [F][3] world position of the IMU (= left camera centre)
    vel: np.ndarray              # [F][3]
    quat: np.ndarray             # [F][4] world-to-IMU (the filter's orientation), w first
    imu_t: np.ndarray            # [N]
    gyro: np.ndarray             # [N][3]
    acc: np.ndarray              # [N][3]
    gravity: float

    def samples_of_frame(self, f: int, per_frame: int):
        """The IMU samples in front of frame f: indices f * per_frame .. (f + 1) * per_frame - 1 (sample times up to the frame time)."""
        sl = slice(f * per_frame, (f + 1) * per_frame)
        return self.imu_t[sl], self.gyro[sl], self.acc[sl]


def true_state(traj: Trajectory, t):
    """World position, velocity, acceleration [n][3], roll and its rate [n], world-to-IMU quaternion [n][4] at the times t."""
    d = traj.derivatives(t, 2)
    pos, vel, acc = d[0, :, :3] @ RWS.T, d[1, :, :3] @ RWS.T, d[2, :, :3] @ RWS.T
    theta, rate = d[0, :, 3], d[1, :, 3]
    R_ic = IMU_TO_CAMERA[:3, :3]
    quat = np.stack([rmat2quat((RWS @ rotz(th) @ R_ic).T) for th in theta])
    return pos, vel, acc, theta, rate, quat


def imu(traj: Trajectory, t, gravity: float = 9.819, noise_seed=None, noise_acc: float = 0.0, noise_gyro: float = 0.0, acc_bias=(0.0, 0.0, 0.0)):
    """gyro, acc [n][3] at the sample times t: specific force and body rate in the IMU frame, plus seeded white noise of the given
    standard deviations per sample and a constant accelerometer bias."""
    _, _, a_w, theta, rate, _ = true_state(traj, t)
    R_ic = IMU_TO_CAMERA[:3, :3]
    acc = np.stack([(RWS @ rotz(th) @ R_ic).T @ (a + np.array([0.0, 0.0, gravity])) for th, a in zip(theta, a_w)])
    gyro = np.stack([np.zeros_like(rate), np.zeros_like(rate), -rate], 1)
    if noise_seed is not None:
        rng = np.random.default_rng(noise_seed)
        acc = acc + rng.normal(0.0, noise_acc, acc.shape)
        gyro = gyro + rng.normal(0.0, noise_gyro, gyro.shape)
    return gyro, acc + np.asarray(acc_bias, np.float64)


def make(seed: int, traj: Trajectory, n_frames: int, rig: Rig | None = None, fps: float = 20.0, imu_rate: float = 200.0,
         gravity: float = 9.819, noise_seed=None, noise_acc: float = 0.0, noise_gyro: float = 0.0, acc_bias=(0.0, 0.0, 0.0),
         image_noise: float = 1.0, render: bool = True) -> Scene:
    """Frame f is taken at t = (f + 1) / fps; the IMU samples are at (k + 1) / imu_rate, so a frame is preceded by imu_rate / fps
    samples, the last of them at the frame time. The right image carries independent N(0, image_noise^2) pixel noise."""
    rig = rig or Rig()
    per = int(round(imu_rate / fps))
    frame_t = (1 + np.arange(n_frames)) / fps
    imu_t = (1 + np.arange(n_frames * per)) / imu_rate
    d = traj.derivatives(frame_t, 0)[0]
    centre, theta = d[:, :3], d[:, 3]
    pos, vel, _, _, _, quat = true_state(traj, frame_t)
    tex = synth.Texture.make(seed)
    H, W = rig.height, rig.width
    left, right = np.zeros((n_frames, H, W), np.uint8), np.zeros((n_frames, H, W), np.uint8)
    warps = []
    for f in range(n_frames):
        cl, cr = camera_centres(rig, centre[f], theta[f])
        wl, wr = warp_of(rig, cl, theta[f]), warp_of(rig, cr, theta[f])
        warps.append((wl, wr))
        if render:
            left[f] = synth.render(tex, W, H, wl)
            right[f] = synth.render(tex, W, H, wr, noise_seed=seed * 1000 + f, noise_sigma=image_noise)
    gyro, acc = imu(traj, imu_t, gravity, noise_seed, noise_acc, noise_gyro, acc_bias)
    return Scene(rig, traj, frame_t, left, right, warps, centre, theta, pos, vel, quat, imu_t, gyro, acc, gravity)
