"""CPU checks of the ground-truth scene (hybvio_amd/scene.py): the stated affine warp is the pinhole projection, and the IMU
samples are consistent with the true trajectory under the oracle's predict (oracle/ekf_oracle.c), whose conventions they follow."""
import numpy as np

from hybvio_amd import scene

POS, VEL, ORI = 0, 3, 6
TRAJ = [scene.Trajectory(amp=(0.12, 0.08, 0.05, 0.10), omega=(1.9, 2.3, 1.3, 1.1)),
        scene.Trajectory(amp=(0.07, 0.13, 0.06, 0.15), omega=(2.4, 1.6, 1.7, 0.9))]


def test_the_stated_warp_is_the_pinhole_projection():
    """200 random plane points per frame and camera: the pixel under Warp equals the projection of the 3-D point from the true
    pose to 1e-9 px, at frames over the whole trajectory (translation in x, y, z and roll all non-zero)."""
    rig = scene.Rig()
    rng = np.random.default_rng(5)
    for traj in TRAJ:
        sc = scene.make(3, traj, 80, rig, render=False)
        for f in (0, 17, 40, 79):
            X = np.concatenate([rng.uniform(-1.5, 1.5, (200, 2)), np.full((200, 1), rig.Z0)], 1)
            for cam, centre in enumerate(scene.camera_centres(rig, sc.centre[f], sc.theta[f])):
                want = scene.project(rig, centre, sc.theta[f], X)
                got = sc.warps[f][cam].invert(rig.tex_per_metre * X[:, :2])
                assert np.abs(got - want).max() < 1e-9, (f, cam)
        assert np.abs(sc.theta).max() > 0.05 and np.ptp(sc.centre, 0).min() > 0.05         # the motion is there
        assert np.allclose(sc.centre[:10], 0) and np.allclose(sc.theta[:10], 0)              # at rest for ten frames
        # the right camera is the baseline away, along the rolled x axis
        cl, cr = scene.camera_centres(rig, sc.centre[40], sc.theta[40])
        assert abs(np.linalg.norm(cr - cl) - rig.baseline) < 1e-15


def test_derivatives_are_consistent():
    """The analytic derivatives against central differences of the order below (the bound of the next test is built on them)."""
    t = np.linspace(0.0, 4.0, 801)
    h = 1e-4
    for traj in TRAJ:
        # (not across the two ends of the ramp: the snap jumps where the C3 step ends, and a central difference straddles it)
        t = t[(np.abs(t - traj.t_rest) > 2 * h) & (np.abs(t - traj.t_rest - traj.ramp_seconds) > 2 * h)]
        d = traj.derivatives(t, 4)
        for n in range(4):
            num = (traj.derivatives(t + h, n)[n] - traj.derivatives(t - h, n)[n]) / (2 * h)
            assert np.abs(num - d[n + 1]).max() < 1e-5 * max(1.0, np.abs(d[n + 1]).max()), n
        assert np.all(d[:, t <= traj.t_rest] == 0.0)


def test_imu_samples_reproduce_the_true_positions_under_the_oracle_predict(oracle):
    """The noise-free samples through orc_ekf_predict alone, from the true initial state. The bound is derived, not tuned:

    The oracle's sample step is pos += vel h, then vel += (R(q)' acc + g) h with the NEW orientation (ekf_oracle.c:365-371), so
    after n steps pos_n - pos_0 = h^2 sum_{m < n} (n - m) a_m: the right Riemann sum of G(u) = (T - u) a(u) over [0, T], T = n h.
    G(0) = G(T) = 0 (the rig starts at rest), so it is also the trapezoid sum, whose error is at most T h^2 / 12 max|G''| with
    G'' = (T - u) a'' - 2 a':   E_int <= T h^2 / 12 (T max|snap| + 2 max|jerk|).
    The orientation is integrated from the gyro by a right Riemann sum as well (the quaternion exponential is exact for the fixed
    roll axis): |dtheta| <= h T max|theta''| / 2. Gravity lies on the roll axis, so only the horizontal acceleration is turned by
    dtheta, |a_err| <= max|a_h| |dtheta|, which the double sum carries into   E_rot <= T^2 / 2 max|a_h| h T max|theta''| / 2."""
    h, fps, frames = 1.0 / 200, 20.0, 80
    for traj in TRAJ:
        sc = scene.make(3, traj, frames, fps=fps, imu_rate=1.0 / h, render=False)
        e = oracle.Ekf(oracle.ekf_default_params(cameraTrailLength=3, hybridMapSize=0))
        m = e.m.copy()
        p0, v0, _, _, _, q0 = scene.true_state(traj, sc.imu_t[:1])
        m[POS:POS + 3], m[VEL:VEL + 3], m[ORI:ORI + 4] = p0[0], v0[0], q0[0]
        e.set_state(m)
        per = int(round(1.0 / (h * fps)))
        err = np.zeros(frames)
        for f in range(frames):
            for t, g, a in zip(*sc.samples_of_frame(f, per)):
                e.predict(float(t), g, a)
            err[f] = np.linalg.norm(e.m[POS:POS + 3] - sc.pos[f])
            assert abs(sc.imu_t[(f + 1) * per - 1] - sc.frame_t[f]) < 1e-12
        T = sc.imu_t[-1] - sc.imu_t[0]
        d = traj.derivatives(np.linspace(0.0, sc.imu_t[-1], 16001), 4)
        jerk, snap = np.linalg.norm(d[3, :, :3], axis=1).max(), np.linalg.norm(d[4, :, :3], axis=1).max()
        a_h, th2 = np.linalg.norm(d[2, :, :2], axis=1).max(), np.abs(d[2, :, 3]).max()
        bound = T * h * h / 12 * (T * snap + 2 * jerk) + 0.5 * T * T * a_h * (0.5 * h * T * th2)
        print(f"dead-reckoning error of the noise-free samples: {err.max():.3e} m, bound {bound:.3e} m, path {np.abs(np.diff(sc.pos, axis=0)).sum():.2f} m")
        assert err.max() < bound
        assert bound < 0.05                                       # (the bound itself is small against the 1 m path)
        # and the final orientation and velocity are the true ones to the same order
        assert np.abs(e.m[ORI:ORI + 4] - sc.quat[-1]).max() < h * T * th2
