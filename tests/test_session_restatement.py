"""Pins of tests/session_restatement.py, the literal restatement the device session entries are compared with (no GPU needed)."""
import math

import numpy as np
import pytest

import session_restatement as R


def drive(ctl, flags, t0=0.0, dt=0.5):
    """Frames at t0, t0 + dt, ...: one IMU sample in front of each; returns the (status, frozen, kind) of every frame."""
    out = []
    for i, g in enumerate(flags):
        ctl.session.imu(t0 + dt * i, (0.0, 0.0, 9.8), 9.819)
        out.append(ctl.frame(bool(g)))
    return out


def test_window_is_60_for_the_defaults_and_truncates():
    assert R.window(R.Params()) == 60
    assert R.window(R.Params(targetFps=2.0)) == 4
    assert R.window(R.Params(targetFps=30.0, visualUpdateForEveryNFrame=4)) == 15
    assert R.window(R.Params(targetFps=2.9, goodFramesTimeWindowSeconds=1.0)) == 2


def test_the_mean_is_only_consulted_above_half_a_window():
    p = R.Params(targetFps=2.0)                                # W = 4: consulted from the third entry on
    s = R.Session(p)
    s.frame(p, True); s.frame(p, True)
    assert s.counter.entries == 2 and s.tracking_status == R.INIT            # entries == W / 2: not yet
    s.frame(p, True)
    assert s.counter.entries == 3 and s.tracking_status == R.TRACKING
    s2 = R.Session(p)
    s2.frame(p, True, full_update=False)
    assert s2.counter.entries == 0                                            # no put on a frame that is not a full update
    odd = R.Params(targetFps=2.5)                                            # W = 5, W / 2 = 2
    s3 = R.Session(odd)
    for _ in range(3):
        s3.frame(odd, True)
    assert s3.tracking_status == R.TRACKING and s3.counter.entries == 3


def test_circular_buffer_mean_runs_over_the_buffer_front_and_wraps():
    b = R.CircularBuffer(4)
    for v in (1, 0, 1, 1, 0):                                  # the fifth put overwrites slot 0
        b.put(v)
    assert b.head == 1 and b.entries == 4 and b.buffer.tolist() == [0, 0, 1, 1]
    assert b.mean() == np.float32(0.5) and b.mean().dtype == np.float32
    c = R.CircularBuffer(60)
    for _ in range(31):
        c.put(1.0)
    assert c.mean() == np.float32(1.0)


def test_scripted_sequence_init_tracking_lost():
    p = R.Params(targetFps=2.0)
    ctl = R.Control(p)
    out = drive(ctl, [1, 1, 1, 1, 0, 0, 0, 0])
    # frame 2 (third): mean 1 > 0.75 -> TRACKING; frames 4..6: means 0.75, 0.5, 0.25; frame 7: mean 0 < 0.05 -> LOST
    tracking = [R.INIT, R.INIT, R.TRACKING, R.TRACKING, R.TRACKING, R.TRACKING, R.TRACKING, R.LOST_TRACKING]
    assert ctl.session.tracking_status == R.LOST_TRACKING and ctl.control_status == R.LOST_TRACKING
    # output.trackingStatus is the control status BEFORE the frame's update: one frame behind
    assert [o[0] for o in out] == [R.INIT] + tracking[:-1]
    assert all(o[1] is False and o[2] == R.RESET_NONE for o in out)          # the defaults never freeze or reset


def test_none_of_the_reset_rules_fires_with_default_parameters():
    ctl = R.Control(R.Params())
    out = drive(ctl, [0] * 200, dt=0.1)                        # 20 s of bad frames from a start that never initialises
    assert {o[2] for o in out} == {R.RESET_NONE} and ctl.control_status == R.INIT


def test_reset_until_init_succeeds_fires_alone():
    p = R.Params(targetFps=2.0, resetUntilInitSucceeds=1)
    ctl = R.Control(p)
    out = drive(ctl, [0] * 8)                                  # t = 0 .. 3.5: expired means 0 + 3 < t, first at t = 3.5
    assert [o[2] for o in out] == [0, 0, 0, 0, 0, 0, 0, R.RESET_FRESH]
    ctl.reset(False)
    assert ctl.last_reset_time == 3.5 and ctl.session.tracking_status == R.INIT and not ctl.session.initialized_orientation
    assert ctl.session.clock.first_sample and ctl.session.counter.entries == 0


def test_reset_on_failed_tracking_fires_alone():
    p = R.Params(targetFps=2.0, resetOnFailedTracking=1)
    ctl = R.Control(p)
    out = drive(ctl, [1, 1, 1, 1, 0, 0, 0, 0])
    assert [o[2] for o in out] == [0] * 7 + [R.RESET_KEEP_POSE]
    ctl.reset(True)
    assert ctl.session.initialized_orientation and ctl.control_status == R.LOST_TRACKING      # Control's status survives


def test_failed_to_initialize_after_a_reset_fires_alone_and_control_status_never_returns_to_init():
    p = R.Params(targetFps=2.0, resetOnFailedTracking=1)
    ctl = R.Control(p)
    drive(ctl, [1, 1, 1, 1, 0, 0, 0, 0])
    ctl.reset(True)                                            # at t = 3.5; the new session is INIT, Control stays LOST
    p.resetOnFailedTracking = 0
    out = drive(ctl, [0] * 8, t0=4.0)                          # expired: 3.5 + 3 < t, first at t = 7.0 (the seventh frame)
    assert [o[2] for o in out] == [0, 0, 0, 0, 0, 0, R.RESET_KEEP_POSE, R.RESET_KEEP_POSE]
    assert [o[0] for o in out] == [R.LOST_TRACKING] * 8 and ctl.control_status == R.LOST_TRACKING


def test_freeze_needs_its_parameter_and_a_control_status_past_init():
    p = R.Params(targetFps=2.0, freezeOnFailedTracking=1)
    ctl = R.Control(p)
    out = drive(ctl, [1, 1, 1, 1, 0, 0, 0, 0, 0])
    # INIT while Control is INIT: not frozen; TRACKING: not frozen; LOST (from the eighth frame on): frozen
    assert [o[1] for o in out] == [False] * 7 + [True, True]
    assert not any(o[1] for o in drive(R.Control(R.Params(targetFps=2.0)), [1, 1, 1, 1, 0, 0, 0, 0, 0]))


def test_clock_first_sample_repeat_and_platform_time():
    c = R.Clock()
    assert c.sample(10.0) == 0.0 and not c.first_sample and c.first_sample_t == 10.0 and c.time == 0.0
    assert c.sample(10.25) == 0.25 and c.time == 0.25
    assert c.sample(10.25) == 0.0 and c.time == 0.25           # a repeated timestamp: dt = 0, the predict is skipped
    assert c.sample(10.125) == -0.125 and c.time == 0.125      # a step back: dt < 0, skipped as well
    assert c.platform_time() == 10.125


@pytest.mark.parametrize("xa", [(0.3, -0.2, 9.7), (0.0, 0.0, 9.819), (5.0, 5.0, 1.0), (-3.0, 0.1, -2.0)])
def test_initialize_orientation_equals_the_oracle(oracle, xa):
    po = oracle.ekf_default_params(cameraTrailLength=3)
    e = oracle.Ekf(po)
    e.initialize_orientation(xa)
    q = R.initialize_orientation(po.gravity, xa)
    assert np.abs(q - e.m[R.ORI:R.ORI + 4]).max() <= 4 * 2.0 ** -53
    assert np.array_equal(np.array(e.P[R.ORI:R.ORI + 4, R.ORI:R.ORI + 4]), R.orientation_block(po))


def test_initialize_orientation_antiparallel_and_zero():
    q = R.initialize_orientation(9.819, (0.0, 0.0, -4.0))
    assert q.tolist() == [0.0, 1.0, 0.0, 0.0]                  # a half-turn about x
    z = R.initialize_orientation(9.819, (0.0, 0.0, 0.0))
    assert z[0] == math.sqrt(2.0) * 0.5 and not z[1:].any()


@pytest.mark.parametrize("trail", [3, 20])
def test_blockwise_transform_of_a_fresh_filter_equals_the_dense_oracle(oracle, trail):
    po = oracle.ekf_default_params(cameraTrailLength=trail)
    rng = np.random.default_rng(trail)
    pos = rng.normal(size=3) * 10
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    dense = R.reset_filter(oracle, po, True, pos, q)
    fresh = oracle.Ekf(po)
    m0, P0 = np.array(fresh.m), np.array(fresh.P)
    m0[R.ORI:R.ORI + 4] = R.initialize_orientation(po.gravity, np.zeros(3))
    P0[R.ORI:R.ORI + 4, R.ORI:R.ORI + 4] = R.orientation_block(po)
    m, P = R.transform_blockwise(m0, P0, trail, pos, q)
    md, Pd = np.array(dense.m), np.array(dense.P)
    assert np.abs(m - md).max() <= 8 * 2.0 ** -53 * max(1.0, np.abs(md).max())
    assert np.abs(P - Pd).max() <= 32 * 2.0 ** -53 * np.abs(Pd).max()
    off = Pd.copy()
    for s, k in [(0, 3), (3, 3), (6, 4)] + [(20 + 7 * c + o, k) for c in range(trail) for o, k in ((0, 3), (3, 4))]:
        off[s:s + k, s:s + k] = 0
    np.fill_diagonal(off, 0)
    assert not off.any()                                       # the dense product leaves nothing outside the diagonal blocks
    # the preserved upstream quirk: q0 is not a unit quaternion, so the mean's orientation is q / 2 and positions are pos
    assert np.abs(md[R.ORI:R.ORI + 4] - 0.5 * q).max() <= 4 * 2.0 ** -53
    assert np.array_equal(md[R.POS:R.POS + 3], pos) and np.array_equal(md[20:23], pos)
