"""Pins tests/ekf_control_restatement.py to the oracle (no GPU): oracle.Ekf is driven through predict(t), update_zupt,
update_zupt_initialization and update_pseudo_velocity over a schedule of times, and at every step the restatement's apply / skip
decision must equal "the oracle's covariance changed" -- the oracle carries its own rate limiters (oracle/ekf_oracle.c:457-499).
Frame period 0.06 s, IMU steps of 0.02 s, t = step * 0.02 with firstSampleT = 0: both sides evaluate the reference's comparisons
on the same doubles, so a difference that lands next to 0.25 s, 0.1 s or 60 s falls the same way for both."""
import math

import numpy as np
import pytest

import ekf_control_restatement as R

VEL = 3
IMU_DT, IMU_PER_FRAME = 0.02, 3
GRAVITY_ACC = np.array([0.0, 0.0, 9.81])


def drive(oracle, p, keyframe_of, n_frames, acc, seen):
    o = oracle.Ekf(oracle.ekf_default_params(cameraTrailLength=1))
    o.initialize_orientation(GRAVITY_ACC)
    o.set_first_sample_time(0.0)
    s = R.State()
    step = 0

    def changed(call):
        before = o.P.copy()
        call()
        return not np.array_equal(before, o.P)

    for frame in range(n_frames):
        for _ in range(IMU_PER_FRAME):
            step += 1
            time = step * IMU_DT
            o.predict(time, np.zeros(3), acc)
            o.normalize_quaternions(1)
            if p.useDecayingZeroVelocityUpdate:
                expired = time > 60 and not s.was_stationary
                want = R.imu_init_zupt(p, s, time)
                assert changed(o.update_zupt_initialization) == want, (frame, time)
                seen["init applied" if want else ("init expired" if expired else "init skipped")] = True
            h = math.sqrt(o.m[VEL] * o.m[VEL] + o.m[VEL + 1] * o.m[VEL + 1])
            if R.imu_pseudo_velocity(p, h):
                assert changed(lambda: o.update_pseudo_velocity(p.pseudoVelocityTarget, p.pseudoVelocityR)), (frame, time)
                seen["pv applied"] = True
            elif p.usePseudoVelocity:
                seen["pv below limit"] = True
        d = R.frame_control(p, s, time, keyframe_of(frame))
        if p.useVisualStationarity and d["stationary"]:
            assert changed(lambda: o.update_zupt(p.visualZuptR)) == d["zupt"], (frame, time)
            seen["zupt applied" if d["zupt"] else "zupt rate-limited"] = True
        else:
            assert not d["zupt"]
            seen["not stationary"] = True
        assert d["undo"] == (not d["keyframe_out"]) and d["keyframe_out"] == bool(keyframe_of(frame))
        assert bool(o.was_stationary()) == bool(s.was_stationary), (frame, time)
    return s


@pytest.mark.parametrize("decay,pv,limit", [(False, False, 1.4), (True, False, 1.4), (False, True, 0.3), (True, True, 0.05)])
def test_decisions_equal_the_oracles_rate_limiters(oracle, decay, pv, limit):
    """40 frames; frames 4-16 are not keyframes (not yet stationary, ZUPT applied, rate-limited, applied again), then every
    other one. A horizontal acceleration of 2 m/s^2 takes the speed through the pseudo-velocity limit (lowered so that the
    ZUPTs do not keep the speed below it)."""
    p = R.Params(useDecayingZeroVelocityUpdate=decay, usePseudoVelocity=pv, pseudoVelocityLimit=limit)
    seen = {}
    drive(oracle, p, lambda f: not (4 <= f <= 16) and f % 2 == 0, 40, GRAVITY_ACC + [2.0, 0.0, 0.0], seen)
    want = {"zupt applied", "zupt rate-limited", "not stationary"}
    if decay:
        want |= {"init applied", "init skipped"}
    if pv:
        want |= {"pv applied", "pv below limit"}
    assert want <= set(seen), sorted(seen)


def test_init_zupt_expires_after_sixty_seconds(oracle):
    """Every frame a keyframe, so no visual ZUPT ever sets wasStationary: the init-ZUPT runs every 0.1 s until time > 60."""
    p = R.Params(useDecayingZeroVelocityUpdate=True)
    seen = {}
    s = drive(oracle, p, lambda f: True, 1010, GRAVITY_ACC, seen)
    assert {"init applied", "init skipped", "init expired", "not stationary"} <= set(seen) and "zupt applied" not in seen
    assert 59.9 < s.init_zupt_time <= 60.0 and s.was_stationary == 0


def test_frame_rule_without_a_full_visual_update():
    """`if (!fullVisualUpdate) keyframe = false` (backend.cpp:790) comes after the counter: a keyframe of a partial frame resets
    framesSinceKeyframe and is still undone."""
    p, s = R.Params(), R.State(frames_since_keyframe=7)
    d = R.frame_control(p, s, 1.0, True, full_update=False)
    assert s.frames_since_keyframe == 0 and d == {"stationary": False, "zupt": False, "keyframe_out": False, "undo": True}
    p.useVisualStationarity = False
    s.frames_since_keyframe = 7
    d = R.frame_control(p, s, 2.0, False)
    assert d["stationary"] and not d["zupt"] and s.zupt_time == -1.0 and s.was_stationary == 0


def test_pseudo_velocity_skips_a_vanishing_speed(oracle):
    o = oracle.Ekf(oracle.ekf_default_params(cameraTrailLength=1))
    for h, due in ((0.0, False), (1e-7, False), (1.0000001e-7, True), (2.0, True)):
        m = o.m.copy(); m[VEL], m[VEL + 1] = h, 0.0
        o.set_state(m)
        before = o.P.copy()
        o.update_pseudo_velocity(0.0, 1e-4)
        assert (not np.array_equal(before, o.P)) == due == R.pseudo_velocity_due(h), h
        o.set_cov(before)
    p = R.Params(usePseudoVelocity=True, pseudoVelocityLimit=-1.0)
    assert not R.imu_pseudo_velocity(p, 1e-7) and R.imu_pseudo_velocity(p, 1e-3) and not R.imu_pseudo_velocity(R.Params(), 5.0)
