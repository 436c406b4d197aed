"""GPU tests of the sessions hv_vio_create_session builds (csrc/vio_engine.hip): mono and stereo, every track filter behind RANSAC2,
the three detectors. Each session against the same entries issued call by call from Python (tests/vio_chain.py), the default session
against hv_vio_create, and a mono session through in-place resets, replayed from one captured graph, and against the true
trajectory. Scenes from hybvio_amd/scene.py: 376 x 240, maxTracks 120, gfttMinDistance 8, two sets, ten IMU samples per frame."""
import functools

import numpy as np
import pytest

from hybvio_amd import capi

import vio_chain as vc
from vio_chain import H_, M, NS, S, W_

pytestmark = pytest.mark.gpu
# (c): on unrelated noise the mono LK still reports tracks with next to no flow, which every essential matrix explains, so set 1 has
# scattered good frames (in a stereo session the right image's noise fails the stereo LK and there are none). With the reference's
# own goodFramesToTracking of 0.75 the four-frame ring must be all good before a session is TRACKING: the scene does that from its
# seventh frame (0.35 s), isolated good frames never do, and a reset timer of 0.4 s lies behind the one and lets the other reset
# about every nine frames.
MONO_STRICT = dict(session__goodFramesToTracking=0.75)
MONO_RESET = dict(MONO_STRICT, session__resetUntilInitSucceeds=1, session__resetAfterTrackingFailsToInitialize=0.4)
UPRIGHT_2P, RANSAC5 = 4, 3                                         # RansacResult::Type as the entries report it

SESSIONS = {
    "mono_hybrid": dict(stereo=False),
    "mono_hybrid_ransac5_never_skipped": dict(stereo=False, ransac5__ransac2InliersToSkipRansac5=2.0),
    "mono_no_filter": dict(stereo=False, useHybridRansac=0),
    "stereo_upright2p": dict(useRansac3=0, useStereoUpright2p=1),
    "stereo_hybrid": dict(useRansac3=0),
    "stereo_fast": dict(featureDetector=capi.DETECTOR_FAST),
    "stereo_gftt_legacy": dict(featureDetector=capi.DETECTOR_GFTT),
}
FILTER_OF = dict(mono_hybrid=vc.FILTER_HYBRID, mono_hybrid_ransac5_never_skipped=vc.FILTER_HYBRID, mono_no_filter=vc.FILTER_NONE,
                 stereo_upright2p=vc.FILTER_UPRIGHT2P, stereo_hybrid=vc.FILTER_HYBRID, stereo_fast=vc.FILTER_RANSAC3,
                 stereo_gftt_legacy=vc.FILTER_RANSAC3)


@functools.lru_cache(maxsize=None)
def _mono_engine_run(frames, kind="plain"):
    p = vc.params(stereo=False, **dict(plain={}, strict=MONO_STRICT, reset=MONO_RESET)[kind])
    return vc.run_engine(p, vc.inputs(vc.scenes(24, "fast"), frames, stereo=False, noise_set=1 if kind == "reset" else None), frames)


@pytest.mark.parametrize("name", list(SESSIONS))
def test_the_engine_is_the_chain(name):
    """(a) 16 frames of two scene sequences: after every frame the table, the index, the session, the control block, the generators
    in use, the mean and covariance, every stage output of the view and the record are bit-equal between hv_vio_frame and the
    call-by-call chain. The chain asserts the facts that make the comparison worth something for the session at hand."""
    frames = 16
    over = SESSIONS[name]
    stereo = over.get("stereo", True)
    p = vc.params(**over)
    assert vc.session_of(p)[1] == FILTER_OF[name]
    inp = vc.inputs(vc.scenes(24, "fast"), frames, stereo=stereo)
    eng = _mono_engine_run(frames) if name == "mono_hybrid" else vc.run_engine(p, inp, frames)
    chain, facts = vc.run_chain(vc.params(**over), inp, frames)
    per_frame = facts["frames"]
    print("chain facts", name, {k: v for k, v in facts.items() if k not in ("full_update", "frames")})
    for f, fact in enumerate(per_frame):
        print("  frame", f, fact)
    for f in range(frames):
        vc.assert_equal(eng[f], chain[f], (name, "frame", f))
    assert facts["resets"] == [0, 0]
    if not stereo:
        assert "second_xy" not in eng[0]["table"] and eng[0]["trail"]["image_point"].shape == (S, p.trail.cameraTrailLength + 1, M, 1, 2)
    if name == "mono_hybrid":
        assert facts["full"] > 0 and facts["culled"] > 0, facts
        assert facts["inliers"] > 0 and facts["blacklisted"] > 0, facts
    if name == "mono_hybrid_ransac5_never_skipped":
        # inliers <= n < 2 n: RANSAC2 can never skip RANSAC5, so it runs wherever there are five valid points
        ran = np.array([[row[2] for row in fact["r5_summary"]] for fact in per_frame])
        assert (ran > 0).any(0).all(), ran.tolist()
    if name == "mono_no_filter":
        # the numpy restatement of ransac_pipeline.cpp:135 is what the chain fed the table: bit-equality above is the assertion;
        # here: the filter changed no status, the score was a real quotient somewhere and the unguarded 0 / 0 occurred
        assert all(fact["filter_changed"] == 0 for fact in per_frame)
        scores = np.array([fact["score"] for fact in per_frame])
        got = np.array([e["stage"]["ransac_score"] for e in eng])
        assert np.isnan(scores[0]).all() and np.isnan(got[0]).all()            # the first frame tracks nothing: 0 / 0
        assert (np.nan_to_num(scores, nan=-1.0) == np.nan_to_num(got, nan=-1.0)).all()
        assert ((scores > 0) & (scores <= 1)).any(0).all(), scores.tolist()
        assert all((np.array(e["stage"]["ransac_result"]) == 0).all() for e in eng)
    if name == "stereo_upright2p":
        res = np.array([fact["result"] for fact in per_frame])                  # [F][S][2]
        assert ((res[:, :, 0] == UPRIGHT_2P) & (res[:, :, 1] > 0)).any(), res.tolist()
    if name in ("stereo_fast", "stereo_gftt_legacy"):
        assert all(n > 0 for n in per_frame[0]["n_corners"]), per_frame[0]
        assert facts["inliers"] > 0, facts


def test_the_default_session_is_hv_vio_create():
    """(b) With default switches hv_vio_create_session builds the engine hv_vio_create builds: 8 frames, every array of the view
    bit-equal after every frame."""
    frames = 8
    inp = vc.inputs(vc.scenes(24, "fast"), frames)
    a = vc.run_engine(vc.params(), inp, frames, session=False)
    b = vc.run_engine(vc.params(), inp, frames, session=True)
    for f in range(frames):
        vc.assert_equal(b[f], a[f], ("frame", f))
    assert max(int(e["table"]["n_tracks"].max()) for e in a) > 0


def test_mono_reset_in_place():
    """(c) 24 mono frames with resetUntilInitSucceeds, resetAfterTrackingFailsToInitialize = 0.4 s and goodFramesToTracking = 0.75;
    set 1's images are unrelated noise, so it never fills its ring with good frames: it resets at least twice, set 0 never; engine
    and chain stay bit-equal through the resets, and set 0 is bit-equal to its run without them."""
    frames = 24
    eng = _mono_engine_run(frames, "reset")
    p = vc.params(stereo=False, **MONO_RESET)
    chain, facts = vc.run_chain(p, vc.inputs(vc.scenes(24, "fast"), frames, stereo=False, noise_set=1), frames)
    print("reset facts", {k: v for k, v in facts.items() if k not in ("full_update", "frames")}, "good",
          [e["stage"]["good_frame"].tolist() for e in eng], "status", [e["stage"]["tracking_status"].tolist() for e in eng], "kind",
          [e["stage"]["reset_kind"].tolist() for e in eng])
    for f in range(frames):
        vc.assert_equal(eng[f], chain[f], ("frame", f))
    assert facts["resets"][1] >= 2 and facts["resets"][0] == 0, facts
    kinds = np.array([e["stage"]["reset_kind"] for e in eng])
    assert (kinds[:, 1] != 0).sum() == facts["resets"][1] and (kinds[:, 0] == 0).all()
    plain = _mono_engine_run(16, "strict")
    for f in range(16):
        vc.assert_equal(eng[f], plain[f], ("set 0, frame", f), sets=[0])


def test_mono_replay_from_one_graph():
    """(d) One eager mono frame, then one frame captured and replayed for the remaining frames with the inputs copied into fixed
    buffers in front of each replay: every record is bit-equal to the eager run."""
    import torch
    frames = 16
    eager = _mono_engine_run(frames)
    inp = vc.inputs(vc.scenes(24, "fast"), frames, stereo=False)
    p = vc.params(stereo=False)
    with capi.Context(width=W_, height=H_, pool_size=2 * S, max_tracks=M) as ctx:
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            fixed = {k: torch.empty_like(v[0]) for k, v in inp.items() if v is not None}
            eng = capi.VioEngine(ctx, p, S, session=True)
            view = eng.view()
            assert eng.replay_period() == 1
            call = lambda: eng.frame(fixed["left"].data_ptr(), 0, H_ * W_, W_, NS, fixed["t"].data_ptr(), fixed["gyro"].data_ptr(),
                                     fixed["acc"].data_ptr())
            for k in fixed:
                fixed[k].copy_(inp[k][0])
            call()
        stream.synchronize()
        vc.assert_equal({"record": vc.host(view["record"])}, {"record": eager[0]["record"]}, "eager frame 0")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            call()
        for f in range(1, frames):
            with torch.cuda.stream(stream):
                for k in fixed:
                    fixed[k].copy_(inp[k][f])
                g.replay()
            stream.synchronize()
            vc.assert_equal({"record": vc.host(view["record"])}, {"record": eager[f]["record"]}, ("replayed frame", f))
        del g
        eng.close()


def test_mono_create_refuses_a_context_that_is_too_small():
    """(f) A mono engine takes 2 * n_sets pyramid slots: it is created on a pool of exactly that size, refused on one slot fewer
    with every slot left free, and its frame refuses a right image (as a stereo engine's frame refuses the lack of one)."""
    import torch
    p = vc.params(stereo=False)
    with capi.Context(width=W_, height=H_, pool_size=2 * S - 1, max_tracks=M) as ctx:
        with pytest.raises(capi.HvError, match="hv_vio_create_session"):
            capi.VioEngine(ctx, p, S, session=True)
        assert len([ctx.acquire() for _ in range(2 * S - 1)]) == 2 * S - 1        # every slot is still free
    with capi.Context(width=W_, height=H_, pool_size=2 * S, max_tracks=M) as ctx:
        with capi.VioEngine(ctx, p, S, session=True) as eng:
            raw = eng.raw_view()
            assert not raw.slot_right and not raw.table.second_xy                 # the stereo-only arrays do not exist
            assert raw.r5_summary and raw.ransac_result and raw.ransac_score      # the default mono filter is the hybrid one
            with pytest.raises(capi.HvError, match="hv_vio_frame"):               # a right image on a mono engine
                eng.frame(16, 16, H_ * W_, W_, NS, 16, 16, 16)
        torch.cuda.synchronize()
    with capi.Context(width=W_, height=H_, pool_size=3 * S, max_tracks=M) as ctx:
        with capi.VioEngine(ctx, vc.params(), S, session=True) as eng:
            assert eng.raw_view().slot_right and not eng.raw_view().r5_summary
            with pytest.raises(capi.HvError, match="hv_vio_frame"):               # no right image on a stereo engine
                eng.frame(16, 0, H_ * W_, W_, NS, 16, 16, 16)
        torch.cuda.synchronize()


def _quat_rot(q):
    w, x, y, z = q
    return np.array([[w*w+x*x-y*y-z*z, 2*x*y-2*w*z, 2*x*z+2*w*y], [2*x*y+2*w*z, w*w-x*x+y*y-z*z, 2*y*z-2*w*x],
                     [2*x*z-2*w*y, 2*y*z+2*w*x, w*w-x*x-y*y+z*z]])


def _dead_reckoning(sc, frames):
    """Strapdown integration of the same samples in numpy from the true initial state, independent of the library: the roll from
    the gyro's z rate, the specific force turned into the world and gravity removed, semi-implicit Euler at the sample rate."""
    pos, vel, th = sc.pos[0] * 0.0, np.zeros(3), 0.0
    h = sc.imu_t[1] - sc.imu_t[0]
    for k in range(1, frames * NS):
        th += sc.gyro[k, 2] * h
        R_wi = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
        pos = pos + vel * h
        vel = vel + (R_wi @ sc.acc[k] - np.array([0, 0, sc.gravity])) * h
    return pos


MONO_FRAMES = 80


def test_mono_ground_truth():
    """(e) The default stereo session's criterion on a mono session (left images only): 80 frames (4 s at 20 Hz) of the two
    trajectories of about 1 m with their rest phase, IMU white noise at the process-noise levels and a constant accelerometer bias of
    0.025 m/s^2; the oscillating trajectories accelerate throughout, which is what makes the scale observable without a second
    camera. e_dr: the position error at the end of a strapdown integration of the same samples; e_vio: the error of the record's
    position after the first record's pose is aligned rigidly to the truth. Every record finite, both sets TRACKING at the end
    without a reset, e_vio < e_dr / 2."""
    frames = MONO_FRAMES
    scs = vc.scenes(frames, "noisy")
    snaps = vc.run_engine(vc.params(fast=False, stereo=False), vc.inputs(scs, frames, stereo=False), frames)
    for s, sc in enumerate(scs):
        e_dr = np.linalg.norm(_dead_reckoning(sc, frames) - sc.pos[frames - 1])
        pose = np.array([sn["record"]["inertial_mean"][s] for sn in snaps])
        status = np.array([sn["record"]["tracking_status"][s] for sn in snaps])
        kinds = np.array([sn["stage"]["reset_kind"][s] for sn in snaps])
        # rigid alignment of the first record's pose to the truth: world_true = Ra (x - p_0) + pos_true_0
        Ra = _quat_rot(sc.quat[0]).T @ _quat_rot(pose[0, 6:10] / np.linalg.norm(pose[0, 6:10]))
        est = (pose[:, 0:3] - pose[0, 0:3]) @ Ra.T + sc.pos[0]
        e_vio = np.linalg.norm(est[-1] - sc.pos[frames - 1])
        first = int(np.argmax(status == capi.TRACKING_TRACKING)) if (status == capi.TRACKING_TRACKING).any() else -1
        print(f"set {s}: e_vio {e_vio:.4f} m, e_dr {e_dr:.4f} m, TRACKING from frame {first}, max error on the way "
              f"{np.linalg.norm(est - sc.pos[:frames], axis=1).max():.4f} m")
        assert all(np.isfinite(v).all() for sn in snaps for v in sn["record"].values() if v.dtype.kind == "f")
        assert (kinds == 0).all() and status[-1] == capi.TRACKING_TRACKING, (s, first, kinds.tolist())
        assert e_vio < 0.5 * e_dr, (s, e_vio, e_dr)
