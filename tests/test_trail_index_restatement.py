"""Answers worked by hand from src/odometry/ekf_state_index.cpp and backend.cpp for tests/trail_index_restatement.py, the
yardstick of the device pose-trail index: a restatement that is wrong would make the GPU tests compare against nothing."""
import numpy as np
import pytest

import ransac3_restatement as R3
import trail_index_restatement as T

CAM = ("pinhole", 400.0, 400.0, 376.0, 240.0)


@pytest.fixture(scope="module")
def cams(oracle):
    c = oracle.Camera(*CAM)
    return (c, c)


def _tracks(ids, f, step=2.0):
    """Track `i` at (100 + 10 i + step f, 100 + i) in the first image, 4 pixels to the left in the second."""
    return [(i, (np.float32(100 + 10 * i + step * f), np.float32(100 + i)), (np.float32(96 + 10 * i + step * f), np.float32(100 + i)))
            for i in ids]


def _frame(ses, cams, f, ids, keyframe=True, t=None, tri=None, gate=None, draws=None, full=True, step=2.0):
    tr = _tracks(ids, f, step)
    sel = ses.select(tr, cams, keyframe, full, f + 1, 0.1 * (f + 1) if t is None else t, np.zeros(len(tr) + 1, np.uint32) if draws is None else draws)
    n = len(sel["candidates"])
    fin = ses.finish([T.TRI_NOT_VISITED] * n if tri is None else tri, [T.NOT_COMPUTED] * n if gate is None else gate, False)
    return sel, fin


def test_defaults_first_twenty_pushes_return_twenty_then_the_hanoi_cycle(cams):
    ses = T.Session(T.Params(), R3.normalize_pixel)
    removed = [_frame(ses, cams, f, range(6))[1]["discarded"] + 1 for f in range(20 + 24)]
    assert removed[:20] == [20] * 20                                       # free physical slots: nothing is removed
    assert [r - 1 for r in removed[20:]] == [16, 17, 16, 18, 16, 17, 16, 19] * 3
    assert ses.ekfStateIndex.frameCounter == 24 and len(ses.ekfStateIndex.keyframes) == 21


def test_an_empty_keyframe_behind_the_head_forces_the_last_slot(cams):
    ses = T.Session(T.Params(cameraTrailLength=6, cameraTrailHanoiLength=2), R3.normalize_pixel)
    for f in range(8):
        _frame(ses, cams, f, range(6))
    assert len(ses.ekfStateIndex.keyframes) == 7 and ses.ekfStateIndex.frameCounter == 2
    sel, fin = _frame(ses, cams, 8, range(10, 16))                          # every track is new: prune empties the trail
    assert fin["discarded"] + 1 == 6 and ses.ekfStateIndex.frameCounter == 2
    assert [len(k.features) for k in ses.ekfStateIndex.keyframes] == [0, 6, 0, 0, 0, 0, 0]
    ses = T.Session(T.Params(cameraTrailLength=6, cameraTrailHanoiLength=2, cameraTrailFixedScheme=True), R3.normalize_pixel)
    for f in range(8):
        _frame(ses, cams, f, range(6))
    assert _frame(ses, cams, 8, range(10, 16))[1]["discarded"] + 1 == 4     # the fixed scheme does not look: counter 3 -> 6 - 2 + 0
    assert ses.ekfStateIndex.frameCounter == 3


def test_strided_rule_length_two_stride_two(cams):
    ses = T.Session(T.Params(cameraTrailLength=8, cameraTrailHanoiLength=2, cameraTrailStridedLength=2, cameraTrailStridedStride=2),
                    R3.normalize_pixel)
    removed = [_frame(ses, cams, f, range(6))[1]["discarded"] + 1 for f in range(8 + 8)]
    assert removed[:8] == [8] * 8
    assert removed[8:] == [3, 6, 3, 7, 3, 6, 3, 8]                          # odd counters: firstNonStrided = 8 - 2 - 2 - 1


def test_gap_index_is_the_unused_poses_plus_the_oldest_holder_and_mark_used(cams):
    p = T.Params(cameraTrailLength=8, cameraTrailHanoiLength=2, trackMinFrames=4, scoreVisualUpdateTracks=False)
    ses = T.Session(p, R3.normalize_pixel)
    for f in range(3):
        sel, _ = _frame(ses, cams, f, range(3))
        assert sel["candidates"] == []                                      # fewer than trackMinFrames poses
    sel = ses.select(_tracks(range(3), 3), cams, True, True, 4, 0.4, np.zeros(4, np.uint32))
    assert [c["index"] for c in sel["candidates"]] == [[0, 1, 2, 3]] * 3
    order = [c["id"] for c in sel["candidates"]]
    ses.finish([T.TRI_OK] * 3, [T.INLIER, T.CHI2, T.INLIER], False)          # first and third are marked, the second blacklisted
    idx = ses.ekfStateIndex
    assert idx.createTrackIndex(order[0], T.GAP) == []                       # the new head is empty: the walk ends at keyframe 0 (:106)
    sel = ses.select(_tracks(range(3), 4), cams, True, True, 5, 0.5, np.zeros(4, np.uint32))
    assert idx.createTrackIndex(order[0], T.GAP) == [0, 4]                   # four used poses: the new one and the oldest holder
    assert idx.createTrackIndex(order[1], T.GAP) == [0, 1, 2, 3, 4] == idx.createTrackIndex(order[0], T.ALL)
    assert sel["candidates"] == [] and [t for _, t in sel["skipped"]] == [order[1]]   # 2 < trackMinFrames; the other is blacklisted
    ses.finish([], [], False)
    ses.select(_tracks(range(3), 5), cams, True, True, 6, 0.6, np.zeros(4, np.uint32))
    assert idx.createTrackIndex(order[0], T.GAP) == [0, 1, 5]                # the new poses + 1


def test_velocity_early_returns_on_equal_timestamps(cams):
    p = T.Params(cameraTrailLength=8, cameraTrailHanoiLength=2)
    ses = T.Session(p, R3.normalize_pixel)
    _frame(ses, cams, 0, [1], t=0.1)
    _frame(ses, cams, 1, [1], t=0.1)                                         # equal timestamps at keyframe 1: nothing is written
    kfs = ses.ekfStateIndex.keyframes
    assert kfs[1].features[1].frames[0].normalizedVelocity == [0.0, 0.0] and kfs[2].features[1].frames[0].normalizedVelocity == [0.0, 0.0]
    _frame(ses, cams, 2, [1], t=0.2)                                         # t0 > t1 = t2... keyframe 2 holds the track: t0 <= t2 fails
    kfs = ses.ekfStateIndex.keyframes
    f0, f1, f2 = (kfs[i].features[1].frames[0] for i in (1, 2, 3))
    v = (f0.normalizedImagePoint[0] - f1.normalizedImagePoint[0]) / (0.2 - 0.1)
    v2 = (f0.normalizedImagePoint[0] - f2.normalizedImagePoint[0]) / (0.2 - 0.1)
    assert f0.normalizedVelocity[0] == v and f1.normalizedVelocity[0] == v2 and v != 0.0
    ses = T.Session(p, R3.normalize_pixel)
    _frame(ses, cams, 0, [1], t=0.3)
    _frame(ses, cams, 1, [1], t=0.1)
    _frame(ses, cams, 2, [1], t=0.3)                                         # t0 > t1 but t0 <= t2: the return inside the loop (:378)
    kfs = ses.ekfStateIndex.keyframes
    head, mid = kfs[1].features[1], kfs[2].features[1]
    assert head.frames[0].normalizedVelocity[0] == (head.frames[0].normalizedImagePoint[0] - mid.frames[0].normalizedImagePoint[0]) / (0.3 - 0.1)
    assert head.frames[1].normalizedVelocity == [0.0, 0.0]                   # the second camera was never reached
    assert mid.frames[0].normalizedVelocity == [0.0, 0.0] and mid.frames[1].normalizedVelocity == [0.0, 0.0]


def test_min_track_score_is_the_median_of_the_int_truncated_scores(cams):
    p = T.Params(cameraTrailLength=8, cameraTrailHanoiLength=2, trackMinFrames=2, trackSampling=T.ALL)
    ses = T.Session(p, R3.normalize_pixel)
    speeds = {1: 0.25, 2: 0.75, 3: 1.5, 4: 2.5, 5: 0.4}                       # pixels per frame along x

    def tr(f):
        return [(i, (np.float32(100 + s * f), np.float32(50 * i)), (np.float32(96 + s * f), np.float32(50 * i))) for i, s in speeds.items()]
    for f in range(3):
        sel = ses.select(tr(f), cams, True, True, f + 1, 0.1 * (f + 1), np.zeros(8, np.uint32))
        ses.finish([T.TRI_NOT_VISITED] * len(sel["candidates"]), [T.NOT_COMPUTED] * len(sel["candidates"]), False)
    sel = ses.select(tr(3), cams, True, True, 4, 0.4, np.zeros(8, np.uint32))
    by_id = dict(zip(ses.track_ids, sel["scores"]))
    assert [float(by_id[i]) for i in (1, 2, 3, 4)] == [0.75, 2.25, 4.5, 7.5]
    assert abs(float(by_id[5]) - 1.2) < 1e-5
    # truncated: 0, 2, 4, 7, 1 -> sorted 0 1 2 4 7 -> element 5 / 2 = 2
    assert sel["minTrackScore"] == 2.0
    assert sorted(c["id"] for c in sel["candidates"]) == [2, 3, 4]            # 2.25 is not below 2


def test_blacklist_carry_before_and_after_the_stop_position(cams):
    p = T.Params(cameraTrailLength=8, cameraTrailHanoiLength=2, trackMinFrames=2, scoreVisualUpdateTracks=False,
                 maxSuccessfulVisualUpdates=1)
    ses = T.Session(p, R3.normalize_pixel)
    for f in range(2):
        _frame(ses, cams, f, range(1, 7))
    ses.blacklistedPrev = [2, 5]
    sel = ses.select(_tracks(range(1, 7), 2), cams, True, True, 3, 0.3, np.zeros(8, np.uint32))
    ids = ses.track_ids                                                       # zero draws: swap(order[i], order[0]) for i = 5 .. 1
    assert ids == [2, 3, 4, 5, 6, 1]
    assert sel["skipped"] == [(0, 2), (3, 5)] and [c["id"] for c in sel["candidates"]] == [3, 4, 6, 1]
    # the first candidate fails, the second succeeds and stops the loop (limit 1) at position 2: 2 is carried, 5 is not
    fin = ses.finish([T.TRI_OK, T.TRI_OK, T.TRI_NOT_VISITED, T.TRI_NOT_VISITED], [T.CHI2, T.INLIER, T.NOT_COMPUTED, T.NOT_COMPUTED], False)
    assert fin["blacklist"] == [2, 3] and fin["delete_ids"] == [3] and fin["good_frame"] and (fin["attempts"], fin["successes"]) == (2, 1)
    # a loop that never stops walks the whole order: both are carried, and the frame is not good unless stationary
    ses.blacklistedPrev = [2, 5]
    sel = ses.select(_tracks(range(1, 7), 3), cams, False, True, 4, 0.4, np.zeros(8, np.uint32))
    fin = ses.finish([T.TRI_OK] + [T.TRI_NOT_VISITED] * 3, [T.CHI2] + [T.NOT_COMPUTED] * 3, False)
    assert fin["blacklist"] == [2, 3, 5] and not fin["good_frame"]


def test_tracks_have_no_gaps_on_a_random_corpus_of_two_hundred_frames(cams):
    """select() asserts after every prune() that a keyframe's tracks are a subset of the head's and of the keyframe before it;
    here additionally: the per-track lengths alone rebuild the whole membership relation, which is what the device keeps."""
    for sampling, seed in ((T.GAP, 5), (T.ALL, 6)):
        p = T.Params(cameraTrailLength=6, cameraTrailHanoiLength=2, maxTracks=24, maxVisualUpdates=6, maxSuccessfulVisualUpdates=3,
                     trackSampling=sampling)
        pops = removed = 0
        for fr in T.drive(p, R3.normalize_pixel, cams, 200, seed):
            st, lengths = fr["after_select"], fr["select"]["lengths"]
            for i, feats in enumerate(st["features"]):
                assert set(feats) == {t for t, n in lengths.items() if n > i}, (fr["frame"], i)
            pops += not fr["keyframe"]
            removed += fr["n_kf_before_push"] == 7 and not fr["empty_tail"]
        assert pops > 20 and removed > 20
