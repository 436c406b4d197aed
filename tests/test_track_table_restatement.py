"""CPU checks of tests/track_table_restatement.py, the yardstick of the device track table: answers worked by hand from
src/tracker/tracker.cpp, and the kernel's key formulation of the culling against the literal all-pairs loop."""
import numpy as np

import track_table_restatement as T


def _grid(n, cols, step=1.0):
    return np.array([[(k % cols) * step, (k // cols) * step] for k in range(n)], np.float32)


def _spread(n):
    """n corners on a 50-pixel grid, then moved apart a little so that no two distances are equal."""
    rng = np.random.default_rng(n)
    return _grid(n, 8, 50.0) + rng.uniform(-5, 5, (n, 2)).astype(np.float32)


def _started(max_tracks, n, stereo=False, **kw):
    """A table after frame 0 holding n NEW tracks (IDs 1 .. n) at _spread(n)."""
    t = T.TrackTable(T.Params(maxTracks=max_tracks, **kw), 752, 480, stereo)
    r = t.update([], [], [])
    assert r["reset"] and r["keyframe"] and len(r["mask"]) == 0
    c = _spread(n)
    assert t.append(c, c + np.float32(1) if stereo else None) == n
    return t, c


def test_culling_takes_exactly_max_tracks_over_20_plus_1_and_only_at_capacity():
    for max_tracks, want in ((40, 3), (20, 2), (19, 1), (5, 1), (200, 11)):
        t, c = _started(max_tracks, max_tracks)
        st = [T.TRACKED] * max_tracks
        t.update(c, None, st)
        assert st.count(T.CULLED) == want == max_tracks // 20 + 1 and len(t.tracks) == max_tracks - want
    t, c = _started(40, 39)                                       # one below capacity: :621 does not hold
    st = [T.TRACKED] * 39
    t.update(c, None, st)
    assert st.count(T.CULLED) == 0 and len(t.tracks) == 39


def test_a_culled_slot_that_held_failed_flow_reads_culled():
    """:634 writes CULLED whatever the slot held. Corners 0 and 1 are made the closest pair, so j = 1 is culled first."""
    t, c = _started(20, 20)
    c[1] = c[0] + np.float32(0.25)
    st = [T.TRACKED] * 20
    st[1] = T.FAILED_FLOW
    r = t.update(c, None, st)
    assert st[1] == T.CULLED and st.count(T.CULLED) == 2
    assert len(r["mask"]) == 19                                   # setMask ran before the culling: only the FAILED_FLOW corner is absent
    assert 1 not in r["src_index"] and len(r["src_index"]) == 18


def test_ties_on_an_integer_grid_follow_generation_order():
    """40 corners at (k % 8, k // 8): the smallest dist2 is 1, shared by every horizontal and vertical neighbour pair.
    std::stable_sort keeps the generation order (i major, j minor) among them: (0, 1), (0, 8), (1, 2), (1, 9), ... The walk
    inserts j = 1, then j = 8, then j = 2, and stops there, because the set then holds 3 > 40 / 20 tracks."""
    c = _grid(40, 8)
    assert T.cull_literal(c, 40) == [1, 8, 2]
    assert T.cull_by_keys(c, 40) == [1, 8, 2]
    t, _ = _started(40, 40)
    st = [T.TRACKED] * 40
    r = t.update(c, None, st)
    assert [i for i, s in enumerate(st) if s == T.CULLED] == [1, 2, 8]
    assert r["src_index"] == [i for i in range(40) if i not in (1, 2, 8)]
    assert len(r["mask"]) == 40                                   # culled corners stay in the mask


def test_ids_over_three_frames():
    """nextTrackId = frameNum * maxTracks + 1 on entry to add() (:199), frameNum = 0, 1, 2."""
    t, c = _started(10, 6)
    assert [k["id"] for k in t.tracks] == [1, 2, 3, 4, 5, 6] and t.frameNum == 1
    st = [T.TRACKED] * 6
    st[2] = T.RANSAC_OUTLIER
    t.update(c, None, st)                                        # track 3 is erased; 5 missing >= 10 / 10
    assert t.append(_spread(9)[6:8]) == 2
    assert [k["id"] for k in t.tracks] == [1, 2, 4, 5, 6, 11, 12] and t.frameNum == 2
    t.update(np.array([k["p0"] for k in t.tracks]), None, [T.TRACKED] * 7)
    assert t.append(_spread(20)[10:20]) == 3                      # only the 3 missing tracks are taken
    assert [k["id"] for k in t.tracks] == [1, 2, 4, 5, 6, 11, 12, 21, 22, 23] and t.frameNum == 3
    assert [k["status"] for k in t.tracks] == [T.TRACKED] * 7 + [T.NEW] * 3
    t.update(np.array([k["p0"] for k in t.tracks]), None, [T.TRACKED] * 10)   # full: 1 culled, 1 missing >= 1
    assert len(t.tracks) == 9 and t.append(_spread(30)[25:30]) == 1 and t.tracks[-1]["id"] == 31


def test_detection_is_skipped_when_fewer_than_a_tenth_is_missing():
    t, c = _started(40, 38)                                       # missing = 2 < 40 / 10
    t.update(c, None, [T.TRACKED] * 38)
    assert t.append(_spread(45)[40:45]) == 0 and len(t.tracks) == 38
    t, c = _started(40, 36)                                       # missing = 4 >= 4
    t.update(c, None, [T.TRACKED] * 36)
    assert t.append(_spread(45)[40:45]) == 4 and len(t.tracks) == 40


def test_the_reset_below_five_tracks_keeps_mask_scale():
    t, c = _started(20, 8)
    st = [T.TRACKED] * 4 + [T.FAILED_FLOW] * 4
    t.update(c, None, st)
    t.append([])                                                 # 4 tracks < 15: maskScale -1
    assert len(t.tracks) == 4 and t.maskScale == -1.0 and t.frameNum == 2
    r = t.update(c[:4], None, [T.TRACKED] * 4)                    # fewer than five tracks: the else branch of add()
    assert r["reset"] and r["keyframe"] and len(r["mask"]) == 0 and t.tracks == [] and t.lastKeyframeCornerByTrackId == {}
    assert t.append(_spread(20)) == 20
    assert t.maskScale == -1.0 and t.frameNum == 3                # no tuning on a reset frame, frameNum still counts
    assert [k["id"] for k in t.tracks] == list(range(41, 61))     # 2 * 20 + 1 ...


def test_mask_radii():
    assert T.mask_radius(0.0, 752, 480, 0.0667) == 32             # 480 * 0.0667 = 32.016
    assert T.mask_radius(5.0, 752, 480, 0.0667) == 119            # 1.3^5 = 3.71293: 118.87
    assert T.mask_radius(-5.0, 752, 480, 0.0667) == 9             # 1.3^-5 = 0.269329: 8.62
    assert T.mask_radius(-5.0, 16, 16, 0.0667) == 2               # 0.287 rounds to 0: the floor
    assert T.mask_radius(0.0, 20, 30, 0.125) == 3                 # 2.5: std::round goes away from zero
    assert T._round(2.5) == 3 and T._round(3.5) == 4 and T._round(2.4999) == 2


def test_mask_steps_below_three_quarters_and_full():
    t, c = _started(20, 10)                                       # 10 < 15 on every frame
    seen = []
    for _ in range(7):
        t.update(c, None, [T.TRACKED] * 10)
        t.append([])
        seen.append(t.mask_steps())
    assert seen == [-2, -4, -6, -8, -10, -10, -10] and t.maskScale == -5.0
    t, c = _started(20, 20)
    seen = []
    for k in range(12):                                           # 2 culled, 2 missing >= 2, 2 appended: full again
        cur = np.array([q["p0"] for q in t.tracks], np.float32)
        t.update(cur, None, [T.TRACKED] * 20)
        assert t.append(_spread(20 + 2 * (k + 1))[-2:] + np.float32(400)) == 2
        seen.append(t.mask_steps())
    assert seen == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10, 10] and t.maskScale == 5.0
    t, c = _started(20, 16)                                       # 15 <= 16 < 20: neither branch
    t.update(c, None, [T.TRACKED] * 16)
    assert t.append([]) == 0 and t.mask_steps() == 0


def test_keyframe_rules():
    kw = dict(maxTrackLength=1)                                   # f + 1 < 1 never holds: stationarity alone decides
    # a new track has no keyframe entry: maxMovement = -1, not stationary, keyframe
    t, c = _started(20, 8, **kw)
    c = np.round(c)                                              # whole pixels, so that the displacements below are exact
    r = t.update(c, None, [T.TRACKED] * 8, score=1.0)
    assert r["max_movement"] == -1.0 and r["keyframe"]
    assert all(k["id"] in t.lastKeyframeCornerByTrackId for k in t.tracks)
    t.append([])
    # 3-4-5: maxMovement == 3.0 is not below 3.0
    moved = c.copy()
    moved[3] += np.array([3, 4], np.float32)
    moved[5] += np.array([1, 1], np.float32)
    r = t.update(moved, None, [T.TRACKED] * 8, score=1.0)
    assert r["max_movement"] == 5.0 and r["keyframe"]
    t.append([])
    moved2 = moved.copy()
    moved2[3] += np.array([0, 3], np.float32)
    r = t.update(moved2, None, [T.TRACKED] * 8, score=1.0)
    assert r["max_movement"] == 3.0 and r["keyframe"]
    t.append([])
    # below the threshold with a score above 0.95: stationary, no keyframe, and the keyframe entries stay
    moved3 = moved2.copy()
    moved3[3] += np.array([1, 1], np.float32)
    r = t.update(moved3, None, [T.TRACKED] * 8, score=0.96)
    assert r["max_movement"] == np.sqrt(np.float64(2)) and not r["keyframe"]
    assert tuple(t.lastKeyframeCornerByTrackId[4]) == tuple(moved2[3])
    t.append([])
    r = t.update(moved3, None, [T.TRACKED] * 8, score=0.95)      # 0.95 > 0.95 is false
    assert r["keyframe"]
    # a track that is not TRACKED takes no part: the only moved track failed
    t.append([])
    st = [T.TRACKED] * 8
    st[3] = T.FAILED_FLOW
    far = moved3.copy()
    far[3] += np.float32(100)
    r = t.update(far, None, st, score=1.0)
    assert r["max_movement"] == 0.0 and not r["keyframe"] and 4 not in t.lastKeyframeCornerByTrackId


def test_every_frame_before_max_track_length_is_a_keyframe():
    """keyframe = frameNum < maxTrackLength with frameNum = f + 1 (:207, 527): stationary frames at f = 19 and f = 20."""
    t, c = _started(20, 8)
    for f in range(1, 21):
        assert t.frameNum == f
        r = t.update(c, None, [T.TRACKED] * 8, score=1.0)
        t.append([])
        if f >= 2:
            assert r["max_movement"] == 0.0
        assert r["keyframe"] == (f <= 19), f                      # f = 19: 20 < 21; f = 20: 21 < 21 fails


def test_delete_track_blacklists_and_ignores_unknown_ids():
    t, c = _started(20, 8)
    t.deleteTrack(3)
    t.deleteTrack(3)
    t.deleteTrack(99)
    a = t.arrays()
    assert list(a["status"]) == [T.NEW, T.NEW, T.BLACKLISTED] + [T.NEW] * 5 and list(a["blacklist"]) == [0, 0, 1, 0, 0, 0, 0, 0]


def test_key_formulation_equals_the_literal_loop():
    """300 random sets, n from 2 to 200 (every set at capacity, maxTracks = n), half of them on integer grids of at most
    12 x 12 where equal distances are the rule: the culled tracks, in the order the walk meets them, are the same."""
    rng = np.random.default_rng(2024)
    sizes = [2, 3, 4, 5, 19, 20, 21, 39, 40, 41, 64, 199, 200] + [int(v) for v in rng.integers(2, 201, 287)]
    ties = 0
    for k, n in enumerate(sizes):
        if k % 2:
            side = int(rng.integers(2, 13))
            c = rng.integers(0, side, (n, 2)).astype(np.float32)
        else:
            c = rng.uniform(0, 752, (n, 2)).astype(np.float32)
        lit = T.cull_literal(c, n)
        assert lit == T.cull_by_keys(c, n), (k, n)
        assert len(lit) == min(n // 20 + 1, n - 1)
        _, _, d2 = T.all_pair_dist2(c)
        ties += len(np.unique(d2)) < len(d2)
    assert ties >= 100
