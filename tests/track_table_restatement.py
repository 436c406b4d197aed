"""Literal restatement of the reference tracker's track bookkeeping (src/tracker/tracker.cpp), the yardstick of the device track
table (hv_tracks_*_batch_dev). TrackTable follows TrackerImplementation line by line: Python lists for `tracks`, a dict keyed by
track ID for lastKeyframeCornerByTrackId, all pairs and a stable sort for the culling, np.float32 / np.float64 exactly where the
C++ has float / double. One add() of the reference is update() followed by append(); the stages between them (detection) and
before them (LK, gate, RANSAC) are the caller's.

cull_by_keys() is the formulation the kernel uses; tests/test_track_table_restatement.py compares it with the literal loop."""
import math

import numpy as np

# tracker::Feature::Status (src/tracker/track.hpp:9-21)
TRACKED, NEW, FAILED_FLOW, RANSAC_OUTLIER, FLOW_OUT_OF_RANGE, OUT_OF_RANGE, FAILED_EPIPOLAR_CHECK, CULLED, BLACKLISTED = range(9)


class Params:
    def __init__(self, maxTracks=200, maxTrackLength=21, relativeMaskRadius=0.0667, visualStationarityMovementThreshold=3.0,
                 visualStationarityScoreThreshold=0.95):
        self.maxTracks = maxTracks                                                     # parameter_definitions.c:262
        self.maxTrackLength = maxTrackLength                                           # :265
        self.relativeMaskRadius = relativeMaskRadius                                   # :308
        self.visualStationarityMovementThreshold = visualStationarityMovementThreshold   # :111
        self.visualStationarityScoreThreshold = visualStationarityScoreThreshold       # :113


def _round(x):
    """std::round: halves away from zero."""
    r = math.floor(abs(x))
    if abs(x) - r >= 0.5:
        r += 1
    return int(math.copysign(r, x))


def mask_radius(mask_scale, width, height, relative_mask_radius):
    """TrackerImplementation::maskRadius (tracker.cpp:569-576)."""
    step = 1.3
    scale = math.pow(step, mask_scale)
    min_dim = min(width, height)
    r = _round(scale * min_dim * relative_mask_radius)
    if r < 2:
        r = 2
    return r


def compute_dist2(p1, p2):
    """computeDist2 (tracker.cpp:16-19): float differences widened to double."""
    dx = np.float64(np.float32(p1[0]) - np.float32(p2[0]))
    dy = np.float64(np.float32(p1[1]) - np.float32(p2[1]))
    return dx * dx + dy * dy


def all_pair_dist2(corners):
    """The (i, j, dist2) of tracker.cpp:624-629 in generation order (i major, j minor), vectorised: the same binary32
    differences, binary64 products and sum as compute_dist2."""
    c = np.asarray(corners, np.float32).reshape(-1, 2)
    i, j = np.triu_indices(len(c), 1)
    d = (c[i] - c[j]).astype(np.float64)
    return i, j, d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]


def cull_literal(corners, max_tracks):
    """tracker.cpp:621-639: all pairs, std::stable_sort by dist2, the walk until the set holds more than maxTracks / 20 tracks.
    -> the culled indices in the order the walk first meets them."""
    _, j, d2 = all_pair_dist2(corners)
    order = np.argsort(d2, kind="stable")
    delete, seen = [], set()
    for jj in j[order]:
        jj = int(jj)
        if jj not in seen:
            seen.add(jj)
            delete.append(jj)
        if len(seen) > max_tracks // 20:
            break
    return delete


def cull_by_keys(corners, max_tracks):
    """The kernel's formulation: the maxTracks / 20 + 1 tracks j >= 1 with the smallest key (min over i < j of dist2(i, j), the
    first i attaining it, j), compared lexicographically, ranked by counting."""
    c = np.asarray(corners, np.float32).reshape(-1, 2)
    n = len(c)
    kd, ki, kj = np.zeros(n - 1), np.zeros(n - 1, np.int64), np.arange(1, n)
    for j in range(1, n):
        d = (c[:j] - c[j]).astype(np.float64)
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        ki[j - 1] = int(np.argmin(d2))                           # the first index of the minimum
        kd[j - 1] = d2[ki[j - 1]]
    out = []
    for d, i, j in zip(kd, ki, kj):
        rank = int(np.count_nonzero((kd < d) | ((kd == d) & ((ki < i) | ((ki == i) & (kj < j))))))
        if rank < max_tracks // 20 + 1:
            out.append((rank, int(j)))
    return [j for _, j in sorted(out)]


class TrackTable:
    """The track state of one TrackerImplementation. A track is a dict(id, status, p0, p1); p1 is None in mono."""

    def __init__(self, params, width, height, stereo):
        self.p = params
        self.width, self.height, self.stereo = width, height, stereo
        self.frameNum = 0                                        # tracker.cpp:167
        self.maskScale = 0.0                                     # changeMaskSize(0.0) (:173)
        self.tracks = []
        self.lastKeyframeCornerByTrackId = {}
        self.maskCorners = []
        self.reset_frame = False
        self.frame_entry = 0

    # -- helpers of the reference --
    def changeMaskSize(self, change):                            # :561-567
        self.maskScale += change
        if self.maskScale < -5.0:
            self.maskScale = -5.0
        if self.maskScale > 5.0:
            self.maskScale = 5.0

    def maskRadius(self):
        return mask_radius(self.maskScale, self.width, self.height, self.p.relativeMaskRadius)

    def mask_steps(self):
        return int(round(2 * self.maskScale))

    def computeMaxPixelCoordinateMovement(self, corners, trackStatus):   # :21-41
        maxDist, n = np.float64(0), 0
        for i in range(len(corners)):
            if trackStatus[i] == TRACKED:
                prev = self.lastKeyframeCornerByTrackId.get(self.tracks[i]["id"])
                if prev is None:
                    continue
                d = np.sqrt(compute_dist2(corners[i], prev))
                maxDist = d if maxDist < d else maxDist          # std::max(maxDist, d)
                n += 1
        if n == 0:
            return np.float64(-1.0)
        return maxDist

    def computeVisualStationarity(self, corners, trackStatus, score):   # :578-602
        maxMovement = self.computeMaxPixelCoordinateMovement(corners, trackStatus)
        self.last_max_movement = maxMovement
        if maxMovement < 0.0:
            return False
        threshold = self.p.visualStationarityMovementThreshold
        stationarityScore = np.float64(score) * (1.0 if maxMovement < threshold else 0.0)
        return bool(stationarityScore > self.p.visualStationarityScoreThreshold)

    # -- one frame: update() then append() --
    def update(self, corners, second_corners, trackStatus, score=0.0):
        """add() up to and including updateTracks. trackStatus is a list, modified in place (CULLED). -> dict(keyframe,
        mask [m, 2], src_index, max_movement, reset)."""
        maxTracks = self.p.maxTracks
        self.frame_entry = self.frameNum
        n = len(self.tracks)
        if self.frameNum == 0 or n < 5:                          # initialize() / the else branch (:201-205, 222-229)
            self.reset_frame = True
            self.maskCorners = []                                # setMask({}, {})
            self.tracks = []                                     # resetAllTracks
            self.lastKeyframeCornerByTrackId = {}
            return dict(keyframe=True, mask=np.zeros((0, 2), np.float32), src_index=[], max_movement=np.float64(-1.0), reset=True)
        self.reset_frame = False
        corners = [(np.float32(x), np.float32(y)) for x, y in np.asarray(corners, np.float32).reshape(-1, 2)[:n]]
        if self.stereo:
            second_corners = [(np.float32(x), np.float32(y)) for x, y in np.asarray(second_corners, np.float32).reshape(-1, 2)[:n]]
        assert len(corners) == n and len(trackStatus) >= n
        frameNum = self.frameNum + 1                             # frameNum++ (:207)

        # setMask (:492, 766-777)
        self.maskCorners = [corners[i] for i in range(n) if trackStatus[i] == TRACKED]

        # :527-528. The reference's || skips computeVisualStationarity on the first frames; it has no side effect, and the table
        # reports maxMovement on every frame, so it is evaluated first here.
        stationary = self.computeVisualStationarity(corners, trackStatus, score)
        keyframe = frameNum < self.p.maxTrackLength or not stationary

        # updateTracks (:604-670)
        if n == maxTracks:
            for j in cull_literal(corners, maxTracks):
                trackStatus[j] = CULLED
        broken, src_index = [], []
        for i in range(n):
            t = self.tracks[i]
            t["status"] = trackStatus[i]
            if trackStatus[i] == TRACKED:
                t["p0"] = corners[i]
                if self.stereo:
                    t["p1"] = second_corners[i]
                if keyframe:
                    self.lastKeyframeCornerByTrackId[t["id"]] = t["p0"]
                src_index.append(i)
            else:
                broken.append(i)
                self.lastKeyframeCornerByTrackId.pop(t["id"], None)
        for i in reversed(broken):
            del self.tracks[i]
        return dict(keyframe=bool(keyframe), mask=np.array(self.maskCorners, np.float32).reshape(-1, 2), src_index=src_index,
                    max_movement=self.last_max_movement, reset=False)

    def append(self, new_corners, new_second=None):
        """detectNewFeatures' append / resetAllTracks, the maskScale tuning and frameNum. -> the number appended."""
        maxTracks = self.p.maxTracks
        new_corners = np.asarray(new_corners, np.float32).reshape(-1, 2)
        nextTrackId = self.frame_entry * maxTracks + 1           # :199
        added = 0
        missing = maxTracks - len(self.tracks)
        if self.reset_frame or missing >= maxTracks // 10:       # :686
            for i in range(len(new_corners)):
                if added >= missing:
                    break
                t = dict(id=nextTrackId, status=NEW, p0=(new_corners[i][0], new_corners[i][1]), p1=None)
                if self.stereo:
                    s = np.asarray(new_second, np.float32).reshape(-1, 2)[i]
                    t["p1"] = (s[0], s[1])
                self.tracks.append(t)
                added += 1
                nextTrackId += 1
        if not self.reset_frame:                                 # :540-546
            if len(self.tracks) < (3 * maxTracks) // 4:
                self.changeMaskSize(-1.0)
            elif len(self.tracks) == maxTracks:
                self.changeMaskSize(0.5)
        self.frameNum = self.frame_entry + 1
        self.reset_frame = False
        return added

    def deleteTrack(self, track_id):                             # :726-738
        for t in self.tracks:
            if t["id"] == track_id:
                t["status"] = BLACKLISTED
                return

    # -- the table's arrays --
    def arrays(self):
        n = len(self.tracks)
        ids = np.array([t["id"] for t in self.tracks], np.int32)
        xy = np.array([t["p0"] for t in self.tracks], np.float32).reshape(n, 2)
        second = np.array([t["p1"] for t in self.tracks], np.float32).reshape(n, 2) if self.stereo else None
        status = np.array([t["status"] for t in self.tracks], np.int32)
        kf_valid = np.array([t["id"] in self.lastKeyframeCornerByTrackId for t in self.tracks], np.uint8)
        kf_xy = np.array([self.lastKeyframeCornerByTrackId.get(t["id"], (0, 0)) for t in self.tracks], np.float32).reshape(n, 2)
        return dict(n_tracks=n, ids=ids, xy=xy, second_xy=second, status=status, blacklist=(status == BLACKLISTED).astype(np.uint8),
                    kf_valid=kf_valid, kf_xy=kf_xy, frame_num=self.frameNum, mask_steps=self.mask_steps(),
                    mask_radius=self.maskRadius())
