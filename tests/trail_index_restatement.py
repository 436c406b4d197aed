"""Literal restatement of the reference's pose-trail index (src/odometry/ekf_state_index.{hpp,cpp}) and of what Session does
with it around the visit loop (src/odometry/backend.cpp:793-805, 909-1052, 1189-1213, 1240-1243, 1269-1274), the yardstick of
the device pose-trail index (hv_trail_*_batch_dev). EKFStateIndex follows the class line by line: a Python list of KeyFrame,
each with a dict keyed by track ID; Python floats where the C++ has double, np.float32 where it has float. Session.select() is
the frame up to the visit loop, Session.finish() the loop's bookkeeping replayed over the outcomes of the visits (the visits
themselves belong to the filter). Pixel normalisation is the caller's `normalize(camera, x, y) -> (ok, u, v)`
(ransac3_restatement.normalize_pixel over oracle.Camera). Nothing here reads the reference tree.

Not restated (HV_ERR_UNSUPPORTED in the library): TrackSampling::RANDOM, the hybrid map, useIndependentStereoTriangulation,
fullPointCloud. drive() at the end is the random corpus the CPU and the GPU tests share."""
import numpy as np

GAP, ALL, RANDOM = 0, 1, 2                                                              # TrackSampling (parameters.hpp)
TRI_OK, TRI_NOT_VISITED = 0, -1                                                         # hybvio_hip.h: HV_TRI_*
INLIER, NOT_COMPUTED, CHI2 = 0, 1, 3                                                    # VuOutlierStatus (output.hpp)
FAILED_UPDATES_THRESHOLD = 5                                                            # backend.cpp:1272


class Params:
    def __init__(self, **over):
        self.cameraTrailLength = 20                                                    # codegen/parameter_definitions.c
        self.cameraTrailHanoiLength = 3
        self.cameraTrailStridedLength = 0
        self.cameraTrailStridedStride = 2
        self.cameraTrailFixedScheme = False
        self.trackSampling = GAP
        self.trackMinFrames = 4
        self.scoreVisualUpdateTracks = True
        self.blacklistTracks = True
        self.maxVisualUpdates = 20
        self.maxSuccessfulVisualUpdates = 5
        self.estimateImuCameraTimeShift = True
        self.useStereo = True
        self.maxTracks = 200
        for k, v in over.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


class Frame:                                                                            # ekf_state_index.hpp:29-42
    def __init__(self):
        self.imagePoint = [-1.0, -1.0]
        self.normalizedImagePoint = [-1.0, -1.0]
        self.normalizedVelocity = [0.0, 0.0]


class Feature:                                                                          # ekf_state_index.hpp:26-57
    def __init__(self):
        self.frames = [Frame(), Frame()]
        self.usedForVisualUpdate = False


class KeyFrame:                                                                         # ekf_state_index.hpp:59-78
    def __init__(self, frameNumber, timestamp):
        self.frameNumber, self.timestamp, self.features = frameNumber, timestamp, {}

    def hasFeature(self, trackId):                                                      # :68-70
        return trackId in self.features

    def insertFeatureUnlessExists(self, trackId, feature):                              # :72-77
        if trackId not in self.features:
            self.features[trackId] = feature


def findTrackBeginMemoryIndex(keyframes, trackId):                                      # ekf_state_index.cpp:7-16
    bestIndex = len(keyframes)
    for i, kf in enumerate(keyframes):
        if kf.hasFeature(trackId):
            bestIndex = i
    return bestIndex


class EKFStateIndex:
    def __init__(self, parameters):                                                     # ekf_state_index.hpp:100-107
        self.parameters = parameters
        self.keyframes = []
        self.frameCounter = 0
        assert parameters.cameraTrailHanoiLength + parameters.cameraTrailStridedLength + 1 < self.maxSize()   # :104
        self.pushHeadKeyframe(0, 0.0)                                                   # :106

    def maxSize(self):                                                                  # :97
        return self.parameters.cameraTrailLength + 1

    def headKeyFrame(self):                                                             # :154
        return self.keyframes[0]

    def pushHeadKeyframe(self, frameNumber, timestamp):                                 # ekf_state_index.cpp:23-31
        removedIdx = self.maxSize() - 1                                                 # :24
        if len(self.keyframes) > self.maxSize() - 1:                                    # :25
            removedIdx = self.removeKeyframe()                                          # :26
        self.keyframes.insert(0, KeyFrame(frameNumber, timestamp))                      # :28-29
        return removedIdx                                                               # :30

    def popHeadKeyframe(self):                                                          # :33-39
        assert self.keyframes                                                           # :34
        del self.keyframes[0]                                                           # :35
        assert self.keyframes                                                           # :36
        self.keyframes[0].features.clear()                                              # :38

    def trackScore(self, trackId, selection):                                           # :41-87
        score = np.float32(0)                                                           # :43
        startIndex = findTrackBeginMemoryIndex(self.keyframes, trackId) if selection == GAP else -1   # :44-46
        prevFeature = None                                                              # :48
        for i, kf in enumerate(self.keyframes):                                         # :49
            feature = kf.features.get(trackId)                                          # :51
            if feature is None:                                                         # :53 "Assume tracks have no gaps."
                break
            useThis = False                                                             # :56
            if selection == ALL:                                                        # :57-59
                useThis = True
            elif selection == GAP:                                                      # :60-64
                if not feature.usedForVisualUpdate or i == startIndex:
                    useThis = True
            else:
                raise AssertionError("no implementation for TrackSampling")
            if useThis and prevFeature is not None:                                     # :70-76, float += double
                a, b = feature.frames[0].imagePoint, prevFeature.frames[0].imagePoint
                l1 = abs(a[0] - b[0]) + abs(a[1] - b[1])                                 # lpNorm<1>()
                score = np.float32(float(score) + l1)
            prevFeature = feature                                                       # :79
        return score                                                                    # :86

    def createTrackIndex(self, trackId, selection):                                     # :90-147 -> index
        index = []
        startIndex = findTrackBeginMemoryIndex(self.keyframes, trackId) if selection == GAP else -1   # :98-100
        for i, kf in enumerate(self.keyframes):                                         # :102
            item = kf.features.get(trackId)                                             # :104
            if item is None:                                                            # :106
                break
            if selection == ALL:                                                        # :108-110
                index.append(i)
            elif selection == GAP:                                                      # :111-115
                if not item.usedForVisualUpdate or i == startIndex:
                    index.append(i)
            else:
                raise AssertionError("no implementation for TrackSampling")
        assert len(index) <= len(self.keyframes)                                        # :146
        return index

    def markTrackUsed(self, trackId, index, selection):                                 # :156-181
        if selection == GAP:                                                            # :161-169
            for kf in self.keyframes:
                item = kf.features.get(trackId)
                if item is not None:
                    item.usedForVisualUpdate = True
        else:
            assert selection == ALL                                                     # :179

    def buildTrackVectors(self, trackId, index, stereo):                                # :192-218 -> imageFeatures, featureVelocities, y
        imageFeatures, featureVelocities, y = [], [], []
        frameCount = 2 if stereo else 1                                                 # :205
        for frameInd in range(frameCount):                                              # :207
            for j in index:                                                             # :208
                frame = self.keyframes[j].features[trackId].frames[frameInd]            # :209
                y += [frame.normalizedImagePoint[0], frame.normalizedImagePoint[1]]     # :211-212
                imageFeatures.append(list(frame.normalizedImagePoint))                  # :213
                featureVelocities.append(list(frame.normalizedVelocity))                # :214
        assert len(featureVelocities) == len(imageFeatures)                             # :217
        return imageFeatures, featureVelocities, y

    def prune(self):                                                                    # :220-242, without the map points
        kfRef = self.headKeyFrame()                                                     # :221
        i = 1
        while i < len(self.keyframes):                                                  # :229
            features = self.keyframes[i].features                                       # :230
            for trackId in [t for t in features if t not in kfRef.features]:            # :231-235
                del features[trackId]
            if not features:                                                            # :236-240
                i += 1
                while i < len(self.keyframes):
                    self.keyframes[i].features.clear()
                    i += 1
                return
            i += 1

    def removeKeyframe(self):                                                           # :244-281
        p = self.parameters
        assert self.keyframes                                                           # :245
        removedIdx = -1                                                                 # :246
        if not p.cameraTrailFixedScheme:                                                # :247-254
            for i in range(1, len(self.keyframes)):
                if not self.keyframes[i].features:
                    removedIdx = self.maxSize() - 1
                    break
        if removedIdx < 0:                                                              # :259
            self.frameCounter += 1                                                      # :260
            stride = p.cameraTrailStridedStride if p.cameraTrailStridedLength > 0 else 1   # :261
            if self.frameCounter % stride != 0:                                         # :262-265
                removedIdx = self.maxSize() - 1 - p.cameraTrailStridedLength - p.cameraTrailHanoiLength - 1
            else:                                                                       # :266-275
                hanoiCounter = self.frameCounter // stride
                removedIdx = self.maxSize() - 1
                for i in range(p.cameraTrailHanoiLength):
                    if (hanoiCounter >> i) & 0x1:
                        removedIdx = self.maxSize() - 1 - p.cameraTrailHanoiLength + i
                        break
        assert removedIdx < len(self.keyframes)                                         # :278
        del self.keyframes[removedIdx]                                                  # :279
        return removedIdx                                                               # :280

    def updateVelocities(self, trackId):                                                # :361-384
        kfs = self.keyframes
        if len(kfs) < 2:                                                                # :362
            return
        if kfs[0].timestamp <= kfs[1].timestamp:                                        # :363
            return
        if trackId not in kfs[0].features or trackId not in kfs[1].features:            # :364
            return
        feature0, feature1 = kfs[0].features[trackId], kfs[1].features[trackId]         # :365-366
        for i in (0, 1):                                                                # :368
            f0, f1 = feature0.frames[i], feature1.frames[i]                             # :369-370
            dt = kfs[0].timestamp - kfs[1].timestamp
            v = [(f0.normalizedImagePoint[0] - f1.normalizedImagePoint[0]) / dt,
                 (f0.normalizedImagePoint[1] - f1.normalizedImagePoint[1]) / dt]        # :371-372
            f0.normalizedVelocity = list(v)                                             # :373
            if len(kfs) == 2 or trackId not in kfs[2].features:                         # :374-376
                f1.normalizedVelocity = list(v)
            else:
                if kfs[0].timestamp <= kfs[2].timestamp:                                # :378
                    return
                f2 = kfs[2].features[trackId].frames[i]                                 # :379
                dt2 = kfs[0].timestamp - kfs[2].timestamp
                f1.normalizedVelocity = [(f0.normalizedImagePoint[0] - f2.normalizedImagePoint[0]) / dt2,
                                         (f0.normalizedImagePoint[1] - f2.normalizedImagePoint[1]) / dt2]   # :380-381

    # ---- not in the reference: what the tests look at ----
    def assert_no_gaps(self):
        """After prune(): every keyframe's features are a subset of the head's, and a track sits in keyframes 0 .. k - 1."""
        head = self.keyframes[0].features
        for i in range(1, len(self.keyframes)):
            cur, older = self.keyframes[i].features, self.keyframes[i - 1].features
            assert set(cur) <= set(head), (i, sorted(set(cur) - set(head)))
            assert set(cur) <= set(older), (i, sorted(set(cur) - set(older)))

    def lengths(self):
        """track ID -> number of keyframes that hold it."""
        out = {}
        for kf in self.keyframes:
            for t in kf.features:
                out[t] = out.get(t, 0) + 1
        return out


def shuffleDeterministic(order, draws):                                                 # util/util.hpp:39-44 -> draws consumed
    n, k = len(order), 0                                                                # :40
    for i in range(n - 1, 0, -1):                                                       # :41
        j = int(draws[k]) % (i + 1)
        k += 1
        order[i], order[j] = order[j], order[i]                                         # :42
    return k


class Session:
    """The members of Session this part of the frame touches: ekfStateIndex and blacklistedPrev."""

    def __init__(self, parameters, normalize):
        self.p, self.normalize = parameters, normalize
        self.ekfStateIndex = EKFStateIndex(parameters)
        self.blacklistedPrev = []
        self.trackOrder, self.track_ids, self.walk, self.candidates = [], [], [], []

    def select(self, tracks, cameras, keyframe, full, frame_num, t, draws):
        """backend.cpp:793-800 and trackerVisualUpdate up to the visit loop's filter (:909-1052). tracks: [(id, (x0, y0), (x1, y1)
        or None)] in table order. -> dict(order, draws_used, scores, minTrackScore, candidates, skipped)."""
        p, idx = self.p, self.ekfStateIndex
        if not keyframe:                                                                # :793-796
            if len(idx.keyframes) >= 2:                                                 # the reference asserts (:36); the library's rule
                idx.popHeadKeyframe()
        head = idx.headKeyFrame()                                                       # :798-800
        head.frameNumber, head.timestamp = int(frame_num), float(t)
        trackOrder = []                                                                 # :907
        for i, (trackId, uv0, uv1) in enumerate(tracks):                                # :909
            frameCount = 2 if p.useStereo else 1                                        # :913
            success, feature = False, Feature()                                         # :914-915
            for frameInd in range(frameCount):                                          # :916
                uv = (uv0, uv1)[frameInd]                                               # :917
                feature.frames[frameInd].imagePoint = [float(np.float32(uv[0])), float(np.float32(uv[1]))]   # :918
                success, u, v = self.normalize(cameras[frameInd], uv[0], uv[1])         # :923
                if not success:                                                         # :924
                    break
                feature.frames[frameInd].normalizedImagePoint = [u, v]
            if success:                                                                 # :944-950
                idx.headKeyFrame().insertFeatureUnlessExists(trackId, feature)
                if p.estimateImuCameraTimeShift:
                    idx.updateVelocities(trackId)
                trackOrder.append(i)
        idx.prune()                                                                     # :955
        idx.assert_no_gaps()
        draws_used = shuffleDeterministic(trackOrder, draws)                            # :964
        ids = [tracks[i][0] for i in trackOrder]
        scores = [idx.trackScore(t_, p.trackSampling) for t_ in ids]
        minTrackScore = np.float32(0.0)                                                 # :976
        if p.scoreVisualUpdateTracks:                                                   # :977-992
            trackScores = sorted(int(s) for s in scores)                                # static_cast<int>
            minTrackScore = np.float32(trackScores[len(trackScores) // 2] if trackScores else -1)
        walk, candidates, skipped = [], [], []
        for pos, trackId in enumerate(ids):                                             # :1012
            poseTrailIndex = idx.createTrackIndex(trackId, p.trackSampling)             # :1017
            nValid = len(poseTrailIndex)                                                # :1018
            score = scores[pos]                                                         # :1021, the same call as at :988
            if p.scoreVisualUpdateTracks and score < minTrackScore:                     # :1022-1025
                walk.append(("score", None)); continue
            if nValid < p.trackMinFrames:                                               # :1026-1029
                walk.append(("short", None)); continue
            if not full:                                                                # :1034
                walk.append(("lite", None)); continue
            if p.blacklistTracks and trackId in self.blacklistedPrev:                   # :1039-1046
                walk.append(("blacklisted", trackId)); skipped.append((pos, trackId)); continue
            if len(candidates) >= p.maxVisualUpdates:                                   # the list closes: the loop has stopped by then
                walk.append(("closed", None)); continue
            f, v, y = idx.buildTrackVectors(trackId, poseTrailIndex, p.useStereo)       # :1051-1052
            walk.append(("candidate", len(candidates)))
            candidates.append(dict(id=trackId, pos=pos, index=poseTrailIndex, features=f, velocities=v, y=y))
        self.trackOrder, self.track_ids, self.walk, self.candidates = trackOrder, ids, walk, candidates
        return dict(order=list(trackOrder), draws_used=draws_used, scores=scores, minTrackScore=minTrackScore,
                    candidates=candidates, skipped=skipped, lengths=idx.lengths())

    def finish(self, tri_status, gate_status, stationary, frame_num=None, t=None):
        """The visit loop (:1012-1252) replayed over the outcome of every candidate's visit, the end of the frame (:1269-1276)
        and the push (:804). tri_status / gate_status: per candidate, TRI_NOT_VISITED where the filter did not visit it."""
        p, idx = self.p, self.ekfStateIndex
        updateAttemptCount = updateSuccessCount = 0                                     # :902-903
        blacklisted, deleted = [], []                                                   # :906
        needMoreVisualUpdates = True                                                    # :999
        for kind, arg in self.walk:                                                     # :1012
            if kind == "blacklisted":                                                   # :1039-1046
                blacklisted.append(arg)
                continue
            if kind != "candidate" or tri_status[arg] == TRI_NOT_VISITED:
                continue
            c = self.candidates[arg]
            updateAttemptCount += 1                                                     # :1121
            if gate_status[arg] == INLIER:                                              # :1161, 1188-1189
                updateSuccessCount += 1
                idx.markTrackUsed(c["id"], c["index"], p.trackSampling)
            elif p.blacklistTracks:                                                     # :1204-1213
                blacklisted.append(c["id"])
                deleted.append(c["id"])
            limitSuccessful = p.maxSuccessfulVisualUpdates > 0 and updateSuccessCount >= p.maxSuccessfulVisualUpdates   # :1240
            limitTotal = p.maxVisualUpdates > 0 and updateAttemptCount >= p.maxVisualUpdates                           # :1241
            if limitSuccessful or limitTotal:                                           # :1242-1244
                needMoreVisualUpdates = False
                break
        self.blacklistedPrev = blacklisted                                              # :1269
        tooManyFailures = updateAttemptCount - updateSuccessCount > FAILED_UPDATES_THRESHOLD   # :1273
        goodFrame = (bool(stationary) or not needMoreVisualUpdates) and not tooManyFailures    # :1274
        head = idx.headKeyFrame()
        droppedPose = idx.pushHeadKeyframe(head.frameNumber if frame_num is None else frame_num,
                                           head.timestamp if t is None else t)          # :804
        return dict(delete_ids=deleted, good_frame=goodFrame, attempts=updateAttemptCount, successes=updateSuccessCount,
                    discarded=droppedPose - 1, blacklist=list(blacklisted))            # :805 "different indexing"

    def state(self):
        """Everything the device state holds, in logical order."""
        idx = self.ekfStateIndex
        return dict(n_keyframes=len(idx.keyframes), frame_counter=idx.frameCounter,
                    frame_number=[k.frameNumber for k in idx.keyframes], timestamp=[k.timestamp for k in idx.keyframes],
                    features=[{t: ([list(f.frames[c].imagePoint) for c in (0, 1)], [list(f.frames[c].normalizedImagePoint) for c in (0, 1)],
                                   [list(f.frames[c].normalizedVelocity) for c in (0, 1)], bool(f.usedForVisualUpdate))
                               for t, f in k.features.items()} for k in idx.keyframes],
                    blacklist=list(self.blacklistedPrev))


# ---- the random corpus ---------------------------------------------------------------------------------------------------------------
def synthetic_outcomes(rng, p, n_candidates, mode):
    """Statuses that obey the loop rule: a visited prefix that ends where the success limit or the attempt limit is reached
    ("limits"), or a shorter one that never stops ("early"). -> tri [n], gate [n]."""
    tri, gate = [TRI_NOT_VISITED] * n_candidates, [NOT_COMPUTED] * n_candidates
    visit = n_candidates if mode == "limits" else int(rng.integers(0, n_candidates + 1))
    attempts = successes = 0
    for v in range(visit):
        r = rng.random()
        if r < 0.45:
            tri[v], gate[v] = TRI_OK, INLIER
        elif r < 0.75:
            tri[v], gate[v] = TRI_OK, CHI2
        else:
            tri[v], gate[v] = int(rng.integers(2, 7)), NOT_COMPUTED                      # a failed triangulation: never gated
        attempts += 1
        successes += gate[v] == INLIER
        if (p.maxSuccessfulVisualUpdates > 0 and successes >= p.maxSuccessfulVisualUpdates) or attempts >= p.maxVisualUpdates:
            break
    return tri, gate


def drive(p, normalize, cameras, frames, seed, width=752, height=480, beyond=None, warm=0, special=(7, 13), drop=0.08, p_key=0.7):
    """One sequence of `frames` frames driven through Session: a little track table of its own (tracks drift, are dropped,
    replaced by new IDs and compacted; a frame without tracks, one with a single track and frames at capacity), random keyframe
    flags with runs of non-keyframes (none in the first `warm` frames, which fill a long trail), timestamps with repeats, blacklists that come from the outcomes, and synthetic outcomes. `beyond`: a
    special: the frames without tracks / with a single track; drop: the chance that a track is lost in a frame; p_key: the chance
    of a keyframe outside a run. callable (rng) -> pixel outside the valid field of view, given to some tracks. Yields per frame a dict of the inputs, what
    select() and finish() returned and the state after each."""
    rng = np.random.default_rng(seed)
    M = p.maxTracks
    ses = Session(p, normalize)
    tracks, next_id, t, run = [], 1, 0.0, 0
    for f in range(frames):
        # the table: drop, move, append
        if f == special[0]:
            tracks = []                                                                 # a frame with zero tracks
        elif f == special[1]:
            tracks = tracks[:1]                                                         # a single track: no draw is consumed
        else:
            tracks = [tr for tr in tracks if rng.random() > (0.5 if f % 11 == 5 else drop)]
            for tr in tracks:
                step = rng.uniform(-3, 3, 2).astype(np.float32)
                tr[1] = (np.float32(tr[1][0] + step[0]), np.float32(tr[1][1] + step[1]))
                tr[2] = (np.float32(tr[1][0] - np.float32(4)), tr[1][1])
            target = M if f % 5 == 0 else int(rng.integers(max(M // 2, 1), M + 1))
            while len(tracks) < target:
                xy = rng.uniform([20, 20], [width - 20, height - 20]).astype(np.float32)
                if beyond is not None and rng.random() < 0.15:
                    xy = np.asarray(beyond(rng), np.float32)
                tracks.append([next_id, (xy[0], xy[1]), (np.float32(xy[0] - np.float32(4)), xy[1])])
                next_id += 1
        # keyframe flags with runs of non-keyframes; frame 0 is a keyframe as in the track table
        if run > 0:
            keyframe, run = False, run - 1
        else:
            keyframe = f < max(warm, 1) or rng.random() < p_key
            if not keyframe:
                run = int(rng.integers(0, 4))
        full = f < warm or rng.random() < 0.9
        keyframe = keyframe and full                                                   # backend.cpp:790
        if rng.random() < 0.8:
            t += float(rng.choice([0.05, 0.1, 0.033]))                                 # else: a repeated timestamp
        draws = rng.integers(0, 2 ** 32, M, dtype=np.uint32)
        table = [(tr[0], tr[1], tr[2] if p.useStereo else None) for tr in tracks]
        sel = ses.select(table, cameras, keyframe, full, f + 1, t, draws)
        after_select = ses.state()
        n_kf_before_push = len(ses.ekfStateIndex.keyframes)
        empty_tail = any(not k.features for k in ses.ekfStateIndex.keyframes[1:])
        mode = "limits" if rng.random() < 0.6 else "early"
        tri, gate = synthetic_outcomes(rng, p, len(sel["candidates"]), mode)
        stationary = bool(rng.random() < 0.3)
        fin = ses.finish(tri, gate, stationary)
        yield dict(frame=f, table=table, keyframe=keyframe, full=full, frame_num=f + 1, time=t, draws=draws, select=sel,
                   after_select=after_select, tri=tri, gate=gate, stationary=stationary, finish=fin, after_finish=ses.state(),
                   n_kf_before_push=n_kf_before_push, empty_tail=empty_tail, walk=list(ses.walk))
        # deleteTrack: blacklisted tracks leave the table at the next update
        gone = set(fin["delete_ids"])
        tracks = [tr for tr in tracks if tr[0] not in gone or rng.random() < 0.5]
