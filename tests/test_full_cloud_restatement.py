"""CPU tests of tests/full_cloud_restatement.py, the yardstick of hv_full_point_cloud_dev: what fullPointCloud adds to the cloud
hv_output_dev reports, that the reference's point and status do not depend on calculateDerivatives (the ground the points-only
kernel stands on), the attempts / goodFrame rule, and that the generated corpus holds the cases it is there for and keeps the
exclusion cap of the GPU test."""
import numpy as np
import pytest

import full_cloud_restatement as F
import output_restatement as OR
import trail_index_restatement as T

SMALL = ("stereo_gap", "mono_all", "trail24_depth")
EXCLUSION_CAP = 0.01                                            # of the tail tracks of the corpus: the two precisions disagree


def _records(name):
    c = F.corpus(name)
    for f, row in enumerate(c["frames"]):
        for s, rec in enumerate(row):
            if rec["judged"]:
                yield c, f, s, rec


def _output_cloud(c, rec):
    """The cloud hv_output_dev reports on the same outcomes: [(candidate, PointFeature::Status)]."""
    status = list(zip(rec["tri"], rec["prep"]))
    return OR.pointCloud(status, rec["gate"], rec["n_cand"], c["V"], c["p"].maxSuccessfulVisualUpdates)


@pytest.mark.parametrize("name", list(F.CASES))
def test_the_prefix_is_the_output_stages_cloud_plus_the_stopping_candidate(name):
    never, stopped, with_stopping_point = 0, 0, 0
    for c, f, s, rec in _records(name):
        if not rec["ready"]:
            assert rec["rest"]["cloud"] == [] and (not rec["rest"]["stopped"] or rec["rest"]["n_attempts"] > 0)
            continue
        walk_ids = {arg: rec["ids"][pos] for pos, (kind, arg) in enumerate(rec["walk"]) if kind == "candidate"}
        base = [(walk_ids[v], st) for v, st in _output_cloud(c, rec)]
        got = [(tid, st) for tid, st, _, _ in rec["rest"]["cloud"]]
        n_tail_ok = sum(st == F.TRI_OK for _, st, _ in rec["rest"]["tail"])
        prefix = got[:len(got) - n_tail_ok]
        if not rec["rest"]["stopped"]:                           # a loop that never stopped has no tail: exactly today's cloud
            never += 1
            assert rec["rest"]["tail"] == [] and got == base, (name, f, s)
            continue
        stopped += 1
        visited = [v for v in range(rec["n_cand"]) if rec["tri"][v] != T.TRI_NOT_VISITED]
        stop = visited[-1]                                       # synthetic_outcomes visits nothing behind the stop
        extra = []
        if rec["tri"][stop] == F.TRI_OK:
            extra = [(walk_ids[stop], F.POINT_OUTLIER if rec["prep"][stop] == 0 and rec["gate"][stop] != T.INLIER else F.POINT_POSE_TRAIL)]
            with_stopping_point += 1
        assert prefix == base + extra, (name, f, s, prefix, base, extra)
        # the tail's points: POSE_TRAIL, in tail order, with the head's corner of the track
        assert [tid for tid, _ in got[len(prefix):]] == [tid for tid, st, _ in rec["rest"]["tail"] if st == F.TRI_OK]
        assert all(st == F.POINT_POSE_TRAIL for _, st in got[len(prefix):])
        corner = {t[0]: t[1] for t in rec["table"]}
        for tid, _, px, _ in rec["rest"]["cloud"]:
            assert px.dtype == np.float32 and tuple(px) == tuple(corner[tid]), (name, f, s, tid)
    assert stopped > 0 and with_stopping_point > 0
    if F.CASES[name][0] == 5:
        assert never > 0


@pytest.mark.parametrize("name", list(F.CASES))
def test_point_and_status_do_not_depend_on_calculate_derivatives(name):
    """Bit-equal pf and equal status with and without the derivative code, on every tail track the derivative run covers."""
    compared = 0
    for c, f, s, rec in _records(name):
        a, b = rec["rest"], rec["rest_d"]
        assert [(t, st) for t, st, _ in a["tail"]] == [(t, st) for t, st, _ in b["tail"]], (name, f, s)
        assert len(a["cloud"]) == len(b["cloud"])
        for (ta, sa, _, pa), (tb, sb, _, pb) in zip(a["cloud"], b["cloud"]):
            assert (ta, sa) == (tb, sb) and np.array(pa, np.float64).tobytes() == np.array(pb, np.float64).tobytes(), (name, f, s, ta)
        compared += len(a["tail"])
    assert compared > 50, compared


def test_attempts_and_good_frame_include_the_tail():
    """updateAttemptCount counts every triangulated track (:1121), so tooManyFailures (:1273) sees the tail: frames that finish()
    calls good turn bad through the tail alone; a loop that never stopped reports finish()'s own figures."""
    turned, same = 0, 0
    for name in SMALL:
        for c, f, s, rec in _records(name):
            r, fin = rec["rest"], rec["finish"]
            visits = sum(x != T.TRI_NOT_VISITED for x in rec["tri"])
            assert r["n_attempts"] == visits + len(r["tail"]) and r["successes"] == fin["successes"], (name, f, s)
            failures = r["n_attempts"] - r["successes"]
            assert r["good_frame"] == ((rec["stationary"] or r["stopped"]) and not failures > T.FAILED_UPDATES_THRESHOLD)
            if not r["tail"]:
                assert (r["n_attempts"], r["good_frame"]) == (fin["attempts"], fin["good_frame"]), (name, f, s)
                same += 1
            turned += bool(fin["good_frame"] and not r["good_frame"])
    assert turned > 0 and same > 0, (turned, same)


def test_the_corpus_contains_the_cases_it_is_there_for():
    seen = dict(statuses=set(), outlier_stop=0, no_tracks=0, one_track=0, not_full=0, never=0, not_ready_tail=0, black_before=0,
                black_behind=0, over_64=0, full_length=0, popped=0, unvisited_candidate_in_tail=0)
    for name in F.CASES:
        S, M, trail, V, succ, stereo, sampling, frames, over = F.CASES[name]
        for c, f, s, rec in _records(name):
            r = rec["rest"]
            seen["statuses"] |= {st for _, st, _ in r["tail"]}
            seen["no_tracks"] += len(rec["table"]) == 0
            seen["one_track"] += len(rec["table"]) == 1
            seen["not_full"] += not rec["full"]
            seen["popped"] += not rec["keyframe"]
            seen["never"] += not r["stopped"] and rec["n_cand"] > 0
            seen["not_ready_tail"] += (not rec["ready"]) and len(r["tail"]) > 0
            seen["over_64"] += len(r["tail"]) > 64
            seen["full_length"] += any(len(index) == trail + 1 for _, _, index in r["tail"])
            visited = [v for v in range(rec["n_cand"]) if rec["tri"][v] != T.TRI_NOT_VISITED]
            if r["stopped"]:
                stop = visited[-1]
                seen["outlier_stop"] += rec["tri"][stop] == F.TRI_OK and rec["prep"][stop] == 0 and rec["gate"][stop] != T.INLIER
                stop_pos = rec["cand_pos"][stop]
                tail_ids = {t for t, _, _ in r["tail"]}
                for pos, (kind, arg) in enumerate(rec["walk"]):
                    if kind == "blacklisted":
                        seen["black_before"] += pos < stop_pos
                        seen["black_behind"] += pos > stop_pos and rec["ids"][pos] in tail_ids
                    if kind == "candidate" and pos > stop_pos:
                        seen["unvisited_candidate_in_tail"] += rec["ids"][pos] in tail_ids
    assert {F.TRI_OK, F.TRI_BEHIND, F.TRI_BAD_COND, F.TRI_NO_CONVERGENCE, F.TRI_BAD_DEPTH} <= seen["statuses"], seen["statuses"]
    seen.pop("statuses")
    assert all(v > 0 for v in seen.values()), seen


def test_the_corpus_keeps_the_exclusion_cap():
    """tail_status is compared wherever the oracle's binary64 and long-double builds agree; the tracks on which they disagree are
    left out, judged by the reference alone -- at most 1 % of the tail tracks of the corpus."""
    total = disagree = 0
    for name in F.CASES:
        for c, f, s, rec in _records(name):
            for (ta, sa, _), (tb, sb, _) in zip(rec["rest"]["tail"], rec["truth"]["tail"]):
                assert ta == tb
                total += 1
                disagree += sa != sb
    print(f"{disagree} of {total} tail tracks: the two precisions disagree")
    assert total > 1000 and disagree <= EXCLUSION_CAP * total, (disagree, total)
