"""CPU checks of the device pose-trail index entries (added within ABI 4): exported symbols, default parameters against
codegen/parameter_definitions.c, the timer class number, and the argument checks decided before the context is looked at."""
import ctypes as C
import os
import re

from hybvio_amd import capi

ENTRIES = ("hv_trail_index_default_params", "hv_trail_init_batch_dev", "hv_trail_select_batch_dev", "hv_trail_finish_batch_dev")
MEMBERS = ("n_keyframes", "frame_counter", "kf_row", "frame_number", "timestamp", "col_id", "col_len", "image_point", "norm_point",
           "norm_velocity", "used", "n_blacklist", "blacklist_ids", "n_order", "n_skipped", "skipped_pos", "skipped_id", "cand_pos",
           "cand_col")
DEFAULTS = dict(cameraTrailLength=20, cameraTrailHanoiLength=3, cameraTrailStridedLength=0, cameraTrailStridedStride=2,
                cameraTrailFixedScheme=0, trackSampling=0, trackMinFrames=4, scoreVisualUpdateTracks=1, blacklistTracks=1,
                maxVisualUpdates=20, maxSuccessfulVisualUpdates=5, estimateImuCameraTimeShift=1, useStereo=1, maxTracks=200,
                hybridMapSize=0, useIndependentStereoTriangulation=0, fullPointCloud=0)


def test_trail_index_symbols_defaults_and_abi_version():
    L = capi.lib()
    for s in ENTRIES:
        assert hasattr(L, s) and s in capi.PROTOTYPES, s
    p = capi.trail_index_default_params()
    assert {k: getattr(p, k) for k, _ in capi.TrailIndexParams._fields_} == DEFAULTS
    assert capi.trail_index_default_params(maxTracks=64).maxTracks == 64
    assert L.hv_abi_version() == 4
    assert capi.K_TRAIL_INDEX == 19 and capi.K_EKF_CONTROL == 18
    assert [k for k, _ in capi.TrailIndexTable._fields_] == list(MEMBERS)
    assert (capi.TRACK_SAMPLING_GAP, capi.TRACK_SAMPLING_ALL, capi.TRACK_SAMPLING_RANDOM) == (0, 1, 2)
    header = open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "hybvio_hip.h")).read()
    assert re.search(r"HV_K_TRAIL_INDEX = 19\b", header) and re.search(r"HV_K_COUNT = 20\b", header)
    assert re.search(r"#define HV_TRAIL_MAX_POSES %d\b" % capi.TRAIL_MAX_POSES, header)
    assert re.search(r"#define HV_TRAIL_MAX_VISITS %d\b" % capi.TRAIL_MAX_VISITS, header)
    # the struct members of the header, in order
    body = header[header.index("typedef struct hv_trail_index {"):header.index("} hv_trail_index;")]
    assert re.findall(r"\*(\w+);", body) == list(MEMBERS)
    body = header[header.index("typedef struct hv_trail_index_params {"):header.index("} hv_trail_index_params;")]
    assert re.findall(r"int (\w+);", body) == [k for k, _ in capi.TrailIndexParams._fields_]
    ms, launches = C.c_double(), C.c_longlong()
    assert L.hv_profile_read(None, capi.K_TRAIL_INDEX, C.byref(ms), C.byref(launches)) == -1      # NULL handle


def test_trail_index_argument_checks_come_before_the_context():
    """HV_ERR_INVALID (-1) for a NULL required pointer (a state member included), a negative size and the parameter ranges the
    reference asserts; HV_ERR_UNSUPPORTED (-2) for what the device form leaves out; all decided with a NULL context, where valid
    arguments give HV_ERR_INVALID for the context itself. A call that is both invalid and unsupported is invalid."""
    L = capi.lib()
    buf = (C.c_double * 4096)()
    a = C.addressof(buf)
    v = C.c_void_p
    cam = capi.camera_model("pinhole", 400.0, 400.0, 376.0, 240.0)

    def trail(**over):
        m = {k: a for k in MEMBERS}
        m.update(over)
        return capi.TrailIndexTable(*(m[k] or None for k in MEMBERS))

    def prm(**over):
        return capi.trail_index_default_params(**over)

    TT = capi.track_table(n_tracks=a, ids=a, xy=a, second_xy=a)
    P, TR = prm(), trail()

    def init(n_sets=1, p=P, t=TR):
        return L.hv_trail_init_batch_dev(None, C.byref(p) if p else None, n_sets, C.byref(t) if t else None)

    def sel(n_sets=1, p=P, t=TR, table=TT, cam0=cam, cam1=cam, full=a, **over):
        names = ("keyframe", "frame_num", "time", "draws", "draws_used", "n_poses", "pose_index", "features", "velocities", "y", "cand_id",
                 "n_cand")
        x = {k: a for k in names}
        x.update(over)
        return L.hv_trail_select_batch_dev(None, C.byref(p) if p else None, n_sets, C.byref(t) if t else None,
                                           C.byref(table) if table else None, C.addressof(cam0) if cam0 else None,
                                           C.addressof(cam1) if cam1 else None, v(x["keyframe"] or None), v(full or None),
                                           *(v(x[k] or None) for k in names[1:]))

    def fin(n_sets=1, p=P, t=TR, stationary=a, good=a, attempts=a, success=a, **over):
        names = ("cand_id", "n_cand", "status", "gate", "delete_ids", "n_delete", "discarded")
        x = {k: a for k in names}
        x.update(over)
        return L.hv_trail_finish_batch_dev(None, C.byref(p) if p else None, n_sets, C.byref(t) if t else None, v(x["cand_id"] or None),
                                           v(x["n_cand"] or None), v(x["status"] or None), v(x["gate"] or None), v(stationary or None),
                                           v(x["delete_ids"] or None), v(x["n_delete"] or None), v(good or None), v(attempts or None),
                                           v(success or None), v(x["discarded"] or None))

    for call in (init, sel, fin):
        assert call() == -1                                                          # valid, no context
        assert call(p=None) == -1 and call(t=None) == -1 and call(n_sets=-1) == -1
        for bad in (dict(maxTracks=0), dict(cameraTrailLength=0), dict(cameraTrailHanoiLength=-1), dict(cameraTrailStridedLength=-1),
                    dict(cameraTrailHanoiLength=20), dict(cameraTrailHanoiLength=10, cameraTrailStridedLength=9),
                    dict(cameraTrailStridedLength=2, cameraTrailStridedStride=0), dict(trackSampling=3), dict(trackSampling=-1)):
            assert call(p=prm(**bad)) == -1, bad
        assert call(p=prm(cameraTrailHanoiLength=19)) == -1                          # 19 + 0 + 1 < 21: valid, no context
        for unsupported in (dict(maxTracks=1025), dict(maxVisualUpdates=0), dict(maxVisualUpdates=65), dict(trackSampling=2),
                            dict(hybridMapSize=2), dict(useIndependentStereoTriangulation=1), dict(fullPointCloud=1),
                            dict(cameraTrailLength=64)):
            assert call(p=prm(**unsupported)) == -2, unsupported
            assert call(p=prm(**unsupported), t=trail(col_len=0)) == -1, unsupported     # the NULL member is reported first
        assert call(n_sets=65536) == -2 and call(p=prm(maxTracks=1024, maxVisualUpdates=64, cameraTrailLength=63)) == -1
        for k in MEMBERS:
            assert call(t=trail(**{k: 0})) == -1 and call(n_sets=65536, t=trail(**{k: 0})) == -1, k

    for k in ("keyframe", "frame_num", "time", "draws", "draws_used", "n_poses", "pose_index", "features", "velocities", "y", "cand_id", "n_cand"):
        assert sel(**{k: 0}) == -1 and sel(n_sets=65536, **{k: 0}) == -1, k
    assert sel(full=0) == -1                                                         # optional
    assert sel(table=None) == -1 and sel(cam0=None) == -1 and sel(cam1=None) == -1
    assert sel(p=prm(maxTracks=1025), cam1=None) == -1 and sel(p=prm(maxTracks=1025, useStereo=0), cam1=None) == -2
    mono = capi.track_table(n_tracks=a, ids=a, xy=a)
    assert sel(table=mono) == -1 and sel(p=prm(maxTracks=1025), table=mono) == -1
    assert sel(p=prm(maxTracks=1025, useStereo=0), table=mono) == -2
    for k in ("n_tracks", "ids", "xy"):
        assert sel(p=prm(maxTracks=1025), table=capi.track_table(**{**dict(n_tracks=a, ids=a, xy=a, second_xy=a), k: 0})) == -1, k

    for k in ("cand_id", "n_cand", "status", "gate", "delete_ids", "n_delete", "discarded"):
        assert fin(**{k: 0}) == -1 and fin(p=prm(trackSampling=2), **{k: 0}) == -1, k
    assert fin(stationary=0, good=0, attempts=0, success=0) == -1                    # the optional ones
    assert fin(p=prm(trackSampling=2), stationary=0, good=0, attempts=0, success=0) == -2
