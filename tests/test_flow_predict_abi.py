"""CPU checks of the device optical-flow predictor entry (added within ABI 4): exported symbols, default parameters against
codegen/parameter_definitions.c:213 and backend.cpp:627, the enum, the struct against the header, and the argument checks, all of
which are decided with a NULL handle."""
import ctypes as C
import os
import re

import numpy as np

from hybvio_amd import capi

ENTRIES = ("hv_flow_predict_default_params", "hv_flow_predict_batch_dev")
TRAIL_MEMBERS = [k for k, _ in capi.TrailIndexTable._fields_]
FIELDS = ["predictOpticalFlowMinTriangulationDistance", "minBaselinePoses", "imuToCamera", "secondImuToCamera", "cameraToImu",
          "secondCameraToImu"]


def _header():
    return open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "hybvio_hip.h")).read()


def test_flow_predict_symbols_defaults_enum_and_struct():
    L = capi.lib()
    for s in ENTRIES:
        assert hasattr(L, s) and s in capi.PROTOTYPES, s
    p = capi.flow_predict_default_params()
    assert p.predictOpticalFlowMinTriangulationDistance == 3.0                       # parameter_definitions.c:213
    assert p.minBaselinePoses == 10                                                  # backend.cpp:627
    for k in FIELDS[2:]:
        assert np.array_equal(np.array(getattr(p, k)[:]).reshape(4, 4), np.eye(4)), k
    T = np.array([[0.0, -1.0, 0.0, 0.1], [1.0, 0.0, 0.0, -0.2], [0.0, 0.0, 1.0, 0.3], [0.0, 0.0, 0.0, 1.0]])
    q = capi.flow_predict_default_params(T, minBaselinePoses=4)
    assert q.minBaselinePoses == 4 and np.array_equal(np.array(q.imuToCamera[:]).reshape(4, 4), T)
    assert np.allclose(np.array(q.cameraToImu[:]).reshape(4, 4) @ T, np.eye(4), atol=1e-15)
    assert np.array_equal(np.array(q.secondCameraToImu[:]).reshape(4, 4), np.eye(4))
    assert (capi.FLOW_PREDICT_LEFT, capi.FLOW_PREDICT_RIGHT, capi.FLOW_PREDICT_STEREO) == (0, 1, 2)
    assert L.hv_abi_version() == 4 and capi.K_TRAIL_INDEX == 19
    header = _header()
    assert re.search(r"HV_FLOW_PREDICT_LEFT = 0, HV_FLOW_PREDICT_RIGHT = 1, HV_FLOW_PREDICT_STEREO = 2\b", header)
    assert re.search(r"HV_K_COUNT = 20\b", header)
    body = header[header.index("typedef struct hv_flow_predict_params {"):header.index("} hv_flow_predict_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[16\])?\s*[,;]", body)
    assert names == FIELDS and [k for k, _ in capi.FlowPredictParams._fields_] == FIELDS
    assert re.findall(r"(double|int)\s+\w+", body) == ["double", "int", "double", "double"]
    assert C.sizeof(capi.FlowPredictParams) == 8 + 8 + 4 * 16 * 8                    # the int is padded to the doubles' alignment


def test_flow_predict_argument_checks_need_no_handle():
    """HV_ERR_INVALID (-1): a NULL required pointer (a state member included), a type outside 0 .. 2, reuse_distance without
    distance_dev, a NULL camera1 for RIGHT / STEREO, minBaselinePoses < 1, the parameter ranges of the trail entries.
    HV_ERR_UNSUPPORTED (-2): maxTracks > HV_TRACKS_MAX_TRACKS, maxSize > HV_TRAIL_MAX_POSES. Invalid wins. Valid arguments give
    HV_ERR_INVALID for the NULL handle itself."""
    L = capi.lib()
    buf = (C.c_double * 4096)()
    a = C.addressof(buf)
    cam = capi.camera_model("pinhole", 400.0, 400.0, 376.0, 240.0)

    def trail(**over):
        m = {k: a for k in TRAIL_MEMBERS}
        m.update(over)
        return capi.TrailIndexTable(*(m[k] or None for k in TRAIL_MEMBERS))

    FP, TP, TR = capi.flow_predict_default_params(), capi.trail_index_default_params(), trail()
    TT = capi.track_table(n_tracks=a, ids=a, xy=a, second_xy=a)

    def call(p=FP, kind=0, tp=TP, t=TR, table=TT, c0=a, cam0=cam, cam1=cam, pred=a, dist=a, reuse=0):
        return L.hv_flow_predict_batch_dev(None, C.byref(p) if p else None, kind, C.byref(tp) if tp else None, C.byref(t) if t else None,
                                           C.byref(table) if table else None, C.c_void_p(c0 or None), C.addressof(cam0) if cam0 else None,
                                           C.addressof(cam1) if cam1 else None, C.c_void_p(pred or None), C.c_void_p(dist or None), reuse)

    big = capi.trail_index_default_params(maxTracks=capi.TRACKS_MAX_TRACKS + 1)
    long_trail = capi.trail_index_default_params(cameraTrailLength=capi.TRAIL_MAX_POSES)
    for kind in (0, 1, 2):
        assert call(kind=kind) == -1 and call(kind=kind, dist=0) == -1 and call(kind=kind, reuse=1) == -1    # valid: the NULL handle
        assert call(kind=kind, tp=big) == -2 and call(kind=kind, tp=long_trail) == -2
        assert call(kind=kind, tp=capi.trail_index_default_params(maxTracks=capi.TRACKS_MAX_TRACKS, cameraTrailLength=capi.TRAIL_MAX_POSES - 1)) == -1
    invalid = [dict(p=None), dict(tp=None), dict(t=None), dict(table=None), dict(c0=0), dict(cam0=None), dict(pred=0), dict(kind=-1),
               dict(kind=3), dict(dist=0, reuse=1), dict(kind=1, cam1=None), dict(kind=2, cam1=None),
               dict(p=capi.flow_predict_default_params(minBaselinePoses=0)), dict(tp=capi.trail_index_default_params(maxTracks=0)),
               dict(tp=capi.trail_index_default_params(cameraTrailLength=0)), dict(tp=capi.trail_index_default_params(trackSampling=3)),
               dict(table=capi.track_table(ids=a, xy=a)), dict(table=capi.track_table(n_tracks=a, xy=a))]
    invalid += [dict(t=trail(**{k: 0})) for k in TRAIL_MEMBERS]
    for bad in invalid:
        assert call(**bad) == -1, bad
        if "tp" not in bad:
            assert call(**{**bad, "tp": big}) == -1 and call(**{**bad, "tp": long_trail}) == -1, bad     # invalid wins over unsupported
    assert call(cam1=None) == -1 and call(cam1=None, tp=big) == -2                  # LEFT does not need the second camera
    assert call(table=capi.track_table(n_tracks=a, ids=a), tp=big) == -2            # xy / second_xy are not read: c0_dev is
    assert call(dist=0, tp=big) == -2                                               # distance_dev is optional
