"""CPU checks of the resident VIO engine's C ABI (hv_vio_*, added within ABI 4): exported symbols, the defaults of
hv_vio_default_params member for member against the owned entries' own default functions, the member order of hv_vio_params and
hv_vio_view against the header, every refusal hv_vio_create decides before the context is looked at (made with a NULL context,
which is itself the last refusal), and what must not have changed (ABI 4, HV_K_COUNT = 20)."""
import ctypes as C
import os
import re

from hybvio_amd import capi

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "hybvio_hip.h")
INVALID, UNSUPPORTED = -1, -2


def _bytes(s):
    return bytes(memoryview(s))


def _struct_members(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = decl.split(",")
        names.append(re.findall(r"\*?\s*(\w+)\s*(?:\[\d+\])?$", first.strip())[0])
        names += [r.strip().lstrip("*").strip() for r in rest]
    return names


def test_symbols_and_unchanged_abi():
    L = capi.lib()
    text = open(HEADER).read()
    for s in ("hv_vio_default_params", "hv_vio_create", "hv_vio_destroy", "hv_vio_frame", "hv_vio_view_get", "hv_vio_replay_period",
              "hv_vio_sets"):
        assert hasattr(L, s) and s in capi.PROTOTYPES and re.search(r"\b%s\(" % s, text), s
    assert L.hv_abi_version() == 4 and "HV_K_COUNT = 20 }" in text
    assert L.hv_vio_replay_period(None) == INVALID and L.hv_vio_sets(None) == INVALID
    assert L.hv_vio_view_get(None, C.byref(capi.VioView())) == INVALID
    assert L.hv_vio_frame(None, 16, 16, 64, 8, 1, 16, 16, 16) == INVALID
    L.hv_vio_destroy(None)                                           # a no-op


def test_defaults_are_those_of_the_owned_entries_member_for_member():
    L = capi.lib()
    p = capi.vio_default_params()
    own = dict(ekf=(capi.EkfParams, "hv_ekf_default_params"), gftt=(capi.GfttParams, "hv_gftt_default_params"),
               subpix=(capi.SubpixParams, "hv_subpix_default_params"), gate=(capi.StereoGateParams, "hv_stereo_gate_default_params"),
               ransac3=(capi.Ransac3Params, "hv_ransac3_default_params"), tracks=(capi.TrackTableParams, "hv_track_table_default_params"),
               trail=(capi.TrailIndexParams, "hv_trail_index_default_params"), flow=(capi.FlowPredictParams, "hv_flow_predict_default_params"),
               vu=(capi.VuParams, "hv_vu_default_params"), control=(capi.EkfControlParams, "hv_ekf_control_default_params"),
               session=(capi.SessionParams, "hv_session_default_params"), output=(capi.OutputParams, "hv_output_default_params"))
    for member, (cls, fn) in own.items():
        d = cls()
        getattr(L, fn)(C.byref(d))
        got = getattr(p, member)
        for name, _ in cls._fields_:
            a, b = getattr(got, name), getattr(d, name)
            assert (list(a) == list(b)) if isinstance(a, C.Array) else (a == b), (member, name)
    assert (p.ransac2Threshold, p.trackChiTestOutlierR, p.visualR) == (4.0, 1.5, 0.05)
    assert (p.ransacRngSeed, p.odometryRngSeed, p.imu_samples_max) == (4649, 0, 32)
    assert (p.featureDetector, p.useRansac3, p.predictOpticalFlow, p.batchVisualUpdate) == (capi.DETECTOR_GPU_GFTT, 1, 1, 0)
    assert _bytes(p.camera0) == _bytes(capi.CameraModel()) and _bytes(p.camera1) == _bytes(capi.CameraModel())
    L.hv_vio_default_params(None)                                    # a no-op


def test_member_order_matches_the_header():
    text = open(HEADER).read()
    assert _struct_members(text, "hv_vio_params") == [k for k, _ in capi.VioParams._fields_]
    assert _struct_members(text, "hv_vio_view") == [k for k, _ in capi.VioView._fields_]
    assert "#define HV_EKF_MAX_PREDICT_SAMPLES 32" in text


def _create(p, n_sets=2, out=True, ctx=None):
    h = C.c_void_p()
    return capi.lib().hv_vio_create(ctx, C.byref(p) if p is not None else None, n_sets, C.byref(h) if out else None)


def test_create_refuses_before_the_device_is_touched():
    ok = capi.vio_default_params
    assert _create(ok()) == INVALID                                  # all parameters good: the NULL context itself, decided last
    assert _create(None) == INVALID and _create(ok(), out=False) == INVALID
    assert _create(ok(), n_sets=0) == INVALID and _create(ok(), n_sets=-1) == INVALID
    for bad in (dict(imu_samples_max=0), dict(imu_samples_max=33), dict(tracks__maxTracks=100), dict(trail__maxTracks=100),
                dict(gftt__maxTracks=100), dict(output__maxTracks=100), dict(ekf__cameraTrailLength=10), dict(output__cameraTrailLength=10),
                dict(output__maxVisualUpdates=10), dict(output__maxSuccessfulVisualUpdates=3),
                dict(trail__useStereo=0), dict(output__useStereo=0),                              # the index and the output disagree about stereo
                dict(session__visualUpdateForEveryNFrame=0)):
        assert _create(ok(**bad)) == INVALID, bad
    # everything outside the default stereo session
    for bad in (dict(trail__useStereo=0, output__useStereo=0),                                    # mono
                dict(featureDetector=capi.DETECTOR_FAST), dict(featureDetector=capi.DETECTOR_GFTT), dict(useRansac3=0),
                dict(gate__independentStereoOpticalFlow=1), dict(predictOpticalFlow=0), dict(batchVisualUpdate=1),
                dict(trail__fullPointCloud=1), dict(ekf__hybridMapSize=4), dict(ransac3__ransac3MaxIterations=capi.RNG_MAX_DRAWS)):
        assert _create(ok(**bad)) == UNSUPPORTED, bad
    assert _create(ok(), n_sets=65536) == UNSUPPORTED and _create(ok(), n_sets=65535) == INVALID
    # an invalid argument is reported before an unsupported one
    assert _create(ok(useRansac3=0, imu_samples_max=0)) == INVALID
    # a consistent non-default size passes every check but the NULL context
    assert _create(ok(tracks__maxTracks=120, trail__maxTracks=120, gftt__maxTracks=120, output__maxTracks=120)) == INVALID
