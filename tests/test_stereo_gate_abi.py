"""CPU checks of the stereo track gate entries (added within ABI 4): exported symbols, default parameters against
codegen/parameter_definitions.c, the timer class number, and the argument checks decided before the context is looked at."""
import ctypes as C

import numpy as np

from hybvio_amd import capi

ENTRIES = ("hv_stereo_gate_default_params", "hv_flow_status_batch_dev", "hv_track_gate", "hv_track_gate_batch_dev",
           "hv_detection_filter", "hv_detection_filter_batch_dev")


def test_stereo_gate_symbols_defaults_and_abi_version():
    L = capi.lib()
    for s in ENTRIES:
        assert hasattr(L, s), s
    p = capi.stereo_gate_default_params()
    assert p.maxStereoEpipolarDistance == 10.0                      # parameter_definitions.c:217
    assert p.partOfImageToDetectFeatures == 1.0                     # :353
    assert p.fisheyeCamera == 0 and p.independentStereoOpticalFlow == 0   # :246, :210
    assert np.array_equal(np.array(p.cam0ToCam1[:]).reshape(4, 4), np.eye(4))
    T = np.arange(16.0).reshape(4, 4)
    assert list(capi.stereo_gate_default_params(cam0ToCam1=T).cam0ToCam1) == list(T.reshape(16))   # row-major
    assert L.hv_abi_version() == 4
    assert capi.K_STEREO_GATE == 14 and capi.K_RANSAC5 == 13
    assert (capi.ST_OUT_OF_RANGE, capi.ST_FAILED_EPIPOLAR_CHECK, capi.ST_BLACKLISTED) == (5, 6, 8)


def test_stereo_gate_argument_checks_come_before_the_context():
    """HV_ERR_INVALID (-1) for NULL required arrays / parameters, negative sizes and a stereo / mono mismatch,
    HV_ERR_UNSUPPORTED (-2) for n_sets > 65535 and detection sets of more than 1024 points; all decided with a NULL context."""
    L = capi.lib()
    p = capi.stereo_gate_default_params()
    cam = capi.camera_model("pinhole", 400.0, 400.0, 376.0, 240.0)
    xy, st, bl, n = (C.c_float * 4096)(), (C.c_int32 * 2048)(), (C.c_uint8 * 2048)(), C.c_int(0)
    P, K = C.byref(p), C.byref(cam)

    flow = lambda n_sets, mp, *arrs: L.hv_flow_status_batch_dev(None, n_sets, mp, *arrs)
    assert flow(1, 10, xy, xy, bl, st) == -1                                   # valid arguments, no context
    assert flow(-1, 10, xy, xy, bl, st) == -1 and flow(1, -1, xy, xy, bl, st) == -1
    assert flow(1, 10, None, xy, bl, st) == -1 and flow(1, 10, xy, xy, bl, None) == -1
    assert flow(65536, 10, xy, xy, bl, st) == -2

    gate = lambda n, a, b, ss, c0=K, c1=K, ts=st, prm=P: L.hv_track_gate(None, prm, n, a, b, ss, None, c0, c1, ts)
    assert gate(10, xy, xy, st) == -1 and gate(10, xy, None, None) == -1          # valid stereo / mono, no context
    assert gate(-1, xy, xy, st) == -1
    assert gate(10, xy, xy, None) == -1 and gate(10, xy, None, st) == -1         # stereo / mono mismatch
    assert gate(10, None, xy, st) == -1 and gate(10, xy, xy, st, ts=None) == -1
    assert gate(10, xy, xy, st, c0=None) == -1 and gate(10, xy, xy, st, c1=None) == -1
    assert gate(10, xy, xy, st, prm=None) == -1

    gb = lambda n_sets, mp, npd=st, a=xy, b=xy, ss=st, ts=st: L.hv_track_gate_batch_dev(None, P, n_sets, mp, npd, a, b, ss, None, K, K,
                                                                                       ts, None)
    assert gb(1, 10) == -1 and gb(65536, 10) == -2 and gb(-1, 10) == -1 and gb(1, -1) == -1
    assert gb(1, 10, npd=None) == -1 and gb(1, 10, ss=None) == -1 and gb(1, 10, ts=None) == -1

    filt = lambda n, a=xy, b=xy, ss=st, oa=xy, ob=xy, no=C.byref(n): L.hv_detection_filter(None, P, n, a, b, ss, K, K, None, oa, ob, no)
    assert filt(10) == -1 and filt(1025) == -2 and filt(-1) == -1
    assert filt(10, b=None, ss=None, ob=None) == -1                               # mono, no context
    assert filt(10, ss=None) == -1 and filt(10, ob=None) == -1 and filt(10, oa=None) == -1 and filt(10, no=None) == -1

    fb = lambda n_sets, mp, npd=st, ss=st, no=st: L.hv_detection_filter_batch_dev(None, P, n_sets, mp, npd, xy, xy, ss, K, K, None, xy, xy, no)
    assert fb(1, 10) == -1 and fb(1, 1025) == -2 and fb(65536, 10) == -2 and fb(-1, 10) == -1 and fb(1, -1) == -1
    assert fb(1, 10, npd=None) == -1 and fb(1, 10, ss=None) == -1 and fb(1, 10, no=None) == -1
