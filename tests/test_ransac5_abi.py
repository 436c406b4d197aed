"""CPU checks of the five-point RANSAC entries (added within ABI 4): exported symbols, default parameters, the timer class
number, and the argument checks decided on the host before any device work."""
import ctypes as C

from hybvio_amd import capi


def test_ransac5_symbols_defaults_and_abi_version():
    L = capi.lib()
    for s in ("hv_ransac5_default_params", "hv_ransac5", "hv_ransac5_batch_dev", "hv_hybrid_ransac_lk_batch_dev"):
        assert hasattr(L, s), s
    p = capi.ransac5_default_params()
    assert (p.ransac5Prob, p.ransac5Threshold, p.ransacMaxIters) == (0.999, 2.0, 75)          # parameter_definitions.c:270-280
    assert (p.ransac2InliersToSkipRansac5, p.ransacMinInlierFraction, p.ransac2InliersOverRansac5Needed) == (0.9, 0.3, 0.9)
    assert L.hv_abi_version() == 4
    assert capi.K_RANSAC5 == 13 and capi.RANSAC5_MAX_ITERS == 75
    assert (capi.R5_TYPE_SKIPPED, capi.R5_TYPE_R2, capi.R5_TYPE_R5) == (0, 1, 3)


def test_ransac5_entries_reject_bad_arguments_before_any_device_work():
    L = capi.lib()
    p = capi.ransac5_default_params()
    cam = capi.camera_model("pinhole", 400.0, 400.0, 376.0, 240.0)
    xy = (C.c_float * 20)()
    st = (C.c_int * 10)()
    # no context
    assert L.hv_ransac5(None, C.byref(p), 10, xy, xy, C.byref(cam), C.byref(cam), st, None, None) == -1
    assert L.hv_ransac5_batch_dev(None, C.byref(p), 1, 10, None, None, None, C.byref(cam), C.byref(cam), None, None, None) == -1
    assert L.hv_hybrid_ransac_lk_batch_dev(None, C.byref(p), 1, 10, *([None] * 6), C.byref(cam), C.byref(cam), None, None, None,
                                           None) == -1


def test_ransac5_parameter_and_size_checks_come_before_the_context():
    """HV_ERR_UNSUPPORTED (-2) for what the kernel's LDS plan does not cover, HV_ERR_INVALID (-1) for what OpenCV asserts on;
    both decided before the context is looked at, so a NULL context still tells them apart."""
    L = capi.lib()
    cam = capi.camera_model("pinhole", 400.0, 400.0, 376.0, 240.0)
    xy = (C.c_float * 4096)()
    st = (C.c_int * 2048)()
    batch = lambda p, max_points, n_sets=1: L.hv_ransac5_batch_dev(None, C.byref(p), n_sets, max_points, None, None, None, C.byref(cam),
                                                                   C.byref(cam), None, None, None)
    hybrid = lambda p, max_points: L.hv_hybrid_ransac_lk_batch_dev(None, C.byref(p), 1, max_points, *([None] * 6), C.byref(cam),
                                                                   C.byref(cam), None, None, None, None)
    sync = lambda p, n: L.hv_ransac5(None, C.byref(p), n, xy, xy, C.byref(cam), C.byref(cam), st, None, None)
    for call in (lambda p, m: batch(p, m), hybrid, sync):
        assert call(capi.ransac5_default_params(), 1025) == -2                             # more than 1024 points
        assert call(capi.ransac5_default_params(ransacMaxIters=76), 100) == -2             # > HV_RANSAC5_MAX_ITERS
        assert call(capi.ransac5_default_params(ransacMaxIters=0), 100) == -1
        assert call(capi.ransac5_default_params(ransac5Prob=1.0), 100) == -1               # CV_Assert(confidence < 1)
        assert call(capi.ransac5_default_params(ransac5Prob=0.0), 100) == -1
        assert call(capi.ransac5_default_params(), 100) == -1                              # valid parameters, no context
    assert batch(capi.ransac5_default_params(), 100, n_sets=65536) == -2
    assert batch(capi.ransac5_default_params(), 100, n_sets=-1) == -1
    assert sync(capi.ransac5_default_params(), -1) == -1
