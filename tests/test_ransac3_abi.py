"""C ABI of the stereo RANSAC3 entry points (no GPU needed: symbols, defaults, and the argument checks that come before any
device work)."""
import ctypes as C

import numpy as np

from hybvio_amd import capi


def test_ransac3_symbols_defaults_and_abi_version():
    L = capi.lib()
    for s in ("hv_ransac3_default_params", "hv_ransac3", "hv_ransac3_batch_dev", "hv_ransac3_lk_batch_dev"):
        assert hasattr(L, s), s
    p = capi.ransac3_default_params()
    assert (p.ransac3ErrorThresh, p.ransac3FailureProbability, p.ransac3MaxIterations, p.ransac3MinIterations, p.ransac3UseMle,
            p.ransacMinInlierFraction) == (1e-4, 1e-4, 500, 50, 1, 0.3)          # parameter_definitions.c:282, 292-296
    assert L.hv_abi_version() == 4
    assert capi.K_RANSAC3 == 17 and capi.RANSAC3_MAX_ITERS == 500 and capi.K_TRACK_TABLE == 16
    assert L.hv_profile_read(None, capi.K_RANSAC3, None, None) == -1             # (no context; the id itself is in range)


def _calls():
    L = capi.lib()
    cam = capi.camera_model("pinhole", 400.0, 400.0, 376.0, 240.0)
    xy = np.zeros((10, 2), np.float32).ctypes.data_as(C.c_void_p)
    st = np.zeros(10, np.int32).ctypes.data_as(C.c_void_p)
    T = np.eye(4).reshape(16).ctypes.data_as(C.c_void_p)
    dr = np.zeros(1500, np.uint32).ctypes.data_as(C.c_void_p)
    cb = C.byref(cam)
    batch = lambda p, max_points, n_sets=1: L.hv_ransac3_batch_dev(None, C.byref(p), n_sets, max_points, None, None, None, None, cb, cb,
                                                                   T, None, None, None, None)
    chain = lambda p, max_points, n_sets=1: L.hv_ransac3_lk_batch_dev(None, C.byref(p), n_sets, max_points, None, None, None, None,
                                                                      None, None, cb, cb, T, None, None, None, None, None)
    sync = lambda p, n: L.hv_ransac3(None, C.byref(p), n, xy, xy, xy, cb, cb, T, dr, st, None, None)
    return batch, chain, sync


def test_ransac3_parameter_and_size_checks_come_before_the_context():
    batch, chain, sync = _calls()
    dp = capi.ransac3_default_params
    for call in (batch, chain, sync):
        assert call(dp(), 1025) == -2                                              # more than 1024 points
        assert call(dp(ransac3MaxIterations=501), 100) == -2                       # > HV_RANSAC3_MAX_ITERS
        assert call(dp(ransac3MaxIterations=0, ransac3MinIterations=0), 100) == -1
        assert call(dp(ransac3MinIterations=501), 100) == -1                       # min > max
        assert call(dp(ransac3FailureProbability=0.0), 100) == -1
        assert call(dp(ransac3FailureProbability=1.0), 100) == -1
        assert call(dp(ransac3ErrorThresh=0.0), 100) == -1
        assert call(dp(ransac3ErrorThresh=-1.0), 100) == -1
        assert call(dp(ransacMinInlierFraction=-0.1), 100) == -1
        assert call(dp(ransacMinInlierFraction=1.1), 100) == -1
        assert call(dp(ransacMinInlierFraction=float("nan")), 100) == -1
        assert call(dp(), 100) == -1                                               # valid parameters, no context
    assert batch(dp(), 100, n_sets=65536) == -2 and chain(dp(), 100, n_sets=65536) == -2
    assert batch(dp(), 100, n_sets=-1) == -1 and chain(dp(), 100, n_sets=-1) == -1
    assert sync(dp(), -1) == -1
    L = capi.lib()
    assert L.hv_ransac3_batch_dev(None, None, 1, 10, None, None, None, None, None, None, None, None, None, None, None) == -1
