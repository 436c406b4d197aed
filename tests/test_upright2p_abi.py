"""C ABI of the stereo upright 2-point entry points (no GPU needed: symbols, defaults, and the argument checks that come before
any device work)."""
import ctypes as C

import numpy as np

from hybvio_amd import capi


def test_upright2p_symbols_defaults_and_abi_version():
    L = capi.lib()
    for s in ("hv_upright2p_default_params", "hv_upright2p", "hv_upright2p_batch_dev", "hv_upright2p_lk_batch_dev"):
        assert hasattr(L, s), s
    p = capi.upright2p_default_params()
    assert (p.ransacStereoUpright2pErrorThresh, p.ransacStereoUpright2pFailureProbability, p.ransacStereoUpright2pMaxIterations,
            p.ransacStereoUpright2pMinIterations, p.ransacStereoUpright2pUseMle, p.ransacMinInlierFraction) == (1e-4, 1e-4, 500, 50, 1, 0.3)
    assert L.hv_abi_version() == 4                                               # parameter_definitions.c:282, 299-303
    assert capi.K_RANSAC3 == 17 and capi.UPRIGHT2P_MAX_ITERS == 500 and capi.U2_TYPE_UPRIGHT_2P == 4
    assert capi.upright2p_default_params(ransacStereoUpright2pUseMle=0).ransacStereoUpright2pUseMle == 0
    for name in ("upright2p", "upright2p_batch_dev"):
        assert callable(getattr(capi.Context, name))
    assert callable(capi.EkfBatch.upright2p_lk_batch_dev)


def _calls():
    L = capi.lib()
    cam = capi.camera_model("pinhole", 400.0, 400.0, 376.0, 240.0)
    xy = np.zeros((10, 2), np.float32).ctypes.data_as(C.c_void_p)
    st = np.zeros(10, np.int32).ctypes.data_as(C.c_void_p)
    T = np.eye(4).reshape(16).ctypes.data_as(C.c_void_p)
    P = np.concatenate([np.eye(4).reshape(16)] * 2).ctypes.data_as(C.c_void_p)
    dr = np.zeros(1000, np.uint32).ctypes.data_as(C.c_void_p)
    par = capi.flow_predict_default_params()
    cb = C.byref(cam)
    batch = lambda p, max_points, n_sets=1: L.hv_upright2p_batch_dev(None, C.byref(p), n_sets, max_points, None, None, None, None, cb, cb,
                                                                     T, None, None, None, None, None)
    chain = lambda p, max_points: L.hv_upright2p_lk_batch_dev(None, C.byref(p), C.byref(par), max_points, st, xy, xy, xy, st, st, cb, cb, T,
                                                              dr, st, st, None, None)
    sync = lambda p, n: L.hv_upright2p(None, C.byref(p), n, xy, xy, xy, cb, cb, T, P, dr, st, None, None)
    return batch, chain, sync, (cb, T, par, xy, st, dr)


def test_upright2p_parameter_and_size_checks_come_before_the_context():
    batch, chain, sync, (cb, T, par, xy, st, dr) = _calls()
    dp = capi.upright2p_default_params
    for call in (batch, chain, sync):
        assert call(dp(), 1025) == -2                                              # more than 1024 points
        assert call(dp(ransacStereoUpright2pMaxIterations=501), 100) == -2         # > HV_UPRIGHT2P_MAX_ITERS
        assert call(dp(ransacStereoUpright2pMaxIterations=0, ransacStereoUpright2pMinIterations=0), 100) == -1
        assert call(dp(ransacStereoUpright2pMinIterations=501), 100) == -1         # min > max
        assert call(dp(ransacStereoUpright2pFailureProbability=0.0), 100) == -1
        assert call(dp(ransacStereoUpright2pFailureProbability=1.0), 100) == -1
        assert call(dp(ransacStereoUpright2pErrorThresh=0.0), 100) == -1
        assert call(dp(ransacStereoUpright2pErrorThresh=-1.0), 100) == -1
        assert call(dp(ransacMinInlierFraction=-0.1), 100) == -1
        assert call(dp(ransacMinInlierFraction=1.1), 100) == -1
        assert call(dp(ransacMinInlierFraction=float("nan")), 100) == -1
        assert call(dp(), 100) == -1                                               # valid parameters, no context / no filter handle
    assert batch(dp(), 100, n_sets=65536) == -2 and batch(dp(), 100, n_sets=-1) == -1
    assert sync(dp(), -1) == -1
    L = capi.lib()
    assert L.hv_upright2p_batch_dev(None, None, 1, 10, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    # the chain entry: a NULL required pointer is refused like a NULL handle, and the size check still comes first
    p = dp()
    assert L.hv_upright2p_lk_batch_dev(None, C.byref(p), None, 100, st, xy, xy, xy, st, st, cb, cb, T, dr, st, st, None, None) == -1
    assert L.hv_upright2p_lk_batch_dev(None, C.byref(p), C.byref(par), 100, st, xy, xy, xy, st, None, cb, cb, T, dr, st, st, None, None) == -1
    assert L.hv_upright2p_lk_batch_dev(None, C.byref(p), None, 1025, None, None, None, None, None, None, None, None, None, None, None, None,
                                       None, None) == -2
