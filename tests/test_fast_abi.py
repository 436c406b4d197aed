"""CPU checks of the FAST detector entries (added within ABI 4): exported symbols, defaults, every argument check that is decided
before the context is looked at (made with a NULL context), what must not have changed (ABI 4, HV_K_COUNT = 20), and that a
context cannot be created without a device."""
import ctypes as C
import os

import pytest

from hybvio_amd import capi

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "hybvio_hip.h")
INVALID, UNSUPPORTED = -1, -2
X = C.c_void_p(16)          # a non-NULL pointer that is never dereferenced: every call below is refused first


def test_fast_symbols_defaults_and_abi_version():
    L = capi.lib()
    for s in ("hv_fast_default_params", "hv_fast_tile_size", "hv_fast_keypoint_bound", "hv_fast_work_bytes",
              "hv_fast_keypoints_batch_dev", "hv_fast_detect_batch_dev", "hv_fast_detect"):
        assert hasattr(L, s), s
    p = capi.fast_default_params()
    assert (p.threshold, p.maxTracks) == (10, 200)
    assert L.hv_abi_version() == 4
    text = open(HEADER).read()
    assert "HV_K_COUNT = 20 }" in text                               # no timer class was added: HV_K_GFTT and HV_K_DETECT_TAIL
    tw, th = capi.fast_tile_size()
    assert f"#define HV_FAST_TILE_W {tw} " in text and f"#define HV_FAST_TILE_H {th}\n" in text
    assert tw % 4 == 0 and tw * th == 1024
    assert L.hv_fast_keypoint_bound(None) == INVALID and L.hv_fast_work_bytes(None, 3) == 0


def _detect(p, n_images=1, slots=X, work=X, max_kp=100, kp=X, n_kp=X, max_prev=4, n_prev=X, prev=X, radius=X, max_corners=200,
            corners=X, n_out=X):
    return capi.lib().hv_fast_detect_batch_dev(None, C.byref(p) if p is not None else None, n_images, slots, work, max_kp, kp, n_kp,
                                               max_prev, n_prev, prev, radius, max_corners, corners, n_out)


def _keypoints(p, n_images=1, slots=X, work=X, max_kp=100, kp=X, n_kp=X):
    return capi.lib().hv_fast_keypoints_batch_dev(None, C.byref(p) if p is not None else None, n_images, slots, work, max_kp, kp, n_kp)


def test_batch_entries_refuse_bad_arguments_with_a_null_context():
    ok = capi.fast_default_params()
    assert _detect(ok) == INVALID and _keypoints(ok) == INVALID      # all arguments good: the NULL context itself
    assert _detect(None) == INVALID and _keypoints(None) == INVALID
    for bad in (dict(maxTracks=0), dict(maxTracks=-3), dict(threshold=-1), dict(threshold=256)):
        p = capi.fast_default_params(**bad)
        assert _detect(p) == INVALID and _keypoints(p) == INVALID, bad
    for bad in (dict(n_images=-1), dict(max_kp=-1), dict(max_prev=-1), dict(max_corners=-1), dict(slots=None), dict(work=None),
                dict(kp=None), dict(n_kp=None), dict(radius=None), dict(corners=None), dict(n_out=None), dict(n_prev=None),
                dict(prev=None), dict(max_corners=99), dict(max_kp=300, max_corners=199)):
        assert _detect(ok, **bad) == INVALID, bad
    for bad in (dict(n_images=-1), dict(max_kp=-1), dict(slots=None), dict(work=None), dict(kp=None), dict(n_kp=None)):
        assert _keypoints(ok, **bad) == INVALID, bad
    # the capacity rule is min(maxTracks, max_keypoints)
    assert _detect(ok, max_kp=100, max_corners=100, n_images=70000) == UNSUPPORTED
    assert _detect(ok, max_kp=300, max_corners=200, n_images=70000) == UNSUPPORTED
    # the limits, every other argument good
    assert _detect(ok, n_images=65536) == UNSUPPORTED and _keypoints(ok, n_images=65536) == UNSUPPORTED
    assert _detect(ok, n_images=65535) == INVALID                    # within the limit: only the NULL context is left
    assert _detect(ok, max_prev=capi.DETECT_TAIL_MAX_PREV + 1) == UNSUPPORTED
    assert _detect(ok, max_prev=capi.DETECT_TAIL_MAX_PREV) == INVALID
    big = capi.fast_default_params(maxTracks=capi.DETECT_TAIL_MAX_TRACKS + 1)
    assert _detect(big) == UNSUPPORTED
    assert _detect(capi.fast_default_params(maxTracks=capi.DETECT_TAIL_MAX_TRACKS)) == INVALID
    # an invalid argument is reported before an unsupported one
    assert _detect(ok, n_images=70000, work=None) == INVALID
    # no live tracks: the two arrays may be NULL
    assert _detect(ok, max_prev=0, n_prev=None, prev=None, n_images=70000) == UNSUPPORTED


def test_host_entry_refuses_bad_arguments_with_a_null_context():
    L = capi.lib()
    ok = capi.fast_default_params()
    xy = (C.c_float * 400)()
    n = C.c_int(0)
    call = lambda p=ok, prev=None, n_prev=0, r=30, out=xy, cap=200, n_out=C.byref(n): \
        L.hv_fast_detect(None, C.byref(p) if p is not None else None, 0, prev, n_prev, r, out, cap, n_out)
    assert call() == INVALID                                         # the NULL context
    assert call(p=None) == INVALID and call(out=None) == INVALID and call(n_out=None) == INVALID
    assert call(n_prev=-1) == INVALID and call(n_prev=2) == INVALID and call(cap=-1) == INVALID
    assert call(r=0) == INVALID and call(r=-5) == INVALID            # the reference asserts maskRadius >= 1
    for bad in (dict(maxTracks=0), dict(threshold=-1), dict(threshold=256)):
        assert call(p=capi.fast_default_params(**bad)) == INVALID


def test_a_context_needs_a_device():
    import torch
    if not torch.cuda.is_available():                                # (with a device the GPU tests create their contexts)
        with pytest.raises(capi.HvError, match="no HIP device"):      # HV_ERR_NO_DEVICE: nothing is computed on the CPU
            with capi.Context(width=64, height=64, levels=1) as ctx:
                ctx.fast_detect(0)
