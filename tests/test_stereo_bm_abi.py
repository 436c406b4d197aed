"""CPU checks of the dense-stereo entries (added within ABI 4): the entries are in the header and bound in capi.py, the defaults, every
argument check that is decided before the context is looked at (made with a NULL context), what must not have changed (ABI 4,
HV_K_COUNT = 20), and that a context cannot be created without a device."""
import ctypes as C
import os
import re

import pytest

from hybvio_amd import capi

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "hybvio_hip.h")
INVALID, UNSUPPORTED = -1, -2
X = C.c_void_p(16)          # a non-NULL pointer that is never dereferenced: every call below is refused first
ENTRIES = ("hv_stereo_num_disparities", "hv_stereo_bm_default_params", "hv_stereo_work_bytes", "hv_filter_speckles_work_bytes",
           "hv_stereo_cloud_bound", "hv_stereo_disparity_batch_dev", "hv_filter_speckles_batch_dev", "hv_stereo_track_depth_batch_dev",
           "hv_stereo_point_cloud_batch_dev", "hv_stereo_disparity", "hv_stereo_track_depth", "hv_stereo_point_cloud")
Q = (C.c_double * 16)(*range(16))


def test_entries_defaults_and_abi_version():
    L = capi.lib()
    text = open(HEADER).read()
    for s in ENTRIES:
        assert hasattr(L, s), s
        assert s in capi.PROTOTYPES, s
        assert re.search(r"\b" + s + r"\(", text), s
    assert [capi.stereo_num_disparities(w) for w in (752, 1280, 320, 160)] == [96, 128, 32, 32]
    assert capi.stereo_num_disparities(0) == 0
    p = capi.stereo_bm_default_params(752)
    assert (p.numDisparities, p.blockSize, p.preFilterCap, p.textureThreshold, p.uniquenessRatio, p.speckleWindowSize, p.speckleRange) \
        == (96, 21, 31, 10, 15, 500, 10)
    assert capi.stereo_bm_default_params(1280).numDisparities == 128
    assert C.sizeof(capi.StereoBmParams) == 28 and capi.STEREO_FILTERED == -16 and "#define HV_STEREO_FILTERED (-16)" in text
    assert L.hv_abi_version() == 4
    assert "HV_K_COUNT = 20 }" in text                               # no timer class was added: HV_K_INGEST and HV_K_STEREO_GATE
    assert "typedef struct hv_stereo_bm_params" in text and "stereo_disparity.cpp" in text and "tracker.cpp:532" in text
    assert L.hv_stereo_work_bytes(None, C.byref(p), 3) == 0 and L.hv_stereo_cloud_bound(None, 5) == INVALID
    assert capi.filter_speckles_work_bytes(300, 200, 2) >= 2 * 8 * 300 * 200 and capi.filter_speckles_work_bytes(0, 5, 1) == 0


def _disparity(p, n_sets=1, left=X, right=X, work=X, disp=X, stride=1 << 20, n_valid=X):
    return capi.lib().hv_stereo_disparity_batch_dev(None, C.byref(p) if p is not None else None, n_sets, left, right, work, disp, stride,
                                                    n_valid)


def test_disparity_entries_refuse_bad_arguments_with_a_null_context():
    L = capi.lib()
    ok = capi.stereo_bm_default_params(752)
    assert _disparity(ok) == INVALID                                 # all arguments good: the NULL context itself
    assert _disparity(ok, n_valid=None) == INVALID                   # (n_valid_dev may be NULL: still only the context)
    assert _disparity(None) == INVALID
    for bad in (dict(numDisparities=0), dict(numDisparities=-16), dict(numDisparities=40), dict(blockSize=20), dict(blockSize=3),
                dict(preFilterCap=0), dict(preFilterCap=64), dict(textureThreshold=-1), dict(uniquenessRatio=-1)):
        assert _disparity(capi.stereo_bm_default_params(752, **bad)) == INVALID, bad
    for bad in (dict(n_sets=-1), dict(left=None), dict(right=None), dict(work=None), dict(disp=None), dict(stride=-1)):
        assert _disparity(ok, **bad) == INVALID, bad
    # the limits, every other argument good: blockSize 21 is the one size served
    for lim in (dict(blockSize=19), dict(blockSize=5), dict(blockSize=23), dict(numDisparities=272), dict(uniquenessRatio=101),
                dict(textureThreshold=65536)):
        assert _disparity(capi.stereo_bm_default_params(752, **lim)) == UNSUPPORTED, lim
    assert _disparity(capi.stereo_bm_default_params(752, numDisparities=256, preFilterCap=63)) == INVALID       # within the limits
    assert _disparity(capi.stereo_bm_default_params(752, numDisparities=16, preFilterCap=1)) == INVALID
    assert _disparity(ok, n_sets=32768) == UNSUPPORTED and _disparity(ok, n_sets=32767) == INVALID
    assert _disparity(capi.stereo_bm_default_params(752, blockSize=19), work=None) == INVALID   # invalid before unsupported
    # the synchronous form
    out = (C.c_int16 * 16)()
    call = lambda p=ok, o=out: L.hv_stereo_disparity(None, C.byref(p) if p is not None else None, 0, 1, o, 752)
    assert call() == INVALID and call(p=None) == INVALID and call(o=None) == INVALID
    assert call(p=capi.stereo_bm_default_params(752, numDisparities=8)) == INVALID


def test_speckle_depth_and_cloud_entries_refuse_bad_arguments_with_a_null_context():
    L = capi.lib()
    spk = lambda n=1, w=64, h=48, disp=X, stride=64 * 48, new_val=-16, size=500, diff=10, work=X: \
        L.hv_filter_speckles_batch_dev(None, n, w, h, disp, stride, new_val, size, diff, work)
    assert spk() == INVALID
    for bad in (dict(n=-1), dict(w=0), dict(h=0), dict(disp=None), dict(work=None), dict(stride=64 * 48 - 1), dict(new_val=40000),
                dict(new_val=-40000), dict(size=-1), dict(diff=-1)):
        assert spk(**bad) == INVALID, bad
    assert spk(n=65536) == UNSUPPORTED and spk(n=65535) == INVALID
    assert spk(w=65536, h=32768, stride=1 << 31) == UNSUPPORTED      # 2^31 pixels: the labels are int32
    depth = lambda n=1, m=10, n_pts=X, xy=X, disp=X, stride=1 << 20, q=Q, out=X: \
        L.hv_stereo_track_depth_batch_dev(None, n, m, n_pts, xy, disp, stride, q, out)
    assert depth() == INVALID
    for bad in (dict(n=-1), dict(m=-1), dict(n_pts=None), dict(xy=None), dict(disp=None), dict(stride=-1), dict(q=None), dict(out=None)):
        assert depth(**bad) == INVALID, bad
    assert depth(n=65536) == UNSUPPORTED and depth(m=0, xy=None, out=None) == INVALID
    cloud = lambda n=1, disp=X, stride=1 << 20, q=Q, s=5, m=100, xyz=X, n_out=X: \
        L.hv_stereo_point_cloud_batch_dev(None, n, disp, stride, q, s, m, xyz, n_out)
    assert cloud() == INVALID
    for bad in (dict(n=-1), dict(disp=None), dict(stride=-1), dict(q=None), dict(s=0), dict(s=-5), dict(m=-1), dict(xyz=None), dict(n_out=None)):
        assert cloud(**bad) == INVALID, bad
    f = (C.c_float * 8)()
    n = C.c_int(0)
    assert L.hv_stereo_track_depth(None, 1, f, X, 752, Q, f) == INVALID
    assert L.hv_stereo_point_cloud(None, X, 752, Q, 5, f, 2, C.byref(n)) == INVALID


def test_a_context_needs_a_device():
    import torch
    if not torch.cuda.is_available():                                # (with a device the GPU tests create their contexts)
        with pytest.raises(capi.HvError, match="no HIP device"):      # HV_ERR_NO_DEVICE: nothing is computed on the CPU
            with capi.Context(width=160, height=96, levels=1) as ctx:
                ctx.stereo_disparity(0, 1)
