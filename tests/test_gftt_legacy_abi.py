"""CPU checks of the legacy GFTT detector entries (added within ABI 4): exported symbols, defaults, every argument check that is
decided before the context is looked at (made with a NULL context), and what must not have changed (ABI 4, HV_K_COUNT = 20)."""
import ctypes as C
import os

from hybvio_amd import capi

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "hybvio_hip.h")
INVALID, UNSUPPORTED = -1, -2
X = C.c_void_p(16)          # a non-NULL pointer that is never dereferenced: every call below is refused first


def test_symbols_defaults_and_abi_version():
    L = capi.lib()
    for s in ("hv_gftt_legacy_default_params", "hv_gftt_legacy_tile_size", "hv_gftt_legacy_min_distance", "hv_gftt_legacy_keypoint_bound",
              "hv_gftt_legacy_work_bytes", "hv_gftt_legacy_keypoints_batch_dev", "hv_gftt_legacy_detect_batch_dev", "hv_gftt_legacy_detect"):
        assert hasattr(L, s), s
    p = capi.gftt_legacy_default_params()
    assert (p.gfttBlockSize, p.gfttQualityLevel, p.gfttMinDistance, p.maxTracks) == (3, 0.01, 50.0, 200)
    assert L.hv_abi_version() == 4
    text = open(HEADER).read()
    assert "HV_K_COUNT = 20 }" in text                               # no timer class was added: HV_K_GFTT and HV_K_DETECT_TAIL
    tw, th = capi.gftt_legacy_tile_size()
    assert f"#define HV_GFTT_LEGACY_TILE_W {tw} " in text and f"#define HV_GFTT_LEGACY_TILE_H {th}\n" in text
    assert L.hv_gftt_legacy_keypoint_bound(None) == INVALID and L.hv_gftt_legacy_work_bytes(None, 3, 100) == 0
    assert L.hv_gftt_legacy_min_distance(None, C.byref(p)) == -1.0
    # every entry cites the reference lines it replaces
    start = text.index("legacy GFTT feature detector")
    section = text[start:text.index("sub-pixel corner refinement", start)]
    assert section.count(":53-139") >= 4 and "feature_detector_legacy.cpp:53-139" in section and "feature_detector_legacy.cpp:20-51" in section


def _detect(p, n_images=1, slots=X, work=X, max_kp=100, n_cand=X, max_prev=4, n_prev=X, prev=X, radius=X, max_corners=200, corners=X,
            resp=X, n_out=X):
    return capi.lib().hv_gftt_legacy_detect_batch_dev(None, C.byref(p) if p is not None else None, n_images, slots, work, max_kp, n_cand,
                                                      max_prev, n_prev, prev, radius, max_corners, corners, resp, n_out)


def _keypoints(p, n_images=1, slots=X, work=X, max_kp=100, n_cand=X, max_corners=200, corners=X, resp=X, n_out=X):
    return capi.lib().hv_gftt_legacy_keypoints_batch_dev(None, C.byref(p) if p is not None else None, n_images, slots, work, max_kp,
                                                         n_cand, max_corners, corners, resp, n_out)


def test_batch_entries_refuse_bad_arguments_with_a_null_context():
    ok = capi.gftt_legacy_default_params()
    assert _detect(ok) == INVALID and _keypoints(ok) == INVALID      # all arguments good: the NULL context itself
    assert _detect(None) == INVALID and _keypoints(None) == INVALID
    for bad in (dict(maxTracks=0), dict(maxTracks=-3), dict(gfttQualityLevel=0.0), dict(gfttQualityLevel=-0.5),
                dict(gfttQualityLevel=float("nan")), dict(gfttMinDistance=-1.0), dict(gfttMinDistance=float("nan"))):
        p = capi.gftt_legacy_default_params(**bad)
        assert _detect(p) == INVALID and _keypoints(p) == INVALID, bad
    for bad in (dict(n_images=-1), dict(max_kp=-1), dict(max_prev=-1), dict(max_corners=-1), dict(slots=None), dict(work=None),
                dict(n_cand=None), dict(radius=None), dict(corners=None), dict(n_out=None), dict(n_prev=None), dict(prev=None),
                dict(max_corners=99), dict(max_kp=300, max_corners=199)):
        assert _detect(ok, **bad) == INVALID, bad
    for bad in (dict(n_images=-1), dict(max_kp=-1), dict(max_corners=-1), dict(slots=None), dict(work=None), dict(n_cand=None),
                dict(corners=None), dict(n_out=None), dict(max_corners=99)):
        assert _keypoints(ok, **bad) == INVALID, bad
    # the responses are optional; gfttMinDistance 0 is the "< 1" branch, not an error
    assert _detect(ok, resp=None, n_images=70000) == UNSUPPORTED and _keypoints(ok, resp=None, n_images=70000) == UNSUPPORTED
    assert _detect(capi.gftt_legacy_default_params(gfttMinDistance=0.0), n_images=70000) == UNSUPPORTED
    # the capacity rule is min(maxTracks, max_keypoints)
    assert _detect(ok, max_kp=100, max_corners=100, n_images=70000) == UNSUPPORTED
    assert _detect(ok, max_kp=300, max_corners=200, n_images=70000) == UNSUPPORTED
    # the limits, every other argument good
    for block in (1, 2, 4, 9, 0, -3):
        p = capi.gftt_legacy_default_params(gfttBlockSize=block)
        assert _detect(p) == UNSUPPORTED and _keypoints(p) == UNSUPPORTED, block
    for block in (3, 5, 7):
        assert _detect(capi.gftt_legacy_default_params(gfttBlockSize=block)) == INVALID      # only the NULL context is left
    assert _detect(ok, n_images=65536) == UNSUPPORTED and _keypoints(ok, n_images=65536) == UNSUPPORTED
    assert _detect(ok, n_images=65535) == INVALID
    assert _detect(ok, max_prev=capi.DETECT_TAIL_MAX_PREV + 1) == UNSUPPORTED
    assert _detect(ok, max_prev=capi.DETECT_TAIL_MAX_PREV) == INVALID
    big = capi.gftt_legacy_default_params(maxTracks=capi.DETECT_TAIL_MAX_TRACKS + 1)
    assert _detect(big, max_corners=5000) == UNSUPPORTED and _keypoints(big, max_corners=5000) == UNSUPPORTED
    assert _detect(capi.gftt_legacy_default_params(maxTracks=capi.DETECT_TAIL_MAX_TRACKS), max_corners=5000) == INVALID
    # an invalid argument is reported before an unsupported one
    assert _detect(ok, n_images=70000, work=None) == INVALID
    assert _detect(capi.gftt_legacy_default_params(gfttBlockSize=4, maxTracks=0)) == INVALID
    # no live tracks: the two arrays may be NULL
    assert _detect(ok, max_prev=0, n_prev=None, prev=None, n_images=70000) == UNSUPPORTED


def test_host_entry_refuses_bad_arguments_with_a_null_context():
    L = capi.lib()
    ok = capi.gftt_legacy_default_params()
    xy = (C.c_float * 400)()
    n = C.c_int(0)
    call = lambda p=ok, prev=None, n_prev=0, r=30, out=xy, cap=200, n_out=C.byref(n): \
        L.hv_gftt_legacy_detect(None, C.byref(p) if p is not None else None, 0, prev, n_prev, r, out, cap, n_out)
    assert call() == INVALID                                         # the NULL context
    assert call(p=None) == INVALID and call(out=None) == INVALID and call(n_out=None) == INVALID
    assert call(n_prev=-1) == INVALID and call(n_prev=2) == INVALID and call(cap=-1) == INVALID
    assert call(r=0) == INVALID and call(r=-5) == INVALID            # the reference asserts maskRadius >= 1
    for bad in (dict(maxTracks=0), dict(gfttQualityLevel=0.0), dict(gfttMinDistance=-0.1)):
        assert call(p=capi.gftt_legacy_default_params(**bad)) == INVALID
