"""CPU checks of the device detect() tail entries (added within ABI 4): exported symbols, the timer class number, the
documented limits, and the argument checks decided before the context is looked at."""
import ctypes as C

from hybvio_amd import capi

ENTRIES = ("hv_apply_min_distance_batch_dev", "hv_gftt_corners_batch_dev", "hv_gftt_detect_batch_dev")


def test_detect_tail_symbols_timer_class_and_abi_version():
    L = capi.lib()
    for s in ENTRIES:
        assert hasattr(L, s), s
        assert hasattr(capi.Context, s[3:]), s
    assert L.hv_abi_version() == 4
    assert capi.K_DETECT_TAIL == 15 and capi.K_STEREO_GATE == 14
    # the limits cover the sizes the suite uses: 1280 x 720 at block edge 8, 1024 live tracks, maxTracks 4096
    assert capi.DETECT_TAIL_MAX_KEYPOINTS >= 16384 and capi.DETECT_TAIL_MAX_PREV >= 1024 and capi.DETECT_TAIL_MAX_TRACKS >= 4096
    assert capi.DETECT_TAIL_MAX_CORNERS >= 2 * capi.DETECT_TAIL_MAX_KEYPOINTS


def test_detect_tail_argument_checks_come_before_the_context():
    """HV_ERR_INVALID (-1) for NULL required arrays / parameters, negative sizes and max_tracks < 1; HV_ERR_UNSUPPORTED (-2) for
    n_sets > 65535 and sizes beyond the documented limits; all decided with a NULL context."""
    L = capi.lib()
    xy, iv = (C.c_float * 4096)(), (C.c_int32 * 64)()
    gp = capi.gftt_default_params()
    P = C.byref(gp)

    def amd(n_sets=1, mc=10, nc=iv, c=xy, mp=5, npv=iv, pv=xy, r=iv, mt=200, no=iv):
        return L.hv_apply_min_distance_batch_dev(None, n_sets, mc, nc, c, mp, npv, pv, r, mt, no)

    assert amd() == -1                                                               # valid arguments, no context
    assert amd(mp=0, npv=None, pv=None) == -1                                        # no live tracks: NULL allowed, still no context
    assert amd(n_sets=-1) == -1 and amd(mc=-1) == -1 and amd(mp=-1) == -1
    assert amd(mt=0) == -1 and amd(mt=-3) == -1
    assert amd(nc=None) == -1 and amd(c=None) == -1 and amd(r=None) == -1 and amd(no=None) == -1
    assert amd(npv=None) == -1 and amd(pv=None) == -1                                # required when max_prev > 0
    assert amd(n_sets=65536) == -2
    assert amd(mc=capi.DETECT_TAIL_MAX_CORNERS + 1) == -2
    assert amd(mp=capi.DETECT_TAIL_MAX_PREV + 1) == -2
    assert amd(mt=capi.DETECT_TAIL_MAX_TRACKS + 1) == -2
    assert amd(mc=capi.DETECT_TAIL_MAX_CORNERS, mp=1024, mt=4096) == -1              # inside the limits: only the context is missing

    def cor(prm=P, n=1, kp=xy, mp=5, npv=iv, pv=xy, r=iv, mc=400, c=xy, no=iv):
        return L.hv_gftt_corners_batch_dev(None, prm, n, kp, mp, npv, pv, r, mc, c, no)

    def det(prm=P, n=1, sl=iv, kp=xy, mp=5, npv=iv, pv=xy, r=iv, mc=400, c=xy, no=iv):
        return L.hv_gftt_detect_batch_dev(None, prm, n, sl, kp, mp, npv, pv, r, mc, c, no)

    for f in (cor, det):
        assert f() == -1 and f(mp=0, npv=None, pv=None) == -1
        assert f(prm=None) == -1 and f(n=-1) == -1 and f(mp=-1) == -1 and f(mc=-1) == -1
        assert f(kp=None) == -1 and f(r=None) == -1 and f(c=None) == -1 and f(no=None) == -1
        assert f(npv=None) == -1 and f(pv=None) == -1
        assert f(n=65536) == -2 and f(mp=capi.DETECT_TAIL_MAX_PREV + 1) == -2
        assert f(mc=capi.DETECT_TAIL_MAX_CORNERS + 1) == -2 and f(mc=capi.DETECT_TAIL_MAX_CORNERS) == -1
        assert f(prm=C.byref(capi.gftt_default_params(maxTracks=0))) == -1
        assert f(prm=C.byref(capi.gftt_default_params(maxTracks=capi.DETECT_TAIL_MAX_TRACKS + 1))) == -2
        assert f(prm=C.byref(capi.gftt_default_params(maxTracks=4096)), mp=1024) == -1
    assert det(sl=None) == -1
