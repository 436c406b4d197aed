"""C ABI of the session lifecycle entries (added within ABI 4; no GPU needed): symbols, defaults, struct layout against the header,
and the argument checks, which are all decided before the filter handle is looked at."""
import ctypes as C
import os
import re

from hybvio_amd import capi

NEW = ("hv_session_default_params", "hv_session_init_dev", "hv_session_imu_dev", "hv_session_status_dev", "hv_session_reset_dev")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hybvio_hip.h")
INVALID, UNSUPPORTED = -1, -2


def header_members(struct):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        names += [n.strip(" *\n") for n in re.sub(r"^\s*(const\s+)?\w+\s+", "", decl.strip()).split(",") if n.strip()]
    return names


def test_session_symbols_defaults_and_abi_version():
    L = capi.lib()
    for s in NEW:
        assert hasattr(L, s) and s in capi.PROTOTYPES, s
    p = capi.session_default_params()
    # codegen/parameter_definitions.c:4, 193-204, 220
    assert (p.targetFps, p.visualUpdateForEveryNFrame, p.goodFramesTimeWindowSeconds, p.goodFramesToTracking,
            p.goodFramesToTrackingFailed, p.resetUntilInitSucceeds, p.resetOnFailedTracking, p.resetAfterTrackingFailsToInitialize,
            p.freezeOnFailedTracking) == (30.0, 1, 2.0, 0.75, 0.05, 0, 0, 3.0, 0)
    assert capi.session_window(p) == 60
    assert capi.session_default_params(targetFps=2.0).targetFps == 2.0
    assert L.hv_abi_version() == 4
    assert capi.K_EKF_CONTROL == 18 and len(capi.PROTOTYPES) > 0
    assert "HV_K_COUNT = 20 }" in open(HEADER).read()                   # no timer class was added: the entries use HV_K_EKF_CONTROL
    L.hv_session_default_params(None)                                   # a NULL pointer is ignored


def test_the_restatement_has_the_same_defaults():
    import session_restatement as R
    p, r = capi.session_default_params(), R.Params()
    for k, _ in capi.SessionParams._fields_:
        assert getattr(p, k) == getattr(r, k), k
    assert capi.session_window(p) == R.window(r)


def test_struct_member_order_matches_the_header():
    assert [k for k, _ in capi.SessionParams._fields_] == header_members("hv_session_params")
    assert [k for k, _ in capi.SessionState._fields_] == header_members("hv_session")
    assert [k for k, _ in capi.SessionState._fields_] == [
        "good_ring", "ring_head", "ring_entries", "tracking_status", "control_status", "last_reset_time", "first_sample",
        "first_sample_t", "prev_sample_t", "time", "initialized_orientation"]


def _tables(addr):
    st = capi.SessionState(*([addr] * len(capi.SessionState._fields_)))
    ctl = capi.EkfControlTable(addr, addr, addr, addr)
    table = capi.TrackTable(*([addr] * len(capi.TrackTable._fields_)))
    trail = capi.TrailIndexTable(*([addr] * len(capi.TrailIndexTable._fields_)))
    return st, ctl, table, trail


def test_every_argument_check_returns_with_a_null_filter():
    L = capi.lib()
    p, tp, ip = capi.session_default_params(), capi.track_table_default_params(), capi.trail_index_default_params()
    buf = (C.c_double * 4)()
    addr = C.addressof(buf)
    st, ctl, table, trail = _tables(addr)
    r = C.byref

    def init(p=p, st=st):
        return L.hv_session_init_dev(None, r(p) if p else None, r(st) if st else None)

    def imu(st=st, n=1, t=addr, acc=addr, dt=addr, time=addr):
        return L.hv_session_imu_dev(None, r(st) if st else None, n, t, acc, None, dt, time)

    def status(p=p, st=st, good=addr, kind=addr):
        return L.hv_session_status_dev(None, r(p) if p else None, r(st) if st else None, good, None, None, None, kind)

    def reset(p=p, st=st, ctl=ctl, tp=tp, table=table, ip=ip, trail=trail, kind=addr):
        a = [r(x) if x is not None else None for x in (p, st, ctl, tp, table, ip, trail)]
        return L.hv_session_reset_dev(None, *a, kind)

    # every argument in order, a NULL handle: the handle is the last thing looked at
    assert init() == imu() == status() == reset() == INVALID
    assert init(p=None) == init(st=None) == INVALID
    assert imu(st=None) == imu(t=None) == imu(acc=None) == imu(dt=None) == imu(time=None) == INVALID
    assert imu(n=0) == imu(n=33) == INVALID and imu(n=32) == INVALID
    assert status(p=None) == status(st=None) == status(good=None) == status(kind=None) == INVALID
    for k in ("p", "st", "ctl", "tp", "table", "ip", "trail", "kind"):
        assert reset(**{k: None}) == INVALID, k
    # a NULL member of every state struct
    for k, _ in capi.SessionState._fields_:
        s2 = _tables(addr)[0]
        setattr(s2, k, None)
        assert init(st=s2) == imu(st=s2) == status(st=s2) == reset(st=s2) == INVALID, k
    for k, _ in capi.EkfControlTable._fields_:
        c2 = _tables(addr)[1]
        setattr(c2, k, None)
        assert reset(ctl=c2) == INVALID, k
    for k, _ in capi.TrackTable._fields_:
        if k == "second_xy":
            continue                                                    # NULL = mono
        t2 = _tables(addr)[2]
        setattr(t2, k, None)
        assert reset(table=t2) == INVALID, k
    for k, _ in capi.TrailIndexTable._fields_:
        t2 = _tables(addr)[3]
        setattr(t2, k, None)
        assert reset(trail=t2) == INVALID, k
    assert reset(tp=capi.track_table_default_params(maxTracks=100)) == INVALID       # the table and the index disagree
    # the W rules: INVALID below 1 and for visualUpdateForEveryNFrame < 1, UNSUPPORTED above HV_SESSION_MAX_WINDOW -- decided
    # without a handle, so UNSUPPORTED (not the NULL handle's INVALID) comes back
    for bad in (capi.session_default_params(targetFps=0.4), capi.session_default_params(visualUpdateForEveryNFrame=0),
                capi.session_default_params(goodFramesTimeWindowSeconds=-1.0), capi.session_default_params(targetFps=float("nan"))):
        assert init(p=bad) == status(p=bad) == reset(p=bad) == INVALID
    big = capi.session_default_params(targetFps=128.5)                   # W = 257
    assert capi.session_window(big) == 257
    assert init(p=big) == status(p=big) == reset(p=big) == UNSUPPORTED
    edge = capi.session_default_params(targetFps=128.0)                  # W = 256: supported, so the NULL handle is what is left
    assert init(p=edge) == status(p=edge) == reset(p=edge) == INVALID
    # too large a table or trail: UNSUPPORTED, again before the handle
    assert reset(tp=capi.track_table_default_params(maxTracks=2000), ip=capi.trail_index_default_params(maxTracks=2000)) == UNSUPPORTED
    assert reset(ip=capi.trail_index_default_params(cameraTrailLength=64)) == UNSUPPORTED
