"""CPU checks of the device track table entries (added within ABI 4): exported symbols, default parameters against
codegen/parameter_definitions.c, the timer class number, and the argument checks decided before the context is looked at."""
import ctypes as C

from hybvio_amd import capi

ENTRIES = ("hv_track_table_default_params", "hv_tracks_init_batch_dev", "hv_tracks_update_batch_dev", "hv_tracks_append_batch_dev",
           "hv_tracks_delete_batch_dev")
MEMBERS = ("n_tracks", "ids", "xy", "second_xy", "status", "blacklist", "kf_xy", "kf_valid", "frame_num", "mask_steps", "mask_radius",
           "frame_flags")


def test_track_table_symbols_defaults_and_abi_version():
    L = capi.lib()
    for s in ENTRIES:
        assert hasattr(L, s), s
    p = capi.track_table_default_params()
    assert p.maxTracks == 200 and p.maxTrackLength == 21                   # parameter_definitions.c:262, :265
    assert p.relativeMaskRadius == 0.0667                                  # :308
    assert p.visualStationarityMovementThreshold == 3.0                    # :111
    assert p.visualStationarityScoreThreshold == 0.95                      # :113
    assert capi.track_table_default_params(maxTracks=64).maxTracks == 64
    assert L.hv_abi_version() == 4
    assert capi.K_TRACK_TABLE == 16 and capi.K_DETECT_TAIL == 15
    assert capi.TRACKS_MAX_TRACKS == capi.DETECTION_FILTER_MAX_POINTS == 1024
    assert [k for k, _ in capi.TrackTable._fields_] == list(MEMBERS)


def test_track_table_argument_checks_come_before_the_context():
    """HV_ERR_INVALID (-1) for a NULL required pointer (a table member included), a negative size, maxTracks < 1 and a stereo /
    mono mismatch; HV_ERR_UNSUPPORTED (-2) for n_sets > 65535 and maxTracks > 1024; all decided with a NULL context, where
    valid arguments give HV_ERR_INVALID for the context itself."""
    L = capi.lib()
    buf = (C.c_float * 4096)()
    a = C.addressof(buf)

    def table(stereo=True, **over):
        m = {k: a for k in MEMBERS}
        if not stereo:
            m["second_xy"] = 0
        m.update(over)
        return capi.track_table(**m)

    def prm(**over):
        return capi.track_table_default_params(**over)

    P, TS, TM = prm(), table(), table(stereo=False)
    v = C.c_void_p

    init = lambda n_sets=1, p=P, t=TS: L.hv_tracks_init_batch_dev(None, C.byref(p) if p else None, n_sets, C.byref(t) if t else None)
    assert init() == -1 and init(t=TM) == -1                                   # valid stereo / mono, no context
    assert init(p=None) == -1 and init(t=None) == -1 and init(n_sets=-1) == -1
    assert init(p=prm(maxTracks=0)) == -1 and init(p=prm(maxTracks=-3)) == -1
    assert init(n_sets=65536) == -2 and init(p=prm(maxTracks=1025)) == -2 and init(p=prm(maxTracks=1024)) == -1
    for k in MEMBERS:
        if k != "second_xy":
            assert init(t=table(**{k: 0})) == -1, k
            assert init(n_sets=65536, t=table(**{k: 0})) == -1, k               # the NULL member is reported first

    def upd(n_sets=1, p=P, t=TS, corners=a, second=a, ts=a, score=a, kf=a, mask=a, n_mask=a, src=a, mm=a):
        return L.hv_tracks_update_batch_dev(None, C.byref(p), n_sets, C.byref(t), v(corners or None), v(second or None), v(ts or None),
                                            v(score or None), v(kf or None), v(mask or None), v(n_mask or None), v(src or None),
                                            v(mm or None))
    assert upd() == -1 and upd(t=TM, second=0) == -1                            # valid stereo / mono, no context
    assert upd(score=0, src=0, mm=0) == -1                                      # the optional ones
    assert upd(second=0) == -1 and upd(t=TM) == -1                              # stereo / mono mismatch
    for k in ("corners", "ts", "kf", "mask", "n_mask"):
        assert upd(**{k: 0}) == -1, k
    assert upd(n_sets=-1) == -1 and upd(p=prm(maxTracks=0)) == -1 and upd(t=table(ids=0)) == -1
    assert upd(n_sets=65536) == -2 and upd(p=prm(maxTracks=1025)) == -2
    assert upd(n_sets=65536, corners=0) == -1 and upd(p=prm(maxTracks=1025), second=0) == -1   # invalid wins over too large

    def app(n_sets=1, p=P, t=TS, max_new=10, n_new=a, new=a, second=a, added=a):
        return L.hv_tracks_append_batch_dev(None, C.byref(p), n_sets, C.byref(t), max_new, v(n_new or None), v(new or None),
                                            v(second or None), v(added or None))
    assert app() == -1 and app(t=TM, second=0) == -1 and app(added=0) == -1
    assert app(second=0) == -1 and app(t=TM) == -1                              # stereo / mono mismatch
    assert app(n_new=0) == -1 and app(new=0) == -1 and app(max_new=-1) == -1 and app(n_sets=-1) == -1
    assert app(t=table(frame_flags=0)) == -1 and app(p=prm(maxTracks=0)) == -1
    assert app(n_sets=65536) == -2 and app(p=prm(maxTracks=2000)) == -2
    assert app(n_sets=65536, new=0) == -1 and app(n_sets=65536, max_new=-1) == -1
    assert app(max_new=0, n_new=0, new=0, second=0) == -1                       # nothing to read: valid, no context

    def dele(n_sets=1, p=P, t=TS, max_ids=4, n_ids=a, ids=a):
        return L.hv_tracks_delete_batch_dev(None, C.byref(p), n_sets, C.byref(t), max_ids, v(n_ids or None), v(ids or None))
    assert dele() == -1 and dele(t=TM) == -1
    assert dele(n_ids=0) == -1 and dele(ids=0) == -1 and dele(max_ids=-1) == -1 and dele(n_sets=-1) == -1
    assert dele(t=table(status=0)) == -1 and dele(p=prm(maxTracks=0)) == -1
    assert dele(n_sets=65536) == -2 and dele(p=prm(maxTracks=1025)) == -2
    assert dele(n_sets=65536, ids=0) == -1
