"""C ABI of the full point cloud entry (added within ABI 4; no GPU needed): the symbol, the struct layout against the header,
every NULL and UNSUPPORTED path, which are all decided before the filter handle is looked at, and what must not have changed:
ABI 4, HV_K_COUNT = 20, and the three index entries still refusing fullPointCloud = 1."""
import ctypes as C

from hybvio_amd import capi
from test_output_abi import HEADER, INVALID, UNSUPPORTED, header_members

OPTIONAL_IN = ("full_update_dev", "stationary_dev", "odometry_to_slam_dev", "ready_dev")
OPTIONAL_OUT = ("n_attempts", "good_frame")
RANDOM = 2


def test_symbol_abi_version_and_timer_classes():
    L = capi.lib()
    assert hasattr(L, "hv_full_point_cloud_dev") and "hv_full_point_cloud_dev" in capi.PROTOTYPES
    assert L.hv_abi_version() == 4
    assert "HV_K_COUNT = 20 }" in open(HEADER).read()          # no timer class was added: HV_K_TRAIL_INDEX and HV_K_VU_TRI
    assert capi.trail_index_default_params().fullPointCloud == 0


def test_struct_member_order_and_size_match_the_header():
    assert [k for k, _ in capi.FullCloudFrame._fields_] == header_members("hv_full_cloud_frame")
    assert [k for k, _ in capi.FullCloudTable._fields_] == header_members("hv_full_cloud")
    assert C.sizeof(capi.FullCloudFrame) == 10 * C.sizeof(C.c_void_p) and C.sizeof(capi.FullCloudTable) == 12 * C.sizeof(C.c_void_p)
    # no existing struct changed its layout
    assert [k for k, _ in capi.TrailIndexParams._fields_] == header_members("hv_trail_index_params")
    assert [k for k, _ in capi.TrailIndexTable._fields_] == header_members("hv_trail_index")
    assert [k for k, _ in capi.OutputFrame._fields_] == header_members("hv_output_frame")
    assert [k for k, _ in capi.OutputTable._fields_] == header_members("hv_output")
    f = capi.full_cloud_frame(draws_dev=16, ready_dev=0)
    assert f.draws_dev == 16 and f.ready_dev is None and f.pf_dev is None


def _tables(addr):
    trail = capi.TrailIndexTable(*([addr] * len(capi.TrailIndexTable._fields_)))
    table = capi.track_table(n_tracks=addr, ids=addr)
    frame = capi.FullCloudFrame(*([addr] * len(capi.FullCloudFrame._fields_)))
    out = capi.FullCloudTable(*([addr] * len(capi.FullCloudTable._fields_)))
    return trail, table, frame, out


def test_every_argument_check_returns_with_a_null_filter():
    L = capi.lib()
    tp, vp = capi.trail_index_default_params(), capi.vu_default_params(useStereo=1)
    buf = (C.c_double * 4)()
    addr = C.addressof(buf)
    trail, table, frame, out = _tables(addr)

    def call(tp=tp, vp=vp, trail=trail, table=table, frame=frame, out=out):
        return L.hv_full_point_cloud_dev(None, *[C.byref(x) if x is not None else None for x in (tp, vp, trail, table, frame, out)])

    assert call() == INVALID                                               # everything given: the NULL handle is what is left
    for k in ("tp", "vp", "trail", "table", "frame", "out"):
        assert call(**{k: None}) == INVALID, k
    for k, _ in capi.TrailIndexTable._fields_:
        t2 = _tables(addr)[0]
        setattr(t2, k, None)
        assert call(trail=t2) == INVALID, k
    for k in ("n_tracks", "ids"):
        assert call(table=capi.track_table(**{j: addr for j in ("n_tracks", "ids") if j != k})) == INVALID, k
    for k, _ in capi.FullCloudFrame._fields_:
        f2 = _tables(addr)[2]
        setattr(f2, k, None)
        assert call(frame=f2) == INVALID, k                                # (an optional one: the NULL handle's INVALID, see below)
    for k, _ in capi.FullCloudTable._fields_:
        if k not in OPTIONAL_OUT:
            o2 = _tables(addr)[3]
            setattr(o2, k, None)
            assert call(out=o2) == INVALID, k
    # the parameter errors hv_trail_* reports
    for over in (dict(maxTracks=0), dict(cameraTrailLength=0), dict(cameraTrailHanoiLength=-1), dict(cameraTrailHanoiLength=20),
                 dict(cameraTrailStridedLength=2, cameraTrailStridedStride=0), dict(trackSampling=3), dict(trackSampling=-1)):
        assert call(tp=capi.trail_index_default_params(**over)) == INVALID, over
    # one index, one rig
    assert call(vp=capi.vu_default_params(useStereo=0)) == INVALID
    # the limits are decided without a handle, so UNSUPPORTED (not the NULL handle's INVALID) comes back; the optional arrays absent
    f3, o3 = _tables(addr)[2], _tables(addr)[3]
    for k in OPTIONAL_IN:
        setattr(f3, k, None)
    for k in OPTIONAL_OUT:
        setattr(o3, k, None)
    for over in (dict(trackSampling=RANDOM), dict(hybridMapSize=1), dict(useIndependentStereoTriangulation=1), dict(maxTracks=1025),
                 dict(cameraTrailLength=64), dict(maxVisualUpdates=65), dict(maxVisualUpdates=0)):
        assert call(tp=capi.trail_index_default_params(**over), frame=f3, out=o3) == UNSUPPORTED, over
    assert call(vp=capi.vu_default_params(useStereo=1, useLinearTriangulation=1), frame=f3, out=o3) == UNSUPPORTED
    assert call(frame=f3, out=o3) == INVALID                               # supported: the NULL handle
    # calling the entry is the switch: fullPointCloud is not read
    assert call(tp=capi.trail_index_default_params(fullPointCloud=1), frame=f3, out=o3) == INVALID
    assert call(tp=capi.trail_index_default_params(maxTracks=1024, cameraTrailLength=63, cameraTrailHanoiLength=3, maxVisualUpdates=64)) == INVALID
    # a call that is both invalid and unsupported is reported as invalid
    assert call(tp=capi.trail_index_default_params(trackSampling=RANDOM), out=None) == INVALID


def test_the_index_entries_still_refuse_full_point_cloud():
    L = capi.lib()
    buf = (C.c_double * 4)()
    addr = C.addressof(buf)
    trail = capi.TrailIndexTable(*([addr] * len(capi.TrailIndexTable._fields_)))
    table = capi.track_table(n_tracks=addr, ids=addr, xy=addr, second_xy=addr)
    cam = capi.camera_model("pinhole", 400.0, 400.0, 300.0, 200.0)
    p = capi.trail_index_default_params(fullPointCloud=1)
    a = C.c_void_p(addr)
    assert L.hv_trail_init_batch_dev(None, C.byref(p), 1, C.byref(trail)) == UNSUPPORTED
    assert L.hv_trail_select_batch_dev(None, C.byref(p), 1, C.byref(trail), C.byref(table), C.addressof(cam), C.addressof(cam), *([a] * 13)) == UNSUPPORTED
    assert L.hv_trail_finish_batch_dev(None, C.byref(p), 1, C.byref(trail), *([a] * 11)) == UNSUPPORTED
