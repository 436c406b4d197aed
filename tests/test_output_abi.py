"""C ABI of the output entry (added within ABI 4; no GPU needed): symbols, defaults, struct layout against the header, and the
argument checks, which are all decided before the filter handle is looked at."""
import ctypes as C
import os
import re

from hybvio_amd import capi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hybvio_hip.h")
INVALID, UNSUPPORTED = -1, -2
IDENTITY = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]
OPTIONAL = ("frozen_dev", "stationary_dev", "slam_to_odometry_dev", "odometry_to_slam_dev", "ready_dev")


def header_members(struct):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = re.sub(r"\[\d+\]", "", decl.strip())
        names += [n.strip(" *\n") for n in re.sub(r"^\s*(const\s+)?\w+\s+", "", decl).split(",") if n.strip()]
    return names


def test_output_symbols_defaults_and_abi_version():
    L = capi.lib()
    for s in ("hv_output_default_params", "hv_output_dev"):
        assert hasattr(L, s) and s in capi.PROTOTYPES, s
    p = capi.output_default_params()
    assert list(p.imuToCamera) == IDENTITY and list(p.imuToOutput) == IDENTITY
    t = capi.trail_index_default_params()
    for k in ("maxVisualUpdates", "maxSuccessfulVisualUpdates", "cameraTrailLength", "maxTracks", "useStereo"):
        assert getattr(p, k) == getattr(t, k), k                           # one set of defaults with the index
    assert (p.maxVisualUpdates, p.maxSuccessfulVisualUpdates, p.cameraTrailLength, p.maxTracks, p.useStereo) == (20, 5, 20, 200, 1)
    q = capi.output_default_params(imu_to_output=[[0, 1, 0, 2], [1, 0, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]], maxTracks=8)
    assert list(q.imuToOutput)[:4] == [0.0, 1.0, 0.0, 2.0] and q.maxTracks == 8 and list(q.imuToCamera) == IDENTITY
    assert L.hv_abi_version() == 4
    assert capi.K_EKF_CONTROL == 18
    assert "HV_K_COUNT = 20 }" in open(HEADER).read()                   # no timer class was added: the entry uses HV_K_EKF_CONTROL
    L.hv_output_default_params(None)                                    # a NULL pointer is ignored


def test_the_restatement_has_the_same_constants():
    import output_restatement as R
    text = open(HEADER).read()
    for name, value in (("HV_TRI_OK", R.TRI_OK), ("HV_TRI_BEHIND", R.TRI_BEHIND), ("HV_TRI_NOT_VISITED", R.TRI_NOT_VISITED),
                        ("HV_PREPARE_VU_OK", R.PREPARE_VU_OK), ("HV_PREPARE_VU_BEHIND", R.PREPARE_VU_BEHIND)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name
    p = R.Params(20, 200, 20, 5)
    d = capi.output_default_params()
    for k in ("maxVisualUpdates", "maxSuccessfulVisualUpdates", "cameraTrailLength", "maxTracks"):
        assert getattr(p, k) == getattr(d, k), k
    assert p.imuToCamera == list(d.imuToCamera) and p.imuToOutput == list(d.imuToOutput)


def test_struct_member_order_matches_the_header():
    assert [k for k, _ in capi.OutputParams._fields_] == header_members("hv_output_params")
    assert [k for k, _ in capi.OutputFrame._fields_] == header_members("hv_output_frame")
    assert [k for k, _ in capi.OutputTable._fields_] == header_members("hv_output")
    assert [k for k, _ in capi.OutputTable._fields_] == [
        "t", "tracking_status", "stationary_visual", "inertial_mean", "inertial_cov_diag", "position_cov", "velocity_cov", "n_trail",
        "trail_time", "trail_pose", "api_pose", "api_trail_pose", "n_points", "point_id", "point_status", "point_first_pixel", "point_xyz"]
    assert C.sizeof(capi.OutputParams) == 2 * 16 * 8 + 5 * 4 + 4            # two matrices, five ints, tail padding to 8


def _tables(addr):
    st = capi.SessionState(*([addr] * len(capi.SessionState._fields_)))
    trail = capi.TrailIndexTable(*([addr] * len(capi.TrailIndexTable._fields_)))
    frame = capi.OutputFrame(*([addr] * len(capi.OutputFrame._fields_)))
    out = capi.OutputTable(*([addr] * len(capi.OutputTable._fields_)))
    return st, trail, frame, out


def test_every_argument_check_returns_with_a_null_filter():
    L = capi.lib()
    p = capi.output_default_params()
    buf = (C.c_double * 4)()
    addr = C.addressof(buf)
    st, trail, frame, out = _tables(addr)

    def call(p=p, st=st, trail=trail, frame=frame, out=out):
        return L.hv_output_dev(None, *[C.byref(x) if x is not None else None for x in (p, st, trail, frame, out)])

    assert call() == INVALID                                               # everything given: the NULL handle is what is left
    for k in ("p", "st", "trail", "frame", "out"):
        assert call(**{k: None}) == INVALID, k
    # a NULL member of every struct: the session's clock, every member of the index, the required arrays of the frame, every output
    for k, _ in capi.SessionState._fields_:
        s2 = _tables(addr)[0]
        setattr(s2, k, None)
        if k in ("first_sample_t", "time"):
            assert call(st=s2) == INVALID, k
    for k, _ in capi.TrailIndexTable._fields_:
        t2 = _tables(addr)[1]
        setattr(t2, k, None)
        assert call(trail=t2) == INVALID, k
    for k, _ in capi.OutputFrame._fields_:
        if k not in OPTIONAL:
            f2 = _tables(addr)[2]
            setattr(f2, k, None)
            assert call(frame=f2) == INVALID, k
    for k, _ in capi.OutputTable._fields_:
        o2 = _tables(addr)[3]
        setattr(o2, k, None)
        assert call(out=o2) == INVALID, k
    # one of the two matrices without the other
    for k in ("slam_to_odometry_dev", "odometry_to_slam_dev"):
        f2 = _tables(addr)[2]
        setattr(f2, k, None)
        assert call(frame=f2) == INVALID, k
    # non-positive sizes
    for k in ("cameraTrailLength", "maxTracks", "maxVisualUpdates"):
        for v in (0, -3):
            assert call(p=capi.output_default_params(**{k: v})) == INVALID, (k, v)
    # the limits are decided without a handle, so UNSUPPORTED (not the NULL handle's INVALID) comes back; the optional arrays absent
    f3 = _tables(addr)[2]
    for k in OPTIONAL:
        setattr(f3, k, None)
    assert call(p=capi.output_default_params(maxVisualUpdates=65), frame=f3) == UNSUPPORTED
    assert call(p=capi.output_default_params(cameraTrailLength=64)) == UNSUPPORTED
    assert call(p=capi.output_default_params(maxVisualUpdates=64, cameraTrailLength=63), frame=f3) == INVALID     # at the limits: supported
    # a call that is both invalid and unsupported is reported as invalid
    assert call(p=capi.output_default_params(maxVisualUpdates=65), out=None) == INVALID
