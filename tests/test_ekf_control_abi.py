"""C ABI of the EKF control entries (no GPU needed: symbols, defaults, and the argument checks that come before any device
work)."""
import ctypes as C

from hybvio_amd import capi

NEW = ("hv_ekf_block_update_dev", "hv_ekf_pseudo_velocity_dev", "hv_ekf_undo_augment_dev", "hv_ekf_control_default_params",
       "hv_ekf_control_init_dev", "hv_ekf_imu_control_dev", "hv_ekf_frame_control_dev")


def test_control_symbols_defaults_and_abi_version():
    L = capi.lib()
    for s in NEW:
        assert hasattr(L, s), s
        assert s in capi.PROTOTYPES, s
    p = capi.ekf_control_default_params()
    # codegen/parameter_definitions.c:87-119
    assert (p.useDecayingZeroVelocityUpdate, p.usePseudoVelocity, p.pseudoVelocityLimit, p.pseudoVelocityTarget, p.pseudoVelocityR,
            p.useVisualStationarity, p.visualStationarityFrameCountThreshold, p.visualZuptR) == (0, 0, 1.4, 0.0, 1e-4, 1, 3, 1e-7)
    assert L.hv_abi_version() == 4
    assert capi.K_EKF_CONTROL == 18 and capi.K_RANSAC3 == 17
    assert L.hv_profile_read(None, capi.K_EKF_CONTROL, None, None) == -1          # (no context; the id itself is in range)
    L.hv_ekf_control_default_params(None)                                         # a NULL pointer is ignored


def test_the_restatement_has_the_same_defaults():
    import ekf_control_restatement as R
    p, r = capi.ekf_control_default_params(), R.Params()
    for k, _ in capi.EkfControlParams._fields_:
        assert getattr(p, k) == getattr(r, k), k


def test_control_entries_reject_null_arguments_before_any_device_work():
    L = capi.lib()
    p = capi.ekf_control_default_params()
    buf = (C.c_double * 4)()
    addr = C.addressof(buf)
    full = capi.EkfControlTable(addr, addr, addr, addr)
    assert L.hv_ekf_block_update_dev(None, 3, 3, None, None, 1e-7, None, 0, None) == -1
    assert L.hv_ekf_pseudo_velocity_dev(None, 1.4, 0.0, 1e-4, None, None) == -1
    assert L.hv_ekf_undo_augment_dev(None, None) == -1
    assert L.hv_ekf_control_init_dev(None, C.byref(full)) == -1
    assert L.hv_ekf_imu_control_dev(None, C.byref(p), C.byref(full), addr, None) == -1
    assert L.hv_ekf_frame_control_dev(None, C.byref(p), C.byref(full), addr, addr, None, None, None, None, None) == -1
    assert L.hv_ekf_control_init_dev(None, None) == -1
    for k, _ in capi.EkfControlTable._fields_:
        t = capi.EkfControlTable(addr, addr, addr, addr)
        setattr(t, k, None)
        assert L.hv_ekf_control_init_dev(None, C.byref(t)) == -1, k
        assert L.hv_ekf_imu_control_dev(None, C.byref(p), C.byref(t), addr, None) == -1, k
        assert L.hv_ekf_frame_control_dev(None, C.byref(p), C.byref(t), addr, addr, None, None, None, None, None) == -1, k
