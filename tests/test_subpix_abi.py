"""CPU checks of the sub-pixel refinement entries (added within ABI 4): exported symbols, defaults, argument checks that are
decided on the host, the kernel timer class number, and the C++ adapter's export from libhybvio_host.so."""
import ctypes as C
import subprocess

from hybvio_amd import build, capi


def test_subpix_symbols_defaults_and_abi_version():
    L = capi.lib()
    for s in ("hv_subpix_default_params", "hv_corner_subpix", "hv_corner_subpix_batch_dev"):
        assert hasattr(L, s), s
    p = capi.subpix_default_params()
    assert (p.subPixWindowSize, p.subPixMaxIter, p.subPixEpsilon) == (10, 20, 0.03)   # parameter_definitions.c:328-332
    assert L.hv_abi_version() == 4
    assert capi.K_SUBPIX == 12 and capi.SUBPIX_MAX_WIN == 16


def test_subpix_entries_reject_bad_arguments_before_any_device_work():
    L = capi.lib()
    p = capi.subpix_default_params()
    xy = (C.c_float * 2)()
    assert L.hv_corner_subpix(None, C.byref(p), 0, 1, xy, None) == -1
    assert L.hv_corner_subpix_batch_dev(None, C.byref(p), 1, None, 4, None, None, None) == -1


def test_host_adapter_exports_subpixel_adjuster_and_links_only_the_c_abi():
    lib, _ = build.build_host()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", "-C", lib], text=True)
    assert "hybvio::tracker::SubPixelAdjuster::buildHip" in syms
    needed = subprocess.check_output(["readelf", "-d", lib], text=True)
    assert "libhybvio_hip.so" in needed and "amdhip64" not in needed
