"""C++ SubPixelAdjuster adapter (hybvio_amd/host): findKeypoints' detect + sub-pixel refinement on the device pyramid.

CPU part: tests/cpp/test_subpix_adapter.cpp compiles and links with plain g++ against the project's libraries (no HIP
header, no HIP runtime on its link line).
GPU part: the program runs FeatureDetector::buildHip -> SubPixelAdjuster::buildHip on a frame; its corners must equal
ctx.gftt_detect followed by the numpy restatement, bit for bit.
"""
import os
import subprocess

import numpy as np
import pytest

import subpix_restatement as R
from hybvio_amd import build, capi, synth

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_subpix_adapter.cpp")


def _build(out_dir):
    lib, _ = build.build_host()
    libdir = os.path.dirname(lib)
    exe = os.path.join(out_dir, "test_subpix_adapter")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", exe, SRC, "-L" + libdir, "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-lhybvio_host", "-lhybvio_hip"])
    return exe


def test_adapter_program_builds_against_the_c_abi_only(tmp_path):
    exe = _build(str(tmp_path))
    assert os.access(exe, os.X_OK)
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "libhybvio_host.so" in needed and "amdhip64" not in needed


@pytest.mark.gpu
def test_detect_then_subpix_through_the_cpp_adapters(tmp_path):
    exe = _build(str(tmp_path))
    w, h, r = 752, 480, 20
    img = synth.stereo_sequence(31, w, h, 1)[0][0]
    with open(tmp_path / "dims.txt", "w") as f:
        f.write(f"{w} {h} {r}\n")
    img.tofile(str(tmp_path / "img.raw"))
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    det = np.loadtxt(tmp_path / "detected.txt", dtype=np.float32).reshape(-1, 2)
    ref = np.loadtxt(tmp_path / "refined.txt", dtype=np.float32).reshape(-1, 2)
    with capi.Context(width=w, height=h) as ctx:
        s = ctx.acquire()
        ctx.build(s, img)
        want_det = ctx.gftt_detect(s, mask_radius=r)
    assert np.array_equal(det, want_det)
    want, _ = R.corner_subpix(img, want_det)
    assert np.array_equal(ref, want)
    assert not np.array_equal(ref, det)                                  # the refinement moved corners off the grid
