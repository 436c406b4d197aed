"""C++ legacy GFTT detector adapter (hybvio_amd/host): FeatureDetector::buildHipGftt, the detect() of featureDetector "GFTT".

CPU part: tests/cpp/test_gftt_legacy_adapter.cpp compiles and links with plain g++ against the project's libraries (no HIP header,
no HIP runtime on its link line), and the host library exports the factory.
GPU part: the program runs buildHipGftt -> detect on a frame with live tracks; its corners must equal the numpy restatement
(tests/gftt_legacy_restatement.py), bit for bit.
"""
import os
import subprocess

import numpy as np
import pytest

import gftt_legacy_cases as K
import gftt_legacy_restatement as R
from hybvio_amd import build, synth

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_gftt_legacy_adapter.cpp")


def _build(out_dir):
    lib, _ = build.build_host()
    libdir = os.path.dirname(lib)
    exe = os.path.join(out_dir, "test_gftt_legacy_adapter")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", exe, SRC, "-L" + libdir, "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-lhybvio_host", "-lhybvio_hip"])
    return exe


def test_adapter_program_builds_against_the_c_abi_only(tmp_path):
    exe = _build(str(tmp_path))
    assert os.access(exe, os.X_OK)
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "libhybvio_host.so" in needed and "amdhip64" not in needed
    lib, _ = build.build_host()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", "-C", lib], text=True)
    assert "hybvio::tracker::FeatureDetector::buildHipGftt" in syms and "hybvio::tracker::FeatureDetector::buildHipFast" in syms


@pytest.mark.gpu
def test_detect_through_the_cpp_adapter(tmp_path):
    exe = _build(str(tmp_path))
    w, h, r, block, quality, md, max_tracks = 320, 240, 12, 3, 0.02, 30.0, 60
    img = synth.stereo_sequence(31, w, h, 1)[0][0]
    prev = K.live_tracks(R.candidates(img, (), 1, block, quality), 4, 40)
    with open(tmp_path / "dims.txt", "w") as f:
        f.write(f"{w} {h} {r} {block} {quality!r} {md!r} {max_tracks} {len(prev)}\n")
    img.tofile(str(tmp_path / "img.raw"))
    prev.tofile(str(tmp_path / "prev.raw"))
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    det = np.loadtxt(tmp_path / "detected.txt", dtype=np.float32).reshape(-1, 2)
    want = R.detect(img, prev, r, block, quality, md, max_tracks)[0]
    assert len(want) == max_tracks and np.array_equal(det, want)
    assert not np.array_equal(want, R.detect(img, (), 1, block, quality, md, max_tracks)[0])     # the mask removed candidates
