"""C++ dense-stereo adapter (hybvio_amd/host): StereoDisparity::buildHip with computeDisparity, getDepth and computePointCloud.

CPU part: tests/cpp/test_stereo_bm_adapter.cpp compiles and links with plain g++ against the project's libraries (no HIP header, no
HIP runtime on its link line), and the host library exports the factory.
GPU part: the program runs buildHip -> computeDisparity -> getDepths -> computePointCloud on two frames' device pyramids; everything
must equal the numpy restatement (tests/stereo_bm_restatement.py), bit for bit.
"""
import os
import subprocess

import numpy as np
import pytest

import stereo_bm_cases as K
import stereo_bm_restatement as R
from hybvio_amd import build

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_stereo_bm_adapter.cpp")


def _build(out_dir):
    lib, _ = build.build_host()
    libdir = os.path.dirname(lib)
    exe = os.path.join(out_dir, "test_stereo_bm_adapter")
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
    assert "amdhip64" not in subprocess.check_output(["readelf", "-d", lib], text=True)      # the host library links the C ABI only
    syms = subprocess.check_output(["nm", "-D", "--defined-only", "-C", lib], text=True)
    assert "hybvio::tracker::StereoDisparity::buildHip" in syms and "hybvio::tracker::StereoDisparity::~StereoDisparity" in syms


@pytest.mark.gpu
def test_disparity_depth_and_cloud_through_the_cpp_adapter(tmp_path):
    exe = _build(str(tmp_path))
    w, h, nd = K.SHAPES[1]
    left, right = K.scenes(w, h, nd)[1]
    want = K.expected(w, h, nd, 1, True)[0]
    q = K.q_matrix(w, h)
    ys, xs = np.nonzero(want >= 16)
    rng = np.random.default_rng(8)
    pick = rng.choice(len(xs), 30, replace=False)
    pts = np.concatenate([np.stack([xs[pick] + 0.4, ys[pick] + 0.7], 1), [[-2.0, 3.0], [w + 1.0, 3.0], [5.0, 5.0]]]).astype(np.float32)
    with open(tmp_path / "dims.txt", "w") as f:
        f.write(f"{w} {h} {nd} 5 {len(pts)}\n")
    left.tofile(str(tmp_path / "left.raw")); right.tofile(str(tmp_path / "right.raw"))
    q.astype(np.float64).tofile(str(tmp_path / "q.raw")); pts.tofile(str(tmp_path / "points.raw"))
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    disp = np.fromfile(tmp_path / "disp.raw", np.int16).reshape(h, w)
    assert np.array_equal(disp, want)
    depth = np.fromfile(tmp_path / "depth.raw", np.float32)
    want_depth = R.track_depths(q, want, pts)
    assert np.array_equal(depth.view(np.uint32), want_depth.view(np.uint32)) and (want_depth > 0).sum() >= 30
    cloud = np.fromfile(tmp_path / "cloud.raw", np.float32).reshape(-1, 3)
    want_cloud = R.point_cloud(q, want, 5)
    assert len(want_cloud) > 50 and np.array_equal(cloud.view(np.uint32), want_cloud.view(np.uint32))
