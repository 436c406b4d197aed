"""C++ StereoGate adapter (hybvio_amd/host): StereoGate::buildHip, markTrackStatus and filterDetections.

CPU part: tests/cpp/test_stereo_gate_adapter.cpp compiles and links with plain g++ against the project's libraries (no HIP
header, no HIP runtime on its link line).
GPU part: the program gates frames of stereo tracks and filters sets of new corners; every status and every kept pair must
equal the numpy restatement, and buildHip must refuse an image size other than the session's.
"""
import os
import subprocess

import numpy as np
import pytest

import stereo_gate_restatement as G
from hybvio_amd import build

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_stereo_gate_adapter.cpp")


def _build(out_dir):
    lib, _ = build.build_host()
    libdir = os.path.dirname(lib)
    exe = os.path.join(out_dir, "test_stereo_gate_adapter")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", exe, SRC, "-L" + libdir, "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-lhybvio_host", "-lhybvio_hip"])
    return exe


def test_adapter_program_builds_against_the_c_abi_only(tmp_path):
    exe = _build(str(tmp_path))
    assert os.access(exe, os.X_OK)
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "libhybvio_host.so" in needed and "amdhip64" not in needed
    syms = subprocess.check_output(["nm", "-D", "--defined-only", "-C", build.build_host()[0]], text=True)
    assert "hybvio::tracker::StereoGate::buildHip" in syms


@pytest.mark.gpu
def test_mark_and_filter_equal_the_restatement(oracle, tmp_path):
    exe = _build(str(tmp_path))
    res = subprocess.run([exe, "--refuse"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "image size" in res.stdout, res.stdout + res.stderr

    w, h = 752, 480
    spec = ("pinhole", 395.0, 398.0, 370.0, 236.0, (-0.25, 0.07, 0.0), 180.0)
    ocam = oracle.Camera(spec[0], *spec[1:5], coeffs=spec[5])
    T = np.eye(4)
    T[:3, 3] = (-0.1, 0.02, 0.0)
    prm = G.Params(partOfImageToDetectFeatures=0.9, cam0ToCam1=T)
    rng = np.random.default_rng(8)

    def pairs(n):
        left = rng.uniform([0, 0], [w, h], (n, 2)).astype(np.float32)
        right = left - np.array([20, 0], np.float32) + rng.normal(0, 3, (n, 2)).astype(np.float32)
        right[rng.random(n) < 0.15] += np.float32(25)
        return left, right

    frames, sets = [], []
    for n in (150, 1, 200):
        left, right = pairs(n)
        frames.append((left, right, rng.choice([0, 0, 0, 0, 2, 4], n), rng.choice([0, 0, 0, 0, 2, 3, 4], n), rng.random(n) < 0.05))
    for n in (120, 3, 300):
        left, right = pairs(n)
        sets.append((left, right, rng.choice([0, 0, 0, 0, 2, 4], n)))
    with open(tmp_path / "in.txt", "w") as f:
        co = list(spec[5]) + [0.0] * (4 - len(spec[5]))
        f.write(f"{w} {h} 0 {spec[1]!r} {spec[2]!r} {spec[3]!r} {spec[4]!r} {len(spec[5])} {' '.join(repr(c) for c in co)} 180.0\n")
        f.write(" ".join(repr(float(x)) for x in T.reshape(16)) + f" {prm.maxStereoEpipolarDistance!r} {prm.partOfImageToDetectFeatures!r} 0 0\n")
        f.write(f"{len(frames)}\n")
        for left, right, ss, ts, bl in frames:
            f.write(f"{len(left)}\n")
            for i in range(len(left)):
                f.write(f"{float(left[i, 0])!r} {float(left[i, 1])!r} {float(right[i, 0])!r} {float(right[i, 1])!r} {ss[i]} {ts[i]} {int(bl[i])}\n")
        f.write(f"{len(sets)}\n")
        for left, right, ss in sets:
            f.write(f"{len(left)}\n")
            for i in range(len(left)):
                f.write(f"{float(left[i, 0])!r} {float(left[i, 1])!r} {float(right[i, 0])!r} {float(right[i, 1])!r} {ss[i]}\n")
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = open(tmp_path / "out.txt").read().split("\n")
    seen = set()
    for k, (left, right, ss, ts, bl) in enumerate(frames):
        want = G.track_gate(left, right, ss, bl, ts, ocam, ocam, w, h, prm)
        assert np.array_equal(np.array(lines[k].split(), np.int32), want), k
        seen |= set(want.tolist())
    assert {G.TRACKED, G.FAILED_FLOW, G.FAILED_EPIPOLAR_CHECK, G.OUT_OF_RANGE, G.BLACKLISTED} <= seen, seen
    pos = len(frames)
    for left, right, ss in sets:
        kl, kr, _ = G.detection_filter(left, right, ss, ocam, ocam, w, h, prm)
        m = int(lines[pos])
        got = np.array(lines[pos + 1].split(), np.float32).reshape(-1, 4)
        assert m == len(kl) and np.array_equal(got[:, :2], kl) and np.array_equal(got[:, 2:], kr)
        pos += 2
