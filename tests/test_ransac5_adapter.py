"""C++ RansacPipeline adapter (hybvio_amd/host): RansacPipeline::buildHip on the hybrid RANSAC2 / RANSAC5 path.

CPU part: tests/cpp/test_ransac5_adapter.cpp compiles and links with plain g++ against the project's libraries (no HIP
header, no HIP runtime on its link line).
GPU part: the program runs compute() over a sequence of frames with one generator; every frame's statuses, result type,
inlier count and score must equal the Python path (hv_rot_ransac with the pipeline's std::mt19937 draws, then
hv_hybrid_ransac_lk_batch_dev), and buildHip must refuse the RANSAC3 and upright 2-point configurations.
"""
import os
import subprocess

import numpy as np
import pytest

import ransac5_restatement as R
from hybvio_amd import build, capi

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_ransac5_adapter.cpp")


def _build(out_dir):
    lib, _ = build.build_host()
    libdir = os.path.dirname(lib)
    exe = os.path.join(out_dir, "test_ransac5_adapter")
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
    assert "hybvio::tracker::RansacPipeline::buildHip" in syms


def _frames(oracle, rng):
    spec = R.CAMERAS["pinhole_radial"]
    ocam = oracle.Camera(spec[0], *spec[1:5], coeffs=spec[5])
    out = []
    for n, outl, scene in ((150, 0.1, "general"), (120, 0.0, "rotation"), (1, 0.0, "general"), (160, 0.25, "general"),
                           (6, 0.0, "general")):
        c1, c2, _, _ = R.make_set(rng, (ocam, spec), n, outl, 0.3, scene)
        extra = rng.integers(3, 9)                                     # features LK lost, interleaved with the tracked ones
        st = np.zeros(n + extra, np.int32)
        st[rng.choice(n + extra, extra, replace=False)] = rng.choice([2, 4], extra)
        a = rng.uniform(0, 700, (n + extra, 2)).astype(np.float32)
        b = a.copy()
        a[st == 0], b[st == 0] = c1, c2
        out.append((a, b, st))
    return spec, out


@pytest.mark.gpu
def test_compute_equals_the_python_path_and_refuses_ransac3(oracle, tmp_path):
    import torch
    exe = _build(str(tmp_path))
    res = subprocess.run([exe, "--refuse"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "useRansac3" in res.stdout and "useStereoUpright2p" in res.stdout, res.stdout + res.stderr

    w, h = 752, 480
    spec, frames = _frames(oracle, np.random.default_rng(17))
    with open(tmp_path / "in.txt", "w") as f:
        co = list(spec[5]) + [0.0] * (4 - len(spec[5]))
        f.write(f"{w} {h} 0 {spec[1]!r} {spec[2]!r} {spec[3]!r} {spec[4]!r} {len(spec[5])} {' '.join(repr(c) for c in co)} 180.0\n")
        f.write(f"{len(frames)}\n")
        for a, b, st in frames:
            f.write(f"{len(st)}\n")
            for i in range(len(st)):
                f.write(f"{float(a[i, 0])!r} {float(a[i, 1])!r} {float(b[i, 0])!r} {float(b[i, 1])!r} {int(st[i])}\n")
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = open(tmp_path / "out.txt").read().split("\n")

    gcam = capi.camera_model(spec[0], *spec[1:5], coeffs=spec[5])
    thr = float(np.float32((4.0 * (min(w, h) / 720.0)) ** 2))                # ransac_pipeline.cpp:91-93
    consumed, types = 0, []
    with capi.Context(width=w, height=h) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        for k, (a, b, st) in enumerate(frames):
            keep = np.nonzero(st == 0)[0]
            N, n = len(st), len(keep)
            r2 = np.full(N, 3, np.int32)
            r2s = np.zeros(2, np.int32)
            if n >= 2:
                draws = oracle.mt19937_draws(4649, 200, skip=consumed)
                pairs = (draws.astype(np.uint64) % np.uint64(n)).astype(np.int32).reshape(100, 2)
                s2, _, best, vis = ctx.rot_ransac(a[keep], b[keep], gcam, gcam, pairs, thr)
                r2[keep], r2s[:] = s2, (best, vis)
                consumed += 2 * vis
            dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
            d_ts = dev(st[None].copy())
            d_res = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
            d_score = torch.zeros(1, dtype=torch.float64, device="cuda")
            keep_alive = [dev(np.array([N], np.int32)), dev(a[None]), dev(b[None]), dev(r2[None]), dev(r2s[None])]
            ctx.hybrid_ransac_lk_batch_dev(1, N, keep_alive[0].data_ptr(), keep_alive[1].data_ptr(), keep_alive[2].data_ptr(),
                                           d_ts.data_ptr(), keep_alive[3].data_ptr(), keep_alive[4].data_ptr(), gcam, gcam,
                                           d_res.data_ptr(), d_score.data_ptr())
            torch.cuda.synchronize()
            typ, cnt, score = lines[2 * k].split()
            assert [int(typ), int(cnt)] == d_res.cpu().numpy()[0].tolist(), k
            assert float(score) == float(d_score.cpu().numpy()[0]), k
            assert np.array_equal(np.array(lines[2 * k + 1].split(), np.int32), d_ts.cpu().numpy()[0]), k
            types.append(int(typ))
    assert {R.TYPE_SKIPPED, R.TYPE_R2, R.TYPE_R5} <= set(types), types
