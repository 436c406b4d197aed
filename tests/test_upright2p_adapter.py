"""C++ RansacPipeline adapter (hybvio_amd/host): buildHipUpright2p, on the stereo upright 2-point branch.

CPU part: tests/cpp/test_upright2p_adapter.cpp compiles and links with plain g++ against the project's libraries (no HIP
header, no HIP runtime on its link line).
GPU part: the program runs compute() with one pipeline over stereo frames with poses (the upright branch), a stereo frame
with null poses and a mono frame (both fall through to the hybrid branch); every frame's statuses, result type, inlier count
and score must equal the Python path (hv_rot_ransac and hv_upright2p fed with the std::mt19937 outputs at the position the
pipeline's generators must have reached). A second pipeline with useRansac3 as well takes the RANSAC3 branch first, and the
two older buildHip overloads still refuse the upright configuration.
"""
import os
import subprocess

import numpy as np
import pytest

import ransac3_restatement as R3
import ransac5_restatement as R5
import upright2p_restatement as U
from hybvio_amd import build, capi

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_upright2p_adapter.cpp")
SEED = 4649                                                             # RansacPipelineParameters::ransacRngSeed
W, H = 752, 480


def _build(out_dir):
    lib, _ = build.build_host()
    libdir = os.path.dirname(lib)
    exe = os.path.join(out_dir, "test_upright2p_adapter")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", exe, SRC, "-L" + libdir, "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-lhybvio_host", "-lhybvio_hip"])
    return exe


def test_adapter_program_builds_against_the_c_abi_only(tmp_path):
    exe = _build(str(tmp_path))
    assert os.access(exe, os.X_OK)
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "libhybvio_host.so" in needed and "amdhip64" not in needed


def _frames(oracle, rng):
    spec = R5.CAMERAS["pinhole_radial"]
    ocam = oracle.Camera(spec[0], *spec[1:5], coeffs=spec[5])
    out = []
    for k, (n, outl, extra, poses) in enumerate(((150, 0.3, (5, 2, 0), 1), (120, 0.6, (3, 0, 0), 1), (1, 0.0, (4, 1, 0), 1), (160, 0.45, (6, 3, 0), 1),
                                                 (80, 0.3, (2, 1, 0), 0), (90, 0.7, (2, 2, 0), 1))):
        d = U.make_set(rng, ocam, n, outl, 1.5, *extra, kind=U.ATTITUDES[k % 4], psi=rng.uniform(-3, 3), tilt_deg=0.1)
        out.append((2, poses, d["poses"], d["prev_left"], d["prev_right"], d["cur_left"], d["status"]))
    c1, c2, _, _ = R5.make_set(rng, (ocam, spec), 100, 0.25, 0.3)      # a mono call on the same pipeline
    out.append((1, 1, out[0][2], c1, np.zeros_like(c1), c2, np.zeros(len(c1), np.int32)))
    return spec, out


def _write(path, spec, use_r3, frames):
    with open(path, "w") as f:
        co = list(spec[5]) + [0.0] * (4 - len(spec[5]))
        f.write(f"{W} {H} 0 {spec[1]!r} {spec[2]!r} {spec[3]!r} {spec[4]!r} {len(spec[5])} {' '.join(repr(c) for c in co)} 180.0\n")
        f.write(" ".join(repr(float(v)) for v in U.SECOND_TO_FIRST) + "\n")
        f.write(f"{use_r3} {len(frames)}\n")
        for cams, have, poses, a, b, c, st in frames:
            f.write(f"{cams} {have} {len(st)}\n" + " ".join(repr(float(v)) for v in poses) + "\n")
            for i in range(len(st)):
                f.write(" ".join(repr(float(v)) for v in (a[i, 0], a[i, 1], b[i, 0], b[i, 1], c[i, 0], c[i, 1])) + f" {int(st[i])}\n")


@pytest.mark.gpu
def test_compute_takes_the_upright_branch_and_equals_the_python_path(oracle, tmp_path):
    import torch
    exe = _build(str(tmp_path))
    res = subprocess.run([exe, "--refuse"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.count("useStereoUpright2p") == 2, res.stdout + res.stderr

    T = U.SECOND_TO_FIRST
    spec, frames = _frames(oracle, np.random.default_rng(29))
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    _write(tmp_path / "a" / "in.txt", spec, 0, frames)
    _write(tmp_path / "b" / "in.txt", spec, 1, frames[:1])              # useRansac3 as well: RANSAC3 comes first (:121-123)
    for sub in ("a", "b"):
        res = subprocess.run([exe, str(tmp_path / sub)], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
    lines = open(tmp_path / "a" / "out.txt").read().split("\n")

    gcam = capi.camera_model(spec[0], *spec[1:5], coeffs=spec[5])
    thr = float(np.float32((4.0 * (min(W, H) / 720.0)) ** 2))               # ransac_pipeline.cpp:91-93
    used2 = used_u = 0                                                      # positions of the two generators
    types = []
    with capi.Context(width=W, height=H) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        for k, (cams, have, poses, a, b, c, st) in enumerate(frames):
            keep = np.nonzero(st == 0)[0]
            N, n = len(st), len(keep)
            r2 = np.full(N, 3, np.int32)
            r2s = np.zeros(2, np.int32)
            if n >= 2:
                draws = oracle.mt19937_draws(SEED, 200, skip=used2)
                pairs = (draws.astype(np.uint64) % np.uint64(n)).astype(np.int32).reshape(100, 2)
                s2, _, best, vis = ctx.rot_ransac(a[keep], c[keep], gcam, gcam, pairs, thr)
                r2[keep], r2s[:] = s2, (best, vis)
                used2 += 2 * vis
            if cams == 2 and have:
                ts, _, sm = ctx.upright2p(st, a, b, c, gcam, gcam, T, poses, oracle.mt19937_draws(SEED, 2 * U.MAX_ITERS, skip=used_u))
                used_u += 2 * int(sm[2])
                done = sm[1] >= 0
                want = [4 if done else 0, int(sm[0]) if done else 0]
                ts = ts if done else np.full(N, 3, np.int32)
                score, size = (float(r2s[0]) / n if n else 0.0), N
            else:
                d_res = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
                d_score = torch.zeros(1, dtype=torch.float64, device="cuda")
                alive = [dev(np.array([N], np.int32)), dev(a[None]), dev(c[None]), dev(r2[None]), dev(r2s[None])]
                d_ts = dev(st[None].copy())
                ctx.hybrid_ransac_lk_batch_dev(1, N, alive[0].data_ptr(), alive[1].data_ptr(), alive[2].data_ptr(), d_ts.data_ptr(),
                                               alive[3].data_ptr(), alive[4].data_ptr(), gcam, gcam, d_res.data_ptr(), d_score.data_ptr())
                torch.cuda.synchronize()
                ts, size, want, score = d_ts.cpu().numpy()[0], n, d_res.cpu().numpy()[0].tolist(), float(d_score.cpu().numpy()[0])
            typ, cnt, isz, sc = lines[2 * k].split()
            assert [int(typ), int(cnt)] == want, (k, typ, cnt, want)
            assert int(isz) == size and float(sc) == score, (k, isz, size, sc, score)
            assert np.array_equal(np.array(lines[2 * k + 1].split(), np.int32), ts), k
            types.append(int(typ))
        # the second pipeline: the same first frame through RANSAC3
        cams, have, poses, a, b, c, st = frames[0]
        _, _, sm3 = ctx.ransac3(st, a, b, c, gcam, gcam, T, oracle.mt19937_draws(SEED, 3 * R3.MAX_ITERS))
        typ, cnt, _, _ = open(tmp_path / "b" / "out.txt").read().split("\n")[0].split()
        assert [int(typ), int(cnt)] == [R3.TYPE_R3, int(sm3[0])]
    assert types[:4] == [4, 4, 0, 4] and types[5] == 4, types
    assert types[4] != 4 and types[6] in (R5.TYPE_R2, R5.TYPE_R5), types    # null poses, mono: the hybrid branch (compared above)
    assert used_u >= 2 * 50 * 4
