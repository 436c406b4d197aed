#!/usr/bin/env python3
"""One call of every host-pointer entry that stages through hv::Stage, on a small fixed input: prints one JSON line with a SHA-256 of
every entry's output buffers (and of the filter states behind the EKF entries). Run it once per build of the library (HV_LIB_OVERRIDE)
and compare the lines: a refactor of the staging leaves every digest as it was.
usage: scripts/host_staging_ab.py [--out file.json]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from hybvio_amd import capi, synth  # noqa: E402


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def states(g):
    return [x for b in range(g.batch) for x in g.get_state(b)]


def tracker_entries(res):
    w, h, M = 160, 120, 23
    rng = np.random.default_rng(11)
    cam = capi.camera_model("pinhole", 98.0, 97.0, 80.2, 60.4, coeffs=[-0.2834, 0.0740, 0.0])
    T = np.eye(4)
    T[:3, 3] = (-0.1, 0.002, 0.0)
    second_to_first = np.linalg.inv(T)
    left, right, _ = synth.stereo_sequence(7, w, h, 2)
    pts = synth.grid_points(w, h, M).astype(np.float32)
    moved = (pts + [-3.0, 0.0] + rng.normal(0, 0.5, pts.shape)).astype(np.float32)
    right_pts = (pts + [-6.0, 0.0] + rng.normal(0, 0.3, pts.shape)).astype(np.float32)
    pairs = rng.integers(0, M, (100, 2))
    ss, ts = np.zeros(M, np.int32), np.zeros(M, np.int32)
    ss[::7] = 2
    blacklist = (np.arange(M) % 5 == 0).astype(np.uint8)
    with capi.Context(width=w, height=h, levels=2, max_tracks=M, pool_size=2) as ctx:
        s0, s1 = ctx.acquire(), ctx.acquire()
        ctx.build(s0, left[0]); ctx.build(s1, left[1])
        res["klt_track"] = digest(*ctx.klt_track(s0, s1, pts))
        res["klt_track_initial_flow"] = digest(*ctx.klt_track(s0, s1, pts, moved))
        st, R, best, visited = ctx.rot_ransac(pts, moved, cam, cam, pairs, 4e-4)
        res["rot_ransac"] = digest(st, R, np.array([best, visited]))
        res["ransac5"] = digest(*ctx.ransac5(pts, moved, cam, cam))
        rp3 = capi.ransac3_default_params()
        res["ransac3"] = digest(*ctx.ransac3(ts, pts, right_pts, moved, cam, cam, second_to_first, rng.integers(0, 2**32, 3 * rp3.ransac3MaxIterations, dtype=np.uint64)))
        rp2 = capi.upright2p_default_params()
        poses = np.stack([np.eye(4), np.eye(4)]); poses[1, :3, 3] = (0.05, 0.0, 0.01)
        res["upright2p"] = digest(*ctx.upright2p(ts, pts, right_pts, moved, cam, cam, second_to_first, poses,
                                                 rng.integers(0, 2**32, 2 * rp2.ransacStereoUpright2pMaxIterations, dtype=np.uint64)))
        gp = capi.stereo_gate_default_params(cam0ToCam1=T)
        res["track_gate_stereo"] = digest(ctx.track_gate(pts, right_pts, ss, ts, cam, cam, blacklist=blacklist, params=gp))
        res["track_gate_mono"] = digest(ctx.track_gate(pts, None, None, ts, cam, params=gp))
        kept, kept2, st = ctx.detection_filter(pts, right_pts, ss, cam, cam, params=gp)
        res["detection_filter_stereo"] = digest(kept, kept2, st)
        kept, _, st = ctx.detection_filter(pts, None, None, cam, params=gp)
        res["detection_filter_mono"] = digest(kept, st)
        res["corner_subpix"] = digest(*ctx.corner_subpix(s0, pts + 0.3))
        res["gftt_detect"] = digest(ctx.gftt_detect(s0, prev=pts[:5], mask_radius=8))
        ctx.ingest_build(s1, left[0])
        res["ingest_build"] = digest(*ctx.download(s1, 1))
        res["match_intensities"] = digest(ctx.match_intensities(left[0], right[0], 0.7))


def ekf_entries(res):
    rng = np.random.default_rng(12)
    B, trail, npose, K, M = 5, 6, 4, 3, 1
    T1, T2, means, idx, feat = synth.visual_tracks(rng, B, trail, npose, True)
    vel = 0.2 * rng.normal(size=feat.shape)
    n = means.shape[1]

    def spd(dim):
        P = np.zeros((B, dim, dim))
        for b in range(B):
            A = rng.normal(size=(dim, dim)) * 1e-3
            P[b] = np.eye(dim) * 1e-4 + A @ A.T
        return P
    P, Pm = spd(n), spd(n + 3 * M)
    ys = feat.reshape(B, -1) + 2e-3 * rng.normal(size=(B, feat.shape[1] * 2))
    ys[1] += 3.0
    vp = capi.vu_default_params(imu_to_camera=T1, second_imu_to_camera=T2)
    H, v = rng.normal(size=(B, 6, n)), 0.01 * rng.normal(size=(B, 6))
    mask = np.array([1, 0, 1, 1, 0], np.uint8)
    vptr = lambda a: a.ctypes.data_as(C.c_void_p)
    L = capi.lib()

    def fresh(ctx, map_size=0, m=means, cov=P):
        g = capi.EkfBatch(ctx, capi.ekf_default_params(cameraTrailLength=trail, hybridMapSize=map_size), B)
        for b in range(B):
            g.set_state(b, m[b], cov[b])
        return g

    with capi.Context(width=64, height=64, levels=1, pool_size=1) as ctx:
        g = fresh(ctx)
        g.predict(0.005, rng.normal(size=(B, 3)) * 0.1, [0.0, 0.0, 9.8])
        res["ekf_predict"] = digest(*states(g))
        dt, gy, ac = np.full((4, B), 0.005), 0.1 * rng.normal(size=(4, B, 3)), np.array([0, 0, 9.8]) + 0.1 * rng.normal(size=(4, B, 3))
        assert L.hv_ekf_predict_n(g._h, 4, dt.ctypes.data_as(capi.f64p), gy.ctypes.data_as(capi.f64p), ac.ctypes.data_as(capi.f64p)) == 0
        ctx.synchronize()
        res["ekf_predict_n"] = digest(*states(g))
        g.update(H, v, np.full(B, 1e-2), active=mask)
        res["ekf_update"] = digest(*states(g))
        res["ekf_visual_gate"] = digest(*g.visual_gate(H, v, 1.5))
        g.visual_update(H, v, 0.05, active=mask)
        res["ekf_visual_update"] = digest(*states(g))
        g.augment(discarded=np.arange(B) % trail, active=mask)
        res["ekf_augment"] = digest(*states(g))
        d, act = np.ascontiguousarray(np.arange(B) % trail, np.int32), mask
        assert L.hv_ekf_symmetrize_augment(g._h, vptr(d), vptr(act)) == 0
        ctx.synchronize()
        res["ekf_symmetrize_augment"] = digest(*states(g))
        g.undo_augment(active=mask)
        res["ekf_undo_augment"] = digest(*states(g))
        g.close()
        g = fresh(ctx)
        res["ekf_visual_track"] = digest(*g.visual_track(vp, idx, feat, vel, ys, 1.5, 0.05), *states(g))
        g.close()
        g = fresh(ctx)
        fK = np.stack([feat + 1e-3 * k for k in range(K)]); vK = np.stack([vel] * K); iK = np.stack([idx] * K)
        yK = fK.reshape(K, B, -1) + 2e-3 * rng.normal(size=(K, B, feat.shape[1] * 2))
        res["ekf_visual_frame"] = digest(*g.visual_frame(vp, iK, fK, vK, yK, 1.5, 0.05, 2), *states(g))
        g.close()
    mm = np.concatenate([means, rng.normal(size=(B, 3 * M))], axis=1)
    with capi.Context(width=64, height=64, levels=1, pool_size=1) as ctx:
        g = fresh(ctx, M, mm, Pm)
        st, gs = np.full((B, 2), -9, np.int32), np.full(B, -9, np.int32)
        chi, pf = np.zeros(B), np.zeros((B, 3))
        idx32 = np.ascontiguousarray(idx, np.int32)
        f, vl, yy = (np.ascontiguousarray(a, np.float64) for a in (feat, vel, ys))
        offer = np.array([-1, -1, 0, -1, -1], np.int32); upd = np.full(B, -1, np.int32)
        rc = L.hv_ekf_visual_track_hybrid(g._h, C.byref(vp), npose, vptr(idx32), vptr(f), vptr(vl), vptr(yy), vptr(upd), vptr(offer), 1.5, 0.05,
                                          vptr(st), vptr(gs), vptr(chi), vptr(pf))
        assert rc == 0, rc
        res["ekf_visual_track_hybrid"] = digest(st, gs, chi, pf, *states(g))
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"library": os.environ.get("HV_LIB_OVERRIDE", "default")}
    tracker_entries(res)
    ekf_entries(res)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
