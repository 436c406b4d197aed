#!/usr/bin/env python3
"""Time of the legacy GFTT detector (hv_gftt_legacy_detect_batch_dev, csrc/gftt_legacy.hip) at the shape a lane set runs: 1024
resident images of 752 x 480 (synthetic frames), radius 30, maxTracks 200, 100 live tracks per image -- and, beside it, of the
GPU-GFTT detector (hv_gftt_detect_batch_dev) and the FAST detector (hv_fast_detect_batch_dev) of ANOTHER tree (the parent commit's,
built in place) on the same images, live tracks and radius. Per call: the event time of the launches (HV_K_GFTT: mask, response and
candidate kernels, or the other detectors' first kernel; HV_K_DETECT_TAIL: the select kernel, or theirs) and a host clock around
`calls` calls ended by a synchronise. A round's figure is the mean over its calls; reported are the median, minimum and maximum over
the rounds.
  --what legacy | gftt | fast   one measurement in this process (--tree DIR: hybvio_amd is imported from DIR; --lib FILE: another
                                build of this tree's library, the A/B of the stored response map against the recomputed response)
  --alternate N --tree DIR [--lib FILE]   N rounds of child processes, legacy, (legacy with FILE,) gftt, fast, alternating; this
                                process opens no device
usage: scripts/gftt_legacy_bench.py --alternate 3 --tree ../parent --lib hybvio_amd/lib/libhybvio_hip_recompute.so \\
       --out profiles/gftt_legacy/gftt_legacy_bench.json"""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
W, H, MAX_TRACKS, FAST_MAX_KP, LEGACY_MAX_KP = 752, 480, 200, 32768, 40000


def algorithmic_bytes(n_cand, w=W, h=H):
    """Bytes per image each legacy GFTT kernel must move, from the shapes (stored-map form): the response kernel reads the image
    once and writes the float map and the mask; the candidate kernel reads both and writes 8 bytes per candidate; the select kernel
    reads the keys once for their range and twice per sorted group (histogram, gather; an upper bound: it stops at maxTracks)."""
    stride = (w + 3) & ~3
    groups = -(-n_cand // 4096)
    return {"image": w * h,
            "legacy_response_kernel": {"read": w * h, "write_map": 4 * w * h, "write_mask": stride * h},
            "legacy_candidates_kernel": {"read_map": 4 * w * h, "read_mask": stride * h, "write_keys": 8 * n_cand},
            "legacy_select_kernel": {"read_keys_upper_bound": 8 * n_cand * (1 + 2 * groups)}}


def measure(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    if a.lib:
        os.environ["HV_LIB_OVERRIDE"] = os.path.abspath(a.lib)
    import torch
    from hybvio_amd import capi, synth
    n, n_prev, radius = a.images, a.n_prev, a.radius
    rng = np.random.default_rng(3)
    left, right, _ = synth.stereo_sequence(11, W, H, 8)
    frames = list(left) + list(right)
    res = {"what": a.what, "tree": a.tree or ".", "library": a.lib or "default", "images": n, "size": [W, H], "radius": radius,
           "maxTracks": MAX_TRACKS, "n_prev": n_prev, "rounds": a.rounds, "calls_per_round": a.calls}
    with capi.Context(width=W, height=H, levels=1, pool_size=n) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        slots = []
        for i in range(n):
            s = ctx.acquire()
            ctx.build(s, frames[i % len(frames)])
            slots.append(s)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        d_slots = dev(np.array(slots, np.int32))
        prev = np.stack([rng.uniform(0, W, (n, max(n_prev, 1))), rng.uniform(0, H, (n, max(n_prev, 1)))], -1).astype(np.float32)
        d_prev, d_nprev, d_radius = dev(prev), dev(np.full(n, n_prev, np.int32)), dev(np.full(n, radius, np.int32))
        d_nout = torch.zeros(n, dtype=torch.int32, device="cuda")
        n_kp = torch.zeros(n, dtype=torch.int32, device="cuda")
        if a.what == "legacy":
            params = capi.gftt_legacy_default_params(maxTracks=MAX_TRACKS)
            work = torch.empty(ctx.gftt_legacy_work_bytes(n, LEGACY_MAX_KP), dtype=torch.uint8, device="cuda")
            corners = torch.empty((n, MAX_TRACKS, 2), dtype=torch.float32, device="cuda")
            resp = torch.empty((n, MAX_TRACKS), dtype=torch.float32, device="cuda")
            call = lambda: ctx.gftt_legacy_detect_batch_dev(n, d_slots.data_ptr(), work.data_ptr(), LEGACY_MAX_KP, n_kp.data_ptr(), n_prev,
                                                            d_nprev.data_ptr(), d_prev.data_ptr(), d_radius.data_ptr(), MAX_TRACKS,
                                                            corners.data_ptr(), resp.data_ptr(), d_nout.data_ptr(), params)
            names = ("mask + response + candidate kernels", "legacy_select_kernel")
        elif a.what == "fast":
            params = capi.fast_default_params(maxTracks=MAX_TRACKS)
            work = torch.empty(ctx.fast_work_bytes(n), dtype=torch.uint8, device="cuda")
            kp = torch.empty((n, FAST_MAX_KP, 3), dtype=torch.float32, device="cuda")
            corners = torch.empty((n, MAX_TRACKS, 2), dtype=torch.float32, device="cuda")
            call = lambda: ctx.fast_detect_batch_dev(n, d_slots.data_ptr(), work.data_ptr(), FAST_MAX_KP, kp.data_ptr(), n_kp.data_ptr(),
                                                     n_prev, d_nprev.data_ptr(), d_prev.data_ptr(), d_radius.data_ptr(), MAX_TRACKS,
                                                     corners.data_ptr(), d_nout.data_ptr(), params)
            names = ("fast_score_kernel", "fast_select_kernel")
        else:
            params = capi.gftt_default_params(maxTracks=MAX_TRACKS)
            nk = ctx.gftt_keypoint_count(params)
            kp = torch.empty((n, nk, 3), dtype=torch.float32, device="cuda")
            mc = 2 * nk
            corners = torch.empty((n, mc, 2), dtype=torch.float32, device="cuda")
            call = lambda: ctx.gftt_detect_batch_dev(n, d_slots.data_ptr(), kp.data_ptr(), n_prev, d_nprev.data_ptr(), d_prev.data_ptr(),
                                                     d_radius.data_ptr(), mc, corners.data_ptr(), d_nout.data_ptr(), params)
            names = ("gftt response kernel", "detect_tail_kernel")
            res["gftt_keypoints_per_image"] = nk
        for _ in range(3):                                                 # warm-up: code objects, first touch
            call()
        ctx.synchronize()
        n_out = d_nout.cpu().numpy()
        assert (n_out > 0).all(), "a set reported an error flag"
        res["corners_per_image_mean"] = float(n_out.mean())
        if a.what == "legacy":
            counts = n_kp.cpu().numpy()
            res["candidates_per_image_mean"] = float(counts.mean())
            res["algorithmic_bytes_per_image"] = algorithmic_bytes(int(counts.mean()))
            # the digest of the results: two builds of the library (stored map, recomputed response) must agree
            c = corners.cpu().numpy()
            res["digest"] = zlib.crc32(b"".join(c[i, :n_out[i]].tobytes() for i in range(n)))
        host = []
        for _ in range(a.rounds):                                          # host clock, profiling off
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call()
            ctx.synchronize()
            host.append(1e6 * (time.perf_counter() - t0) / a.calls / n)
        ctx.profile_enable(True)
        ev = {capi.K_GFTT: [], capi.K_DETECT_TAIL: []}
        for _ in range(a.rounds):
            ctx.profile_reset()
            for _ in range(a.calls):
                call()
            for k in ev:
                ms, launches = ctx.profile_read(k)
                assert launches == a.calls, (k, launches)
                ev[k].append(1e3 * ms / a.calls / n)
        ctx.profile_enable(False)
        stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
        res["us_per_image"] = {"host_clock_per_call": stat(host), names[0]: stat(ev[capi.K_GFTT]), names[1]: stat(ev[capi.K_DETECT_TAIL])}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("legacy", "gftt", "fast"), default="legacy")
    ap.add_argument("--tree", default=None, help="the other commit's tree, built (gftt and fast are measured from it)")
    ap.add_argument("--lib", default=None, help="another build of this tree's library (legacy only)")
    ap.add_argument("--alternate", type=int, default=0)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--n-prev", type=int, default=100, help="live tracks per image (0: no mask boxes)")
    ap.add_argument("--radius", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.alternate:
        assert a.tree, "--alternate needs --tree"
        runs = []
        common = ["--images", str(a.images), "--rounds", str(a.rounds), "--calls", str(a.calls), "--n-prev", str(a.n_prev),
                  "--radius", str(a.radius)]
        legs = [("legacy", [])] + ([("legacy", ["--lib", a.lib])] if a.lib else []) + [("gftt", ["--tree", a.tree]), ("fast", ["--tree", a.tree])]
        for _ in range(a.alternate):
            for what, extra in legs:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--what", what] + extra + common, capture_output=True,
                                     text=True, timeout=600)
                if out.returncode != 0:                                    # nothing more is started on the device
                    sys.stderr.write(out.stdout + out.stderr)
                    sys.exit(out.returncode)
                runs.append(json.loads(out.stdout.strip().splitlines()[-1]))
        res = {"runs": runs}
    else:
        res = measure(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
