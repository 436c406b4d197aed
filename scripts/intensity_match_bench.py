#!/usr/bin/env python3
"""Times hv_match_intensities_batch_dev for resident stereo pairs of 752 x 480 (default 1024), both options on
(matchSuccessiveIntensities 0.5, matchStereoIntensities), beside the pyramid build and one stereo LK launch of the same batch in
the same process.

Per region: the frames are restored from a pristine copy (outside the timed events), the call is issued `reps` times and the
HV_K_INGEST events -- one pair around the call's three launches -- give the device time per call; the region is repeated `rounds`
times and every round is reported (the spread). A second loop without the restore gives the host's wall time per call, ending in a
synchronise.

Agreed traffic of one call: 1 byte per pixel read for each histogram, 1 read + 1 written for each rewritten image; with both options
on that is 2 histograms + 2 rewrites = 6 bytes per pixel of a pair. The rate is set beside the HBM ceilings measured in
profiles/r01/hbm_ceiling_measured.txt (16-byte reads, copy) and, like the other stage figures, beside 8 TB/s; `floor_ms` is what the
call would take with its reads at the read ceiling and its rewrites at the copy ceiling.

usage: scripts/intensity_match_bench.py [--sets N] [--reps N] [--rounds N] [--no-tracker] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from hybvio_amd import capi, synth  # noqa: E402

W, H, NPTS = 752, 480, 200
HBM_READ_GBS, HBM_COPY_GBS, HBM_PEAK_GBS = 6509.5, 4746.5, 8000.0            # profiles/r01/hbm_ceiling_measured.txt; the nominal peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-tracker", action="store_true", help="skip the pyramid and LK launches (kernel-trace runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    S = a.sets
    left, right, _ = synth.stereo_sequence(11, W, H, 4)
    base = torch.from_numpy(np.concatenate([left, right])).cuda().float()     # 8 frames
    gains = ((1.0, 0.0), (0.8, 12.0), (1.25, -20.0), (0.55, 40.0), (0.9, 10.0))

    def batch(first):
        out = torch.empty((S, H, W), dtype=torch.uint8, device="cuda")
        for s in range(S):
            g, o = gains[(s // 4 + first) % len(gains)]
            out[s] = (base[first + s % 4] * g + o).round().clamp(0, 255).to(torch.uint8)
        return out

    pristine = (batch(0), batch(4))
    L, Rt = pristine[0].clone(), pristine[1].clone()
    params = capi.intensity_default_params(matchSuccessiveIntensities=0.5, matchStereoIntensities=1)
    pixels = S * W * H
    traffic = 6 * pixels
    floor_ms = (2 * pixels / (HBM_READ_GBS * 1e9) + 4 * pixels / (HBM_COPY_GBS * 1e9)) * 1e3
    res = {"device": torch.cuda.get_device_name(0), "library": os.environ.get("HV_LIB_OVERRIDE", "default"), "sets": S,
           "width": W, "height": H, "reps": a.reps, "agreed_bytes_per_call": traffic, "floor_ms": round(floor_ms, 4), "rounds": []}

    with capi.Context(width=W, height=H, max_tracks=NPTS, pool_size=2 * S, max_pairs=S) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        st = capi.intensity_state(S)
        ctx.intensity_init_batch_dev(S, st.table)
        P = lambda t: t.data_ptr()

        def call():
            ctx.match_intensities_batch_dev(params, S, W, H, P(L), W * H, P(Rt), W * H, W, st.table, 0, P(st.record))

        def restore():
            L.copy_(pristine[0]); Rt.copy_(pristine[1])

        for _ in range(3):                                                    # warm-up; has_prev is set from here on
            restore(); call()
        torch.cuda.synchronize()
        ctx.profile_enable(True)
        if not a.no_tracker:
            slots = torch.arange(2 * S, dtype=torch.int32, device="cuda")
            for _ in range(2 * S):
                ctx.acquire()
            pts = torch.from_numpy(np.tile(synth.grid_points(W, H, NPTS), (S, 1, 1))).cuda()
            nxt = pts.clone()
            status = torch.zeros((S, NPTS), dtype=torch.uint8, device="cuda")
            err = torch.zeros((S, NPTS), dtype=torch.float32, device="cuda")

            def pyramid():
                ctx.build_batch_dev(S, P(slots), P(L), W * H, W)
                ctx.build_batch_dev(S, P(slots) + 4 * S, P(Rt), W * H, W)

            def klt():
                nxt.copy_(pts)
                ctx.klt_track_batch_dev(S, P(slots), P(slots) + 4 * S, NPTS, P(pts), P(nxt), P(status), P(err), use_initial_flow=True)

        for rnd in range(a.rounds):
            row = {"round": rnd}
            ctx.profile_reset()
            for _ in range(a.reps):
                restore(); call()
            ms, n = ctx.profile_read(capi.K_INGEST)
            assert n == a.reps, (n, a.reps)
            per = ms / n
            row["match_event_ms_per_call"] = round(per, 4)
            row["match_GBs_agreed"] = round(traffic / (per * 1e-3) / 1e9, 1)
            row["match_frac_of_floor"] = round(floor_ms / per, 3)
            row["match_frac_of_8TBs"] = round(traffic / (per * 1e-3) / 1e9 / HBM_PEAK_GBS, 3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                call()
            torch.cuda.synchronize()
            row["match_wall_ms_per_call_no_restore"] = round((time.perf_counter() - t0) / a.reps * 1e3, 4)
            if not a.no_tracker:
                restore(); call()
                for fn in (pyramid, klt):
                    fn()
                ctx.profile_reset()
                for _ in range(a.reps):
                    pyramid()
                l0, n0 = ctx.profile_read(capi.K_PYR_L0)
                ln, _ = ctx.profile_read(capi.K_PYR_LN)
                row["pyramid_event_ms_per_batch"] = round((l0 + ln) / a.reps, 4)          # both cameras: two builds
                ctx.profile_reset()
                for _ in range(a.reps):
                    klt()
                k, nk = ctx.profile_read(capi.K_KLT)
                row["klt_stereo_event_ms_per_launch"] = round(k / nk, 4)                   # left -> right, 200 points per pair
                row["tracked_fraction"] = round(float(status.float().mean().item()), 3)
            res["rounds"].append(row)
            print(json.dumps(row), flush=True)
        per = [r["match_event_ms_per_call"] for r in res["rounds"]]
        res["match_event_ms_per_call_median"] = float(np.median(per))
        res["match_event_ms_per_call_min_max"] = [min(per), max(per)]
        flags = [r.flags for r in st.records()]
        res["sets_matched_left_and_right"] = sum(f == 12 for f in flags)
    print(json.dumps({k: v for k, v in res.items() if k != "rounds"}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
