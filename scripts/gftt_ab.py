#!/usr/bin/env python3
"""The f1_gftt measurement of bench.py on its own: the hipEvent class K_GFTT over 20 launches of the detector on the B left
images of the tracker leg, after 3 warm launches, plus a digest of the key points. One library per process; for an A/B run
it once per library with HV_LIB_OVERRIDE set, alternating, and compare the digests.
usage: gftt_ab.py [B] [launches]"""
import hashlib, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import bench
from hybvio_amd import capi

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
N = int(sys.argv[2]) if len(sys.argv) > 2 else 20
tb = bench.TrackerBench(B, 0, seed=0)
for _ in range(2):
    tb.step()
torch.cuda.synchronize()
nk = tb.ctx.gftt_keypoint_count()
kp = torch.zeros((B, nk, 3), dtype=torch.float32, device="cuda:0")
left_slots = tb.L[(tb.k - 1) % 2]
for _ in range(3):
    tb.ctx.gftt_keypoints_batch_dev(B, left_slots.data_ptr(), kp.data_ptr())
tb.ctx.profile_enable(True)
tb.ctx.profile_reset()
for _ in range(N):
    tb.ctx.gftt_keypoints_batch_dev(B, left_slots.data_ptr(), kp.data_ptr())
ms, n = tb.ctx.profile_read(capi.K_GFTT)
tb.ctx.profile_enable(False)
torch.cuda.synchronize()
print(json.dumps({"library": os.environ.get("HV_LIB_OVERRIDE", "default"), "images": B, "launches": n, "us_per_launch": 1e3 * ms / n,
                  "blocks_with_a_corner": float((kp[:, :, 2] > 0).float().mean().item()),
                  "keypoints_sha1": hashlib.sha1(kp.cpu().numpy().tobytes()).hexdigest()}))
