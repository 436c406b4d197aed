"""Border, straddling-wave, threshold and tie cases of the GFTT detector against oracle/gftt_oracle.c, bit for bit, through both
kernels: shapes at which every block touches a border, waves straddle images and block rows, the last strip's 8-byte row
segment crosses the image width; images that leave blocks on either side of min_response and that hold exactly equal maxima
inside a block (the comparison then pins the raster tie order of the column-wise arg-max)."""
import numpy as np
import pytest

from hybvio_amd import capi

pytestmark = pytest.mark.gpu

GFTT_TILED = {"marching": 0, "tiled": 1}     # HV_GFTT_TILED, read in hv_create
MIN_DISTANCE = {8: 8.0, 16: 20.0, 32: 50.0}
SHAPES = [(64, 64, 32),      # every block touches a border; a wave holds two images
          (35, 72, 8),       # the right edge mirrors; waves straddle images and block rows
          (40, 33, 16),      # the last strip's 8-byte segment crosses w
          (37, 41, 8),       # ragged in both directions
          (8, 8, 8),         # a single block (an image below the LK window: a context of one level, no tracking on it)
          (32, 32, 32)]      # a single block of 32
KINDS = ["uniform", "binary", "flat", "low_contrast", "periodic"]
_REF = {}


def _images(kind, h, w):
    rng = np.random.default_rng(1000 * h + w + 7 * KINDS.index(kind))
    out = []
    for _ in range(3):
        if kind == "uniform":
            im = rng.integers(0, 256, (h, w), dtype=np.uint8)
        elif kind == "binary":
            im = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
        elif kind == "flat":
            im = np.full((h, w), 90, np.uint8)
        elif kind == "low_contrast":
            im = (100 + rng.integers(0, 6, (h, w))).astype(np.uint8)
        else:
            im = np.tile(rng.integers(0, 256, (4, 4), dtype=np.uint8), ((h + 3) // 4, (w + 3) // 4))[:h, :w]
        out.append(np.ascontiguousarray(im))
    return out


def _case(oracle, kind, shape):
    """images, per-image response maps and reference key points of a case: computed once, shared by both kernels"""
    key = (kind, shape)
    if key not in _REF:
        h, w, bs = shape
        imgs = _images(kind, h, w)
        resp = [oracle.corner_min_eigen_val(im) for im in imgs]
        _REF[key] = (imgs, resp, [oracle.gftt_collect_max(r, bs, 1e-3) for r in resp])
    return _REF[key]


def _tied_blocks(resp, bs):
    """blocks whose maximum is reached at two or more pixels and passes min_response (1e-3 on 16 * response)"""
    h, w = resp.shape
    n = 0
    for yb in range(h // bs):
        for xb in range(w // bs):
            blk = resp[yb * bs:(yb + 1) * bs, xb * bs:(xb + 1) * bs]
            n += int((blk == blk.max()).sum() >= 2 and blk.max() * np.float32(16) > np.float32(1e-3))
    return n


@pytest.mark.parametrize("kernel", ["marching", "tiled"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_edge_shapes_bit_exact(oracle, shape, kind, kernel, monkeypatch):
    import torch
    monkeypatch.setenv("HV_GFTT_TILED", str(GFTT_TILED[kernel]))
    h, w, bs = shape
    imgs, _, refs = _case(oracle, kind, shape)
    gp = capi.gftt_default_params(gfttMinDistance=MIN_DISTANCE[bs])
    assert oracle.gftt_block_size(MIN_DISTANCE[bs]) == bs
    with capi.Context(width=w, height=h, pool_size=3) as ctx:
        slots = []
        for im in imgs:
            s = ctx.acquire(); ctx.build(s, im); slots.append(s)
        nk = ctx.gftt_keypoint_count(gp)
        sl = torch.tensor(slots, dtype=torch.int32, device="cuda")
        kp = torch.full((3, nk, 3), -7.0, dtype=torch.float32, device="cuda")
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.gftt_keypoints_batch_dev(3, sl.data_ptr(), kp.data_ptr(), gp)
        torch.cuda.synchronize()
        got = kp.cpu().numpy()
    for i in range(3):
        assert got[i].shape == refs[i].shape
        assert np.array_equal(got[i], refs[i]), (i, np.nonzero((got[i] != refs[i]).any(1))[0][:5])
    if kind == "flat":
        assert all((r == np.array([0, 0, -1e10], np.float32)).all() for r in refs)       # no corner anywhere


def test_references_hold_the_cases_they_are_there_for(oracle):
    """no GPU work: the low-contrast images leave blocks on both sides of the threshold, the periodic ones tie in every shape"""
    over = under = 0
    for shape in SHAPES:
        for ref in _case(oracle, "low_contrast", shape)[2]:
            over += int((ref[:, 2] > 0).sum()); under += int((ref[:, 2] < 0).sum())
    assert over >= 1 and under >= 1, (over, under)
    for shape in SHAPES:
        if shape in ((8, 8, 8), (32, 32, 32)):               # one block: its border rows mirror, the periodic maxima need not tie
            continue
        _, resp, _ = _case(oracle, "periodic", shape)
        assert sum(_tied_blocks(r, shape[2]) for r in resp) >= 1, shape
