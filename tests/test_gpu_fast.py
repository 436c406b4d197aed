"""hv_fast_keypoints_batch_dev / hv_fast_detect_batch_dev / hv_fast_detect on the MI355X against the numpy restatement of the
reference's FAST path (tests/fast_restatement.py): full equality of counts, order and float bits of (x, y, score) and of the
corners, no case excluded, no tolerance. Sizes: the smallest a context holds, an odd one that is no multiple of any tile, and
752 x 480 (more key points than the GPU-GFTT tail's 16 384); the hand-built images of the CPU test across the score kernel's tile
seams; the device-side error flags with sentinel rows; the batched form against the synchronous one, eager and replayed from a
captured HIP graph; and the sub-pixel + stereo LK chain the corners feed."""
import functools

import numpy as np
import pytest

import fast_cases as K
import fast_restatement as R
from hybvio_amd import capi, synth

pytestmark = pytest.mark.gpu

SIZES = [(33, 33), (97, 130), (752, 480)]
IDS = [f"{w}x{h}" for w, h in SIZES]
SENTINEL = -77.0


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _images(w, h):
    return K.seeded_images(w, h)


@functools.lru_cache(maxsize=None)
def _want_keypoints(w, h, k, t):
    kp = R.keypoints(_images(w, h)[k], t)
    kp.setflags(write=False)
    return kp


def _levels(w, h):
    return 1 if min(w, h) < 64 else 4


class Dev:
    """The device arrays of one batched call, pre-filled with a sentinel."""

    def __init__(self, ctx, slots, max_kp, max_prev=0, prevs=None, radii=None, max_corners=0):
        import torch
        self.torch, self.ctx, self.n, self.max_kp, self.max_prev, self.max_corners = torch, ctx, len(slots), max_kp, max_prev, max_corners
        n = self.n
        self.slots = torch.tensor(list(slots), dtype=torch.int32, device="cuda")
        self.work = torch.empty(max(ctx.fast_work_bytes(n), 16), dtype=torch.uint8, device="cuda")
        self.kp = torch.full((n, max(max_kp, 1), 3), SENTINEL, dtype=torch.float32, device="cuda")
        self.n_kp = torch.full((n,), -99, dtype=torch.int32, device="cuda")
        self.corners = torch.full((n, max(max_corners, 1), 2), SENTINEL, dtype=torch.float32, device="cuda")
        self.n_out = torch.full((n,), -99, dtype=torch.int32, device="cuda")
        pv = np.zeros((n, max(max_prev, 1), 2), np.float32)
        npv = np.zeros(n, np.int32)
        for i, p in enumerate(prevs or []):
            p = np.asarray(p, np.float32).reshape(-1, 2)
            pv[i, :len(p)] = p
            npv[i] = len(p)
        self.prev, self.n_prev = torch.from_numpy(pv).cuda(), torch.from_numpy(npv).cuda()
        self.radius = torch.tensor(list(radii) if radii is not None else [1] * n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def reset(self):
        self.kp.fill_(SENTINEL); self.corners.fill_(SENTINEL); self.n_kp.fill_(-99); self.n_out.fill_(-99)

    def keypoints(self, params):
        self.ctx.fast_keypoints_batch_dev(self.n, self.slots.data_ptr(), self.work.data_ptr(), self.max_kp, self.kp.data_ptr(),
                                          self.n_kp.data_ptr(), params)

    def detect(self, params):
        self.ctx.fast_detect_batch_dev(self.n, self.slots.data_ptr(), self.work.data_ptr(), self.max_kp, self.kp.data_ptr(),
                                       self.n_kp.data_ptr(), self.max_prev, self.n_prev.data_ptr() if self.max_prev else 0,
                                       self.prev.data_ptr() if self.max_prev else 0, self.radius.data_ptr(), self.max_corners,
                                       self.corners.data_ptr(), self.n_out.data_ptr(), params)

    def read(self):
        self.ctx.synchronize()
        return self.kp.cpu().numpy(), self.n_kp.cpu().numpy(), self.corners.cpu().numpy(), self.n_out.cpu().numpy()


def _build_all(ctx, imgs):
    slots = [ctx.acquire() for _ in imgs]
    for s, im in zip(slots, imgs):
        ctx.build(s, im)
    return slots


def _check_rows(got, n_got, want, what):
    """Row i of got holds exactly want[i] and sentinels behind it."""
    for i, wnt in enumerate(want):
        assert n_got[i] == len(wnt), (what, i, n_got[i], len(wnt))
        if not _bits_equal(got[i, :len(wnt)], wnt):
            bad = np.nonzero((got[i, :len(wnt)] != wnt).any(1))[0]
            raise AssertionError((what, i, bad[:5], got[i, bad[:5]], wnt[bad[:5]]))
        assert (got[i, len(wnt):] == SENTINEL).all(), (what, i)


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_keypoints_equal_the_restatement(size):
    w, h = size
    imgs = _images(w, h)
    with capi.Context(width=w, height=h, levels=_levels(w, h), pool_size=3) as ctx:
        slots = _build_all(ctx, imgs)
        bound = ctx.fast_keypoint_bound()
        assert bound == ((w - 5) // 2) * ((h - 5) // 2)
        d = Dev(ctx, slots, bound)
        for t in (10, 0, 40, 255):
            d.reset()
            d.keypoints(capi.fast_default_params(threshold=t))
            kp, n_kp, _, _ = d.read()
            want = [_want_keypoints(w, h, k, t) for k in range(3)]
            _check_rows(kp, n_kp, want, ("threshold", t))
            if t == 10:
                assert all(len(x) > 0 for x in want) and all(len(np.unique(x[:, 2])) < len(x) for x in want)     # key points and ties
            if t == 255:
                assert all(len(x) == 0 for x in want)


def test_hand_built_images_across_the_tile_seams():
    # (the slot is tile_w + 32 wide, 96 x 64 at a 64 x 16 tile: a 64 x 64 slot would hold no vertical seam of a 64-wide tile)
    tw, th = capi.fast_tile_size()                       # the kernel's own constants: the cases move with them
    w, h = tw + 32, max(64, 2 * th + 32)
    cases = K.hand_images(10)
    imgs, tags = [], []
    for name, (img, bg, score) in cases.items():
        for cx in (tw - 1, tw):                          # the pixel under test in the last column of a tile, and the first of the next
            for cy in (th - 1, th, 2 * th - 1, 2 * th):
                imgs.append(K.embed(img, bg, w, h, cx, cy))
                tags.append((name, cx, cy, score))
    with capi.Context(width=w, height=h, levels=1, pool_size=len(imgs)) as ctx:
        slots = _build_all(ctx, imgs)
        d = Dev(ctx, slots, ctx.fast_keypoint_bound())
        d.keypoints(capi.fast_default_params())
        kp, n_kp, _, _ = d.read()
        want = [R.keypoints(im, 10) for im in imgs]
        _check_rows(kp, n_kp, want, "hand-built")
        for (name, cx, cy, score), got in zip(tags, want):
            here = [row for row in got.tolist() if row[:2] == [cx, cy]]
            if score == 0 or name.endswith("_equal"):
                assert here == [], (name, cx, cy)
            elif name in ("single_dot", "255_in_zero", "zero_in_255"):
                assert here == [[cx, cy, score]], (name, cx, cy)


def _prev_lists(w, h, kp, seed):
    """No live tracks; up to 150 tracked points near key points (fractional, so (int) matters); corners that draw nothing."""
    return [np.zeros((0, 2), np.float32), K.golden_prev(w, h, kp, seed), K.OUT_OF_RANGE_PREV(w, h)]


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_detect_equals_the_restatement(size):
    w, h = size
    imgs = _images(w, h)
    radii = (2, 7, 30)
    sets = []                                            # (image, radius, previous corners)
    for k in range(3):
        prevs = _prev_lists(w, h, _want_keypoints(w, h, k, 10), k)
        for j, r in enumerate(radii):
            # every combination at the small sizes; at 752 x 480 each image meets each radius and each list once
            for q in (range(3) if w * h < 100000 else [(k + j) % 3]):
                sets.append((k, r, prevs[q]))
    # boxes wider than one tile and than 32 dwords: the reference's maskRadius runs up to round(1.3^5 * 480 * 0.0667) = 119 at
    # 752 x 480 (tracker.cpp:561-576); few tracks, so that key points are left, one box clipped at each edge of the image
    edge = np.array([[w - 10.5, h * 0.4], [9.25, h * 0.6], [w * 0.5, 3.5], [w * 0.3, h - 2.5], [w * 0.7, h * 0.5]], np.float32)
    for k, r in ((0, 70), (1, 119), (2, 63), (0, 64)):
        sets.append((k, r, edge if r > 64 else np.concatenate([edge, _prev_lists(w, h, _want_keypoints(w, h, k, 10), 7)[1][:20]])))
    want = [R.detect(imgs[k], pv, r, 10, 4096, kp=_want_keypoints(w, h, k, 10)) for k, r, pv in sets]
    if w == 752:
        wide = [(c, srt) for (c, srt), (_, r, _) in zip(want, sets) if r >= 63]
        assert len(wide) == 4 and all(len(c) > 0 and len(srt) > 100 for c, srt in wide)      # the boxes leave key points to choose from
    with capi.Context(width=w, height=h, levels=_levels(w, h), pool_size=3) as ctx:
        slots = _build_all(ctx, imgs)
        bound = ctx.fast_keypoint_bound()
        for max_tracks in (5, 200, 4096):
            cap = min(max_tracks, bound)
            d = Dev(ctx, [slots[k] for k, _, _ in sets], bound, 150, [pv for _, _, pv in sets], [r for _, r, _ in sets], cap)
            d.detect(capi.fast_default_params(maxTracks=max_tracks))
            kp, n_kp, corners, n_out = d.read()
            capped = [c if max_tracks == 4096 else R.min_distance(srt[:, :2], r, max_tracks) for (c, srt), (_, r, _) in zip(want, sets)]
            assert all(_bits_equal(x, c[:max_tracks]) for x, (c, _) in zip(capped, want))        # the cap cuts the uncapped walk
            _check_rows(corners, n_out, capped, ("corners", max_tracks))
            _check_rows(kp, n_kp, [s for _, s in want], ("masked, sorted key points", max_tracks))
        assert any(len(c) > 200 for c, _ in want) or w * h < 10000
        # the synchronous form
        for i in (0, len(sets) // 2, len(sets) - 1):
            k, r, pv = sets[i]
            assert _bits_equal(ctx.fast_detect(slots[k], pv, r), want[i][0][:200])


def test_device_side_error_flags_leave_their_rows_untouched():
    w, h = 97, 130
    imgs = _images(w, h)
    with capi.Context(width=w, height=h, levels=1, pool_size=4) as ctx:
        slots = _build_all(ctx, imgs)
        empty = ctx.acquire()                            # in use, but no image was ever built in it
        bound = ctx.fast_keypoint_bound()
        radii = [30, 0, 7, -1, 2, 5, 5, 5]
        which = [0, 1, 2, 0, 1, 2, 0, 1]
        set_slots = [slots[k] for k in which]
        set_slots[5], set_slots[6], set_slots[7] = 99, -1, empty             # not a slot, not a slot, no image
        d = Dev(ctx, set_slots, bound, 0, None, radii, 200)
        d.detect(capi.fast_default_params())
        kp, n_kp, corners, n_out = d.read()
        for i, (k, r) in enumerate(zip(which, radii)):
            if r < 1 or i >= 5:
                assert n_kp[i] == -1 and n_out[i] == -1
                assert (kp[i] == SENTINEL).all() and (corners[i] == SENTINEL).all()
            else:
                c, s = R.detect(imgs[k], [], r, 10, 200, kp=_want_keypoints(w, h, k, 10))
                _check_rows(corners[i:i + 1], n_out[i:i + 1], [c], i)
                _check_rows(kp[i:i + 1], n_kp[i:i + 1], [s], i)
        d2 = Dev(ctx, set_slots, bound)
        d2.keypoints(capi.fast_default_params())
        kp, n_kp, _, _ = d2.read()
        assert list(n_kp[5:]) == [-1, -1, -1] and (kp[5:] == SENTINEL).all()
        _check_rows(kp[:5], n_kp[:5], [_want_keypoints(w, h, k, 10) for k in which[:5]], "keypoints")
        # counts read from device memory are clamped to their capacity
        pv = _prev_lists(w, h, _want_keypoints(w, h, 0, 10), 5)[1][:40]
        d3 = Dev(ctx, [slots[0], slots[0]], bound, 40, [pv, pv], [7, 7], 200)
        d3.n_prev.copy_(d3.torch.tensor([1000, -5], dtype=d3.torch.int32))
        d3.detect(capi.fast_default_params())
        kp, n_kp, corners, n_out = d3.read()
        for i, p in enumerate((pv, [])):
            c, s = R.detect(imgs[0], p, 7, 10, 200, kp=_want_keypoints(w, h, 0, 10))
            _check_rows(corners[i:i + 1], n_out[i:i + 1], [c], ("clamped", i))
        with pytest.raises(capi.HvError):
            ctx.fast_detect(empty)                       # HV_ERR_POOL: the slot holds no image


def test_more_key_points_than_the_capacity_are_reported_never_truncated():
    w, h = 752, 480
    frame = _images(w, h)[0]
    want_kp = _want_keypoints(w, h, 0, 10)
    assert len(want_kp) > capi.DETECT_TAIL_MAX_KEYPOINTS
    with capi.Context(width=w, height=h, pool_size=1) as ctx:
        slots = _build_all(ctx, [frame])
        d = Dev(ctx, slots, 16384, 0, None, [30], 200)
        d.detect(capi.fast_default_params())
        kp, n_kp, corners, n_out = d.read()
        assert n_kp[0] == -1 and n_out[0] == -1 and (kp == SENTINEL).all() and (corners == SENTINEL).all()
        d.reset()
        d.keypoints(capi.fast_default_params())
        kp, n_kp, _, _ = d.read()
        assert n_kp[0] == -1 and (kp == SENTINEL).all()
        d = Dev(ctx, slots, ctx.fast_keypoint_bound(), 0, None, [30], 200)
        d.detect(capi.fast_default_params())
        kp, n_kp, corners, n_out = d.read()
        c, s = R.detect(frame, [], 30, 10, 200, kp=want_kp)
        _check_rows(corners, n_out, [c], "bound")
        _check_rows(kp, n_kp, [s], "bound")
        # exactly enough room is enough
        d = Dev(ctx, slots, len(want_kp))
        d.keypoints(capi.fast_default_params())
        kp, n_kp, _, _ = d.read()
        _check_rows(kp, n_kp, [want_kp], "exact capacity")


def test_batch_matches_the_synchronous_form_eager_and_graph_replayed():
    import torch
    w, h = 752, 480
    left, right, _ = synth.stereo_sequence(5, w, h, 2)
    frames = [left[0], left[1], right[0], _images(w, h)[2]]
    n_sets, max_prev = 48, 150
    rng = np.random.default_rng(9)
    with capi.Context(width=w, height=h, pool_size=len(frames)) as ctx:
        slots = _build_all(ctx, frames)
        which = rng.integers(0, len(frames), n_sets)
        radii = rng.choice([2, 7, 30, 55], n_sets)
        prevs = [np.stack([rng.uniform(-5, w + 5, m), rng.uniform(-5, h + 5, m)], 1).astype(np.float32)
                 for m in rng.integers(0, max_prev + 1, n_sets)]
        params = capi.fast_default_params()
        want = [ctx.fast_detect(slots[k], pv, int(r), params) for k, pv, r in zip(which, prevs, radii)]
        assert all(len(c) > 0 for c in want)
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        d = Dev(ctx, [slots[k] for k in which], 40000, max_prev, prevs, radii, 200)
        d.detect(params)
        kp, n_kp, corners, n_out = d.read()
        _check_rows(corners, n_out, want, "eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            d.detect(params)
        for _ in range(2):
            with torch.cuda.stream(stream):
                d.reset()
                g.replay()
            stream.synchronize()
            kp2, n_kp2, corners2, n_out2 = d.read()
            assert np.array_equal(n_kp2, n_kp) and np.array_equal(n_out2, n_out) and _bits_equal(kp2, kp) and _bits_equal(corners2, corners)
        del g


def test_profile_classes_count_the_two_launches():
    w, h = 97, 130
    with capi.Context(width=w, height=h, levels=1, pool_size=1) as ctx:
        s = ctx.acquire()
        ctx.build(s, _images(w, h)[0])
        ctx.profile_enable(True)
        ctx.profile_reset()
        ctx.fast_detect(s, mask_radius=7)
        assert ctx.profile_read(capi.K_GFTT)[1] == 1 and ctx.profile_read(capi.K_DETECT_TAIL)[1] == 1


def test_corners_feed_the_subpixel_and_stereo_lk_chain():
    import torch
    w, h = 752, 480
    left, right, _ = synth.stereo_sequence(17, w, h, 1)
    with capi.Context(width=w, height=h, pool_size=2) as ctx:
        sl, sr = _build_all(ctx, [left[0], right[0]])
        d = Dev(ctx, [sl], ctx.fast_keypoint_bound(), 0, None, [30], 200)
        d.detect(capi.fast_default_params())
        want, _ = R.detect(left[0], [], 30, 10, 200)
        assert 50 < len(want) <= 200

        def chain(xy, n_pts):
            """hv_corner_subpix_batch_dev, then the left -> right LK call (tracker.cpp:249-262), all on device arrays."""
            nxt = xy.clone()
            st = torch.zeros(200, dtype=torch.uint8, device="cuda")
            err = torch.zeros(200, dtype=torch.float32, device="cuda")
            prv, nxt_s = torch.tensor([sl], dtype=torch.int32, device="cuda"), torch.tensor([sr], dtype=torch.int32, device="cuda")
            ctx.corner_subpix_batch_dev(1, prv.data_ptr(), 200, n_pts.data_ptr(), xy.data_ptr())
            ctx.klt_track_batch_dev(1, prv.data_ptr(), nxt_s.data_ptr(), 200, xy.data_ptr(), nxt.data_ptr(), st.data_ptr(),
                                    err.data_ptr(), use_initial_flow=False)        # (rows behind the count hold the sentinel: not compared)
            ctx.synchronize()
            n = int(n_pts.cpu()[0])
            return xy.cpu().numpy()[0, :n], nxt.cpu().numpy()[0, :n], st.cpu().numpy()[:n]

        got = chain(d.corners, d.n_out)                  # the detector's own device outputs, no host step in between
        ref_xy = torch.full((1, 200, 2), SENTINEL, dtype=torch.float32, device="cuda")
        ref_xy[0, :len(want)] = torch.from_numpy(want).cuda()
        ref = chain(ref_xy, torch.tensor([len(want)], dtype=torch.int32, device="cuda"))
        assert len(got[0]) == len(want)
        assert _bits_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]) and got[2].sum() > len(want) // 2
        assert _bits_equal(got[1][got[2] > 0], ref[1][ref[2] > 0])
