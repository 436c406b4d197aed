"""hv_gftt_legacy_keypoints_batch_dev / hv_gftt_legacy_detect_batch_dev / hv_gftt_legacy_detect on the MI355X against the numpy
restatement of the reference's legacy GFTT path (tests/gftt_legacy_restatement.py): full equality of counts, order and float bits of
the corners and their responses, no case excluded, no tolerance. Sizes: the smallest a context holds, an odd one that is no multiple
of the tile, and 752 x 480 (19 575 to 24 201 candidates, more than one sorted group of the select kernel, thousands of equal
responses); the hand-built images of the CPU test across the tile seams; the device-side flags with sentinel rows; the batched form
against the synchronous one, eager and replayed from a captured HIP graph; and the sub-pixel + stereo LK chain the corners feed."""
import functools

import numpy as np
import pytest

import gftt_legacy_cases as K
import gftt_legacy_restatement as R
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
def _eig(w, h, k, block=3):
    e = R.response(_images(w, h)[k], block)
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def _cand(w, h, k, block=3, quality=0.01):
    """The unmasked candidates of a seeded image (computed once, shared, read-only)."""
    c = R.candidates(_images(w, h)[k], (), 1, block, quality, eig=_eig(w, h, k, block))
    c.setflags(write=False)
    return c


def _levels(w, h):
    return 1 if min(w, h) < 64 else 4


class Dev:
    """The device arrays of one batched call, pre-filled with a sentinel."""

    def __init__(self, ctx, slots, max_kp, max_prev=0, prevs=None, radii=None, max_corners=0):
        import torch
        self.torch, self.ctx, self.n, self.max_kp, self.max_prev, self.max_corners = torch, ctx, len(slots), max_kp, max_prev, max_corners
        n = self.n
        self.slots = torch.tensor(list(slots), dtype=torch.int32, device="cuda")
        self.work = torch.empty(max(ctx.gftt_legacy_work_bytes(n, max_kp), 16), dtype=torch.uint8, device="cuda")
        self.n_cand = torch.full((n,), -99, dtype=torch.int32, device="cuda")
        self.corners = torch.full((n, max(max_corners, 1), 2), SENTINEL, dtype=torch.float32, device="cuda")
        self.resp = torch.full((n, max(max_corners, 1)), SENTINEL, dtype=torch.float32, device="cuda")
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
        self.corners.fill_(SENTINEL); self.resp.fill_(SENTINEL); self.n_cand.fill_(-99); self.n_out.fill_(-99)

    def keypoints(self, params):
        self.ctx.gftt_legacy_keypoints_batch_dev(self.n, self.slots.data_ptr(), self.work.data_ptr(), self.max_kp, self.n_cand.data_ptr(),
                                                 self.max_corners, self.corners.data_ptr(), self.resp.data_ptr(), self.n_out.data_ptr(),
                                                 params)

    def detect(self, params, with_resp=True):
        self.ctx.gftt_legacy_detect_batch_dev(self.n, self.slots.data_ptr(), self.work.data_ptr(), self.max_kp, self.n_cand.data_ptr(),
                                              self.max_prev, self.n_prev.data_ptr() if self.max_prev else 0,
                                              self.prev.data_ptr() if self.max_prev else 0, self.radius.data_ptr(), self.max_corners,
                                              self.corners.data_ptr(), self.resp.data_ptr() if with_resp else 0, self.n_out.data_ptr(),
                                              params)

    def read(self):
        self.ctx.synchronize()
        return self.n_cand.cpu().numpy(), self.corners.cpu().numpy(), self.resp.cpu().numpy(), self.n_out.cpu().numpy()


def _build_all(ctx, imgs):
    slots = [ctx.acquire() for _ in imgs]
    for s, im in zip(slots, imgs):
        ctx.build(s, im)
    return slots


def _check(got, want, what):
    """got = Dev.read(); want = a list of R.detect results: set i holds exactly want[i] and sentinels behind it."""
    n_cand, corners, resp, n_out = got
    for i, (c, v, cand) in enumerate(want):
        assert n_cand[i] == len(cand), (what, i, "candidates", n_cand[i], len(cand))
        assert n_out[i] == len(c), (what, i, "corners", n_out[i], len(c))
        if not _bits_equal(corners[i, :len(c)], c):
            bad = np.nonzero((corners[i, :len(c)] != c).any(1))[0]
            raise AssertionError((what, i, bad[:5], corners[i, bad[:5]], c[bad[:5]]))
        assert _bits_equal(resp[i, :len(c)], v), (what, i, "responses")
        assert (corners[i, len(c):] == SENTINEL).all() and (resp[i, len(c):] == SENTINEL).all(), (what, i, "rows behind the count")


def _params(block=3, quality=0.01, md=50.0, mt=200):
    return capi.gftt_legacy_default_params(gfttBlockSize=block, gfttQualityLevel=quality, gfttMinDistance=md, maxTracks=mt)


# (quality, gfttMinDistance, maxTracks): every quality, every distance branch and every cap; 4096 walks every candidate
COMBOS = [(0.01, 50.0, 200), (0.1, 7.3, 4096), (0.9, 0.0, 4096), (0.01, 0.0, 1), (0.01, 7.3, 200), (0.01, 50.0, 4096), (0.01, 0.0, 4096),
          (0.1, 50.0, 1)]


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_keypoints_equal_the_restatement(size):
    w, h = size
    imgs = _images(w, h)
    with capi.Context(width=w, height=h, levels=_levels(w, h), pool_size=3) as ctx:
        slots = _build_all(ctx, imgs)
        bound = ctx.gftt_legacy_keypoint_bound()
        assert bound == (w - 2) * (h - 2)
        assert ctx.gftt_legacy_min_distance(_params(md=7.3)) == 7.3 * (min(w, h) / 720.0)
        for j, (q, md, mt) in enumerate(COMBOS):
            # the default on all three images; at 752 x 480 every other combination on one image, each image in turn
            ks = [0, 1, 2] if (j == 0 or w * h < 100000) else [j % 3]
            cap = min(mt, bound)
            d = Dev(ctx, [slots[k] for k in ks], bound, max_corners=cap)
            d.keypoints(_params(3, q, md, mt))
            want = [R.detect(imgs[k], (), 1, 3, q, md, mt, cand=_cand(w, h, k, 3, q)) for k in ks]
            _check(d.read(), want, (q, md, mt))
            if j == 0 and w == 752:
                assert all(len(c) > capi.DETECT_TAIL_MAX_KEYPOINTS for _, _, c in want)
                assert len(np.unique(want[2][2][:, 2])) < len(want[2][2]) - 1000          # thousands of equal responses
            if mt == 4096 and md == 0.0:
                assert all(len(c) == min(len(cand), 4096) for c, _, cand in want)


def test_block_sizes_5_and_7():
    w, h = 97, 130
    imgs = _images(w, h)
    with capi.Context(width=w, height=h, levels=4, pool_size=3) as ctx:
        slots = _build_all(ctx, imgs)
        bound = ctx.gftt_legacy_keypoint_bound()
        for block in (5, 7):
            for q, md, mt in ((0.01, 50.0, 200), (0.1, 0.0, 4096)):
                d = Dev(ctx, slots, bound, max_corners=min(mt, bound))
                d.keypoints(_params(block, q, md, mt))
                want = [R.detect(imgs[k], (), 1, block, q, md, mt, cand=_cand(w, h, k, block, q)) for k in range(3)]
                assert all(len(c) > 0 for c, _, _ in want)
                _check(d.read(), want, (block, q, md, mt))


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_detect_equals_the_restatement(size):
    w, h = size
    imgs = _images(w, h)
    sets = []                                            # (image, radius, live tracks)
    for k in range(3):
        near = K.live_tracks(_cand(w, h, k), k)
        top = _cand(w, h, k)[0, :2]                      # the global maximum of the unmasked image: a box over it
        for j, (r, pv) in enumerate(((1, near), (30, near[:30]), (119, K.edge_tracks(w, h)), (7, K.OUT_OF_RANGE_PREV(w, h)),
                                     (1, np.array([top + 0.25], np.float32)), (5, np.zeros((0, 2), np.float32)),
                                     (30, K.edge_tracks(w, h)))):
            if w * h < 100000 or (j + k) % 3 == 0 or j == 4:
                sets.append((k, r, pv))
    masks_top = [(k, pv) for k, r, pv in sets if len(pv) == 1]
    assert all(not R.mask(pv, 1, w, h)[int(_cand(w, h, k)[0, 1]), int(_cand(w, h, k)[0, 0])] for k, pv in masks_top)
    cands = [R.candidates(imgs[k], pv, r, eig=_eig(w, h, k)) for k, r, pv in sets]
    with capi.Context(width=w, height=h, levels=_levels(w, h), pool_size=3) as ctx:
        slots = _build_all(ctx, imgs)
        bound = ctx.gftt_legacy_keypoint_bound()
        for md, mt in ((50.0, 200), (7.3, 4096), (0.0, 1)):
            want = [R.detect(imgs[k], pv, r, 3, 0.01, md, mt, cand=c) for (k, r, pv), c in zip(sets, cands)]
            d = Dev(ctx, [slots[k] for k, _, _ in sets], bound, 100, [pv for _, _, pv in sets], [r for _, r, _ in sets], min(mt, bound))
            d.detect(_params(3, 0.01, md, mt))
            _check(d.read(), want, ("detect", md, mt))
            if mt == 200:
                # the synchronous form; and the batched form without the optional responses
                for i in (0, len(sets) // 2, len(sets) - 1):
                    k, r, pv = sets[i]
                    assert _bits_equal(ctx.gftt_legacy_detect(slots[k], pv, r, _params(3, 0.01, md, mt)), want[i][0])
                d.reset()
                d.detect(_params(3, 0.01, md, mt), with_resp=False)
                got = d.read()
                assert (got[2] == SENTINEL).all()
                assert all(got[3][i] == len(c) and _bits_equal(got[1][i, :len(c)], c) for i, (c, _, _) in enumerate(want))


def test_hand_built_images_across_the_tile_seams():
    tw, th = capi.gftt_legacy_tile_size()               # the kernels' own constants: the cases move with them
    w, h = tw + 32, max(64, 2 * th + 32)
    imgs, tags = [], []
    for name, (patch, offs) in K.hand_patches().items():
        for cx in (tw - 1, tw):                          # the pixel under test in the last column of a tile, and the first of the next
            for cy in (th - 1, th, 2 * th - 1, 2 * th):
                imgs.append(K.embed(patch, 0, w, h, cx, cy))
                tags.append((name, [(cx + dx, cy + dy) for dx, dy in offs]))
    for name, (img, pts) in K.border_images(w, h).items():
        imgs.append(img)
        tags.append((name, pts))
    for x0, y0 in ((tw - 2, th - 3), (tw - 22, 2 * th - 4)):                      # a rejected and an accepted pair across the seams
        img, md, pts = K.distance_pairs(w, h, x0, y0)
        imgs.append(img)
        tags.append((("pairs", md), list(pts)))
    with capi.Context(width=w, height=h, levels=1, pool_size=len(imgs) + 1) as ctx:
        slots = _build_all(ctx, imgs)
        bound = ctx.gftt_legacy_keypoint_bound()
        n_plain = len(imgs) - 2
        d = Dev(ctx, slots[:n_plain], bound, max_corners=200)
        d.keypoints(_params(md=0.0))
        want = [R.detect(im, (), 1, 3, 0.01, 0.0, 200) for im in imgs[:n_plain]]
        _check(d.read(), want, "hand-built")
        for (name, pts), (c, _, _) in zip(tags, want):
            assert c.tolist() == [[float(x), float(y)] for x, y in pts], name
        for i in (n_plain, n_plain + 1):
            (_, md), pts = tags[i]
            d = Dev(ctx, [slots[i]], bound, max_corners=200)
            d.keypoints(_params(md=md))
            wnt = R.detect(imgs[i], (), 1, 3, 0.01, md, 200)
            assert abs(ctx.gftt_legacy_min_distance(_params(md=md)) - 6.5) < 1e-9 and len(wnt[2]) == 4
            _check(d.read(), [wnt], "pairs")
            assert wnt[0].tolist() == [[float(x), float(y)] for x, y in pts]
        # the masked maximum, its pixel on either side of a seam
        s = ctx.acquire()
        for ax, ay in ((tw, th), (tw - 1, 2 * th - 1)):
            img, pv, r, q = K.masked_maximum(w, h, ax, ay)
            ctx.build(s, img)
            d = Dev(ctx, [s], bound, 4, [pv], [r], 200)
            d.detect(_params(quality=q, md=0.0))
            wnt = R.detect(img, pv, r, 3, q, 0.0, 200)
            _check(d.read(), [wnt], "masked maximum")
            assert wnt[0].tolist() == [[ax + 15.0, ay + 10.0]]


def test_device_side_flags_leave_their_rows_untouched():
    w, h = 97, 130
    imgs = _images(w, h)
    with capi.Context(width=w, height=h, levels=1, pool_size=4) as ctx:
        slots = _build_all(ctx, imgs)
        empty = ctx.acquire()                            # in use, but no image was ever built in it
        bound = ctx.gftt_legacy_keypoint_bound()
        radii = [30, 0, 7, -1, 2, 5, 5, 5]
        which = [0, 1, 2, 0, 1, 2, 0, 1]
        set_slots = [slots[k] for k in which]
        set_slots[5], set_slots[6], set_slots[7] = 99, -1, empty             # not a slot, not a slot, no image
        near = K.live_tracks(_cand(w, h, 0), 3, 40)
        d = Dev(ctx, set_slots, bound, 40, [near] * 8, radii, 200)
        d.detect(_params())
        n_cand, corners, resp, n_out = got = d.read()
        for i, (k, r) in enumerate(zip(which, radii)):
            if r < 1 or i >= 5:
                assert n_cand[i] == -1 and n_out[i] == -1
                assert (corners[i] == SENTINEL).all() and (resp[i] == SENTINEL).all()
            else:                                        # the healthy neighbours are what they are alone
                wnt = R.detect(imgs[k], near, r, cand=R.candidates(imgs[k], near, r, eig=_eig(w, h, k)))
                _check(tuple(x[i:i + 1] for x in got), [wnt], i)
        # max_keypoints one below the candidate count of the richest image: reported, never truncated, beside two healthy neighbours;
        # exactly enough room is enough
        counts = [len(_cand(w, h, k)) for k in range(3)]
        rich = int(np.argmax(counts))
        assert sorted(counts)[1] < counts[rich]
        for cap_kp in (counts[rich] - 1, counts[rich]):
            d = Dev(ctx, slots, cap_kp, max_corners=200)
            d.keypoints(_params())
            n_cand, corners, resp, n_out = got = d.read()
            for k in range(3):
                if counts[k] <= cap_kp:
                    _check(tuple(x[k:k + 1] for x in got), [R.detect(imgs[k], cand=_cand(w, h, k))], ("capacity", cap_kp, k))
                else:
                    assert k == rich and cap_kp == counts[rich] - 1
                    assert n_cand[k] == -1 and n_out[k] == -1 and (corners[k] == SENTINEL).all() and (resp[k] == SENTINEL).all()
        # counts read from device memory are clamped to their capacity
        d3 = Dev(ctx, [slots[0], slots[0]], bound, 40, [near, near], [7, 7], 200)
        d3.n_prev.copy_(d3.torch.tensor([1000, -5], dtype=d3.torch.int32))
        d3.detect(_params())
        got = d3.read()
        for i, p in enumerate((near, [])):
            _check(tuple(x[i:i + 1] for x in got), [R.detect(imgs[0], p, 7, cand=R.candidates(imgs[0], p, 7, eig=_eig(w, h, 0)))], ("clamped", i))
        with pytest.raises(capi.HvError):
            ctx.gftt_legacy_detect(empty)                # HV_ERR_POOL: the slot holds no image


def test_batch_eager_and_graph_replayed_on_three_radii():
    import torch
    w, h = 752, 480
    imgs = _images(w, h)
    radii = [1, 30, 119]
    prevs = [K.live_tracks(_cand(w, h, 0), 20), K.live_tracks(_cand(w, h, 1), 21, 30), K.edge_tracks(w, h)]
    want = [R.detect(imgs[k], prevs[k], radii[k], cand=R.candidates(imgs[k], prevs[k], radii[k], eig=_eig(w, h, k))) for k in range(3)]
    assert all(len(c) > 0 for c, _, _ in want)
    with capi.Context(width=w, height=h, pool_size=3) as ctx:
        slots = _build_all(ctx, imgs)
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        d = Dev(ctx, slots, 40000, 100, prevs, radii, 200)
        params = _params()
        d.detect(params)
        _check(d.read(), want, "eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            d.detect(params)
        for _ in range(2):
            with torch.cuda.stream(stream):
                d.reset()
                g.replay()
            stream.synchronize()
            _check(d.read(), want, "replayed")
        del g


def test_profile_classes_count_the_launches():
    w, h = 97, 130
    with capi.Context(width=w, height=h, levels=1, pool_size=1) as ctx:
        s = ctx.acquire()
        ctx.build(s, _images(w, h)[0])
        ctx.profile_enable(True)
        ctx.profile_reset()
        ctx.gftt_legacy_detect(s, mask_radius=7)
        assert ctx.profile_read(capi.K_GFTT)[1] == 1 and ctx.profile_read(capi.K_DETECT_TAIL)[1] == 1


def test_corners_feed_the_subpixel_and_stereo_lk_chain():
    import torch
    w, h = 752, 480
    left, right, _ = synth.stereo_sequence(17, w, h, 1)
    with capi.Context(width=w, height=h, pool_size=2) as ctx:
        sl, sr = _build_all(ctx, [left[0], right[0]])
        d = Dev(ctx, [sl], ctx.gftt_legacy_keypoint_bound(), 0, None, [30], 200)
        d.detect(_params())
        want = R.detect(left[0], (), 30)[0]
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
