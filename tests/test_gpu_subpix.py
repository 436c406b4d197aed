"""hv_corner_subpix / hv_corner_subpix_batch_dev on the MI355X: bit-identical to the numpy restatement of cv::cornerSubPix +
SubPixelAdjuster::adjust (tests/subpix_restatement.py), positions and update counts, over image sizes, point lists and
parameters; the batched form against the synchronous one, eager and replayed from a captured HIP graph; and the stereo LK
call that the refined corners feed (tracker.cpp:249-262)."""
import ctypes as C

import numpy as np
import pytest

import subpix_restatement as R
from hybvio_amd import capi, synth

pytestmark = pytest.mark.gpu

# 33 x 33 is 2 * win + 5 for win 14: the smallest image cornerSubPix accepts for that window (a context holds images of more
# than 31 pixels in each dimension, so the window-10 minimum of 25 x 25 cannot be a pyramid slot)
SIZES = [(752, 480), (1280, 720), (97, 130), (33, 33)]


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _images(w, h):
    """A synthetic stereo frame and a noise image with a flat block (the det break)."""
    frame = synth.stereo_sequence(11, w, h, 1)[0][0]
    rng = np.random.default_rng(w * 7 + h)
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    fx0, fy0 = w // 4, h // 4
    noise[fy0:fy0 + h // 2, fx0:fx0 + w // 2] = 128
    return [frame, noise], (fx0, fy0, w // 2, h // 2)


def _point_lists(ctx, slot, img, flat, seed):
    w, h = img.shape[1], img.shape[0]
    rng = np.random.default_rng(seed)
    lists = []
    md = 50.0 if min(w, h) >= 64 else 8.0
    for r in (20, 50):
        lists.append(ctx.gftt_detect(slot, mask_radius=r, params=capi.gftt_default_params(gfttMinDistance=md)))
    m = 12
    edge = np.concatenate([
        np.stack([rng.uniform(0, m, 40), rng.uniform(0, h, 40)], 1), np.stack([rng.uniform(w - m, w, 40), rng.uniform(0, h, 40)], 1),
        np.stack([rng.uniform(0, w, 40), rng.uniform(0, m, 40)], 1), np.stack([rng.uniform(0, w, 40), rng.uniform(h - m, h, 40)], 1),
        [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]]]).astype(np.float32)
    edge = np.minimum(edge, np.nextafter(np.array([w, h], np.float32), 0))
    lists.append(edge)
    lists.append(np.array([[-1, 5], [w, 3], [4, h + 0.5], [-0.25, -0.25], [np.nan, 3], [1e9, 2]], np.float32))
    fx0, fy0, fw, fh = flat
    lists.append(np.stack([rng.uniform(fx0 + 12, fx0 + fw - 12, 10), rng.uniform(fy0 + 12, fy0 + fh - 12, 10)], 1).astype(np.float32)
                 if fw > 30 and fh > 30 else np.zeros((0, 2), np.float32))
    lists.append(np.stack([rng.uniform(0, w, 60), rng.uniform(0, h, 60)], 1).astype(np.float32))
    return [p for p in lists if len(p)]


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_bit_identical_to_the_restatement(size):
    w, h = size
    imgs, flat = _images(w, h)
    big = min(capi.SUBPIX_MAX_WIN, (min(w, h) - 5) // 2)                    # the largest window the image allows
    # (window, subPixMaxIter, subPixEpsilon): every setting at the default window, the defaults at every window, and the
    # clamped / exhausting iteration counts at the smallest and the largest window
    runs = [(10, it, eps) for it, eps in ((20, 0.03), (0, 0.03), (1, 0.03), (150, 0.0), (20, 0.0))]
    runs += [(win, 20, 0.03) for win in (3, 5, big)] + [(3, 150, 0.0), (big, 150, 0.0), (big, 1, 0.0), (5, 0, 0.0)]
    with capi.Context(width=w, height=h, levels=1 if min(w, h) < 64 else 4, pool_size=2) as ctx:
        for k, img in enumerate(imgs):
            s = ctx.acquire()
            ctx.build(s, img)
            lists = _point_lists(ctx, s, img, flat if k == 1 else (0, 0, 0, 0), seed=k)
            pts = np.concatenate(lists)
            for win, it, eps in runs:
                p = capi.subpix_default_params(subPixWindowSize=win, subPixMaxIter=it, subPixEpsilon=eps)
                got, gi = ctx.corner_subpix(s, pts, p)
                want, wi = R.corner_subpix(img, pts, win, it, eps)
                bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)).all(1)) | (gi != wi))[0]
                assert len(bad) == 0, (win, it, eps, bad[:5], got[bad[:5]], want[bad[:5]], gi[bad[:5]], wi[bad[:5]])
                assert wi.max() <= max(min(it, 100), 1)
            ctx.release(s)


def test_argument_errors():
    L = capi.lib()
    with capi.Context(width=32, height=60, levels=1, pool_size=1) as ctx:
        s = ctx.acquire()
        ctx.build(s, np.zeros((60, 32), np.uint8))
        xy = np.array([[10, 10]], np.float32)
        call = lambda p: L.hv_corner_subpix(ctx._h, C.byref(p), s, 1, xy.ctypes.data_as(capi.f32p), None)
        assert call(capi.subpix_default_params(subPixWindowSize=14)) == -1         # 32 < 2 * 14 + 5
        assert call(capi.subpix_default_params(subPixWindowSize=0)) == -1
        assert call(capi.subpix_default_params(subPixWindowSize=17)) == -2         # beyond HV_SUBPIX_MAX_WIN
        assert call(capi.subpix_default_params(subPixWindowSize=13)) == 0          # 32 >= 2 * 13 + 5 = 31
        assert L.hv_corner_subpix(ctx._h, C.byref(capi.subpix_default_params()), s + 5, 1,
                                  xy.ctypes.data_as(capi.f32p), None) == -5        # HV_ERR_POOL
        assert L.hv_corner_subpix_batch_dev(ctx._h, C.byref(capi.subpix_default_params()), 1, None, 4, None, None, None) == -1
        assert L.hv_corner_subpix_batch_dev(ctx._h, C.byref(capi.subpix_default_params(subPixWindowSize=14)), 0, None, 0, None,
                                            None, None) == -1
        assert L.hv_corner_subpix_batch_dev(ctx._h, C.byref(capi.subpix_default_params()), 0, None, 0, None, None, None) == 0


def _batch_inputs(ctx, frames, n_sets, max_points, seed):
    rng = np.random.default_rng(seed)
    slots = [ctx.acquire() for _ in frames]
    for s, f in zip(slots, frames):
        ctx.build(s, f)
    corners = [ctx.gftt_detect(s, mask_radius=20) for s in slots]
    set_slot = rng.integers(0, len(slots), n_sets)
    counts = rng.integers(0, max_points + 1, n_sets)
    counts[::97] = 0                                                       # empty sets
    xy = np.zeros((n_sets, max_points, 2), np.float32)
    for i in range(n_sets):
        c = corners[set_slot[i]]
        pick = c[rng.integers(0, len(c), counts[i])] + rng.integers(-2, 3, (counts[i], 2)).astype(np.float32)
        xy[i, :counts[i]] = np.clip(pick, 0, [frames[0].shape[1] - 1, frames[0].shape[0] - 1])
    return slots, np.array([slots[k] for k in set_slot], np.int32), counts.astype(np.int32), xy


def test_batch_matches_the_synchronous_form_eager_and_graph_replayed():
    import torch
    w, h = 752, 480
    left, right, _ = synth.stereo_sequence(5, w, h, 3)
    frames = [left[0], left[1], left[2], right[0]]
    n_sets, max_points = 1024, 200
    with capi.Context(width=w, height=h, pool_size=len(frames)) as ctx:
        slots, set_slots, counts, xy = _batch_inputs(ctx, frames, n_sets, max_points, 3)
        want = xy.copy()
        want_it = np.zeros((n_sets, max_points), np.int32)
        for i in range(n_sets):
            if counts[i]:
                want[i, :counts[i]], want_it[i, :counts[i]] = ctx.corner_subpix(int(set_slots[i]), xy[i, :counts[i]])
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        d_slots = torch.from_numpy(set_slots).cuda()
        d_n = torch.from_numpy(counts).cuda()
        d_in = torch.from_numpy(xy).cuda()
        d_xy = d_in.clone()
        d_it = torch.full((n_sets, max_points), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.corner_subpix_batch_dev(n_sets, d_slots.data_ptr(), max_points, d_n.data_ptr(), d_xy.data_ptr(), d_it.data_ptr())
        ctx.synchronize()
        got, got_it = d_xy.cpu().numpy(), d_it.cpu().numpy()
        live = np.arange(max_points)[None, :] < counts[:, None]
        assert _bits_equal(got[live], want[live]) and np.array_equal(got_it[live], want_it[live])
        assert _bits_equal(got[~live], xy[~live]) and (got_it[~live] == -1).all()        # padding is never touched
        # the same launch captured once on one stream and replayed
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            ctx.corner_subpix_batch_dev(n_sets, d_slots.data_ptr(), max_points, d_n.data_ptr(), d_xy.data_ptr(), d_it.data_ptr())
        for _ in range(2):
            with torch.cuda.stream(stream):
                d_xy.copy_(d_in)
                d_it.fill_(-1)
                g.replay()
            stream.synchronize()
            assert _bits_equal(d_xy.cpu().numpy(), got) and np.array_equal(d_it.cpu().numpy(), got_it)
        del g


def test_profile_class_counts_the_launches():
    w, h = 320, 240
    img = synth.stereo_sequence(2, w, h, 1)[0][0]
    with capi.Context(width=w, height=h) as ctx:
        s = ctx.acquire()
        ctx.build(s, img)
        c = ctx.gftt_detect(s, mask_radius=20)
        ctx.profile_enable(True)
        ctx.profile_reset()
        ctx.corner_subpix(s, c)
        ctx.corner_subpix(s, c)
        ms, n = ctx.profile_read(capi.K_SUBPIX)
        assert n == 2 and ms > 0
        assert ctx.profile_read(capi.K_GFTT)[1] == 0


def test_refined_corners_feed_the_stereo_lk_call(oracle):
    w, h = 752, 480
    left, right, _ = synth.stereo_sequence(17, w, h, 1)
    with capi.Context(width=w, height=h, pool_size=2) as ctx:
        sl, sr = ctx.acquire(), ctx.acquire()
        ctx.build(sl, left[0])
        ctx.build(sr, right[0])
        det = ctx.gftt_detect(sl, mask_radius=20)
        ref, _ = ctx.corner_subpix(sl, det)
        want, _ = R.corner_subpix(left[0], det)
        assert _bits_equal(ref, want)
        # tracker.cpp:249-262: left -> right LK from the refined left corners
        xy, st, _ = ctx.klt_track(sl, sr, ref)
        oxy, ost, _ = oracle.klt_track(oracle.Pyramid(left[0]), oracle.Pyramid(right[0]), want)
        assert np.array_equal(st, ost) and st.sum() > len(st) // 2
        assert np.array_equal(xy[st > 0], oxy[ost > 0])
