"""The dense stereo entries on the MI355X against the numpy restatement (tests/stereo_bm_restatement.py): hv_stereo_disparity_batch_dev
with and without the speckle filter, hv_filter_speckles_batch_dev on crafted maps, hv_stereo_track_depth_batch_dev and
hv_stereo_point_cloud_batch_dev, the chain behind the rectifying ingest, and one captured graph. Every result must be EQUAL to the
restatement (int16 values, counts, float bits): there is no tolerance anywhere. The restatement is not pinned against an OpenCV
build (its docstring lists the doubts); the kernels follow it either way."""
import numpy as np
import pytest

import stereo_bm_cases as K
import stereo_bm_restatement as R
from hybvio_amd import capi

pytestmark = pytest.mark.gpu

SENTINEL = 12345                                       # an int16 no result can be (nd <= 64 here: values < 1024)
FSENT = -77.0


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _build_all(ctx, imgs):
    slots = [ctx.acquire() for _ in imgs]
    for s, im in zip(slots, imgs):
        ctx.build(s, im)
    return slots


class Pairs:
    """A context with the three scenes of a shape built into six slots, and the device arrays of one batched call."""

    def __init__(self, ctx, w, h, nd, left_slots, right_slots):
        import torch
        self.torch, self.ctx, self.w, self.h, self.n = torch, ctx, w, h, len(left_slots)
        self.left = torch.tensor(list(left_slots), dtype=torch.int32, device="cuda")
        self.right = torch.tensor(list(right_slots), dtype=torch.int32, device="cuda")
        self.work = torch.empty(max(ctx.stereo_work_bytes(self.n, capi.stereo_bm_default_params(w, numDisparities=nd)), 16),
                                dtype=torch.uint8, device="cuda")
        self.disp = torch.full((self.n, h, w), SENTINEL, dtype=torch.int16, device="cuda")
        self.n_valid = torch.full((self.n,), -99, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def run(self, params):
        self.ctx.stereo_disparity_batch_dev(self.n, self.left.data_ptr(), self.right.data_ptr(), self.work.data_ptr(),
                                            self.disp.data_ptr(), self.w * self.h, self.n_valid.data_ptr(), params)

    def read(self):
        self.ctx.synchronize()
        return self.disp.cpu().numpy(), self.n_valid.cpu().numpy()


def _differences(got, want):
    bad = np.argwhere(got != want)
    return [(int(y), int(x), int(got[y, x]), int(want[y, x])) for y, x in bad[:6]], len(bad)


@pytest.mark.parametrize("speckles", [False, True], ids=["no_speckles", "speckles"])
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.IDS)
def test_disparity_equals_the_restatement(shape, speckles):
    """(a) and (b): three distinct scenes per batch, slots in shuffled order, one set with an invalid slot."""
    w, h, nd = shape
    scenes = K.scenes(w, h, nd)
    with capi.Context(width=w, height=h, levels=1, pool_size=8) as ctx:
        slots = _build_all(ctx, [im for pair in scenes for im in pair])          # left k in slots[2k], right k in slots[2k + 1]
        empty = ctx.acquire()                                                    # in use, but no image was ever built in it
        order = [2, 0, 1, 0, 2]
        left = [slots[2 * k] for k in order] + [slots[0], 99]
        right = [slots[2 * k + 1] for k in order] + [empty, slots[1]]
        d = Pairs(ctx, w, h, nd, left, right)
        params = capi.stereo_bm_default_params(w, numDisparities=nd, speckleWindowSize=500 if speckles else 0)
        d.run(params)
        disp, n_valid = d.read()
        for i, k in enumerate(order):
            want, _ = K.expected(w, h, nd, k, speckles)
            first, n_bad = _differences(disp[i], want)
            assert n_bad == 0, (i, k, n_bad, first)
            assert n_valid[i] == int((want != R.FILTERED).sum()), (i, k)
        for i in (5, 6):                                                          # no image / not a slot: -1 and an untouched row
            assert n_valid[i] == -1 and (disp[i] == SENTINEL).all(), i
        # the synchronous form, and a NULL n_valid_dev
        want, _ = K.expected(w, h, nd, 1, speckles)
        assert np.array_equal(ctx.stereo_disparity(slots[2], slots[3], params), want)
        with pytest.raises(capi.HvError):
            ctx.stereo_disparity(slots[0], empty, params)                        # HV_ERR_POOL: the slot holds no image
        d.disp.fill_(SENTINEL)
        ctx.stereo_disparity_batch_dev(2, d.left.data_ptr(), d.right.data_ptr(), d.work.data_ptr(), d.disp.data_ptr(), w * h, 0, params)
        ctx.synchronize()
        assert np.array_equal(d.disp.cpu().numpy()[1], K.expected(w, h, nd, order[1], speckles)[0])


def test_an_empty_valid_rectangle_gives_filtered_everywhere():
    w, h = 64, 64                                                                 # nd 64: 63 + 10 >= 64 - 10
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (h, w)).astype(np.uint8) for _ in range(2)]
    with capi.Context(width=w, height=h, levels=1, pool_size=2) as ctx:
        sl, sr = _build_all(ctx, imgs)
        d = Pairs(ctx, w, h, 64, [sl], [sr])
        d.run(capi.stereo_bm_default_params(w, numDisparities=64))
        disp, n_valid = d.read()
        assert (disp == R.FILTERED).all() and n_valid[0] == 0


def _serpentine(w, h, gap):
    """One path of value 100 that runs along every other row and turns at alternating ends: a single long component."""
    m = np.full((h, w), R.FILTERED, np.int16)
    for i, y in enumerate(range(0, h, gap)):
        m[y, :] = 100
        if y + gap < h:
            m[y:y + gap, w - 1 if i % 2 == 0 else 0] = 100
    return m


def _crafted_maps(w, h):
    F = R.FILTERED
    maps = []
    a = np.full((h, w), F, np.int16)                       # a component of exactly 500 and one of 501, apart
    a[1:11, 2:52] = 200
    a[20:30, 2:52] = 300; a[30, 2] = 300
    maps.append(a)
    b = np.full((h, w), F, np.int16)                       # 10 joins, 11 does not: two blocks of 300 pixels each
    b[0:10, 0:30] = 50; b[0:10, 30:60] = 60                # joined: 600 pixels, kept
    b[20:30, 0:30] = 50; b[20:30, 30:60] = 61              # not joined: 300 + 300, removed
    maps.append(b)
    c = np.full((h, w), F, np.int16)                       # a non-transitive chain: 0 - 10 - 20, each 200 pixels; 0 and 20 alone would not join
    c[5:15, 0:20] = 0; c[5:15, 20:40] = 10; c[5:15, 40:60] = 20
    c[30:40, 0:20] = 0; c[30:40, 20:21] = F; c[30:40, 21:40] = 20      # the same without the link: 200 and 190, removed
    maps.append(c)
    maps.append(_serpentine(w, h, 3))                      # crosses every tile seam, far more than 500 pixels
    maps.append(np.full((h, w), F, np.int16))
    maps.append(np.full((h, w), 7, np.int16))
    return maps


@pytest.mark.parametrize("size", [(64, 48), (300, 200)], ids=["64x48", "300x200"])
def test_speckle_filter_alone_on_crafted_maps(size):
    """(c)"""
    import torch
    w, h = size
    maps = _crafted_maps(w, h)
    want = [R.filter_speckles(m, R.FILTERED, 500, 10) for m in maps]
    assert (want[0] == 200).sum() == 0 and (want[0] == 300).sum() == 501
    assert (want[1][0:10] != R.FILTERED).sum() == 600 and (want[1][20:30] != R.FILTERED).sum() == 0
    assert (want[2][5:15] != R.FILTERED).sum() == 600 and (want[2][30:40] != R.FILTERED).sum() == 0
    assert np.array_equal(want[3], maps[3]) and (maps[3] != R.FILTERED).sum() > 500
    assert np.array_equal(want[5], maps[5]) == (w * h > 500)
    with capi.Context(width=64, height=64, levels=1, pool_size=1) as ctx:           # the maps need not have the context's size
        stride = w * h + 24
        dev = torch.full((len(maps), stride), SENTINEL, dtype=torch.int16, device="cuda")
        for i, m in enumerate(maps):
            dev[i, :w * h] = torch.from_numpy(m.reshape(-1)).cuda()
        work = torch.empty(capi.filter_speckles_work_bytes(w, h, len(maps)), dtype=torch.uint8, device="cuda")
        ctx.filter_speckles_batch_dev(len(maps), w, h, dev.data_ptr(), stride, R.FILTERED, 500, 10, work.data_ptr())
        ctx.synchronize()
        got = dev.cpu().numpy()
        for i, wnt in enumerate(want):
            first, n_bad = _differences(got[i, :w * h].reshape(h, w), wnt)
            assert n_bad == 0, (i, n_bad, first)
            assert (got[i, w * h:] == SENTINEL).all()
        # other arguments: a positive new_val, a size of 0 and a difference of 0
        m2 = np.array(maps[1]); m2[m2 == R.FILTERED] = 0
        dev2 = torch.from_numpy(np.stack([m2, m2])).cuda()
        ctx.filter_speckles_batch_dev(2, w, h, dev2.data_ptr(), w * h, 0, 300, 0, work.data_ptr())
        ctx.synchronize()
        assert np.array_equal(dev2.cpu().numpy()[1], R.filter_speckles(m2, 0, 300, 0))


def _track_points(w, h, disp, rng):
    ys, xs = np.nonzero(disp >= 16)
    pick = rng.choice(len(xs), 60, replace=False)
    pts = np.stack([xs[pick] + rng.uniform(0, 0.99, 60), ys[pick] + rng.uniform(0, 0.99, 60)], 1)
    edge = [[0, 0], [-0.5, 10.5], [10.5, -0.5], [-1.0, 5], [5, -1.0], [w - 0.5, h - 0.5], [w, 5], [5, h], [w - 1, h - 1],
            [np.nan, 5], [5, np.nan], [np.inf, 5], [5, -np.inf], [3e9, 5], [-3e9, 5], [w + 0.25, h + 0.25]]
    return np.concatenate([pts, np.array(edge)]).astype(np.float32)


def test_track_depth_and_point_cloud_equal_the_restatement():
    """(d)"""
    import torch
    w, h, nd = K.SHAPES[1]
    disps = [np.array(K.expected(w, h, nd, k, True)[0]) for k in range(3)]
    disps[2][0:3, :] = 16                                  # val = 1 on the border rows, 15 / 16 beside it
    disps[2][3, :] = 15
    disps[2][h - 1, w - 1] = 40; disps[2][0, 0] = 40; disps[2][10, 0] = 48; disps[2][0, 10] = 48
    q = K.q_matrix(w, h)
    rng = np.random.default_rng(21)
    pts = [_track_points(w, h, d, rng) for d in disps]
    max_points = max(len(p) for p in pts) + 3
    want_depth = [R.track_depths(q, d, p) for d, p in zip(disps, pts)]
    assert all((x > 0).sum() >= 60 and (x == -1).sum() >= 10 for x in want_depth) and all(np.isfinite(x).all() for x in want_depth)
    assert want_depth[2][60] > 0 and want_depth[2][61] > 0 and want_depth[2][63] == -1          # (int)(-0.5) is 0; -1.0 is outside
    clouds = [R.point_cloud(q, d, 5) for d in disps] + [R.point_cloud(q, disps[0], 3)]
    assert all(len(c) > 50 for c in clouds)
    with capi.Context(width=w, height=h, levels=1, pool_size=1) as ctx:
        stride = w * h + 7
        dd = torch.zeros((3, stride), dtype=torch.int16, device="cuda")
        for i, d in enumerate(disps):
            dd[i, :w * h] = torch.from_numpy(d.reshape(-1)).cuda()
        xy = torch.full((3, max_points, 2), FSENT, dtype=torch.float32, device="cuda")
        for i, p in enumerate(pts):
            xy[i, :len(p)] = torch.from_numpy(p).cuda()
        n_pts = torch.tensor([len(p) for p in pts], dtype=torch.int32, device="cuda")
        depth = torch.full((3, max_points), FSENT, dtype=torch.float32, device="cuda")
        ctx.stereo_track_depth_batch_dev(3, max_points, n_pts.data_ptr(), xy.data_ptr(), dd.data_ptr(), stride, q, depth.data_ptr())
        ctx.synchronize()
        got = depth.cpu().numpy()
        for i, wnt in enumerate(want_depth):
            assert _bits_equal(got[i, :len(wnt)], wnt), (i, np.nonzero(got[i, :len(wnt)] != wnt)[0][:5])
            assert (got[i, len(wnt):] == FSENT).all()
        # the cloud: stride 5 with room to spare, with exactly enough room, and one below a set's count
        bound = ctx.stereo_cloud_bound(5)
        assert bound == R.cloud_bound(w, h, 5)
        for cap in (bound, max(len(c) for c in clouds[:3]), len(clouds[1]) - 1):
            xyz = torch.full((3, max(cap, 1), 3), FSENT, dtype=torch.float32, device="cuda")
            n_out = torch.full((3,), -99, dtype=torch.int32, device="cuda")
            ctx.stereo_point_cloud_batch_dev(3, dd.data_ptr(), stride, q, 5, cap, xyz.data_ptr(), n_out.data_ptr())
            ctx.synchronize()
            g, n = xyz.cpu().numpy(), n_out.cpu().numpy()
            for i, c in enumerate(clouds[:3]):
                if len(c) > cap:
                    assert n[i] == -1 and (g[i] == FSENT).all(), (cap, i)         # never truncated
                else:
                    assert n[i] == len(c) and _bits_equal(g[i, :len(c)], c) and (g[i, len(c):] == FSENT).all(), (cap, i)
            assert cap != len(clouds[1]) - 1 or n[1] == -1
        xyz = torch.full((1, ctx.stereo_cloud_bound(3), 3), FSENT, dtype=torch.float32, device="cuda")
        n_out = torch.full((1,), -99, dtype=torch.int32, device="cuda")
        ctx.stereo_point_cloud_batch_dev(1, dd.data_ptr(), stride, q, 3, xyz.shape[1], xyz.data_ptr(), n_out.data_ptr())
        ctx.synchronize()
        assert int(n_out.cpu()[0]) == len(clouds[3]) and _bits_equal(xyz.cpu().numpy()[0, :len(clouds[3])], clouds[3])


def test_disparity_behind_the_rectifying_ingest():
    """(e): the pair goes through hv_ingest_build_batch_dev with a remap; the slot's level-0 images, downloaded, feed the restatement."""
    import torch
    w, h, nd = K.SHAPES[0]
    left, right = K.scenes(w, h, nd)[0]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    pix = np.stack([xx + 0.8 * np.sin(yy / 17.0) + 0.3, yy + 0.6 * np.cos(xx / 23.0) - 0.2], 2)      # a mild, smooth remap
    with capi.Context(width=w, height=h, levels=1, pool_size=2) as ctx:
        ctx.ingest_set_undistort_map(0, pix)
        ctx.ingest_set_undistort_map(1, pix)
        sl, sr = ctx.acquire(), ctx.acquire()
        src = torch.from_numpy(np.stack([left, right])).cuda()
        slots = torch.tensor([sl, sr], dtype=torch.int32, device="cuda")
        ctx.ingest_build_batch_dev(1, slots.data_ptr(), src.data_ptr(), w * h, w, 1, 0)
        ctx.ingest_build_batch_dev(1, slots.data_ptr() + 4, src.data_ptr() + w * h, w * h, w, 1, 1)
        d = Pairs(ctx, w, h, nd, [sl], [sr])
        params = capi.stereo_bm_default_params(w, numDisparities=nd)
        d.run(params)
        disp, n_valid = d.read()
        rl, rr = ctx.download(sl, 0)[0], ctx.download(sr, 0)[0]
        assert not np.array_equal(rl, left)                                       # the remap did something
        want = R.compute_disparity(rl, rr, K.params_for(w, nd))
        first, n_bad = _differences(disp[0], want)
        assert n_bad == 0, (n_bad, first)
        x0, x1, y0, y1 = R.valid_rect(w, h, nd)
        assert n_valid[0] == (want != R.FILTERED).sum() > 0.25 * (x1 - x0) * (y1 - y0)


def test_disparity_depth_and_cloud_replayed_from_one_graph():
    """(f): one captured graph, replayed on two different inputs, equal to the eager run."""
    import torch
    w, h, nd = K.SHAPES[0]
    scenes = K.scenes(w, h, nd)
    q = K.q_matrix(w, h)
    rng = np.random.default_rng(5)
    max_points = 80
    with capi.Context(width=w, height=h, levels=1, pool_size=2) as ctx:
        sl, sr = ctx.acquire(), ctx.acquire()
        d = Pairs(ctx, w, h, nd, [sl], [sr])
        params = capi.stereo_bm_default_params(w, numDisparities=nd)
        bound = ctx.stereo_cloud_bound(5)
        xy = torch.zeros((1, max_points, 2), dtype=torch.float32, device="cuda")
        n_pts = torch.tensor([max_points], dtype=torch.int32, device="cuda")
        depth = torch.full((1, max_points), FSENT, dtype=torch.float32, device="cuda")
        xyz = torch.full((1, bound, 3), FSENT, dtype=torch.float32, device="cuda")
        n_out = torch.full((1,), -99, dtype=torch.int32, device="cuda")

        def chain():
            d.run(params)
            ctx.stereo_track_depth_batch_dev(1, max_points, n_pts.data_ptr(), xy.data_ptr(), d.disp.data_ptr(), w * h, q, depth.data_ptr())
            ctx.stereo_point_cloud_batch_dev(1, d.disp.data_ptr(), w * h, q, 5, bound, xyz.data_ptr(), n_out.data_ptr())

        def results():
            ctx.synchronize()
            return d.disp.cpu().numpy()[0], int(d.n_valid.cpu()[0]), depth.cpu().numpy()[0], xyz.cpu().numpy()[0], int(n_out.cpu()[0])

        def load(k):
            ctx.build(sl, scenes[k][0]); ctx.build(sr, scenes[k][1])
            want = K.expected(w, h, nd, k, True)[0]
            pts = _track_points(w, h, want, rng)[:max_points]
            xy[0, :len(pts)] = torch.from_numpy(pts).cuda()
            torch.cuda.synchronize()
            return want, R.track_depths(q, want, xy.cpu().numpy()[0]), R.point_cloud(q, want, 5)

        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)
        load(0)
        chain()                                                                   # eager once (nothing lazy is left for the capture)
        ctx.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            chain()
        for k in (1, 2):
            want, want_depth, want_cloud = load(k)
            chain()
            eager = results()
            assert np.array_equal(eager[0], want) and _bits_equal(eager[2], want_depth)
            assert eager[4] == len(want_cloud) and _bits_equal(eager[3][:eager[4]], want_cloud)
            with torch.cuda.stream(stream):
                d.disp.fill_(SENTINEL); depth.fill_(FSENT); xyz.fill_(FSENT); n_out.fill_(-99); d.n_valid.fill_(-99)
                g.replay()
            stream.synchronize()
            replayed = results()
            assert np.array_equal(replayed[0], eager[0]) and replayed[1] == eager[1] == (want != R.FILTERED).sum()
            assert _bits_equal(replayed[2], eager[2]) and _bits_equal(replayed[3], eager[3]) and replayed[4] == eager[4]
        del g


def test_profile_classes_count_the_calls():
    w, h, nd = K.SHAPES[0]
    scenes = K.scenes(w, h, nd)
    with capi.Context(width=w, height=h, levels=1, pool_size=2) as ctx:
        sl, sr = _build_all(ctx, scenes[0])
        ctx.profile_enable(True)
        ctx.profile_reset()
        ctx.stereo_disparity(sl, sr, capi.stereo_bm_default_params(w, numDisparities=nd))
        assert ctx.profile_read(capi.K_INGEST)[1] == 1 and ctx.profile_read(capi.K_STEREO_GATE)[1] == 0
