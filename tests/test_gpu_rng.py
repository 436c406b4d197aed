"""GPU tests of the device std::mt19937 streams (hv_rng_seed / draw / advance_batch_dev). Everything is an integer, so every
comparison is np.array_equal: the state against tests/rng_restatement.py (itself pinned to the oracle's std::mt19937, to numpy's
MT19937 and to the standard's known answer by tests/test_rng_restatement.py), the outputs against oracle.mt19937_draws at the right
skip. The positions and counts are the ones at which the three-phase twist of rng.hip can go wrong (226|227, 453|454, 622|623,
623 -> 0, the lazy twist at 624); the chains run the entries the way a frame does -- draw, consumer, advance by the count the
consumer left on the device -- against one continuous host stream per set, eagerly and replayed from one captured graph."""
import functools

import numpy as np
import pytest

import rng_restatement as R
import trail_index_restatement as T
import ransac3_restatement as R3
from hybvio_amd import capi

pytestmark = pytest.mark.gpu
NONE, FRESH, KEEP_POSE = 0, 1, 2                                            # HV_RESET_*
SENTINEL = np.uint32(0xa5a5a5a5)


def _dev(x):
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _upload(st, gens):
    """The device state := the restatement generators' (mt, pos)."""
    st.mt.copy_(_dev(np.stack([g.state()[0] for g in gens])))
    st.pos.copy_(_dev(np.array([g.pos for g in gens], np.int32)))


def _assert_state(st, gens, what=""):
    mt, pos = _u32(st.mt), st.pos.cpu().numpy()
    for s, g in enumerate(gens):
        assert pos[s] == g.pos, (what, s, pos[s], g.pos)
        assert np.array_equal(mt[s], g.state()[0]), (what, s, np.nonzero(mt[s] != g.state()[0])[0][:8])


def _seeds(n):
    return [(0, 1, 4649, 5489, 0xffffffff)[s] if s < 5 else (2654435761 * s + 12345) & 0xffffffff for s in range(n)]


@pytest.fixture(scope="module")
def ctx():
    import torch
    with capi.Context(width=64, height=64) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        yield c
        torch.cuda.synchronize()


# ---- 1. seed -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 5, 67])                                   # 67: no multiple of a workgroup's four sets
def test_seed_per_set_scalar_and_masked(ctx, S):
    import torch
    seeds = _seeds(S)
    st = capi.rng_state(S)
    st.mt.fill_(-1); st.pos.fill_(-1)
    d_seeds = _dev(np.array(seeds, np.uint32))
    ctx.rng_seed_batch_dev(S, st.table, seed=99, seed_dev=d_seeds.data_ptr())
    torch.cuda.synchronize()
    _assert_state(st, [R.Mt19937(x) for x in seeds], "per-set seeds")
    # the scalar form
    st.mt.fill_(-1); st.pos.fill_(-1)
    ctx.rng_seed_batch_dev(S, st.table, seed=4649)
    torch.cuda.synchronize()
    _assert_state(st, [R.Mt19937(4649)] * S, "scalar seed")
    # a masked re-seed of advanced states: kinds NONE, FRESH, NONE, KEEP_POSE, NONE (repeated over the sets)
    gens = [R.Mt19937(x).advance(100 + 211 * (s % 7)) for s, x in enumerate(seeds)]
    _upload(st, gens)
    kinds = np.array([(NONE, FRESH, NONE, KEEP_POSE, NONE)[s % 5] for s in range(S)], np.int32)
    d_kinds = _dev(kinds)
    ctx.rng_seed_batch_dev(S, st.table, seed=7, reset_kind_dev=d_kinds.data_ptr())
    torch.cuda.synchronize()
    _assert_state(st, [R.Mt19937(7) if kinds[s] else gens[s] for s in range(S)], "masked re-seed")
    # ... with per-set seeds
    ctx.rng_seed_batch_dev(S, st.table, seed=7, seed_dev=d_seeds.data_ptr(), reset_kind_dev=d_kinds.data_ptr())
    torch.cuda.synchronize()
    _assert_state(st, [R.Mt19937(seeds[s]) if kinds[s] else gens[s] for s in range(S)], "masked re-seed, per-set seeds")
    # n_sets = 0: no launch, nothing written
    ctx.rng_seed_batch_dev(0, st.table, seed=1)


# ---- 2. draw -----------------------------------------------------------------------------------------------------------------

DRAW_POS = (624, 1, 226, 227, 396, 397, 453, 454, 622, 623)                 # one per set; 10 sets = three workgroups (4 + 4 + 2)


@functools.lru_cache(maxsize=None)
def _draw_gens():
    """Set s: seed s's generator with pos = DRAW_POS[s] (set 0 freshly seeded, the others inside the array of the first twist)
    and its skip."""
    seeds = _seeds(len(DRAW_POS))
    skips = [0 if p == 624 else p for p in DRAW_POS]
    gens = [R.Mt19937(x).advance(k) for x, k in zip(seeds, skips)]
    assert [g.pos for g in gens] == list(DRAW_POS)
    return seeds, skips, gens


@pytest.mark.parametrize("n", [1, 2, 200, 624, 625, 1500, 2048])
def test_draw_from_every_phase_boundary(ctx, oracle, n):
    import torch
    seeds, skips, gens = _draw_gens()
    S = len(gens)
    st = capi.rng_state(S)
    _upload(st, gens)
    out = torch.full((S + 1, n), int(SENTINEL.view(np.int32)), dtype=torch.int32, device="cuda")     # one row longer than needed
    ctx.rng_draw_batch_dev(S, st.table, n, out.data_ptr())
    torch.cuda.synchronize()
    got = _u32(out)
    for s in range(S):
        want = oracle.mt19937_draws(seeds[s], n, skip=skips[s])
        assert np.array_equal(got[s], want), (s, DRAW_POS[s], n, np.nonzero(got[s] != want)[0][:8])
    assert (got[S] == SENTINEL).all()
    _assert_state(st, gens, "draw leaves the state alone")


def test_draw_after_a_full_array_was_handed_out(ctx, oracle):
    """pos = 624 behind a twist (not the seeded array): the next output needs the second twist."""
    import torch
    g = R.Mt19937(4649).advance(624)
    assert g.pos == 624
    st = capi.rng_state(1)
    _upload(st, [g])
    out = torch.zeros((1, 700), dtype=torch.int32, device="cuda")
    ctx.rng_draw_batch_dev(1, st.table, 700, out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_u32(out)[0], oracle.mt19937_draws(4649, 700, skip=624))


# ---- 3. advance --------------------------------------------------------------------------------------------------------------

COUNTS = (0, 1, 623, 624, 625, 1248, 2048, -5, 3000)                        # a negative one (-> 0), one above every max_draws
START = (0, 5, 1, 624, 300, 623, 100, 226, 454)                             # outputs each set's generator has already produced


@pytest.mark.parametrize("stride,offset,mult,max_draws", [(1, 0, 1, 2048), (2, 1, 2, 2048), (4, 2, 3, 1500), (4, 2, 2, 1000)])
def test_advance_by_counts_read_out_of_summary_arrays(ctx, oracle, stride, offset, mult, max_draws):
    import torch
    S = len(COUNTS)
    seeds = _seeds(S)
    gens = [R.Mt19937(x).advance(k) for x, k in zip(seeds, START)]
    st = capi.rng_state(S)
    _upload(st, gens)
    summ = np.full((S, stride), 777777, np.int32)                           # the other columns must not be read as counts
    summ[:, offset] = COUNTS
    d_summ = _dev(summ)
    ctx.rng_advance_batch_dev(S, st.table, d_summ.data_ptr() + 4 * offset, stride, mult, max_draws)
    torch.cuda.synchronize()
    c = [R.consumed(k, mult, max_draws) for k in COUNTS]
    assert c[0] == 0 and c[7] == 0 and c[8] == max_draws and c[1] == mult
    want = [g.copy().advance(k) for g, k in zip(gens, c)]
    _assert_state(st, want, "advance")
    assert all(1 <= g.pos <= 624 for g in want)
    # (a count of 0 left the set bit-identical: want[0] is gens[0], and the set at -5 likewise)
    assert want[0].mt == gens[0].mt and want[0].pos == gens[0].pos
    out = torch.zeros((S, 50), dtype=torch.int32, device="cuda")
    ctx.rng_draw_batch_dev(S, st.table, 50, out.data_ptr())
    torch.cuda.synchronize()
    for s in range(S):
        assert np.array_equal(_u32(out)[s], oracle.mt19937_draws(seeds[s], 50, skip=START[s] + c[s])), (s, START[s], c[s])
    assert np.array_equal(d_summ.cpu().numpy(), summ)


def test_a_position_out_of_range_is_clamped_and_touches_no_other_set(ctx, oracle):
    import torch
    S = 6
    seeds = _seeds(S)
    gens = [R.Mt19937(x).advance(40 + s) for s, x in enumerate(seeds)]
    st = capi.rng_state(S)
    _upload(st, gens)
    st.pos[2] = 100000
    st.pos[4] = -3
    counts = _dev(np.array([10, 0, 10, 700, 10, 1], np.int32))
    out = torch.zeros((S, 30), dtype=torch.int32, device="cuda")
    ctx.rng_draw_batch_dev(S, st.table, 30, out.data_ptr())
    ctx.rng_advance_batch_dev(S, st.table, counts.data_ptr(), 1, 1, 2048)
    torch.cuda.synchronize()
    want = [g.copy() for g in gens]
    want[2].pos, want[4].pos = 624, 0                                        # the clamped positions
    drawn = [g.draw(30) for g in want]
    for s, k in enumerate((10, 0, 10, 700, 10, 1)):
        want[s].advance(k)
    for s in range(S):
        assert np.array_equal(_u32(out)[s], drawn[s]), s
        if s not in (2, 4):
            assert np.array_equal(drawn[s], oracle.mt19937_draws(seeds[s], 30, skip=40 + s))
    _assert_state(st, want, "advance behind a bad position")


# ---- 4. RANSAC2 chain ----------------------------------------------------------------------------------------------------------

CHAIN_FRAMES, CHAIN_M, CHAIN_SEEDS = 6, 48, (4649, 4650, 4651)


@functools.lru_cache(maxsize=None)
def _chain_reference():
    """Six frames of three sets and the oracle's RotRansac::fit on them, each set fed from ONE continuous host stream. Set A: an
    exact rotation between its corners (the loop leaves at the first hypothesis with distinct indices); set B: noise and
    outliers (100 hypotheses, 200 draws); set C: one tracked point (skipped, no draw)."""
    from oracle import orc
    from test_gpu_rot_ransac import THR, _cams, _scene
    ocam, _ = _cams(orc, "pinhole")
    M, n = CHAIN_M, 40
    skip = [0, 0, 0]
    frames = []
    for f in range(CHAIN_FRAMES):
        rng = np.random.default_rng(500 + f)
        c1 = np.zeros((3, M, 2), np.float32); c2 = np.zeros((3, M, 2), np.float32); lk = np.zeros((3, M), np.uint8)
        c1[0, :n], c2[0, :n] = _scene(ocam, rng, n, 0, noise=0.0)
        c1[1, :n], c2[1, :n] = _scene(ocam, rng, n, 10, noise=0.3)
        c1[2, :n], c2[2, :n] = _scene(ocam, rng, n, 10, noise=0.3)
        lk[0, :n] = 1; lk[1, :n] = 1; lk[2, 7 + f] = 1
        lk[:, n:] = 1                                                        # beyond the count: never picked up
        fr = dict(c1=c1, c2=c2, lk=lk, n=np.full(3, n, np.int32), skip=list(skip), draws=[], ref=[])
        for s in range(3):
            d = orc.mt19937_draws(CHAIN_SEEDS[s], 200, skip=skip[s])
            fr["draws"].append(d)
            if s == 2:
                fr["ref"].append(None)
                continue
            st_o, R_o, best_o, used_o = orc.rot_ransac_fit(c1[s, :n], c2[s, :n], ocam, ocam, d, THR)
            fr["ref"].append((st_o, R_o, best_o, used_o))
            skip[s] += used_o
        frames.append(fr)
    return frames, skip


class _ChainBuffers:
    def __init__(self):
        import torch
        M = CHAIN_M
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        self.n, self.c1, self.c2 = z(3, torch.int32), z((3, M, 2), torch.float32), z((3, M, 2), torch.float32)
        self.lk, self.draws = z((3, M), torch.uint8), z((3, 200), torch.int32)
        self.st, self.R, self.summ = z((3, M), torch.int32), z((3, 9), torch.float32), z((3, 2), torch.int32)
        self.rng = capi.rng_state(3)

    def load(self, fr):
        self.n.copy_(_dev(fr["n"])); self.c1.copy_(_dev(fr["c1"])); self.c2.copy_(_dev(fr["c2"])); self.lk.copy_(_dev(fr["lk"]))
        self.st.fill_(-7); self.R.fill_(7.0); self.summ.fill_(-1); self.draws.fill_(0)

    def frame(self, ctx, gcam, thr):
        """draw -> RANSAC2 -> advance by two draws per hypothesis visited."""
        P = lambda x: x.data_ptr()
        ctx.rng_draw_batch_dev(3, self.rng.table, 200, P(self.draws))
        ctx.rot_ransac_lk_batch_dev(3, CHAIN_M, P(self.n), P(self.c1), P(self.c2), P(self.lk), 1, gcam, gcam, P(self.draws), thr, P(self.st),
                                    P(self.R), P(self.summ))
        ctx.rng_advance_batch_dev(3, self.rng.table, P(self.summ) + 4, 2, 2, 200)

    def check(self, fr, what):
        st, Rm, summ, draws = self.st.cpu().numpy(), self.R.cpu().numpy(), self.summ.cpu().numpy(), _u32(self.draws)
        for s in range(3):
            assert np.array_equal(draws[s], fr["draws"][s]), (what, s, "the draws are the host stream at the accumulated skip", fr["skip"][s])
            if fr["ref"][s] is None:                                         # skipped: ransac_pipeline.cpp:209
                assert summ[s].tolist() == [0, 0] and (st[s] == -7).all() and (Rm[s] == 7.0).all(), (what, s)
                continue
            st_o, R_o, best_o, used_o = fr["ref"][s]
            n = len(st_o)
            assert np.array_equal(st[s, :n], st_o) and (st[s, n:] == -7).all(), (what, s)
            assert summ[s].tolist() == [best_o, used_o // 2], (what, s, summ[s], best_o, used_o)
            assert np.array_equal(Rm[s].view(np.uint32), R_o.reshape(-1).view(np.uint32)), (what, s)


def test_the_chain_reference_has_the_three_kinds_of_sets():
    frames, total = _chain_reference()
    for fr in frames:
        assert fr["ref"][0][3] < 200 and fr["ref"][0][2] == 40               # A: every point an inlier, left early
        assert fr["ref"][1][3] == 200 and fr["ref"][1][2] < 40               # B: all 100 hypotheses
    assert total[1] == 200 * CHAIN_FRAMES and total[2] == 0 and 0 < total[0] < 200 * CHAIN_FRAMES
    assert len(set(total)) == 3


def test_ransac2_chain_consumes_what_the_reference_consumes(ctx):
    import torch
    from oracle import orc
    from test_gpu_rot_ransac import THR, _cams
    _, gcam = _cams(orc, "pinhole")
    frames, total = _chain_reference()
    b = _ChainBuffers()
    d_seeds = _dev(np.array(CHAIN_SEEDS, np.uint32))
    ctx.rng_seed_batch_dev(3, b.rng.table, seed_dev=d_seeds.data_ptr())
    for f, fr in enumerate(frames):
        b.load(fr)
        b.frame(ctx, gcam, THR)
        torch.cuda.synchronize()
        b.check(fr, f"frame {f}")
    _assert_state(b.rng, [R.Mt19937(x).advance(k) for x, k in zip(CHAIN_SEEDS, total)], "after six frames")
    assert len(set(total)) == 3 and total[0] != 200 * CHAIN_FRAMES and total[2] != 200 * CHAIN_FRAMES


# ---- 5. shuffle chain ----------------------------------------------------------------------------------------------------------

SHUFFLE_M, SHUFFLE_SEEDS = 8, (5489, 77)
SHUFFLE_COUNTS = ((5, 2), (8, 6), (3, 1))                                   # tracks of (set 0, set 1) per frame


@functools.lru_cache(maxsize=None)
def _shuffle_reference():
    """Three frames of two sequences through the restatement of the index, each fed from ONE continuous host stream: per frame and
    set the record that the helpers of test_gpu_trail_index.py read, and the draws each stream has consumed at the end."""
    from oracle import orc
    from test_gpu_trail_index import PLAIN, _cams, _pack, _params
    M, seeds = SHUFFLE_M, SHUFFLE_SEEDS
    p, _ = _params(M, 4, 2, False, T.GAP, trackMinFrames=2)
    ocam, _ = _cams(PLAIN)
    ses = [T.Session(p, R3.normalize_pixel) for _ in seeds]
    skip = [0] * len(seeds)
    rng = np.random.default_rng(3)
    xy = rng.uniform([40, 40], [700, 440], (len(seeds), M, 2)).astype(np.float32)
    frames = []
    for f, cnt in enumerate(SHUFFLE_COUNTS):
        xy = (xy + rng.uniform(-2, 2, xy.shape)).astype(np.float32)
        frs = []
        for s in range(len(seeds)):
            table = [(10 * s + i + 1, (xy[s, i, 0], xy[s, i, 1]), None) for i in range(cnt[s])]    # IDs persist: tracks grow longer
            draws = orc.mt19937_draws(seeds[s], M, skip=skip[s])
            sel = ses[s].select(table, (ocam, ocam), True, True, f + 1, 0.1 * (f + 1), draws)
            after_select = _pack(ses[s].state(), 1)
            n_cand = len(sel["candidates"])
            tri, gate = [T.TRI_OK] * n_cand, [T.INLIER] * n_cand             # every visit a success: nothing is blacklisted
            fin = ses[s].finish(tri, gate, False)
            skip[s] += sel["draws_used"]
            frs.append(dict(table=table, keyframe=True, full=True, frame_num=f + 1, time=0.1 * (f + 1), draws=np.zeros(M, np.uint32),
                            host_draws=draws, select=sel, after_select=after_select, tri=tri, gate=gate, stationary=False, finish=fin,
                            after_finish=_pack(ses[s].state(), 1)))
        frames.append(frs)
    return frames, skip


def test_the_shuffle_reference_consumes_a_different_count_every_frame():
    frames, skip = _shuffle_reference()
    used = [tuple(fr["select"]["draws_used"] for fr in frs) for frs in frames]
    assert used == [(4, 1), (7, 5), (2, 0)] and skip == [13, 6]
    assert sum(len(fr["select"]["candidates"]) for frs in frames for fr in frs) >= 4      # the order shows in the candidates
    # the shuffle did something: some frame's order is not the table order
    assert any(fr["select"]["order"] != sorted(fr["select"]["order"]) for frs in frames for fr in frs)


def test_shuffle_chain_advances_by_draws_used(ctx):
    """Three frames of two sets with maxTracks = 8: draw(8) -> hv_trail_select_batch_dev -> advance(draws_used) -> finish against
    the restatement of the index fed from one continuous stream per set. The sets' track counts change from frame to frame, and
    with them draws_used = n - 1. The order (through the candidates' positions in it), the candidates, the index and the final
    generator state must all be equal."""
    import torch
    from test_gpu_trail_index import PLAIN, DevTrail, _assert_finish, _assert_select, _assert_state as _assert_index, _cams, _pack_dev, _params
    M, S, seeds = SHUFFLE_M, len(SHUFFLE_SEEDS), SHUFFLE_SEEDS
    frames, skip = _shuffle_reference()
    _, gp = _params(M, 4, 2, False, T.GAP, trackMinFrames=2)
    _, gcam = _cams(PLAIN)
    dt = DevTrail(S, gp, False)
    dt.init(ctx)
    st = capi.rng_state(S)
    d_seeds = _dev(np.array(seeds, np.uint32))
    ctx.rng_seed_batch_dev(S, st.table, seed_dev=d_seeds.data_ptr())
    for f, frs in enumerate(frames):
        dt.load_select_inputs(frs)                                           # (uploads zeros as draws: the device's own must be used)
        dt.load_finish_inputs(frs)
        ctx.rng_draw_batch_dev(S, st.table, M, dt.i["draws"].data_ptr())
        dt.select(ctx, gcam, gcam)
        ctx.rng_advance_batch_dev(S, st.table, dt.o["draws_used"].data_ptr(), 1, 1, M)
        torch.cuda.synchronize()
        h = dt.host()
        for s, fr in enumerate(frs):
            what = f"frame {f} set {s}"
            assert np.array_equal(_u32(dt.i["draws"])[s], fr["host_draws"]), what
            assert h["draws_used"][s] == SHUFFLE_COUNTS[f][s] - 1, what
            _assert_select(h, s, fr, dt, what)
            _assert_index(_pack_dev(h, s, dt.K, dt.ncam, False), fr["after_select"], what)
        dt.finish(ctx)
        torch.cuda.synchronize()
        h = dt.host()
        for s, fr in enumerate(frs):
            _assert_finish(h, s, fr, f"finish frame {f} set {s}")
            _assert_index(_pack_dev(h, s, dt.K, dt.ncam, True), fr["after_finish"], f"finish frame {f} set {s}")
    _assert_state(st, [R.Mt19937(x).advance(k) for x, k in zip(seeds, skip)], "after three frames")


# ---- 6. graph ------------------------------------------------------------------------------------------------------------------

def test_captured_chain_replays_with_the_stream_moving_on():
    """[draw(200) -> hv_rot_ransac_lk_batch_dev -> advance] captured once on a lane's stream, after one eager frame (the library's
    capture rule), then replayed four times with new corners copied into the same buffers: the draws buffer follows the host
    stream at the accumulated skip, statuses, R and summaries equal the oracle's on the chain's frames 1 .. 4. The random numbers
    of a replayed frame come from nowhere but the device."""
    import torch
    from oracle import orc
    from test_gpu_rot_ransac import THR, _cams
    _, gcam = _cams(orc, "pinhole")
    frames, _ = _chain_reference()
    with capi.Lanes(1, width=64, height=64) as lanes:
        c = lanes.ctx[0]
        stream = torch.cuda.ExternalStream(c.get_stream())
        b = _ChainBuffers()
        d_seeds = _dev(np.array(CHAIN_SEEDS, np.uint32))
        b.load(frames[0])
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            c.rng_seed_batch_dev(3, b.rng.table, seed_dev=d_seeds.data_ptr())
            b.frame(c, gcam, THR)
        torch.cuda.synchronize()
        b.check(frames[0], "eager frame 0")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            b.frame(c, gcam, THR)
        torch.cuda.synchronize()
        # (the capture ran nothing: the state is still the one behind frame 0)
        _assert_state(b.rng, [R.Mt19937(x).advance(k) for x, k in zip(CHAIN_SEEDS, frames[1]["skip"])], "behind the capture")
        for f in range(1, 5):
            b.load(frames[f])
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            b.check(frames[f], f"replay {f}")
        _assert_state(b.rng, [R.Mt19937(x).advance(k) for x, k in zip(CHAIN_SEEDS, frames[5]["skip"])], "after four replays")
        del graph
