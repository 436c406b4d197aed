"""GPU tests of hv_match_intensities_batch_dev, hv_intensity_init_batch_dev, hv_match_intensities and the C++ adapter against
tests/intensity_match_restatement.py. Pixels, the sums, prev_sum, prev_sqsum, has_prev and the flags are integers and must be EQUAL;
the record's doubles (k, mean0, mean) must be within 4 ulp -- each is a chain of at most three divisions or square roots, and 4 ulp
of k move a table entry by at most 255 * 4 * 2^-52 ~ 2e-13, four orders of magnitude inside the 1e-9 that
test_intensity_match_restatement.py demands of every fixture here, so pixel equality does not rest on that bound.

The fixtures and their expected results are tests/intensity_match_cases.py (computed once per case, shared). Every buffer carries
poisoned padding between the width and the row stride, and a poisoned row behind each image; both must come back unchanged."""
import os
import subprocess

import numpy as np
import pytest

import intensity_match_cases as K
import intensity_match_restatement as R
from hybvio_amd import build, capi

pytestmark = pytest.mark.gpu
POISON = 0xA5
MAX_ULP = 4
SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_intensity_match_adapter.cpp")


@pytest.fixture(scope="module")
def ctx():
    import torch
    with capi.Context(width=64, height=64) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        yield c
        torch.cuda.synchronize()


def _ulps(got, want):
    return 0.0 if got == want else abs(got - want) / np.spacing(abs(want))


class Buffers:
    """Device frames of a case: [sets][h + 1 rows of `stride` bytes], poisoned, and the state."""

    def __init__(self, case):
        import torch
        self.c = case
        self.image_stride = (case.h + 1) * case.stride
        self.left = torch.empty((case.sets, self.image_stride), dtype=torch.uint8, device="cuda")
        self.right = torch.empty_like(self.left)
        self.state = capi.intensity_state(case.sets)
        self.active = None
        if case.inactive:
            self.active = torch.ones((case.sets,), dtype=torch.uint8, device="cuda")
            self.active[list(case.inactive)] = 0
        self.params = capi.intensity_default_params(matchSuccessiveIntensities=case.successive, matchStereoIntensities=int(case.stereo))

    def _host(self, imgs):
        c = self.c
        buf = np.full((c.sets, c.h + 1, c.stride), POISON, np.uint8)
        buf[:, :c.h, :c.w] = imgs
        return buf.reshape(c.sets, -1)

    def upload(self, L, Rt):
        import torch
        self.left.copy_(torch.from_numpy(self._host(L)))
        self.right.copy_(torch.from_numpy(self._host(Rt)))

    def call(self, ctx):
        c = self.c
        ctx.match_intensities_batch_dev(self.params, c.sets, c.w, c.h, self.left.data_ptr(), self.image_stride,
                                        0 if c.mono else self.right.data_ptr(), self.image_stride, c.stride, self.state.table,
                                        self.active.data_ptr() if self.active is not None else 0, self.state.record.data_ptr())

    def check(self, e, what):
        """Everything the device left behind against Expected e."""
        c = self.c
        assert np.array_equal(self.state.hist.cpu().numpy(), np.zeros((c.sets, 2, 256), np.int32)), (what, "workspace not cleared")
        for name, t, want in (("left", self.left, e.left), ("right", self.right, e.right)):
            got = t.cpu().numpy().reshape(c.sets, c.h + 1, c.stride)
            bad = np.nonzero(got[:, :c.h, :c.w] != want)
            assert len(bad[0]) == 0, (what, name, len(bad[0]), [int(b[0]) for b in bad])
            pad = got.copy()
            pad[:, :c.h, :c.w] = POISON
            assert np.all(pad == POISON), (what, name, "padding written")
        assert [int(x) for x in self.state.prev_sum.cpu().numpy()] == e.prev_sum, what
        assert [int(x) for x in self.state.prev_sqsum.cpu().numpy()] == e.prev_sqsum, what
        assert [int(x) for x in self.state.has_prev.cpu().numpy()] == e.has_prev, what
        worst = 0.0
        for s, (got, want) in enumerate(zip(self.state.records(), e.records)):
            if want is None:
                continue
            assert got.flags == want.flags and got.reserved == 0, (what, s, got.flags, want.flags)
            for f in ("in_sum", "in_sqsum", "out_sum", "out_sqsum"):
                assert list(getattr(got, f)) == getattr(want, f), (what, s, f, list(getattr(got, f)), getattr(want, f))
            for f in ("k", "mean0", "mean"):
                for cam in range(2):
                    u = _ulps(getattr(got, f)[cam], getattr(want, f)[cam])
                    worst = max(worst, u)
                    assert u <= MAX_ULP, (what, s, f, cam, getattr(got, f)[cam], getattr(want, f)[cam], u)
        return worst


def _run(ctx, name):
    import torch
    b = Buffers(K.CASES[name])
    ctx.intensity_init_batch_dev(b.c.sets, b.state.table)
    worst = 0.0
    for f, ((L, Rt), e) in enumerate(zip(K.frames(name), K.expected(name))):
        b.upload(L, Rt)
        b.state.record.fill_(POISON)
        b.call(ctx)
        torch.cuda.synchronize()
        if b.c.inactive:                                                     # an inactive set's record stays bit for bit
            raw = b.state.record.cpu().numpy()
            assert np.all(raw[list(b.c.inactive)] == POISON)
        worst = max(worst, b.check(e, (name, f)))                   # the state is compared after EVERY frame
    print(f"{name}: record doubles within {worst:g} ulp of the restatement")
    return b


# ---- 1. shapes x modes, sets, mask, recursion, special images ----------------------------------------------------------------

SHAPE_MODE = ["480x752_both"] + [f"{s}_{m}" for s in ("97x131", "33x47", "5x7") for m in ("stereo", "successive_mono", "both")]


@pytest.mark.parametrize("name", SHAPE_MODE)
def test_shapes_and_modes(ctx, name):
    """Stereo only, successive only on mono frames (right_dev = NULL: the right buffer must stay as it is), both; two frames each, so
    the second one is matched against the first one's matched statistics. 97 x 131 has a row stride rounded up past the width,
    33 x 47 rows that are not 16-byte aligned, 5 x 7 is dense and shorter than one load."""
    _run(ctx, name)


@pytest.mark.parametrize("name", ["sets1", "sets67"])                       # three sets: every case above
def test_every_set_has_its_own_image(ctx, name):
    """A different crop and gain in every set: a set counted into a neighbour's histogram changes sums and pixels."""
    b = _run(ctx, name)
    assert len({tuple(r.in_sum) for r in b.state.records()}) == b.c.sets


def test_inactive_sets_keep_pixels_state_and_record(ctx):
    """active_dev with inactive sets first, in the middle and last; their state is given a value first so that 'kept' shows."""
    import torch
    name = "mask"
    c = K.CASES[name]
    b = Buffers(c)
    for s in c.inactive:
        b.state.prev_sum[s], b.state.prev_sqsum[s], b.state.has_prev[s] = 1000 + s, 2000 + s, 7
    for f, ((L, Rt), e) in enumerate(zip(K.frames(name), K.expected(name))):
        b.upload(L, Rt)
        b.state.record.fill_(POISON)
        b.call(ctx)
        torch.cuda.synchronize()
        assert np.all(b.state.record.cpu().numpy()[list(c.inactive)] == POISON)
        e = K.Expected(e.left, e.right, e.records, list(e.prev_sum), list(e.prev_sqsum), list(e.has_prev))
        for s in c.inactive:
            e.prev_sum[s], e.prev_sqsum[s], e.has_prev[s] = 1000 + s, 2000 + s, 7
        b.check(e, (name, f))


@pytest.mark.parametrize("name", ["recursion_w025", "recursion_w1"])
def test_four_frame_recursion(ctx, name):
    """Four frames with a brightness drift; prev_sum, prev_sqsum and has_prev are downloaded and compared after every frame."""
    b = _run(ctx, name)
    assert all(r.flags == R.MATCHED_LEFT | R.MATCHED_RIGHT for r in b.state.records())


def test_tables_clamp_at_0_and_at_255(ctx):
    b = _run(ctx, "clamp")
    got = b.right.cpu().numpy().reshape(3, 34, 50)[:, :33, :47]
    assert (got == 0).sum() > 50 and (got == 255).sum() > 50


def test_all_255_and_two_valued_images(ctx):
    b = _run(ctx, "special")
    assert [r.flags for r in b.state.records()] == [R.CONSTANT_LEFT | R.MATCHED_RIGHT, R.MATCHED_LEFT | R.CONSTANT_RIGHT,
                                                    R.MATCHED_LEFT | R.MATCHED_RIGHT]


def test_one_pixel_image_raises_the_constant_flags(ctx):
    b = _run(ctx, "one_pixel")
    assert all(r.flags == R.CONSTANT_LEFT | R.CONSTANT_RIGHT for r in b.state.records())
    assert [int(x) for x in b.state.has_prev.cpu().numpy()] == [1, 1]        # its statistics still became the prev statistics


def test_options_off_and_no_sets_launch_nothing(ctx):
    import torch
    c = K.CASES["33x47_both"]
    b = Buffers(c)
    L, Rt = K.frames("33x47_both")[0]
    b.upload(L, Rt)
    before = (b.left.clone(), b.right.clone())
    b.state.record.fill_(POISON)
    b.params = capi.intensity_default_params()
    b.call(ctx)                                                              # both options off
    b.params = capi.intensity_default_params(matchStereoIntensities=1)
    ctx.match_intensities_batch_dev(b.params, c.sets, c.w, c.h, b.left.data_ptr(), b.image_stride, 0, 0, c.stride, b.state.table)   # mono
    b.params = capi.intensity_default_params(matchSuccessiveIntensities=0.5, matchStereoIntensities=1)
    ctx.match_intensities_batch_dev(b.params, 0, c.w, c.h, b.left.data_ptr(), b.image_stride, b.right.data_ptr(), b.image_stride,
                                    c.stride, b.state.table)
    torch.cuda.synchronize()
    assert torch.equal(b.left, before[0]) and torch.equal(b.right, before[1])
    assert np.all(b.state.record.cpu().numpy() == POISON) and int(b.state.has_prev.sum()) == 0


# ---- 2. chained with the pyramid build ----------------------------------------------------------------------------------------

def test_pyramid_of_the_matched_frames(oracle):
    """Match, then hv_pyramid_build_batch_dev on the same buffers: every gray and gradient level equals oracle.Pyramid of the
    restatement's output, bit for bit."""
    import torch
    name = "97x131_both"
    c = K.CASES[name]
    with capi.Context(width=c.w, height=c.h, pool_size=8) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        b = Buffers(c)
        slots = [ctx.acquire() for _ in range(2 * c.sets)]
        d_slots = torch.tensor(slots, dtype=torch.int32, device="cuda")
        for (L, Rt), e in zip(K.frames(name), K.expected(name)):
            b.upload(L, Rt)
            b.call(ctx)
            ctx.build_batch_dev(c.sets, d_slots.data_ptr(), b.left.data_ptr(), b.image_stride, c.stride)
            ctx.build_batch_dev(c.sets, d_slots.data_ptr() + 4 * c.sets, b.right.data_ptr(), b.image_stride, c.stride)
            ctx.synchronize()
        assert not np.array_equal(e.left, L) and not np.array_equal(e.right, Rt)
        for i, img in enumerate(list(e.left) + list(e.right)):                # the second frame's
            ref = oracle.Pyramid(img, max_level=ctx.levels - 1)
            for l in range(ctx.levels):
                g, d = ctx.download(slots[i], l)
                assert np.array_equal(g, ref.gray(l)), (i, "gray level", l)
                assert np.array_equal(d, ref.deriv(l)), (i, "gradient level", l)


# ---- 3. captured ------------------------------------------------------------------------------------------------------------

def test_captured_call_replays_like_the_eager_one(ctx):
    """The second frame's call captured on the context stream after one eager warm-up, replayed twice from the restored state."""
    import torch
    name = "33x47_both"
    c = K.CASES[name]
    (L0, R0), (L1, R1) = K.frames(name)
    e0, e1 = K.expected(name)
    b = Buffers(c)
    ctx.intensity_init_batch_dev(c.sets, b.state.table)
    b.upload(L0, R0)
    b.call(ctx)                                                              # eager: frame 0 (also the warm-up)
    torch.cuda.synchronize()
    b.check(e0, "eager frame 0")
    saved = [t.clone() for t in (b.state.prev_sum, b.state.prev_sqsum, b.state.has_prev)]
    b.upload(L1, R1)
    b.call(ctx)                                                              # eager: frame 1
    torch.cuda.synchronize()
    b.check(e1, "eager frame 1")
    eager = [t.clone() for t in (b.left, b.right, b.state.record, b.state.prev_sum, b.state.prev_sqsum, b.state.has_prev)]
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)
        try:
            for t, s in zip((b.state.prev_sum, b.state.prev_sqsum, b.state.has_prev), saved):
                t.copy_(s)
            b.upload(L1, R1)
            stream.synchronize()
            with torch.cuda.graph(graph, stream=stream):
                b.call(ctx)
            for replay in range(2):
                for t, s in zip((b.state.prev_sum, b.state.prev_sqsum, b.state.has_prev), saved):
                    t.copy_(s)
                b.upload(L1, R1)
                b.state.record.fill_(POISON)
                graph.replay()
                stream.synchronize()
                b.check(e1, ("replay", replay))
                now = (b.left, b.right, b.state.record, b.state.prev_sum, b.state.prev_sqsum, b.state.has_prev)
                assert all(torch.equal(x, y) for x, y in zip(now, eager)), ("replay", replay)
        finally:
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    del graph


# ---- 4. one-pair host entry and the C++ adapter ---------------------------------------------------------------------------------

def test_one_pair_host_entry(ctx):
    """hv_match_intensities = matchIntensities(l, r, weight) at 97 x 131, contiguous and strided rows; l is only read."""
    for l, r, w in K.host_pairs():
        want = R.match_intensities(l, r, w)
        assert not np.array_equal(want, r)
        l_before = l.copy()
        assert np.array_equal(ctx.match_intensities(l, r, w), want)
        assert np.array_equal(l, l_before)
        wide = np.full((97, 160), POISON, np.uint8)                          # l with a row stride of its own
        wide[:, :131] = l
        assert np.array_equal(ctx.match_intensities(wide[:, :131], r, w), want)
        assert np.all(wide[:, 131:] == POISON)
    flat = np.full((97, 131), 77, np.uint8)
    assert np.array_equal(ctx.match_intensities(l, flat, 1.0), flat)         # a constant r stays as it is


def _build_adapter(out_dir):
    lib, _ = build.build_host()
    libdir = os.path.dirname(lib)
    exe = os.path.join(out_dir, "test_intensity_match_adapter")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", exe, SRC, "-L" + libdir, "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-lhybvio_host", "-lhybvio_hip"])
    return exe


def test_match_through_the_cpp_adapter(tmp_path):
    """hybvio::tracker::util::matchIntensities on a session: the program reads l and r (r with a padded row stride), writes the
    matched r for weight 1 (the default argument) and for 0.25."""
    exe = _build_adapter(str(tmp_path))
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "libhybvio_host.so" in needed and "amdhip64" not in needed
    (l, r, _), _ = K.host_pairs()
    h, w, stride = 97, 131, 144
    with open(tmp_path / "dims.txt", "w") as f:
        f.write(f"{w} {h} {stride} 0.25\n")
    l.tofile(str(tmp_path / "l.raw"))
    padded = np.full((h, stride), POISON, np.uint8)
    padded[:, :w] = r
    padded.tofile(str(tmp_path / "r.raw"))
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    for fname, weight in (("r_default.raw", 1.0), ("r_weighted.raw", 0.25)):
        got = np.fromfile(tmp_path / fname, np.uint8).reshape(h, stride)
        assert np.array_equal(got[:, :w], R.match_intensities(l, r, weight)), fname
        assert np.all(got[:, w:] == POISON), fname
