"""C ABI of the device std::mt19937 entries (added within ABI 4; no GPU needed): the symbols, the struct layout against the header,
every argument check -- all decided before the context is looked at, so a NULL context touches no device -- and what must not have
changed: ABI 4 and HV_K_COUNT = 20."""
import ctypes as C
import re

from hybvio_amd import capi
from test_output_abi import HEADER, INVALID, UNSUPPORTED, header_members

ENTRIES = ("hv_rng_seed_batch_dev", "hv_rng_draw_batch_dev", "hv_rng_advance_batch_dev")


def test_symbols_abi_version_and_timer_classes():
    L = capi.lib()
    for s in ENTRIES:
        assert hasattr(L, s) and s in capi.PROTOTYPES, s
    assert L.hv_abi_version() == 4
    text = open(HEADER).read()
    assert "HV_K_COUNT = 20 }" in text                                     # no timer class was added: HV_K_TRAIL_INDEX
    assert "hv_rng_*_batch_dev" in next(ln for ln in text.splitlines() if "HV_K_TRAIL_INDEX = 19" in ln)
    assert int(re.search(r"#define HV_RNG_STATE_WORDS\s+(\d+)", text).group(1)) == capi.RNG_STATE_WORDS == 624
    max_draws = int(re.search(r"#define HV_RNG_MAX_DRAWS\s+(\d+)", text).group(1))
    assert max_draws == capi.RNG_MAX_DRAWS == 2048
    assert max_draws >= 3 * int(re.search(r"#define HV_RANSAC3_MAX_ITERS\s+(\d+)", text).group(1))
    assert max_draws >= 2 * int(re.search(r"#define HV_UPRIGHT2P_MAX_ITERS\s+(\d+)", text).group(1))
    assert max_draws >= int(re.search(r"#define HV_TRACKS_MAX_TRACKS\s+(\d+)", text).group(1))


def test_struct_member_order_and_size_match_the_header():
    assert [k for k, _ in capi.RngState._fields_] == header_members("hv_rng") == ["mt", "pos"]
    assert C.sizeof(capi.RngState) == 2 * C.sizeof(C.c_void_p)


def _state(addr):
    return capi.RngState(addr, addr)


def test_every_argument_check_returns_with_a_null_context():
    L = capi.lib()
    buf = (C.c_uint32 * 8)()
    addr = C.addressof(buf)
    a = C.c_void_p(addr)
    st = _state(addr)

    def seed(n=3, st=st, seed_dev=a, kind=a):
        return L.hv_rng_seed_batch_dev(None, n, C.byref(st) if st is not None else None, 4649, seed_dev, kind)

    def draw(n=3, st=st, n_draws=200, out=a):
        return L.hv_rng_draw_batch_dev(None, n, C.byref(st) if st is not None else None, n_draws, out)

    def advance(n=3, st=st, count=a, stride=2, mult=2, max_draws=200):
        return L.hv_rng_advance_batch_dev(None, n, C.byref(st) if st is not None else None, count, stride, mult, max_draws)

    for call in (seed, draw, advance):
        assert call() == INVALID                                           # everything given: the NULL context is what is left
        assert call(n=0) == INVALID and call(n=65535) == INVALID           # supported sizes: still the NULL context
        assert call(st=None) == INVALID
        assert call(st=capi.RngState(None, addr)) == INVALID and call(st=capi.RngState(addr, None)) == INVALID
        assert call(n=-1) == INVALID
        assert call(n=65536) == UNSUPPORTED                                # decided without a context
        assert call(n=65536, st=None) == INVALID                           # invalid and unsupported: invalid
    # the optional arrays of seed
    assert seed(seed_dev=None, kind=None) == INVALID
    # draw
    assert draw(out=None) == INVALID
    assert draw(n_draws=0) == INVALID and draw(n_draws=-5) == INVALID
    assert draw(n_draws=1) == INVALID and draw(n_draws=2048) == INVALID    # the limits themselves are supported
    assert draw(n_draws=2049) == UNSUPPORTED
    assert draw(n_draws=2049, out=None) == INVALID
    # advance
    assert advance(count=None) == INVALID
    assert advance(stride=0) == INVALID and advance(stride=-1) == INVALID
    assert advance(mult=0) == INVALID and advance(mult=-2) == INVALID
    assert advance(max_draws=-1) == INVALID
    assert advance(max_draws=0) == INVALID and advance(max_draws=2048) == INVALID
    assert advance(max_draws=2049) == UNSUPPORTED
    assert advance(max_draws=2049, mult=0) == INVALID
    for stride, mult in ((1, 1), (2, 2), (4, 3), (4, 2)):
        assert advance(stride=stride, mult=mult) == INVALID


def test_allocator_and_binding_shapes():
    st = capi.rng_state(5, device="cpu")
    assert tuple(st.mt.shape) == (5, 624) and tuple(st.pos.shape) == (5,)
    assert st.mt.element_size() == 4 and st.pos.element_size() == 4
    assert st.table.mt == st.mt.data_ptr() and st.table.pos == st.pos.data_ptr()
    for m in ("rng_seed_batch_dev", "rng_draw_batch_dev", "rng_advance_batch_dev"):
        assert callable(getattr(capi.Context, m))
