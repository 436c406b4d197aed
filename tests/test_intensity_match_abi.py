"""C ABI of the intensity-matching entries (added within ABI 4; no GPU needed): the symbols and defaults, the struct layouts against
the header, every argument check -- all decided before the context is looked at, so a NULL context touches no device --, the C++
adapter's symbol, and what must not have changed: ABI 4, HV_K_COUNT = 20 and a host library that does not link the HIP runtime."""
import ctypes as C
import subprocess

from hybvio_amd import build, capi
from test_output_abi import HEADER, INVALID, UNSUPPORTED, header_members

ENTRIES = ("hv_intensity_default_params", "hv_intensity_init_batch_dev", "hv_match_intensities_batch_dev", "hv_match_intensities")


def test_symbols_defaults_abi_version_and_timer_classes():
    L = capi.lib()
    for s in ENTRIES:
        assert hasattr(L, s) and s in capi.PROTOTYPES, s
    assert L.hv_abi_version() == 4
    text = open(HEADER).read()
    assert "HV_K_COUNT = 20 }" in text                                      # no timer class was added: HV_K_INGEST
    assert "#define HV_ABI_VERSION 4 " in text
    p = capi.intensity_default_params()
    assert p.matchSuccessiveIntensities == 0.0 and p.matchStereoIntensities == 0     # codegen/parameter_definitions.c:533-534
    L.hv_intensity_default_params(None)                                      # tolerated
    q = capi.intensity_default_params(matchSuccessiveIntensities=0.25, matchStereoIntensities=1)
    assert (q.matchSuccessiveIntensities, q.matchStereoIntensities) == (0.25, 1)
    for name, bit in (("CONSTANT_LEFT", 1), ("CONSTANT_RIGHT", 2), ("MATCHED_LEFT", 4), ("MATCHED_RIGHT", 8)):
        assert f"HV_INTENSITY_{name} = {bit}" in text


def test_struct_member_order_and_size_match_the_header():
    assert [k for k, _ in capi.IntensityParams._fields_] == header_members("hv_intensity_params")
    assert [k for k, _ in capi.IntensityState._fields_] == header_members("hv_intensity_state") == ["prev_sum", "prev_sqsum", "has_prev", "hist"]
    assert [k for k, _ in capi.IntensityRecord._fields_] == header_members("hv_intensity_record")
    assert C.sizeof(capi.IntensityState) == 4 * C.sizeof(C.c_void_p)
    assert C.sizeof(capi.IntensityRecord) == 8 * 8 + 6 * 8 + 8 and C.sizeof(capi.IntensityParams) == 16


def test_every_argument_check_returns_with_a_null_context():
    L = capi.lib()
    buf = (C.c_uint64 * 8)()
    addr = C.addressof(buf)
    a = C.c_void_p(addr)
    full = capi.IntensityState(addr, addr, addr, addr)
    both = capi.intensity_default_params(matchSuccessiveIntensities=0.5, matchStereoIntensities=1)
    stereo = capi.intensity_default_params(matchStereoIntensities=1)

    def ref(x):
        return C.byref(x) if x is not None else None

    def match(p=both, n=3, w=752, h=480, left=a, right=a, row=752, st=full, active=a, rec=a):
        return L.hv_match_intensities_batch_dev(None, ref(p), n, w, h, left, 480 * row, right, 480 * row, row, ref(st), active, rec)

    assert match() == INVALID                                               # everything given: the NULL context is what is left
    assert match(n=0) == INVALID and match(n=65535) == INVALID and match(w=65535, row=65535, h=65535) == INVALID
    assert match(right=None, active=None, rec=None) == INVALID              # the optional pointers
    assert match(p=capi.intensity_default_params()) == INVALID              # both options off: still the NULL context
    assert match(p=None) == INVALID and match(left=None) == INVALID and match(st=None) == INVALID
    assert match(st=capi.IntensityState(addr, addr, addr, None)) == INVALID
    for st in (capi.IntensityState(None, addr, addr, addr), capi.IntensityState(addr, None, addr, addr),
               capi.IntensityState(addr, addr, None, addr)):
        assert match(st=st) == INVALID                                      # the successive step needs them ...
        assert match(p=stereo, st=st, n=65536) == UNSUPPORTED               # ... the stereo step alone does not
    for w in (-0.25, 1.0001, float("nan"), float("inf")):
        assert match(p=capi.intensity_default_params(matchSuccessiveIntensities=w), n=65536) == INVALID
    assert match(p=capi.intensity_default_params(matchSuccessiveIntensities=1.0), n=65536) == UNSUPPORTED    # the limit itself
    assert match(n=-1) == INVALID
    assert match(w=0) == INVALID and match(h=0) == INVALID and match(w=-3) == INVALID and match(h=-3) == INVALID
    assert match(row=751) == INVALID
    # decided without a context
    assert match(n=65536) == UNSUPPORTED
    assert match(w=65536, row=65536) == UNSUPPORTED and match(h=65536) == UNSUPPORTED
    assert match(n=65536, left=None) == INVALID and match(w=65536, row=65535) == INVALID          # invalid and unsupported: invalid

    def init(n=3, st=full):
        return L.hv_intensity_init_batch_dev(None, n, ref(st))

    assert init() == INVALID and init(n=0) == INVALID and init(n=65535) == INVALID
    assert init(st=None) == INVALID and init(n=-1) == INVALID
    for i in range(4):
        members = [addr] * 4
        members[i] = None
        assert init(st=capi.IntensityState(*members)) == INVALID
        assert init(n=65536, st=capi.IntensityState(*members)) == INVALID
    assert init(n=65536) == UNSUPPORTED

    def pair(w=131, h=97, l=a, r=a, ls=144, rs=131, weight=1.0):
        return L.hv_match_intensities(None, w, h, l, ls, r, rs, weight)

    assert pair() == INVALID and pair(weight=0.0) == INVALID and pair(w=65535, ls=65535, rs=65535, h=65535) == INVALID
    assert pair(l=None) == INVALID and pair(r=None) == INVALID
    assert pair(w=0) == INVALID and pair(h=0) == INVALID and pair(ls=130) == INVALID and pair(rs=130) == INVALID
    for w in (-0.25, 1.0001, float("nan")):
        assert pair(weight=w, h=65536) == INVALID
    assert pair(h=65536) == UNSUPPORTED and pair(w=65536, ls=65536, rs=65536) == UNSUPPORTED
    assert pair(h=65536, r=None) == INVALID


def test_allocator_and_binding_shapes():
    st = capi.intensity_state(5, device="cpu")
    assert tuple(st.prev_sum.shape) == tuple(st.prev_sqsum.shape) == tuple(st.has_prev.shape) == (5,)
    assert st.prev_sum.element_size() == 8 and st.has_prev.element_size() == 4
    assert tuple(st.hist.shape) == (5, 2, 256) and st.hist.element_size() == 4
    assert tuple(st.record.shape) == (5, C.sizeof(capi.IntensityRecord))
    assert (st.table.prev_sum, st.table.hist) == (st.prev_sum.data_ptr(), st.hist.data_ptr())
    recs = st.records()
    assert len(recs) == 5 and recs[0].flags == 0 and list(recs[0].k) == [0.0, 0.0]
    for m in ("intensity_init_batch_dev", "match_intensities_batch_dev", "match_intensities"):
        assert callable(getattr(capi.Context, m))


def test_adapter_symbol_is_exported_and_the_host_library_links_only_the_c_abi():
    host, _ = build.build_host()
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", host], text=True)
    assert "hybvio::tracker::util::matchIntensities(hybvio::Session&, hybvio::tracker::GrayImage const&, hybvio::tracker::GrayImage&, double)" in syms
    needed = subprocess.check_output(["readelf", "-d", host], text=True)
    assert "libhybvio_hip.so" in needed and "amdhip64" not in needed
