"""The detector's square root (csrc/gftt.hip sqrt_rn: the hardware approximation corrected by the residuals of its two
neighbours, sqrtf below 2^-96) must be the IEEE round-to-nearest root of every non-negative finite binary32, bit for bit as
numpy.sqrt on float32: the response is compared with the oracle to the last bit."""
import numpy as np
import pytest

from hybvio_amd import capi

pytestmark = pytest.mark.gpu

BOUND_BITS = 0x0F800000          # 2^-96, where the cheap path starts


def _inputs():
    rng = np.random.default_rng(20240)
    parts = [np.zeros(1, np.float32),
             np.ldexp(np.float32(1), np.arange(-149, 128)).astype(np.float32)]                     # every power of two
    # 4096 random mantissas for each binary exponent field 0 (denormals) .. 254
    expo = np.repeat(np.arange(0, 255, dtype=np.uint32), 4096)
    parts.append(((expo << 23) | rng.integers(0, 1 << 23, expo.size, dtype=np.uint32)).view(np.float32))
    sq = (np.arange(0, 4097, dtype=np.float64) ** 2).astype(np.float32)                            # exact squares and neighbours
    parts += [sq, np.nextafter(sq, np.float32(np.inf)), np.nextafter(sq[1:], np.float32(0))]
    parts.append(np.arange(BOUND_BITS - 64, BOUND_BITS + 65, dtype=np.uint32).view(np.float32))    # either side of the bound
    parts.append(rng.integers(1, 0x7F800000, 1 << 20, dtype=np.uint32).view(np.float32))           # positive finite patterns
    x = np.concatenate([p.astype(np.float32) for p in parts])
    assert np.isfinite(x).all() and (x >= 0).all()
    return x


@pytest.mark.parametrize("wide", [False, True], ids=["scalar", "four_at_once"])
def test_sqrt_helper_is_correctly_rounded(wide):
    """scalar: sqrt_rn of the tiled and the box kernel; four_at_once: sqrt_rn4 of the marching kernel (a rare argument sends the
    whole wave through the branch, its neighbours in the group of four included)"""
    import torch
    x = _inputs()
    assert x[1] == np.float32(2.0 ** -149) and x[277] == np.float32(2.0 ** 127)
    with np.errstate(all="ignore"):
        ref = np.sqrt(x)
    assert ref.dtype == np.float32
    with capi.Context(width=64, height=64, pool_size=1) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        xd = torch.from_numpy(x).cuda()
        yd = torch.full_like(xd, -1.0)
        ctx.gftt_sqrt_dev(xd.data_ptr(), yd.data_ptr(), x.size, wide)
        torch.cuda.synchronize()
        got = yd.cpu().numpy()
    bad = np.nonzero(got.view(np.uint32) != ref.view(np.uint32))[0]
    assert bad.size == 0, (bad.size, [(hex(int(x.view(np.uint32)[i])), hex(int(got.view(np.uint32)[i])), hex(int(ref.view(np.uint32)[i]))) for i in bad[:5]])
