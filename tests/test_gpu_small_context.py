"""A context for an image that is not larger than the 31-pixel LK window: hv_create serves it with a pyramid of one level (the
detector and the pyramid build work on it), and every LK entry answers HV_ERR_UNSUPPORTED instead of tracking through levels
its reflection and tile staging are not laid out for."""
import numpy as np
import pytest

from hybvio_amd import capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(8, 8), (31, 40), (40, 31)])
def test_small_context_builds_detects_and_refuses_lk(oracle, shape):
    import torch
    h, w = shape
    rng = np.random.default_rng(h * 100 + w)
    imgs = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(2)]
    with capi.Context(width=w, height=h, pool_size=2) as ctx:
        assert ctx.levels == 1 and ctx.level_sizes == [(w, h)]
        slots = []
        for im in imgs:
            s = ctx.acquire(); ctx.build(s, im); slots.append(s)
        gp = capi.gftt_default_params(gfttMinDistance=8.0)
        for s, im in zip(slots, imgs):                                    # the detector reads the level-0 image the build left
            assert np.array_equal(ctx.gftt_detect(s, params=gp), oracle.gftt_detect(im, mask_radius=0, min_distance=8.0))
        pts = np.array([[w / 2, h / 2], [1.0, 1.0]], np.float32)
        with pytest.raises(capi.HvError, match="unsupported"):
            ctx.klt_track(slots[0], slots[1], pts)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        sl = torch.tensor(slots, dtype=torch.int32, device="cuda")
        xy = torch.from_numpy(pts).cuda()
        out, st, err = torch.zeros_like(xy), torch.zeros(2, dtype=torch.uint8, device="cuda"), torch.zeros(2, device="cuda")
        with pytest.raises(capi.HvError, match="unsupported"):
            ctx.klt_track_batch_dev(1, sl[:1].data_ptr(), sl[1:].data_ptr(), 2, xy.data_ptr(), out.data_ptr(), st.data_ptr(), err.data_ptr(), False)
        torch.cuda.synchronize()
