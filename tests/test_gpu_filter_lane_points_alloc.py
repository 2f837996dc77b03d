"""Device memory of the mask chain's arenas is given back.

lt_filter_lane_points runs the chain on a one-slot arena of its own for the length of a call (one frame: the one-frame top-hat
kernels, which need no boundary zones); live device bytes (the library's own account, lt_device_cache_stats) are the same before
and after 20 calls.  A context's arena allocates the split-band walks' boundary zones with its first batch chain of three or
more frames and frees them with everything else when the context closes: live bytes return to where they were across
create / filter_run(3) / close cycles."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_filter_lane_points_leaves_no_device_memory_behind():
    from lane_tracker_amd import _native, calib
    cal = calib.reference_calibration()
    ctx = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], device=0, capacity=2)
    try:
        rng = np.random.default_rng(7)
        imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w) in ((236, 188), (240, 256))]
        first = [ctx.filter_lane_points(im) for im in imgs]            # whatever a first call sets up for good
        live = _native.device_cache_stats()["live_bytes"]
        for i in range(20):
            im = imgs[i % 2]
            fp = _native.filter_params(mask_noise=bool(i & 2))
            out = ctx.filter_lane_points(im, fp)
            if not (i & 2):
                assert np.array_equal(out, first[i % 2])
        assert _native.device_cache_stats()["live_bytes"] == live
    finally:
        ctx.close()


def test_boundary_zones_of_a_batch_chain_are_freed_with_the_context():
    from lane_tracker_amd import _native, calib
    cal = calib.reference_calibration()
    rng = np.random.default_rng(11)
    bev = rng.integers(0, 256, (3, 236, 188, 3), dtype=np.uint8)
    before = None
    for cycle in range(3):
        ctx = _native.Context(cal["img_size"], (188, 236), cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], device=0, capacity=3)
        try:
            if before is None:
                before_ctx = _native.device_cache_stats()["live_bytes"]
            ctx.upload_bev(bev)
            ctx.filter_run(3)
            assert ctx.last_tophat_path() in (0, 1, 2, 3)
            grown = _native.device_cache_stats()["live_bytes"]
            ctx.filter_run(3)                                   # a second chain allocates nothing more
            assert _native.device_cache_stats()["live_bytes"] == grown
        finally:
            ctx.close()
        after = _native.device_cache_stats()["live_bytes"]
        if before is None:
            before = after
        assert after == before, (cycle, before, after)
    assert grown >= before_ctx
