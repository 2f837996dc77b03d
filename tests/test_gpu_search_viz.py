"""Search visualisation and split view on the device (lt_search_viz_run, lt_split_panes_run, lt_resize_linear_u8) and in the stream
pipeline (`process_batch` / `process_stream` with `visualize_search=True` / `split_view=True`).  Every comparison is bit for bit:
against the fixtures the reference's own visualisation methods produced (tests/golden/viz_*.npz), against `overlay.py` /
`utils.resize_linear` (which tests/test_presentation_cpu.py holds to those fixtures), and against `process()` frame by frame.
Reference: lane_tracker.py:687-793, 1130-1137."""
import numpy as np
import pytest

from helpers import golden_files, params_of, unpack_mask
from lane_tracker_amd import _native, calib, overlay, synth, utils
from lane_tracker_amd.device import DeviceFrames
from lane_tracker_amd.lane_tracker import LaneTracker

pytestmark = pytest.mark.gpu


def _ctx(cal, capacity):
    return _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0],
                           device=0, capacity=capacity)


def _points(size, left, right, partial=1):
    """get_poly_points as (left (y, x) pairs, right (y, x) pairs) and as upstream's four arrays."""
    h = size[1]
    ploty = np.linspace(h * (1 - partial), h - 1, int(h * partial))
    _, _, lyx, ryx = _native.poly_points(size, np.concatenate([left, right])[None], ploty, ploty ** 2)
    return (lyx, ryx), (lyx[:, 0].astype(np.int64), lyx[:, 1].astype(np.int64), ryx[:, 0].astype(np.int64), ryx[:, 1].astype(np.int64))


_NONE = np.zeros((0, 2), np.int32)


def _run(ctx, descs, panes=False):
    """descs: (slot, kind, dict of lt_viz_item fields, fit pairs or None, band pairs or None) -> the pictures."""
    items = np.zeros(len(descs), _native.VIZ_ITEM_DTYPE)
    lists = [[], [], [], []]
    for q, (slot, kind, kw, fit, band) in enumerate(descs):
        items[q]["slot"], items[q]["kind"] = slot, kind
        for k, v in kw.items():
            items[q][k] = v
        for c, pts in enumerate((fit or (_NONE, _NONE)) + (band or (_NONE, _NONE))):
            lists[c].append(pts)
            items[q][("n_fit_left", "n_fit_right", "n_band_left", "n_band_right")[c]] = len(pts)
    lists = [np.concatenate(a) if a else _NONE for a in lists]
    return (ctx.split_panes_run if panes else ctx.search_viz_run)(items, *lists)


def _expected(ctx, slot, kind, kw, fit4, band4):
    """The picture of a slot by overlay.py, fed from what the device reports for it."""
    mask = ctx.download_masks(1, first=slot)[0]
    ly, lx, ry, rx, cl, cr = tuple(ctx.download_lane_lists(slot, kind == 1))[:6]
    if kind == 1:
        return overlay.visualize_sliding_window_search(mask, cl, cr, (ly, lx), (ry, rx), fit4, kw["window_width"], kw["window_height"],
                                                       kw["ignore_bottom"])
    return overlay.visualize_band_search(mask, (ly, lx), (ry, rx), band4, fit4, kw["bandwidth"])


def test_fixture_pictures_from_uploaded_masks():
    """Searches over uploaded masks (packed lists, form 0, among them): the reference's own pictures."""
    cal = calib.reference_calibration()
    size = cal["warped_size"]
    files = golden_files("viz_sws_") + golden_files("viz_band_")
    assert len(files) >= 6
    ctx = _ctx(cal, len(files))
    try:
        descs, want = [], []
        for slot, path in enumerate(files):
            d = np.load(path)
            mask = unpack_mask(d)
            ctx.upload_masks(mask[None], first=slot)
            if str(d["kind"]) == "sws":
                p = params_of(d)
                ctx.sws_fit_run(1, _native.search_params(**p), first=slot)
                fit, _ = _points(size, d["left_coeffs"], d["right_coeffs"])
                descs.append((slot, 1, dict(window_width=p["window_width"], window_height=p["window_height"], ignore_bottom=p["ignore_bottom"]),
                              fit, None))
                want.append(d["vis"])
            else:
                bw, partial = int(d["param_bandwidth"]), d["param_partial"].item()
                ctx.band_fit_run(1, np.concatenate([d["prev_left"], d["prev_right"]]),
                                 _native.search_params(bandwidth=bw, ignore_bottom=30, partial=partial), first=slot)
                band, band4 = _points(size, d["prev_left"], d["prev_right"], partial)
                if bool(d["detected"]):
                    fit, _ = _points(size, d["left_coeffs"], d["right_coeffs"])
                    want.append(d["vis"])
                else:                    # nothing to fit: the band and whatever one side found
                    fit = None
                    want.append(_expected(ctx, slot, 2, dict(bandwidth=bw), (np.zeros(0, np.int64),) * 4, band4))
                descs.append((slot, 2, dict(bandwidth=bw), fit, band))
        assert 0 in {int(r["_pad"]) for r in ctx.download_records(len(files))}     # (wide windows / bands leave packed lists)
        got = _run(ctx, descs)
        for q, path in enumerate(files):
            assert got[q].shape == want[q].shape and np.array_equal(got[q], want[q]), path
        # the bare mask, in the same call as a picture, and in reverse slot order
        two = _run(ctx, [(3, 0, {}, None, None), descs[0]])
        assert np.array_equal(two[0], np.repeat(ctx.download_masks(1, first=3)[0][:, :, None], 3, axis=2)) and np.array_equal(two[1], want[0])
    finally:
        ctx.close()


def test_column_mask_forms_from_the_mask_chain():
    """Forms 1 (k_sws_fit2) and 2 (k_band_fit2 / the chain): masks from the mask chain, lists as column masks per row."""
    cal = calib.reference_calibration()
    size = cal["warped_size"]
    frames = synth.stream_lanes(3, seed=101)
    ctx = _ctx(cal, 3)
    try:
        ctx.upload_frames(frames)
        ctx.mask_run(3)
        sp = dict(window_width=30, window_height=40, ignore_bottom=30)
        ctx.sws_fit_run(1, _native.search_params(**sp), first=0)
        r0 = ctx.download_records(1)[0]
        assert r0["detected"]
        prev = np.concatenate([r0["left_coeffs"], r0["right_coeffs"]])
        ctx.band_fit_run(1, prev, _native.search_params(bandwidth=25, ignore_bottom=30, partial=1.0), first=1)
        ctx.band_fit_chain_run(1, prev, _native.search_params(bandwidth=25, ignore_bottom=30, partial=0.5), first=2)
        ctx.band_fit_chain_collect(1, first=2)
        rec = ctx.download_records(3)
        assert [int(r["_pad"]) for r in rec[:2]] == [1, 2] and int(rec[2]["_pad"]) == 2, [int(r["_pad"]) for r in rec]
        descs, want = [], []
        for slot, (kind, kw, partial) in enumerate([(1, sp, 1), (2, dict(bandwidth=25), 1), (2, dict(bandwidth=25), 0.5)]):
            fit, fit4 = _points(size, rec[slot]["left_coeffs"], rec[slot]["right_coeffs"])
            band, band4 = _points(size, prev[:3], prev[3:], partial)
            descs.append((slot, kind, kw, fit, band if kind == 2 else None))
            want.append(_expected(ctx, slot, kind, kw, fit4, band4))
        got = _run(ctx, descs)
        for q in range(3):
            assert np.array_equal(got[q], want[q]), q
        assert (want[0][:, :, 0] != want[0][:, :, 1]).any() and (want[1][:, :, 1] == 76).any()     # windows and bands were drawn
        # the split-view panes of the same frames: the scaled bird's-eye image and the scaled picture side by side
        sw, sh, x2 = ctx.split_panes_size()
        assert (sw, sh, x2) == (640, 652, 640) == _native.split_panes_size(cal["img_size"], size)
        panes = _run(ctx, descs, panes=True)
        bev = ctx.download_bev(3)
        for q in range(3):
            assert np.array_equal(panes[q][:, :x2], utils.resize_linear(bev[q], (sw, sh))), q
            assert np.array_equal(panes[q][:, x2:], utils.resize_linear(want[q], (sw, sh))), q
        # more items than the staging ring holds: through it in pieces, same pictures
        many = _run(ctx, [descs[q % 3] for q in range(70)])
        for q in range(70):
            assert np.array_equal(many[q], want[q % 3]), q
    finally:
        ctx.close()


def test_odd_geometry_takes_the_per_pixel_path():
    """A bird's-eye width that is no multiple of 4 and an odd height; odd window width; masks that hold 1."""
    ref = calib.reference_calibration()
    S, T = np.diag([10.0, 10.0, 1.0]), np.diag([90 / 1080, 71 / 1100, 1.0])
    cal = dict(img_size=(128, 72), warped_size=(90, 71), cam_matrix=np.diag([0.1, 0.1, 1.0]) @ ref["cam_matrix"], dist_coeffs=ref["dist_coeffs"],
               warp_matrices=(T @ ref["warp_matrices"][0] @ S, None))
    size = cal["warped_size"]
    rng = np.random.default_rng(17)
    masks = (rng.random((3, 71, 90)) < 0.05).astype(np.uint8) * 255
    masks[:, :, 24:27] = 255                                       # two lanes in the noise
    masks[:, :, 60:63] = 255
    masks[2] //= 255                                               # values 0 / 1
    ctx = _ctx(cal, 3)
    try:
        ctx.upload_masks(masks)
        sp = dict(window_width=31, window_height=7, ignore_bottom=3)
        sws = _native.search_params(search_range=8, ignore_sides=10, **sp)
        ctx.sws_fit_run(1, sws, first=0)
        ctx.sws_fit_run(1, sws, first=2)
        prev = np.array([0.0, 0.0, 25.0, 0.0, 0.0, 60.0])
        ctx.band_fit_run(1, prev, _native.search_params(bandwidth=5, ignore_bottom=3, partial=1.0), first=1)
        rec = ctx.download_records(3)
        descs, want = [], []
        for slot, (kind, kw) in enumerate([(1, sp), (2, dict(bandwidth=5)), (1, sp)]):
            fit, fit4 = _points(size, rec[slot]["left_coeffs"], rec[slot]["right_coeffs"])
            band, band4 = _points(size, prev[:3], prev[3:], 1)
            descs.append((slot, kind, kw, fit, band if kind == 2 else None))
            want.append(_expected(ctx, slot, kind, kw, fit4, band4))
        got = _run(ctx, descs + [(2, 0, {}, None, None)])
        for q in range(3):
            assert got[q].shape == (71, 90, 3) and np.array_equal(got[q], want[q]), q
        assert np.array_equal(got[3], np.repeat(masks[2][:, :, None], 3, axis=2)) and got[3].max() == 1
        assert (want[0][:, :, 1] == 128).any() and (want[1][:, :, 1] == 76).any() and rec["detected"].all()
        assert ctx.split_panes_size() == _native.split_panes_size(cal["img_size"], size)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def any_ctx():
    ctx = _ctx(calib.reference_calibration(), 1)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("shape,dsize", [((110, 108, 3), (65, 64)), ((53, 37), (27, 19)), ((8, 8, 3), (8, 8)), ((5, 7), (9, 11)),
                                         ((1100, 1080, 3), (640, 652))])
def test_resize_linear_u8_equals_the_host_arithmetic(any_ctx, shape, dsize):
    img = np.random.default_rng(5).integers(0, 256, shape, dtype=np.uint8)
    got = any_ctx.resize_linear(img, dsize)
    want = utils.resize_linear(img, dsize)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_resize_linear_u8_reproduces_the_split_view_fixture(any_ctx):
    d = np.load(golden_files("viz_split")[0])
    sw, sh, x2 = _native.split_panes_size((128, 72), (108, 110))
    strip = np.zeros((sh, 128, 3), np.uint8)
    strip[:, :min(sw, 128)] = any_ctx.resize_linear(d["img1"], (sw, sh))[:, :128]
    strip[:, x2:x2 + sw] = any_ctx.resize_linear(d["img2"], (sw, sh))[:, :128 - x2]
    assert d["out"].shape == (72 + sh, 128, 3) and np.array_equal(strip, d["out"][72:])
    with pytest.raises(ValueError):
        any_ctx.resize_linear(np.zeros((4, 4, 2), np.uint8), (3, 3))
    with pytest.raises(ValueError):
        any_ctx.resize_linear(np.zeros((4, 4), np.uint8), (0, 3))
    assert any_ctx.resize_linear(np.full((4, 4), 7, np.uint8), (3, 3)).tolist() == [[7] * 3] * 3        # still usable


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
def _state(lt):
    b = lambda a: None if a is None else np.asarray(a).tobytes()
    return dict(detected=lt.detected_pixels, valid=lt.valid_lane_lines, last_detection=lt.last_detection, success=lt.success,
                counter=lt.counter, left_avg=b(lt.left_avg_coeffs), right_avg=b(lt.right_avg_coeffs), last_left=b(lt.last_left_coeffs),
                last_right=b(lt.last_right_coeffs), hist=[b(c) for c in lt.left_fit_coeffs] + [b(c) for c in lt.right_fit_coeffs],
                radii=list(lt.average_curve_radii), radius=lt.average_curve_radius, ecc=lt.eccentricity,
                pix=(b(lt.left_y), b(lt.left_x), b(lt.right_y), b(lt.right_x)), cent=(list(lt.left_window_centroids), list(lt.right_window_centroids)))


@pytest.fixture(scope="module")
def stream():
    a = synth.stream_lanes(3, seed=101)
    b = synth.stream_lanes(3, seed=202)
    noise, black = synth.frame_uniform(4001), np.zeros_like(a[0])
    mirrored, shifted = np.ascontiguousarray(a[1][:, ::-1]), np.roll(a[2], 200, axis=1)
    return np.stack([noise, a[0], a[1], mirrored, a[2], black, noise, a[1], shifted, a[0], black, black, black, black, black, noise,
                     b[0], b[1]], 0)


@pytest.fixture(scope="module")
def by_process(stream):
    """Tracker A, once: `process()` frame by frame -> per frame (annotated, picture, state), and the kind of every picture."""
    lt = LaneTracker(**calib.reference_calibration())
    try:
        out, kinds = [], []
        for f in stream:
            was_sws = lt.last_detection > lt.n_reset
            annotated, pic = lt.process(f, visualize_search=True)
            out.append((annotated.copy(), pic.copy(), _state(lt)))
            # (a band picture has a band: green 76 over black; the second try may have searched the other way round)
            kinds.append("mask" if pic.ndim == 2 else ("sws" if was_sws else "band") + ("" if lt.valid_lane_lines else " failed"))
    finally:
        lt.close()
    return out, kinds


@pytest.fixture(scope="module")
def split_by_process(stream):
    lt = LaneTracker(**calib.reference_calibration())
    try:
        return [lt.process(f, split_view=True).copy() for f in stream]
    finally:
        lt.close()


def test_the_stream_meets_every_kind(by_process):
    out, kinds = by_process
    assert {"mask", "sws", "band", "sws failed"} <= set(kinds), kinds
    assert kinds[1] == "sws" and kinds[0] == kinds[15] == "sws failed" and kinds[5] == "mask" and kinds[17] == "band", kinds


@pytest.mark.parametrize("windows", [(18,), (5, 13), (7, 4, 7)])
def test_process_batch_returns_what_process_returns(stream, by_process, windows):
    want, _ = by_process
    lt = LaneTracker(**calib.reference_calibration())
    try:
        lo = 0
        for w in windows:
            got = lt.process_batch(stream[lo:lo + w], visualize_search=True)
            assert len(got) == w
            for q, (annotated, pic) in enumerate(got):
                assert pic.ndim == want[lo + q][1].ndim and np.array_equal(pic, want[lo + q][1]), (windows, lo + q, "picture")
                assert np.array_equal(annotated, want[lo + q][0]), (windows, lo + q, "annotated")
            assert _state(lt) == want[lo + w - 1][2], (windows, lo)
            lo += w
    finally:
        lt.close()


def test_process_stream_returns_what_process_returns(stream, by_process):
    want, _ = by_process
    lt = LaneTracker(**calib.reference_calibration())
    try:
        for k, got in enumerate(lt.process_stream([stream[0:6], stream[6:12], stream[12:18]], visualize_search=True)):
            for q, (annotated, pic) in enumerate(got):
                assert pic.ndim == want[6 * k + q][1].ndim and np.array_equal(pic, want[6 * k + q][1]), (k, q, "picture")
                assert np.array_equal(annotated, want[6 * k + q][0]), (k, q, "annotated")
            assert _state(lt) == want[6 * k + 5][2], k
    finally:
        lt.close()


def test_split_view_of_windows_equals_process(stream, split_by_process):
    lt = LaneTracker(**calib.reference_calibration())
    try:
        lo = 0
        for w in (7, 4, 7):
            got = lt.process_batch(stream[lo:lo + w], split_view=True)
            for q, view in enumerate(got):
                assert view.shape == split_by_process[lo + q].shape == (720 + 652, 1280, 3)
                assert np.array_equal(view, split_by_process[lo + q]), lo + q
            lo += w
    finally:
        lt.close()


def test_device_frames_window_equals_process(stream, by_process, split_by_process):
    want, _ = by_process
    lt = LaneTracker(**calib.reference_calibration())
    try:
        got = lt.process_batch(DeviceFrames.from_host(stream, "rgb"), visualize_search=True)
        for q, (annotated, pic) in enumerate(got):
            assert pic.ndim == want[q][1].ndim and np.array_equal(pic, want[q][1]) and np.array_equal(annotated, want[q][0]), q
        assert _state(lt) == want[17][2]
    finally:
        lt.close()
    lt = LaneTracker(**calib.reference_calibration())
    try:
        for q, view in enumerate(lt.process_batch(DeviceFrames.from_host(stream, "rgb"), split_view=True)):
            assert np.array_equal(view, split_by_process[q]), q
    finally:
        lt.close()


def test_unannotated_windows_carry_the_pictures_alone(stream, by_process):
    want, _ = by_process
    lt = LaneTracker(**calib.reference_calibration())
    try:
        for q, (none, pic) in enumerate(lt.process_batch(stream, annotate=False, visualize_search=True)):
            assert none is None and pic.ndim == want[q][1].ndim and np.array_equal(pic, want[q][1]), q
        assert _state(lt) == want[17][2]
    finally:
        lt.close()


# ---- refusals, memory ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    cal = calib.reference_calibration()
    ctx = _ctx(cal, 2)
    lib, h = ctx.lib, ctx._h
    H, W = ctx.warp_h, ctx.warp_w
    out = np.zeros((2, H, W, 3), np.uint8)
    pts = np.zeros((4, 2), np.int32)

    def call(n, items, lists=(pts, pts, pts, pts), fn=None, dst=out):
        items = np.ascontiguousarray(items, _native.VIZ_ITEM_DTYPE)
        return (fn or lib.lt_search_viz_run)(h, n, items.ctypes.data if len(items) else None, *[None if a is None else a.ctypes.data for a in lists],
                                             None if dst is None else dst.ctypes.data)

    def item(**kw):
        it = np.zeros(1, _native.VIZ_ITEM_DTYPE)
        for k, v in kw.items():
            it[0][k] = v
        return it
    try:
        assert call(1, item()) == -5                                       # LT_ERR_STATE: no mask in the slots
        ctx.upload_masks(np.zeros((2, H, W), np.uint8))
        assert call(1, item(kind=1, window_height=40)) == -5               # ... no search has run
        assert call(1, item(kind=2)) == -5
        ctx.band_fit_run(1, np.array([0, 0, 400.0, 0, 0, 600.0]), _native.search_params(bandwidth=25))
        ctx.sws_fit_run(1)
        assert call(-1, item()) == -1                                      # LT_ERR_INVALID from here on
        assert call(1, np.zeros(0, _native.VIZ_ITEM_DTYPE)) == -1
        assert call(1, item(), dst=None) == -1
        assert call(1, item(slot=2)) == -1 and call(1, item(slot=-1)) == -1
        assert call(1, item(kind=3)) == -1 and call(1, item(kind=-1)) == -1
        assert call(1, item(kind=1, window_height=40, n_fit_left=-1)) == -1
        assert call(1, item(kind=2, n_band_right=-2)) == -1
        assert call(1, item(kind=1, window_height=0)) == -1
        assert call(1, item(kind=1, window_height=40, n_fit_left=2), lists=(None, pts, pts, pts)) == -1
        assert call(1, item(kind=2, n_band_left=2), lists=(pts, pts, None, pts)) == -1
        assert call(1, item(kind=3), fn=lib.lt_split_panes_run) == -1
        assert lib.lt_split_panes_size(None, None, None, None) == -1 and lib.lt_search_viz_wait(None) == -1
        assert call(0, np.zeros(0, _native.VIZ_ITEM_DTYPE)) == 0
        out[:] = 7
        assert call(2, np.concatenate([item(slot=1), item(slot=0, kind=1, window_width=30, window_height=40, ignore_bottom=30)]),
                    lists=(None, None, None, None)) == 0
        ctx.search_viz_wait()
        assert not out[0].any() and np.array_equal(out[1][:, :, 0], out[1][:, :, 2])       # black masks; green windows at most
    finally:
        ctx.close()


def test_value_errors_of_the_pipeline(stream):
    lt = LaneTracker(**calib.reference_calibration())
    try:
        with pytest.raises(ValueError):
            lt.process_batch(stream[:2], annotate=False, split_view=True)
        with pytest.raises(ValueError):
            lt.process_batch(stream[:2].copy(), annotate="inplace", split_view=True)
        with pytest.raises(ValueError):
            next(lt.process_stream([stream[:2]], annotate=False, split_view=True))
        assert lt.counter == 0
    finally:
        lt.close()


def test_live_device_memory_stays_flat(stream):
    lt = LaneTracker(**calib.reference_calibration())
    try:
        lt.warm(6, visualize_search=True)
        lt.process_batch(stream[:6], visualize_search=True)
        before = _native.device_cache_stats()["live_bytes"]
        for _ in range(10):
            lt.process_batch(stream[:6], visualize_search=True)
        assert _native.device_cache_stats()["live_bytes"] == before
    finally:
        lt.close()
