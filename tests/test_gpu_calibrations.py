"""Calibration sets of a context (lt_add_calibration, lt_set_slot_calibrations): one context whose slots hold cameras of different
calibrations against one-set contexts created with each calibration alone -- bit for bit, slot by slot -- against the oracle, and
what is refused."""
import ctypes as C
import functools

import numpy as np
import pytest

import calibration_cameras as CC
from helpers import coeff_close
from lane_tracker_amd import _native, synth
from lane_tracker_amd.device import DeviceFrames

pytestmark = pytest.mark.gpu

CAPACITY = 8
PATTERN = [0, 1, 1, 2, 4, 3, 0]           # by slot: two sets in the pairs (0, 1), (2, 3), (4, 5); 2 | 4 across the slice boundary 3 | 4
LT_ERR_INVALID, LT_ERR_STATE = -1, -5


@functools.lru_cache(maxsize=None)
def _scenes():
    r = synth.SceneRenderer()
    return np.stack([r.render(s)[0] for s in range(CAPACITY)])


def _outputs(ctx, n, first, search=None):
    """Everything the front end, the mask chain and the search left in slots [first, first + n)."""
    ctx.mask_run(n, first=first)
    ctx.sws_fit_run(n, search, first=first)
    return _collect(ctx, n, first)


def _collect(ctx, n, first):
    i = ctx.info()
    return dict(planes=[ctx.download_plane(p, n, first=first) for p in range(6)], mask=ctx.download_masks(n, first=first),
                rec=ctx.download_records(n, first=first), und=ctx.download_undistorted(n, first=first), rows=(i.src_row0, i.src_row1))


def _assert_slots_equal(got, solo_of, ids, what):
    """Slot j of `got` (the mixed context) against slot j of the solo context of set ids[j]."""
    for j, s in enumerate(ids):
        want = solo_of(s)
        for p in range(6):
            assert np.array_equal(got["planes"][p][j], want["planes"][p][j]), (what, "plane", p, "slot", j, "set", s)
        assert np.array_equal(got["mask"][j], want["mask"][j]), (what, "mask", j, s)
        assert got["rec"][j].tobytes() == want["rec"][j].tobytes(), (what, "record", j, s)
        (u0, u1), (s0, s1) = got["rows"], want["rows"]
        assert u0 <= s0 and s1 <= u1, (what, got["rows"], want["rows"])
        assert np.array_equal(got["und"][j][s0 - u0:s1 - u0], want["und"][j]), (what, "undistorted rows", j, s)


@pytest.fixture(scope="module")
def contexts():
    """One context with the sets A-E and five one-set contexts, each over two slot streams."""
    cams = CC.cameras()
    made = []
    try:
        mixed = CC.native_context(cams["A"], CAPACITY)
        made.append(mixed)
        for name in "BCDE":
            c = cams[name]
            assert mixed.add_calibration(c["cam_matrix"], c["dist_coeffs"], c["warp_matrices"][0]) == "ABCDE".index(name)
        solos = []
        for name in "ABCDE":
            solos.append(CC.native_context(cams[name], CAPACITY))
            made.append(solos[-1])
        for c in made:
            c.set_streams(2)
        assert mixed.calibration_count() == 5 and all(s.calibration_count() == 1 for s in solos)
        yield mixed, solos
    finally:
        for c in made:
            c.close()


def test_the_rows_of_a_context_are_the_union_over_its_sets(contexts):
    mixed, solos = contexts
    rows = [(s.info().src_row0, s.info().src_row1) for s in solos]
    assert rows[0] == (457, 695) and rows[1] == (447, 685)
    i = mixed.info()
    assert (i.src_row0, i.src_row1) == (min(r[0] for r in rows), max(r[1] for r in rows)) == (447, 695)
    src = [s.source_rows() for s in solos]
    assert mixed.source_rows() == (min(r[0] for r in src), max(r[1] for r in src))


@pytest.mark.parametrize("n,first", [(1, 0), (1, 1), (2, 0), (2, 3), (3, 1), (7, 0), (7, 1)])
def test_mixed_ranges_equal_solo_contexts_bit_for_bit(contexts, n, first):
    mixed, solos = contexts
    frames = _scenes()[first:first + n]
    cache = {}

    def solo_of(s):
        if s not in cache:
            solos[s].upload_frames(frames, first=first)
            cache[s] = _outputs(solos[s], n, first)
        return cache[s]

    ids = [PATTERN[(first + j) % 7] for j in range(n)]
    mixed.upload_frames(frames, first=first)
    mixed.set_slot_calibrations(ids, first=first)
    assert list(mixed.slot_calibrations(n, first=first)) == ids
    _assert_slots_equal(_outputs(mixed, n, first), solo_of, ids, ("first", n, first))
    # the sets reassigned twice over the same slots, the second time with the first run still queued: nothing waits in between
    ids2 = [PATTERN[(first + j + 3) % 7] for j in range(n)]
    ids3 = [PATTERN[(first + j + 5) % 7] for j in range(n)]
    mixed.set_slot_calibrations(ids2, first=first)
    mixed.mask_run(n, first=first)
    mixed.sws_fit_run(n, first=first)
    mixed.set_slot_calibrations(ids3, first=first)
    _assert_slots_equal(_outputs(mixed, n, first), solo_of, ids3, ("reassigned", n, first))
    # a re-run over slots whose set changed must not reuse planes made with the other set
    mixed.set_slot_calibrations(ids, first=first)
    mixed.mask_run(n, first=first, reuse_front=True)
    mixed.sws_fit_run(n, first=first)
    _assert_slots_equal(_collect(mixed, n, first), solo_of, ids, ("rerun", n, first))
    mixed.set_slot_calibrations([0] * n, first=first)


def test_a_range_of_one_other_set_takes_that_sets_tables(contexts):
    mixed, solos = contexts
    n, first = 3, 1
    frames = _scenes()[first:first + n]
    solos[3].upload_frames(frames, first=first)
    want = _outputs(solos[3], n, first)
    mixed.upload_frames(frames, first=first)
    mixed.set_slot_calibrations([3] * n, first=first)
    try:
        _assert_slots_equal(_outputs(mixed, n, first), lambda s: want, [3] * n, "all of set 3")
    finally:
        mixed.set_slot_calibrations([0] * n, first=first)


def test_masks_and_fits_of_other_cameras_equal_the_oracle(contexts, oracle):
    mixed, _ = contexts
    cams = CC.cameras()
    names = "BBCCDDEE"
    scenes = _scenes()
    frames = np.stack([CC.frames_for(nm, scenes[j % 2]) for j, nm in enumerate(names)])
    mixed.upload_frames(frames)
    mixed.set_slot_calibrations(["ABCDE".index(nm) for nm in names])
    try:
        mixed.mask_run(8)
        mixed.sws_fit_run(8)
        masks, rec = mixed.download_masks(8), mixed.download_records(8)
    finally:
        mixed.set_slot_calibrations([0] * 8)
    for j, nm in enumerate(names):
        oc = CC.oracle_calib(oracle, cams[nm])
        assert np.array_equal(masks[j], oracle.mask_from_frame(oc, frames[j])), (j, nm)
        want = oracle.frame_sws_fit(oc, frames[j])
        assert bool(rec[j]["detected"]) == want["detected"] and want["detected"], (j, nm)
        assert (int(rec[j]["n_left"]), int(rec[j]["n_right"])) == (want["n_left"], want["n_right"]), (j, nm)
        assert coeff_close(rec[j]["left_coeffs"], want["coeffs"][0]) and coeff_close(rec[j]["right_coeffs"], want["coeffs"][1]), (j, nm)


# ---- small geometries ------------------------------------------------------------------------------------------------------------
W, H = 64, 48
SMALL = [dict(cam_matrix=np.eye(3), dist_coeffs=np.zeros(5), M=np.eye(3)),                                   # the identity: every row and column
         dict(cam_matrix=np.array([[40.0, 0, 31.5], [0, 40.0, 23.5], [0, 0, 1]]), dist_coeffs=np.array([0.3, 0.0, 0.01, 0.0, 0.0]),
              M=np.array([[1.0, 0, -9.5], [0, 1.0, 6.25], [0, 0, 1]])),                                    # taps outside the image, both remaps
         dict(cam_matrix=np.eye(3), dist_coeffs=np.zeros(5), M=np.array([[1.0, 0, 0], [0, 2.0, -30.5], [0, 0, 1]]))]   # rows 15 .. 39 only


def _small_ctx(sets, layout, capacity=4):
    c = _native.Context((W, H), (W, H), sets[0]["cam_matrix"], sets[0]["dist_coeffs"], sets[0]["M"], capacity=capacity)
    try:
        if layout != "rgb":
            c.set_input_format(layout, "bt601")
        for s in sets[1:]:
            c.add_calibration(s["cam_matrix"], s["dist_coeffs"], s["M"])
    except BaseException:
        c.close()
        raise
    return c


def _feed(ctx, frames, first, layout, surfaces):
    """The frames into slots first, ...: uploaded, or attached where they lie in device memory (returned: keep alive)."""
    if not surfaces:
        ctx.upload_frames(frames, first=first)
        return None
    if layout == "rgb":
        df = DeviceFrames.from_host(frames, layout, pitch=W * 3 + 20, offset=1)
    else:
        df = DeviceFrames.from_host(frames, layout, pitch=W + 6, chroma_pitch=(W if layout == "nv12" else W // 2) + 5, offset=3)
    return ctx.attach_device_frames(df, first=first)


@pytest.mark.parametrize("surfaces", [False, True])
@pytest.mark.parametrize("layout", ["rgb", "nv12", "i420"])
def test_small_cameras_with_border_taps_and_a_narrow_set(layout, surfaces):
    rng = np.random.default_rng(7)
    shape = (4, H, W, 3) if layout == "rgb" else (4, H * 3 // 2, W)
    frames = rng.integers(0, 256, shape, dtype=np.uint8)
    mixed = _small_ctx(SMALL, layout)
    solos = [_small_ctx([s], layout) for s in SMALL]
    try:
        assert (mixed.info().src_row0, mixed.info().src_row1) == (0, H)
        r2 = (solos[2].info().src_row0, solos[2].info().src_row1)
        assert 0 < r2[0] and r2[1] < H, r2                                  # narrower than the union
        for n, first, ids in ((4, 0, [1, 0, 2, 1]), (3, 1, [2, 1, 0]), (2, 2, [2, 2])):
            cache = {}

            def solo_of(s):
                if s not in cache:
                    keep = _feed(solos[s], frames[:n], first, layout, surfaces)
                    cache[s] = _outputs(solos[s], n, first)
                    del keep
                return cache[s]
            keep = _feed(mixed, frames[:n], first, layout, surfaces)
            mixed.set_slot_calibrations(ids, first=first)
            _assert_slots_equal(_outputs(mixed, n, first), solo_of, ids, (layout, surfaces, n, first))
            del keep
    finally:
        mixed.close()
        for s in solos:
            s.close()


def test_odd_sizes_with_two_sets_in_one_pair():
    """Camera 641 x 361, bird's-eye 541 x 551: the one-pixel form of the warp, frames at a stride that is no multiple of 4."""
    from lane_tracker_amd import calib
    S = np.diag([0.5, 0.5, 1.0])
    K = S @ calib.CAM_MATRIX
    M = S @ calib.M @ np.diag([2.0, 2.0, 1.0])
    T = np.array([[1.0, 0, 6.0], [0, 1.0, -4.0], [0, 0, 1]])
    sets = [dict(cam_matrix=K, dist_coeffs=calib.DIST_COEFFS, M=M), dict(cam_matrix=T @ K, dist_coeffs=calib.DIST_COEFFS * 0.5, M=M @ np.linalg.inv(T))]
    size, warped = (641, 361), (541, 551)
    mk = lambda ss: _native.Context(size, warped, ss[0]["cam_matrix"], ss[0]["dist_coeffs"], ss[0]["M"], capacity=3)
    mixed, solos = mk(sets), [mk([s]) for s in sets]
    try:
        mixed.add_calibration(sets[1]["cam_matrix"], sets[1]["dist_coeffs"], sets[1]["M"])
        frames = np.random.default_rng(12).integers(0, 256, (3, 361, 641, 3), dtype=np.uint8)
        sp = _native.search_params(window_width=14, window_height=20, search_range=10, ignore_sides=180, ignore_bottom=15)
        want = []
        for s in solos:
            s.upload_frames(frames)
            want.append(_outputs(s, 3, 0, sp))
        mixed.upload_frames(frames)
        for ids in ([0, 1, 1], [1, 0, 0]):
            mixed.set_slot_calibrations(ids)
            _assert_slots_equal(_outputs(mixed, 3, 0, sp), lambda s: want[s], ids, ids)
    finally:
        mixed.close()
        for s in solos:
            s.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_sets_of_another_size_late_sets_and_unknown_ids_are_refused():
    cams = CC.cameras()
    c = CC.native_context(cams["A"], 2)
    try:
        b = cams["B"]
        i = C.c_int(-7)
        for size, warped in (((1280, 704), b["warped_size"]), (b["img_size"], (1080, 1096))):
            bad = _native.make_calib(size, warped, b["cam_matrix"], b["dist_coeffs"], b["warp_matrices"][0])
            assert c.lib.lt_add_calibration(c._h, C.byref(bad), C.byref(i)) == LT_ERR_INVALID and i.value == -7
        assert c.calibration_count() == 1
        assert c.add_calibration(b["cam_matrix"], b["dist_coeffs"], b["warp_matrices"][0]) == 1
        for ids in ([2], [-1], [0, 2]):
            with pytest.raises(ValueError):
                c.set_slot_calibrations(ids)
        assert list(c.slot_calibrations()) == [0, 0]                        # a refused list changes nothing
        with pytest.raises(_native.NativeError):
            c.set_slot_calibrations([0, 1, 0])                              # past the capacity
        c.upload_frames(_scenes()[:1])
        good = _native.make_calib(b["img_size"], b["warped_size"], b["cam_matrix"], b["dist_coeffs"], b["warp_matrices"][0])
        assert c.lib.lt_add_calibration(c._h, C.byref(good), C.byref(i)) == LT_ERR_STATE
        assert c.calibration_count() == 2
        c.set_slot_calibrations([1, 0])
        c.upload_frames(_scenes()[:2])
        c.mask_run(2)                                                       # the context is usable
        assert c.download_masks(2).any()
    finally:
        c.close()


def test_entry_points_that_know_set_zero_only_refuse_other_sets():
    cams = CC.cameras()
    c = CC.native_context(cams["A"], 2)
    try:
        b = cams["B"]
        assert c.add_calibration(b["cam_matrix"], b["dist_coeffs"], b["warp_matrices"][0]) == 1
        c.overlay_configure(cams["A"]["warp_matrices"][1])
        c.overlay_configure(b["warp_matrices"][1], calibration=1)
        frames = _scenes()[:2]
        c.upload_frames(frames)
        c.set_slot_calibrations([0, 1])
        c.mask_run(2)
        c.sws_fit_run(2)
        lib, h = c.lib, c._h
        zero, out = np.zeros(1, np.int32), _native.pinned_empty((1,) + frames.shape[1:])
        rows = np.array([0, 0, 400, 700], np.int32)
        ploty = np.linspace(0, c.warp_h - 1, c.warp_h)
        ploty2, six, draw = ploty ** 2, np.zeros(6), np.ones(1, np.uint8)
        item = np.zeros(1, _native.VIZ_ITEM_DTYPE)
        item["slot"] = 1
        pics = np.empty((1, c.warp_h, c.warp_w, 3), np.uint8)
        calls = {
            "lt_present_frame": lambda s: lib.lt_present_frame(h, s, zero.ctypes.data, zero.ctypes.data, None, None, 0.3, None, 0, 0, 20, 8, 35, out.ctypes.data, None),
            "lt_present_lane_async": lambda s: lib.lt_present_lane_async(h, s, zero.ctypes.data, zero.ctypes.data, None, None, 0.3, out.ctypes.data, rows.ctypes.data),
            "lt_present_lane_from_fit_async": lambda s: lib.lt_present_lane_from_fit_async(h, s, six.ctypes.data, 1, ploty.ctypes.data, ploty2.ctypes.data, len(ploty), 0.3,
                                                                                          out.ctypes.data, rows.ctypes.data),
            "lt_present_finish": lambda s: lib.lt_present_finish(h, s, None, 0, 0, 20, 8, 35, out.ctypes.data, rows.ctypes.data),
            "lt_lane_spans_from_fit": lambda s: lib.lt_lane_spans_from_fit(h, six.ctypes.data, 1, 0, six.ctypes.data, 1, ploty.ctypes.data, ploty2.ctypes.data, len(ploty),
                                                                          np.empty((c.warp_h, 2), np.int16).ctypes.data),
            "lt_overlay_run_strip": lambda s: lib.lt_overlay_run_strip(h, s, 1, zero.ctypes.data, zero.ctypes.data, None, None, 0.3),
            "lt_overlay_run_strip_coeffs": lambda s: lib.lt_overlay_run_strip_coeffs(h, s, 1, six.ctypes.data, draw.ctypes.data, ploty.ctypes.data, ploty2.ctypes.data,
                                                                                    len(ploty), 0.3),
            "lt_search_viz_run": lambda s: lib.lt_search_viz_run(h, 1, item.ctypes.data, None, None, None, None, pics.ctypes.data),
            "lt_split_panes_run": lambda s: lib.lt_split_panes_run(h, 1, item.ctypes.data, None, None, None, None, pics.ctypes.data),
        }
        for name, call in calls.items():
            assert call(1) == LT_ERR_STATE, name
            assert b"calibration set 1" in lib.lt_last_error(), (name, lib.lt_last_error())
        # ... and the context is as it was: both slots drawn with their own tables, the masks still there
        masks = c.download_masks(2)
        poly = (np.arange(600, 1000), np.full(400, 400), np.arange(600, 1000), np.full(400, 700))
        c.overlay_run([poly, poly])
        both = c.download_overlay(2).copy()
        assert np.array_equal(c.download_masks(2), masks)
        solo = CC.native_context(b, 1)
        try:
            solo.overlay_configure(b["warp_matrices"][1])
            solo.upload_frames(frames[1:2])
            solo.overlay_run([poly])
            assert np.array_equal(both[1], solo.download_overlay(1)[0])
        finally:
            solo.close()
        assert not np.array_equal(both[0], frames[0]) and not np.array_equal(both[1], frames[1])      # a lane was drawn
        c.set_slot_calibrations([0, 0])
        assert lib.lt_lane_spans_from_fit(h, six.ctypes.data, 1, 0, six.ctypes.data, 1, ploty.ctypes.data, ploty2.ctypes.data, len(ploty),
                                          np.empty((c.warp_h, 2), np.int16).ctypes.data) == 0
    finally:
        c.close()
