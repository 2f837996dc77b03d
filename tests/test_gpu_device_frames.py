"""Camera frames that are already in device memory (lt_attach_device_frames, device.DeviceFrames).  Everything here is bit for
bit: a context or tracker that reads its frames where they lie on the device must give exactly what a second one gives that is
fed the same bytes from the host.  There is no tolerance anywhere."""
import functools
import itertools

import numpy as np
import pytest

import yuv_reference as R
from lane_tracker_amd import _native, calib, synth
from lane_tracker_amd.device import DeviceBuffer, DeviceFrames, pack_host_frames
from lane_tracker_amd.lane_tracker import LaneTracker

pytestmark = pytest.mark.gpu

LAYOUTS = ("rgb", "nv12", "i420")
W, H = calib.IMAGE_WIDTH_HEIGHT
CASES = ((1, 0), (1, 1), (2, 0), (2, 3), (3, 0), (3, 1), (16, 0), (16, 5), (64, 0), (64, 1))


def _ctx(cal, capacity, pixel_format="rgb", matrix="bt601"):
    c = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0],
                        capacity=capacity)
    if pixel_format != "rgb":
        c.set_input_format(pixel_format, matrix)
    return c


@functools.lru_cache(maxsize=None)
def _rgb_scenes():
    r = synth.SceneRenderer()
    return np.stack([r.render(s)[0] for s in range(58)])


@functools.lru_cache(maxsize=None)
def _mix(layout):
    """The 64-frame mix of tests/test_gpu_yuv.py: 10 scenes, 6 frames of uniform noise, 48 scenes -- in `layout`."""
    rgb = _rgb_scenes()
    if layout == "rgb":
        noise = np.random.default_rng(11).integers(0, 256, (6, H, W, 3), dtype=np.uint8)
        return np.concatenate([rgb[:10], noise, rgb[10:]])
    yuv = np.stack([R.rgb_to_yuv420(f, layout) for f in rgb])
    noise = np.random.default_rng(11).integers(0, 256, (6, H * 3 // 2, W), dtype=np.uint8)
    return np.concatenate([yuv[:10], noise, yuv[10:]])


def _valid_lanes(records):
    """How many of the records show both lines detected and a lane check_validity accepts."""
    cal = calib.reference_calibration()
    t = LaneTracker(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"], cal["mpp_conversion"])
    try:
        ok = 0
        for r in records:
            if r["detected"] and not r["fit_flags"]:
                t.check_validity(r["left_coeffs"], r["right_coeffs"])
                ok += bool(t.valid_lane_lines)
        return ok
    finally:
        t.close()


def _join(parts, like):
    return DeviceFrames(np.concatenate([p.surfaces for p in parts]), like.img_size, like.pixel_format, owner=parts)


def _plane_block(planes, pitch):
    """planes (n, rows, row bytes) at `pitch` in a DeviceBuffer of their own that ends with the last row -> (buffer, plane addresses)."""
    n, rows, rb = planes.shape
    host = np.full((n * rows, pitch), 0xC3, np.uint8)
    host[:, :rb] = planes.reshape(n * rows, rb)
    buf = DeviceBuffer(n * rows * pitch - (pitch - rb)).copy_from_host(host.reshape(-1)[:n * rows * pitch - (pitch - rb)])
    return buf, [buf.ptr + k * rows * pitch for k in range(n)]


def _surfaces(frames, layout, variant):
    """`frames` on the device as the variant says -> DeviceFrames (which owns its buffers)."""
    kind, arg = variant
    if kind == "dense":
        return DeviceFrames.from_host(frames, layout)
    if kind == "pitched":                                   # (pitch, chroma pitch, base offset)
        return DeviceFrames.from_host(frames, layout, pitch=arg[0], chroma_pitch=arg[1], offset=arg[2])
    if kind == "uv_elsewhere":                              # NV12: the Y planes in one allocation, the UV planes in another
        ys, yp = _plane_block(frames[:, :H], W + 32)
        uv, up = _plane_block(frames[:, H:], W + 2)
        return DeviceFrames.from_planes(list(zip(yp, up)), (W, H), "nv12", pitch=W + 32, chroma_pitch=W + 2, owner=(ys, uv))
    if kind == "scattered":                                 # three allocations, made in reverse order of the frames they hold
        idx = [a for a in np.array_split(np.arange(len(frames)), 3) if len(a)]
        parts = [DeviceFrames.from_host(frames[a], layout) for a in reversed(idx)][::-1]
        return _join(parts, parts[0])
    raise AssertionError(variant)


def _variants(layout):
    if layout == "rgb":
        p = W * 3 + 20
        return [("dense", None), ("pitched", (p, None, 0))] + [("pitched", (p, None, k)) for k in (1, 2, 3)] + [("scattered", None)]
    if layout == "nv12":
        return [("dense", None), ("pitched", (W + 64, None, 0)), ("pitched", (W + 6, None, 0))] + \
               [("pitched", (W + 6, W + 10, k)) for k in (1, 2, 3)] + [("uv_elsewhere", None), ("scattered", None)]
    return [("dense", None), ("pitched", (W + 64, W // 2 + 40, 0)), ("pitched", (W + 6, W // 2 + 5, 0))] + \
           [("pitched", (W + 6, W // 2 + 5, k)) for k in (1, 2, 3)] + [("scattered", None)]


def _run(c, n, first):
    c.mask_run(n, first=first)
    c.sws_fit_run(n, first=first)


def _results(c, n, first):
    return dict(und=c.download_undistorted(n, first=first), planes=[c.download_plane(p, n, first=first) for p in range(6)],
                masks=c.download_masks(n, first=first), rec=c.download_records(n, first=first).tobytes())


def _assert_same(got, want, what, planes=range(6)):
    assert np.array_equal(got["und"], want["und"]), (what, "undistorted rows")
    for p in planes:
        assert np.array_equal(got["planes"][p], want["planes"][p]), (what, "plane", p)
    assert np.array_equal(got["masks"], want["masks"]), (what, "masks")
    assert got["rec"] == want["rec"], (what, "records")


# ---- 1. the mask chain over attached surfaces = over the same bytes uploaded from the host ----------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_mask_chain_parity_at_the_abi(layout):
    cal = calib.reference_calibration()
    frames = _mix(layout)
    a, b = _ctx(cal, 66, layout), _ctx(cal, 66, layout)
    try:
        # the scenes must be ones a tracker FINDS lanes in: asked of the host-fed context before anything is compared
        a.upload_frame_rows(frames[:10])
        _run(a, 10, 0)
        assert _valid_lanes(a.download_records(10)) >= 9
        for n, first in CASES:
            rot = (n + first) % 7                           # other frames in the slots every time
            f = np.ascontiguousarray(np.roll(frames, rot, 0)[:n])
            a.upload_frame_rows(f, first=first)
            _run(a, n, first)
            want = _results(a, n, first)
            for variant in _variants(layout):
                df = _surfaces(f, layout, variant)
                assert len(df) == n
                keep = b.attach_device_frames(df, first=first)
                _run(b, n, first)
                _assert_same(_results(b, n, first), want, (layout, n, first, variant))
                del keep, df
    finally:
        a.close()
        b.close()


# ---- 2. only the surfaces' bytes count --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,pitch,cpitch,offset", [("rgb", W * 3 + 20, None, 1), ("nv12", W + 6, W + 10, 3), ("i420", W + 6, W // 2 + 5, 2)])
def test_bytes_around_and_between_the_rows_do_not_count(layout, pitch, cpitch, offset):
    cal = calib.reference_calibration()
    n, first = 5, 1
    f = np.ascontiguousarray(_mix(layout)[7:7 + n])           # scenes and noise
    a, b = _ctx(cal, 8, layout), _ctx(cal, 8, layout)
    try:
        a.upload_frame_rows(f, first=first)
        _run(a, n, first)
        want = _results(a, n, first)
        for poison in (0x00, 0xFF, 0x5A):
            block, surf, size, _ = pack_host_frames(f, layout, pitch, cpitch, offset, fill=poison)
            with DeviceBuffer(block.nbytes) as buf:
                buf.copy_from_host(block)
                nplanes = {"rgb": 1, "nv12": 2, "i420": 3}[layout]
                surf["plane"][:, :nplanes] += np.uint64(buf.ptr)
                df = DeviceFrames(surf, size, layout, owner=buf)
                assert np.array_equal(df.to_host(), f)
                b.attach_device_frames(df, first=first)
                _run(b, n, first)
                _assert_same(_results(b, n, first), want, (layout, hex(poison)))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_surface_may_end_on_the_last_byte_of_its_allocation(layout):
    """A small camera whose bird's-eye view reads EVERY row and column of the frame (identity maps), so that the windows of the
    last pixels of the last row overrun the plane: the last plane ends on the last byte of its DeviceBuffer, at every alignment.
    The overrun comes back as zeros from the buffer resource's range check and is never used: the results are the host-fed ones."""
    w, h = 64, 48
    rng = np.random.default_rng(5)
    shape = (3, h, w, 3) if layout == "rgb" else (3, h * 3 // 2, w)
    f = rng.integers(0, 256, shape, dtype=np.uint8)
    mk = lambda: _native.Context((w, h), (w, h), np.eye(3), np.zeros(5), np.eye(3), capacity=4)
    a, b = mk(), mk()
    try:
        for c in (a, b):
            if layout != "rgb":
                c.set_input_format(layout, "bt601")
            assert c.source_rows() == (0, h)
        a.upload_frame_rows(f, first=1)
        a.mask_run(3, first=1)
        want = [a.download_undistorted(3, first=1), a.download_plane(0, 3, first=1), a.download_plane(1, 3, first=1)]
        row = w * 3 if layout == "rgb" else w
        crow = {"rgb": None, "nv12": w, "i420": w // 2}[layout]
        for extra in (0, 1, 6):
            for offset in (0, 1, 2, 3):
                block, surf, size, _ = pack_host_frames(f, layout, row + extra, None if crow is None else crow + extra, offset, fill=0xEE)
                with DeviceBuffer(block.nbytes) as buf:
                    buf.copy_from_host(block)
                    nplanes = {"rgb": 1, "nv12": 2, "i420": 3}[layout]
                    surf["plane"][:, :nplanes] += np.uint64(buf.ptr)
                    last_rows, last_row = (h, row) if layout == "rgb" else (h // 2, crow)
                    last_pitch = int(surf[-1]["pitch" if layout == "rgb" else "chroma_pitch"])
                    assert int(surf["plane"][-1, nplanes - 1]) + last_pitch * (last_rows - 1) + last_row == buf.ptr + buf.nbytes
                    b.attach_device_frames(DeviceFrames(surf, size, layout, owner=buf), first=1)
                    b.mask_run(3, first=1)
                    got = [b.download_undistorted(3, first=1), b.download_plane(0, 3, first=1), b.download_plane(1, 3, first=1)]
                    for g, x in zip(got, want):
                        assert np.array_equal(g, x), (layout, extra, offset)
                    assert np.array_equal(got[0], f if layout == "rgb" else np.stack([R.yuv420_to_rgb(q, layout) for q in f]))   # identity maps
    finally:
        a.close()
        b.close()


# ---- 3. refusals, before any launch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["rgb", "nv12"])
def test_wrong_surfaces_are_refused_and_the_context_stays_usable(layout):
    cal = calib.reference_calibration()
    f = np.ascontiguousarray(_mix(layout)[:2])
    a, b = _ctx(cal, 2, layout), _ctx(cal, 2, layout)
    try:
        a.upload_frame_rows(f)
        _run(a, 2, 0)
        want = _results(a, 2, 0)
        good = DeviceFrames.from_host(f, layout)
        b.attach_device_frames(good)
        _run(b, 2, 0)
        _assert_same(_results(b, 2, 0), want, "before")
        lib, last = b.lib, (1 if layout == "nv12" else 0)

        def refused(change, message):
            s = good.surfaces.copy()
            change(s)
            assert lib.lt_attach_device_frames(b._h, s.ctypes.data, 0, 2) == -1, message                 # LT_ERR_INVALID
            assert message in lib.lt_last_error().decode(), (message, lib.lt_last_error())
        host = np.zeros(f[0].nbytes + 64, np.uint8)

        def host_pointer(s): s["plane"][1, 0] = host.ctypes.data
        def null_pointer(s): s["plane"][0, last] = 0
        def one_byte_past(s): s["plane"][1, last] += 1      # the last plane of the last frame ends on the allocation's last byte
        def narrow_pitch(s): s["pitch"][1] = (W * 3 if layout == "rgb" else W) - 1
        refused(host_pointer, "not device memory")
        refused(null_pointer, "null pointer")
        refused(one_byte_past, "runs past the end of its allocation")
        refused(narrow_pitch, "is below the row's")
        if layout == "nv12":
            def narrow_chroma(s): s["chroma_pitch"][0] = W - 2
            refused(narrow_chroma, "chroma pitch")
        assert lib.lt_attach_device_frames(b._h, None, 0, 2) == -1
        assert lib.lt_attach_device_frames(b._h, good.surfaces.ctypes.data, 1, 2) == -4                  # LT_ERR_CAPACITY
        assert lib.lt_device_frames_rest(b._h, 0, 2, np.array([5, 4, 9, 9], np.int32).ctypes.data) == -1
        # nothing was launched or changed: the attached frames still give their results, and a new attach works
        _run(b, 2, 0)
        _assert_same(_results(b, 2, 0), want, "after the refusals")
        b.attach_device_frames(DeviceFrames.from_host(f, layout, pitch=good.surfaces["pitch"][0] + 7, offset=1))
        _run(b, 2, 0)
        _assert_same(_results(b, 2, 0), want, "a new attach")
        other = "nv12" if layout == "rgb" else "rgb"
        with pytest.raises(ValueError):
            b.attach_device_frames(DeviceFrames.from_planes([(good.surfaces["plane"][0, 0],) * (2 if other == "nv12" else 1)], (W, H), other,
                                                            pitch=W * 3, chroma_pitch=W))
        with pytest.raises(ValueError):
            b.attach_device_frames(DeviceFrames.from_host(np.zeros((2, 34, 66, 3) if layout == "rgb" else (2, 51, 66), np.uint8), layout))
    finally:
        a.close()
        b.close()


def test_trackers_refuse_frames_of_another_kind():
    cal = calib.reference_calibration()
    t = LaneTracker(**cal, pixel_format="nv12")
    try:
        rgb = DeviceFrames.from_host(_mix("rgb")[:2], "rgb")
        small = DeviceFrames.from_host(np.zeros((2, 51, 66), np.uint8), "nv12")
        for wrong in (rgb[0], small[0]):
            with pytest.raises(ValueError):
                t.process(wrong)
        for wrong in (rgb, small):
            with pytest.raises(ValueError):
                t.process_batch(wrong, annotate=False)
            with pytest.raises(ValueError):
                list(t.process_stream([wrong], annotate=False))
        with pytest.raises(ValueError):
            t.process(DeviceFrames.from_host(_mix("nv12")[:2], "nv12"))          # two frames are not a frame
        with pytest.raises(ValueError):
            t.process_batch(DeviceFrames.from_host(_mix("nv12")[:2], "nv12"), annotate="inplace")
        assert t.counter == 0
    finally:
        t.close()


# ---- 4. attach, detach, reuse ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_attach_detach_and_reuse(layout):
    cal = calib.reference_calibration()
    frames = _mix(layout)
    X, Y = np.ascontiguousarray(frames[0:4]), np.ascontiguousarray(frames[20:24])
    a, b = _ctx(cal, 4, layout), _ctx(cal, 4, layout)
    second = _native.filter_params("neighborhood", 15, 5, 35, 5)
    try:
        def host(f, fp=None):
            a.upload_frame_rows(f)
            a.mask_run(4, fp)
            a.sws_fit_run(4)
            return _results(a, 4, 0)
        want_x, want_y, want_x2 = host(X), host(Y), host(X, second)
        mixed = X.copy()
        mixed[1] = Y[1]
        want_mixed = host(mixed)
        block, surf, size, _ = pack_host_frames(X, layout, offset=2)
        with DeviceBuffer(block.nbytes) as buf:
            buf.copy_from_host(block)
            surf["plane"][:, :{"rgb": 1, "nv12": 2, "i420": 3}[layout]] += np.uint64(buf.ptr)
            df = DeviceFrames(surf, size, layout, owner=buf)
            b.attach_device_frames(df)
            _run(b, 4, 0)
            _assert_same(_results(b, 4, 0), want_x, "first attach")
            # the second parameter set over the front end that has run: lt_mask_rerun = lt_mask_run
            b.mask_run(4, second, reuse_front=True)
            b.sws_fit_run(4)
            # (the 'neighborhood' filter writes no top-hat planes: those keep whatever the call before left in either context)
            _assert_same(_results(b, 4, 0), want_x2, "lt_mask_rerun", planes=(_native.PLANE_R, _native.PLANE_LAB_B, _native.PLANE_MASK))
            # other frames in the same surfaces (the records above were waited for), attached again: no stale front end
            buf.copy_from_host(pack_host_frames(Y, layout, offset=2)[0])
            b.attach_device_frames(df)
            b.mask_run(4, reuse_front=True)                  # (a rerun right after an attach runs the front end)
            b.sws_fit_run(4)
            _assert_same(_results(b, 4, 0), want_y, "second attach")
            # an upload into an attached slot takes over; the range then mixes attached and plain slots
            buf.copy_from_host(block)
            b.attach_device_frames(df)
            b.upload_frame_rows(Y[1:2], first=1)
            _run(b, 4, 0)
            _assert_same(_results(b, 4, 0), want_mixed, "a mixed range")
            assert b.lib.lt_device_frames_rest(b._h, 0, 4, None) == -5           # LT_ERR_STATE: slot 1 is not attached any more
            b.sync()
    finally:
        a.close()
        b.close()


# ---- 5. shown frames ----------------------------------------------------------------------------------------------------------
def _polygons(n):
    ys = np.arange(300, 1100, dtype=np.int64)
    return [(ys, np.full_like(ys, 400 + 3 * k), ys, np.full_like(ys, 700 - 2 * k)) for k in range(n)]


def _shown(c, n, first, rows=None):
    if rows is None:
        c.overlay_run(_polygons(n), first=first)
        return c.download_overlay(n, first=first)
    c.overlay_run(_polygons(n), first=first, rows=rows.ctypes.data)
    out = _native.pinned_empty((n, H, W, 3))
    out[:] = 0
    c.download_overlay_async(out, first=first, rows=rows.ctypes.data)
    c.sync()
    return np.array(out)


def _camera(c, n, first):
    e = np.zeros(0, np.int64)
    c.overlay_run([(e, e, e, e)] * n, first=first)
    return c.download_overlay(n, first=first)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_shown_frames_equal_the_host_fed_ones(layout):
    cal = calib.reference_calibration()
    n, first = 4, 1
    f = np.ascontiguousarray(np.concatenate([_mix(layout)[12:15], _mix(layout)[3:4]]))       # noise and a scene
    rgb = f if layout == "rgb" else np.stack([R.yuv420_to_rgb(q, layout) for q in f])
    a, b = _ctx(cal, 6, layout), _ctx(cal, 6, layout)
    pitched = {"rgb": (W * 3 + 20, None), "nv12": (W + 64, W + 32), "i420": (W + 6, W // 2 + 5)}[layout]
    try:
        for c in (a, b):
            c.overlay_configure(cal["warp_matrices"][1])
        r0, r1 = a.source_rows()
        keep = [a.upload_frame_rows(f, first=first, enqueue=True)]
        a.mask_run(n, first=first)
        keep.append(a.upload_frame_rest(f, first=first))
        want = _shown(a, n, first)
        assert np.array_equal(_camera(a, n, first), rgb)
        a.sync()
        for variant in (dict(), dict(pitch=pitched[0], chroma_pitch=pitched[1], offset=0), dict(pitch=pitched[0], chroma_pitch=pitched[1], offset=3)):
            df = DeviceFrames.from_host(f, layout, **variant)
            b.attach_device_frames(df, first=first)
            b.mask_run(n, first=first)
            b.device_frames_rest(n, first=first)
            assert np.array_equal(_shown(b, n, first), want), (layout, variant, "annotated")
            assert np.array_equal(_camera(b, n, first), rgb), (layout, variant, "the slot's camera frame")
            b.sync()
        # two runs of rows (odd bounds among them): those runs, whole
        for runs in ((5, 62, r0 + 9, H - 3), (0, 1, r0 - 7, r1 + 1), (r0 + 1, r0 + 2, H - 1, H)):
            rows = np.array(runs, np.int32)
            g = np.ascontiguousarray(np.roll(f, 1 + runs[0] % 2, 0))
            keep = [a.upload_frame_rows(g, first=0, enqueue=True)]
            a.mask_run(n, first=0)
            keep.append(a.upload_frame_rest(g, first=0, rows=rows.ctypes.data))
            want_rows = _shown(a, n, 0, rows)
            a.sync()
            df = DeviceFrames.from_host(g, layout, pitch=pitched[0], chroma_pitch=pitched[1], offset=1)
            b.attach_device_frames(df, first=0)
            b.mask_run(n, first=0)
            b.device_frames_rest(n, first=0, rows=rows.ctypes.data)
            got = _shown(b, n, 0, rows)
            for lo, hi in ((runs[0], runs[1]), (runs[2], runs[3])):
                assert np.array_equal(got[:, lo:hi], want_rows[:, lo:hi]), (layout, runs, lo, hi)
            b.sync()
    finally:
        a.close()
        b.close()


# ---- 6. trackers ----------------------------------------------------------------------------------------------------------------
def _state(lt):
    b = lambda a: None if a is None else np.asarray(a).tobytes()
    return dict(detected=lt.detected_pixels, valid=lt.valid_lane_lines, last_detection=lt.last_detection, success=lt.success,
                counter=lt.counter, left_avg=b(lt.left_avg_coeffs), right_avg=b(lt.right_avg_coeffs), last_left=b(lt.last_left_coeffs),
                last_right=b(lt.last_right_coeffs), hist=[b(c) for c in lt.left_fit_coeffs] + [b(c) for c in lt.right_fit_coeffs],
                radii=list(lt.average_curve_radii), radius=lt.average_curve_radius, ecc=lt.eccentricity,
                pix=(b(lt.left_y), b(lt.left_x), b(lt.right_y), b(lt.right_x)), cent=(lt.left_window_centroids, lt.right_window_centroids))


@functools.lru_cache(maxsize=None)
def _lane_frames(layout):
    """64 frames of a drifting lane in `layout` (RGB rendered once, converted once)."""
    rgb = synth.stream_lanes(64, seed=7)
    return rgb if layout == "rgb" else np.stack([R.rgb_to_yuv420(f, layout) for f in rgb])


def _video(layout, n, blank=()):
    """n frames: the 64 played forwards and backwards (the lane never jumps); `blank`: positions of black frames."""
    base = _lane_frames(layout)
    order = np.concatenate([np.arange(64), np.arange(63, -1, -1)])
    v = base[order[np.arange(n) % 128]].copy()
    black = np.zeros((H, W, 3), np.uint8) if layout == "rgb" else \
        np.concatenate([np.full((H, W), 16, np.uint8), np.full((H // 2, W), 128, np.uint8)])
    for k in blank:
        v[k] = black
    return v


def _on_device(frames, layout):
    """Dense for one layout, pitched (and at an odd base) for the others."""
    if layout == "nv12":
        return DeviceFrames.from_host(frames, layout)
    if layout == "rgb":
        return DeviceFrames.from_host(frames, layout, pitch=W * 3 + 20, offset=1)
    return DeviceFrames.from_host(frames, layout, pitch=W + 6, chroma_pitch=W // 2 + 5, offset=3)


def _pair(layout):
    cal = calib.reference_calibration()
    return LaneTracker(**cal, pixel_format=layout), LaneTracker(**cal, pixel_format=layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_process_equals_the_host_fed_tracker(layout):
    blank = tuple(range(14, 22))                       # an outage beyond n_reset: failure pictures, second tries, the sliding-window restart
    v = _video(layout, 40, blank)
    dv = _on_device(v, layout)
    a, b = _pair(layout)
    try:
        for k in range(40):
            out_b = b.process(v[k])
            # one stream fed alternately from the host and from the device equals the host-fed one
            out_a = a.process(dv[k] if (k % 5) else v[k])
            assert isinstance(out_a, np.ndarray) and out_a.shape == (H, W, 3) and np.array_equal(out_a, out_b), k
            assert _state(a) == _state(b), k
        assert b.success * 10 >= (40 - len(blank)) * 9 and b.success < b.counter
        assert a.get_state() == b.get_state()
        va, vb = a.process(dv[3], visualize_search=True), b.process(v[3], visualize_search=True)
        assert all(np.array_equal(x, y) for x, y in zip(va, vb))
        assert np.array_equal(a.process(dv[4], split_view=True), b.process(v[4], split_view=True))
        assert np.array_equal(a.draw_lane(dv[6]), b.draw_lane(v[6]))             # a frame that is not the resident one
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("layout", ["rgb", "nv12"])
def test_process_batch_and_stream_equal_the_host_fed_tracker(layout):
    v = _video(layout, 256, blank=(20, 21, 22, 140, 141, 142, 143, 144, 145, 146))
    dv = _on_device(v, layout)
    for annotate in (False, True):
        a, b = _pair(layout)
        try:
            oa, ob = a.process_batch(dv[:24], annotate=annotate), b.process_batch(v[:24], annotate=annotate)
            assert _state(a) == _state(b), annotate
            if annotate:
                assert all(isinstance(x, np.ndarray) and np.array_equal(x, y) for x, y in zip(oa, ob))
            else:
                assert oa == ob == [None] * 24
            with pytest.raises(ValueError):
                a.process_batch(dv[:2], annotate="inplace")
            # windows of 128 (the second one with an outage), behind the batch: host-fed in one call, device-fed in the next
            ga = a.process_stream([dv[:128], dv[128:]], annotate=annotate)
            gb = b.process_stream([v[:128], v[128:]], annotate=annotate)
            for w, (oa, ob) in enumerate(itertools.zip_longest(ga, gb)):         # (both generators run to their end)
                if annotate:
                    assert len(oa) == 128 and all(np.array_equal(x, y) for x, y in zip(oa, ob)), w
                else:
                    assert oa == ob == [None] * 128
            assert _state(a) == _state(b) and a.get_state() == b.get_state(), annotate
            assert a.counter == 24 + 256 and b.success < b.counter and b.success * 10 >= (b.counter - 16) * 9      # (16 black frames)
            with pytest.raises(ValueError):
                list(a.process_stream([dv[:4], v[4:8]], annotate=annotate))      # one stream, one kind of window
        finally:
            a.close()
            b.close()


def test_group_of_four_with_an_idle_stream():
    from lane_tracker_amd.group import LaneTrackerGroup
    cal = calib.reference_calibration()
    layout = "nv12"
    base = _lane_frames(layout)
    streams = [np.ascontiguousarray(base[8 * i:8 * i + 6]) for i in range(4)]
    dev = [DeviceFrames.from_host(s, layout, pitch=W + 64 * (i % 2)) for i, s in enumerate(streams)]
    ga, gb = LaneTrackerGroup(4, **cal, pixel_format=layout), LaneTrackerGroup(4, **cal, pixel_format=layout)
    try:
        for tick in range(6):
            idle = tick % 4                            # one stream skips every call; stream 3 stays host-fed in odd ticks
            fb = [None if i == idle else streams[i][tick] for i in range(4)]
            fa = [None if i == idle else (streams[i][tick] if (i == 3 and tick % 2) else dev[i][tick]) for i in range(4)]
            oa, ob = ga.process(fa), gb.process(fb)
            for i in range(4):
                assert (oa[i] is None) == (ob[i] is None) == (i == idle)
                if i != idle:
                    assert np.array_equal(oa[i], ob[i]), (tick, i)
                assert _state(ga.trackers[i]) == _state(gb.trackers[i]), (tick, i)
        assert sum(t.success for t in gb.trackers) * 10 >= sum(t.counter for t in gb.trackers) * 9
        with pytest.raises(ValueError):
            ga.process([dev[0][:2], None, None, None])
    finally:
        ga.close()
        gb.close()


# ---- 7. a long run keeps device memory where it was --------------------------------------------------------------------------------
def test_a_long_run_keeps_device_memory_where_it_was():
    layout = "nv12"
    v = _video(layout, 128)
    a, _b = _pair(layout)
    _b.close()
    try:
        dv = DeviceFrames.from_host(v[:10], layout, pitch=W + 64)
        for k in range(10):
            a.process(dv[k])
        for w in a.process_stream([DeviceFrames.from_host(v, layout) for _ in range(2)], annotate=False):
            pass
        for k in range(10):              # (the first shown frames behind a stream size the presentation buffers for the grown context)
            a.process(dv[k])
        live = _native.device_cache_stats()["live_bytes"]
        evictions = _native.device_cache_counters()["evicted_blocks"]
        for k in range(2000):
            a.process(dv[k % 10])
        assert _native.device_cache_stats()["live_bytes"] == live
        wins = (DeviceFrames.from_host(v, layout) for _ in range(50))        # every window in a block of its own, dropped behind the stream
        for w in a.process_stream(wins, annotate=False):
            assert w == [None] * 128
        a.process(dv[0])                 # (the tracker's resident frame -- the stream's last -- kept its window alive, as it keeps a host window)
        assert a.counter == 10 + 256 + 10 + 2000 + 50 * 128 + 1
        assert _native.device_cache_stats()["live_bytes"] == live
        assert _native.device_cache_counters()["evicted_blocks"] == evictions
    finally:
        a.close()
