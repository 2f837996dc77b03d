"""Device sinks: annotated frames written into surfaces the caller owns -- RGB, NV12 or I420, pitched, planes anywhere
(lt_rgb_to_surfaces, lt_overlay_store_device, process_batch / process_stream with out=).  Everything here is bit for bit: the
4:2:0 bytes are the NumPy restatement (tests/sink_reference.py) of what an RGB download holds, the RGB bytes are that download,
and every byte of a sink that is not inside a row of a plane keeps the 0xC3 it was filled with."""
import functools
import itertools

import numpy as np
import pytest

import sink_reference as S
import yuv_reference as R
from lane_tracker_amd import _native, calib, synth, utils
from lane_tracker_amd.device import DeviceBuffer, DeviceFrames, pack_host_frames
from lane_tracker_amd.lane_tracker import LaneTracker

pytestmark = pytest.mark.gpu

LAYOUTS = ("rgb", "nv12", "i420")
W, H = calib.IMAGE_WIDTH_HEIGHT
FILL = 0xC3
SIZES = ((2, 2), (14, 2), (16, 2), (18, 4), (32, 2), (46, 6), (64, 4))      # (w, h): both the 16-column and the byte-wise form run
COUNTS = (1, 3, 33)                                                         # 33 crosses the 32-surface chunk
PITCH_EXTRA = (0, 1, 16, 37)


def _row_bytes(layout, w):
    """(row bytes of plane 0, row bytes of a chroma plane or None)."""
    return (3 * w, None) if layout == "rgb" else (w, w if layout == "nv12" else w // 2)


def _frames(n, h, w, seed):
    """Uniform noise; from three frames on, frame 1 is all 0 and frame 2 all 255."""
    f = np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if n >= 3:
        f[1], f[2] = 0, 255
    return f


def _expected(rgb, layout, matrix="bt601"):
    return rgb if layout == "rgb" else S.rgb_to_yuv420(rgb, layout, matrix)


def _pitched(planes, pitch, offset):
    """planes (n, rows, row bytes) -> the host image of a block that holds them `pitch` apart from `offset` on, FILL elsewhere, and
    ends on the last byte of the last row; the planes' offsets into it."""
    n, rows, rb = planes.shape
    total = offset + n * rows * pitch - (pitch - rb)
    block = np.full(total, FILL, np.uint8)
    view = np.lib.stride_tricks.as_strided(block[offset:], shape=(n * rows, rb), strides=(pitch, 1))
    view[...] = planes.reshape(n * rows, rb)
    return block, [offset + k * rows * pitch for k in range(n)]


class _Sink:
    """A sink pre-filled with FILL, and the bytes it must hold after `want` (the expected frames) has been written into it."""

    def __init__(self, want, layout, size, pitch, chroma_pitch, offset, split):
        w, h = size
        n = want.shape[0]
        self.blocks = []                 # (DeviceBuffer, expected host image)
        if not split:
            block, surf, _, _ = pack_host_frames(want, layout, pitch, chroma_pitch, offset, fill=FILL)
            buf = DeviceBuffer(block.nbytes).copy_from_host(np.full(block.nbytes, FILL, np.uint8))
            surf["plane"][:, :LAYOUTS.index(layout) + 1] += np.uint64(buf.ptr)     # (one, two or three planes)
            self.blocks.append((buf, block))
            self.frames = DeviceFrames(surf, size, layout, owner=buf)
            return
        # every kind of plane in an allocation of its own, each ending on the last byte of its last row
        assert layout != "rgb"
        flat = want.reshape(n, -1)
        y = flat[:, :h * w].reshape(n, h, w)
        c = flat[:, h * w:]
        chroma = [c.reshape(n, h // 2, w)] if layout == "nv12" else [c[:, :c.shape[1] // 2].reshape(n, h // 2, w // 2), c[:, c.shape[1] // 2:].reshape(n, h // 2, w // 2)]
        addrs = []
        for planes, p in [(y, pitch)] + [(q, chroma_pitch) for q in chroma]:
            block, offs = _pitched(planes, p, offset)
            buf = DeviceBuffer(block.nbytes).copy_from_host(np.full(block.nbytes, FILL, np.uint8))
            self.blocks.append((buf, block))
            addrs.append([buf.ptr + o for o in offs])
        self.frames = DeviceFrames.from_planes(list(zip(*addrs)), size, layout, pitch=pitch, chroma_pitch=chroma_pitch, owner=[b for b, _ in self.blocks])

    def check(self, what):
        for i, (buf, block) in enumerate(self.blocks):
            got = buf.copy_to_host()
            if not np.array_equal(got, block):
                bad = np.flatnonzero(got != block)
                raise AssertionError("%r: block %d differs at %d bytes, first at %d (got %d, want %d)" % (what, i, bad.size, bad[0], got[bad[0]], block[bad[0]]))

    def untouched(self):
        return all((buf.copy_to_host() == FILL).all() for buf, _ in self.blocks)

    def close(self):
        for buf, _ in self.blocks:
            buf.close()


def _sweep(layout, size, matrix, counts, extras, offsets, splits):
    w, h = size
    rb, crb = _row_bytes(layout, w)
    for n in counts:
        rgb = _frames(n, h, w, seed=n * 1000 + w * 10 + h)
        want = _expected(rgb, layout, matrix)
        with DeviceBuffer(rgb.nbytes) as src:
            src.copy_from_host(rgb)
            for extra, offset, split in itertools.product(extras, offsets, splits):
                sink = _Sink(want, layout, size, rb + extra, None if crb is None else crb + extra, offset, split)
                try:
                    _native.rgb_to_surfaces(src.ptr, h * w * 3, size, sink.frames, matrix)
                    sink.check((layout, size, n, extra, offset, split))
                finally:
                    sink.close()


# ---- 1. the converter alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_converter_sweep(layout, size):
    _sweep(layout, size, "bt601", COUNTS, PITCH_EXTRA, range(16), (False,) if layout == "rgb" else (False, True))


# ---- 2. user matrices -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix", ["bt709", S.CLAMPING], ids=["bt709", "clamping"])
@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_user_matrices(layout, matrix):
    for size in ((18, 4), (32, 2), (64, 4)):
        _sweep(layout, size, matrix, (3,), (0, 37), (0, 5), (False, True))


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------
def _ctx(cal, capacity, pixel_format="rgb"):
    c = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], capacity=capacity)
    if pixel_format != "rgb":
        c.set_input_format(pixel_format)
    return c


def _refused(kind, call):
    """The call is refused with LT_ERR_INVALID (-1: ValueError) or LT_ERR_STATE (-5) and a message."""
    with pytest.raises(ValueError if kind == "invalid" else _native.NativeError) as e:
        call()
    assert str(e.value).strip() and (kind == "invalid" or "error -5" in str(e.value)), str(e.value)


def test_refusals_of_the_converter():
    w, h, n = 32, 4, 2
    rgb = _frames(n, h, w, 5)
    with DeviceBuffer(rgb.nbytes) as src:
        src.copy_from_host(rgb)
        run = lambda frames, size=(w, h), matrix="bt601", ptr=None, stride=h * w * 3: _native.rgb_to_surfaces(
            src.ptr if ptr is None else ptr, stride, size, frames, matrix)
        for layout in ("nv12", "rgb", "i420"):
            want = _expected(rgb, layout)
            rb, crb = _row_bytes(layout, w)
            sink = _Sink(want, layout, (w, h), rb + 16, None if crb is None else crb + 16, 0, False)
            try:
                good = sink.frames
                def variant(**kw):
                    s = good.surfaces.copy()
                    for k, v in kw.items():
                        if k.startswith("plane"):
                            s["plane"][:, int(k[5:])] = v
                        else:
                            s[k] = v
                    return DeviceFrames(s, (w, h), layout, owner=good.owner)
                last = 0 if layout == "rgb" else (1 if layout == "nv12" else 2)
                _refused("invalid", lambda: run(variant(**{"plane%d" % last: 0})))                       # a null plane
                _refused("invalid", lambda: run(variant(pitch=rb - 1)))                                  # a pitch below the row
                if crb is not None:
                    _refused("invalid", lambda: run(variant(chroma_pitch=crb - 1)))
                host = np.zeros(1 << 16, np.uint8)
                _refused("invalid", lambda: run(variant(plane0=host.ctypes.data)))                       # a host pointer
                s = good.surfaces.copy()
                s["plane"][1] = s["plane"][0]                                                             # two destinations, one place
                _refused("invalid", lambda: run(DeviceFrames(s, (w, h), layout, owner=good.owner)))
                s = good.surfaces.copy()
                s["plane"][1, 0] = s["plane"][0, 0] + np.uint64(rb - 1)                                  # ... sharing one byte
                _refused("invalid", lambda: run(DeviceFrames(s, (w, h), layout, owner=good.owner)))
                s = good.surfaces.copy()
                s["plane"][:, last] += np.uint64(1)                                                       # an extent one byte past the allocation
                _refused("invalid", lambda: run(DeviceFrames(s, (w, h), layout, owner=good.owner)))
                if layout != "rgb":
                    top = ((1 << 31) - 1 - (1 << 19) - (128 << 20)) // 255      # the largest row sum sum |c| the int32 rule takes
                    run(good, matrix=[0, 0, 0, 0, 0, top, 0, 0])                 # (at the limit: taken)
                    sink.blocks[0][0].copy_from_host(np.full(sink.blocks[0][1].nbytes, FILL, np.uint8))
                    for k in ([1 << 23] + [0] * 7, [0, 0, 0, 0, 0, top + 1, 0, 0], [4000000, 4000000, 0, 0, 0, 0, 0, 0]):
                        _refused("invalid", lambda: run(good, matrix=k))                                   # coefficients out of bounds
                _refused("invalid", lambda: run(good, ptr=host.ctypes.data))                             # the source is not a library block
                _refused("invalid", lambda: run(good, stride=h * w * 3 + 64))                            # ... or runs past its end
                assert sink.untouched(), layout                                                           # nothing reached the device
                run(good)
                sink.check(("after the refusals", layout))
            finally:
                sink.close()
        # odd sizes: the library is asked directly (DeviceFrames itself refuses to describe odd 4:2:0 frames)
        lib = _native.load()
        k = _native.rgb2yuv_coeffs("bt601")
        with DeviceBuffer(4096) as dst:
            dst.copy_from_host(np.full(4096, FILL, np.uint8))
            surf = np.zeros(1, _native.SURFACE_DTYPE)
            surf["plane"][0, :2] = dst.ptr, dst.ptr + 2048
            surf["pitch"], surf["chroma_pitch"] = 64, 64
            for ww, hh in ((31, 4), (32, 3)):
                rc = lib.lt_rgb_to_surfaces(0, src.ptr, ww * hh * 3, hh, ww, 1, surf.ctypes.data, 1, k.ctypes.data)
                assert rc == -1 and lib.lt_last_error(), (ww, hh)
            assert lib.lt_rgb_to_surfaces(0, src.ptr, 32 * 4 * 3, 4, 32, 1, surf.ctypes.data, 3, k.ctypes.data) == -1     # no such layout
            assert lib.lt_rgb_to_surfaces(0, src.ptr, 32 * 4 * 3, 4, 32, 1, surf.ctypes.data, 1, None) == -1              # no coefficients
            assert (dst.copy_to_host() == FILL).all()


def _poly(warped, lf, rf, partial=1.0):
    """get_poly_points for two parabolas: (left_y, left_x, right_y, right_x) inside the bird's-eye image."""
    bw, bh = warped
    ys = np.arange(int(bh * (1 - partial)), bh, dtype=np.float64)
    out = []
    for c in (lf, rf):
        x = c[0] * ys * ys + c[1] * ys + c[2]
        x = x[(x >= 0) & (x <= bw - 1)].astype(np.int64)
        out += [np.arange(bh - len(x), bh, dtype=np.int64), x]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _scenes():
    r = synth.SceneRenderer()
    return np.stack([r.render(40 + i)[0] for i in range(6)])


def _polys(cal, shift):
    return [_poly(cal["warped_size"], (1e-5 * (i - 2), -0.05 + 0.01 * i, 400.0 + 10 * i + shift), (1e-5 * (i - 2), -0.05 + 0.01 * i, 600.0 + 10 * i + shift),
                  1.0 if i % 2 else 0.6) for i in range(6)]


def test_refusals_of_the_context_store():
    cal = calib.reference_calibration()
    frames = _scenes()[:2]
    c = _ctx(cal, 4)
    sink = DeviceFrames.empty(2, (W, H), "nv12", fill=FILL)
    feed = DeviceFrames.from_host(frames, "rgb")
    try:
        _refused("state", lambda: c.store_overlay_device(sink))                                   # before any overlay
        c.overlay_configure(cal["warp_matrices"][1])
        c.upload_frames(frames)
        rows = np.array([0, 100, 400, 700], np.int32)
        c.overlay_run(_polys(cal, 0)[:2], rows=rows.ctypes.data)
        _refused("state", lambda: c.store_overlay_device(sink))                                   # row runs only: no whole annotated frame
        c.overlay_run(_polys(cal, 0)[:2])
        want = c.download_overlay(2)
        with pytest.raises(ValueError):
            c.store_overlay_device(DeviceFrames.empty(2, (W, H + 2), "nv12"))                     # another size
        with pytest.raises(_native.NativeError):
            c.store_overlay_device(sink, first=3)                                                 # slots outside the capacity
        _refused("invalid", lambda: c.store_overlay_device(sink, matrix=[1 << 23] + [0] * 7))
        s = sink.surfaces.copy()
        s["plane"][1, 1] = s["plane"][0, 0] + np.uint64(5)
        _refused("invalid", lambda: c.store_overlay_device(DeviceFrames(s, (W, H), "nv12", owner=sink.owner)))
        # a destination that overlaps a camera surface attached to a slot -- any slot -- of the context
        c.attach_device_frames(feed, first=2)
        over = DeviceFrames(feed.surfaces.copy(), (W, H), "rgb", owner=feed.owner)
        _refused("invalid", lambda: c.store_overlay_device(over))
        c.sync()
        assert np.array_equal(feed.to_host(), frames)                                             # ... and it was not written
        assert (sink.owner.copy_to_host() == FILL).all()                                          # nothing has reached the sink so far
        c.store_overlay_device(sink)
        c.store_wait()
        assert np.array_equal(sink.to_host(), S.rgb_to_yuv420(want, "nv12"))
    finally:
        c.close()
        sink.owner.close()
        feed.owner.close()


# ---- 4. the context path ----------------------------------------------------------------------------------------------------------------
def _sink_variants(layout, n):
    """dense, and pitched at an odd offset."""
    rb, crb = _row_bytes(layout, W)
    return [DeviceFrames.empty(n, (W, H), layout, fill=FILL),
            DeviceFrames.empty(n, (W, H), layout, pitch=rb + 37, chroma_pitch=None if crb is None else crb + 21, offset=3, fill=FILL)]


def _outside_rows_untouched(sink):
    """Every byte of the sink's block that is not inside a row of a plane still holds FILL."""
    raw = sink.owner.copy_to_host()
    inside = np.zeros(raw.size, bool)
    for s in sink.surfaces:
        for i, (rows, rb, which) in enumerate(sink._plane_sizes()):
            at, pitch = int(s["plane"][i]) - sink.owner.ptr, int(s[which])
            for r in range(rows):
                inside[at + r * pitch:at + r * pitch + rb] = True
    return bool((raw[~inside] == FILL).all())


def test_context_store_equals_the_download():
    from lane_tracker_amd import overlay
    cal = calib.reference_calibration()
    frames = _scenes()
    n = len(frames)
    c = _ctx(cal, n)
    sinks = []
    try:
        c.overlay_configure(cal["warp_matrices"][1])
        font = overlay.font_atlas()
        if font is not None:
            c.overlay_set_font(*font)
        texts = [["Curve Radius: %d m" % (900 + i), "Eccentricity: -0.25 m"] for i in range(n)]
        c.upload_frames(frames)

        def draw(shift):
            c.overlay_run(_polys(cal, shift))
            if font is not None:
                c.overlay_text(texts)
        draw(0)
        first = c.download_overlay(n).copy()
        draw(60)
        second = c.download_overlay(n).copy()
        assert not np.array_equal(first, second) and not np.array_equal(first, frames)
        for layout in LAYOUTS:
            for a, b in zip(_sink_variants(layout, n), _sink_variants(layout, n)):
                sinks += [a, b]
                # two overlays and two stores over the same slots, the host waiting once: each store reads what the overlay in
                # front of it drew, and the second overlay does not overtake the first store
                draw(0)
                c.store_overlay_device(a)
                draw(60)
                c.store_overlay_device(b)
                c.store_wait()
                for sink, want in ((a, first), (b, second)):
                    assert np.array_equal(sink.to_host(), _expected(want, layout)), (layout, int(sink.surfaces["pitch"][0]))
                    assert _outside_rows_untouched(sink), layout
        # a piece of the slots, into a piece of a sink; an lt_sync instead of the store's own wait
        part = DeviceFrames.empty(n, (W, H), "i420", fill=FILL)
        sinks.append(part)
        c.store_overlay_device(part[2:5], first=2, matrix="bt709")
        c.sync()
        got = part.to_host()
        assert np.array_equal(got[2:5], S.rgb_to_yuv420(second[2:5], "i420", "bt709")) and (got[:2] == FILL).all() and (got[5:] == FILL).all()
    finally:
        c.close()
        for s in sinks:
            s.owner.close()


# ---- 5., 6. trackers ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _video(layout):
    """24 frames of a drifting lane with a blank frame (an outage) in the middle of each dozen, in `layout`."""
    rgb = synth.stream_lanes(24, seed=7).copy()
    rgb[5], rgb[17] = 0, 0
    return rgb if layout == "rgb" else np.stack([R.rgb_to_yuv420(f, layout) for f in rgb])


def _pair(layout):
    cal = calib.reference_calibration()
    return LaneTracker(**cal, pixel_format=layout), LaneTracker(**cal, pixel_format=layout)


CONFIGS = {"host rgb -> rgb": ("rgb", False, "rgb"), "device nv12 -> nv12": ("nv12", True, "nv12"), "device rgb -> i420": ("rgb", True, "i420")}


def _new_sink(out_layout, n, k=0):
    rb, crb = _row_bytes(out_layout, W)
    if k % 2 == 0:
        return DeviceFrames.empty(n, (W, H), out_layout, fill=FILL)
    return DeviceFrames.empty(n, (W, H), out_layout, pitch=rb + 37, chroma_pitch=None if crb is None else crb + 21, offset=3, fill=FILL)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_process_batch_into_a_sink(config):
    in_layout, on_device, out_layout = CONFIGS[config]
    v = _video(in_layout)[:12]
    a, b = _pair(in_layout)
    feed = DeviceFrames.from_host(v, in_layout) if on_device else v
    sink = _new_sink(out_layout, 12, 1)
    try:
        want = np.stack(b.process_batch(v, annotate=True))
        got = a.process_batch(feed, out=sink)
        assert len(got) == 12 and all(isinstance(g, DeviceFrames) and g.single and g.pixel_format == out_layout for g in got)
        assert np.array_equal(got[7].to_host(), sink.to_host()[7])
        assert np.array_equal(sink.to_host(), _expected(want, out_layout))
        assert _outside_rows_untouched(sink)
        assert a.get_state() == b.get_state()
        assert b.success < b.counter == 12 and b.success >= 8                  # the outage was one, and the lane was found around it
        # the route without chained searches ends in the same store; one frame per call is a window of one
        a.chain_searches = b.chain_searches = False
        want = np.stack(b.process_batch(v[:3], annotate=True))
        again = _new_sink(out_layout, 3, 0)
        try:
            a.process_batch(feed[:3], out=again)
            assert np.array_equal(again.to_host(), _expected(want, out_layout))
        finally:
            again.owner.close()
        a.chain_searches = b.chain_searches = True
        want = b.process_batch(v[3:4], annotate=True)[0]
        a.process_batch(feed[3:4], out=sink[3:4], out_yuv_matrix="bt709")
        assert np.array_equal(sink[3].to_host(), _expected(want[None], out_layout, "bt709")[0])
        assert a.get_state() == b.get_state()
    finally:
        a.close()
        b.close()
        sink.owner.close()
        if on_device:
            feed.owner.close()


@pytest.mark.parametrize("config", list(CONFIGS))
def test_process_stream_into_sinks(config):
    in_layout, on_device, out_layout = CONFIGS[config]
    v = _video(in_layout)
    a, b = _pair(in_layout)
    feed = DeviceFrames.from_host(v, in_layout) if on_device else v
    sinks = [_new_sink(out_layout, 8, k) for k in range(3)]
    try:
        windows = [feed[8 * k:8 * k + 8] for k in range(3)]
        gb = b.process_stream([v[8 * k:8 * k + 8] for k in range(3)], annotate=True)
        ga = a.process_stream(windows, out=iter(sinks))
        count = 0
        for k, (oa, ob) in enumerate(itertools.zip_longest(ga, gb)):
            assert len(oa) == 8 and all(isinstance(g, DeviceFrames) for g in oa)
            # the window is final when it is yielded
            assert np.array_equal(sinks[k].to_host(), _expected(np.stack(ob), out_layout)), k
            assert _outside_rows_untouched(sinks[k])
            count += 1
        assert count == 3 and a.get_state() == b.get_state() and b.counter == 24 and b.success < 24
    finally:
        a.close()
        b.close()
        for s in sinks:
            s.owner.close()
        if on_device:
            feed.owner.close()


def test_keyword_combinations_a_sink_refuses():
    v = _video("rgb")[:4]
    a, b = _pair("rgb")
    b.close()
    sink = DeviceFrames.empty(4, (W, H), "nv12")
    small = DeviceFrames.empty(4, (W, H - 2), "nv12")
    try:
        bad = [dict(annotate=False), dict(annotate="inplace"), dict(visualize_search=True), dict(split_view=True)]
        for kw in bad:
            with pytest.raises(ValueError):
                a.process_batch(v, out=sink, **kw)
            with pytest.raises(ValueError):
                list(a.process_stream([v], out=[sink], **kw))
        for wrong in (sink[:3], small, v):                                     # a wrong count, a wrong size, not a sink at all
            with pytest.raises(ValueError):
                a.process_batch(v, out=wrong)
            with pytest.raises(ValueError):
                list(a.process_stream([v], out=[wrong]))
        elsewhere = DeviceFrames(sink.surfaces, (W, H), "nv12", owner=sink.owner, device=1)
        with pytest.raises(ValueError):
            a.process_batch(v, out=elsewhere)                                  # a sink on another device
        with pytest.raises(ValueError):
            list(a.process_stream([v, v], out=[sink]))                         # fewer sinks than windows
        assert a.counter == 0                                                  # every one of them was refused before a frame was touched
    finally:
        a.close()
        sink.owner.close()
        small.owner.close()


# ---- 7. utils.rgb_to_yuv ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_utils_rgb_to_yuv(layout):
    rgb = _scenes()[1]
    got = utils.rgb_to_yuv(rgb, layout)
    assert got.shape == (H * 3 // 2, W) and got.dtype == np.uint8
    assert np.array_equal(got, S.rgb_to_yuv420(rgb, layout, "bt601"))
    assert np.array_equal(utils.rgb_to_yuv(rgb[:46, :18], layout, "bt709"), S.rgb_to_yuv420(rgb[:46, :18], layout, "bt709"))
    with pytest.raises(ValueError):
        utils.rgb_to_yuv(rgb[:45], layout)
    with pytest.raises(ValueError):
        utils.rgb_to_yuv(rgb, "rgb")
