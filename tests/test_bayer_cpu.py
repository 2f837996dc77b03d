"""8-bit raw Bayer input without a GPU: the NumPy restatement (`tests/bayer_reference.py`) held against itself -- border form against
clamp form, a scalar loop written from the header's definition, mosaics of one colour -- and against OpenCV where it imports; the
arithmetic of `csrc/bayer_arith.h` compiled for the host and run over random mosaics against the restatement
(`tests/bayer_arith_host.cpp`, once more under ASan + UBSan: a stand-alone program); the name tables; what a tracker, a group,
`DeviceFrames` and `video.py` accept and refuse before any device call; the state contract on the CPU stand-in for a context.

On the commit before this format existed `pixel_format='bayer_rggb'` raises ValueError and `_native.BAYER_FORMATS` does not exist:
everything below the restatement's own tests fails there."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bayer_reference as RB
import fake_context
from lane_tracker_amd import _native, calib, synth, utils, video
from lane_tracker_amd.device import DeviceFrames, pack_host_frames
from lane_tracker_amd.group import LaneTrackerGroup
from lane_tracker_amd.lane_tracker import LaneTracker

try:
    import cv2
except Exception:   # ImportError, or a broken binary wheel
    cv2 = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
PATTERNS = list(RB.PATTERNS)
SIZES = [(4, 4), (6, 8), (64, 48)]       # (H, W)
BASE = 0x7f0000001000                    # a made-up device address: nothing here dereferences it


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _loop_form(m, pattern):
    """The header's definition, pixel by pixel: interior pixels, then the border columns, then the border rows."""
    h, w = m.shape
    m = m.astype(int)
    out = np.zeros((h, w, 3), np.uint8)
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            own = RB.colour_at(pattern, y, x)
            cross = (m[y - 1, x] + m[y + 1, x] + m[y, x - 1] + m[y, x + 1] + 2) >> 2
            diag = (m[y - 1, x - 1] + m[y - 1, x + 1] + m[y + 1, x - 1] + m[y + 1, x + 1] + 2) >> 2
            px = [0, 0, 0]
            if own != 1:
                px[own], px[1], px[2 - own] = m[y, x], cross, diag
            else:
                px[1] = m[y, x]
                px[RB.colour_at(pattern, y, x + 1)] = (m[y, x - 1] + m[y, x + 1] + 1) >> 1
                px[RB.colour_at(pattern, y + 1, x)] = (m[y - 1, x] + m[y + 1, x] + 1) >> 1
            out[y, x] = px
    out[:, 0], out[:, w - 1] = out[:, 1], out[:, w - 2]
    out[0], out[h - 1] = out[1], out[h - 2]
    return out


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("h,w", SIZES)
def test_border_form_is_clamp_form_is_the_written_out_loop(pattern, h, w):
    m = np.random.default_rng(h * 100 + w).integers(0, 256, (h, w), dtype=np.uint8)
    clamp = RB.bayer_to_rgb(m, pattern)
    assert clamp.shape == (h, w, 3) and clamp.dtype == np.uint8
    assert np.array_equal(clamp, RB.bayer_to_rgb_border(m, pattern))
    assert np.array_equal(clamp, _loop_form(m, pattern))
    assert np.array_equal(RB.bayer_to_rgb(np.stack([m, m[::-1].copy()]), pattern)[0], clamp)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("h,w", SIZES)
def test_a_mosaic_of_one_colour_comes_back_as_that_colour(pattern, h, w):
    for colour in ((200, 40, 90), (0, 255, 1), (255, 255, 255), (0, 0, 0)):
        m = RB.rgb_to_bayer(np.full((h, w, 3), colour, np.uint8), pattern)
        assert m.shape == (h, w)
        assert (RB.bayer_to_rgb(m, pattern) == np.array(colour, np.uint8)).all()
    # the name says which colour the top-left block carries
    block = RB.rgb_to_bayer(np.broadcast_to(np.array([10, 20, 30], np.uint8), (h, w, 3)), pattern)[:2, :2].reshape(-1)
    assert [{"r": 10, "g": 20, "b": 30}[c] for c in pattern[6:]] == list(block)


def test_the_restatement_refuses_what_is_no_mosaic():
    for bad in (np.zeros((5, 8), np.uint8), np.zeros((4, 2), np.uint8), np.zeros((4, 4, 1), np.uint8), np.zeros((4, 4), np.int32)):
        with pytest.raises(ValueError):
            RB.bayer_to_rgb(bad, "bayer_rggb")


@pytest.mark.skipif(cv2 is None, reason="UNVERIFIED vs OpenCV (cv2 absent)")
@pytest.mark.parametrize("pattern", PATTERNS)
def test_restatement_is_opencv(pattern):
    """What the definition is understood to be: cv2.cvtColor(frame, cv2.COLOR_BayerRGGB2RGB) and its three siblings."""
    frame = np.random.default_rng(9).integers(0, 256, (48, 64), dtype=np.uint8)
    code = getattr(cv2, "COLOR_Bayer%s2RGB" % pattern[6:].upper())
    assert np.array_equal(RB.bayer_to_rgb(frame, pattern), cv2.cvtColor(frame, code))


# ---- bayer_arith.h on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def arith_host(request, tmp_path_factory):
    if CXX is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("bayer_arith") / "bayer_arith_host")
    build = subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", *request.param, "-I", os.path.join(ROOT, "lane_tracker_amd", "csrc"),
                            os.path.join(ROOT, "tests", "bayer_arith_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    return exe


@pytest.mark.parametrize("pattern", PATTERNS)
def test_header_arithmetic_is_the_restatement(arith_host, tmp_path, pattern):
    """Random mosaics (and the two extremes) of 4x4, 6x4, 8x6 and 14x10: every sample position with sy in -3 .. H + 2 and sx in -3 ..
    W + 2 -- below 0, at 0, interior, at H - 2 / W - 2 and beyond -- through the walk's clamps, the window placement, four 4-byte
    window rows out of a heap block of exactly H * W bytes and the tap demosaic; each of the four taps must be the restatement's
    pixel at the tap's coordinate clamped to the image."""
    rng = np.random.default_rng(PATTERNS.index(pattern))
    for h, w in ((4, 4), (4, 6), (6, 8), (10, 14)):
        for rep in range(4):
            m = rng.integers(0, 256, (h, w), dtype=np.uint8) if rep < 2 else np.full((h, w), 255 * (rep - 2), np.uint8)
            src, dst = str(tmp_path / "m.bin"), str(tmp_path / "out.bin")
            m.tofile(src)
            run = subprocess.run([arith_host, str(PATTERNS.index(pattern)), str(h), str(w), src, dst], capture_output=True, text=True, timeout=120,
                                 env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
            assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
            assert run.stdout.strip() == "ok %d" % ((h + 6) * (w + 6))
            got = np.fromfile(dst, "<u4").reshape(h + 6, w + 6, 2, 2)
            want = RB.bayer_to_rgb(m, pattern).astype(np.uint32)
            packed = want[..., 0] | (want[..., 1] << 8) | (want[..., 2] << 16)
            sy, sx = np.mgrid[-3:h + 3, -3:w + 3]
            for j in range(2):
                for i in range(2):
                    assert np.array_equal(got[:, :, j, i], packed[np.clip(sy + j, 0, h - 1), np.clip(sx + i, 0, w - 1)]), (pattern, h, w, rep, j, i)


# ---- name tables ----------------------------------------------------------------------------------------------------------------
def test_new_ids_and_the_pinned_tables():
    assert _native.BAYER_FORMATS == {"bayer_rggb": 16, "bayer_grbg": 17, "bayer_gbrg": 18, "bayer_bggr": 19} == RB.LAYOUT
    assert _native.PIXEL_FORMATS == {"rgb": 0, "nv12": 1, "i420": 2}
    assert _native.INPUT_FORMATS == {"rgb": 0, "nv12": 1, "i420": 2, "yuy2": 3, "uyvy": 4}
    assert _native.RGB_FAMILY == {"bgr": 5, "rgba": 6, "bgra": 7}
    header = open(os.path.join(ROOT, "include", "lane_tracker_amd.h")).read()
    for name, value in _native.BAYER_FORMATS.items():
        assert re.search(r"\bLT_INPUT_%s = %d\b" % (name.upper(), value), header)
        assert _native.pixel_format_id(name) == value and _native.format_name(value) == name
        assert not _native.is_yuv(value)
        assert _native.frame_shape((64, 48), name) == _native.input_frame_shape((64, 48), name) == (48, 64)
        with pytest.raises(ValueError, match="input format only"):
            _native.sink_format_id(name)
        with pytest.raises(ValueError, match="input format only"):
            _native.draw_sink_format_id(name)
        with pytest.raises(ValueError, match="RGB"):
            _native.checked_input_size((1920, 1080), (1280, 720), name)
        for size in ((63, 48), (64, 47), (2, 48), (64, 2), (0, 0)):
            with pytest.raises(ValueError):
                _native.frame_shape(size, name)
    assert int(re.search(r"#define LT_ABI_VERSION (\d+)", header).group(1)) == 5 == _native.ABI_VERSION
    assert re.search(r"\blt_bayer_to_rgb\s*\(", header) and "lt_bayer_to_rgb" in _native._SIGNATURES
    assert "lt_bayer_to_rgb" in _native.exported_symbols() and hasattr(_native.load(), "lt_bayer_to_rgb")
    with pytest.raises(ValueError):
        _native.pixel_format_id("bayer")
    # null arguments are errors without a GPU
    lib = _native.load()
    assert lib.lt_bayer_to_rgb(None, None, 4, 4, 16, None) == -1


# ---- DeviceFrames ------------------------------------------------------------------------------------------------------------------
def _iface(shape, strides=None, ptr=BASE, **more):
    return dict({"shape": tuple(shape), "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": strides}, **more)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_device_frames_take_one_plane(pattern):
    H, W = 6, 8
    for pitch in (W, W + 5):
        one = DeviceFrames.from_cuda_array(_iface((H, W), (pitch, 1)), pattern)
        assert one.single and len(one) == 1 and one.img_size == (W, H) and one.shape == (H, W) and one.pixel_format == pattern
        assert int(one.surfaces["plane"][0, 0]) == BASE and int(one.surfaces["pitch"][0]) == pitch and not one.surfaces["plane"][0, 1:].any()
        fs = H * pitch + 11
        many = DeviceFrames.from_cuda_array(_iface((3, H, W), (fs, pitch, 1)), pattern)
        assert not many.single and many.shape == (3, H, W)
        assert [int(p) for p in many.surfaces["plane"][:, 0]] == [BASE + k * fs for k in range(3)] and set(many.surfaces["pitch"]) == {pitch}
        p = DeviceFrames.from_planes([(BASE,), (BASE + fs,)], (W, H), pattern, pitch=pitch)
        assert len(p) == 2 and p.shape == (2, H, W) and set(p.surfaces["pitch"]) == {pitch} and set(p.surfaces["chroma_pitch"]) == {0}
        p.check_for((W, H), pattern)
        with pytest.raises(ValueError):
            p.check_for((W, H), "rgb")
        with pytest.raises(ValueError):
            p.check_for((W + 2, H), pattern)
    for bad in (_iface((H, W - 1)), _iface((H + 1, W)), _iface((2, W)), _iface((H, W, 1)), _iface((2, H, W, 3)),
                _iface((H, W), (2 * W, 2)),                  # a pixel stride that is not 1
                _iface((H, W), (W - 1, 1)),                  # a pitch below W
                _iface((H, W), (1 << 23, 1))):
        with pytest.raises(ValueError):
            DeviceFrames.from_cuda_array(bad, pattern)
    with pytest.raises(ValueError):
        DeviceFrames.from_planes([(BASE,)], (W, H), pattern, pitch=W - 1)
    with pytest.raises(ValueError, match="input format only"):
        DeviceFrames.empty(2, (W, H), pattern)                # not a sink
    frames = np.random.default_rng(3).integers(0, 256, (2, H, W), dtype=np.uint8)
    pitch, off = W + 5, 3
    block, surf, size, single = pack_host_frames(frames, pattern, pitch=pitch, offset=off, fill=0xEE)
    assert size == (W, H) and not single and block.size == off + 2 * H * pitch - 5               # it ends on the last byte of the last row
    for k in range(2):
        rows = np.lib.stride_tricks.as_strided(block[int(surf["plane"][k, 0]):], shape=(H, W), strides=(pitch, 1))
        assert np.array_equal(rows, frames[k])
    assert pack_host_frames(frames[0], pattern)[3]
    for bad in (np.zeros((H, W, 3), np.uint8), np.zeros((H, W + 1), np.uint8), np.zeros((2, 2, H, W), np.uint8)):
        with pytest.raises(ValueError):
            pack_host_frames(bad, pattern)


# ---- the Python layer on the CPU stand-in -----------------------------------------------------------------------------------------
class _Ctx(fake_context.FakeContext):
    """The CPU stand-in as a raw Bayer context: uploads take mosaics (n, H, W) and hold their demosaiced form, as the device context
    holds it in the slot's camera frame."""
    touched = 0

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.layout = "rgb"

    def set_input_format(self, pixel_format, matrix="bt601"):
        self.layout = pixel_format

    def set_input_size(self, size):
        raise AssertionError("an input size reached the context")

    def attach_device_frames(self, frames, first=0):
        type(self).touched += 1
        raise AssertionError("a frame in device memory reached the context")

    def upload_frame_rows(self, frames, first=0, enqueue=False):
        type(self).touched += 1
        if self.layout == "rgb":
            return super().upload_frame_rows(frames, first, enqueue)
        f = np.asarray(frames).reshape(-1, self.img_h, self.img_w)
        return super().upload_frame_rows(RB.bayer_to_rgb(f, self.layout), first, enqueue)
    upload_frames = upload_frame_rows


@pytest.fixture()
def fake(monkeypatch):
    monkeypatch.setattr(_native, "Context", _Ctx)
    _Ctx.touched = 0
    return _Ctx


@pytest.mark.parametrize("pattern", PATTERNS)
def test_refusals_come_before_any_device_call(fake, pattern):
    cal = calib.reference_calibration()
    W, H = cal["img_size"]

    def no_device(*a, **k):
        raise AssertionError("a device context was created")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_native, "Context", no_device)
        for kind in (LaneTracker, lambda **k: LaneTrackerGroup(2, **k)):
            with pytest.raises(ValueError, match="RGB"):
                kind(**cal, pixel_format=pattern, input_size=(W // 2, H // 2))              # these frames are not resized
            for size in ((W + 1, H), (W, H + 1), (2, H), (W, 2)):                          # odd or too small
                with pytest.raises(ValueError, match="even width and height of at least 4"):
                    kind(**dict(cal, img_size=size), pixel_format=pattern)
    t, rgb = LaneTracker(**cal, pixel_format=pattern), LaneTracker(**cal)
    try:
        assert t._ctx.layout == pattern and t._frame_shape == (H, W)
        host = np.zeros((2, H, W), np.uint8)
        rgb_host = np.zeros((2, H, W, 3), np.uint8)
        feed = DeviceFrames.from_planes([(BASE,), (BASE + H * W,)], (W, H), pattern, pitch=W)
        # a raw Bayer container as out=, whatever the tracker's own format
        for tracker, frames in ((t, host), (t, feed), (rgb, rgb_host)):
            with pytest.raises(ValueError, match="input format only"):
                tracker.process_batch(frames, out=feed)
            with pytest.raises(ValueError, match="input format only"):
                list(tracker.process_stream([frames], out=[feed]))
        # nothing is drawn into raw Bayer frames
        for frames in (feed, host):
            with pytest.raises(ValueError):
                t.process_batch(frames, out="inplace")
            with pytest.raises(ValueError):
                list(t.process_stream([frames], out="inplace"))
            with pytest.raises(ValueError):
                t.process_batch(frames, annotate="inplace")
            with pytest.raises(ValueError):
                list(t.process_stream([frames], annotate="inplace"))
        with pytest.raises(ValueError, match="input format only"):
            t.process_batch(feed, out="inplace", out_yuv_matrix="bt601")
        # frames of another shape: a trailing axis of 1, a 4:2:0 block, RGB
        for bad in (np.zeros((2, H, W, 1), np.uint8), np.zeros((2, H * 3 // 2, W), np.uint8), rgb_host, np.zeros((H, W), np.uint8)):
            with pytest.raises(ValueError):
                t.process_batch(bad, annotate=False)
        for bad in (np.zeros((H, W, 1), np.uint8), np.zeros((H * 3 // 2, W), np.uint8), np.zeros((H, W, 3), np.uint8), np.zeros((1, H, W), np.uint8), None,
                    DeviceFrames.from_planes((BASE,), (W, H), "rgb", pitch=3 * W)):
            with pytest.raises(ValueError):
                t.process(bad)
        with pytest.raises(ValueError):
            rgb.process(feed[0])
        assert t._rows_for(np.zeros((H, W, 3), np.uint8)) is None            # host frames never travel as row runs copied by the host
        assert t.counter == 0 and rgb.counter == 0 and fake.touched == 0
        st = t.get_state()                                                   # the format's name travels in the state
        assert st["pixel_format"] == pattern
        with pytest.raises(ValueError):
            rgb.set_state(st)
    finally:
        t.close()
        rgb.close()
    g = LaneTrackerGroup(2, **cal, pixel_format=pattern)
    try:
        assert g._ctx.layout == pattern and all(m.pixel_format == pattern for m in g.trackers)
        for bad in (np.zeros((H, W, 1), np.uint8), np.zeros((H * 3 // 2, W), np.uint8), np.zeros((H, W, 3), np.uint8)):
            with pytest.raises(ValueError):
                g.process([bad, None], annotate=False)
        with pytest.raises(ValueError):
            g.process([np.zeros((H, W), np.uint8), None], out="inplace")
        with pytest.raises(ValueError, match="input format only"):
            g.process([np.zeros((H, W), np.uint8)] * 2, out=feed)
        assert fake.touched == 0
    finally:
        g.close()
    with pytest.raises(ValueError):
        utils.rgb_to_yuv(np.zeros((4, 8, 3), np.uint8), pattern)
    with pytest.raises(ValueError):
        utils.yuv_to_rgb(np.zeros((4, 8), np.uint8), pattern)
    with pytest.raises(ValueError):
        utils.bayer_to_rgb(np.zeros((4, 8), np.uint8), "rggb")


def _scene_mosaics(pattern, n):
    r = synth.SceneRenderer()
    return RB.rgb_to_bayer(np.stack([r.render(i)[0] for i in range(n)], 0), pattern)


def test_state_is_that_of_an_rgb_tracker_fed_the_demosaiced_frames(fake):
    """Six scenes mosaiced by sampling the pattern are the camera's frames: a raw Bayer tracker fed them and an RGB tracker fed their
    demosaiced form end with equal state dicts but for the format's name, and the RGB tracker found its lane in every frame."""
    cal = calib.reference_calibration()
    pattern = "bayer_grbg"
    raw = _scene_mosaics(pattern, 6)
    back = RB.bayer_to_rgb(raw, pattern)
    assert raw.shape == (6, cal["img_size"][1], cal["img_size"][0])
    bay, plain = LaneTracker(**cal, pixel_format=pattern), LaneTracker(**cal)
    try:
        bay.process_batch(raw[:3], annotate=False)
        plain.process_batch(back[:3], annotate=False)
        for _ in bay.process_stream([raw[3:5], raw[5:]], annotate=False):
            pass
        for _ in plain.process_stream([back[3:5], back[5:]], annotate=False):
            pass
        a, b = bay.get_state(), plain.get_state()
        assert a.pop("pixel_format") == pattern
        a.pop("yuv_matrix")
        assert a == b and a["counter"] == 6
        assert plain.get_success_ratio() == (1.0, 6, 6)
        assert fake.touched >= 4
        twin = LaneTracker(**cal, pixel_format=pattern)
        try:
            twin.set_state(bay.get_state())
            assert twin.get_state() == bay.get_state()
        finally:
            twin.close()
    finally:
        bay.close()
        plain.close()


# ---- video.py -------------------------------------------------------------------------------------------------------------------------
def test_raw_bayer_files_need_their_pattern_named(tmp_path, fake, capsys):
    w, h = 18, 6
    frames = np.random.default_rng(1).integers(0, 256, (5, h, w), dtype=np.uint8)
    path = str(tmp_path / "clip.bayer")
    frames.tofile(path)
    with pytest.raises(ValueError, match="--pixel-format bayer_rggb"):
        video.FrameSource(path, size=(w, h))                         # the suffix cannot name the pattern
    with pytest.raises(ValueError):
        video.FrameSource(path, size=(w, h), pixel_format="rgb")
    with pytest.raises(ValueError):
        video.FrameSource(path, pixel_format="bayer_gbrg")           # size is required, as for .rgb
    with pytest.raises(ValueError):
        video.FrameSource(path, size=(w, h + 2), pixel_format="bayer_gbrg")    # not a whole number of frames
    with pytest.raises(ValueError):
        video.FrameSource(path, size=(w // 2, 2 * h), pixel_format="bayer_gbrg")       # an odd width
    with pytest.raises(ValueError):
        video.FrameSource(str(tmp_path / "clip.rgb"), size=(w, h), pixel_format="bayer_gbrg")     # the pattern of a file that is none
    src = video.FrameSource(path, size=(w, h), pixel_format="bayer_gbrg")
    assert (src.pixel_format, len(src), src.size) == ("bayer_gbrg", 5, (w, h))
    assert np.array_equal(src.read(1, 4), frames[1:4]) and src.read(1, 4).flags["C_CONTIGUOUS"]
    assert np.array_equal(np.stack(list(src)), frames)
    # the command line: two scenes through a raw Bayer tracker; without the flag an error that says so
    cal = calib.reference_calibration()
    utils.save_calibration_npz(str(tmp_path / "cam.npz"), str(tmp_path / "warp.npz"), cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0],
                               cal["warp_matrices"][1], cal["img_size"], cal["warped_size"], *cal["mpp_conversion"])
    clip = str(tmp_path / "scenes.bayer")
    _scene_mosaics("bayer_bggr", 2).tofile(clip)
    args = [clip, "-", "--cam", str(tmp_path / "cam.npz"), "--warp", str(tmp_path / "warp.npz")]
    assert video.main(args + ["--pixel-format", "bayer_bggr"]) == 0
    assert fake.touched >= 1 and "Total frames:  2" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        video.main(args)
    assert "--pixel-format bayer_rggb" in capsys.readouterr().err
