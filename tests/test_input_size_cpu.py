"""Frames of another size than the calibration's (`input_size=`) without a GPU: the arithmetic of `csrc/resize_arith.h` compiled for
the host and held against `utils._resize_taps` and `oracle.resize_linear` (`tests/resize_arith_host.cpp`, once more under ASan +
UBSan); the new names at the C boundary; what a tracker and a group refuse before any device call; and, on `tests/fake_context.py`,
the state contract -- a tracker with an input size ends with the state dict of a plain tracker fed the resized frames."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fake_context
from lane_tracker_amd import _native, calib, synth, utils, video
from lane_tracker_amd.device import DeviceFrames
from lane_tracker_amd.group import LaneTrackerGroup
from lane_tracker_amd.lane_tracker import LaneTracker
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
NEW_NAMES = ("lt_set_input_size", "lt_get_input_size", "lt_get_input_rows")
BASE = 0x7f0000001000          # a made-up device address: nothing here dereferences it

PAIRS = [(s, d) for s in range(1, 41) for d in range(1, 41)] + [(1080, 720), (2160, 720), (720, 1080), (1081, 719)]


def _image_cases():
    """(sh, sw, dh, dw): small sizes of every kind -- one sample, up- and downscales, equal sizes -- and the long axes of the issue's
    sizes against a short other axis."""
    rng = np.random.default_rng(7)
    cases = [(1, 1, 1, 1), (1, 1, 3, 5), (3, 5, 1, 1), (2, 2, 4, 4), (4, 4, 2, 2), (7, 9, 7, 9), (1, 40, 1, 13), (40, 1, 13, 1)]
    cases += [tuple(int(v) for v in rng.integers(1, 41, 4)) for _ in range(120)]
    cases += [(1080, 7, 720, 5), (5, 1920, 3, 1280), (9, 1081, 6, 719), (2160, 3, 720, 2), (6, 720, 9, 1080)]
    return cases


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """The taps of every pair as utils._resize_taps gives them, and images with oracle.resize_linear's result: the files the host
    program reads, and what it must count."""
    d = tmp_path_factory.mktemp("resize_arith")
    entries = 0
    with open(d / "taps.bin", "wb") as f:
        f.write(np.int32(len(PAIRS)).tobytes())
        for s, n in PAIRS:
            t = np.stack(utils._resize_taps(s, n), 1).astype(np.int32)
            assert t.shape == (n, 4)
            f.write(np.array([s, n], np.int32).tobytes() + t.tobytes())
            entries += n
    runs = sum((n + 1) * (n + 2) // 2 if n <= 40 else 64 for _, n in PAIRS)
    rng = np.random.default_rng(11)
    pixels = 0
    with open(d / "images.bin", "wb") as f:
        cases = _image_cases()
        f.write(np.int32(len(cases)).tobytes())
        for i, (sh, sw, dh, dw) in enumerate(cases):
            img = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
            if i % 7 == 0:
                img[:] = 255 * (i % 2)                                  # the extremes
            want = O.resize_linear(img, (dw, dh))
            assert want.shape == (dh, dw, 3)
            f.write(np.array([sh, sw, dh, dw], np.int32).tobytes() + img.tobytes() + want.tobytes())
            pixels += dh * dw * 3
    return str(d / "taps.bin"), str(d / "images.bin"), "ok %d %d %d" % (entries, runs, pixels)


@pytest.mark.skipif(CXX is None, reason="no C++ compiler")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_taps_blend_and_input_rows_on_the_host(tmp_path, tables, flags):
    exe = str(tmp_path / "resize_arith_host")
    build = subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", os.path.join(ROOT, "lane_tracker_amd", "csrc"),
                            os.path.join(ROOT, "tests", "resize_arith_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe, tables[0], tables[1]], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert run.stdout.strip() == tables[2]


def test_coefficients_sum_to_2048_and_input_rows_of_the_reference_calibration():
    for s, n in PAIRS:
        t0, t1, c0, c1 = utils._resize_taps(s, n)
        assert ((c0 + c1) == 2048).all() and (t1 - t0 <= 1).all() and (np.diff(t0) >= 0).all(), (s, n)
    y0, y1, _, _ = utils._resize_taps(1080, 720)
    assert (int(y0[457]), int(y1[695]) + 1) == (685, 1044)            # rows 457 .. 695 of 720 read source rows 685 .. 1043 of 1080


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------
def test_new_names_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "lane_tracker_amd.h")).read()
    assert int(re.search(r"#define LT_ABI_VERSION (\d+)", header).group(1)) == 5 == _native.ABI_VERSION
    lib = _native.load()
    for name in NEW_NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native._SIGNATURES and name in _native.exported_symbols() and hasattr(lib, name), name
    for method in ("set_input_size", "input_size", "input_rows"):
        assert callable(getattr(_native.Context, method))


def test_null_and_invalid_arguments_are_errors_without_a_gpu():
    lib = _native.load()
    a, b = C.c_int(0), C.c_int(0)
    assert lib.lt_set_input_size(None, 1920, 1080) == -1 and b"context" in lib.lt_last_error()
    assert lib.lt_set_input_size(None, 0, 0) == -1
    assert lib.lt_get_input_size(None, C.byref(a), C.byref(b)) == -1
    assert lib.lt_get_input_rows(None, C.byref(a), C.byref(b)) == -1
    for bad in ((0, 720), (1280, 0), (16385, 720), (1280, 16385), (-1, -1), "1920x1080", (1920,), 1920):
        with pytest.raises(ValueError):
            _native.checked_input_size(bad, (1280, 720))
    assert _native.checked_input_size(None, (1280, 720)) is None
    assert _native.checked_input_size((1280, 720), (1280, 720)) is None                      # the calibration's own size: a plain tracker
    assert _native.checked_input_size((1280, 720), (1280, 720), "nv12") is None
    assert _native.checked_input_size([1920, 1080], (1280, 720)) == (1920, 1080)
    assert _native.checked_input_size((16384, 1), (1280, 720)) == (16384, 1)
    with pytest.raises(ValueError, match="RGB"):
        _native.checked_input_size((1920, 1080), (1280, 720), "nv12")


# ---- the Python layer, no device --------------------------------------------------------------------------------------------------
class _Ctx(fake_context.FakeContext):
    """The CPU stand-in with an input size: uploads take frames of that size and hold their oracle.resize_linear form, as the device
    context holds the resized rows in the slot's camera frame."""
    touched = 0

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.src = None

    def set_input_size(self, size):
        w, h = int(size[0]), int(size[1])
        self.src = None if (w, h) == (self.img_w, self.img_h) else (w, h)

    def set_input_format(self, pixel_format, matrix="bt601"):
        raise AssertionError("an RGB tracker sets no input format")

    def attach_device_frames(self, frames, first=0):
        raise AssertionError("a frame in device memory reached the context")

    def upload_frame_rows(self, frames, first=0, enqueue=False):
        type(self).touched += 1
        if self.src is None:
            return super().upload_frame_rows(frames, first, enqueue)
        f = np.asarray(frames).reshape(-1, self.src[1], self.src[0], 3)
        return super().upload_frame_rows(np.stack([O.resize_linear(q, (self.img_w, self.img_h)) for q in f], 0), first, enqueue)
    upload_frames = upload_frame_rows


@pytest.fixture()
def fake(monkeypatch):
    monkeypatch.setattr(_native, "Context", _Ctx)
    _Ctx.touched = 0
    return _Ctx


def test_everything_out_of_scope_is_refused_before_a_context_call(fake):
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    Wi, Hi = 1920, 1080

    def no_device(*a, **k):
        raise AssertionError("a device context was created")
    for layout in ("nv12", "i420", "yuy2", "uyvy"):
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(_native, "Context", no_device)
            with pytest.raises(ValueError, match="RGB"):
                LaneTracker(**cal, pixel_format=layout, input_size=(Wi, Hi))
            with pytest.raises(ValueError, match="RGB"):
                LaneTrackerGroup(2, **cal, pixel_format=layout, input_size=(Wi, Hi))
            for bad in ((0, 10), (Wi, 16385), (Wi,)):
                with pytest.raises(ValueError):
                    LaneTracker(**cal, input_size=bad)
    with pytest.raises(TypeError):
        LaneTracker(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"], cal["mpp_conversion"],
                    8, 4, 2, False, 0, (Wi, Hi))                                           # keyword only

    t = LaneTracker(**cal, input_size=(Wi, Hi))
    try:
        assert t.input_size == (Wi, Hi) and t._ctx.src == (Wi, Hi) and t._frame_shape == (Hi, Wi, 3)
        host = np.zeros((2, Hi, Wi, 3), np.uint8)
        small = np.zeros((2, H, W, 3), np.uint8)
        feed = DeviceFrames.from_planes([(BASE,), (BASE + 3 * Hi * Wi,)], (Wi, Hi), "rgb", pitch=3 * Wi)
        feed_small = DeviceFrames.from_planes([(BASE,), (BASE + 3 * H * W,)], (W, H), "rgb", pitch=3 * W)
        for frames in (feed, feed_small):                    # frames in device memory
            with pytest.raises(ValueError, match="device memory"):
                t.process_batch(frames, annotate=False)
            with pytest.raises(ValueError, match="device memory"):
                list(t.process_stream([frames], annotate=False))
            with pytest.raises(ValueError, match="device memory"):
                t.process(frames[0])
        for frames in (host, feed):                          # nothing is drawn in place
            with pytest.raises(ValueError, match="inplace"):
                t.process_batch(frames, annotate="inplace")
            with pytest.raises(ValueError, match="inplace"):
                list(t.process_stream([frames], annotate="inplace"))
            with pytest.raises(ValueError, match="inplace"):
                t.process_batch(frames, out="inplace")
            with pytest.raises(ValueError, match="inplace"):
                list(t.process_stream([frames], out="inplace"))
        for bad in (small, np.zeros((2, Hi, Wi), np.uint8), np.zeros((Hi, Wi, 3), np.uint8), np.zeros((2, Hi, Wi + 1, 3), np.uint8)):
            with pytest.raises(ValueError):                  # frames of another shape -- the calibration's own size among them
                t.process_batch(bad, annotate=False)
        for bad in (small[0], host, np.zeros((Hi, Wi), np.uint8), None):
            with pytest.raises(ValueError):
                t.process(bad)
        with pytest.raises(ValueError, match="1280x720"):    # a sink is img_size
            t.process_batch(host, out=DeviceFrames.from_planes([(BASE,), (BASE + 3 * Hi * Wi,)], (Wi, Hi), "rgb", pitch=3 * Wi))
        assert t.counter == 0 and fake.touched == 0
    finally:
        t.close()

    same = LaneTracker(**cal, input_size=(W, H))             # the calibration's own size: today's tracker
    try:
        assert same.input_size == (W, H) and same._resize_from is None and same._ctx.src is None and same._frame_shape == (H, W, 3)
    finally:
        same.close()
    g = LaneTrackerGroup(2, **cal, input_size=(Wi, Hi))
    try:
        assert g.input_size == (Wi, Hi) and g._ctx.src == (Wi, Hi) and all(m.input_size == (Wi, Hi) for m in g.trackers)
        with pytest.raises(ValueError):
            g.process([np.zeros((H, W, 3), np.uint8), None], annotate=False)
        with pytest.raises(ValueError, match="device memory"):
            g.process([feed[0], None], annotate=False)
        with pytest.raises(ValueError, match="inplace"):
            g.process([feed[0], None], out="inplace")
        assert fake.touched == 0
    finally:
        g.close()


def test_state_is_a_plain_trackers_state(fake):
    """Six scenes scaled to 960x540 are the camera's frames: a tracker with input_size=(960, 540) fed them and a plain tracker fed their
    oracle.resize_linear form end with equal state dicts -- no key tells them apart -- and each accepts the other's."""
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    r = synth.SceneRenderer()
    cam = np.stack([O.resize_linear(r.render(i)[0], (960, 540)) for i in range(6)], 0)
    back = np.stack([O.resize_linear(f, (W, H)) for f in cam], 0)
    sized, plain = LaneTracker(**cal, input_size=(960, 540)), LaneTracker(**cal)
    try:
        sized.process_batch(cam[:3], annotate=False)
        plain.process_batch(back[:3], annotate=False)
        for w in sized.process_stream([cam[3:5], cam[5:]], annotate=False):
            pass
        for w in plain.process_stream([back[3:5], back[5:]], annotate=False):
            pass
        a, b = sized.get_state(), plain.get_state()
        assert a == b and "input_size" not in a
        assert a["counter"] == 6 and a["success"] >= 1
        plain.set_state(a)
        sized.set_state(b)
        assert sized.get_state() == plain.get_state() == a
    finally:
        sized.close()
        plain.close()


# ---- video.py -------------------------------------------------------------------------------------------------------------------------
def test_video_cli_sizes_raw_input_with_input_size(tmp_path, fake, capsys):
    cal = calib.reference_calibration()
    utils.save_calibration_npz(str(tmp_path / "cam.npz"), str(tmp_path / "warp.npz"), cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0],
                               cal["warp_matrices"][1], cal["img_size"], cal["warped_size"], *cal["mpp_conversion"])
    r = synth.SceneRenderer()
    clip = np.stack([O.resize_linear(r.render(i)[0], (96, 54)) for i in range(2)], 0)
    path = str(tmp_path / "clip.rgb")
    clip.tofile(path)
    args = [path, "-", "--cam", str(tmp_path / "cam.npz"), "--warp", str(tmp_path / "warp.npz")]
    assert video.main(args + ["--input-size", "96x54"]) == 0
    assert fake.touched >= 1 and "Total frames:  2" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        video.main(args + ["--input-size", "96x54", "--size", "48x27"])
    with pytest.raises(ValueError):                          # without it the file is not a whole number of 1280x720 frames
        video.main(args)
