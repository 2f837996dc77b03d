"""10- / 12-bit raw Bayer input ('bayer10_*' / 'bayer12_*': uint16 frames, the sample in the low bits of a 16-bit word, looked up in a
table uint8[4][2**bits] on the device) without a GPU: the name tables and the C boundary's new names; `utils.raw_lut(bits=...)` against a
scalar restatement of its formula; `utils.apply_raw_lut` on wide frames against a per-pixel loop; the wide expression of
`csrc/bayer_arith.h` that both kernels run, compiled for the host (`tests/bayer_wide_host.cpp`, once more under ASan + UBSan: a stand-alone
program) against NumPy; `DeviceFrames` of 16-bit planes; what trackers and groups refuse before any device call; the invariant -- a wide
tracker with table L fed frames F ends where the 8-bit tracker of that pattern without a table fed `apply_raw_lut(F, ., L)` ends -- on the
CPU stand-in for a context; `video.py` reading `.bayer16` files.

On the commit before this format `pixel_format='bayer12_rggb'` is a ValueError, `_native.BAYER_WIDE_FORMATS` does not exist and
`lt_set_raw_lut_wide` is neither declared nor exported: every test below fails there."""
import ctypes as C
import math
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
PATTERNS = list(RB.PATTERNS)                                      # the 8-bit names, in pattern order
DEPTHS = (10, 12)


def wide_name(pattern, bits):
    return "bayer%d_%s" % (bits, pattern[6:])


WIDE = [wide_name(p, b) for b in DEPTHS for p in PATTERNS]


def random_table(bits, seed):
    """Four independently drawn rows: any mix-up of phases shows."""
    return np.random.default_rng(seed).integers(0, 256, (4, 1 << bits), dtype=np.uint8)


# ---- names ----------------------------------------------------------------------------------------------------------------------------
def test_name_tables():
    assert _native.BAYER_WIDE_FORMATS == {"bayer10_rggb": 32, "bayer10_grbg": 33, "bayer10_gbrg": 34, "bayer10_bggr": 35,
                                          "bayer12_rggb": 48, "bayer12_grbg": 49, "bayer12_gbrg": 50, "bayer12_bggr": 51}
    assert list(_native.BAYER_WIDE_FORMATS) == WIDE
    # the pinned tables are what they were
    assert _native.BAYER_FORMATS == {"bayer_rggb": 16, "bayer_grbg": 17, "bayer_gbrg": 18, "bayer_bggr": 19}
    assert _native.PIXEL_FORMATS == {"rgb": 0, "nv12": 1, "i420": 2}
    assert _native.INPUT_FORMATS == {"rgb": 0, "nv12": 1, "i420": 2, "yuy2": 3, "uyvy": 4}
    assert _native.RGB_FAMILY == {"bgr": 5, "rgba": 6, "bgra": 7}
    with pytest.raises(ValueError):
        _native.pixel_format_id("bayer")
    for name, code in _native.BAYER_WIDE_FORMATS.items():
        bits = int(name[5:7])
        assert _native.pixel_format_id(name) == code and _native.format_name(code) == name
        assert code & 3 == PATTERNS.index("bayer_" + name[8:]) and _native.raw_bits(name) == bits
        assert _native.frame_dtype(name) == np.uint16
        assert _native.frame_shape((8, 6), name) == (6, 8) == _native.input_frame_shape((8, 6), name)
        for size in ((7, 6), (8, 5), (2, 6), (8, 2)):
            with pytest.raises(ValueError, match="even width and height of at least 4"):
                _native.frame_shape(size, name)
        with pytest.raises(ValueError, match="input format only"):
            _native.sink_format_id(name)
        with pytest.raises(ValueError, match="input format only"):
            _native.draw_sink_format_id(name)
        with pytest.raises(ValueError, match="RGB"):
            _native.checked_input_size((16, 12), (8, 6), name)
        assert _native.checked_input_size((8, 6), (8, 6), name) is None
    for name in ("rgb", "nv12", "yuy2", "bgra", "bayer_rggb"):
        assert _native.frame_dtype(name) == np.uint8
    assert _native.raw_bits("bayer_gbrg") == 8 and _native.raw_bits("rgb") == 0
    header = open(os.path.join(ROOT, "include", "lane_tracker_amd.h")).read()
    for p, pattern in enumerate(PATTERNS):
        for bits, base in ((10, 32), (12, 48)):
            assert re.search(r"\bLT_INPUT_BAYER%d_%s\s*=\s*%d\b" % (bits, pattern[6:].upper(), base + p), header), (bits, pattern)


def test_new_names_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "lane_tracker_amd.h")).read()
    assert int(re.search(r"#define LT_ABI_VERSION (\d+)", header).group(1)) == 5 == _native.ABI_VERSION
    lib = _native.load()
    assert lib.lt_abi_version() == 5
    for name in ("lt_set_raw_lut_wide", "lt_get_raw_lut_wide", "lt_raw16_to_rgb"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native._SIGNATURES and name in _native.exported_symbols() and hasattr(lib, name)
    flat = " ".join(header.replace("*", " ").split())
    assert "BITS ABOVE ARE IGNORED" in flat and flat.lower().count("not a per-frame") >= 2      # once for each table call


def test_null_arguments_are_errors_without_a_gpu():
    lib = _native.load()
    table = np.zeros(4 << 12, np.uint8)
    frame, out = np.zeros((4, 4), np.uint16), np.zeros((4, 4, 3), np.uint8)
    assert lib.lt_set_raw_lut_wide(None, table.ctypes.data, 4096) == -1 and b"context" in lib.lt_last_error()
    assert lib.lt_set_raw_lut_wide(None, None, 1024) == -1 and b"context" in lib.lt_last_error()
    assert lib.lt_get_raw_lut_wide(None, table.ctypes.data, 4096) == -1 and b"context" in lib.lt_last_error()
    assert not table.any()
    assert lib.lt_raw16_to_rgb(None, frame.ctypes.data, 4, 4, 48, None, out.ctypes.data) == -1 and b"null" in lib.lt_last_error()


# ---- utils.raw_lut(bits=) ---------------------------------------------------------------------------------------------------------------
def _entry(s, black, white, gain, gamma):
    """The docstring's four steps for one sample, in Python floats (float64)."""
    v = min(max((s - black) / (white - black), 0.0), 1.0)
    v = min(max(v * gain, 0.0), 1.0)
    if gamma == "srgb":
        v = 12.92 * v if v <= 0.0031308 else 1.055 * v ** (1.0 / 2.4) - 0.055
    else:
        v = v ** (1.0 / gamma)
    return int(math.floor(255.0 * v + 0.5))


def _table(bits, black, white, gains, gamma):
    g = list(gains) if len(gains) == 4 else [gains[0], gains[1], gains[1], gains[2]]
    return np.array([[_entry(s, float(black), float(white), float(g[p]), gamma) for s in range(1 << bits)] for p in range(4)], np.uint8)


@pytest.mark.parametrize("bits", DEPTHS)
def test_raw_lut_is_its_formula_at_every_depth(bits):
    top = (1 << bits) - 1
    default = utils.raw_lut(bits=bits)
    assert default.shape == (4, 1 << bits) and default.dtype == np.uint8
    assert np.array_equal(default, _table(bits, 0, top, (1, 1, 1), 1.0))                    # white_level defaults to 2**bits - 1
    assert default[0, 0] == 0 and default[3, top] == 255 and (np.diff(default.astype(int), axis=1) >= 0).all()
    scale = 1 << (bits - 8)
    for black, white, gains, gamma in ((16 * scale, 240 * scale, (1.9, 1, 1.6), "srgb"), (16 * scale, 240 * scale, (1.9, 1.0, 1.05, 1.6), 2.2),
                                       (0, top, (0, 0.5, 2), 0.5), (12.5 * scale, 200.25 * scale, (2.5, 1, 1, 3), "srgb")):
        assert np.array_equal(utils.raw_lut(black, white, gains, gamma, bits=bits), _table(bits, black, white, gains, gamma)), (black, white, gains, gamma)
    assert np.array_equal(utils.raw_lut(64, None, (1, 1, 1), bits=bits), _table(bits, 64, top, (1, 1, 1), 1.0))
    with pytest.raises(ValueError):
        utils.raw_lut(black_level=top, bits=bits)                   # the default white level is not above it


def test_raw_lut_at_eight_bits_is_what_it_was():
    assert np.array_equal(utils.raw_lut(), np.tile(np.arange(256, dtype=np.uint8), (4, 1)))
    for args in ((16, 240, (1.9, 1, 1.6), "srgb"), (0, 255, (0, 0.5, 2), 0.5), (12.5, 200.25, (2.5, 1, 1, 3), 2.2)):
        want = np.array([[_entry(s, float(args[0]), float(args[1]), float((args[2] if len(args[2]) == 4 else (args[2][0], args[2][1], args[2][1], args[2][2]))[p]),
                                 args[3]) for s in range(256)] for p in range(4)], np.uint8)
        assert np.array_equal(utils.raw_lut(*args), want) and np.array_equal(utils.raw_lut(*args, bits=8), want)
    assert np.array_equal(utils.raw_lut(16), utils.raw_lut(16, 255))
    for bits in (9, 14, 16, 0):
        with pytest.raises(ValueError):
            utils.raw_lut(bits=bits)


# ---- utils.apply_raw_lut ------------------------------------------------------------------------------------------------------------------
def _phase_at(pattern, y, x):
    """0: a red site, 3: a blue site, 1: green on a red row, 2: green on a blue row -- from the colours the pattern's name gives."""
    own = RB.colour_at(pattern, y, x)
    if own != 1:
        return 0 if own == 0 else 3
    return 1 if RB.colour_at(pattern, y, x ^ 1) == 0 else 2


def _apply_loop(m, pattern, lut, bits):
    out = np.zeros(m.shape, np.uint8)
    for y in range(m.shape[0]):
        for x in range(m.shape[1]):
            out[y, x] = lut[_phase_at(pattern, y, x)][int(m[y, x]) % (1 << bits)]
    return out


@pytest.mark.parametrize("bits", DEPTHS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_apply_raw_lut_on_wide_frames_is_the_per_pixel_loop(pattern, bits):
    name, lut = wide_name(pattern, bits), random_table(bits, 7 + bits)
    rng = np.random.default_rng(PATTERNS.index(pattern) + bits)
    for h, w in ((4, 4), (6, 8)):
        m = rng.integers(0, 1 << bits, (h, w), dtype=np.uint16)
        got = utils.apply_raw_lut(m, name, lut)
        assert got.dtype == np.uint8 and got.shape == m.shape and np.array_equal(got, _apply_loop(m, pattern, lut, bits))
        high = m | (rng.integers(0, 1 << (16 - bits), (h, w), dtype=np.uint16) << bits)      # the bits above are ignored
        assert (high >> bits).any() and np.array_equal(utils.apply_raw_lut(high, name, lut), got)
        assert np.array_equal(_apply_loop(high, pattern, lut, bits), got)
    stack = rng.integers(0, 1 << 16, (3, 6, 8), dtype=np.uint16)
    assert np.array_equal(utils.apply_raw_lut(stack, name, lut), np.stack([_apply_loop(f, pattern, lut, bits) for f in stack]))
    other = 22 - bits
    for bad in (lut[:3], lut.astype(np.int32), lut.astype(np.float64), lut.reshape(-1), lut.T, random_table(other, 1), random_table(8, 1)):
        with pytest.raises(ValueError):
            utils.apply_raw_lut(stack, name, bad)
    with pytest.raises(ValueError):
        utils.apply_raw_lut(stack.astype(np.uint8), name, lut)                 # 8-bit frames with a wide pattern
    with pytest.raises(ValueError):
        utils.apply_raw_lut(stack, "bayer%d" % bits, lut)
    # ... and what the 8-bit patterns refused they still refuse
    with pytest.raises(ValueError):
        utils.apply_raw_lut(stack, pattern, random_table(8, 1))                # uint16 frames with an 8-bit pattern
    with pytest.raises(ValueError, match=r"\(4, 256\)"):
        utils.apply_raw_lut(stack.astype(np.uint8), pattern, lut)              # a wide table with an 8-bit pattern


# ---- bayer_arith.h on the host --------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(CXX is None, reason="no C++ compiler")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_header_expression_is_numpy(tmp_path, flags):
    """Random 4 x 4 windows of 16-bit sites with every bit of the words drawn (and the all-zero, the all-0xFFFF and the all-(2**bits - 1)
    window) at all four (by & 1, bx & 1) parities x four patterns x both depths: the window placed at a site of those parities in a larger
    mosaic, conditioned by apply_raw_lut, is what the header's expressions give."""
    exe = str(tmp_path / "bayer_wide_host")
    build = subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "lane_tracker_amd", "csrc"),
                            os.path.join(ROOT, "tests", "bayer_wide_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    rng = np.random.default_rng(5)
    for bits in DEPTHS:
        lut = random_table(bits, 11 + bits)
        win = np.concatenate([rng.integers(0, 1 << 16, (61, 4, 4), dtype=np.uint16), np.zeros((1, 4, 4), np.uint16),
                              np.full((1, 4, 4), 0xFFFF, np.uint16), np.full((1, 4, 4), (1 << bits) - 1, np.uint16)])
        lut.tofile(str(tmp_path / "lut.bin"))
        win.astype("<u2").tofile(str(tmp_path / "win.bin"))
        for p, pattern in enumerate(PATTERNS):
            dst = str(tmp_path / ("out%d_%d.bin" % (bits, p)))
            run = subprocess.run([exe, str(p), str(bits), str(tmp_path / "lut.bin"), str(tmp_path / "win.bin"), dst], capture_output=True, text=True,
                                 timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
                                                       UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
            assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
            assert run.stdout.strip() == "ok %d" % len(win)
            got = np.fromfile(dst, "<u4").reshape(len(win), 2, 2, 2, 4)          # window, by & 1, bx & 1, (dword form, site form), row
            got = got.view(np.uint8).reshape(len(win), 2, 2, 2, 4, 4)
            for py in range(2):
                for px in range(2):
                    mosaic = np.zeros((len(win), 6, 6), np.uint16)
                    mosaic[:, py:py + 4, px:px + 4] = win
                    want = utils.apply_raw_lut(mosaic, wide_name(pattern, bits), lut)[:, py:py + 4, px:px + 4]
                    for form in range(2):
                        assert np.array_equal(got[:, py, px, form], want), (bits, pattern, py, px, form)


# ---- DeviceFrames of 16-bit planes --------------------------------------------------------------------------------------------------------
def _cai(ptr, shape, strides, typestr="<u2"):
    return {"version": 3, "typestr": typestr, "shape": shape, "strides": strides, "data": (ptr, False)}


def test_device_frames_of_words():
    W, H = 8, 6
    name = "bayer12_grbg"
    f = np.arange(2 * H * W, dtype=np.uint16).reshape(2, H, W) * 37
    block, surf, size, single = pack_host_frames(f, name, pitch=2 * W + 6, offset=2, fill=0xAB)
    assert size == (W, H) and not single and block.dtype == np.uint8
    pitch = 2 * W + 6
    assert surf["pitch"].tolist() == [pitch, pitch] and surf["plane"][:, 0].tolist() == [2, 2 + H * pitch]
    assert block.size == 2 + 2 * H * pitch - 6
    for k in range(2):
        for y in range(H):
            at = 2 + (k * H + y) * pitch
            assert np.array_equal(block[at:at + 2 * W].view("<u2"), f[k, y])                  # little-endian words, as they lie
            if k * H + y < 2 * H - 1:
                assert (block[at + 2 * W:at + pitch] == 0xAB).all()
    assert (block[:2] == 0xAB).all()
    assert pack_host_frames(f[0], name)[3] and pack_host_frames(f[0], name)[1]["pitch"][0] == 2 * W
    for bad, kw in ((f.astype(np.uint8), {}), (f, dict(pitch=2 * W - 2)), (f, dict(pitch=2 * W + 5)), (f, dict(offset=1)), (f[:, :, :7], {}), (f[:, :5], {})):
        with pytest.raises(ValueError):
            pack_host_frames(bad, name, **kw)
    with pytest.raises(ValueError):
        pack_host_frames(f, "bayer_grbg")                          # uint16 frames in an 8-bit format
    # explicit pointers
    d = DeviceFrames.from_planes([(0x1000,), (0x2000,)], (W, H), name, pitch=2 * W + 6)
    assert len(d) == 2 and d.shape == (2, H, W) and d.surfaces["pitch"].tolist() == [pitch, pitch]
    assert DeviceFrames.from_planes((0x1000,), (W, H), name, pitch=2 * W).single
    for planes, p in (([(0x1001,)], 2 * W), ([(0x1000,)], 2 * W + 1), ([(0x1000,)], 2 * W - 2), ([(0x1000,), (0x2003,)], 2 * W)):
        with pytest.raises(ValueError):
            DeviceFrames.from_planes(planes, (W, H), name, pitch=p)
    # __cuda_array_interface__
    d = DeviceFrames.from_cuda_array(_cai(0x4000, (3, H, W), (H * pitch, pitch, 2)), name)
    assert len(d) == 3 and d.img_size == (W, H) and d.surfaces["pitch"].tolist() == [pitch] * 3
    assert d.surfaces["plane"][:, 0].tolist() == [0x4000 + k * H * pitch for k in range(3)]
    one = DeviceFrames.from_cuda_array(_cai(0x4000, (H, W), None), name)
    assert one.single and one.surfaces["pitch"][0] == 2 * W
    for ai in (_cai(0x4000, (H, W), (pitch, 2), "|u1"), _cai(0x4000, (H, W), (pitch, 2), ">u2"), _cai(0x4000, (H, W), (pitch, 1)),
               _cai(0x4000, (H, W), (pitch, 4)), _cai(0x4000, (H, W), (2 * W - 2, 2)), _cai(0x4000, (H, W), (2 * W + 1, 2)),
               _cai(0x4001, (H, W), (pitch, 2)), _cai(0x4000, (2, H, W), (H * pitch + 1, pitch, 2)), _cai(0x4000, (H, W, 1), None)):
        with pytest.raises(ValueError):
            DeviceFrames.from_cuda_array(ai, name)
    with pytest.raises(ValueError):
        DeviceFrames.from_cuda_array(_cai(0x4000, (H, W), (pitch, 2)), "bayer_grbg")            # '<u2' in an 8-bit format
    with pytest.raises(ValueError, match="input format only"):
        DeviceFrames.empty(2, (W, H), name)
    with pytest.raises(ValueError):
        d.check_for((W, H), "bayer10_grbg")
    d.check_for((W, H), name)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------
class _Ctx(fake_context.FakeContext):
    """The CPU stand-in as a raw Bayer context: uploads take mosaics (n, H, W) -- uint8, or uint16 in a wide layout --, condition them with
    the table that is set at that moment and hold the demosaiced form, as the device context's kernels do.  A wide layout always has a
    table: the tracker hands one over before its first upload."""
    touched = 0

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.layout, self.lut, self.lut_calls = "rgb", None, 0

    def set_input_format(self, pixel_format, matrix="bt601"):
        self.layout = pixel_format

    def set_raw_lut(self, lut):
        bits = _native.raw_bits(self.layout)
        assert bits
        assert (lut is None and bits == 8) or (lut.dtype == np.uint8 and lut.shape == (4, 1 << bits))
        self.lut = None if lut is None else lut.copy()
        self.lut_calls += 1

    def upload_frame_rows(self, frames, first=0, enqueue=False):
        type(self).touched += 1
        if self.layout == "rgb":
            return super().upload_frame_rows(frames, first, enqueue)
        f = np.asarray(frames)
        assert f.dtype == _native.frame_dtype(self.layout)
        f = f.reshape(-1, self.img_h, self.img_w)
        pattern = self.layout
        if self.layout in _native.BAYER_WIDE_FORMATS:
            assert self.lut is not None
            pattern = "bayer_" + self.layout[8:]
        if self.lut is not None:
            f = utils.apply_raw_lut(f, self.layout, self.lut)
        return super().upload_frame_rows(RB.bayer_to_rgb(f, pattern), first, enqueue)
    upload_frames = upload_frame_rows


@pytest.fixture()
def fake(monkeypatch):
    monkeypatch.setattr(_native, "Context", _Ctx)
    _Ctx.touched = 0
    return _Ctx


def test_refusals_come_before_any_device_call():
    cal = calib.reference_calibration()
    W, H = cal["img_size"]

    def no_device(*a, **k):
        raise AssertionError("a device context was created")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_native, "Context", no_device)
        for kind in (LaneTracker, lambda **k: LaneTrackerGroup(2, **k)):
            for bits in DEPTHS:
                name, lut = "bayer%d_rggb" % bits, random_table(bits, 3)
                for bad in (lut[:3], lut.reshape(-1), lut.T, lut.astype(np.int16), lut.astype(np.float32), lut[None], random_table(8, 1),
                            random_table(22 - bits, 1)):
                    with pytest.raises(ValueError, match=r"\(4, %d\)" % (1 << bits)):
                        kind(**cal, pixel_format=name, raw_lut=bad)
                with pytest.raises(ValueError, match=r"\(4, 256\)"):
                    kind(**cal, pixel_format="bayer_rggb", raw_lut=lut)
                with pytest.raises(ValueError, match="raw Bayer"):
                    kind(**cal, pixel_format="rgb", raw_lut=lut)
                with pytest.raises(ValueError, match="RGB"):
                    kind(**cal, pixel_format=name, input_size=(W // 2, H // 2))
            odd = dict(cal, img_size=(W - 1, H))
            with pytest.raises(ValueError, match="even width and height of at least 4"):
                kind(**odd, pixel_format="bayer12_bggr")
            with pytest.raises(ValueError):
                kind(**cal, pixel_format="bayer14_rggb")
            with pytest.raises(ValueError):
                kind(**cal, pixel_format="bayer12")
    for name in ("bayer10_grbg", "bayer12_grbg"):
        with pytest.raises(ValueError, match="RGB, NV12 or I420"):
            LaneTracker._inplace_matrix(type("T", (), dict(_resize_from=None, pixel_format=name))(), "inplace", None)


def test_frames_of_the_other_width_are_refused_not_cast(fake):
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    wide, narrow, rgb = LaneTracker(**cal, pixel_format="bayer12_rggb"), LaneTracker(**cal, pixel_format="bayer_rggb"), LaneTracker(**cal)
    try:
        before = fake.touched
        for t, frames in ((wide, np.zeros((2, H, W), np.uint8)), (narrow, np.zeros((2, H, W), np.uint16)), (rgb, np.zeros((2, H, W, 3), np.uint16))):
            with pytest.raises(ValueError, match="uint"):
                t.process_batch(frames, annotate=False)
            with pytest.raises(ValueError, match="uint"):
                t.process(frames[0])
            with pytest.raises(ValueError, match="uint"):
                for _ in t.process_stream([frames], annotate=False):
                    pass
        with pytest.raises(ValueError):
            wide.process_batch(np.zeros((2, H, W, 3), np.uint16), annotate=False)          # another shape
        assert fake.touched == before
        assert wide.get_state()["pixel_format"] == "bayer12_rggb" and "raw_lut" not in wide.get_state()
    finally:
        wide.close(), narrow.close(), rgb.close()
    g = LaneTrackerGroup(2, **cal, pixel_format="bayer10_gbrg")
    try:
        before = fake.touched
        with pytest.raises(ValueError, match="uint"):
            g.process([np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)], annotate=False)
        assert fake.touched == before
    finally:
        g.close()


def test_set_raw_lut_on_trackers_and_groups(fake):
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    for bits in DEPTHS:
        one, two, default = random_table(bits, 1), utils.raw_lut(64, 960 << (bits - 10), (1.9, 1, 1.6), "srgb", bits=bits), utils.raw_lut(bits=bits)
        t, plain = LaneTracker(**cal, pixel_format="bayer%d_gbrg" % bits, raw_lut=one), LaneTracker(**cal, pixel_format="bayer%d_gbrg" % bits)
        try:
            assert np.array_equal(t.raw_lut, one) and np.array_equal(t._ctx.lut, one)
            assert np.array_equal(plain.raw_lut, default) and np.array_equal(plain._ctx.lut, default)      # None: the default table
            t.raw_lut[0, 0] ^= 1                                   # the property hands out a copy
            assert np.array_equal(t.raw_lut, one)
            t.set_raw_lut(two)
            assert np.array_equal(t.raw_lut, two) and np.array_equal(t._ctx.lut, two)
            for bad in (two[:2], two.astype(np.int32), random_table(8, 2), random_table(22 - bits, 2)):
                with pytest.raises(ValueError):
                    t.set_raw_lut(bad)
            assert np.array_equal(t._ctx.lut, two)
            gen = t.process_stream([np.zeros((2, H, W), np.uint16), np.zeros((1, H, W), np.uint16)], annotate=False)
            next(gen)
            calls = t._ctx.lut_calls
            with pytest.raises(RuntimeError, match="process_stream"):
                t.set_raw_lut(one)
            assert t._ctx.lut_calls == calls and np.array_equal(t.raw_lut, two)
            gen.close()
            t.set_raw_lut(None)                                    # back to the default
            assert np.array_equal(t.raw_lut, default) and np.array_equal(t._ctx.lut, default)
        finally:
            t.close()
            plain.close()
        g = LaneTrackerGroup(2, **cal, pixel_format="bayer%d_bggr" % bits, raw_lut=one)
        try:
            assert np.array_equal(g.raw_lut, one) and np.array_equal(g._ctx.lut, one) and g._ctx.lut_calls == 1
            assert all(np.array_equal(m.raw_lut, one) for m in g.trackers)
            g.set_raw_lut(two)
            assert np.array_equal(g.raw_lut, two) and np.array_equal(g._ctx.lut, two) and all(np.array_equal(m.raw_lut, two) for m in g.trackers)
            with pytest.raises(RuntimeError):
                g.trackers[0].set_raw_lut(one)                     # one table for the whole group
            with pytest.raises(ValueError):
                g.set_raw_lut(two.reshape(-1))
            g.set_raw_lut(None)
            assert np.array_equal(g.raw_lut, default) and np.array_equal(g._ctx.lut, default)
        finally:
            g.close()
        g = LaneTrackerGroup(2, **cal, pixel_format="bayer%d_bggr" % bits)
        try:
            assert np.array_equal(g.raw_lut, default) and np.array_equal(g._ctx.lut, default)
        finally:
            g.close()


def _scene_mosaics(pattern, n):
    r = synth.SceneRenderer()
    return RB.rgb_to_bayer(np.stack([r.render(i)[0] for i in range(n)], 0), pattern)


def _darkened(pattern, n, bits=12, seed=0):
    """Scene mosaics the way a 12-bit sensor delivers them: scaled into the range above a pedestal of 256, noise in the low bits."""
    m = _scene_mosaics(pattern, n).astype(np.uint16)
    return (m * 8 + 256 + np.random.default_rng(seed).integers(0, 8, m.shape, dtype=np.uint16)).astype(np.uint16)


def test_a_wide_tracker_is_the_8_bit_one_fed_the_conditioned_frames(fake):
    """Five scenes mosaiced by sampling the pattern, lifted onto a pedestal as 12-bit samples: a 'bayer12_grbg' tracker with the table that
    undoes it and a plain 'bayer_grbg' tracker fed apply_raw_lut's frames end with equal records and state dicts (apart from the format's
    name); the table changes between two windows on both sides alike."""
    cal = calib.reference_calibration()
    pattern, name = "bayer_grbg", "bayer12_grbg"
    raw = _darkened(pattern, 5)
    one, two = utils.raw_lut(256, 256 + 255 * 8, (1, 1, 1), 1.0, bits=12), utils.raw_lut(256, 256 + 255 * 8, (1.1, 1, 0.9), 1.2, bits=12)
    a, b = LaneTracker(**cal, pixel_format=name, raw_lut=one), LaneTracker(**cal, pixel_format=pattern)
    try:
        a.process_batch(raw[:2], annotate=False)
        b.process_batch(utils.apply_raw_lut(raw[:2], name, one), annotate=False)

        def state(t):
            s = t.get_state()
            assert s.pop("pixel_format") == t.pixel_format and "raw_lut" not in s
            return s
        assert state(a) == state(b)
        a.set_raw_lut(two)
        for _ in a.process_stream([raw[2:4], raw[4:]], annotate=False):
            pass
        cond = utils.apply_raw_lut(raw[2:], name, two)
        for _ in b.process_stream([cond[:2], cond[2:]], annotate=False):
            pass
        sa, sb = state(a), state(b)
        assert sa == sb and sa["counter"] == 5
        assert np.array_equal(a._ctx.download_records(2), b._ctx.download_records(2))
        assert b.get_success_ratio()[1] >= 4                       # the lane was found: the states are not equal for being empty
        assert fake.touched >= 6
    finally:
        a.close()
        b.close()


# ---- video.py -------------------------------------------------------------------------------------------------------------------------------
def test_video_reads_bayer16_files(tmp_path):
    W, H = 8, 6
    f = np.random.default_rng(2).integers(0, 4096, (3, H, W), dtype=np.uint16)
    clip = str(tmp_path / "clip.bayer16")
    f.astype("<u2").tofile(clip)
    src = video.FrameSource(clip, (W, H), pixel_format="bayer12_gbrg")
    assert len(src) == 3 and src.pixel_format == "bayer12_gbrg" and src.size == (W, H)
    got = src.read(0, 3)
    assert got.dtype == np.uint16 and np.array_equal(got, f) and np.array_equal(src.read(1, 2)[0], f[1])
    for kw in (dict(pixel_format=None), dict(pixel_format="bayer_gbrg"), dict(pixel_format="nv12")):
        with pytest.raises(ValueError):
            video.FrameSource(clip, (W, H), **kw)
    with pytest.raises(ValueError):
        video.FrameSource(clip, (W, H + 2), pixel_format="bayer12_gbrg")       # not a whole number of frames
    with pytest.raises(ValueError):
        video.FrameSource(clip, (W + 1, H), pixel_format="bayer12_gbrg")
    with pytest.raises(ValueError):
        video.FrameSource(str(tmp_path / "clip.bayer"), (W, H), pixel_format="bayer12_gbrg")      # a wide name for an 8-bit file


def test_video_cli_hands_the_wide_table_to_the_tracker(tmp_path, fake, capsys):
    cal = calib.reference_calibration()
    utils.save_calibration_npz(str(tmp_path / "cam.npz"), str(tmp_path / "warp.npz"), cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0],
                               cal["warp_matrices"][1], cal["img_size"], cal["warped_size"], *cal["mpp_conversion"])
    clip = str(tmp_path / "scenes.bayer16")
    _darkened("bayer_bggr", 2).astype("<u2").tofile(clip)
    seen = []
    real = _Ctx.set_raw_lut

    def spy(self, lut):
        seen.append(None if lut is None else lut.copy())
        return real(self, lut)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_Ctx, "set_raw_lut", spy)
        args = [clip, "-", "--cam", str(tmp_path / "cam.npz"), "--warp", str(tmp_path / "warp.npz"), "--pixel-format", "bayer12_bggr"]
        assert video.main(args + ["--raw-black-level", "64", "--raw-white-level", "3840", "--raw-gains", "1.9,1,1.6", "--raw-gamma", "srgb"]) == 0
        assert len(seen) == 1 and np.array_equal(seen[0], utils.raw_lut(64, 3840, (1.9, 1, 1.6), "srgb", bits=12))
        assert video.main(args + ["--raw-black-level", "256"]) == 0
        assert len(seen) == 2 and np.array_equal(seen[1], utils.raw_lut(256, 4095, bits=12))          # the white level follows the depth
        assert video.main(args) == 0
        assert len(seen) == 3 and np.array_equal(seen[2], utils.raw_lut(bits=12))                     # no flag: the default table
        for bad in (["--pixel-format", "bayer10_bggr", "--raw-white-level", "0"], ["--pixel-format", "bayer_bggr"], ["--pixel-format", "rgb"]):
            with pytest.raises(SystemExit) as e:
                video.main(args[:-2] + bad)
            assert e.value.code == 2
    capsys.readouterr()
