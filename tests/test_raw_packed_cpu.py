"""MIPI-packed RAW10 / RAW12 Bayer input ('bayer10p_*' / 'bayer12p_*': one plane of bytes, five for four samples or three for two, unpacked
in the kernels) without a GPU: the name tables, the header's enum values, exports.map and the ABI version; `utils.pack_raw` / `unpack_raw`
against a site-by-site restatement of the definitions; shapes and dtypes at every layer that sizes a frame; what trackers, groups and the
one-shot converters refuse before any device call; the extraction of `csrc/mipi_arith.h` that the kernels run, compiled for the host
(`tests/raw_packed_host.cpp`, plain and under ASan + UBSan: a stand-alone program); the invariant -- a packed tracker fed frames F ends where
the 16-bit tracker of that pattern fed `unpack_raw(F)` ends -- on the CPU stand-in for a context; `video.py` and its command line on
`.bayer10p` / `.bayer12p` files.

On the commit before this format `pixel_format='bayer10p_rggb'` is a ValueError and `utils.pack_raw`, `_native.BAYER_PACKED_FORMATS` and
`csrc/mipi_arith.h` do not exist: every test below fails there."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import test_bayer_wide_cpu as BWC
from lane_tracker_amd import _native, calib, utils, video
from lane_tracker_amd.device import DeviceFrames, pack_host_frames
from lane_tracker_amd.group import LaneTrackerGroup
from lane_tracker_amd.lane_tracker import LaneTracker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
PATTERNS = ("rggb", "grbg", "gbrg", "bggr")
PACKED = ["bayer%dp_%s" % (b, p) for b in (10, 12) for p in PATTERNS]
SIZES = {10: ((64, 48), (68, 50)), 12: ((64, 48), (66, 50))}           # (W, H): row bytes 80 / 85 and 96 / 99


def row_bytes(bits, w):
    return w * 5 // 4 if bits == 10 else w * 3 // 2


# ---- the definitions, site by site ----------------------------------------------------------------------------------------------------------
def pack_site_by_site(f, bits):
    h, w = f.shape
    out = np.zeros((h, row_bytes(bits, w)), np.uint8)
    for y in range(h):
        for x in range(w):
            s = int(f[y, x])
            if bits == 10:
                g, i = divmod(x, 4)
                out[y, 5 * g + i] = s >> 2
                out[y, 5 * g + 4] |= (s & 3) << (2 * i)
            else:
                g, i = divmod(x, 2)
                out[y, 3 * g + i] = s >> 4
                out[y, 3 * g + 2] |= (s & 15) << (4 * i)
    return out


def unpack_site_by_site(p, bits, w):
    h = p.shape[0]
    out = np.zeros((h, w), np.uint16)
    for y in range(h):
        for x in range(w):
            if bits == 10:
                g, i = divmod(x, 4)
                out[y, x] = (int(p[y, 5 * g + i]) << 2) | ((int(p[y, 5 * g + 4]) >> (2 * i)) & 3)
            else:
                g, i = divmod(x, 2)
                out[y, x] = (int(p[y, 3 * g + i]) << 4) | ((int(p[y, 3 * g + 2]) >> (4 * i)) & 15)
    return out


@pytest.mark.parametrize("bits", (10, 12))
def test_pack_and_unpack_are_the_definitions(bits):
    rng = np.random.default_rng(bits)
    top = (1 << bits) - 1
    for w, h in SIZES[bits]:
        low = (1 << (bits - 8)) - 1
        frames = [rng.integers(0, top + 1, (h, w), dtype=np.uint16), np.zeros((h, w), np.uint16), np.full((h, w), top, np.uint16),
                  rng.integers(0, low + 1, (h, w), dtype=np.uint16), (rng.integers(0, 256, (h, w), dtype=np.uint16) << (bits - 8)).astype(np.uint16)]
        for k, f in enumerate(frames):
            for fmt in ("bayer%dp_grbg" % bits, "%dp" % bits):
                p = utils.pack_raw(f, fmt)
                assert p.dtype == np.uint8 and p.shape == (h, row_bytes(bits, w)) and p.flags.c_contiguous
                assert np.array_equal(p, pack_site_by_site(f, bits)), (w, h, k)
                u = utils.unpack_raw(p, fmt)
                assert u.dtype == np.uint16 and u.shape == (h, w) and np.array_equal(u, f)
                assert np.array_equal(u, unpack_site_by_site(p, bits, w))
        stack = np.stack(frames)
        ps = utils.pack_raw(stack, "%dp" % bits)
        assert ps.shape == (len(frames), h, row_bytes(bits, w)) and all(np.array_equal(ps[k], utils.pack_raw(frames[k], "%dp" % bits)) for k in range(len(frames)))
        assert np.array_equal(utils.unpack_raw(ps, "%dp" % bits), stack)
        # any bytes are a packed frame: unpacking and packing again gives them back (no bit is ignored)
        anyb = rng.integers(0, 256, (h, row_bytes(bits, w)), dtype=np.uint8)
        assert np.array_equal(utils.pack_raw(utils.unpack_raw(anyb, "%dp" % bits), "%dp" % bits), anyb)
        assert np.array_equal(utils.unpack_raw(anyb, "%dp" % bits), unpack_site_by_site(anyb, bits, w))
    ok = np.zeros((4, 8), np.uint16)
    for bad, fmt in ((ok.astype(np.uint8), "10p"), (ok[:, :6], "10p"), (ok[:, :7], "12p"), (ok + (1 << bits), "%dp" % bits), (ok[0], "10p"), (ok, "bayer10_rggb"),
                     (ok, "14p"), (ok[None, None], "12p")):
        with pytest.raises(ValueError):
            utils.pack_raw(bad, fmt)
    for bad, fmt in ((np.zeros((4, 10), np.uint16), "10p"), (np.zeros((4, 9), np.uint8), "10p"), (np.zeros((4, 10), np.uint8), "12p"), (np.zeros(10, np.uint8), "10p"),
                     (np.zeros((4, 10), np.uint8), "bayer10_rggb")):
        with pytest.raises(ValueError):
            utils.unpack_raw(bad, fmt)


def test_apply_raw_lut_takes_the_packed_names():
    rng = np.random.default_rng(4)
    for name in PACKED:
        bits = int(name[5:7])
        w, h = SIZES[bits][1]
        f = rng.integers(0, 1 << bits, (2, h, w), dtype=np.uint16)
        lut = BWC.random_table(bits, 7)
        assert np.array_equal(utils.apply_raw_lut(utils.pack_raw(f, name), name, lut), utils.apply_raw_lut(f, _native.unpacked_format(name), lut))
        assert _native.unpacked_format(name) == "bayer%d_%s" % (bits, name[9:]) and _native.unpacked_format("bayer_rggb") == "bayer_rggb"


# ---- names, enum values, exports, ABI ------------------------------------------------------------------------------------------------------
def test_names_enum_values_exports_and_abi():
    assert _native.BAYER_PACKED_FORMATS == {"bayer10p_rggb": 36, "bayer10p_grbg": 37, "bayer10p_gbrg": 38, "bayer10p_bggr": 39,
                                            "bayer12p_rggb": 52, "bayer12p_grbg": 53, "bayer12p_gbrg": 54, "bayer12p_bggr": 55}
    assert list(_native.BAYER_PACKED_FORMATS) == PACKED
    header = open(os.path.join(ROOT, "include", "lane_tracker_amd.h")).read()
    for name, code in _native.BAYER_PACKED_FORMATS.items():
        bits, pat = int(name[5:7]), name[9:]
        assert re.search(r"\bLT_INPUT_BAYER%dP_%s\s*=\s*%d\b" % (bits, pat.upper(), code), header), name
        wide = _native.BAYER_WIDE_FORMATS["bayer%d_%s" % (bits, pat)]
        assert code == wide | 4 and code & 3 == PATTERNS.index(pat) and code & 4                     # the pattern stays layout & 3, bit 2 says packed
        assert _native.pixel_format_id(name) == code and _native.format_name(code) == name and _native.raw_bits(name) == bits
        assert _native.frame_dtype(name) == np.uint8
        assert _native.frame_shape((8, 6), name) == (6, row_bytes(bits, 8)) == _native.input_frame_shape((8, 6), name)
        assert _native.frame_shape((1280, 720), name) == (720, row_bytes(bits, 1280))
        for size in ((7, 6), (8, 5), (2, 6), (8, 2)):
            with pytest.raises(ValueError, match="even width and height of at least 4"):
                _native.frame_shape(size, name)
        if bits == 10:
            with pytest.raises(ValueError, match="multiple of 4"):
                _native.frame_shape((10, 6), name)
        else:
            assert _native.frame_shape((10, 6), name) == (6, 15)
        with pytest.raises(ValueError, match="input format only"):
            _native.sink_format_id(name)
        with pytest.raises(ValueError, match="input format only"):
            _native.draw_sink_format_id(name)
        with pytest.raises(ValueError, match="input format only"):
            DeviceFrames.empty(2, (8, 6), name)
        with pytest.raises(ValueError, match="RGB"):
            _native.checked_input_size((16, 12), (8, 6), name)
    # what was pinned stays what it was
    assert list(_native.BAYER_WIDE_FORMATS.values()) == [32, 33, 34, 35, 48, 49, 50, 51] and _native.frame_dtype("bayer10_rggb") == np.uint16
    assert int(re.search(r"#define LT_ABI_VERSION (\d+)", header).group(1)) == 5 == _native.ABI_VERSION
    lib = _native.load()
    assert lib.lt_abi_version() == 5
    # additive: the layouts travel through the entry points that were there, and the version script exports the lt_ names only
    exports = open(os.path.join(ROOT, "lane_tracker_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*lt_\*;", exports) and re.search(r"local:\s*\*;", exports)
    for fn in ("lt_set_input_format", "lt_set_raw_lut_wide", "lt_set_raw_color", "lt_set_raw_shading", "lt_raw_to_rgb_color", "lt_raw_to_rgb_shaded",
               "lt_attach_device_frames"):
        assert fn in _native.exported_symbols() and hasattr(lib, fn) and re.search(r"\b%s\s*\(" % fn, header)
    flat = " ".join(header.replace("*", " ").split())
    assert "MIPI-PACKED RAW10 / RAW12" in flat and "nothing is masked or ignored" in flat and "bit 2 says packed" in flat


def test_null_arguments_are_errors_without_a_gpu():
    lib = _native.load()
    frame, out = np.zeros((4, 5), np.uint8), np.zeros((4, 4, 3), np.uint8)
    for layout in (36, 52):
        assert lib.lt_raw_to_rgb_color(None, frame.ctypes.data, 4, 4, layout, None, 0, None, None, out.ctypes.data) == -1 and b"null" in lib.lt_last_error()
        assert lib.lt_raw_to_rgb_shaded(None, frame.ctypes.data, 4, 4, layout, None, 0, None, None, None, 0, 0, None, out.ctypes.data) == -1
    assert lib.lt_set_input_format(None, 36, None) == -1 and b"context" in lib.lt_last_error()


# ---- shapes: DeviceFrames of packed planes ---------------------------------------------------------------------------------------------------
def _cai(ptr, shape, strides, typestr="|u1"):
    return {"version": 3, "typestr": typestr, "shape": shape, "strides": strides, "data": (ptr, False)}


@pytest.mark.parametrize("bits", (10, 12))
def test_device_frames_of_packed_planes(bits):
    name = "bayer%dp_grbg" % bits
    W, H = SIZES[bits][1]
    rb = row_bytes(bits, W)
    f = utils.pack_raw(np.random.default_rng(1).integers(0, 1 << bits, (2, H, W), dtype=np.uint16), name)
    pitch = rb + 3                                                    # any byte alignment of plane and pitch
    block, surf, size, single = pack_host_frames(f, name, pitch=pitch, offset=1, fill=0xAB)
    assert size == (W, H) and not single and block.dtype == np.uint8
    assert surf["pitch"].tolist() == [pitch, pitch] and surf["plane"][:, 0].tolist() == [1, 1 + H * pitch]
    assert block.size == 1 + 2 * H * pitch - 3                        # the block ends with the last byte of the last row
    for k in range(2):
        for y in range(H):
            at = 1 + (k * H + y) * pitch
            assert np.array_equal(block[at:at + rb], f[k, y])
            if k * H + y < 2 * H - 1:
                assert (block[at + rb:at + pitch] == 0xAB).all()
    assert pack_host_frames(f[0], name)[3] and pack_host_frames(f[0], name)[1]["pitch"][0] == rb
    for bad, kw in ((f.astype(np.uint16), {}), (f, dict(pitch=rb - 1)), (f[:, :, :rb - 1], {}), (f[:, :H - 1], {}), (f[..., None], {})):
        with pytest.raises(ValueError):
            pack_host_frames(bad, name, **kw)
    d = DeviceFrames.from_planes([(0x1001,), (0x2003,)], (W, H), name, pitch=pitch)
    assert len(d) == 2 and d.shape == (2, H, rb) and d.surfaces["pitch"].tolist() == [pitch, pitch]
    assert DeviceFrames.from_planes((0x1000,), (W, H), name, pitch=rb).single
    with pytest.raises(ValueError, match="below the row"):
        DeviceFrames.from_planes([(0x1000,)], (W, H), name, pitch=rb - 1)
    d = DeviceFrames.from_cuda_array(_cai(0x4001, (3, H, rb), (H * pitch, pitch, 1)), name)
    assert len(d) == 3 and d.img_size == (W, H) and d.surfaces["pitch"].tolist() == [pitch] * 3
    assert d.surfaces["plane"][:, 0].tolist() == [0x4001 + k * H * pitch for k in range(3)]
    one = DeviceFrames.from_cuda_array(_cai(0x4000, (H, rb), None), name)
    assert one.single and one.surfaces["pitch"][0] == rb and one.img_size == (W, H)
    for ai in (_cai(0x4000, (H, rb), (pitch, 1), "<u2"), _cai(0x4000, (H, rb), (pitch, 2)), _cai(0x4000, (H, rb), (rb - 1, 1)), _cai(0x4000, (H, rb - 1), None),
               _cai(0x4000, (H - 1, rb), None), _cai(0x4000, (H, rb, 1), None)):
        with pytest.raises(ValueError):
            DeviceFrames.from_cuda_array(ai, name)
    with pytest.raises(ValueError):
        d.check_for((W, H), "bayer%d_grbg" % bits)
    d.check_for((W, H), name)


# ---- the header's extraction, on the host ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(CXX is None, reason="no C++ compiler")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_header_extraction_is_the_plain_unpack(tmp_path, flags):
    exe = str(tmp_path / "raw_packed_host")
    subprocess.run([CXX, "-std=c++17", *flags, "-I", os.path.join(ROOT, "lane_tracker_amd", "csrc"), os.path.join(ROOT, "tests", "raw_packed_host.cpp"),
                    "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-600:])
    m = re.match(rb"ok (\d+)", r.stdout)
    # every bx of W = 64, 68 (RAW10) and 64, 66, 68 (RAW12) at four alignments and nine rows each: four samples a window at the least
    assert m and int(m.group(1)) >= 4 * 9 * 4 * ((61 + 65) + (61 + 63 + 65))


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------------
class _Ctx(BWC._Ctx):
    """The CPU stand-in as a context that takes MIPI-packed frames too: it unpacks them by the definition and goes on as the 16-bit layout."""

    def upload_frame_rows(self, frames, first=0, enqueue=False):
        if self.layout not in _native.BAYER_PACKED_FORMATS:
            return super().upload_frame_rows(frames, first, enqueue)
        f = np.asarray(frames)
        assert f.dtype == np.uint8
        packed = self.layout
        f = utils.unpack_raw(f.reshape(-1, self.img_h, _native.packed_row_bytes(packed, self.img_w)), packed)
        self.layout = _native.unpacked_format(packed)
        try:
            return super().upload_frame_rows(f, first, enqueue)
        finally:
            self.layout = packed
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
        mp.setattr("lane_tracker_amd.lane_tracker._context_for_module_functions", no_device)
        for kind in (LaneTracker, lambda **k: LaneTrackerGroup(2, **k)):
            for bits in (10, 12):
                name, lut = "bayer%dp_rggb" % bits, BWC.random_table(bits, 3)
                for bad in (lut[:3], lut.reshape(-1), lut.astype(np.int16), BWC.random_table(8, 1), BWC.random_table(22 - bits, 1)):
                    with pytest.raises(ValueError, match=r"\(4, %d\)" % (1 << bits)):
                        kind(**cal, pixel_format=name, raw_lut=bad)
                with pytest.raises(ValueError, match="RGB"):
                    kind(**cal, pixel_format=name, input_size=(W // 2, H // 2))
                with pytest.raises(ValueError, match="even width and height of at least 4"):
                    kind(**dict(cal, img_size=(W - 1, H)), pixel_format=name)
                with pytest.raises(ValueError, match="even width and height of at least 4"):
                    kind(**dict(cal, img_size=(W, H - 1)), pixel_format=name)
                with pytest.raises(ValueError, match="even width and height of at least 4"):
                    kind(**dict(cal, img_size=(W, 2)), pixel_format=name)
                with pytest.raises(ValueError):
                    kind(**cal, pixel_format=name, raw_ccm=np.zeros((3, 3), np.float32))
                with pytest.raises(ValueError):
                    kind(**cal, pixel_format=name, raw_shading=utils.raw_shading(np.ones((4, 4)), black_level=1 << bits, bits=12))
            with pytest.raises(ValueError, match="multiple of 4"):
                kind(**dict(cal, img_size=(W - 2, H)), pixel_format="bayer10p_bggr")
            for wrong in ("bayer14p_rggb", "bayer10p", "bayer8p_rggb", "bayerp_rggb"):
                with pytest.raises(ValueError):
                    kind(**cal, pixel_format=wrong)
        # the one-shot converters: sizes and dtypes before a context is made
        for name in PACKED:
            bits = int(name[5:7])
            per = 5 if bits == 10 else 3
            for bad in (np.zeros((6, 2 * per + 1), np.uint8), np.zeros((5, 2 * per), np.uint8), np.zeros((2, 2 * per), np.uint8), np.zeros((6, 2 * per), np.uint16),
                        np.zeros((6,), np.uint8)):
                with pytest.raises(ValueError):
                    utils.bayer_to_rgb(bad, name)
                with pytest.raises(ValueError):
                    utils.bayer_to_rgb_color(bad, name)
            with pytest.raises(ValueError, match=r"\(4, %d\)" % (1 << bits)):
                utils.bayer_to_rgb(np.zeros((6, 2 * per), np.uint8), name, raw_lut=BWC.random_table(8, 1))
    for name in ("bayer10p_grbg", "bayer12p_grbg"):
        with pytest.raises(ValueError, match="RGB, NV12 or I420"):
            LaneTracker._inplace_matrix(type("T", (), dict(_resize_from=None, pixel_format=name))(), "inplace", None)


def test_frames_of_another_shape_or_dtype_are_refused(fake):
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    for name in ("bayer10p_rggb", "bayer12p_bggr"):
        rb = _native.packed_row_bytes(name, W)
        t = LaneTracker(**cal, pixel_format=name)
        try:
            before = fake.touched
            for frames in (np.zeros((2, H, W), np.uint16), np.zeros((2, H, rb), np.uint16)):
                with pytest.raises(ValueError, match="uint"):
                    t.process_batch(frames, annotate=False)
            for frames in (np.zeros((2, H, W), np.uint8), np.zeros((2, H, rb + 1), np.uint8), np.zeros((2, H - 2, rb), np.uint8)):
                with pytest.raises(ValueError):
                    t.process_batch(frames, annotate=False)
            assert fake.touched == before
            assert t.get_state()["pixel_format"] == name
        finally:
            t.close()


def test_a_packed_tracker_is_the_16_bit_one_fed_the_unpacked_frames(fake):
    cal = calib.reference_calibration()
    for bits, pat in ((10, "grbg"), (12, "bggr")):
        name, wide = "bayer%dp_%s" % (bits, pat), "bayer%d_%s" % (bits, pat)
        raw = (BWC._darkened("bayer_" + pat, 5) >> (12 - bits)).astype(np.uint16)
        packed = utils.pack_raw(raw, name)
        one = utils.raw_lut(256 >> (12 - bits), (256 + 255 * 8) >> (12 - bits), (1, 1, 1), 1.0, bits=bits)
        two = utils.raw_lut(256 >> (12 - bits), (256 + 255 * 8) >> (12 - bits), (1.1, 1, 0.9), 1.2, bits=bits)
        a, b = LaneTracker(**cal, pixel_format=name, raw_lut=one), LaneTracker(**cal, pixel_format=wide, raw_lut=one)
        try:
            assert np.array_equal(a.raw_lut, one) and np.array_equal(a._ctx.lut, one)
            a.process_batch(packed[:2], annotate=False)
            b.process_batch(utils.unpack_raw(packed[:2], name), annotate=False)

            def state(t):
                s = t.get_state()
                assert s.pop("pixel_format") == t.pixel_format
                return s
            assert state(a) == state(b)
            a.set_raw_lut(two), b.set_raw_lut(two)
            for _ in a.process_stream([packed[2:4], packed[4:]], annotate=False):
                pass
            for _ in b.process_stream([raw[2:4], raw[4:]], annotate=False):
                pass
            sa, sb = state(a), state(b)
            assert sa == sb and sa["counter"] == 5
            assert np.array_equal(a._ctx.download_records(2), b._ctx.download_records(2))
            assert b.get_success_ratio()[1] >= 4
        finally:
            a.close()
            b.close()
        g = LaneTrackerGroup(2, **cal, pixel_format=name, raw_lut=one)
        try:
            assert np.array_equal(g.raw_lut, one) and np.array_equal(g._ctx.lut, one)
            g.set_raw_lut(None)
            assert np.array_equal(g.raw_lut, utils.raw_lut(bits=bits)) and np.array_equal(g._ctx.lut, utils.raw_lut(bits=bits))
            before = fake.touched
            with pytest.raises(ValueError, match="uint"):
                g.process([raw[0], raw[1]], annotate=False)        # words handed to a packed group
            assert fake.touched == before
        finally:
            g.close()


# ---- video.py -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", (10, 12))
def test_video_reads_packed_files(tmp_path, bits):
    W, H = 8, 6
    name = "bayer%dp_gbrg" % bits
    f = utils.pack_raw(np.random.default_rng(2).integers(0, 1 << bits, (3, H, W), dtype=np.uint16), name)
    clip = str(tmp_path / ("clip.bayer%dp" % bits))
    f.tofile(clip)
    src = video.FrameSource(clip, (W, H), pixel_format=name)
    assert len(src) == 3 and src.pixel_format == name and src.size == (W, H)
    got = src.read(0, 3)
    assert got.dtype == np.uint8 and np.array_equal(got, f) and np.array_equal(src.read(1, 2)[0], f[1])
    other = "bayer%dp_gbrg" % (22 - bits)
    for kw in (dict(pixel_format=None), dict(pixel_format="bayer_gbrg"), dict(pixel_format="bayer%d_gbrg" % bits), dict(pixel_format=other)):
        with pytest.raises(ValueError):
            video.FrameSource(clip, (W, H), **kw)                  # the suffix names the depth: the format must agree with it
    with pytest.raises(ValueError):
        video.FrameSource(clip, (W, H + 2), pixel_format=name)     # not a whole number of frames
    with pytest.raises(ValueError):
        video.FrameSource(clip, (W + 1, H), pixel_format=name)
    if bits == 10:
        with pytest.raises(ValueError, match="multiple of 4"):
            video.FrameSource(clip, (W + 2, H), pixel_format=name)
    with pytest.raises(ValueError):
        video.FrameSource(str(tmp_path / "clip.bayer16"), (W, H), pixel_format=name)


def test_video_cli_on_a_packed_file(tmp_path, fake, capsys):
    cal = calib.reference_calibration()
    utils.save_calibration_npz(str(tmp_path / "cam.npz"), str(tmp_path / "warp.npz"), cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0],
                               cal["warp_matrices"][1], cal["img_size"], cal["warped_size"], *cal["mpp_conversion"])
    clip = str(tmp_path / "scenes.bayer12p")
    utils.pack_raw(BWC._darkened("bayer_bggr", 2), "12p").tofile(clip)
    seen = []
    real = _Ctx.set_raw_lut

    def spy(self, lut):
        seen.append(None if lut is None else lut.copy())
        return real(self, lut)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_Ctx, "set_raw_lut", spy)
        args = [clip, "-", "--cam", str(tmp_path / "cam.npz"), "--warp", str(tmp_path / "warp.npz"), "--pixel-format", "bayer12p_bggr"]
        assert video.main(args + ["--raw-black-level", "256", "--raw-white-level", "2296"]) == 0
        assert len(seen) == 1 and np.array_equal(seen[0], utils.raw_lut(256, 2296, bits=12))
        out = capsys.readouterr().out
        assert "Frames: 2" in out and "Success absolute:  2" in out
        assert video.main(args) == 0
        assert len(seen) == 2 and np.array_equal(seen[1], utils.raw_lut(bits=12))
        for bad in (["--pixel-format", "bayer10p_bggr"], ["--pixel-format", "bayer12_bggr"], ["--pixel-format", "bayer_bggr"], ["--pixel-format", "rgb"]):
            with pytest.raises(SystemExit) as e:
                video.main(args[:-2] + bad)
            assert e.value.code == 2
