"""Lens-shading correction of raw Bayer input -- a gain that depends on the position in the image, from a mesh (lt_set_raw_shading) --
without a GPU: the NumPy definitions (utils.raw_shading_plane, utils.apply_raw_shading) against plain Python-integer loops,
utils.raw_shading, the refusals (before any device call), the Python layer over the CPU stand-in, the C ABI's new names and their NULL
handling, the header's expressions (csrc/shade_arith.h) under ASan / UBSan, the command line.  The device side is
tests/test_gpu_raw_shading.py; the instruction budget tests/test_raw_shading_isa.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bayer_reference as RB
import test_gpu_raw_shading as GS
import test_raw_color_cpu as RC
from lane_tracker_amd import _native, calib, synth, utils, video
from lane_tracker_amd.group import LaneTrackerGroup
from lane_tracker_amd.lane_tracker import LaneTracker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = RC.CXX
PATTERNS = ("rggb", "grbg", "gbrg", "bggr")
SIZES = ((4, 4), (64, 48), (66, 50))                       # (W, H)
MESHES = ((2, 2), (5, 4), (17, 13), (64, 64))              # (mw, mh)


def name_of(p, bits):
    return "bayer_%s" % PATTERNS[p] if bits == 8 else "bayer%d_%s" % (bits, PATTERNS[p])


def random_map(seed, mw, mh, bits=8, black=None):
    rng = np.random.default_rng(seed)
    smax = (1 << bits) - 1
    b = rng.integers(0, smax + 1, 4) if black is None else np.broadcast_to(black, (4,))
    return utils.RawShading(rng.integers(0, 65536, (4, mh, mw)).astype(np.uint16), np.asarray(b, np.int32))


def const_map(q, mw=3, mh=2, black=0):
    return utils.RawShading(np.full((4, mh, mw), q, np.uint16), np.full(4, black, np.int32))


def frames_of(seed, n, w, h, bits):
    """Uniform random samples; 10 / 12 bits: with random bits above the sample, which everything ignores."""
    rng = np.random.default_rng(seed)
    if bits == 8:
        return rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    return rng.integers(0, 65536, (n, h, w)).astype(np.uint16)


# ---- the definitions --------------------------------------------------------------------------------------------------------------------
def plane_loop(shading, p, w, h):
    """raw_shading_plane in Python integers, as the issue writes it."""
    mesh = shading.mesh.tolist()
    mh, mw = shading.mesh.shape[1:]
    out = np.empty((h, w), np.uint16)
    for y in range(h):
        v = y * (mh - 1) * 256 // (h - 1)
        i = min(v >> 8, mh - 2)
        b = v - (i << 8)
        for x in range(w):
            u = x * (mw - 1) * 256 // (w - 1)
            j = min(u >> 8, mw - 2)
            a = u - (j << 8)
            m = mesh[2 * ((y ^ (p >> 1)) & 1) + ((x ^ (p & 1)) & 1)]
            total = (256 - a) * (256 - b) * m[i][j] + a * (256 - b) * m[i][j + 1] + (256 - a) * b * m[i + 1][j] + a * b * m[i + 1][j + 1] + 32768
            assert 0 <= a <= 256 and 0 <= b <= 256 and total < 1 << 32
            out[y, x] = total >> 16
    return out


def apply_loop(frame, shading, p, bits, gain):
    """apply_raw_shading of one frame in Python integers (>> on a negative int floors, as the definition asks)."""
    smax = (1 << bits) - 1
    black = shading.black.tolist()
    out = np.empty_like(frame)
    g = gain.tolist()
    for y, row in enumerate(frame.tolist()):
        for x, word in enumerate(row):
            s, b = word & smax, black[2 * ((y ^ (p >> 1)) & 1) + ((x ^ (p & 1)) & 1)]
            prod = (s - b) * g[y][x]
            assert abs(prod) < 1 << 31
            out[y, x] = min(max(b + ((prod + 2048) >> 12), 0), smax)
    return out


def test_the_gain_plane_is_the_integer_loop():
    for k, (w, h) in enumerate(SIZES):
        for mw, mh in MESHES:
            s = random_map(10 * k + mw, mw, mh)
            for p in range(4):
                got = utils.raw_shading_plane(s, name_of(p, 8), (w, h))
                assert got.dtype == np.uint16 and got.shape == (h, w)
                assert np.array_equal(got, plane_loop(s, p, w, h)), (w, h, mw, mh, p)
                # the image's corners take the corner nodes' values of their phases
                for y, i in ((0, 0), (h - 1, mh - 1)):
                    for x, j in ((0, 0), (w - 1, mw - 1)):
                        assert got[y, x] == s.mesh[2 * ((y ^ (p >> 1)) & 1) + ((x ^ (p & 1)) & 1), i, j]
    # a constant mesh gives that constant, whatever it is; the plane does not depend on the sample depth
    for q in (0, 1, 4096, 40000, 65535):
        assert (utils.raw_shading_plane(const_map(q, 7, 5), "bayer_grbg", (66, 50)) == q).all()
    s = random_map(3, 5, 4)
    assert np.array_equal(utils.raw_shading_plane(s, "bayer_gbrg", (64, 48)), utils.raw_shading_plane(s, "bayer12_gbrg", (64, 48)))
    with pytest.raises(ValueError, match="pattern"):
        utils.raw_shading_plane(s, "rgb", (64, 48))


@pytest.mark.parametrize("bits", [8, 10, 12])
def test_apply_raw_shading_is_the_integer_loop(bits):
    smax = (1 << bits) - 1
    w, h = 66, 50
    f = frames_of(bits, 2, w, h, bits)
    f[0, :2, :8] = [[0, 1, 2, 3, smax, smax - 1, smax >> 1, 5]] * 2            # both ends of the range under every kind of map
    maps = [random_map(1, 5, 4, bits), random_map(2, 17, 13, bits, black=0), random_map(3, 2, 2, bits, black=smax),
            const_map(65535, black=0), const_map(65535, black=smax), const_map(0, black=smax >> 2), const_map(0, black=0),
            utils.RawShading(np.full((4, 2, 2), 4095, np.uint16), np.array([smax, 0, smax, 7], np.int32))]
    for k, s in enumerate(maps):
        for p in ((k & 3), 3 - (k & 3)):
            name = name_of(p, bits)
            gain = utils.raw_shading_plane(s, name, (w, h))
            got = utils.apply_raw_shading(f, name, s)
            assert got.dtype == f.dtype and got.shape == f.shape
            for n in range(2):
                assert np.array_equal(got[n], apply_loop(f[n], s, p, bits, gain)), (bits, k, p, n)
            assert np.array_equal(utils.apply_raw_shading(f[1], name, s), got[1])            # one frame (H, W)
            assert got.max() <= smax
    # 4096 is the identity: the frames come back as they are (10 / 12 bits: their samples, the bits above them dropped)
    for black in (0, smax, (1, smax, 0, smax >> 1)):
        ident = utils.RawShading(np.full((4, 3, 3), 4096, np.uint16), np.broadcast_to(np.asarray(black, np.int32), (4,)))
        assert np.array_equal(utils.apply_raw_shading(f, name_of(1, bits), ident), f & smax)
    # samples below the pedestal: the product is negative and the shift floors -- (-1 * 4095 + 2048) >> 12 = -1, not 0
    s = utils.RawShading(np.full((4, 2, 2), 4095, np.uint16), np.full(4, smax, np.int32))
    below = np.full((4, 4), smax - 1, f.dtype)
    assert (utils.apply_raw_shading(below, name_of(0, bits), s) == smax - 1).all()
    s = utils.RawShading(np.full((4, 2, 2), 2047, np.uint16), np.full(4, smax, np.int32))
    assert (utils.apply_raw_shading(below, name_of(0, bits), s) == smax).all()               # (-2047 + 2048) >> 12 = 0: the step is gone
    s = utils.RawShading(np.full((4, 2, 2), 2049, np.uint16), np.full(4, smax, np.int32))
    assert (utils.apply_raw_shading(below, name_of(0, bits), s) == smax - 1).all()           # (-2049 + 2048) >> 12 = -1
    s = utils.RawShading(np.full((4, 2, 2), 2048, np.uint16), np.full(4, smax, np.int32))
    assert (utils.apply_raw_shading(below, name_of(0, bits), s) == smax).all()               # (-2048 + 2048) >> 12 = 0: gone
    # the extremes: gain 65535 of a full-scale sample over black 0 clamps to smax, gain 0 gives the pedestal
    full = np.full((4, 4), smax, f.dtype)
    assert (utils.apply_raw_shading(full, name_of(2, bits), const_map(65535)) == smax).all()
    assert (utils.apply_raw_shading(np.zeros((4, 4), f.dtype), name_of(2, bits), const_map(65535, black=smax)) == 0).all()
    assert (utils.apply_raw_shading(full, name_of(2, bits), const_map(0, black=9)) == 9).all()
    for bad in (f.astype(np.int32), f[0, 0], f.astype(np.uint8 if bits != 8 else np.uint16)):
        with pytest.raises(ValueError):
            utils.apply_raw_shading(bad, name_of(0, bits), maps[0])
    with pytest.raises(ValueError, match="0 \\.\\. %d" % smax):
        utils.apply_raw_shading(f, name_of(0, bits), const_map(4096, black=smax + 1))


def test_raw_shading_rounds_to_q12_and_refuses_bad_input():
    g = np.array([[1.0, 1.5, 2.0], [0.0, 0.00012, 15.9998]])
    s = utils.raw_shading(g)
    assert isinstance(s, utils.RawShading) and s.mesh.dtype == np.uint16 and s.mesh.shape == (4, 2, 3) and s.black.dtype == np.int32
    assert s.mesh[0].tolist() == [[4096, 6144, 8192], [0, 0, 65535]] and (s.mesh == s.mesh[0]).all() and s.black.tolist() == [0, 0, 0, 0]
    assert utils.raw_shading([[1.00012, 1.00013], [1, 1]]).mesh[0, 0].tolist() == [4096, 4097]       # rint(4096.49), rint(4096.53)
    assert utils.raw_shading([[15.99995, 1], [1, 1]]).mesh[0, 0, 0] == 65535                          # (would round to 2^16)
    four = np.stack([g, 1.05 * g / 1.05, g / 2, g / 4])
    s4 = utils.raw_shading(four, black_level=(16, 17, 18, 19), bits=10)
    assert s4.mesh.shape == (4, 2, 3) and s4.mesh[2, 0].tolist() == [2048, 3072, 4096] and s4.black.tolist() == [16, 17, 18, 19]
    assert utils.raw_shading(g, black_level=255).black.tolist() == [255] * 4
    assert utils.raw_shading(g, black_level=4095, bits=12).black.tolist() == [4095] * 4
    assert utils.raw_shading(np.ones((64, 64))).mesh.shape == (4, 64, 64)
    ok = np.ones((3, 3))
    for bad in (np.ones((1, 3)), np.ones((3, 65)), np.ones(5), np.ones((3, 3, 3)), np.ones((4, 1, 2)), np.ones((2, 2, 2, 2)),
                [[16.0, 1], [1, 1]], [[-0.001, 1], [1, 1]], [[np.nan, 1], [1, 1]], [[np.inf, 1], [1, 1]]):
        with pytest.raises(ValueError):
            utils.raw_shading(bad)
    for kw in (dict(black_level=256), dict(black_level=-1), dict(black_level=1024, bits=10), dict(black_level=(1, 2, 3)), dict(black_level=1.5),
               dict(bits=9), dict(bits=16), dict(black_level=(0, 0, 0, 4096), bits=12)):
        with pytest.raises(ValueError):
            utils.raw_shading(ok, **kw)
    # what the device takes is checked as it is, never cast
    good = utils.raw_shading(ok, 3)
    assert utils.checked_raw_shading(good) is not good and np.array_equal(utils.checked_raw_shading(tuple(good)).mesh, good.mesh)
    for bad in (None, good.mesh, (good.mesh.astype(np.float32), good.black), (good.mesh[:3], good.black), (good.mesh[0], good.black),
                (np.ones((4, 1, 2), np.uint16), good.black), (np.ones((4, 2, 65), np.uint16), good.black), (good.mesh, good.black[:3]),
                (good.mesh, good.black.astype(np.float64)), (good.mesh, [0, 0, 0, 256]), (good.mesh, [0, -1, 0, 0])):
        with pytest.raises(ValueError):
            utils.checked_raw_shading(bad)
    assert utils.checked_raw_shading((good.mesh, [0, 0, 0, 256]), 10).black.tolist() == [0, 0, 0, 256]


# ---- the GPU tests' camera-like map ------------------------------------------------------------------------------------------------------
def test_the_vignette_changes_most_samples_and_saturates_few():
    """The camera-like map of tests/test_gpu_raw_shading.py on the frames its tests use, in NumPy alone: a map that changes nothing, or
    saturates everything, shows nothing -- at least half of the samples change and at most half end on either clamp."""
    for kind in GS.KINDS:
        bits = GS.bits_of(kind)
        s, smax = GS.maps(bits)[3][1], (1 << bits) - 1
        for pattern in GS.PATTERNS:
            for size in ("A", "B"):
                fmt, _, pool = GS._kind(pattern, kind, size)
                got = utils.apply_raw_shading(pool, fmt, s)
                changed, clamped = (got != (pool & smax)).mean(), ((got == 0) | (got == smax)).mean()
                print(fmt, size, "changed %.3f clamped %.3f" % (changed, clamped))
                assert changed >= 0.5 and clamped <= 0.5, (fmt, size, changed, clamped)


# ---- the header's expressions, on the host ------------------------------------------------------------------------------------------------
@pytest.mark.skipif(CXX is None, reason="no C++ compiler")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_header_expressions_are_numpy(tmp_path, flags):
    exe = str(tmp_path / "raw_shading_host")
    subprocess.run([CXX, "-std=c++17", *flags, "-I", os.path.join(ROOT, "lane_tracker_amd", "csrc"), os.path.join(ROOT, "tests", "raw_shading_host.cpp"),
                    "-o", exe], check=True, capture_output=True, timeout=300)
    rng = np.random.default_rng(21)
    cases = [(8, 0, (64, 48), random_map(1, 5, 4)), (8, 3, (4, 4), random_map(2, 2, 2)), (8, 1, (1280, 6), random_map(3, 64, 64)),
             (10, 2, (68, 50), random_map(4, 17, 13, 10)), (12, 1, (64, 48), random_map(5, 64, 64, 12)), (12, 0, (8, 4), const_map(65535, black=4095)),
             (12, 3, (8, 4), const_map(65535, black=0)), (8, 2, (8, 4), const_map(0, black=255)), (10, 0, (8, 6), const_map(4096, black=1023))]
    for k, (bits, p, (w, h), s) in enumerate(cases):
        f = frames_of(k, 1, w, h, bits)[0]
        table = rng.integers(0, 256, (4, 1 << bits), dtype=np.uint8)
        mh, mw = s.mesh.shape[1:]
        inp, outp = str(tmp_path / ("in%d.bin" % k)), str(tmp_path / ("out%d.bin" % k))
        with open(inp, "wb") as fh:
            fh.write(np.array([h, w, mw, mh, p, bits], "<i4").tobytes() + s.black.astype("<i4").tobytes() + s.mesh.astype("<u2").tobytes()
                     + f.astype("<u2").tobytes() + table.tobytes())
        r = subprocess.run([exe, inp, outp], capture_output=True, timeout=60)
        assert r.returncode == 0, (k, r.returncode, r.stderr[-600:])
        out = np.fromfile(outp, np.uint8)
        plane, shaded, looked = out[:2 * h * w].view("<u2").reshape(h, w), out[2 * h * w:4 * h * w].view("<u2").reshape(h, w), out[4 * h * w:].reshape(h, w)
        name = name_of(p, bits)
        assert np.array_equal(plane, utils.raw_shading_plane(s, name, (w, h))), k
        want = utils.apply_raw_shading(f, name, s)
        assert np.array_equal(shaded, want), k
        assert np.array_equal(looked, utils.apply_raw_lut(want, name, table)), k


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
NEW = ("lt_set_raw_shading", "lt_get_raw_shading", "lt_get_raw_shading_plane", "lt_raw_to_rgb_shaded")


def test_new_names_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "lane_tracker_amd.h")).read()
    assert int(re.search(r"#define LT_ABI_VERSION (\d+)", header).group(1)) == 5 == _native.ABI_VERSION
    lib = _native.load()
    assert lib.lt_abi_version() == 5
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native._SIGNATURES and name in _native.exported_symbols() and hasattr(lib, name)
    assert [len(_native._SIGNATURES[n][1]) for n in NEW] == [6, 6, 2, 14]
    flat = " ".join(header.replace("*", " ").split())
    assert "LENS SHADING" in flat and flat.lower().count("not a per-frame") >= 4
    assert "+ 2048) >> 12" in flat and "+ 32768) >> 16" in flat                                  # the two formulas
    lists = [flat[m.end():m.end() + 300] for m in re.finditer("Not built:", flat)]                # ... and no list of things not built names it
    assert len(lists) >= 4 and not any("shading correction" in text for text in lists)


def test_null_arguments_are_errors_without_a_gpu():
    lib = _native.load()
    ptr = _native.C.POINTER(_native.C.c_int)
    mesh, black = np.full((4, 2, 2), 4096, np.uint16), np.zeros(4, np.int32)
    frame, out, plane = np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.uint8), np.full((4, 4), 7, np.uint16)
    got = np.array([7, 7, 7], np.int32)
    assert lib.lt_set_raw_shading(None, mesh.ctypes.data, 2, 2, black.ctypes.data, 1) == -1 and b"context" in lib.lt_last_error()
    assert lib.lt_set_raw_shading(None, None, 0, 0, None, 0) == -1 and b"context" in lib.lt_last_error()
    g = got.ctypes.data
    assert lib.lt_get_raw_shading(None, mesh.ctypes.data, _native.C.cast(g, ptr), _native.C.cast(g + 4, ptr), black.ctypes.data, _native.C.cast(g + 8, ptr)) == -1
    assert b"context" in lib.lt_last_error() and got.tolist() == [7, 7, 7] and (mesh == 4096).all()
    assert lib.lt_get_raw_shading_plane(None, plane.ctypes.data) == -1 and b"null" in lib.lt_last_error() and (plane == 7).all()
    assert lib.lt_raw_to_rgb_shaded(None, frame.ctypes.data, 4, 4, 16, None, 0, None, None, mesh.ctypes.data, 2, 2, black.ctypes.data, out.ctypes.data) == -1
    assert b"null" in lib.lt_last_error()
    assert lib.lt_raw_to_rgb_shaded(None, frame.ctypes.data, 4, 4, 16, None, 0, None, None, None, 0, 0, None, out.ctypes.data) == -1      # (no mesh: lt_raw_to_rgb_color's answer)
    assert not out.any()


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------
class _Ctx(RC._Ctx):
    """The colour stage's CPU stand-in with a shading map in front of everything: uploads shade the mosaics with the map that is set at
    that moment, then do what they did."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.shading, self.shading_calls = None, 0

    def set_raw_shading(self, shading):
        assert _native.raw_bits(self.layout)
        assert shading is None or (isinstance(shading, utils.RawShading) and shading.mesh.dtype == np.uint16 and shading.black.dtype == np.int32)
        self.shading = shading
        self.shading_calls += 1

    def upload_frame_rows(self, frames, first=0, enqueue=False):
        if self.shading is not None:
            frames = utils.apply_raw_shading(np.asarray(frames).reshape(-1, self.img_h, self.img_w), self.layout, self.shading)
        return super().upload_frame_rows(frames, first, enqueue)
    upload_frames = upload_frame_rows


class _OldCtx(RC._OldCtx):
    """A stand-in from before lens shading: it has no set_raw_shading at all."""

    def __getattr__(self, name):
        if name in ("set_raw_shading", "get_raw_shading"):
            raise AssertionError("the shading map's context call was made")
        return super().__getattr__(name)


@pytest.fixture()
def fake(monkeypatch):
    monkeypatch.setattr(_native, "Context", _Ctx)
    _Ctx.touched = 0
    return _Ctx


def vignette(bits=8, mw=17, mh=13):
    """A camera-like map: 1 + 1.5 r^2 (r = 1 in the corners), per colour 1 / 1.05 / 1.05 / 1.1, pedestal 16 (8 bits) or its 10- / 12-bit value."""
    y, x = np.linspace(-1, 1, mh)[:, None], np.linspace(-1, 1, mw)[None, :]
    g = 1 + 1.5 * (x * x + y * y) / 2
    return utils.raw_shading(np.stack([g, 1.05 * g, 1.05 * g, 1.1 * g]), black_level=16 << (bits - 8), bits=bits)


def test_refusals_come_before_any_device_call():
    cal = calib.reference_calibration()
    s = vignette()

    def no_device(*a, **k):
        raise AssertionError("a device context was created")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_native, "Context", no_device)
        for kind in (LaneTracker, lambda **k: LaneTrackerGroup(2, **k)):
            for fmt in ("rgb", "nv12", "yuy2", "bgra"):
                with pytest.raises(ValueError, match="raw Bayer"):
                    kind(**cal, pixel_format=fmt, raw_shading=s)
            for fmt, smax in (("bayer_rggb", 255), ("bayer10_grbg", 1023), ("bayer12_bggr", 4095)):
                with pytest.raises(ValueError, match="0 \\.\\. %d" % smax):
                    kind(**cal, pixel_format=fmt, raw_shading=utils.RawShading(s.mesh, np.array([0, 0, smax + 1, 0], np.int32)))
                for bad in (s.mesh, (s.mesh.astype(np.float32) / 4096, s.black), (s.mesh[:, :1], s.black), (s.mesh[1:], s.black), 1.5):
                    with pytest.raises(ValueError, match="shading"):
                        kind(**cal, pixel_format=fmt, raw_shading=bad)
        with pytest.raises(ValueError):
            utils.bayer_to_rgb_color(np.zeros((4, 4), np.uint8), "bayer_rggb", shading=(s.mesh, [0, 0, 0, 300]))
        with pytest.raises(ValueError, match="pattern"):
            utils.bayer_to_rgb_color(np.zeros((4, 4, 3), np.uint8), "rgb", shading=s)


def test_a_tracker_without_the_keyword_never_calls_the_new_context_method(monkeypatch):
    monkeypatch.setattr(_native, "Context", _OldCtx)
    cal = calib.reference_calibration()
    lut = np.random.default_rng(0).integers(0, 256, (4, 256), dtype=np.uint8)
    made = [LaneTracker(**cal), LaneTracker(**cal, pixel_format="bayer_rggb"), LaneTracker(**cal, pixel_format="bayer_gbrg", raw_lut=lut),
            LaneTracker(**cal, pixel_format="bayer12_rggb"), LaneTrackerGroup(2, **cal), LaneTrackerGroup(2, **cal, pixel_format="bayer10_bggr")]
    try:
        for t in made:
            assert t.raw_shading is None
        made[0].set_raw_shading(None)                             # None on a tracker that takes no map: nothing to ask
        made[4].set_raw_shading(None)
        with pytest.raises(AssertionError, match="context call"):
            made[1].set_raw_shading(vignette())                   # ... and this stand-in does tell
    finally:
        for t in made:
            t.close()


def test_set_raw_shading_on_trackers_and_groups(fake):
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    for fmt, dtype, bits in (("bayer_gbrg", np.uint8, 8), ("bayer12_gbrg", np.uint16, 12)):
        s1, s2 = vignette(bits), random_map(7, 5, 4, bits)
        t, plain = LaneTracker(**cal, pixel_format=fmt, raw_shading=s1), LaneTracker(**cal, pixel_format=fmt)
        try:
            assert np.array_equal(t.raw_shading.mesh, s1.mesh) and np.array_equal(t.raw_shading.black, s1.black)
            assert t._ctx.shading_calls == 1 and np.array_equal(t._ctx.shading.mesh, s1.mesh)
            assert plain.raw_shading is None and plain._ctx.shading is None and plain._ctx.shading_calls == 0
            t.raw_shading.mesh[0, 0, 0] ^= 1                       # the property hands out a copy
            t.raw_shading.black[0] ^= 1
            assert np.array_equal(t.raw_shading.mesh, s1.mesh) and np.array_equal(t.raw_shading.black, s1.black)
            assert "raw_shading" not in t.get_state()              # configuration, not state
            t.set_raw_shading(s2)
            assert np.array_equal(t.raw_shading.mesh, s2.mesh) and np.array_equal(t._ctx.shading.black, s2.black)
            for bad in (s2.mesh, (s2.mesh.astype(np.int32), s2.black), (s2.mesh, s2.black + (1 << bits))):
                with pytest.raises(ValueError):
                    t.set_raw_shading(bad)
            assert np.array_equal(t._ctx.shading.mesh, s2.mesh)
            gen = t.process_stream([np.zeros((2, H, W), dtype), np.zeros((1, H, W), dtype)], annotate=False)
            next(gen)
            calls = t._ctx.shading_calls
            with pytest.raises(RuntimeError, match="process_stream"):
                t.set_raw_shading(s1)
            with pytest.raises(RuntimeError, match="process_stream"):
                t.set_raw_shading(None)
            assert t._ctx.shading_calls == calls and np.array_equal(t.raw_shading.mesh, s2.mesh)
            gen.close()
            t.set_raw_shading(None)
            assert t.raw_shading is None and t._ctx.shading is None and t._ctx.shading_calls == calls + 1
            plain.set_raw_shading(s1)
            assert np.array_equal(plain.raw_shading.mesh, s1.mesh) and plain._ctx.shading_calls == 1
        finally:
            t.close(), plain.close()
        g = LaneTrackerGroup(2, **cal, pixel_format=fmt, raw_shading=s1)
        try:
            assert np.array_equal(g.raw_shading.mesh, s1.mesh) and g._ctx.shading_calls == 1
            assert all(np.array_equal(x.raw_shading.mesh, s1.mesh) for x in g.trackers)
            g.set_raw_shading(s2)
            assert np.array_equal(g.raw_shading.black, s2.black) and all(np.array_equal(x.raw_shading.mesh, s2.mesh) for x in g.trackers)
            with pytest.raises(RuntimeError):
                g.trackers[0].set_raw_shading(s1)                  # one map for the whole group
            with pytest.raises(ValueError):
                g.set_raw_shading(s2.mesh)
            g.set_raw_shading(None)
            assert g.raw_shading is None and g._ctx.shading is None and all(x.raw_shading is None for x in g.trackers)
        finally:
            g.close()
    rgb = LaneTracker(**cal)
    try:
        rgb.set_raw_shading(None)                                  # nothing to do on a tracker that takes no map
        with pytest.raises(ValueError, match="raw Bayer"):
            rgb.set_raw_shading(vignette())
        assert rgb._ctx.shading_calls == 0
    finally:
        rgb.close()


def test_a_tracker_with_a_map_is_the_plain_one_fed_the_shaded_frames(fake):
    cal = calib.reference_calibration()
    r = synth.SceneRenderer()
    pattern = "bayer_grbg"
    mos = RB.rgb_to_bayer(np.stack([r.render(i)[0] for i in range(3)], 0), pattern)
    s = vignette()
    m, c, lut = utils.raw_ccm(RC.CAMERA), utils.raw_curve("srgb"), utils.raw_lut(16, 240, (1.5, 1, 1.3))
    kw = dict(pixel_format=pattern, raw_lut=lut, raw_ccm=m, raw_curve=c)
    t, ref = LaneTracker(**cal, **kw, raw_shading=s), LaneTracker(**cal, **kw)
    try:
        shaded = utils.apply_raw_shading(mos, pattern, s)
        assert (shaded != mos).mean() > 0.5
        got = t.process_batch(mos, annotate=False)
        want = ref.process_batch(shaded, annotate=False)
        assert repr(got) == repr(want)
        assert repr(t.get_state()) == repr(ref.get_state())
    finally:
        t.close(), ref.close()


# ---- video.py -------------------------------------------------------------------------------------------------------------------------------
def test_video_cli_hands_the_map_to_the_tracker(tmp_path, fake, capsys):
    cal = calib.reference_calibration()
    utils.save_calibration_npz(str(tmp_path / "cam.npz"), str(tmp_path / "warp.npz"), cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0],
                               cal["warp_matrices"][1], cal["img_size"], cal["warped_size"], *cal["mpp_conversion"])
    r = synth.SceneRenderer()
    clip = str(tmp_path / "scenes.bayer")
    RB.rgb_to_bayer(np.stack([r.render(i)[0] for i in range(2)], 0), "bayer_bggr").tofile(clip)
    y, x = np.linspace(-1, 1, 13)[:, None], np.linspace(-1, 1, 17)[None, :]
    gains = 1 + 0.75 * (x * x + y * y)
    one, four = str(tmp_path / "one.npy"), str(tmp_path / "four.npy")
    np.save(one, gains)
    np.save(four, np.stack([gains, 1.05 * gains, 1.05 * gains, 1.1 * gains]))
    np.save(str(tmp_path / "big.npy"), np.full((3, 3), 16.0))
    np.save(str(tmp_path / "flat.npy"), np.ones(9))
    seen = []
    real = _Ctx.set_raw_shading

    def spy(self, shading):
        seen.append(shading)
        return real(self, shading)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_Ctx, "set_raw_shading", spy)
        args = [clip, "-", "--cam", str(tmp_path / "cam.npz"), "--warp", str(tmp_path / "warp.npz"), "--pixel-format", "bayer_bggr"]
        assert video.main(args + ["--raw-shading", one]) == 0
        assert len(seen) == 1 and np.array_equal(seen[0].mesh, utils.raw_shading(gains).mesh) and seen[0].black.tolist() == [0] * 4
        assert video.main(args + ["--raw-shading", four, "--raw-black-level", "16"]) == 0
        assert len(seen) == 2 and np.array_equal(seen[1].mesh, utils.raw_shading(np.load(four)).mesh) and seen[1].black.tolist() == [16] * 4
        assert video.main(args) == 0
        assert len(seen) == 2                                      # no flag: no map, no call
        for bad in (["--raw-shading", str(tmp_path / "big.npy")], ["--raw-shading", str(tmp_path / "flat.npy")],
                    ["--raw-shading", str(tmp_path / "missing.npy")], ["--raw-shading", one, "--raw-black-level", "300"]):
            with pytest.raises(SystemExit) as e:
                video.main(args + bad)
            assert e.value.code == 2
    # without a raw format the option is refused, whatever the input is
    rgb_clip = str(tmp_path / "scenes.rgb")
    np.stack([r.render(i)[0] for i in range(2)], 0).tofile(rgb_clip)
    W, H = cal["img_size"]
    base = [rgb_clip, "-", "--cam", str(tmp_path / "cam.npz"), "--warp", str(tmp_path / "warp.npz"), "--size", "%dx%d" % (W, H)]
    for bad in (["--raw-shading", one], ["--pixel-format", "rgb", "--raw-shading", one]):
        with pytest.raises(SystemExit) as e:
            video.main(base + bad)
        assert e.value.code == 2
    assert len(seen) == 2
    capsys.readouterr()
