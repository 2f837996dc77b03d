"""Raw Bayer statistics -- per-colour histograms and the zone sums of an auto-white-balance step (lt_raw_stats) -- without a GPU: the NumPy
definition (utils.raw_stats) against a plain per-site Python loop, the header's expressions (csrc/stats_arith.h) through a stand-alone host
program, plain and under ASan / UBSan, utils.awb_gains on exact means, the C ABI's new name and its NULL handling, the refusals of the
Python layer (before any device call) and the tracker's method over a CPU stand-in.  The device side is tests/test_gpu_raw_stats.py; the
kernels' budget tests/test_raw_stats_isa.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fake_context
from lane_tracker_amd import _native, calib, utils
from lane_tracker_amd.group import LaneTrackerGroup
from lane_tracker_amd.lane_tracker import LaneTracker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
PATTERNS = ("rggb", "grbg", "gbrg", "bggr")
FORMATS = ["bayer_%s" % p for p in PATTERNS] + ["bayer%d%s_%s" % (b, k, p) for b in (10, 12) for k in ("", "p") for p in PATTERNS]
SIZES = ((12, 8), (16, 12))                                # (W, H)
ENC = {"8": 0, "10": 1, "12": 1, "10p": 2, "12p": 3}       # stats_arith.h: ENC_BYTES, ENC_WORDS, ENC_RAW10, ENC_RAW12


def kind_of(fmt):
    return fmt[5:fmt.index("_")] or "8"


def bits_of(fmt):
    return int(kind_of(fmt).rstrip("p"))


def frames_of(fmt, n, w, h, seed):
    """Random frames in `fmt`; 16-bit words with random garbage above the sample's bits."""
    rng = np.random.default_rng(seed)
    bits = bits_of(fmt)
    if bits == 8:
        return rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    if fmt in _native.BAYER_PACKED_FORMATS:
        return utils.pack_raw(rng.integers(0, 1 << bits, (n, h, w)).astype(np.uint16), fmt)
    return rng.integers(0, 65536, (n, h, w)).astype(np.uint16)


def shading_of(bits, seed):
    rng = np.random.default_rng(seed)
    return utils.RawShading(rng.integers(2000, 9000, (4, 3, 4)).astype(np.uint16), rng.integers(0, 1 << (bits - 3), 4).astype(np.int32))


def samples_of(frame, fmt, shading=None):
    """One frame's samples as they enter the raw table, (H, W) Python-int friendly: unpacked, masked, shaded."""
    bits = bits_of(fmt)
    plain = _native.unpacked_format(fmt)
    s = utils.unpack_raw(frame, fmt) if fmt in _native.BAYER_PACKED_FORMATS else np.asarray(frame)
    s = s & ((1 << bits) - 1) if bits > 8 else s
    if shading is not None:
        s = utils.apply_raw_shading(s.astype(np.uint8 if bits == 8 else np.uint16), plain, shading)
    return s.astype(np.int64)


def stats_loop(s, fmt, grid, rows, cols, lo, hi):
    """The issue's definition, site by site and cell by cell, in Python integers."""
    bits, p = bits_of(fmt), PATTERNS.index(fmt[-4:])
    bins = 1 << bits
    (row0, row1), (col0, col1), (gh, gw) = rows, cols, grid
    ncy, ncx = (row1 - row0) // 2, (col1 - col0) // 2
    phase = lambda y, x: 2 * ((y ^ (p >> 1)) & 1) + ((x ^ (p & 1)) & 1)
    hist = [[0] * bins for _ in range(4)]
    count = [[0] * gw for _ in range(gh)]
    total = [[[0] * 4 for _ in range(gw)] for _ in range(gh)]
    v = s.tolist()
    for y in range(row0, row1):
        for x in range(col0, col1):
            hist[phase(y, x)][v[y][x]] += 1
    for cy in range(ncy):
        for cx in range(ncx):
            sites = [(row0 + 2 * cy + dy, col0 + 2 * cx + dx) for dy in (0, 1) for dx in (0, 1)]
            assert sorted(phase(y, x) for y, x in sites) == [0, 1, 2, 3]
            if all(lo[phase(y, x)] <= v[y][x] <= hi[phase(y, x)] for y, x in sites):
                zy, zx = cy * gh // ncy, cx * gw // ncx
                count[zy][zx] += 1
                for y, x in sites:
                    total[zy][zx][phase(y, x)] += v[y][x]
    return np.array(hist, np.uint32), np.array(count, np.uint32), np.array(total, np.uint64)


def cases_for(fmt, w, h):
    """(grid, rows, cols, lo, hi) of one frame size: the three grids; the whole frame, a non-default rectangle and its one-cell-per-zone grid;
    the default bounds, bounds that exclude something per phase, and lo > hi."""
    smax = (1 << bits_of(fmt)) - 1
    full, part = ((0, h), (0, w)), ((2, h - 2), (4, w))
    some = ([smax // 8, smax // 16, 0, smax // 4], [smax, smax - smax // 8, smax - smax // 4, smax - smax // 16])
    out = []
    for rows, cols in (full, part):
        ncy, ncx = (rows[1] - rows[0]) // 2, (cols[1] - cols[0]) // 2
        for grid in ((1, 1), (2, 3), (ncy, ncx)):
            for lo, hi in (([0] * 4, [smax] * 4), some):
                out.append((grid, rows, cols, lo, hi))
    out.append(((2, 2), full[0], full[1], [5, 0, 0, 0], [4, smax, smax, smax]))
    return out


def assert_stats(got, want, where):
    for name, g, w in zip(("hist", "zone_count", "zone_sum"), got[:3], want):
        assert g.dtype == w.dtype and g.shape == w.shape, (where, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), "%s: %s differs at %d places" % (where, name, int((g != w).sum()))


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_the_numpy_definition_is_the_per_site_loop(fmt):
    for w, h in SIZES:
        frames = frames_of(fmt, 2, w, h, seed=len(fmt) + w)
        for shading in (None, shading_of(bits_of(fmt), 3)):
            s = [samples_of(f, fmt, shading) for f in frames]
            for grid, rows, cols, lo, hi in cases_for(fmt, w, h):
                where = "%s %dx%d grid %r rows %r cols %r lo %r shading %s" % (fmt, w, h, grid, rows, cols, lo, shading is not None)
                got = utils.raw_stats(frames, fmt, grid, rows, cols, lo, hi, shading)
                assert got.rows == rows and got.cols == cols and got.hist.shape[0] == 2
                for k in range(2):
                    assert_stats([a[k] for a in got[:3]], stats_loop(s[k], fmt, grid, rows, cols, lo, hi), where)
                one = utils.raw_stats(frames[1], fmt, grid, rows, cols, lo, hi, shading)                  # one frame: no frame axis
                assert_stats(one, [a[1] for a in got[:3]], where)
        # the defaults: the whole frame, an 8 x 8 grid where it fits, every cell valid; one bound for all four phases
        d = utils.raw_stats(frames[0], fmt, grid=(4, 6))
        assert d.rows == (0, h) and d.cols == (0, w) and int(d.zone_count.sum()) == h * w // 4 and int(d.hist.sum()) == h * w
        assert_stats(utils.raw_stats(frames[0], fmt, (1, 1), lo=3, hi=200), utils.raw_stats(frames[0], fmt, (1, 1), lo=[3] * 4, hi=[200] * 4)[:3], fmt)


def test_the_definition_refuses_what_it_cannot_take():
    f = np.zeros((8, 12), np.uint8)
    smax = 255
    for bad in (dict(rows=(1, 8)), dict(rows=(0, 7)), dict(rows=(4, 4)), dict(rows=(6, 2)), dict(rows=(0, 10)), dict(rows=(-2, 4)), dict(cols=(0, 14)),
                dict(cols=(3, 8)), dict(grid=(0, 1)), dict(grid=(1, 65)), dict(grid=(5, 1)), dict(grid=(1, 7)), dict(grid=(2.5, 1)), dict(grid=3),
                dict(lo=-1), dict(hi=smax + 1), dict(lo=[0, 0, 0]), dict(hi=1.5), dict(rows=(0, 4), grid=(3, 1)), dict(rows=(0.5, 4))):
        with pytest.raises(ValueError):
            utils.raw_stats(f, "bayer_rggb", **bad)
    for frames, fmt in ((f.astype(np.uint16), "bayer_rggb"), (f, "bayer12_rggb"), (f[None, None], "bayer_rggb"), (f[:7], "bayer_rggb"), (f, "rgb"),
                        (f, "bayer10p_rggb")):
        with pytest.raises(ValueError):
            utils.raw_stats(frames, fmt, grid=(1, 1))
    assert utils.raw_stats(f, "bayer_rggb", (4, 6)).zone_count.tolist() == [[1] * 6] * 4          # one cell per zone is the limit, and legal


# ---- stats_arith.h on the host ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def stats_host(request, tmp_path_factory):
    if CXX is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("raw_stats_host") / "raw_stats_host")
    build = subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", *request.param, "-I", os.path.join(ROOT, "lane_tracker_amd", "csrc"),
                            os.path.join(ROOT, "tests", "raw_stats_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe


def run_host(exe, tmp, fmt, frame, pitch, grid, rows, cols, lo, hi, shading=None, input_rows=(0, 0)):
    """One case through the host program: the frame's bytes at `pitch`, the plane ending on its last byte.  rows / cols None: zeros, the
    header's defaults."""
    kind, bits, p = kind_of(fmt), bits_of(fmt), PATTERNS.index(fmt[-4:])
    raw = np.ascontiguousarray(frame).view(np.uint8).reshape(frame.shape[0], -1)
    h, rb = raw.shape
    w = rb if kind == "8" else rb // 2 if kind in ("10", "12") else rb * 4 // 5 if kind == "10p" else rb * 2 // 3
    plane = np.full(pitch * (h - 1) + rb, 0x5a, np.uint8)
    np.lib.stride_tricks.as_strided(plane, shape=(h, rb), strides=(pitch, 1))[:] = raw
    r, c = rows or (0, 0), cols or (0, 0)
    head = [ENC[kind], bits, p, h, w, pitch, input_rows[0], input_rows[1], r[0], r[1], c[0], c[1], grid[0], grid[1], *lo, *hi,
            0 if shading is None else 1, *([0] * 4 if shading is None else shading.black.tolist())]
    inp, outp = str(tmp / "case.bin"), str(tmp / "result.bin")
    with open(inp, "wb") as f:
        f.write(np.array(head, np.int32).tobytes() + plane.tobytes())
        if shading is not None:
            f.write(utils.raw_shading_plane(shading, fmt, (w, h)).tobytes())
    run = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (fmt, run.returncode, run.stderr[-3000:])
    out = open(outp, "rb").read()
    bins, zones = 1 << bits, grid[0] * grid[1]
    hist = np.frombuffer(out, np.uint32, 4 * bins).reshape(4, bins)
    count = np.frombuffer(out, np.uint32, zones, 16 * bins).reshape(grid)
    total = np.frombuffer(out, np.uint64, 4 * zones, 16 * bins + 4 * zones).reshape(grid + (4,))
    rect = np.frombuffer(out, np.int32, 4, 16 * bins + 36 * zones).tolist()
    assert len(out) == 16 * bins + 36 * zones + 16
    return hist, count, total, rect


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_header_computes_the_loops_statistics(stats_host, tmp_path, fmt):
    """stats_arith.h -- sample extraction by bytes and out of aligned dwords at all four alignments, shading, phases, validity, zones --
    against the per-site loop: dense planes and a pitch of three bytes more (two for words), with and without a map."""
    step = 2 if kind_of(fmt) in ("10", "12") else 3
    for w, h in SIZES:
        frame = frames_of(fmt, 1, w, h, seed=7 * w + len(fmt))[0]
        rb = frame.view(np.uint8).reshape(h, -1).shape[1]
        for j, (grid, rows, cols, lo, hi) in enumerate(cases_for(fmt, w, h)):
            shading = shading_of(bits_of(fmt), 11) if j % 2 else None
            got = run_host(stats_host, tmp_path, fmt, frame, rb + step * (j % 3 == 1), grid, rows, cols, lo, hi, shading)
            assert got[3] == [rows[0], rows[1], cols[0], cols[1]]
            assert_stats(got, stats_loop(samples_of(frame, fmt, shading), fmt, grid, rows, cols, lo, hi), "%s %dx%d case %d" % (fmt, w, h, j))


def test_the_header_rounds_the_default_rows_inward(stats_host, tmp_path):
    fmt, (w, h) = "bayer_grbg", SIZES[1]
    frame = frames_of(fmt, 1, w, h, seed=1)[0]
    for r0, r1 in ((0, 12), (1, 12), (2, 11), (3, 9), (5, 9)):
        want = ((r0 + 1) & ~1, r1 & ~1)
        assert _native.default_stats_rows((r0, r1)) == want and want[0] >= r0 and want[1] <= r1 and want[0] % 2 == want[1] % 2 == 0
        got = run_host(stats_host, tmp_path, fmt, frame, w, (1, 2), None, None, [0] * 4, [255] * 4, input_rows=(r0, r1))
        assert got[3] == [want[0], want[1], 0, w]
        assert_stats(got, stats_loop(samples_of(frame, fmt), fmt, (1, 2), want, (0, w), [0] * 4, [255] * 4), "run [%d, %d)" % (r0, r1))


# ---- grey world ------------------------------------------------------------------------------------------------------------------------------
def test_awb_gains_of_exact_means_are_exact():
    """mosaic = grey x (1/2, 1, 1, 1/4) + pedestal, every value an integer: the means are exact, and only float division is in play."""
    pedestal = 64
    rng = np.random.default_rng(4)
    grey = 8 * rng.integers(20, 100, (3, 6, 8))                              # per cell, divisible by 2 and 4
    frames = np.empty((3, 12, 16), np.uint16)
    for fmt in ("bayer12_rggb", "bayer12_grbg", "bayer12_gbrg", "bayer12_bggr"):
        p = PATTERNS.index(fmt[-4:])
        for py in range(2):
            for px in range(2):
                ph = 2 * (py ^ (p >> 1)) + (px ^ (p & 1))
                frames[:, py::2, px::2] = grey // (2, 1, 1, 4)[ph] + pedestal
        s = utils.raw_stats(frames, fmt, grid=(2, 4))
        assert int(s.zone_count.sum()) == 3 * 48
        for black in (pedestal, [pedestal] * 4, np.full(4, pedestal)):
            g = utils.awb_gains(s, black)
            assert isinstance(g, tuple) and all(isinstance(v, float) for v in g)
            assert np.allclose(g, (2.0, 1.0, 4.0), rtol=0, atol=1e-12), (fmt, g)
        assert np.allclose(utils.awb_gains(utils.raw_stats(frames[0], fmt, grid=(1, 1)), pedestal), (2.0, 1.0, 4.0), rtol=0, atol=1e-12)
        assert utils.raw_lut(pedestal, 4095, utils.awb_gains(s, pedestal), 1.0, 12).shape == (4, 4096)        # what closes the loop
    # known sums and counts, by hand: 10 cells, sums (100, 400, 400, 50) -> means (10, 40, 40, 5), pedestal 0 and (2, 8, 8, 1)
    hand = utils.RawStats(None, np.array([[4, 6]], np.uint32), np.array([[[40, 160, 160, 20], [60, 240, 240, 30]]], np.uint64), (0, 2), (0, 4))
    assert utils.awb_gains(hand) == (4.0, 1.0, 8.0)
    assert utils.awb_gains(hand, [2, 8, 8, 1]) == (4.0, 1.0, 8.0)
    for bad, black in ((hand._replace(zone_count=np.zeros((1, 2), np.uint32)), 0), (hand, 5), (hand, [0, 0, 40, 0]), (hand, 10)):
        with pytest.raises(ValueError):
            utils.awb_gains(bad, black)
    for black in (1.5, [0, 0], "0"):
        with pytest.raises(ValueError):
            utils.awb_gains(hand, black)
    none = utils.raw_stats(frames[0], "bayer12_rggb", grid=(1, 1), lo=4095, hi=0)
    with pytest.raises(ValueError, match="no valid cell"):
        utils.awb_gains(none)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_lt_raw_stats_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "lane_tracker_amd.h")).read()
    assert re.search(r"\bint\s+lt_raw_stats\(lt_ctx\* ctx, int first_slot, int n, const lt_raw_stats_params\* p", header)
    assert re.search(r"typedef struct lt_raw_stats_params \{[^}]*int32_t lo\[4\], hi\[4\];[^}]*\} lt_raw_stats_params;", header)
    assert "#define LT_ABI_VERSION 5" in header
    assert "lt_raw_stats" in _native._SIGNATURES and "lt_raw_stats" in _native.exported_symbols()
    assert _native.C.sizeof(_native.RawStatsParams) == 14 * 4
    lib = _native.load()
    p = _native.RawStatsParams(0, 0, 0, 0, 1, 1, (_native.C.c_int32 * 4)(0, 0, 0, 0), (_native.C.c_int32 * 4)(255, 255, 255, 255))
    hist, rect = np.full(1024, 7, np.uint32), np.full(4, 7, np.int32)
    assert lib.lt_raw_stats(None, 0, 1, _native.C.byref(p), hist.ctypes.data, None, None, rect.ctypes.data) == -1
    assert b"context" in lib.lt_last_error() and (hist == 7).all() and (rect == 7).all()
    assert lib.lt_raw_stats(None, 0, 0, None, None, None, None, None) == -1
    assert "stats_arith.h" in open(os.path.join(ROOT, "lane_tracker_amd", "csrc", "Makefile")).read()


# ---- the Python layer's refusals --------------------------------------------------------------------------------------------------------------
def test_arguments_are_refused_before_any_device_call():
    size, run = (64, 48), (13, 41)                         # the default rows: [14, 40)
    ok = _native.checked_raw_stats("bayer10_rggb", size, run)
    assert (ok.row0, ok.row1, ok.col0, ok.col1, ok.grid_h, ok.grid_w, list(ok.lo), list(ok.hi)) == (14, 40, 0, 64, 8, 8, [0] * 4, [1023] * 4)
    ok = _native.checked_raw_stats("bayer12p_bggr", size, run, (13, 32), None, (0, 64), 1, [4095, 4094, 4093, 0])
    assert (ok.grid_h, ok.grid_w, list(ok.lo), list(ok.hi)) == (13, 32, [1] * 4, [4095, 4094, 4093, 0])
    ok = _native.checked_raw_stats("bayer_gbrg", size, run, (24, 2), (0, 48), (60, 64))
    assert (ok.row0, ok.row1, ok.col0, ok.col1) == (0, 48, 60, 64)
    for bad in (dict(rows=(15, 40)), dict(rows=(14, 41)), dict(cols=(1, 64)), dict(cols=(0, 63)), dict(rows=(14, 50)), dict(cols=(0, 66)), dict(rows=(20, 20)),
                dict(rows=(-2, 40)), dict(grid=(0, 8)), dict(grid=(8, 0)), dict(grid=(65, 8)), dict(grid=(8, 65)), dict(grid=(14, 8)), dict(grid=(8, 33)),
                dict(rows=(0, 48), cols=(0, 8), grid=(8, 5)), dict(lo=-1), dict(lo=1024), dict(hi=1024), dict(hi=[0, 0, 0, -1]), dict(lo=[0, 0]),
                dict(hi=2.0), dict(grid=8), dict(rows=14)):
        with pytest.raises(ValueError):
            _native.checked_raw_stats("bayer10_rggb", size, run, **bad)
    with pytest.raises(ValueError):
        _native.checked_raw_stats("bayer_rggb", size, run, hi=256)
    for fmt in ("rgb", "nv12", "yuy2", "bgra", "bayer14_rggb"):
        with pytest.raises(ValueError, match="raw"):
            _native.checked_raw_stats(fmt, size, run)


# ---- the tracker over a CPU stand-in ---------------------------------------------------------------------------------------------------------
class _Ctx(fake_context.FakeContext):
    """The CPU stand-in as a raw Bayer context that keeps the mosaics it was handed: `raw_stats` answers with `utils.raw_stats` of what was
    uploaded into the slots, behind the map that is set.  It runs no front end: frames of such a tracker are not processed here."""
    log = []

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.layout, self.lut, self.shading, self.raw = "rgb", None, None, {}

    def set_input_format(self, pixel_format, matrix="bt601"):
        self.layout = pixel_format

    def set_raw_lut(self, lut):
        self.lut = lut

    def set_raw_shading(self, shading):
        self.shading = shading

    def input_rows(self):
        return (401, 719)

    def _put(self, how, frames, first):
        f = np.asarray(frames)
        assert f.dtype == _native.frame_dtype(self.layout) and f.ndim == 3 and first + f.shape[0] <= self.capacity
        type(self).log.append((how, first, f.shape[0]))
        for k in range(f.shape[0]):
            self.raw[first + k] = f[k].copy()

    def upload_frame_rows(self, frames, first=0, enqueue=False):
        if self.layout == "rgb":
            return super().upload_frame_rows(frames, first, enqueue)
        self._put("rows", frames, first)

    def upload_frames(self, frames, first=0):
        if self.layout == "rgb":
            return super().upload_frames(frames, first)
        self._put("frames", frames, first)

    def raw_stats(self, n, first=0, grid=(8, 8), rows=None, cols=None, lo=None, hi=None):
        type(self).log.append(("stats", first, n))
        rows = _native.default_stats_rows(self.input_rows()) if rows is None else rows
        shading = None if self.shading is None else utils.RawShading(self.shading.mesh, self.shading.black)
        plain = _native.unpacked_format(self.layout)
        frames = np.stack([self.raw[first + k] for k in range(n)])
        if plain != self.layout:                           # (a map acts on the unpacked samples)
            frames = utils.unpack_raw(frames, self.layout)
        return utils.raw_stats(frames, plain, grid, rows, cols, lo, hi, shading)


@pytest.fixture()
def fake(monkeypatch):
    monkeypatch.setattr(_native, "Context", _Ctx)
    _Ctx.log = []
    return _Ctx


def test_tracker_raw_stats_over_the_stand_in(fake):
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    rgb = LaneTracker(**cal)
    try:
        for frames in (np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint8)):
            with pytest.raises(ValueError, match="raw Bayer"):
                rgb.raw_stats(frames)
        assert fake.log == []
    finally:
        rgb.close()
    shading = utils.raw_shading(np.linspace(1.0, 1.5, 12).reshape(3, 4), black_level=16, bits=10)
    for fmt, dtype, tail, sh in (("bayer_grbg", np.uint8, (H, W), None), ("bayer10_rggb", np.uint16, (H, W), shading), ("bayer12p_bggr", np.uint8, (H, W * 3 // 2), None)):
        fake.log = []
        t = LaneTracker(**cal, pixel_format=fmt, raw_shading=sh)
        try:
            rng = np.random.default_rng(5)
            frames = rng.integers(0, 256 if dtype == np.uint8 else 1 << 10, (5,) + tail).astype(dtype)
            plain = _native.unpacked_format(fmt)
            unpacked = utils.unpack_raw(frames, fmt) if plain != fmt else frames
            before = t.get_state()
            # the default rectangle: the rows alone go up, in pieces of the context's two slots, and the answer is the definition's
            s = t.raw_stats(frames, grid=(3, 5), lo=1)
            assert fake.log == [("rows", 0, 2), ("stats", 0, 2)] * 2 + [("rows", 0, 1), ("stats", 0, 1)]
            assert s.rows == (402, 718) and s.cols == (0, W) and s.hist.shape[0] == 5
            assert_stats(s, utils.raw_stats(unpacked, plain, (3, 5), (402, 718), None, 1, None, sh)[:3], fmt)
            # rows outside the default run: whole frames; one frame: no frame axis
            fake.log = []
            one = t.raw_stats(frames[3], grid=(2, 2), rows=(0, H), cols=(2, 10))
            assert fake.log == [("frames", 0, 1), ("stats", 0, 1)] and one.hist.ndim == 2 and one.rows == (0, H) and one.cols == (2, 10)
            assert_stats(one, utils.raw_stats(unpacked[3], plain, (2, 2), (0, H), (2, 10), None, None, sh)[:3], fmt)
            assert t._resident is None and t.get_state() == before and t.counter == 0
            assert utils.awb_gains(s) == utils.awb_gains(utils.raw_stats(unpacked, plain, (3, 5), (402, 718), None, 1, None, sh))
            # refusals: before anything is uploaded
            fake.log = []
            for bad in (dict(rows=(401, 719)), dict(grid=(0, 1)), dict(grid=(65, 1)), dict(cols=(0, 4), grid=(1, 3)), dict(hi=1 << 12), dict(lo=-1)):
                with pytest.raises(ValueError):
                    t.raw_stats(frames, **bad)
            for wrong in (frames[:, :-2], frames.astype(np.uint16 if dtype == np.uint8 else np.uint8), np.zeros((H, W, 3), np.uint8), frames[None]):
                with pytest.raises(ValueError):
                    t.raw_stats(wrong)
            # inside an active stream
            t._in_stream = True
            try:
                with pytest.raises(RuntimeError, match="process_stream"):
                    t.raw_stats(frames)
            finally:
                t._in_stream = False
            assert fake.log == [] and t.get_state() == before
        finally:
            t.close()


def test_a_group_member_has_no_statistics_of_its_own(fake):
    cal = calib.reference_calibration()
    g = LaneTrackerGroup(2, **cal, pixel_format="bayer_rggb")
    try:
        with pytest.raises(RuntimeError, match="LaneTrackerGroup"):
            g.trackers[0].raw_stats(np.zeros((cal["img_size"][1], cal["img_size"][0]), np.uint8))
    finally:
        g.close()
