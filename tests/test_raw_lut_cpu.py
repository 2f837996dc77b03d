"""Raw tables (black level, white balance, tone curve of raw Bayer input as uint8[4][256], looked up on the device) without a GPU:
`utils.raw_lut` against a scalar restatement of its formula; `utils.apply_raw_lut` against a per-pixel loop over
`bayer_reference.colour_at`; the expression of `csrc/bayer_arith.h` that both kernels run, compiled for the host
(`tests/raw_lut_host.cpp`, once more under ASan + UBSan: a stand-alone program) against NumPy; the C boundary's new names; what trackers,
groups and `video.py` refuse before any device call; the invariant -- a tracker with a table fed frames F ends where a plain Bayer
tracker fed `apply_raw_lut(F)` ends -- on the CPU stand-in for a context.

On the commit before raw tables `LaneTracker(..., raw_lut=...)` raises TypeError, `utils.raw_lut` does not exist and `lt_set_raw_lut` is
neither declared nor exported: every test below fails there."""
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
from lane_tracker_amd.group import LaneTrackerGroup
from lane_tracker_amd.lane_tracker import LaneTracker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
PATTERNS = list(RB.PATTERNS)


def permutation_table(seed):
    """Four independent random permutations of 0 .. 255: any mix-up of phases shows."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(256) for _ in range(4)]).astype(np.uint8)


# ---- utils.raw_lut ----------------------------------------------------------------------------------------------------------------
def _entry(s, black, white, gain, gamma):
    """The docstring's four steps for one sample, in Python floats (float64)."""
    v = min(max((s - black) / (white - black), 0.0), 1.0)
    v = min(max(v * gain, 0.0), 1.0)
    if gamma == "srgb":
        v = 12.92 * v if v <= 0.0031308 else 1.055 * v ** (1.0 / 2.4) - 0.055
    else:
        v = v ** (1.0 / gamma)
    return int(math.floor(255.0 * v + 0.5))


def _table(black, white, gains, gamma):
    g = list(gains) if len(gains) == 4 else [gains[0], gains[1], gains[1], gains[2]]
    return np.array([[_entry(s, float(black), float(white), float(g[p]), gamma) for s in range(256)] for p in range(4)], np.uint8)


def test_raw_lut_is_its_formula():
    ident = utils.raw_lut()
    assert ident.shape == (4, 256) and ident.dtype == np.uint8
    assert np.array_equal(ident, np.tile(np.arange(256, dtype=np.uint8), (4, 1)))         # the defaults: the identity
    cases = [(0, 255, (1, 1, 1), 1.0), (16, 240, (1.9, 1, 1.6), "srgb"), (16, 240, (1.9, 1.0, 1.05, 1.6), 2.2), (0, 255, (0, 0.5, 2), 0.5),
             (12.5, 200.25, (2.5, 1, 1, 3), "srgb"), (64, 65, (1, 1, 1), 1.0)]
    for black, white, gains, gamma in cases:
        got = utils.raw_lut(black, white, gains, gamma)
        assert np.array_equal(got, _table(black, white, gains, gamma)), (black, white, gains, gamma)
        assert (np.diff(got.astype(int), axis=1) >= 0).all()                              # monotone for gains >= 0
        # the endpoints: everything at or below black is 0; at or above white, the gain's ceiling
        lo, hi = int(math.floor(black)), int(math.ceil(white))
        assert (got[:, :lo + 1] == 0).all()
        g4 = gains if len(gains) == 4 else (gains[0], gains[1], gains[1], gains[2])
        for p in range(4):
            assert (got[p, hi:] == _entry(255, 0.0, 255.0, g4[p], gamma)).all()
    three, four = utils.raw_lut(16, 240, (1.9, 1, 1.6), "srgb"), utils.raw_lut(16, 240, (1.9, 1, 1, 1.6), "srgb")
    assert np.array_equal(three, four) and np.array_equal(three[1], three[2]) and not np.array_equal(three[0], three[3])
    assert three[1, 240] == 255 and three[1, 16] == 0 and three[1, 128] == _entry(128, 16.0, 240.0, 1.0, "srgb")


def test_raw_lut_refuses_what_is_no_table():
    for kw in (dict(black_level=10, white_level=10), dict(black_level=200, white_level=100), dict(gains=(1, -0.5, 1)), dict(gains=(1, 1)),
               dict(gains=(1, 1, 1, 1, 1)), dict(gamma=0), dict(gamma=-2.2), dict(gamma="linear")):
        with pytest.raises(ValueError):
            utils.raw_lut(**kw)


# ---- utils.apply_raw_lut ----------------------------------------------------------------------------------------------------------
def _phase_at(pattern, y, x):
    """0: a red site, 3: a blue site, 1: green on a red row, 2: green on a blue row -- from the colours the pattern's name gives."""
    own = RB.colour_at(pattern, y, x)
    if own != 1:
        return 0 if own == 0 else 3
    return 1 if RB.colour_at(pattern, y, x ^ 1) == 0 else 2


def _apply_loop(m, pattern, lut):
    out = np.zeros_like(m)
    for y in range(m.shape[0]):
        for x in range(m.shape[1]):
            out[y, x] = lut[_phase_at(pattern, y, x)][m[y, x]]
    return out


@pytest.mark.parametrize("pattern", PATTERNS)
def test_apply_raw_lut_is_the_per_pixel_loop(pattern):
    lut = permutation_table(7)
    rng = np.random.default_rng(PATTERNS.index(pattern))
    for h, w in ((4, 4), (6, 8)):
        m = rng.integers(0, 256, (h, w), dtype=np.uint8)
        got = utils.apply_raw_lut(m, pattern, lut)
        assert got.dtype == np.uint8 and got.shape == m.shape and np.array_equal(got, _apply_loop(m, pattern, lut))
    stack = rng.integers(0, 256, (3, 6, 8), dtype=np.uint8)
    got = utils.apply_raw_lut(stack, pattern, lut)
    assert np.array_equal(got, np.stack([_apply_loop(f, pattern, lut) for f in stack]))
    assert np.array_equal(utils.apply_raw_lut(stack, pattern, utils.raw_lut()), stack)
    for bad in (lut[:3], lut.astype(np.int32), lut.astype(np.float64), lut.reshape(1024), lut.T):
        with pytest.raises(ValueError):
            utils.apply_raw_lut(stack, pattern, bad)
    with pytest.raises(ValueError):
        utils.apply_raw_lut(stack, "rggb", lut)
    with pytest.raises(ValueError):
        utils.apply_raw_lut(stack.astype(np.uint16), pattern, lut)


# ---- bayer_arith.h on the host ----------------------------------------------------------------------------------------------------
@pytest.mark.skipif(CXX is None, reason="no C++ compiler")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_header_expression_is_numpy(tmp_path, flags):
    """Random 4 x 4 windows (and the two extremes) at all four (by & 1, bx & 1) parities x four patterns: the window placed at a site of
    those parities in a larger mosaic, conditioned by apply_raw_lut, is what the header's expression gives."""
    exe = str(tmp_path / "raw_lut_host")
    build = subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "lane_tracker_amd", "csrc"),
                            os.path.join(ROOT, "tests", "raw_lut_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    lut = permutation_table(11)
    rng = np.random.default_rng(5)
    win = np.concatenate([rng.integers(0, 256, (62, 4, 4), dtype=np.uint8), np.zeros((1, 4, 4), np.uint8), np.full((1, 4, 4), 255, np.uint8)])
    lut.tofile(str(tmp_path / "lut.bin"))
    win.tofile(str(tmp_path / "win.bin"))
    for p, pattern in enumerate(PATTERNS):
        dst = str(tmp_path / ("out%d.bin" % p))
        run = subprocess.run([exe, str(p), str(tmp_path / "lut.bin"), str(tmp_path / "win.bin"), dst], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
        assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
        assert run.stdout.strip() == "ok %d" % len(win)
        got = np.fromfile(dst, "<u4").reshape(len(win), 2, 2, 2, 4)          # window, by & 1, bx & 1, (dword form, byte form), row
        got = got.view(np.uint8).reshape(len(win), 2, 2, 2, 4, 4)
        for py in range(2):
            for px in range(2):
                mosaic = np.zeros((len(win), 6, 6), np.uint8)
                mosaic[:, py:py + 4, px:px + 4] = win
                want = utils.apply_raw_lut(mosaic, pattern, lut)[:, py:py + 4, px:px + 4]
                for form in range(2):
                    assert np.array_equal(got[:, py, px, form], want), (pattern, py, px, form)


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------
def test_new_names_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "lane_tracker_amd.h")).read()
    assert int(re.search(r"#define LT_ABI_VERSION (\d+)", header).group(1)) == 5 == _native.ABI_VERSION
    lib = _native.load()
    assert lib.lt_abi_version() == 5
    for name in ("lt_set_raw_lut", "lt_get_raw_lut"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native._SIGNATURES and name in _native.exported_symbols() and hasattr(lib, name)
    for method in ("set_raw_lut", "raw_lut"):
        assert callable(getattr(_native.Context, method))
    assert "not a per-frame call" in " ".join(header.replace("*", " ").split()).lower()         # the header says what kind of call it is


def test_null_context_is_an_error_without_a_gpu():
    lib = _native.load()
    table = np.zeros(1024, np.uint8)
    is_set = C.c_int(7)
    assert lib.lt_set_raw_lut(None, table.ctypes.data) == -1 and b"context" in lib.lt_last_error()
    assert lib.lt_set_raw_lut(None, None) == -1 and b"context" in lib.lt_last_error()
    assert lib.lt_get_raw_lut(None, table.ctypes.data, C.byref(is_set)) == -1 and b"context" in lib.lt_last_error()
    assert is_set.value == 7 and not table.any()


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------
class _Ctx(fake_context.FakeContext):
    """The CPU stand-in as a raw Bayer context with a raw table: uploads take mosaics (n, H, W), condition them with the table that is
    set at that moment and hold the demosaiced form, as the device context's kernels do."""
    touched = 0

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.layout, self.lut, self.lut_calls = "rgb", None, 0

    def set_input_format(self, pixel_format, matrix="bt601"):
        self.layout = pixel_format

    def set_raw_lut(self, lut):
        assert self.layout in RB.PATTERNS
        assert lut is None or (lut.dtype == np.uint8 and lut.shape == (4, 256))
        self.lut = None if lut is None else lut.copy()
        self.lut_calls += 1

    def upload_frame_rows(self, frames, first=0, enqueue=False):
        type(self).touched += 1
        if self.layout == "rgb":
            return super().upload_frame_rows(frames, first, enqueue)
        f = np.asarray(frames).reshape(-1, self.img_h, self.img_w)
        if self.lut is not None:
            f = utils.apply_raw_lut(f, self.layout, self.lut)
        return super().upload_frame_rows(RB.bayer_to_rgb(f, self.layout), first, enqueue)
    upload_frames = upload_frame_rows


@pytest.fixture()
def fake(monkeypatch):
    monkeypatch.setattr(_native, "Context", _Ctx)
    _Ctx.touched = 0
    return _Ctx


def test_refusals_come_before_any_device_call():
    cal = calib.reference_calibration()
    lut = permutation_table(3)

    def no_device(*a, **k):
        raise AssertionError("a device context was created")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_native, "Context", no_device)
        for kind in (LaneTracker, lambda **k: LaneTrackerGroup(2, **k)):
            for fmt in ("rgb", "bgr", "rgba", "nv12", "yuy2"):
                with pytest.raises(ValueError, match="raw Bayer"):
                    kind(**cal, pixel_format=fmt, raw_lut=lut)
            with pytest.raises(ValueError, match="raw Bayer"):
                kind(**cal, raw_lut=lut)
            for bad in (lut[:3], lut.reshape(1024), lut.T, lut.astype(np.int16), lut.astype(np.float32), lut[None], [[0] * 256] * 4):
                with pytest.raises(ValueError, match=r"\(4, 256\)"):
                    kind(**cal, pixel_format="bayer_rggb", raw_lut=bad)
            with pytest.raises(TypeError):
                kind(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"], cal["mpp_conversion"],
                     8, 4, 2, False, 0, lut)                      # keyword only


def test_set_raw_lut_on_trackers_and_groups(fake):
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    one, two = permutation_table(1), utils.raw_lut(16, 240, (1.9, 1, 1.6), "srgb")
    t, rgb = LaneTracker(**cal, pixel_format="bayer_gbrg", raw_lut=one), LaneTracker(**cal)
    try:
        assert np.array_equal(t.raw_lut, one) and np.array_equal(t._ctx.lut, one) and rgb.raw_lut is None and rgb._ctx.lut_calls == 0
        t.raw_lut[0, 0] ^= 1                                       # the property hands out a copy
        assert np.array_equal(t.raw_lut, one)
        t.set_raw_lut(two)
        assert np.array_equal(t.raw_lut, two) and np.array_equal(t._ctx.lut, two)
        for bad in (two[:2], two.astype(np.int32)):
            with pytest.raises(ValueError):
                t.set_raw_lut(bad)
        assert np.array_equal(t._ctx.lut, two)
        with pytest.raises(ValueError, match="raw Bayer"):
            rgb.set_raw_lut(two)
        assert rgb._ctx.lut_calls == 0
        assert "raw_lut" not in t.get_state()                     # configuration, like the format's matrix: not state
        gen = t.process_stream([np.zeros((2, H, W), np.uint8), np.zeros((1, H, W), np.uint8)], annotate=False)
        next(gen)
        calls = t._ctx.lut_calls
        with pytest.raises(RuntimeError, match="process_stream"):
            t.set_raw_lut(one)
        assert t._ctx.lut_calls == calls and np.array_equal(t.raw_lut, two)
        gen.close()
        t.set_raw_lut(None)
        assert t.raw_lut is None and t._ctx.lut is None
    finally:
        t.close()
        rgb.close()
    g = LaneTrackerGroup(2, **cal, pixel_format="bayer_bggr", raw_lut=one)
    try:
        assert np.array_equal(g.raw_lut, one) and np.array_equal(g._ctx.lut, one) and g._ctx.lut_calls == 1
        assert all(np.array_equal(m.raw_lut, one) for m in g.trackers)
        g.set_raw_lut(two)
        assert np.array_equal(g.raw_lut, two) and np.array_equal(g._ctx.lut, two) and all(np.array_equal(m.raw_lut, two) for m in g.trackers)
        with pytest.raises(RuntimeError):
            g.trackers[0].set_raw_lut(one)                         # one table for the whole group
        with pytest.raises(ValueError):
            g.set_raw_lut(two.reshape(1024))
        g.set_raw_lut(None)
        assert g.raw_lut is None and g._ctx.lut is None
    finally:
        g.close()
    plain = LaneTrackerGroup(2, **cal)
    try:
        with pytest.raises(ValueError, match="raw Bayer"):
            plain.set_raw_lut(one)
        assert plain._ctx.lut_calls == 0
    finally:
        plain.close()


def _scene_mosaics(pattern, n):
    r = synth.SceneRenderer()
    return RB.rgb_to_bayer(np.stack([r.render(i)[0] for i in range(n)], 0), pattern)


def test_a_tracker_with_a_table_is_a_plain_one_fed_the_conditioned_frames(fake):
    """Five scenes mosaiced by sampling the pattern, darkened onto a pedestal the way a sensor delivers them: a Bayer tracker with the
    table that undoes it and a plain Bayer tracker fed apply_raw_lut's frames end with equal records and state dicts; the table changes
    between two windows on both sides alike."""
    cal = calib.reference_calibration()
    pattern = "bayer_grbg"
    raw = (_scene_mosaics(pattern, 5) // 2 + 16).astype(np.uint8)
    one, two = utils.raw_lut(16, 143, (1, 1, 1), 1.0), utils.raw_lut(16, 143, (1.1, 1, 0.9), 1.2)
    a, b = LaneTracker(**cal, pixel_format=pattern, raw_lut=one), LaneTracker(**cal, pixel_format=pattern)
    try:
        a.process_batch(raw[:2], annotate=False)
        b.process_batch(utils.apply_raw_lut(raw[:2], pattern, one), annotate=False)
        assert a.get_state() == b.get_state()
        a.set_raw_lut(two)
        for _ in a.process_stream([raw[2:4], raw[4:]], annotate=False):
            pass
        cond = utils.apply_raw_lut(raw[2:], pattern, two)
        for _ in b.process_stream([cond[:2], cond[2:]], annotate=False):
            pass
        sa, sb = a.get_state(), b.get_state()
        assert sa == sb and sa["counter"] == 5 and "raw_lut" not in sa
        assert np.array_equal(a._ctx.download_records(2), b._ctx.download_records(2))
        assert b.get_success_ratio()[1] >= 4                       # the lane was found: the states are not equal for being empty
        assert fake.touched >= 6
    finally:
        a.close()
        b.close()


# ---- video.py -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["--raw-black-level", "16"], ["--raw-white-level", "240"], ["--raw-gains", "1.9,1,1.6"], ["--raw-gamma", "srgb"]])
def test_video_cli_refuses_raw_flags_without_a_bayer_format(tmp_path, capsys, flags):
    def no_device(*a, **k):
        raise AssertionError("a device context was created")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_native, "Context", no_device)
        for fmt in (["--pixel-format", "rgb"], []):
            with pytest.raises(SystemExit) as e:
                video.main([str(tmp_path / "clip.rgb"), "-"] + fmt + flags)
            assert e.value.code == 2 and "bayer" in capsys.readouterr().err
        for bad in (["--raw-gains", "1,2"], ["--raw-gains", "a,b,c"], ["--raw-gamma", "linear"], ["--raw-black-level", "200", "--raw-white-level", "100"]):
            with pytest.raises(SystemExit) as e:
                video.main([str(tmp_path / "clip.bayer"), "-", "--pixel-format", "bayer_rggb"] + bad)
            assert e.value.code == 2
            capsys.readouterr()


def test_video_cli_hands_the_table_to_the_tracker(tmp_path, fake, capsys):
    cal = calib.reference_calibration()
    utils.save_calibration_npz(str(tmp_path / "cam.npz"), str(tmp_path / "warp.npz"), cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0],
                               cal["warp_matrices"][1], cal["img_size"], cal["warped_size"], *cal["mpp_conversion"])
    clip = str(tmp_path / "scenes.bayer")
    _scene_mosaics("bayer_bggr", 2).tofile(clip)
    seen = []
    real = _Ctx.set_raw_lut

    def spy(self, lut):
        seen.append(None if lut is None else lut.copy())
        return real(self, lut)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_Ctx, "set_raw_lut", spy)
        args = [clip, "-", "--cam", str(tmp_path / "cam.npz"), "--warp", str(tmp_path / "warp.npz"), "--pixel-format", "bayer_bggr"]
        assert video.main(args + ["--raw-black-level", "16", "--raw-white-level", "240", "--raw-gains", "1.9,1,1.6", "--raw-gamma", "srgb"]) == 0
        assert len(seen) == 1 and np.array_equal(seen[0], utils.raw_lut(16, 240, (1.9, 1, 1.6), "srgb"))
        assert video.main(args) == 0 and len(seen) == 1            # no flag: no table
    capsys.readouterr()
