"""The colour stage of raw Bayer input -- a colour-correction matrix and an output curve behind the demosaic (lt_set_raw_color) -- without a
GPU: the NumPy definition against a plain integer loop, utils.raw_ccm / raw_curve, the refusals (before any device call), the Python
layer over the CPU stand-in, the C ABI's new names and their NULL handling, the header's expression under ASan / UBSan, the command line.
The device side is tests/test_gpu_raw_color.py; the instruction budget tests/test_raw_color_isa.py."""
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
IDENT = (np.eye(3) * 1024).astype(np.int16)
PERM = np.array([[0, 1024, 0], [0, 0, 1024], [1024, 0, 0]], np.int16)          # R -> B, G -> R, B -> G
CAMERA = [[1.9, -0.7, -0.2], [-0.3, 1.6, -0.3], [0.0, -0.6, 1.6]]


def random_stage(seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-32768, 32768, (3, 3)).astype(np.int16), rng.integers(0, 256, 256, dtype=np.uint8)


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def _loop(rgb, m, t):
    """apply_raw_color in Python integers (>> on a negative int floors, as the definition asks)."""
    out = np.empty_like(rgb)
    flat, o = rgb.reshape(-1, 3), out.reshape(-1, 3)
    for i, (r, g, b) in enumerate(flat.tolist()):
        for c in range(3):
            v = (int(m[c][0]) * r + int(m[c][1]) * g + int(m[c][2]) * b + 512) >> 10
            o[i, c] = t[min(max(v, 0), 255)]
    return out


def test_apply_raw_color_is_the_integer_loop():
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, (300, 3), dtype=np.uint8)
    px[:4] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 0, 255]]
    curve = rng.integers(0, 256, 256, dtype=np.uint8)
    mats = [random_stage(s)[0] for s in range(6)]
    mats += [np.full((3, 3), -32768, np.int16), np.full((3, 3), 32767, np.int16),
             np.array([[-32768] * 3, [32767] * 3, [1, -1, 0]], np.int16), (rng.integers(-1500, 1500, (3, 3))).astype(np.int16)]
    for m in mats:
        for t in (curve, None):
            want = _loop(px, m, np.arange(256) if t is None else t)
            got = utils.apply_raw_color(px, m, t)
            assert got.dtype == np.uint8 and got.shape == px.shape and np.array_equal(got, want)
    # both clamp ends, and the floor on negative sums: -1 * 1 + 512 >> 10 = 0, -1024 * 1 ... = -1 -> 0; -513 >> 10 = -1
    low = np.array([[-1, 0, 0], [-3, 0, 0], [4, 0, 0]], np.int16)
    assert utils.apply_raw_color(np.array([[255, 0, 0]], np.uint8), low).tolist() == [[0, 0, 1]]
    assert (utils.apply_raw_color(px, np.full((3, 3), -32768, np.int16), curve)[px.any(axis=1)] == curve[0]).all()
    assert (utils.apply_raw_color(px, np.full((3, 3), 32767, np.int16), curve)[px.sum(axis=1) > 8] == curve[255]).all()
    # any leading shape
    frames = rng.integers(0, 256, (2, 4, 6, 3), dtype=np.uint8)
    assert np.array_equal(utils.apply_raw_color(frames, mats[0], curve), _loop(frames, mats[0], curve))
    for bad in (frames.astype(np.int16), frames[..., :2]):
        with pytest.raises(ValueError):
            utils.apply_raw_color(bad)


def test_identity_and_permutation_are_exact():
    x = np.random.default_rng(1).integers(0, 256, (6, 10, 3), dtype=np.uint8)
    ident = np.arange(256, dtype=np.uint8)
    for m, t in ((None, None), (IDENT, None), (None, ident), (IDENT, ident)):
        assert np.array_equal(utils.apply_raw_color(x, m, t), x)
    assert np.array_equal(utils.apply_raw_color(x, PERM), x[..., [1, 2, 0]])
    assert np.array_equal(utils.apply_raw_color(x, PERM)[..., 2], x[..., 0])        # R went to B
    curve = random_stage(2)[1]
    assert np.array_equal(utils.apply_raw_color(x, PERM, curve), curve[x[..., [1, 2, 0]]])


def test_raw_ccm_rounds_and_keeps_row_sums():
    m = utils.raw_ccm(CAMERA)
    assert m.dtype == np.int16 and m.shape == (3, 3)
    assert m.tolist() == [[1946, -717, -205], [-307, 1638, -307], [0, -614, 1638]]
    assert m.sum(axis=1).tolist() == [1024, 1024, 1024]
    plain = utils.raw_ccm(CAMERA, preserve_white=False)
    assert np.array_equal(plain, np.rint(1024 * np.array(CAMERA)).astype(np.int16))
    thirds = [[0.3337, 0.3337, 0.3337], [0.25, 0.5, 0.25], [0.3337, 0.3337, 0.3337]]      # 341.7 -> 342 three times: 1026, not rint(1025.1)
    plain, kept = utils.raw_ccm(thirds, preserve_white=False), utils.raw_ccm(thirds)
    assert plain.tolist() == [[342, 342, 342], [256, 512, 256], [342, 342, 342]]
    assert kept.tolist() == [[341, 342, 342], [256, 512, 256], [342, 342, 341]]           # only the diagonal entry moves
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    assert np.array_equal(utils.apply_raw_color(grey, m), grey)       # grey stays grey
    assert np.array_equal(utils.raw_ccm(np.eye(3)), IDENT)
    rows = [[0.3337, 0.3337, 0.3337], [1.2, -0.1, -0.1], [-2.5, 1.25, 2.2499]]
    q = utils.raw_ccm(rows)
    assert q.sum(axis=1).tolist() == [int(np.rint(1024 * sum(r))) for r in rows]
    assert utils.raw_ccm([[31.9, 0, 0], [0, -32, 0], [0, 0, 1]], preserve_white=False)[1, 1] == -32768
    for bad in (np.eye(4), np.eye(3)[:2], [1, 2, 3], [[np.nan, 0, 0], [0, 1, 0], [0, 0, 1]], [[np.inf, 0, 0], [0, 1, 0], [0, 0, 1]],
                [[32.0, 0, 0], [0, 1, 0], [0, 0, 1]], [[1, 0, 0], [0, -32.01, 0], [0, 0, 1]]):
        with pytest.raises(ValueError):
            utils.raw_ccm(bad)


def test_raw_curve_is_raw_luts_tone_step():
    s = np.arange(256)
    assert np.array_equal(utils.raw_curve(), s) and np.array_equal(utils.raw_curve(1.0), s)
    for gamma in ("srgb", 2.2, 0.5):
        c = utils.raw_curve(gamma)
        assert c.dtype == np.uint8 and c.shape == (256,)
        assert np.array_equal(c, utils.raw_lut(gamma=gamma)[0])       # 8-bit points: s / 255 is raw_lut's v
        assert c[0] == 0 and c[255] == 255 and (np.diff(c.astype(int)) >= 0).all()
    # a 12-bit table's curve at the samples that are 8-bit points: 4095 = 255 * 16 + 15 has none but 0 and full scale; the formula itself
    v = s / 255.0
    want = np.floor(255 * np.where(v <= 0.0031308, 12.92 * v, 1.055 * v ** (1 / 2.4) - 0.055) + 0.5).astype(np.uint8)
    assert np.array_equal(utils.raw_curve("srgb"), want)
    for bad in (0, -1.0, "rec709"):
        with pytest.raises(ValueError):
            utils.raw_curve(bad)


# ---- the header's expression, on the host ------------------------------------------------------------------------------------------------
@pytest.mark.skipif(CXX is None, reason="no C++ compiler")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_header_expression_is_numpy(tmp_path, flags):
    exe = str(tmp_path / "raw_color_host")
    subprocess.run([CXX, "-std=c++17", *flags, "-I", os.path.join(ROOT, "lane_tracker_amd", "csrc"), os.path.join(ROOT, "tests", "raw_color_host.cpp"),
                    "-o", exe], check=True, capture_output=True, timeout=300)
    rng = np.random.default_rng(9)
    px = rng.integers(0, 256, (500, 3), dtype=np.uint8)
    for k, (m, t) in enumerate([random_stage(1), (np.full((3, 3), -32768, np.int16), random_stage(2)[1]),
                                (np.full((3, 3), 32767, np.int16), random_stage(3)[1]), (utils.raw_ccm(CAMERA), utils.raw_curve("srgb"))]):
        inp, outp = str(tmp_path / ("in%d.bin" % k)), str(tmp_path / ("out%d.bin" % k))
        with open(inp, "wb") as f:
            f.write(m.astype("<i2").tobytes() + t.tobytes() + px.tobytes())
        subprocess.run([exe, inp, outp, str(len(px))], check=True, capture_output=True, timeout=60)
        got = np.fromfile(outp, np.uint8).reshape(-1, 3)
        assert np.array_equal(got, utils.apply_raw_color(px, m, t)), k


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
NEW = ("lt_set_raw_color", "lt_get_raw_color", "lt_raw_to_rgb_color")


def test_new_names_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "lane_tracker_amd.h")).read()
    assert int(re.search(r"#define LT_ABI_VERSION (\d+)", header).group(1)) == 5 == _native.ABI_VERSION
    lib = _native.load()
    assert lib.lt_abi_version() == 5
    exports = open(os.path.join(ROOT, "lane_tracker_amd", "csrc", "exports.map")).read()
    assert "lt_*" in exports
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native._SIGNATURES and name in _native.exported_symbols() and hasattr(lib, name)
    assert len(_native._SIGNATURES["lt_set_raw_color"][1]) == 4 and len(_native._SIGNATURES["lt_get_raw_color"][1]) == 4
    assert len(_native._SIGNATURES["lt_raw_to_rgb_color"][1]) == 10
    flat = " ".join(header.replace("*", " ").split())
    assert "THE COLOUR STAGE" in flat and flat.lower().count("not a per-frame") >= 3


def test_null_arguments_are_errors_without_a_gpu():
    lib = _native.load()
    m, t = IDENT.copy(), np.arange(256, dtype=np.uint8)
    frame, out = np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.uint8)
    is_set = np.array([7], np.int32)
    assert lib.lt_set_raw_color(None, m.ctypes.data, t.ctypes.data, 1) == -1 and b"context" in lib.lt_last_error()
    assert lib.lt_set_raw_color(None, None, None, 0) == -1 and b"context" in lib.lt_last_error()
    assert lib.lt_get_raw_color(None, m.ctypes.data, t.ctypes.data, is_set.ctypes.data_as(_native.C.POINTER(_native.C.c_int))) == -1
    assert b"context" in lib.lt_last_error() and is_set[0] == 7 and np.array_equal(m, IDENT)
    assert lib.lt_raw_to_rgb_color(None, frame.ctypes.data, 4, 4, 16, None, 0, None, None, out.ctypes.data) == -1 and b"null" in lib.lt_last_error()
    assert not out.any()


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------
class _Ctx(fake_context.FakeContext):
    """The CPU stand-in as a raw Bayer context with a colour stage: uploads take mosaics (n, H, W), condition them with the table that is
    set at that moment, demosaic them, take them through the stage that is set at that moment, and hold the result, as the device
    context's kernels do."""
    touched = 0

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.layout, self.lut, self.color, self.color_calls = "rgb", None, None, 0

    def set_input_format(self, pixel_format, matrix="bt601"):
        self.layout = pixel_format

    def set_raw_lut(self, lut):
        assert _native.raw_bits(self.layout)
        self.lut = None if lut is None else lut.copy()

    def set_raw_color(self, ccm=None, curve=None, enable=True):
        assert _native.raw_bits(self.layout)
        assert ccm is None or (ccm.dtype == np.int16 and ccm.shape == (3, 3))
        assert curve is None or (curve.dtype == np.uint8 and curve.shape == (256,))
        self.color = (None if ccm is None else ccm.copy(), None if curve is None else curve.copy()) if enable else None
        self.color_calls += 1

    def upload_frame_rows(self, frames, first=0, enqueue=False):
        type(self).touched += 1
        if self.layout == "rgb":
            return super().upload_frame_rows(frames, first, enqueue)
        f = np.asarray(frames)
        assert f.dtype == _native.frame_dtype(self.layout)
        f = f.reshape(-1, self.img_h, self.img_w)
        pattern = self.layout
        if self.layout in _native.BAYER_WIDE_FORMATS:
            pattern = "bayer_" + self.layout[8:]
        if self.lut is not None:
            f = utils.apply_raw_lut(f, self.layout, self.lut)
        rgb = RB.bayer_to_rgb(f, pattern)
        if self.color is not None:
            rgb = utils.apply_raw_color(rgb, *self.color)
        return super().upload_frame_rows(rgb, first, enqueue)
    upload_frames = upload_frame_rows


class _OldCtx(fake_context.FakeContext):
    """A stand-in from before the colour stage: it has no set_raw_color at all."""

    def set_input_format(self, pixel_format, matrix="bt601"):
        pass

    def set_raw_lut(self, lut):
        pass

    def __getattr__(self, name):
        if name in ("set_raw_color", "get_raw_color"):
            raise AssertionError("the colour stage's context call was made")
        raise AttributeError(name)


@pytest.fixture()
def fake(monkeypatch):
    monkeypatch.setattr(_native, "Context", _Ctx)
    _Ctx.touched = 0
    return _Ctx


def test_refusals_come_before_any_device_call():
    cal = calib.reference_calibration()
    m, t = random_stage(4)

    def no_device(*a, **k):
        raise AssertionError("a device context was created")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_native, "Context", no_device)
        for kind in (LaneTracker, lambda **k: LaneTrackerGroup(2, **k)):
            for fmt in ("rgb", "nv12", "yuy2", "bgra"):
                for kw in (dict(raw_ccm=m), dict(raw_curve=t), dict(raw_ccm=m, raw_curve=t)):
                    with pytest.raises(ValueError, match="raw Bayer"):
                        kind(**cal, pixel_format=fmt, **kw)
            for fmt in ("bayer_rggb", "bayer10_grbg", "bayer12_bggr"):
                for bad in (m.astype(np.float32), m.astype(np.float64) / 1024, m.astype(np.int32), m[:2], m.reshape(-1), m[None], CAMERA):
                    with pytest.raises(ValueError, match=r"utils\.raw_ccm"):
                        kind(**cal, pixel_format=fmt, raw_ccm=bad)
                    with pytest.raises(ValueError, match=r"utils\.raw_ccm"):
                        kind(**cal, pixel_format=fmt, raw_ccm=bad, raw_curve=t)
                for bad in (t[:255], t.astype(np.int16), t.astype(np.float32), t[None], np.zeros((4, 256), np.uint8)):
                    with pytest.raises(ValueError, match=r"\(256,\)"):
                        kind(**cal, pixel_format=fmt, raw_curve=bad)
                    with pytest.raises(ValueError, match=r"\(256,\)"):
                        kind(**cal, pixel_format=fmt, raw_ccm=m, raw_curve=bad)
        for bad in (dict(ccm=m.astype(np.float32)), dict(curve=t[:10])):
            with pytest.raises(ValueError):
                utils.bayer_to_rgb_color(np.zeros((4, 4), np.uint8), "bayer_rggb", **bad)
        with pytest.raises(ValueError, match="pattern"):
            utils.bayer_to_rgb_color(np.zeros((4, 4, 3), np.uint8), "rgb", ccm=m)


def test_a_tracker_without_the_keywords_never_calls_the_new_context_method(monkeypatch):
    monkeypatch.setattr(_native, "Context", _OldCtx)
    cal = calib.reference_calibration()
    lut = np.random.default_rng(0).integers(0, 256, (4, 256), dtype=np.uint8)
    made = [LaneTracker(**cal), LaneTracker(**cal, pixel_format="bayer_rggb"), LaneTracker(**cal, pixel_format="bayer_gbrg", raw_lut=lut),
            LaneTracker(**cal, pixel_format="bayer12_rggb"), LaneTrackerGroup(2, **cal), LaneTrackerGroup(2, **cal, pixel_format="bayer10_bggr")]
    try:
        for t in made:
            assert t.raw_ccm is None and t.raw_curve is None
        made[0].set_raw_color()                                   # (None, None) on a tracker that takes no stage: nothing to ask
        made[4].set_raw_color(None, None)
        with pytest.raises(AssertionError, match="context call"):
            made[1].set_raw_color(IDENT)                          # ... and this stand-in does tell
    finally:
        for t in made:
            t.close()


def test_set_raw_color_on_trackers_and_groups(fake):
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    (m1, t1), (m2, t2) = random_stage(1), (utils.raw_ccm(CAMERA), utils.raw_curve("srgb"))
    for fmt, dtype in (("bayer_gbrg", np.uint8), ("bayer12_gbrg", np.uint16)):
        t, plain, half = LaneTracker(**cal, pixel_format=fmt, raw_ccm=m1, raw_curve=t1), LaneTracker(**cal, pixel_format=fmt), LaneTracker(**cal, pixel_format=fmt, raw_curve=t1)
        try:
            assert np.array_equal(t.raw_ccm, m1) and np.array_equal(t.raw_curve, t1)
            assert np.array_equal(t._ctx.color[0], m1) and np.array_equal(t._ctx.color[1], t1) and t._ctx.color_calls == 1
            assert plain.raw_ccm is None and plain.raw_curve is None and plain._ctx.color is None and plain._ctx.color_calls == 0
            assert half.raw_ccm is None and np.array_equal(half.raw_curve, t1) and half._ctx.color[0] is None      # either one turns it on
            t.raw_ccm[0, 0] ^= 1                                   # the properties hand out copies
            t.raw_curve[0] ^= 1
            assert np.array_equal(t.raw_ccm, m1) and np.array_equal(t.raw_curve, t1)
            assert "raw_ccm" not in t.get_state() and "raw_curve" not in t.get_state()          # configuration, not state
            t.set_raw_color(m2, t2)
            assert np.array_equal(t.raw_ccm, m2) and np.array_equal(t._ctx.color[1], t2)
            for bad in (dict(ccm=m2.astype(np.float32)), dict(ccm=m2[:2]), dict(curve=t2[:100]), dict(curve=t2.astype(np.int8))):
                with pytest.raises(ValueError):
                    t.set_raw_color(**bad)
            assert np.array_equal(t._ctx.color[0], m2) and np.array_equal(t.raw_curve, t2)
            gen = t.process_stream([np.zeros((2, H, W), dtype), np.zeros((1, H, W), dtype)], annotate=False)
            next(gen)
            calls = t._ctx.color_calls
            with pytest.raises(RuntimeError, match="process_stream"):
                t.set_raw_color(m1, t1)
            with pytest.raises(RuntimeError, match="process_stream"):
                t.set_raw_color()
            assert t._ctx.color_calls == calls and np.array_equal(t.raw_ccm, m2)
            gen.close()
            t.set_raw_color()                                      # (None, None): off
            assert t.raw_ccm is None and t.raw_curve is None and t._ctx.color is None and t._ctx.color_calls == calls + 1
            plain.set_raw_color(curve=t1)
            assert plain.raw_ccm is None and np.array_equal(plain.raw_curve, t1) and plain._ctx.color[0] is None
        finally:
            t.close(), plain.close(), half.close()
        g = LaneTrackerGroup(2, **cal, pixel_format=fmt, raw_ccm=m1, raw_curve=t1)
        try:
            assert np.array_equal(g.raw_ccm, m1) and np.array_equal(g.raw_curve, t1) and g._ctx.color_calls == 1
            assert all(np.array_equal(x.raw_ccm, m1) and np.array_equal(x.raw_curve, t1) for x in g.trackers)
            g.set_raw_color(m2)
            assert np.array_equal(g.raw_ccm, m2) and g.raw_curve is None and all(np.array_equal(x.raw_ccm, m2) and x.raw_curve is None for x in g.trackers)
            with pytest.raises(RuntimeError):
                g.trackers[0].set_raw_color(m1, t1)                # one stage for the whole group
            with pytest.raises(ValueError):
                g.set_raw_color(m2.reshape(-1))
            g.set_raw_color()
            assert g.raw_ccm is None and g._ctx.color is None and all(x.raw_ccm is None for x in g.trackers)
        finally:
            g.close()
    rgb = LaneTracker(**cal)
    try:
        rgb.set_raw_color()                                        # nothing to do on a tracker that takes no stage
        with pytest.raises(ValueError, match="raw Bayer"):
            rgb.set_raw_color(m1)
        assert rgb._ctx.color_calls == 0
    finally:
        rgb.close()


def test_a_tracker_with_a_stage_is_the_rgb_one_fed_the_converted_frames(fake):
    cal = calib.reference_calibration()
    r = synth.SceneRenderer()
    pattern = "bayer_grbg"
    mos = RB.rgb_to_bayer(np.stack([r.render(i)[0] for i in range(3)], 0), pattern)
    m, c = utils.raw_ccm(CAMERA), utils.raw_curve("srgb")
    lut = utils.raw_lut(8, 240, (1.5, 1, 1.3))
    want_frames = utils.apply_raw_color(RB.bayer_to_rgb(utils.apply_raw_lut(mos, pattern, lut), pattern), m, c)
    t, ref = LaneTracker(**cal, pixel_format=pattern, raw_lut=lut, raw_ccm=m, raw_curve=c), LaneTracker(**cal)
    try:
        got = t.process_batch(mos, annotate=False)
        want = ref.process_batch(want_frames, annotate=False)
        assert repr(got) == repr(want)
        sa, sb = t.get_state(), ref.get_state()
        for key in ("pixel_format", "yuv_matrix"):                 # (what tells the two apart: the format, and nothing of the stage)
            sa.pop(key, None), sb.pop(key, None)
        assert repr(sa) == repr(sb)
    finally:
        t.close(), ref.close()


# ---- video.py -------------------------------------------------------------------------------------------------------------------------------
def test_video_cli_hands_the_stage_to_the_tracker(tmp_path, fake, capsys):
    cal = calib.reference_calibration()
    utils.save_calibration_npz(str(tmp_path / "cam.npz"), str(tmp_path / "warp.npz"), cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0],
                               cal["warp_matrices"][1], cal["img_size"], cal["warped_size"], *cal["mpp_conversion"])
    r = synth.SceneRenderer()
    clip = str(tmp_path / "scenes.bayer")
    RB.rgb_to_bayer(np.stack([r.render(i)[0] for i in range(2)], 0), "bayer_bggr").tofile(clip)
    seen = []
    real = _Ctx.set_raw_color

    def spy(self, ccm=None, curve=None, enable=True):
        seen.append((ccm, curve, enable))
        return real(self, ccm, curve, enable)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_Ctx, "set_raw_color", spy)
        args = [clip, "-", "--cam", str(tmp_path / "cam.npz"), "--warp", str(tmp_path / "warp.npz"), "--pixel-format", "bayer_bggr"]
        text = ",".join(str(v) for row in CAMERA for v in row)
        assert video.main(args + ["--raw-ccm", text, "--raw-out-gamma", "srgb"]) == 0
        assert len(seen) == 1 and np.array_equal(seen[0][0], utils.raw_ccm(CAMERA)) and np.array_equal(seen[0][1], utils.raw_curve("srgb")) and seen[0][2]
        assert video.main(args + ["--raw-out-gamma", "2.2"]) == 0
        assert len(seen) == 2 and seen[1][0] is None and np.array_equal(seen[1][1], utils.raw_curve(2.2))
        assert video.main(args + ["--raw-ccm", text]) == 0
        assert len(seen) == 3 and seen[2][1] is None
        assert video.main(args) == 0
        assert len(seen) == 3                                      # no flag: no stage, no call
        for bad in (["--pixel-format", "bayer_bggr", "--raw-ccm", "1,0,0,0,1,0,0,0"], ["--pixel-format", "bayer_bggr", "--raw-ccm", "40,0,0,0,1,0,0,0,1"],
                    ["--pixel-format", "bayer_bggr", "--raw-ccm", "a,0,0,0,1,0,0,0,1"], ["--pixel-format", "bayer_bggr", "--raw-out-gamma", "0"],
                    ["--pixel-format", "bayer_bggr", "--raw-out-gamma", "rec709"]):
            with pytest.raises(SystemExit) as e:
                video.main(args[:-2] + bad)
            assert e.value.code == 2
    # without a raw format both options are refused, whatever the input is
    rgb_clip = str(tmp_path / "scenes.rgb")
    np.stack([r.render(i)[0] for i in range(2)], 0).tofile(rgb_clip)
    W, H = cal["img_size"]
    base = [rgb_clip, "-", "--cam", str(tmp_path / "cam.npz"), "--warp", str(tmp_path / "warp.npz"), "--size", "%dx%d" % (W, H)]
    for bad in (["--raw-ccm", text], ["--raw-out-gamma", "srgb"], ["--pixel-format", "rgb", "--raw-ccm", text]):
        with pytest.raises(SystemExit) as e:
            video.main(base + bad)
        assert e.value.code == 2
    assert len(seen) == 3
    capsys.readouterr()
