"""YUV 4:2:0 input without a GPU: the NumPy restatement of the conversion (`tests/yuv_reference.py`) held against the real-valued
formula, OpenCV where it imports, and bytes written out here; the host logic of a 4:2:0 tracker on a CPU stand-in for the device
context; raw `.nv12` / `.i420` frame sources; the C header, the binding's table and the library's exports."""
import os
import re
import subprocess

import numpy as np
import pytest

import fake_context
import yuv_reference as R
from lane_tracker_amd import _native, calib, synth, video
from lane_tracker_amd.lane_tracker import LaneTracker

try:
    import cv2
except Exception:   # ImportError, or a broken binary wheel
    cv2 = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,largest", [("bt601", 560969128), ("bt709", 573487137)])
def test_integer_form_is_the_real_formula_rounded_once(matrix, largest):
    """All 256^3 (Y, U, V) triples, a plane of (U, V) per Y: |integer form - real-valued formula| <= 1 on every channel (the
    integer form rounds once, half up), and no intermediate leaves int32."""
    cy, cvr, cvg, cug, cub = (c / 2.0 ** 20 for c in R.MATRICES[matrix])
    icy, icvr, icvg, icug, icub = R.MATRICES[matrix]
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst, biggest = 0.0, 0
    for y in range(256):
        yy = max(0, y - 16)
        real = np.stack([cy * yy + cvr * (v - 128), cy * yy + cvg * (v - 128) + cug * (u - 128), cy * yy + cub * (u - 128)], -1)
        got = R.convert_triples(np.full_like(u, y), u, v, matrix)
        worst = max(worst, float(np.abs(got.astype(np.float64) - np.clip(real, 0, 255)).max()))
        base = icy * yy + (1 << 19)
        for t in (base + icvr * (v - 128), base + icvg * (v - 128) + icug * (u - 128), base + icub * (u - 128)):
            biggest = max(biggest, int(np.abs(t).max()))
    print("worst |integer - real| =", worst, " largest |intermediate| =", biggest)
    assert worst <= 1.0
    assert biggest == largest and biggest < 2 ** 31


TRIPLES = [((16, 128, 128), (0, 0, 0), (0, 0, 0)), ((235, 128, 128), (255, 255, 255), (255, 255, 255)),
           ((81, 90, 240), (254, 0, 0), (255, 24, 0)), ((145, 54, 34), (0, 255, 1), (0, 216, 0)),
           ((41, 240, 110), (0, 0, 255), (0, 15, 255))]


@pytest.mark.parametrize("yuv,bt601,bt709", TRIPLES)
def test_written_out_triples(yuv, bt601, bt709):
    assert tuple(int(c) for c in R.convert_triples(*yuv, "bt601")) == bt601
    assert tuple(int(c) for c in R.convert_triples(*yuv, "bt709")) == bt709


def test_layouts_hold_the_same_picture():
    rgb = np.random.default_rng(4).integers(0, 256, (34, 66, 3), dtype=np.uint8)
    nv12, i420 = R.rgb_to_yuv420(rgb, "nv12"), R.rgb_to_yuv420(rgb, "i420")
    assert nv12.shape == i420.shape == (51, 66) and not np.array_equal(nv12, i420)
    assert np.array_equal(R.yuv420_to_rgb(nv12, "nv12"), R.yuv420_to_rgb(i420, "i420"))
    flat = np.full((8, 8, 3), (200, 40, 90), np.uint8)                      # a flat colour survives the round trip to within rounding
    assert np.abs(R.yuv420_to_rgb(R.rgb_to_yuv420(flat, "i420"), "i420").astype(int) - flat).max() <= 2


@pytest.mark.skipif(cv2 is None, reason="UNVERIFIED vs OpenCV (cv2 absent)")
@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_restatement_is_opencv(layout):
    frame = np.random.default_rng(9).integers(0, 256, (720 * 3 // 2, 1280), dtype=np.uint8)
    code = cv2.COLOR_YUV2RGB_NV12 if layout == "nv12" else cv2.COLOR_YUV2RGB_I420
    assert np.array_equal(R.yuv420_to_rgb(frame, layout, "bt601"), cv2.cvtColor(frame, code))


# ---- the host logic of a 4:2:0 tracker -------------------------------------------------------------------------------------------
class YuvFakeContext(fake_context.FakeContext):
    """The CPU stand-in with an input format: 4:2:0 frames are converted with the restatement and handed on as RGB."""
    layout, matrix = "rgb", "bt601"

    def set_input_format(self, pixel_format="rgb", yuv_matrix="bt601"):
        _native.frame_shape((self.img_w, self.img_h), pixel_format)
        self.layout, self.matrix = pixel_format, yuv_matrix

    def _rgb(self, frames):
        if self.layout == "rgb":
            return frames
        f = np.asarray(frames)
        if f.shape[-2:] != (self.img_h * 3 // 2, self.img_w) or f.ndim not in (2, 3):
            raise ValueError("expected 4:2:0 frames, got %r" % (f.shape,))
        return np.stack([R.yuv420_to_rgb(x, self.layout, self.matrix) for x in f.reshape(-1, self.img_h * 3 // 2, self.img_w)])

    def upload_frame_rows(self, frames, first=0, enqueue=False):
        return super().upload_frame_rows(self._rgb(frames), first, enqueue)
    upload_frames = upload_frame_rows

    def upload_frame_rows_async(self, frames, first=0):
        super().upload_frame_rows(self._rgb(frames), first)
        return frames


@pytest.fixture()
def fake(monkeypatch):
    monkeypatch.setattr(_native, "Context", YuvFakeContext)
    yield YuvFakeContext


def _state(lt):
    b = lambda a: None if a is None else np.asarray(a).tobytes()
    return dict(detected=lt.detected_pixels, valid=lt.valid_lane_lines, last_detection=lt.last_detection, success=lt.success,
                counter=lt.counter, left_avg=b(lt.left_avg_coeffs), right_avg=b(lt.right_avg_coeffs), last_left=b(lt.last_left_coeffs),
                last_right=b(lt.last_right_coeffs), hist=[b(c) for c in lt.left_fit_coeffs] + [b(c) for c in lt.right_fit_coeffs],
                radii=list(lt.average_curve_radii), radius=lt.average_curve_radius, ecc=lt.eccentricity,
                pix=(b(lt.left_y), b(lt.left_x), b(lt.right_y), b(lt.right_x)), cent=(lt.left_window_centroids, lt.right_window_centroids))


PLAN = [0, 1, 2, 1, 4, 1, 2, 3, 2, 4, 4, 4, 4, 4, 4, 0, 1, 2]          # lanes, a one-off failure, an outage beyond n_reset, recovery


@pytest.fixture(scope="module")
def streams():
    """The same stream three times: NV12 frames, I420 frames, and the RGB frames they convert to."""
    a, b = synth.stream_lanes(3, seed=101), synth.stream_lanes(1, seed=202)
    pool = [a[0], a[1], a[2], b[0], np.zeros_like(a[0])]
    out = {}
    for layout in ("nv12", "i420"):
        y = [R.rgb_to_yuv420(f, layout) for f in pool]
        out[layout] = np.stack([y[k] for k in PLAN])
    out["rgb"] = np.stack([R.yuv420_to_rgb(f, "nv12") for f in out["nv12"]])
    assert np.array_equal(out["rgb"][3], R.yuv420_to_rgb(out["i420"][3], "i420"))
    return out


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_yuv_tracker_gives_the_records_of_an_rgb_tracker_on_the_converted_frames(fake, streams, layout):
    cal = calib.reference_calibration()
    ref = LaneTracker(**cal)
    ref.chain_searches = False
    want = []
    for f in streams["rgb"]:
        ref.process_batch(f[None], annotate=False)
        want.append(_state(ref))
    assert 0 < ref.success < ref.counter == len(PLAN)                # lanes are found, and lost, along the way

    kw, first_try, _ = ref._batch_arguments({})
    one = LaneTracker(**cal, pixel_format=layout)                    # _step, frame by frame
    for k, f in enumerate(streams[layout]):
        one._ctx.upload_frame_rows(f[None], first=0)
        one._ctx.mask_run(1, first=0)
        one._step(f, first_try, kw["n_tries"], False, slot=0, have_mask=True, lazy=True, annotate=False)
        assert _state(one) == want[k], k

    bat = LaneTracker(**cal, pixel_format=layout)                    # process_batch: the chained driver
    bat.chain_chunk = 4
    for lo, hi in ((0, 7), (7, 18)):
        assert bat.process_batch(streams[layout][lo:hi], annotate=False) == [None] * (hi - lo)
        assert _state(bat) == want[hi - 1], (lo, hi)

    stm = LaneTracker(**cal, pixel_format=layout, yuv_matrix="bt601")     # process_stream: three windows
    bounds = ((0, 6), (6, 12), (12, 18))
    for (lo, hi), out in zip(bounds, stm.process_stream([streams[layout][lo:hi] for lo, hi in bounds], annotate=False)):
        assert out == [None] * (hi - lo)
    assert _state(stm) == want[-1]
    for t in (ref, one, bat, stm):
        t.close()


def test_argument_and_state_errors(fake, streams):
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    with pytest.raises(ValueError):
        LaneTracker(**cal, pixel_format="yuyv")
    with pytest.raises(ValueError):
        LaneTracker(**cal, pixel_format="nv12", yuv_matrix="bt2020")
    with pytest.raises(TypeError):
        LaneTracker(*[cal[k] for k in ("img_size", "warped_size", "cam_matrix", "dist_coeffs", "warp_matrices", "mpp_conversion")],
                    8, 4, 2, False, 0, "nv12")                       # keyword-only
    with pytest.raises(ValueError):
        LaneTracker(**dict(cal, img_size=(W + 1, H)), pixel_format="nv12")       # odd width
    with pytest.raises(ValueError):
        LaneTracker(**dict(cal, img_size=(W, H + 1)), pixel_format="i420")       # odd height
    rgb, nv12, i420 = LaneTracker(**cal), LaneTracker(**cal, pixel_format="nv12"), LaneTracker(**cal, pixel_format="i420")
    try:
        for bad in (np.zeros((H, W, 3), np.uint8), np.zeros((H * 3 // 2, W + 2), np.uint8), np.zeros((1, H * 3 // 2, W), np.uint8), None):
            with pytest.raises(ValueError):
                nv12.process(bad)
        assert nv12.counter == 0                                                 # nothing was uploaded, nothing counted
        for annotate in (False, True):
            with pytest.raises(ValueError):
                nv12.process_batch(np.zeros((2, H, W, 3), np.uint8), annotate=annotate)
        with pytest.raises(ValueError):
            nv12.process_batch(streams["nv12"][:2], annotate="inplace")
        with pytest.raises(ValueError):
            list(nv12.process_stream([streams["nv12"][:2]], annotate="inplace"))
        with pytest.raises(ValueError):
            list(nv12.process_stream([np.zeros((2, H, W, 3), np.uint8)], annotate=False))
        # state: an RGB tracker's is what it was; a 4:2:0 tracker's names its format, and moves only between trackers of that format
        assert "pixel_format" not in rgb.get_state() and "yuv_matrix" not in rgb.get_state()
        nv12.process_batch(streams["nv12"][:3], annotate=False)
        st = nv12.get_state()
        assert (st["pixel_format"], st["yuv_matrix"], st["version"]) == ("nv12", "bt601", LaneTracker.STATE_VERSION)
        for other in (rgb, i420):
            with pytest.raises(ValueError):
                other.set_state(st)
        with pytest.raises(ValueError):
            nv12.set_state(rgb.get_state())
        twin = LaneTracker(**cal, pixel_format="nv12")
        twin.set_state(st)
        assert _state(twin)["hist"] == _state(nv12)["hist"] and twin.counter == 3
        twin.close()
    finally:
        for t in (rgb, nv12, i420):
            t.close()


def test_group_takes_the_keywords(fake):
    from lane_tracker_amd.group import LaneTrackerGroup
    cal = calib.reference_calibration()
    W, H = cal["img_size"]
    g = LaneTrackerGroup(2, **cal, pixel_format="i420", yuv_matrix="bt709")
    try:
        assert g._ctx.layout == "i420" and g._ctx.matrix == "bt709"
        assert all(t.pixel_format == "i420" and t.yuv_matrix == "bt709" for t in g.trackers)
        with pytest.raises(ValueError):
            g.process([np.zeros((H, W, 3), np.uint8), None], annotate=False)
    finally:
        g.close()
    with pytest.raises(ValueError):
        LaneTrackerGroup(2, **cal, pixel_format="p010")


# ---- raw 4:2:0 files ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext,layout", [(".nv12", "nv12"), (".i420", "i420"), (".yuv", "i420")])
def test_raw_yuv_files_round_trip_through_frame_source(tmp_path, ext, layout):
    frames = np.random.default_rng(1).integers(0, 256, (5, 36 * 3 // 2, 64), dtype=np.uint8)
    path = tmp_path / ("clip" + ext)
    frames.tofile(path)
    with pytest.raises(ValueError):
        video.FrameSource(path)                                      # size is required, as for .rgb
    with pytest.raises(ValueError):
        video.FrameSource(path, size=(64, 34))                       # not a whole number of frames
    src = video.FrameSource(path, size=(64, 36))
    assert (src.pixel_format, len(src), src.size) == (layout, 5, (64, 36))
    assert np.array_equal(src.read(1, 4), frames[1:4]) and src.read(1, 4).flags["C_CONTIGUOUS"]
    assert np.array_equal(np.stack(list(src)), frames)
    assert video.VideoFileClip(str(path), size=(64, 36)).pixel_format == layout
    rgb = tmp_path / "clip.rgb"
    np.zeros((2, 36, 64, 3), np.uint8).tofile(rgb)
    assert video.FrameSource(rgb, size=(64, 36)).pixel_format == "rgb"


def test_process_frames_wants_a_tracker_of_the_sources_format(fake, tmp_path, streams):
    cal = calib.reference_calibration()
    path = tmp_path / "clip.nv12"
    streams["nv12"][:5].tofile(path)
    src = video.FrameSource(path, size=cal["img_size"])
    rgb, nv12 = LaneTracker(**cal), LaneTracker(**cal, pixel_format="nv12")
    try:
        with pytest.raises(ValueError):
            video.process_frames(rgb, src, window=4)
        assert video.process_frames(nv12, src, window=4)[0] == 5
        assert nv12.counter == 5 and nv12.success >= 3
    finally:
        rgb.close()
        nv12.close()


# ---- header, binding table, exports ------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported():
    names = {"lt_set_input_format", "lt_get_input_format", "lt_yuv_to_rgb"}
    header = open(os.path.join(ROOT, "include", "lane_tracker_amd.h")).read()
    declared = set(re.findall(r"\b(lt_[a-z0-9_]+)\s*\(", header))
    exported = {l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True).splitlines()
                if l.split()[-1].startswith("lt_")}
    assert names <= declared and names <= set(_native._SIGNATURES) and names <= exported
    assert declared == exported == set(_native._SIGNATURES)          # and the three lists still agree as a whole
    for name, value in (("LT_INPUT_RGB", 0), ("LT_INPUT_NV12", 1), ("LT_INPUT_I420", 2)):
        assert re.search(r"\b%s = %d\b" % (name, value), header)
    assert _native.PIXEL_FORMATS == {"rgb": 0, "nv12": 1, "i420": 2}
    for key, macro in (("bt601", "LT_YUV_BT601"), ("bt709", "LT_YUV_BT709")):
        in_header = tuple(int(v) for v in re.search(r"#define %s \{([^}]*)\}" % macro, header).group(1).split(","))
        assert in_header == _native.YUV_MATRICES[key] == R.MATRICES[key]
    assert int(re.search(r"#define LT_ABI_VERSION (\d+)", header).group(1)) == 5 == _native.ABI_VERSION
