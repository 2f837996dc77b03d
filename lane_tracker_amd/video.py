"""Frame source / sink either side of the tracker.

The reference drives `LaneTracker.process` through moviepy (`process_video.py:41-44`: VideoFileClip ->
fl_image -> write_videofile).  moviepy and ffmpeg do not exist in this image, so video containers are out
of scope; what a lane-tracking run needs is an ordered sequence of RGB u8 frames in and the annotated
frames out.  Supported on both sides:

  * a directory of images (PNG/JPEG/BMP/PPM, sorted by name; Pillow),
  * a `.npy` array of shape (n, H, W, 3) (memory-mapped, so a long clip never has to fit in RAM),
  * a headerless raw RGB24 file (`.rgb` / `.raw`; what `ffmpeg -pix_fmt rgb24 -f rawvideo` writes and reads),
  * on the input side, a headerless raw YUV 4:2:0 file as cameras and decoders produce it: `.nv12`, or `.i420` / `.yuv` (I420;
    `ffmpeg -pix_fmt nv12 | yuv420p -f rawvideo`).  Its frames are (H * 3 // 2, W) arrays for a tracker built with the same
    `pixel_format`, which converts them on the device; what comes out, and every sink, is RGB -- unless
  * or a headerless raw packed 4:2:2 file as cameras and capture cards produce it: `.yuy2` (Y0 U Y1 V) or `.uyvy` (U Y0 V Y1),
    H * W * 2 bytes a frame (`ffmpeg -pix_fmt yuyv422 | uyvy422 -f rawvideo`); its frames are (H, W, 2) arrays.  A `FrameSink`
    with such a `pixel_format` writes the same files (the bytes as given; the tracker itself has no 4:2:2 output)
  * or a headerless raw file of another member of the RGB family, as users' own software holds frames: `.bgr` (B G R, H * W * 3
    bytes a frame; OpenCV's order), `.rgba` / `.bgra` (H * W * 4; `ffmpeg -pix_fmt bgr24 | rgba | bgra -f rawvideo`); frames of
    shape (H, W, 3) / (H, W, 4), alpha not read.  These three are output formats too (`--out-format`, alpha written as 255)
  * `--out-format nv12 | i420` (or `rgb`) asks for the annotated frames through a device sink (`process_stream(..., out=)`): they
    are converted on the device and written as a raw `.nv12` / `.i420` (`.rgb`) file, which this module also reads.

`process_frames()` feeds the tracker in windows through `LaneTracker.process_stream` (the stream pipeline:
masks of the whole window batched ahead on the GPU, state machine trailing), which gives exactly the
frames `process()` would return one by one.  `VideoFileClip` is the small part of moviepy's interface that
`process_video.py` uses, on top of the same sources and sinks.

CLI:  python -m lane_tracker_amd.video IN OUT [--cam cam_calib.p] [--warp warp_params.p] [--size WxH] ...
"""
import argparse
import os
import sys
import time

import numpy as np

_IMAGE_EXT = (".png", ".jpg", ".jpeg", ".bmp", ".ppm")


_VIDEO_EXT = (".mp4", ".avi", ".mov", ".mkv", ".webm")


def _is_raw(path):
    return str(path).lower().endswith((".rgb", ".raw"))


def _yuv_layout(path):
    """'nv12' / 'i420' for a raw 4:2:0 file name, 'yuy2' / 'uyvy' for a raw packed 4:2:2 one, 'bgr' / 'rgba' / 'bgra' for a raw
    file of the RGB family's other members, else None."""
    p = str(path).lower()
    for name in _RGB_FAMILY:
        if p.endswith("." + name):
            return name
    return ("nv12" if p.endswith(".nv12") else "i420" if p.endswith((".i420", ".yuv")) else "yuy2" if p.endswith(".yuy2")
            else "uyvy" if p.endswith(".uyvy") else None)


_RGB_FAMILY = ("bgr", "rgba", "bgra")
# 8-bit raw Bayer: headerless `.bayer` files; the suffix cannot name the pattern, the caller does (FrameSource's pixel_format)
_BAYER = ("bayer_rggb", "bayer_grbg", "bayer_gbrg", "bayer_bggr")
# 10- / 12-bit raw Bayer: headerless `.bayer16` files of little-endian uint16, the sample in the low bits; the caller names depth and pattern
_BAYER_WIDE = tuple("bayer%d_%s" % (b, n[6:]) for b in (10, 12) for n in _BAYER)


# the same MIPI-packed (CSI-2 RAW10 / RAW12): headerless `.bayer10p` / `.bayer12p` files of packed rows, 5 W / 4 or 3 W / 2 bytes each; the
# suffix names the depth, the caller the pattern -- and a depth that agrees
_BAYER_PACKED = tuple("bayer%dp_%s" % (b, n[6:]) for b in (10, 12) for n in _BAYER)
_RAW_ALL = _BAYER + _BAYER_WIDE + _BAYER_PACKED


def _packed_file_bits(path):
    """10 / 12 for a `.bayer10p` / `.bayer12p` file, 0 for any other."""
    p = str(path).lower()
    return 10 if p.endswith(".bayer10p") else 12 if p.endswith(".bayer12p") else 0


def _is_bayer_file(path):
    return str(path).lower().endswith(".bayer")


def _is_bayer16_file(path):
    return str(path).lower().endswith(".bayer16")


def _raw_format_bits(pixel_format):
    return 8 if pixel_format in _BAYER else int(pixel_format[5:7])


def _yuv_tail(pixel_format, width, height):
    """(shape of one frame, the format's family name); ValueError for a size the format does not take."""
    if pixel_format in _RGB_FAMILY:
        if width < 2 or height < 1:
            raise ValueError(f"{pixel_format} frames need a width of at least 2, got {width}x{height}")
        return (height, width, 3 if pixel_format == "bgr" else 4), pixel_format.upper()
    if pixel_format in _RAW_ALL:
        if width % 2 or height % 2 or width < 4 or height < 4:
            raise ValueError(f"raw Bayer frames need an even width and height of at least 4, got {width}x{height}")
        if pixel_format in _BAYER_PACKED:
            if pixel_format.startswith("bayer10p") and width % 4:
                raise ValueError(f"MIPI-packed RAW10 frames need a width that is a multiple of 4, got {width}x{height}")
            return (height, width * 5 // 4 if pixel_format.startswith("bayer10p") else width * 3 // 2), "MIPI-packed raw Bayer"
        return (height, width), "raw Bayer"
    if pixel_format in ("yuy2", "uyvy"):
        if width % 2 or width < 4 or height < 1:
            raise ValueError(f"4:2:2 frames need an even width of at least 4, got {width}x{height}")
        return (height, width, 2), "4:2:2"
    if width % 2 or height % 2 or width < 2 or height < 2:
        raise ValueError(f"4:2:0 frames need an even width and height, got {width}x{height}")
    return (height * 3 // 2, width), "4:2:0"


def resolve_clip_path(path, must_exist=True):
    """A video file name as process_video.py spells it ('clip.mp4') -> the frame sequence standing in for
    it: 'clip.mp4' itself if it is a directory, else 'clip/' , 'clip.npy' or 'clip.rgb' next to it.  For
    outputs (must_exist=False) a video extension is dropped and the result is a directory of PNGs."""
    path = str(path)
    stem, ext = os.path.splitext(path)
    if ext.lower() not in _VIDEO_EXT:
        return path
    if not must_exist:
        return stem
    for cand in (path, stem, stem + ".npy", stem + ".rgb"):
        if os.path.isdir(cand) or (cand != path and os.path.isfile(cand)):
            return cand
    raise FileNotFoundError(f"{path}: video containers cannot be decoded here (no ffmpeg); put the frames in "
                            f"{stem}/ (images), {stem}.npy or {stem}.rgb")


class FrameSource:
    """Ordered u8 frames: RGB (n, H, W, 3), or -- `pixel_format` 'nv12' / 'i420', raw 4:2:0 files -- (n, H * 3 // 2, W), or --
    'yuy2' / 'uyvy', raw packed 4:2:2 files -- (n, H, W, 2), or -- 'bgr' / 'rgba' / 'bgra', raw files -- (n, H, W, 3) / (n, H, W, 4).
    Headerless 8-bit raw Bayer files (`.bayer`) hold frames (n, H, W); their suffix cannot name the pattern, so `pixel_format` must
    ('bayer_rggb', 'bayer_grbg', 'bayer_gbrg', 'bayer_bggr').  `size` = (width, height) is required for raw files only."""

    pixel_format = "rgb"

    def __init__(self, path, size=None, pixel_format=None):
        self.path = str(path)
        if pixel_format in _BAYER and not _is_bayer_file(self.path):
            raise ValueError(f"pixel_format={pixel_format!r} names the pattern of a raw .bayer file; {self.path!r} is none")
        if pixel_format in _BAYER_WIDE and not _is_bayer16_file(self.path):
            raise ValueError(f"pixel_format={pixel_format!r} names depth and pattern of a raw .bayer16 file; {self.path!r} is none")
        if pixel_format in _BAYER_PACKED and _packed_file_bits(self.path) != _raw_format_bits(pixel_format):
            raise ValueError(f"pixel_format={pixel_format!r} names the pattern of a raw .bayer{_raw_format_bits(pixel_format)}p file; {self.path!r} is none")
        self._dtype = np.dtype(np.uint8)
        self._files = None
        self._array = None
        self._tail = None                # shape of one frame
        if os.path.isdir(self.path):
            self._files = sorted(os.path.join(self.path, f) for f in os.listdir(self.path)
                                 if f.lower().endswith(_IMAGE_EXT))
            if not self._files:
                raise ValueError(f"no image files in {self.path}")
            first = self._read_image(self._files[0])
            self.height, self.width = first.shape[:2]
            self._n = len(self._files)
        elif self.path.lower().endswith(".npy"):
            self._array = np.load(self.path, mmap_mode="r")
            if self._array.ndim != 4 or self._array.shape[3] != 3 or self._array.dtype != np.uint8:
                raise ValueError("expected a uint8 array of shape (n, H, W, 3)")
            self._n, self.height, self.width = self._array.shape[:3]
        elif _is_raw(self.path):
            if size is None:
                raise ValueError("raw RGB24 input needs size=(width, height)")
            self.width, self.height = int(size[0]), int(size[1])
            fb = self.width * self.height * 3
            nbytes = os.path.getsize(self.path)
            if nbytes % fb:
                raise ValueError(f"{self.path}: {nbytes} bytes is not a whole number of {self.width}x{self.height} frames")
            self._n = nbytes // fb
            self._array = np.memmap(self.path, np.uint8, "r", shape=(self._n, self.height, self.width, 3)) if self._n \
                else np.zeros((0, self.height, self.width, 3), np.uint8)
        elif _is_bayer_file(self.path):
            if pixel_format not in _BAYER:
                raise ValueError(f"{self.path}: a .bayer file holds raw Bayer frames and its suffix cannot name the pattern: say which with "
                                 "--pixel-format bayer_rggb / bayer_grbg / bayer_gbrg / bayer_bggr (FrameSource's pixel_format=)")
            if size is None:
                raise ValueError("raw Bayer input needs size=(width, height)")
            self.pixel_format = pixel_format
            self.width, self.height = int(size[0]), int(size[1])
            self._tail, family = _yuv_tail(self.pixel_format, self.width, self.height)
            fb = int(np.prod(self._tail))
            nbytes = os.path.getsize(self.path)
            if nbytes % fb:
                raise ValueError(f"{self.path}: {nbytes} bytes is not a whole number of {self.width}x{self.height} {family} frames")
            self._n = nbytes // fb
            self._array = np.memmap(self.path, np.uint8, "r", shape=(self._n,) + self._tail) if self._n \
                else np.zeros((0,) + self._tail, np.uint8)
        elif _packed_file_bits(self.path):
            bits = _packed_file_bits(self.path)
            if pixel_format not in _BAYER_PACKED or _raw_format_bits(pixel_format) != bits:
                raise ValueError(f"{self.path}: a .bayer{bits}p file holds MIPI-packed RAW{bits} frames and its suffix cannot name the pattern: say which "
                                 f"with --pixel-format bayer{bits}p_rggb / _grbg / _gbrg / _bggr (FrameSource's pixel_format=)")
            if size is None:
                raise ValueError("raw Bayer input needs size=(width, height)")
            self.pixel_format = pixel_format
            self.width, self.height = int(size[0]), int(size[1])
            self._tail, family = _yuv_tail(self.pixel_format, self.width, self.height)
            fb = int(np.prod(self._tail))
            nbytes = os.path.getsize(self.path)
            if nbytes % fb:
                raise ValueError(f"{self.path}: {nbytes} bytes is not a whole number of {self.width}x{self.height} {family} frames")
            self._n = nbytes // fb
            self._array = np.memmap(self.path, np.uint8, "r", shape=(self._n,) + self._tail) if self._n \
                else np.zeros((0,) + self._tail, np.uint8)
        elif _is_bayer16_file(self.path):
            if pixel_format not in _BAYER_WIDE:
                raise ValueError(f"{self.path}: a .bayer16 file holds 10- or 12-bit raw Bayer frames in 16-bit words and its suffix names neither "
                                 "depth nor pattern: say which with --pixel-format bayer10_rggb ... bayer12_bggr (FrameSource's pixel_format=)")
            if size is None:
                raise ValueError("raw Bayer input needs size=(width, height)")
            self.pixel_format = pixel_format
            self._dtype = np.dtype("<u2")
            self.width, self.height = int(size[0]), int(size[1])
            self._tail, family = _yuv_tail(self.pixel_format, self.width, self.height)
            fb = int(np.prod(self._tail)) * 2
            nbytes = os.path.getsize(self.path)
            if nbytes % fb:
                raise ValueError(f"{self.path}: {nbytes} bytes is not a whole number of {self.width}x{self.height} 16-bit {family} frames")
            self._n = nbytes // fb
            self._array = np.memmap(self.path, self._dtype, "r", shape=(self._n,) + self._tail) if self._n \
                else np.zeros((0,) + self._tail, np.uint16)
        elif _yuv_layout(self.path):
            if size is None:
                raise ValueError("raw 4:2:0 input needs size=(width, height)" if _yuv_layout(self.path) in ("nv12", "i420")
                                 else "raw %s input needs size=(width, height)" % _yuv_layout(self.path).upper() if _yuv_layout(self.path) in _RGB_FAMILY
                                 else "raw 4:2:2 input needs size=(width, height)")
            self.pixel_format = _yuv_layout(self.path)
            self.width, self.height = int(size[0]), int(size[1])
            self._tail, family = _yuv_tail(self.pixel_format, self.width, self.height)
            fb = int(np.prod(self._tail))
            nbytes = os.path.getsize(self.path)
            if nbytes % fb:
                raise ValueError(f"{self.path}: {nbytes} bytes is not a whole number of {self.width}x{self.height} {family} frames")
            self._n = nbytes // fb
            self._array = np.memmap(self.path, np.uint8, "r", shape=(self._n,) + self._tail) if self._n \
                else np.zeros((0,) + self._tail, np.uint8)
        else:
            raise ValueError(f"unsupported frame source {self.path!r} (directory of images, .npy, .rgb/.raw, .bgr, .rgba, .bgra, .nv12, .i420/.yuv, .yuy2, .uyvy, .bayer, .bayer16, .bayer10p, .bayer12p)")
        if self._tail is None:
            self._tail = (self.height, self.width, 3)
        if size is not None and (self.width, self.height) != (int(size[0]), int(size[1])):
            raise ValueError(f"frames are {self.width}x{self.height}, expected {size[0]}x{size[1]}")

    @staticmethod
    def _buffer(shape, dtype=np.uint8):
        """Frames are read straight into page-locked memory when the library is there: the tracker's uploads then run
        at the PCIe rate instead of the pageable-copy rate."""
        try:
            from ._native import pinned_empty
            return pinned_empty(shape, dtype)
        except Exception:
            return np.empty(shape, dtype)

    @staticmethod
    def _read_image(path):
        from PIL import Image
        with Image.open(path) as im:
            return np.asarray(im.convert("RGB"), np.uint8)

    def __len__(self):
        return self._n

    @property
    def size(self):
        return (self.width, self.height)

    def read(self, start, stop):
        """Frames [start, stop) as one contiguous array (n, H, W, 3) -- 4:2:0: (n, H * 3 // 2, W); 4:2:2: (n, H, W, 2)."""
        start, stop = max(0, start), min(self._n, stop)
        out = self._buffer((max(stop - start, 0),) + self._tail) if self._dtype == np.uint8 else \
            self._buffer((max(stop - start, 0),) + self._tail, np.uint16)
        if self._files is None:
            out[...] = self._array[start:stop]
            return out
        for i in range(start, stop):
            img = self._read_image(self._files[i])
            if img.shape != out.shape[1:]:
                raise ValueError(f"{self._files[i]}: {img.shape[1]}x{img.shape[0]}, expected {self.width}x{self.height}")
            out[i - start] = img
        return out

    def __iter__(self):
        for i in range(self._n):
            yield self.read(i, i + 1)[0]


class FrameSink:
    """Where processed frames go.  Directories get `frame_000000.png`, ...; `.npy` needs `n` up front.  `pixel_format` 'nv12' /
    'i420': frames of shape (H * 3 // 2, W) into a raw 4:2:0 file (`.nv12`, `.i420` / `.yuv`); 'yuy2' / 'uyvy': frames of shape
    (H, W, 2) into a raw packed 4:2:2 file (`.yuy2`, `.uyvy`); 'bgr' / 'rgba' / 'bgra': frames of shape (H, W, 3) / (H, W, 4) into
    a raw file of that name (`.bgr`, `.rgba`, `.bgra`)."""

    def __init__(self, path, size, n=None, pixel_format="rgb"):
        self.path = str(path)
        self.width, self.height = int(size[0]), int(size[1])
        self.count = 0
        self._raw = None
        self._array = None
        self._tail = (self.height, self.width, 3)
        if pixel_format != "rgb":
            if _yuv_layout(self.path) != pixel_format:
                raise ValueError("%s frames go into a raw file named *.%s, got %s" % (pixel_format, pixel_format, self.path))
            self._tail = _yuv_tail(pixel_format, self.width, self.height)[0]
            self._raw = open(self.path, "wb")
        elif self.path.lower().endswith(".npy"):
            if n is None:
                raise ValueError(".npy output needs the number of frames")
            self._array = np.lib.format.open_memmap(self.path, "w+", np.uint8, (int(n), self.height, self.width, 3))
        elif _is_raw(self.path):
            self._raw = open(self.path, "wb")
        else:
            os.makedirs(self.path, exist_ok=True)

    def write(self, frames):
        frames = np.asarray(frames, np.uint8)
        if frames.ndim == len(self._tail):
            frames = frames[None]
        if frames.shape[1:] != self._tail:
            raise ValueError(f"sink takes frames of shape {self._tail}, got {frames.shape[1:]}")
        if self._array is not None:
            self._array[self.count:self.count + len(frames)] = frames
        elif self._raw is not None:
            self._raw.write(np.ascontiguousarray(frames).tobytes())
        else:
            from PIL import Image
            for k, f in enumerate(frames):
                Image.fromarray(f).save(os.path.join(self.path, "frame_{:06d}.png".format(self.count + k)))
        self.count += len(frames)

    def close(self):
        if self._raw is not None:
            self._raw.close()
            self._raw = None
        if self._array is not None:
            self._array.flush()
            self._array = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def process_frames(tracker, source, sink=None, window=64, viz_sink=None, out_format=None, out_yuv_matrix="bt601", **process_kwargs):
    """Run every frame of `source` through the tracker, in order, `window` frames per GPU batch; write the
    annotated frames to `sink` if there is one -- the split views with `split_view=True` among the keywords, for a sink of
    that size -- and the search visualisations (bird's-eye size; `visualize_search=True` is set) to `viz_sink` if there
    is one.  `out_format` ('rgb', 'bgr', 'rgba', 'bgra', 'nv12', 'i420'): the annotated frames leave through device sinks in that pixel format
    (`process_stream(..., out=)`; 4:2:0 converted on the device with `out_yuv_matrix`) and `sink` receives what the sinks hold.
    Returns (frames, seconds)."""
    t0 = time.perf_counter()
    n = len(source)
    want, have = getattr(source, "pixel_format", "rgb"), getattr(tracker, "pixel_format", "rgb")
    if want != have:
        raise ValueError("the source delivers %r frames, the tracker was built with pixel_format=%r" % (want, have))
    windows = (source.read(start, start + window) for start in range(0, n, window))
    # process_stream: the uploads and masks of window k+1 run while the searches of window k drain
    if viz_sink is not None:
        process_kwargs = dict(process_kwargs, visualize_search=True)
    if out_format is not None:
        if sink is None or viz_sink is not None:
            raise ValueError("out_format writes the annotated frames: it needs a sink, and no visualisation sink")
        from .device import DeviceFrames
        # (a tracker with an input size hands out frames of its own img_size, not of the source's)
        out_size = tuple(int(v) for v in tracker.img_size) if getattr(tracker, "input_size", None) is not None else source.size
        sinks = (DeviceFrames.empty(min(window, n - start), out_size, out_format, device=tracker.device) for start in range(0, n, window))
        for out in tracker.process_stream(windows, annotate=True, out=sinks, out_yuv_matrix=out_yuv_matrix, **process_kwargs):
            for f in out:                # one-frame DeviceFrames of the window's sink
                sink.write(f.to_host())
            if out:
                out[0].owner.close()
        return n, time.perf_counter() - t0
    for out in tracker.process_stream(windows, annotate=sink is not None, **process_kwargs):
        if process_kwargs.get("visualize_search"):        # (annotated frame or None, picture) per frame
            pictures = [p if p.ndim == 3 else np.repeat(p[:, :, None], 3, axis=2) for _, p in out]
            out = [a for a, _ in out]
            if viz_sink is not None:
                viz_sink.write(np.stack(pictures, 0))
        if sink is not None:
            sink.write(np.stack(out, 0))
    return n, time.perf_counter() - t0


class VideoFileClip:
    """The slice of `moviepy.editor.VideoFileClip` that process_video.py touches (`:41-44`), over frame
    sequences: `clip.fl_image(fn)` returns a lazy clip, `write_videofile(path)` evaluates it.  When `fn`
    is the bound `process` of a `lane_tracker_amd` LaneTracker, evaluation goes through `process_stream`
    windows instead of one call per frame (same frames, higher throughput)."""

    def __init__(self, filename, size=None, fps=25.0, _fn=None, _source=None):
        self.filename = filename
        self.fps = fps
        self._source = _source if _source is not None else FrameSource(resolve_clip_path(filename), size)
        self._fn = _fn
        self.size = self._source.size
        self.pixel_format = self._source.pixel_format     # what a tracker for this clip is built with

    def fl_image(self, image_func):
        return VideoFileClip(self.filename, fps=self.fps, _fn=image_func, _source=self._source)

    def iter_frames(self):
        for f in self._source:
            yield f if self._fn is None else self._fn(f)

    def write_videofile(self, filename, audio=False, window=64, **_ignored):
        from .lane_tracker import LaneTracker
        fn = self._fn
        tracker = getattr(fn, "__self__", None)
        n = len(self._source)
        with FrameSink(resolve_clip_path(filename, must_exist=False), self.size, n=n) as sink:
            if isinstance(tracker, LaneTracker) and getattr(fn, "__func__", None) is LaneTracker.process:
                process_frames(tracker, self._source, sink, window=window)
            else:
                for f in self.iter_frames():
                    sink.write(f)
        return filename


def _parse_size(text):
    w, h = text.lower().split("x")
    return int(w), int(h)


def _parse_gains(text):
    try:
        g = tuple(float(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError("gains are numbers R,G,B or R,Gr,Gb,B, got %r" % (text,)) from None
    if len(g) not in (3, 4):
        raise argparse.ArgumentTypeError("gains are R,G,B or R,Gr,Gb,B, got %d values" % len(g))
    return g


def _parse_gamma(text):
    if text == "srgb":
        return text
    try:
        return float(text)
    except ValueError:
        raise argparse.ArgumentTypeError("gamma is a positive number or 'srgb', got %r" % (text,)) from None


def _parse_ccm(text):
    try:
        m = tuple(float(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError("a colour-correction matrix is nine numbers m00,...,m22, got %r" % (text,)) from None
    if len(m) != 9:
        raise argparse.ArgumentTypeError("a colour-correction matrix is nine numbers m00,...,m22 (row-major), got %d values" % len(m))
    return (m[0:3], m[3:6], m[6:9])


def main(argv=None):
    ap = argparse.ArgumentParser(description="Lane tracking over a frame sequence (process_video.py without moviepy)")
    ap.add_argument("input", help="directory of images, .npy (n,H,W,3), raw .rgb / .bgr / .rgba / .bgra, raw 4:2:0 (.nv12, .i420 / .yuv) or raw packed 4:2:2 (.yuy2, .uyvy)")
    ap.add_argument("output", help="directory (PNG), .npy or raw .rgb; '-' to discard the frames")
    ap.add_argument("--cam", default="cam_calib.p", help="camera calibration (.p pickle or .npz)")
    ap.add_argument("--warp", default="warp_params.p", help="warp parameters (.p pickle or .npz)")
    ap.add_argument("--size", type=_parse_size, default=None, help="WxH of raw input frames")
    ap.add_argument("--input-size", type=_parse_size, default=None,
                    help="WxH of the input frames when that is not the calibration's size: raw RGB input is read in this size and the "
                         "tracker resizes the frames on the device (cv2.resize, INTER_LINEAR); what is written has the calibration's size")
    ap.add_argument("--window", type=int, default=64, help="frames per GPU batch")
    ap.add_argument("--pixel-format", choices=("rgb", "nv12", "i420", "yuy2", "uyvy") + _RGB_FAMILY + _RAW_ALL, default=None,
                    help="pixel format of the input frames (default: by the input's name); must match a raw input's extension; a raw "
                         ".bayer input needs it: bayer_rggb / bayer_grbg / bayer_gbrg / bayer_bggr, the sensor's pattern; a raw .bayer16 input (10- / 12-bit samples in "
                         "little-endian 16-bit words) needs depth and pattern: bayer10_rggb ... bayer12_bggr; a raw .bayer10p / .bayer12p input (MIPI-packed rows) "
                         "needs the pattern, with the suffix's depth: bayer10p_rggb ... / bayer12p_rggb ...")
    ap.add_argument("--yuv-matrix", choices=("bt601", "bt709"), default="bt601", help="conversion matrix of 4:2:0 / 4:2:2 input")
    ap.add_argument("--raw-black-level", type=float, default=None, metavar="N", help="raw Bayer input: the sensor's black pedestal, in sample values (default 0)")
    ap.add_argument("--raw-white-level", type=float, default=None, metavar="N", help="raw Bayer input: the sample value of full scale (default 255; 1023 / 4095 for 10- / 12-bit input)")
    ap.add_argument("--raw-gains", type=_parse_gains, default=None, metavar="R,G,B[,..]",
                    help="raw Bayer input: white-balance gains R,G,B or R,Gr,Gb,B (default 1,1,1)")
    ap.add_argument("--raw-gamma", type=_parse_gamma, default=None, metavar="G|srgb", help="raw Bayer input: tone curve, v ** (1 / G) or the sRGB encoding (default 1)")
    ap.add_argument("--raw-ccm", type=_parse_ccm, default=None, metavar="m00,...,m22",
                    help="raw Bayer input: colour-correction matrix applied after the demosaic, nine numbers row-major (sensor RGB to display "
                         "RGB; rounded to Q10, each row's sum kept)")
    ap.add_argument("--raw-out-gamma", type=_parse_gamma, default=None, metavar="G|srgb",
                    help="raw Bayer input: output curve applied after the matrix, v ** (1 / G) or the sRGB encoding (with it, keep --raw-gamma at 1)")
    ap.add_argument("--raw-shading", default=None, metavar="FILE.npy",
                    help="raw Bayer input: lens-shading correction from a mesh of float gains, an .npy array (mh, mw) or (4, mh, mw) -- R, Gr, "
                         "Gb, B --, 2 .. 64 nodes a side, corner nodes on the image's corners; the pedestal is --raw-black-level")
    ap.add_argument("--out-format", choices=("rgb", "nv12", "i420") + _RGB_FAMILY, default=None,
                    help="write the annotated frames through a device sink in this pixel format: a raw .rgb / .nv12 / .i420 file for "
                         "4:2:0 (converted on the device, --out-yuv-matrix), a raw .bgr / .rgba / .bgra file (permuted on the device, "
                         "alpha 255); default: RGB frames brought back by the host")
    ap.add_argument("--out-yuv-matrix", choices=("bt601", "bt709"), default="bt601", help="conversion matrix of 4:2:0 output")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--frame-count", action="store_true", help="print the frame number onto each image")
    ap.add_argument("--settings", choices=("default", "demo1", "demo2", "demo3"), default="default",
                    help="parameter set of tracker_settings.md (process() keywords + validity limits)")
    ap.add_argument("--split-view", action="store_true",
                    help="write split views: the annotated frame above the bird's-eye image and the search visualisation")
    ap.add_argument("--visualize-search", metavar="DIR", default=None,
                    help="a second sink (directory, .npy or raw .rgb) for the search visualisations, bird's-eye size")
    a = ap.parse_args(argv)
    raw = {k: v for k, v in (("black_level", a.raw_black_level), ("white_level", a.raw_white_level), ("gains", a.raw_gains),
                             ("gamma", a.raw_gamma)) if v is not None}
    if raw and a.pixel_format not in _RAW_ALL:
        ap.error("--raw-black-level / --raw-white-level / --raw-gains / --raw-gamma condition raw Bayer samples: they need --pixel-format bayer_*")
    raw_table = None
    if raw:
        from .utils import raw_lut
        try:
            raw_table = raw_lut(**raw) if a.pixel_format in _BAYER else raw_lut(bits=_raw_format_bits(a.pixel_format), **raw)
        except ValueError as e:
            ap.error(str(e))
    if (a.raw_ccm is not None or a.raw_out_gamma is not None) and a.pixel_format not in _RAW_ALL:
        ap.error("--raw-ccm / --raw-out-gamma follow the demosaic of raw Bayer frames: they need --pixel-format bayer_*")
    raw_matrix = raw_out_curve = None
    try:
        if a.raw_ccm is not None:
            from .utils import raw_ccm
            raw_matrix = raw_ccm(a.raw_ccm)
        if a.raw_out_gamma is not None:
            from .utils import raw_curve
            raw_out_curve = raw_curve(a.raw_out_gamma)
    except ValueError as e:
        ap.error(str(e))
    raw_shade = None
    if a.raw_shading is not None:
        if a.pixel_format not in _RAW_ALL:
            ap.error("--raw-shading corrects raw Bayer samples: it needs --pixel-format bayer_*")
        import numpy as np
        from .utils import raw_shading
        try:
            raw_shade = raw_shading(np.load(a.raw_shading, allow_pickle=False), black_level=int(round(a.raw_black_level or 0)),
                                    bits=8 if a.pixel_format in _BAYER else _raw_format_bits(a.pixel_format))
        except (OSError, ValueError) as e:
            ap.error("--raw-shading %s: %s" % (a.raw_shading, e))
    if a.split_view and a.output == "-":
        ap.error("--split-view shows the annotated frames: it needs an output")
    if a.split_view and a.visualize_search:
        ap.error("--split-view and --visualize-search are two runs: process() returns one or the other")
    if a.out_format is not None and (a.split_view or a.visualize_search or a.output == "-"):
        ap.error("--out-format writes the annotated frames through a device sink: it needs an output, and neither --split-view nor --visualize-search")
    if a.out_format in ("nv12", "i420") + _RGB_FAMILY and _yuv_layout(a.output) != a.out_format:
        ap.error("--out-format %s needs an output file named *.%s" % (a.out_format, a.out_format))
    from . import _native
    from .lane_tracker import LaneTracker
    from .utils import load_camera_calib, load_warp_params
    cam_matrix, dist_coeffs = load_camera_calib(a.cam)
    M, Minv, image_wh, warped_wh, mppv, mpph = load_warp_params(a.warp)
    if a.input_size is not None and a.size is not None and tuple(a.size) != tuple(a.input_size):
        ap.error("--size %dx%d and --input-size %dx%d name two sizes for the input frames" % (tuple(a.size) + tuple(a.input_size)))
    try:
        src = FrameSource(a.input, a.input_size or a.size or image_wh, pixel_format=a.pixel_format if a.pixel_format in _RAW_ALL else None)
    except ValueError as e:
        if not (_is_bayer_file(a.input) or _is_bayer16_file(a.input) or _packed_file_bits(a.input) or a.pixel_format in _RAW_ALL):
            raise
        ap.error(str(e))
    if a.pixel_format is not None and a.pixel_format != src.pixel_format:
        ap.error("--pixel-format %s, but %s holds %s frames" % (a.pixel_format, a.input, src.pixel_format))
    lt = LaneTracker(img_size=image_wh, warped_size=warped_wh, cam_matrix=cam_matrix, dist_coeffs=dist_coeffs,
                     warp_matrices=(M, Minv), mpp_conversion=(mppv, mpph), n_fail=8, n_reset=4, n_average=2,
                     print_frame_count=a.frame_count, device=a.device, pixel_format=src.pixel_format, yuv_matrix=a.yuv_matrix,
                     input_size=a.input_size, raw_lut=raw_table, raw_ccm=raw_matrix, raw_curve=raw_out_curve, raw_shading=raw_shade)
    try:
        out_size = src.size if a.input_size is None else tuple(int(v) for v in image_wh)
        if a.split_view:                 # the annotated frame on top, the pane strip below it
            out_size = (out_size[0], out_size[1] + _native.split_panes_size(out_size, warped_wh)[1])
        sink = None if a.output == "-" else FrameSink(a.output, out_size, n=len(src), pixel_format=a.out_format or "rgb")
        viz_sink = FrameSink(a.visualize_search, warped_wh, n=len(src)) if a.visualize_search else None
        kw = {}
        if a.settings != "default":
            from . import settings
            kw = settings.apply(lt, settings.DEMOS[a.settings])
        if a.split_view:
            kw["split_view"] = True
        n, dt = process_frames(lt, src, sink, window=a.window, viz_sink=viz_sink, out_format=a.out_format, out_yuv_matrix=a.out_yuv_matrix, **kw)
        for s_ in (sink, viz_sink):
            if s_ is not None:
                s_.close()
        ratio, success, total = lt.get_success_ratio() if lt.counter else (0.0, 0, 0)
        print("Frames: {}  ({:.1f} frames/s including I/O)".format(n, n / dt if dt > 0 else 0.0))
        print("Success ratio: ", ratio)
        print("Success absolute: ", success)
        print("Total frames: ", total)
    finally:
        lt.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
