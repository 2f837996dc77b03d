"""Camera frames that are already in device memory.

`DeviceBuffer` owns a block of device memory out of the library's own cache (lt_device_alloc); `DeviceFrames` DESCRIBES n frames of
one size and pixel format that lie somewhere in device memory -- plane pointers and row pitches per frame, nothing else -- and is
what `LaneTracker.process / process_batch / process_stream`, `LaneTrackerGroup.process` and `Context.attach_device_frames` take in
place of NumPy arrays.  Nothing is copied for a search-only call: the undistortion reads the surfaces where they lie.

The producer must live in the HIP runtime the library is linked against (a decoder linked against the system ROCm does; a
framework that bundles its own copy of the runtime does not): the library checks every pointer before it launches anything and
refuses what its runtime does not know.  No framework is imported here.
"""
import numpy as np

from . import _native
from ._native import (BAYER_FORMATS, BAYER_PACKED_FORMATS, BAYER_WIDE_FORMATS, RAW_FORMATS, SURFACE_DTYPE, frame_dtype, frame_shape, packed_row_bytes,
                      pixel_format_id, raw_bits)

__all__ = ["DeviceBuffer", "DeviceFrames", "pack_host_frames", "feed_rows_list", "feed_rest_list"]


class DeviceBuffer:
    """`nbytes` of device memory on `device`, owned: freed by close() (or the context manager, or the collector)."""

    def __init__(self, nbytes, device=0):
        import ctypes as C
        self.ptr = 0
        nbytes = int(nbytes)
        if nbytes <= 0:
            raise ValueError("a DeviceBuffer needs a positive size, got %d" % nbytes)
        out = C.c_void_p()
        _native._check(_native.load().lt_device_alloc(int(device), nbytes, C.byref(out)))
        self.ptr, self.nbytes, self.device = int(out.value), nbytes, int(device)

    def _range(self, offset, nbytes):
        offset, nbytes = int(offset), int(nbytes)
        if not self.ptr:
            raise ValueError("the DeviceBuffer is closed")
        if offset < 0 or nbytes < 0 or offset + nbytes > self.nbytes:
            raise ValueError("bytes [%d, %d) outside a DeviceBuffer of %d bytes" % (offset, offset + nbytes, self.nbytes))
        return offset, nbytes

    def copy_from_host(self, array, offset=0):
        a = np.ascontiguousarray(array)
        offset, n = self._range(offset, a.nbytes)
        if n:
            _native._check(_native.load().lt_device_write(self.ptr + offset, a.ctypes.data, n))
        return self

    def copy_to_host(self, nbytes=None, offset=0):
        offset, n = self._range(offset, self.nbytes - int(offset) if nbytes is None else nbytes)
        out = np.empty(n, np.uint8)
        if n:
            _native._check(_native.load().lt_device_read(out.ctypes.data, self.ptr + offset, n))
        return out

    @property
    def __cuda_array_interface__(self):
        if not self.ptr:
            raise ValueError("the DeviceBuffer is closed")
        return {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 3, "strides": None}

    def close(self):
        if self.ptr:
            p, self.ptr = self.ptr, 0
            _native._check(_native.load().lt_device_free(p))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _plane_rows(img_size, pixel_format):
    """-> ((rows, row bytes) of plane 0, (rows, row bytes) of each chroma plane or None, number of planes)."""
    w, h = int(img_size[0]), int(img_size[1])
    layout = pixel_format_id(pixel_format)
    frame_shape((w, h), pixel_format)                    # (ValueError for odd 4:2:0 sizes)
    if pixel_format in BAYER_PACKED_FORMATS:             # one plane of MIPI-packed samples: 5 W / 4 or 3 W / 2 bytes a row
        return (h, packed_row_bytes(pixel_format, w)), None, 1
    bpp = _PIXEL_BYTES.get(layout)
    if bpp:                                              # one plane of whole pixels: 3 W (RGB, BGR), 2 W (packed 4:2:2), 4 W (RGBA, BGRA) or W (raw Bayer) bytes a row
        return (h, bpp * w), None, 1
    return (h, w), ((h // 2, w) if layout == 1 else (h // 2, w // 2)), layout + 1


_PIXEL_BYTES = {0: 3, 3: 2, 4: 2, 5: 3, 6: 4, 7: 4, 16: 1, 17: 1, 18: 1, 19: 1}       # bytes a pixel of the layouts that are one plane of whole pixels
_PIXEL_BYTES.update({v: 2 for v in BAYER_WIDE_FORMATS.values()})                       # (10- / 12-bit raw Bayer: one 16-bit word)
_RAW_LAYOUTS = frozenset(RAW_FORMATS.values())


def _packed_width(pixel_format, row_bytes):
    """The width of a MIPI-packed row of `row_bytes` bytes (ValueError where that is no whole number of groups); any other format: the value itself."""
    if pixel_format not in BAYER_PACKED_FORMATS:
        return row_bytes
    per, of = (5, 4) if raw_bits(pixel_format) == 10 else (3, 2)
    if row_bytes % per:
        raise ValueError("a MIPI-packed %r row is W * %d // %d bytes, W a multiple of %d: got %d bytes" % (pixel_format, per, of, of, row_bytes))
    return row_bytes // per * of


def _check_word_planes(pixel_format, planes, pitches):
    """10- / 12-bit raw Bayer: a plane of 16-bit words lies at an even address and has an even pitch (the library checks the same)."""
    if pixel_format in BAYER_WIDE_FORMATS:
        if any(int(p) % 2 for p in np.asarray(pitches).reshape(-1)):
            raise ValueError("a plane of 16-bit samples needs an even pitch, got %r" % (np.asarray(pitches).reshape(-1).tolist(),))
        if any(int(p) % 2 for p in np.asarray(planes).reshape(-1)):
            raise ValueError("a plane of 16-bit samples needs an even address")


def _frame_dims(layout):
    """-> (dimensions of one frame's array, its last axis or 0): RGB / BGR (H, W, 3), RGBA / BGRA (H, W, 4), packed 4:2:2 (H, W, 2),
    4:2:0 (H * 3 // 2, W); raw Bayer (H, W): no last axis, 1 stands for it."""
    if layout in _RAW_LAYOUTS:
        return 2, 1
    return (3, _PIXEL_BYTES[layout]) if layout in _PIXEL_BYTES else (2, 0)


_SHAPE_NAMES = {3: "(H, W, 3)", 4: "(H, W, 4)", 2: "(H, W, 2)", 1: "(H, W)", 0: "(H * 3 // 2, W)"}


def _extent(rows, row_bytes, pitch):
    return pitch * (rows - 1) + row_bytes


def _layout_block(n, img_size, pixel_format, pitch, chroma_pitch, offset):
    """n frames of `img_size` as pitched surfaces in one block: frame after frame, plane after plane, every row `pitch` (chroma
    rows: `chroma_pitch`) bytes after the one before, the first at `offset`; the block ends with the last byte of the last plane.
    -> (bytes of the block, surfaces with plane OFFSETS into it, [(rows, row bytes, pitch) per plane])."""
    layout = pixel_format_id(pixel_format)
    (rows, rb), chroma, nplanes = _plane_rows(img_size, pixel_format)
    pitch = rb if pitch is None else int(pitch)
    if pitch < rb:
        raise ValueError("pitch %d is below the row's %d bytes" % (pitch, rb))
    sizes = [(rows, rb, pitch)]
    if chroma:
        default = pitch if layout == 1 else (pitch // 2 if pitch % 2 == 0 else chroma[1])
        cp = default if chroma_pitch is None else int(chroma_pitch)
        if cp < chroma[1]:
            raise ValueError("chroma pitch %d is below the row's %d bytes" % (cp, chroma[1]))
        sizes += [(chroma[0], chroma[1], cp)] * (nplanes - 1)
    offset = int(offset)
    if offset < 0:
        raise ValueError("offset must not be negative")
    frame_stride = sum(r * p for r, _, p in sizes)
    total = offset + n * frame_stride - (sizes[-1][2] - sizes[-1][1])
    surf = np.zeros(n, SURFACE_DTYPE)
    surf["pitch"] = pitch
    surf["chroma_pitch"] = sizes[1][2] if chroma else 0
    for k in range(n):
        at = offset + k * frame_stride
        for i, (r, _, p) in enumerate(sizes):
            surf["plane"][k, i] = at
            at += r * p
    return total, surf, sizes


def pack_host_frames(frames, pixel_format="rgb", pitch=None, chroma_pitch=None, offset=0, fill=0):
    """Host frames -- (n, H, W, 3) / (H, W, 3) ('rgb', 'bgr'), (n, H, W, 4) / (H, W, 4) ('rgba', 'bgra'), (n, H * 3 // 2, W) /
    (H * 3 // 2, W) for 4:2:0, (n, H, W, 2) / (H, W, 2) for packed 4:2:2, or (n, H, W) / (H, W) for raw Bayer -- laid out as pitched surfaces in
    one block: frame after frame, plane after plane, every row `pitch` (chroma rows: `chroma_pitch`) bytes after the one before,
    the first at `offset`; bytes between and around the rows are `fill`.  The block ends with the last byte of the last plane.
    -> (the block as a u8 array, surfaces with plane OFFSETS into it, img_size, whether `frames` was one frame)."""
    f = np.asarray(frames)
    layout = pixel_format_id(pixel_format)
    if f.dtype != frame_dtype(pixel_format):
        raise ValueError("%s, got %s" % ("camera frames are uint8" if f.dtype != np.uint16 and frame_dtype(pixel_format) == np.uint8
                                         else "%r camera frames are %s" % (pixel_format, frame_dtype(pixel_format)), f.dtype))
    nd, last = _frame_dims(layout)
    if f.ndim not in (nd, nd + 1) or (last > 1 and f.shape[-1] != last):
        raise ValueError("expected camera frames of shape %s, got %r" % (_SHAPE_NAMES[last], f.shape))
    single = f.ndim == nd
    f = f[None] if single else f
    if last:
        h, w = f.shape[1], _packed_width(pixel_format, f.shape[2])
    else:
        if f.shape[1] % 3:
            raise ValueError("a 4:2:0 frame is a 2-D array of shape (H * 3 // 2, W) with H and W even, got %r" % (f.shape[1:],))
        h, w = f.shape[1] // 3 * 2, f.shape[2]
    n = f.shape[0]
    total, surf, sizes = _layout_block(n, (w, h), pixel_format, pitch, chroma_pitch, offset)
    _check_word_planes(pixel_format, surf["plane"][:, 0], surf["pitch"])
    block = np.full(total, fill, np.uint8)
    flat = np.ascontiguousarray(f).view(np.uint8).reshape(n, -1)          # (16-bit samples: their bytes as they lie, little-endian)
    for k in range(n):
        src = 0
        for i, (r, b, p) in enumerate(sizes):
            dst = np.lib.stride_tricks.as_strided(block[int(surf["plane"][k, i]):], shape=(r, b), strides=(p, 1))
            dst[...] = flat[k, src:src + r * b].reshape(r, b)
            src += r * b
    return block, surf, (w, h), single


class DeviceFrames:
    """n camera frames of `img_size` = (width, height) in `pixel_format` somewhere in device memory: a description, not an owner
    (`owner` is whatever keeps the memory alive; it is only referenced).  `surfaces` is a SURFACE_DTYPE array, one entry per
    frame: plane pointers (RGB, BGR, RGBA, BGRA, YUY2, UYVY, raw Bayer: one; NV12: Y, UV; I420: Y, U, V), the pitch of plane 0 and the chroma pitch, in bytes.
    `single`: made from one frame (what process() takes); `stream`: the producer's stream to wait for before the frames are read;
    `readonly`: the producer said so (`__cuda_array_interface__`'s data[1]) -- such frames are never drawn into (`out="inplace"`)."""

    def __init__(self, surfaces, img_size, pixel_format, owner=None, single=False, stream=None, device=0, readonly=False):
        self.surfaces = surfaces
        self.img_size = (int(img_size[0]), int(img_size[1]))
        self.pixel_format = pixel_format
        self.owner, self.single, self.stream, self.device = owner, bool(single), stream, int(device)
        self.readonly = bool(readonly)

    # -- construction
    @classmethod
    def from_planes(cls, planes, img_size, pixel_format, pitch, chroma_pitch=None, owner=None, stream=None, device=0):
        """Explicit pointers: `planes` is one tuple of plane addresses per frame (RGB: (rgb,); NV12: (y, uv); I420: (y, u, v); YUY2 /
        UYVY: (plane,), pitch >= 2 W; BGR: (plane,), pitch >= 3 W; RGBA / BGRA: (plane,), pitch >= 4 W; raw Bayer: (plane,), pitch >= W) --
        or a single such tuple for one frame -- `pitch` / `chroma_pitch` the bytes between rows (one value, or one per frame)."""
        (rows, rb), chroma, nplanes = _plane_rows(img_size, pixel_format)
        single = len(planes) > 0 and not hasattr(planes[0], "__len__")
        rows_ = np.array([planes] if single else list(planes), dtype=np.uint64).reshape(-1, nplanes) if len(planes) else np.zeros((0, nplanes), np.uint64)
        n = rows_.shape[0]
        surf = np.zeros(n, SURFACE_DTYPE)
        surf["plane"][:, :nplanes] = rows_
        p = np.broadcast_to(np.asarray(pitch, dtype=np.int64), (n,))
        cp = np.broadcast_to(np.asarray(0 if chroma_pitch is None else chroma_pitch, dtype=np.int64), (n,))
        if (rows_ == 0).any():
            raise ValueError("a plane pointer is null")
        if n and p.min() < rb:
            raise ValueError("pitch %d is below the row's %d bytes" % (p.min(), rb))
        if chroma:
            if chroma_pitch is None:
                raise ValueError("4:2:0 surfaces need a chroma pitch")
            if n and cp.min() < chroma[1]:
                raise ValueError("chroma pitch %d is below the row's %d bytes" % (cp.min(), chroma[1]))
        if n and max(p.max(), cp.max()) >= 1 << 23:
            raise ValueError("pitches must stay below 2**23")
        _check_word_planes(pixel_format, rows_, p)
        surf["pitch"], surf["chroma_pitch"] = p, cp
        return cls(surf, img_size, pixel_format, owner=owner, single=single, stream=stream, device=device)

    @classmethod
    def from_cuda_array(cls, obj, pixel_format="rgb", device=0):
        """Anything with `__cuda_array_interface__` (or the dict itself): '|u1', shape (n, H, W, 3) / (H, W, 3) for RGB and
        (n, H * 3 // 2, W) / (H * 3 // 2, W) for NV12 / I420 with dense planes, (n, H, W, 2) / (H, W, 2) for YUY2 / UYVY (strides
        (frame, pitch, 2, 1), pitch >= 2 W), (n, H, W, 3) / (H, W, 3) for BGR as for RGB, (n, H, W, 4) / (H, W, 4) for RGBA / BGRA
        (a pixel stride of 4: a `uint8` (H, W, 4) tensor), (n, H, W) / (H, W) for raw Bayer (strides (frame, pitch, 1), pitch >= W);
        row and frame strides come from `strides`."""
        ai = obj if isinstance(obj, dict) else getattr(obj, "__cuda_array_interface__", None)
        if not isinstance(ai, dict):
            raise ValueError("the object has no __cuda_array_interface__")
        if int(ai.get("version", 0)) < 2:
            raise ValueError("__cuda_array_interface__ version %r is not supported (2 or later)" % (ai.get("version"),))
        word = pixel_format in BAYER_WIDE_FORMATS          # 10- / 12-bit raw Bayer: '<u2', strides (frame, pitch, 2)
        if word and ai.get("typestr") != "<u2":
            raise ValueError("%r camera frames are little-endian uint16 ('<u2'), got typestr %r" % (pixel_format, ai.get("typestr"),))
        if not word and ai.get("typestr") != "|u1":
            raise ValueError("camera frames are uint8 ('|u1'), got typestr %r" % (ai.get("typestr"),))
        if ai.get("mask") is not None:
            raise ValueError("masked arrays are not supported")
        shape = tuple(int(v) for v in ai["shape"])
        layout = pixel_format_id(pixel_format)
        nd, last = _frame_dims(layout)
        if len(shape) not in (nd, nd + 1) or (last > 1 and shape[-1] != last):
            raise ValueError("expected camera frames of shape %s, got %r" % (_SHAPE_NAMES[last], shape))
        if any(v <= 0 for v in shape[-nd:]):
            raise ValueError("empty camera frames: shape %r" % (shape,))
        strides = ai.get("strides")
        if strides is None:
            strides, acc = [], 2 if word else 1
            for v in reversed(shape):
                strides.insert(0, acc)
                acc *= v
        strides = tuple(int(v) for v in strides)
        if len(strides) != len(shape) or any(v <= 0 for v in strides):
            raise ValueError("strides must be positive, one per dimension: got %r" % (strides,))
        data = ai.get("data")
        ptr = int(data[0]) if data and data[0] is not None else 0
        if not ptr:
            raise ValueError("the data pointer is null")
        single = len(shape) == nd
        n, fstride = (1, 0) if single else (shape[0], strides[0])
        if last in (3, 4):
            h, w = shape[-3], shape[-2]
            if strides[-1] != 1 or strides[-2] != last:
                raise ValueError("%s frames are interleaved: a pixel stride of %d and a channel stride of 1, got %r"
                                 % ("RGB" if layout == 0 else pixel_format.upper(), last, strides[-2:]))
            pitch = strides[-3]
        elif last == 2:
            h, w = shape[-3], shape[-2]
            if strides[-1] != 1 or strides[-2] != 2:
                raise ValueError("4:2:2 frames are packed: a pixel stride of 2 and a sample stride of 1, got %r" % (strides[-2:],))
            pitch = strides[-3]
        elif last == 1:
            h, w = shape[-2], _packed_width(pixel_format, shape[-1])
            if word and strides[-1] != 2:
                raise ValueError("a %r plane holds one 16-bit word per pixel: a pixel stride of 2, got %d" % (pixel_format, strides[-1]))
            if not word and strides[-1] != 1:
                raise ValueError("a raw Bayer plane holds one byte per pixel: a pixel stride of 1, got %d" % strides[-1])
            pitch = strides[-2]
        else:
            if shape[-2] % 3:
                raise ValueError("a 4:2:0 frame is a 2-D array of shape (H * 3 // 2, W) with H and W even, got %r" % (shape[-2:],))
            h, w = shape[-2] // 3 * 2, shape[-1]
            if strides[-1] != 1:
                raise ValueError("4:2:0 planes hold one byte per sample: a sample stride of 1, got %d" % strides[-1])
            pitch = strides[-2]
        (rows, rb), chroma, nplanes = _plane_rows((w, h), pixel_format)
        if pitch < rb:
            raise ValueError("pitch %d is below the row's %d bytes" % (pitch, rb))
        if layout == 2 and pitch != w:
            raise ValueError("I420 through __cuda_array_interface__ needs dense planes (a row stride of %d, got %d): use from_planes" % (w, pitch))
        if pitch >= 1 << 23:
            raise ValueError("pitches must stay below 2**23")
        surf = np.zeros(n, SURFACE_DTYPE)
        base = ptr + np.arange(n, dtype=np.uint64) * np.uint64(fstride)
        _check_word_planes(pixel_format, base, pitch)
        surf["plane"][:, 0] = base
        surf["pitch"] = pitch
        if layout == 1:
            surf["plane"][:, 1] = base + np.uint64(h * pitch)
            surf["chroma_pitch"] = pitch
        elif layout == 2:
            surf["plane"][:, 1] = base + np.uint64(h * w)
            surf["plane"][:, 2] = base + np.uint64(h * w + (h // 2) * (w // 2))
            surf["chroma_pitch"] = w // 2
        return cls(surf, (w, h), pixel_format, owner=obj, single=single, stream=ai.get("stream"), device=device,
                   readonly=len(data) > 1 and bool(data[1]))

    @classmethod
    def from_host(cls, frames, pixel_format="rgb", pitch=None, chroma_pitch=None, offset=0, device=0):
        """Copies host frames into a fresh DeviceBuffer at the given pitches (pack_host_frames): for tests, tools and warm-up."""
        block, surf, size, single = pack_host_frames(frames, pixel_format, pitch, chroma_pitch, offset)
        buf = DeviceBuffer(block.nbytes, device).copy_from_host(block)
        nplanes = _plane_rows(size, pixel_format)[2]
        surf["plane"][:, :nplanes] += np.uint64(buf.ptr)
        return cls(surf, size, pixel_format, owner=buf, single=single, device=device)

    @classmethod
    def empty(cls, n, img_size, pixel_format="rgb", pitch=None, chroma_pitch=None, offset=0, fill=None, device=0):
        """A sink (packed 4:2:2: a container for input frames only, refused as a sink): n surfaces of `img_size` in `pixel_format` in a fresh DeviceBuffer it owns, laid out as pack_host_frames lays
        frames out (the block ends on the last byte of the last plane) -- what `Context.store_overlay_device`, `process_batch(...,
        out=)` and `utils.rgb_to_yuv` write into and `to_host()` reads back.  `fill`: a byte value the whole block is set to first
        (None: whatever the memory held)."""
        n = int(n)
        if pixel_format in RAW_FORMATS:
            raise ValueError("%r is an input format only: annotated frames go into 'rgb', 'bgr', 'rgba', 'bgra', 'nv12' or 'i420' surfaces" % (pixel_format,))
        if n < 0:
            raise ValueError("a sink holds zero or more frames, got %d" % n)
        size = (int(img_size[0]), int(img_size[1]))
        total, surf, _ = _layout_block(n, size, pixel_format, pitch, chroma_pitch, offset)
        nplanes = _plane_rows(size, pixel_format)[2]
        buf = None
        if n:
            buf = DeviceBuffer(total, device)
            if fill is not None:
                buf.copy_from_host(np.full(total, int(fill), np.uint8))
            surf["plane"][:, :nplanes] += np.uint64(buf.ptr)
        return cls(surf, size, pixel_format, owner=buf, device=device)

    # -- a sequence of frames
    def __len__(self):
        return len(self.surfaces)

    def __getitem__(self, idx):
        if isinstance(idx, (int, np.integer)):
            n = len(self.surfaces)
            if not -n <= idx < n:
                raise IndexError("frame %d of %d" % (idx, n))
            s, single = self.surfaces[int(idx) % n:int(idx) % n + 1], True
        elif isinstance(idx, slice):
            s, single = self.surfaces[idx], False
        else:
            raise TypeError("DeviceFrames take an integer or a slice, got %r" % (idx,))
        return DeviceFrames(s, self.img_size, self.pixel_format, owner=self.owner, single=single, stream=self.stream, device=self.device,
                            readonly=self.readonly)

    def select(self, indices):
        """The frames at `indices` (any order, as a list), as a window: what `frames[a:b]` is for a slice."""
        n = len(self.surfaces)
        idx = [int(i) for i in indices]
        for i in idx:
            if not -n <= i < n:
                raise IndexError("frame %d of %d" % (i, n))
        return DeviceFrames(self.surfaces[np.asarray(idx, np.intp)], self.img_size, self.pixel_format, owner=self.owner, single=False,
                            stream=self.stream, device=self.device, readonly=self.readonly)

    @property
    def shape(self):
        """The shape of the host array these frames would be."""
        tail = frame_shape(self.img_size, self.pixel_format)
        return tail if self.single else (len(self),) + tail

    def _plane_sizes(self):
        (rows, rb), chroma, nplanes = _plane_rows(self.img_size, self.pixel_format)
        return [(rows, rb, "pitch")] + ([(chroma[0], chroma[1], "chroma_pitch")] * (nplanes - 1) if chroma else [])

    def to_host(self):
        """The frames as a dense host array (memory of DeviceBuffers only: the library copies from its own blocks)."""
        import ctypes as C
        lib = _native.load()
        tail = frame_shape(self.img_size, self.pixel_format)
        out = np.empty((len(self), int(np.prod(tail)) * frame_dtype(self.pixel_format).itemsize), np.uint8)
        for k, s in enumerate(self.surfaces):
            at = 0
            for i, (rows, rb, which) in enumerate(self._plane_sizes()):
                pitch = int(s[which])
                raw = np.empty(_extent(rows, rb, pitch), np.uint8)
                _native._check(lib.lt_device_read(raw.ctypes.data, C.c_void_p(int(s["plane"][i])), raw.nbytes))
                out[k, at:at + rows * rb] = np.lib.stride_tricks.as_strided(raw, shape=(rows, rb), strides=(pitch, 1)).reshape(-1)
                at += rows * rb
        out = out.view(frame_dtype(self.pixel_format)).reshape((len(self),) + tail)
        return out[0] if self.single else out

    def wait_for_producer(self):
        """The host waits for the producer's stream, if the frames came with one (__cuda_array_interface__'s `stream`)."""
        if self.stream is not None:
            if int(self.stream) == 0:
                raise ValueError("__cuda_array_interface__: a stream of 0 is not allowed (1: legacy default, 2: per-thread default)")
            _native._check(_native.load().lt_device_stream_wait(self.device, int(self.stream)))

    def check_for(self, img_size, pixel_format):
        """ValueError unless these are frames of `img_size` in `pixel_format` (a tracker's or a context's)."""
        if self.pixel_format != pixel_format:
            raise ValueError("expected camera frames in pixel format %r, got DeviceFrames in %r" % (pixel_format, self.pixel_format))
        if self.img_size != (int(img_size[0]), int(img_size[1])):
            raise ValueError("expected camera frames of shape %r, got %r" % (frame_shape(img_size, pixel_format), frame_shape(self.img_size, self.pixel_format)))


def _runs(imgs):
    """Runs of consecutive entries of one kind: (first index, [entries], are they DeviceFrames?)."""
    a = 0
    while a < len(imgs):
        dev = isinstance(imgs[a], DeviceFrames)
        b = a + 1
        while b < len(imgs) and isinstance(imgs[b], DeviceFrames) == dev:
            b += 1
        yield a, imgs[a:b], dev
        a = b


def feed_rows_list(ctx, imgs, first):
    """Context.upload_frame_rows_list for a list whose entries are host arrays or one-frame DeviceFrames: frame k into (or
    attached to) slot first + k.  Returns what must stay alive until the work over these slots has been waited for."""
    keep = []
    for a, run, dev in _runs(imgs):
        if dev:
            for f in run:
                f.wait_for_producer()
            one = DeviceFrames(np.concatenate([f.surfaces for f in run]), run[0].img_size, run[0].pixel_format, owner=run, device=run[0].device)
            keep.append(ctx.attach_device_frames(one, first=first + a))
        else:
            keep.append(ctx.upload_frame_rows_list(run, first=first + a))
    return keep


def feed_rest_list(ctx, imgs, first):
    """Context.upload_frame_rest_list for such a list (the attached frames' rows are brought on the device)."""
    keep = []
    for a, run, dev in _runs(imgs):
        if dev:
            ctx.device_frames_rest(len(run), first=first + a)
        else:
            keep.append(ctx.upload_frame_rest_list(run, first=first + a))
    return keep
