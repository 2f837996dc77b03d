"""Frames that are already in device memory, the part that needs no GPU: how `DeviceFrames` reads a `__cuda_array_interface__`
(pointers, pitches, what it refuses), its slicing arithmetic against NumPy views of a host array with the same strides, the
packing of host frames into pitched surfaces, and the new names at the C boundary."""
import os
import re

import numpy as np
import pytest

from lane_tracker_amd import _native
from lane_tracker_amd.device import DeviceFrames, pack_host_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 0x7f0000001000          # a made-up device address: nothing here dereferences it


def _iface(shape, strides=None, ptr=BASE, typestr="|u1", version=3, **more):
    d = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": version, "strides": strides}
    d.update(more)
    return d


class _Holder:
    def __init__(self, iface):
        self.__cuda_array_interface__ = iface


def _host_like(shape, strides, ptr=BASE):
    """A host array with these strides whose element addresses, relative to its own base, are those of the device array."""
    need = sum((n - 1) * s for n, s in zip(shape, strides)) + 1
    raw = np.zeros(need, np.uint8)
    return np.lib.stride_tricks.as_strided(raw, shape=shape, strides=strides), raw.ctypes.data - ptr


def _addr(view, delta):
    return view.__array_interface__["data"][0] - delta


# ---- __cuda_array_interface__ -> surfaces --------------------------------------------------------------------------------------
def test_rgb_dense_pitched_single_and_sliced():
    H, W = 6, 8
    f = DeviceFrames.from_cuda_array(_Holder(_iface((4, H, W, 3))), "rgb")
    assert len(f) == 4 and f.img_size == (W, H) and f.shape == (4, H, W, 3) and not f.single
    assert [int(p) for p in f.surfaces["plane"][:, 0]] == [BASE + k * H * W * 3 for k in range(4)]
    assert set(f.surfaces["pitch"]) == {W * 3}
    # pitched rows, and a frame stride that is not the frame's bytes (a slice [::2] of a batch)
    pitch, fs = W * 3 + 20, 2 * H * (W * 3 + 20)
    f = DeviceFrames.from_cuda_array(_iface((3, H, W, 3), (fs, pitch, 3, 1)), "rgb")      # (the dict itself is taken too)
    assert [int(p) for p in f.surfaces["plane"][:, 0]] == [BASE + k * fs for k in range(3)] and set(f.surfaces["pitch"]) == {pitch}
    # one frame
    f = DeviceFrames.from_cuda_array(_iface((H, W, 3), (pitch, 3, 1)), "rgb")
    assert f.single and len(f) == 1 and f.shape == (H, W, 3) and int(f.surfaces["plane"][0, 0]) == BASE
    # a column crop: odd base, the pitch of the frame it was cut from
    x0, full = 3, 40
    f = DeviceFrames.from_cuda_array(_iface((2, H, W, 3), (H * full * 3, full * 3, 3, 1), ptr=BASE + 3 * x0), "rgb")
    assert int(f.surfaces["plane"][0, 0]) == BASE + 9 and int(f.surfaces["plane"][0, 0]) % 2 == 1
    assert set(f.surfaces["pitch"]) == {full * 3}


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_yuv_planes_follow_the_array(layout):
    H, W = 8, 12
    f = DeviceFrames.from_cuda_array(_iface((3, H * 3 // 2, W)), layout)
    assert f.img_size == (W, H) and f.shape == (3, H * 3 // 2, W)
    fb = H * W * 3 // 2
    for k in range(3):
        y, u, v = (int(p) for p in f.surfaces["plane"][k])
        assert y == BASE + k * fb and u == y + H * W
        assert v == (0 if layout == "nv12" else u + H * W // 4)
    assert set(f.surfaces["pitch"]) == {W} and set(f.surfaces["chroma_pitch"]) == {W if layout == "nv12" else W // 2}
    one = DeviceFrames.from_cuda_array(_iface((H * 3 // 2, W)), layout)
    assert one.single and one.shape == (H * 3 // 2, W)
    if layout == "nv12":                 # pitched NV12: the UV rows follow the Y rows at the same pitch
        p = W + 64
        f = DeviceFrames.from_cuda_array(_iface((2, H * 3 // 2, W), (5000, p, 1)), layout)
        assert int(f.surfaces["plane"][1, 0]) == BASE + 5000 and int(f.surfaces["plane"][1, 1]) == BASE + 5000 + H * p
        assert set(f.surfaces["pitch"]) == {p} and set(f.surfaces["chroma_pitch"]) == {p}
    else:                                # pitched I420 has no single chroma pitch inside one 2-D array: from_planes is its form
        with pytest.raises(ValueError):
            DeviceFrames.from_cuda_array(_iface((2, H * 3 // 2, W), (5000, W + 64, 1)), layout)


@pytest.mark.parametrize("bad", [
    dict(typestr="<f4"), dict(typestr="|i1"),
    dict(shape=(6, 8)), dict(shape=(2, 2, 6, 8, 3)), dict(shape=(2, 6, 8, 4)),
    dict(strides=(6 * 8 * 6, 8 * 6, 6, 1)), dict(strides=(6 * 8 * 3, 8 * 3, 3, 2)),
    dict(strides=(6 * 8 * 3, -8 * 3, 3, 1)), dict(strides=(0, 8 * 3, 3, 1)), dict(strides=(6 * 8 * 3, 8 * 3 - 1, 3, 1)),
    dict(ptr=0), dict(version=1), dict(version=0),
], ids=lambda b: "%s=%s" % next(iter(b.items())))
def test_refused_rgb_interfaces(bad):
    kw = dict(shape=(2, 6, 8, 3), strides=(6 * 8 * 3, 8 * 3, 3, 1))
    kw.update(bad)
    with pytest.raises(ValueError):
        DeviceFrames.from_cuda_array(_iface(**kw), "rgb")


@pytest.mark.parametrize("shape", [(2, 9, 7), (2, 10, 8), (2, 9, 8, 3), (9,)], ids=str)      # odd width, rows not H * 3 / 2 with H even, wrong rank
@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_refused_yuv_interfaces(layout, shape):
    with pytest.raises(ValueError):
        DeviceFrames.from_cuda_array(_iface(shape), layout)
    with pytest.raises(ValueError):
        DeviceFrames.from_cuda_array(_iface((2, 9, 8), (72, 8, 2)), layout)      # a sample stride that is not 1
    with pytest.raises(ValueError):
        DeviceFrames.from_cuda_array(_iface((2, 9, 8)), "yuy2")
    with pytest.raises(ValueError):
        DeviceFrames.from_cuda_array(object(), layout)


def test_stream_entry_is_kept_for_the_attach():
    assert DeviceFrames.from_cuda_array(_iface((6, 8, 3), stream=2), "rgb").stream == 2
    assert DeviceFrames.from_cuda_array(_iface((6, 8, 3)), "rgb").stream is None
    with pytest.raises(ValueError):                                              # the protocol forbids 0
        DeviceFrames.from_cuda_array(_iface((6, 8, 3), stream=0), "rgb").wait_for_producer()
    DeviceFrames.from_cuda_array(_iface((6, 8, 3)), "rgb").wait_for_producer()   # nothing to wait for: no call, no GPU needed


# ---- slicing = NumPy's arithmetic -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [slice(None), slice(1, 5), slice(None, None, 2), slice(5, 1, -1), slice(-3, None), slice(4, 4), 0, 3, -1, -7],
                         ids=str)
def test_slicing_matches_numpy_views(idx):
    H, W, n = 4, 6, 7
    strides = (2 * H * (W * 3 + 5), W * 3 + 5, 3, 1)
    f = DeviceFrames.from_cuda_array(_iface((n, H, W, 3), strides), "rgb")
    host, delta = _host_like((n, H, W, 3), strides)
    got, want = f[idx], host[idx]
    if isinstance(idx, int):
        assert got.single and len(got) == 1 and got.shape == want.shape
        assert int(got.surfaces["plane"][0, 0]) == _addr(want, delta)
    else:
        assert not got.single and len(got) == len(want) and got.shape == want.shape
        assert [int(p) for p in got.surfaces["plane"][:, 0]] == [_addr(want[k], delta) for k in range(len(want))]
    assert got.owner is f.owner and got.img_size == f.img_size and got.pixel_format == "rgb"
    assert set(got.surfaces["pitch"]) <= {strides[1]}


def test_slicing_errors():
    f = DeviceFrames.from_cuda_array(_iface((3, 4, 6, 3)), "rgb")
    with pytest.raises(IndexError):
        f[3]
    with pytest.raises(IndexError):
        f[-4]
    with pytest.raises(TypeError):
        f[[0, 1]]
    assert len(f[1:][1:]) == 1 and int(f[1:][1:].surfaces["plane"][0, 0]) == BASE + 2 * 4 * 6 * 3


# ---- from_planes, pack_host_frames, the checks a tracker makes -------------------------------------------------------------------
def test_from_planes_takes_the_decoder_form():
    W, H = 16, 8
    f = DeviceFrames.from_planes([(BASE, BASE + 100000), (BASE + 4096, BASE + 200001)], (W, H), "nv12", pitch=[64, 80], chroma_pitch=[64, 96])
    assert len(f) == 2 and not f.single and list(f.surfaces["pitch"]) == [64, 80] and list(f.surfaces["chroma_pitch"]) == [64, 96]
    assert int(f.surfaces["plane"][1, 1]) == BASE + 200001 and int(f.surfaces["plane"][1, 2]) == 0
    one = DeviceFrames.from_planes((BASE, BASE + 1000, BASE + 2001), (W, H), "i420", pitch=W, chroma_pitch=W // 2 + 3)
    assert one.single and len(one) == 1 and one.shape == (H * 3 // 2, W)
    for kw in (dict(pitch=W - 1, chroma_pitch=W), dict(pitch=W, chroma_pitch=W - 2), dict(pitch=W), dict(pitch=1 << 23, chroma_pitch=W)):
        with pytest.raises(ValueError):
            DeviceFrames.from_planes([(BASE, BASE + 1000)], (W, H), "nv12", **kw)
    with pytest.raises(ValueError):
        DeviceFrames.from_planes([(BASE, 0)], (W, H), "nv12", pitch=W, chroma_pitch=W)
    with pytest.raises(ValueError):
        DeviceFrames.from_planes([(BASE, BASE + 1000)], (W + 1, H), "nv12", pitch=W + 1, chroma_pitch=W + 1)
    with pytest.raises(ValueError):
        one.check_for((W, H), "nv12")
    with pytest.raises(ValueError):
        one.check_for((W, H + 2), "i420")
    one.check_for((W, H), "i420")


@pytest.mark.parametrize("layout,pitch,cpitch", [("rgb", None, None), ("rgb", 8 * 3 + 20, None), ("nv12", 8 + 6, None), ("nv12", 8 + 64, 8 + 3),
                                                 ("i420", None, None), ("i420", 8 + 6, 4 + 5)])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_pack_host_frames_puts_every_byte_where_the_surfaces_say(layout, pitch, cpitch, offset):
    H, W, n = 6, 8, 3
    rng = np.random.default_rng(H * W + offset)
    frames = rng.integers(0, 256, (n, H, W, 3) if layout == "rgb" else (n, H * 3 // 2, W), dtype=np.uint8)
    block, surf, size, single = pack_host_frames(frames, layout, pitch, cpitch, offset, fill=0xA5)
    assert size == (W, H) and not single and len(surf) == n
    planes = [(H, W * 3)] if layout == "rgb" else [(H, W)] + [(H // 2, W if layout == "nv12" else W // 2)] * (1 if layout == "nv12" else 2)
    used = np.zeros(block.size, bool)
    for k in range(n):
        flat, at = frames[k].reshape(-1), 0
        for i, (rows, rb) in enumerate(planes):
            p = int(surf[k]["pitch" if i == 0 else "chroma_pitch"])
            for r in range(rows):
                a = int(surf[k]["plane"][i]) + r * p
                assert np.array_equal(block[a:a + rb], flat[at:at + rb]), (k, i, r)
                assert not used[a:a + rb].any()
                used[a:a + rb] = True
                at += rb
    assert (block[~used] == 0xA5).all() and used[-1] and int(surf[0]["plane"][0]) == offset      # the block ends with the last plane's last byte
    one = pack_host_frames(frames[0], layout, pitch, cpitch, offset)
    assert one[3] and len(one[1]) == 1
    with pytest.raises(ValueError):
        pack_host_frames(frames, layout, pitch=7)
    with pytest.raises(ValueError):
        pack_host_frames(frames.astype(np.float32), layout)


# ---- the C boundary ----------------------------------------------------------------------------------------------------------------
NEW_NAMES = ("lt_attach_device_frames", "lt_device_frames_rest", "lt_device_alloc", "lt_device_free", "lt_device_write", "lt_device_read",
             "lt_device_stream_wait")


def test_new_names_are_declared_exported_and_bound():
    import ctypes as C
    header = open(os.path.join(ROOT, "include", "lane_tracker_amd.h")).read()
    assert int(re.search(r"#define LT_ABI_VERSION (\d+)", header).group(1)) == 5 == _native.ABI_VERSION
    assert re.search(r"typedef struct lt_device_surface \{\s*const void\* plane\[3\];\s*int32_t pitch;[^}]*int32_t chroma_pitch;[^}]*\} lt_device_surface;", header)
    assert "lt_*" in open(os.path.join(ROOT, "lane_tracker_amd", "csrc", "exports.map")).read()
    lib = _native.load()
    for name in NEW_NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native.exported_symbols() and hasattr(lib, name), name
    assert lib.lt_abi_version() == 5
    assert C.sizeof(_native.DeviceSurface) == 32 == _native.SURFACE_DTYPE.itemsize
    assert _native.DeviceSurface.pitch.offset == 24 and _native.DeviceSurface.chroma_pitch.offset == 28


def test_null_arguments_are_errors_without_a_gpu():
    import ctypes as C
    lib = _native.load()
    s = np.zeros(1, _native.SURFACE_DTYPE)
    assert lib.lt_attach_device_frames(None, s.ctypes.data, 0, 1) == -1 and b"context" in lib.lt_last_error()
    assert lib.lt_attach_device_frames(None, None, 0, 1) == -1
    assert lib.lt_device_frames_rest(None, 0, 1, None) == -1
    out = C.c_void_p()
    assert lib.lt_device_alloc(0, 0, C.byref(out)) == -1 and not out.value
    assert lib.lt_device_alloc(0, 64, None) == -1
    assert lib.lt_device_free(None) == 0
    host = np.zeros(64, np.uint8)
    assert lib.lt_device_free(host.ctypes.data) == -1                           # not a block of the library: never passed on to the runtime
    assert lib.lt_device_write(host.ctypes.data, host.ctypes.data, 64) == -1    # a host address is not a device block
    assert lib.lt_device_read(host.ctypes.data, host.ctypes.data, 64) == -1 and b"lt_device_alloc" in lib.lt_last_error()
    assert lib.lt_device_stream_wait(0, 0) == -1
