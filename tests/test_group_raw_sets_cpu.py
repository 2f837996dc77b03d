"""Raw sets without a GPU: what LaneTrackerGroup(raw_setups=...) refuses before it touches the device, how streams share and split raw
sets, what the members report, the new names at the C boundary -- and the three identities a set-per-slot launch relies on for a set that
lacks a part of the union (the identity table, the matrix 1024 I with the identity curve, a plane of unit gains with pedestals 0), each
held to the NumPy definitions over random frames of all twelve raw formats.

The host bookkeeping of the union (raw_setup.h: raw_staged_as, raw_set_entry) is compiled with the system compiler and checked here too
(tests/raw_sets_host.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bayer_reference as RB
import fake_context
from lane_tracker_amd import _native, calib, group, utils
from lane_tracker_amd.group import LaneTrackerGroup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
NEW_NAMES = ("lt_add_raw_set", "lt_raw_set_count", "lt_set_slot_raw_sets", "lt_get_slot_raw_sets", "lt_set_raw_lut_of", "lt_get_raw_lut_of",
             "lt_set_raw_color_of", "lt_get_raw_color_of", "lt_set_raw_shading_of", "lt_get_raw_shading_of", "lt_get_raw_shading_plane_of",
             "lt_last_raw_walk_form")
RAW_FORMATS = [p for p in RB.PATTERNS] + ["bayer%d%s_%s" % (b, k, p[6:]) for b in (10, 12) for k in ("", "p") for p in RB.PATTERNS]


class _Ctx(fake_context.FakeContext):
    """The CPU stand-in as a raw Bayer context that holds raw sets: it records what every set holds and which set every slot was given."""
    made = 0

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        type(self).made += 1
        self.layout = "rgb"
        self.sets = [dict(lut=None, color=None, shading=None)]
        self.slot_sets = {}
        self.calls = []

    def set_input_format(self, pixel_format, matrix="bt601"):
        self.layout = pixel_format

    def add_raw_set(self):
        self.sets.append(dict(self.sets[0]))
        return len(self.sets) - 1

    def raw_set_count(self):
        return len(self.sets)

    def set_raw_lut(self, lut, raw_set=0):
        self.calls.append(("lut", raw_set))
        self.sets[raw_set]["lut"] = None if lut is None else lut.copy()

    def set_raw_color(self, ccm=None, curve=None, enable=True, raw_set=0):
        self.calls.append(("color", raw_set))
        self.sets[raw_set]["color"] = (ccm, curve) if enable else None

    def set_raw_shading(self, shading, raw_set=0):
        self.calls.append(("shading", raw_set))
        self.sets[raw_set]["shading"] = shading

    def set_slot_raw_sets(self, ids, first=0):
        for i, s in enumerate(ids):
            assert 0 <= s < len(self.sets)
            self.slot_sets[first + i] = int(s)

    def upload_frame_rows(self, frames, first=0, enqueue=False):
        f = np.asarray(frames).reshape(-1, self.img_h, self.img_w)
        return super().upload_frame_rows(RB.bayer_to_rgb(f, self.layout), first, enqueue)
    upload_frames = upload_frame_rows

    def upload_frame_rows_list(self, frames, first=0):
        for k, f in enumerate(frames):
            self.upload_frame_rows(f, first + k)
        return frames

    def search_fit_list(self, items, sws, band):
        for it in items:
            if it["mode"]:
                self.band_fit_run(1, it["prev_coeffs"], band, first=int(it["slot"]))
            else:
                self.sws_fit_run(1, sws, first=int(it["slot"]))


@pytest.fixture()
def fake(monkeypatch):
    monkeypatch.setattr(_native, "Context", _Ctx)
    _Ctx.made = 0
    return _Ctx


def _tables():
    rng = np.random.default_rng(4)
    return [rng.integers(0, 256, (4, 256), dtype=np.uint8) for _ in range(3)]


def _shading(k=0):
    return utils.raw_shading(np.full((4, 3, 3), 1.0 + 0.1 * k), black_level=4 + k)


# ---- 1. the constructor's checks -----------------------------------------------------------------------------------------------------------
def test_a_wrong_raw_setups_argument_is_refused_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device context was created")
    monkeypatch.setattr(_native, "Context", no_device)
    cal = calib.reference_calibration()
    t = _tables()
    kw = dict(cal, pixel_format="bayer_rggb")
    for bad, exc in (([None, {}], ValueError), ([None] * 4, ValueError), ([None, dict(raw_table=t[0]), None], ValueError),
                     ([None, dict(cam_matrix=np.eye(3)), None], ValueError), ([None, 3, None], TypeError), ([None, t[0], None], TypeError),
                     ([None, dict(raw_lut=t[0][:3]), None], ValueError), ([None, dict(raw_lut=t[0].astype(np.int16)), None], ValueError),
                     ([None, dict(raw_ccm=np.eye(2)), None], ValueError), ([None, dict(raw_curve=np.zeros(255, np.uint8)), None], ValueError),
                     ([None, dict(raw_shading=t[0]), None], (ValueError, TypeError))):
        with pytest.raises(exc):
            LaneTrackerGroup(3, **kw, raw_setups=bad)
    for fmt in ("rgb", "nv12", "yuy2", "bgra"):                    # not raw Bayer: refused, even a list of Nones
        with pytest.raises(ValueError, match="raw Bayer"):
            LaneTrackerGroup(3, **dict(cal, pixel_format=fmt), raw_setups=[None] * 3)
    with pytest.raises(ValueError, match=r"\(4, 4096\)|4096"):      # a 12-bit group takes 12-bit tables
        LaneTrackerGroup(3, **dict(cal, pixel_format="bayer12_rggb"), raw_setups=[None, dict(raw_lut=t[0]), None])
    with pytest.raises(AssertionError, match="device context"):
        LaneTrackerGroup(3, **kw, raw_setups=[None, dict(raw_lut=t[0]), {}])     # a good list gets as far as the device
    with pytest.raises(TypeError):
        LaneTrackerGroup(3, cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"],
                         cal["mpp_conversion"], 8, 4, 2, False, 0, [None] * 3)             # keyword only


# ---- 2. sharing, splitting, reporting ------------------------------------------------------------------------------------------------------
def test_streams_with_equal_setups_share_a_set(fake):
    cal = calib.reference_calibration()
    t, sh = _tables(), _shading()
    cams = [None, dict(raw_lut=t[1]), dict(raw_lut=t[1].copy()), {}, dict(raw_lut=t[0].copy()), dict(raw_lut=None, raw_shading=sh), dict(raw_shading=sh)]
    g = LaneTrackerGroup(7, **cal, pixel_format="bayer_gbrg", raw_lut=t[0], raw_setups=cams)
    try:
        assert fake.made == 1
        ids = g._raw_ids
        assert ids[0] == ids[3] == ids[4] == 0 and ids[1] == ids[2] != 0 and len({ids[1], ids[5], ids[6]}) == 3
        assert g.raw_set_count() == 4 == g._ctx.raw_set_count()
        s = g._ctx.sets
        assert np.array_equal(s[0]["lut"], t[0]) and np.array_equal(s[ids[1]]["lut"], t[1])
        assert s[ids[5]]["lut"] is None and s[ids[5]]["shading"] is sh or np.array_equal(s[ids[5]]["shading"].mesh, sh.mesh)
        assert np.array_equal(s[ids[6]]["lut"], t[0]) and s[ids[6]]["shading"] is not None and s[ids[1]]["shading"] is None
        # every member reports its own camera's values
        for i, want in enumerate((t[0], t[1], t[1], t[0], t[0], None, t[0])):
            got = g.trackers[i].raw_lut
            assert (got is None and want is None) or np.array_equal(got, want), i
        assert [m.raw_shading is not None for m in g.trackers] == [False] * 5 + [True, True]
        assert np.array_equal(g.raw_lut, t[0])
        # the context is told every tick which set each slot of the tick has, skipped streams left out
        W, H = cal["img_size"]
        frames = [np.zeros((H, W), np.uint8) if i != 2 else None for i in range(7)]
        g.process(frames, annotate=False)
        assert [g._ctx.slot_sets[k] for k in range(6)] == [ids[i] for i in range(7) if i != 2]
    finally:
        g.close()
    plain = LaneTrackerGroup(3, **cal, pixel_format="bayer_gbrg", raw_lut=t[0])
    try:
        assert plain.raw_set_count() == 1 and plain._ctx.raw_set_count() == 1 and plain._raw_ids == [0, 0, 0]
        plain.process([np.zeros((H, W), np.uint8)] * 3, annotate=False)
        assert plain._ctx.slot_sets == {}                          # one set: the context is never asked
    finally:
        plain.close()


def test_stream_i_splits_a_set_and_none_sets_all(fake):
    cal = calib.reference_calibration()
    t = _tables()
    m, c = utils.raw_ccm(np.eye(3) * 1.1), utils.raw_curve(1.0)
    g = LaneTrackerGroup(3, **cal, pixel_format="bayer_bggr", raw_lut=t[0], raw_setups=[None, None, dict(raw_ccm=m, raw_curve=c)])
    try:
        assert g._raw_ids == [0, 0, 1] and g.raw_set_count() == 2
        g.set_raw_lut(t[1], stream=1)                              # shared with stream 0: split off first
        assert g._raw_ids == [0, 2, 1] and g.raw_set_count() == 3
        assert np.array_equal(g._ctx.sets[2]["lut"], t[1]) and np.array_equal(g._ctx.sets[0]["lut"], t[0]) and np.array_equal(g._ctx.sets[1]["lut"], t[0])
        assert g._ctx.sets[2]["color"] is None and g._ctx.sets[1]["color"] is not None
        assert [np.array_equal(x.raw_lut, w) for x, w in zip(g.trackers, (t[0], t[1], t[0]))] == [True] * 3
        assert np.array_equal(g.raw_lut, t[0])                     # the group's own value is not one camera's
        n = len(g._ctx.sets)
        g.set_raw_lut(t[2], stream=1)                              # its own set now: changed in place
        assert len(g._ctx.sets) == n and np.array_equal(g._ctx.sets[2]["lut"], t[2]) and g._ctx.calls[-1] == ("lut", 2)
        g.set_raw_color(m, None, stream=0)
        assert g.trackers[0].raw_ccm is not None and g.trackers[1].raw_ccm is None and g._ctx.sets[0]["color"] is not None
        g.set_raw_shading(_shading(1), stream=2)
        assert [x.raw_shading is not None for x in g.trackers] == [False, False, True] and g._ctx.sets[1]["shading"] is not None
        # without a stream every camera changes, as it always did
        g.set_raw_lut(t[0])
        assert all(np.array_equal(s["lut"], t[0]) for k, s in enumerate(g._ctx.sets) if k in g._raw_ids)
        assert all(np.array_equal(x.raw_lut, t[0]) for x in g.trackers) and np.array_equal(g.raw_lut, t[0])
        g.set_raw_color(None, None)
        assert all(x.raw_ccm is None and x.raw_curve is None for x in g.trackers) and all(g._ctx.sets[k]["color"] is None for k in g._raw_ids)
        g.set_raw_shading(None)
        assert all(x.raw_shading is None for x in g.trackers)
        for bad in (-1, 3):
            with pytest.raises(ValueError, match="stream"):
                g.set_raw_lut(t[1], stream=bad)
        with pytest.raises(ValueError):
            g.set_raw_lut(t[1][:2], stream=0)
        for refused in (lambda: g.trackers[0].set_raw_lut(t[1]), lambda: g.trackers[0].set_raw_color(m, c), lambda: g.trackers[0].set_raw_shading(None),
                        lambda: g.trackers[0].raw_stats(np.zeros((4, 4), np.uint8))):
            with pytest.raises(RuntimeError):
                refused()
    finally:
        g.close()


def test_setup_keys_compare_bytes():
    t, sh = _tables(), _shading()
    own = dict(raw_lut=t[0], raw_ccm=None, raw_curve=None, raw_shading=None)
    full = group._stream_raw_setups([None, {}, dict(raw_lut=t[0].copy()), dict(raw_lut=None), dict(raw_shading=sh),
                                     dict(raw_shading=utils.RawShading(sh.mesh.copy(), sh.black.copy()))], 6, own, "bayer_rggb")
    keys = [group._raw_setup_key(s) for s in full]
    assert keys[0] == keys[1] == keys[2] and keys[3] != keys[0] and keys[4] == keys[5] != keys[0] and len(set(keys)) == 3
    assert full[3]["raw_lut"] is None
    wide = group._stream_raw_setups([None, dict(raw_lut=None)], 2, dict(own, raw_lut=None), "bayer10_rggb")
    assert np.array_equal(wide[1]["raw_lut"], utils.raw_lut(bits=10)) and group._raw_setup_key(wide[0]) == group._raw_setup_key(wide[1])


# ---- 3. the C boundary -----------------------------------------------------------------------------------------------------------------------
def test_new_names_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "lane_tracker_amd.h")).read()
    assert int(re.search(r"#define LT_ABI_VERSION (\d+)", header).group(1)) == 5 == _native.ABI_VERSION
    lib = _native.load()
    for name in NEW_NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native._SIGNATURES and name in _native.exported_symbols() and hasattr(lib, name), name
    for method in ("add_raw_set", "raw_set_count", "set_slot_raw_sets", "slot_raw_sets", "last_raw_walk_form"):
        assert callable(getattr(_native.Context, method))


def test_null_arguments_are_errors_without_a_gpu():
    lib = _native.load()
    i, ids, buf = C.c_int(0), np.zeros(2, np.int32), np.zeros(4096 * 4, np.uint16)
    assert lib.lt_add_raw_set(None, C.byref(i)) == -1 and lib.lt_raw_set_count(None, C.byref(i)) == -1
    assert lib.lt_set_slot_raw_sets(None, 0, 2, ids.ctypes.data) == -1 and b"context" in lib.lt_last_error()
    assert lib.lt_get_slot_raw_sets(None, 0, 2, ids.ctypes.data) == -1
    assert lib.lt_set_raw_lut_of(None, 0, buf.ctypes.data, 256) == -1 and lib.lt_get_raw_lut_of(None, 0, buf.ctypes.data, 256, C.byref(i)) == -1
    assert lib.lt_set_raw_color_of(None, 0, None, None, 1) == -1 and lib.lt_get_raw_color_of(None, 0, None, None, C.byref(i)) == -1
    assert lib.lt_set_raw_shading_of(None, 0, buf.ctypes.data, 2, 2, None, 1) == -1
    assert lib.lt_get_raw_shading_of(None, 0, None, None, None, None, C.byref(i)) == -1
    assert lib.lt_get_raw_shading_plane_of(None, 0, buf.ctypes.data) == -1
    assert lib.lt_last_raw_walk_form(None) == -1


# ---- 4. the identities of the union ---------------------------------------------------------------------------------------------------------
def _frames(fmt, rng, n=3, h=12, w=16):
    bits = _native.raw_bits(fmt)
    f = rng.integers(0, 1 << bits, (n, h, w), dtype=np.uint16)
    f[0] = 0
    f[1] = (1 << bits) - 1
    return f.astype(np.uint8) if bits == 8 else f


@pytest.mark.parametrize("fmt", RAW_FORMATS)
def test_the_identities_of_a_missing_part_are_exact(fmt):
    """What a set without a part runs in a launch whose union has it, in the NumPy definitions: nothing changes, for every sample value
    and every pedestal sign of s - B."""
    rng = np.random.default_rng(RAW_FORMATS.index(fmt))
    bits, word = _native.raw_bits(fmt), _native.unpacked_format(fmt)
    f = _frames(fmt, rng)
    fed = utils.pack_raw(f, fmt) if fmt in _native.BAYER_PACKED_FORMATS else f
    # the unit map: Q12 4096 everywhere, pedestals 0
    unit = utils.RawShading(np.full((4, 2, 2), 4096, np.uint16), np.zeros(4, np.int32))
    assert np.array_equal(utils.apply_raw_shading(f, word, unit), f)
    assert (utils.raw_shading_plane(unit, word, (16, 12)) == 4096).all()
    # ... and the arithmetic itself at any pedestal, below and above the sample: B + (((s - B) * 4096 + 2048) >> 12) == s
    s = np.arange(1 << bits, dtype=np.int64)
    for B in (0, 1, (1 << bits) // 16, (1 << bits) - 1):
        assert np.array_equal(B + (((s - B) * 4096 + 2048) >> 12), s)
        some = utils.RawShading(np.full((4, 2, 2), 4096, np.uint16), np.full(4, B, np.int32))
        assert np.array_equal(utils.apply_raw_shading(f, word, some), f)
    # the identity table (8 bits), in front of the demosaic
    if bits == 8:
        ident = np.tile(np.arange(256, dtype=np.uint8), (4, 1))
        assert np.array_equal(utils.raw_lut(), ident) and np.array_equal(utils.apply_raw_lut(f, fmt, ident), f)
    # the identity stage: 1024 I and the identity curve, (1024 v + 512) >> 10 == v
    cond = utils.apply_raw_lut(fed if bits > 8 else f, fmt, utils.raw_lut(bits=bits))
    rgb = RB.bayer_to_rgb(cond, "bayer_" + fmt.split("_")[1])
    eye = (np.eye(3) * 1024).astype(np.int16)
    for m, t in ((None, None), (eye, None), (None, np.arange(256, dtype=np.uint8)), (eye, np.arange(256, dtype=np.uint8))):
        assert np.array_equal(utils.apply_raw_color(rgb, m, t), rgb)
    v = np.arange(256, dtype=np.int64)
    assert np.array_equal((1024 * v + 512) >> 10, v)
    x = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    assert np.array_equal(utils.apply_raw_color(x, eye, None), x)


# ---- 5. the host bookkeeping, with the system compiler --------------------------------------------------------------------------------------
@pytest.mark.skipif(CXX is None, reason="no C++ compiler")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_union_bookkeeping_of_raw_setup_h(tmp_path, flags):
    exe = str(tmp_path / "raw_sets_host")
    subprocess.run([CXX, "-std=c++17", "-Wall", *flags, "-I", os.path.join(ROOT, "lane_tracker_amd", "csrc"), os.path.join(ROOT, "tests", "raw_sets_host.cpp"),
                    "-o", exe], check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok 192", out.stdout + out.stderr
