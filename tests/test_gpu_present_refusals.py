"""The same faulty call through every family of lane-drawing entry points -- lt_overlay_run_rows (annotated frames kept in the
context), lt_overlay_run_inplace (into the attached surfaces), lt_overlay_run_to_surfaces (into device sinks): each family answers
with the status code and the words it has always answered with, launches nothing and leaves the sink and the camera surfaces as
they were; then one good call per family, bit for bit against the host route of a twin context.

Two contexts of 64x48 with capacity 4: the twin is test_gpu_inplace_device._small_ctx; the context under test is made of the same
steps, spread out -- a second calibration set (never given an overlay) is added before the first upload, and the font is set only
after the calls that need a context without one.  Slots 0 and 1 are fed from the host (the rows and the sink family), slots 2 and
3 are attached to camera surfaces (the in-place family)."""
import ctypes as C

import numpy as np
import pytest

from lane_tracker_amd import _native
from test_gpu_inplace_device import FONT, TEXT_KW, TEXTS, _annotated, _expected_frames, _noise, _polygons, _small_ctx, _Surfaces

pytestmark = pytest.mark.gpu

SIZE = (64, 48)
OK, INVALID, STATE = 0, -1, -5


def _ptr(a):
    return None if a is None else a.ctypes.data


class _Families:
    """The three raw calls over two slots each, with everything but the arguments under test in order."""

    def __init__(self, ctx, sink):
        self.ctx, self.lib, self.h = ctx, ctx.lib, ctx._h
        self.surf = np.ascontiguousarray(sink.frames.surfaces)

    def rows(self, n, ln, rn, lyx, ryx, text=None):
        assert text is None                                                     # (this family has no text argument)
        return self.lib.lt_overlay_run_rows(self.h, 0, n, _ptr(ln), _ptr(rn), _ptr(lyx), _ptr(ryx), 0.3, None)

    def inplace(self, n, ln, rn, lyx, ryx, text=None):
        return self.lib.lt_overlay_run_inplace(self.h, 2, n, _ptr(ln), _ptr(rn), _ptr(lyx), _ptr(ryx), 0.3, text, None)

    def sink(self, n, ln, rn, lyx, ryx, text=None):
        return self.lib.lt_overlay_run_to_surfaces(self.h, 0, n, _ptr(ln), _ptr(rn), _ptr(lyx), _ptr(ryx), 0.3, text,
                                                   self.surf.ctypes.data if n else None, 0, None)

    def error(self):
        return self.lib.lt_last_error().decode()


def _text(lines, step):
    buf, nl = _native.text_bytes(lines, TEXT_KW["line_len"])
    t = _native.InplaceText(buf, nl, TEXT_KW["line_len"], TEXT_KW["origin"][0], TEXT_KW["origin"][1], step)
    return (buf, t), C.addressof(t)


def test_every_family_refuses_alike_and_then_works():
    w, h = SIZE
    a = _small_ctx(SIZE, "rgb", 4)
    b = _native.Context(SIZE, SIZE, np.eye(3), np.zeros(5), np.eye(3), capacity=4)
    polys = _polygons(w, h)
    frames = _noise(2, h, w, "rgb", seed=9)
    ps, ts = [polys[0], polys[2]], TEXTS[:2]
    s, cam = _Surfaces(np.zeros_like(frames), "rgb", 3, 1), _Surfaces(frames, "rgb", 5, 2)
    try:
        annotated = _annotated(a, frames, ps, ts)
        want_inplace, changed = _expected_frames(frames, annotated, "rgb")
        assert changed[:, 19:].any() and changed[:, 3:19].any()
        assert b.add_calibration(np.eye(3), np.zeros(5), np.eye(3)) == 1                       # set 1: no overlay, ever
        b.overlay_configure(np.eye(3))
        b.upload_frames(frames)
        b.attach_device_frames(cam.frames, first=2)
        f = _Families(b, s)
        ln, rn, lyx, ryx = _native.pack_polygons(ps)
        good = (2, ln, rn, lyx, ryx)

        def refused(family, args, code, phrase, text=None):
            rc = getattr(f, family)(*args, text=text)
            msg = f.error()
            assert rc == code and phrase in msg, (family, rc, msg)
            b.sync()
            assert b.last_overlay_launches() == -1, family                                     # nothing was launched ...
            assert s.unchanged() and cam.unchanged(), family                                   # ... and nothing stored

        # text before lt_overlay_set_font (the families that take text)
        keep, text = _text(ts, TEXT_KW["step"])
        refused("inplace", good, STATE, "lt_overlay_run_inplace with text before lt_overlay_set_font", text)
        refused("sink", good, STATE, "lt_overlay_run_to_surfaces with text before lt_overlay_set_font", text)
        b.overlay_set_font(*FONT)
        # text lines closer than a glyph is high
        keep6, text6 = _text(ts, 6)
        for family in ("inplace", "sink"):
            refused(family, good, INVALID, "text lines 6 rows apart would overlap (the glyphs are 7 rows high)", text6)
        # the point counts and lists
        neg = np.array([3, -1], np.int32)
        for family in ("rows", "inplace", "sink"):
            refused(family, (2, None, None, None, None), INVALID, "null point counts")
            refused(family, (2, ln, None, lyx, ryx), INVALID, "null point counts")
            refused(family, (2, neg, rn, lyx, ryx), INVALID, "negative point count")
            refused(family, (2, ln, neg, lyx, ryx), INVALID, "negative point count")
            refused(family, (2, ln, rn, None, ryx), INVALID, "null point list")
            refused(family, (2, ln, rn, lyx, None), INVALID, "null point list")
        # a slot whose calibration set has no overlay configured
        b.set_slot_calibrations([1], first=1)
        b.set_slot_calibrations([1], first=3)
        tail = " before lt_overlay_configure: slot %d has calibration set 1, whose overlay is not configured"
        refused("rows", good, STATE, "lt_overlay_run" + tail % 1)
        refused("inplace", good, STATE, "lt_overlay_run_inplace" + tail % 3)
        refused("sink", good, STATE, "lt_overlay_run_to_surfaces" + tail % 1)
        b.set_slot_calibrations([0], first=1)
        b.set_slot_calibrations([0], first=3)
        # a slot that holds part of its frame only (the families that read the slots' camera frames)
        b.upload_frame_rows(frames[:1], first=1)
        partial = ("slot 1 holds only part of its camera frame (lt_upload_frame_rows without lt_upload_frame_rest): a whole-frame "
                   "overlay would show rows of the block's previous occupant")
        refused("rows", good, STATE, partial)
        refused("sink", good, STATE, partial)
        b.upload_frames(frames)
        # no slots at all: nothing to check, nothing to do
        for family in ("rows", "inplace", "sink"):
            assert getattr(f, family)(0, None, None, None, None) == OK, (family, f.error())
        b.sync()
        assert b.last_overlay_launches() == -1 and s.unchanged() and cam.unchanged()
        del keep, keep6

        # the context still works, through every family
        b.overlay_run(ps)
        assert b.last_overlay_launches() == 1
        b.overlay_text(ts, **TEXT_KW)
        assert np.array_equal(b.download_overlay(2), annotated)
        b.overlay_run_to_surfaces(ps, s.frames, lines=ts, **TEXT_KW)
        b.store_wait()
        s.check(annotated, "the sink after the refusals")
        assert cam.unchanged()
        b.overlay_run_inplace(ps, first=2, lines=ts, **TEXT_KW)
        b.store_wait()
        cam.check(want_inplace, "in place after the refusals")
    finally:
        a.close()
        b.close()
        s.close()
        cam.close()
