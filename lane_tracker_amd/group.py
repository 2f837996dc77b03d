"""Many independent video streams, one frame each per call, on one device context: `LaneTrackerGroup`.

A deployment with K cameras holds one tracker per camera and feeds each one frame at a time.  K `LaneTracker`s pay K upload +
mask chain + search + record round trip + overlay + download per tick, each chain far too small to fill the chip.  A group
runs the K frames of a tick as ONE batch: the camera rows of the active frames go into consecutive slots of one context
(lt_upload_frame_rows_list, no gather on the host), one mask chain runs over them, one launch searches every frame in its own
stream's mode around its own stream's prior fits (lt_search_fit_list), the records come back in one download, and each stream's
state machine then runs on its record exactly as `LaneTracker.process()` runs it on its own.  Frames whose first try failed get
the second parameter set together, in a spare slot range.  One overlay launch and one download return the annotated frames.

Slots (K streams): [0, K) and [K, 2K) hold the first tries of alternate ticks, [2K, 3K) and [3K, 4K) their second tries -- the
lane-pixel lists a stream has not read yet stay on the device until its slot comes round again (then they are fetched first), as
`process()` alternates two slots for the same reason.
"""
import functools

import numpy as np

from . import _native
from .device import DeviceFrames, feed_rest_list, feed_rows_list
from .lane_tracker import LaneTracker
from .stream import StreamPipeline, _pack_deferred


class _GroupMember(LaneTracker):
    """One stream of a `LaneTrackerGroup`: every public attribute of `LaneTracker`, `get_state()` / `set_state()` and
    `get_success_ratio()`, on the group's device context.  It owns no context, so it cannot process frames itself."""

    _search_cus_set = True          # (the group's context never runs the chained stream pipeline: no CUs to reserve)

    def __init__(self, group, cal_id, *args, **kwargs):
        self._group, self._group_ctx = group, group._ctx
        self._cal_id = cal_id           # the calibration set of the group's context this stream's slots take
        super().__init__(*args, **kwargs)

    def _overlay_tables(self):
        """The table of this stream's calibration set, once per set of the group."""
        done = self._group._overlay_sets
        if self._cal_id not in done:
            if self._cal_id:
                self._ctx.overlay_configure(self.Minv, calibration=self._cal_id)
            else:
                self._ctx.overlay_configure(self.Minv)
            done.add(self._cal_id)

    def _make_context(self, device):
        return self._group_ctx

    def _not_owned(self, *args, **kwargs):
        raise RuntimeError("a LaneTrackerGroup member does not own a device context: feed its frames through the group's process()")

    # (wraps: process()'s signature stays LaneTracker.process's -- _batch_arguments reads the keywords and defaults from it)
    process = functools.wraps(LaneTracker.process)(_not_owned)
    process_batch = process_stream = warm = _not_owned
    set_raw_lut = _not_owned        # (the group sets its streams' tables: LaneTrackerGroup.set_raw_lut(lut, stream=i))
    set_raw_color = _not_owned      # (... and their colour stages: LaneTrackerGroup.set_raw_color)
    set_raw_shading = _not_owned    # (... and their lens-shading maps: LaneTrackerGroup.set_raw_shading)
    raw_stats = _not_owned          # (it uploads into slots, which are the group's: LaneTrackerGroup.raw_stats(frames, stream))
    _owns_context = False           # close() leaves the group's context to LaneTrackerGroup.close


_CALIBRATION_KEYS = ("cam_matrix", "dist_coeffs", "warp_matrices", "mpp_conversion")


def _stream_calibrations(calibrations, k, own):
    """`calibrations` of LaneTrackerGroup -> one complete mapping per stream (missing keys: the group's own).  ValueError /
    TypeError for a list of another length, an entry that is no mapping, unknown keys.  Touches no device."""
    if calibrations is None:
        return [dict(own) for _ in range(k)]
    cals = list(calibrations)
    if len(cals) != k:
        raise ValueError("calibrations: expected %d entries (None for the group's own calibration), got %d" % (k, len(cals)))
    out = []
    for i, c in enumerate(cals):
        full = dict(own)
        if c is not None:
            if not hasattr(c, "keys"):
                raise TypeError("calibrations[%d]: expected None or a mapping with any of %s" % (i, ", ".join(_CALIBRATION_KEYS)))
            unknown = sorted(set(c.keys()) - set(_CALIBRATION_KEYS))
            if unknown:
                raise ValueError("calibrations[%d]: unknown keys %s (known: %s)" % (i, ", ".join(map(repr, unknown)), ", ".join(_CALIBRATION_KEYS)))
            full.update(c)
        if len(full["warp_matrices"]) != 2 or len(full["mpp_conversion"]) != 2:
            raise ValueError("calibrations[%d]: warp_matrices is (M, Minv) and mpp_conversion is (vertical, horizontal)" % i)
        out.append(full)
    return out


_RAW_SETUP_KEYS = ("raw_lut", "raw_ccm", "raw_curve", "raw_shading")


def _checked_raw_setup(s, pixel_format):
    """One stream's raw_lut / raw_ccm / raw_curve / raw_shading through the checks a tracker's go through (ValueError)."""
    ccm, curve = _native.checked_raw_color(s["raw_ccm"], s["raw_curve"], pixel_format)
    return dict(raw_lut=_native.effective_raw_lut(s["raw_lut"], pixel_format), raw_ccm=ccm, raw_curve=curve,
                raw_shading=_native.checked_raw_shading(s["raw_shading"], pixel_format))


def _stream_raw_setups(raw_setups, k, own, pixel_format):
    """`raw_setups` of LaneTrackerGroup -> one complete, checked mapping per stream (missing keys: the group's own value; an explicit None:
    none for this camera).  ValueError / TypeError for a pixel format that is not raw Bayer, a list of another length, an entry that is
    no mapping, unknown keys, and whatever a tracker refuses of the values.  Touches no device."""
    own = _checked_raw_setup(own, pixel_format)
    if raw_setups is None:
        return [dict(own) for _ in range(k)]
    if not _native.raw_bits(pixel_format):
        raise ValueError("raw_setups condition raw Bayer frames: pixel_format=%r takes none" % (pixel_format,))
    setups = list(raw_setups)
    if len(setups) != k:
        raise ValueError("raw_setups: expected %d entries (None for the group's own setup), got %d" % (k, len(setups)))
    out = []
    for i, s in enumerate(setups):
        full = dict(own)
        if s is not None:
            if not hasattr(s, "keys"):
                raise TypeError("raw_setups[%d]: expected None or a mapping with any of %s" % (i, ", ".join(_RAW_SETUP_KEYS)))
            unknown = sorted(set(s.keys()) - set(_RAW_SETUP_KEYS))
            if unknown:
                raise ValueError("raw_setups[%d]: unknown keys %s (known: %s)" % (i, ", ".join(map(repr, unknown)), ", ".join(_RAW_SETUP_KEYS)))
            full.update(s)
            full = _checked_raw_setup(full, pixel_format)
        out.append(full)
    return out


def _raw_setup_key(s):
    """What a raw set of the context is made of, byte for byte: streams with equal keys share a set."""
    part = lambda a: b"-" if a is None else repr((a.shape, str(a.dtype))).encode() + np.ascontiguousarray(a).tobytes()
    sh = s["raw_shading"]
    return b"|".join([part(s["raw_lut"]), part(s["raw_ccm"]), part(s["raw_curve"]), b"-" if sh is None else part(sh.mesh) + part(sh.black)])


def _table_key(c):
    """What a calibration set of the context is made of, byte for byte: entries with equal keys share a set."""
    d = np.asarray(c["dist_coeffs"], np.float64).reshape(-1)
    parts = [np.asarray(c["cam_matrix"], np.float64).reshape(9), np.concatenate([d[:5], np.zeros(max(0, 5 - d.size))]),
             np.asarray(c["warp_matrices"][0], np.float64).reshape(9), np.asarray(c["warp_matrices"][1], np.float64).reshape(9)]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


class LaneTrackerGroup:
    """`k` independent lane trackers -- one per video stream, same image sizes and history lengths -- advanced one frame each
    per `process()` call in one batch on one device context.

    `calibrations` (keyword only): one entry per stream -- None for the group's own calibration, or a mapping with any of
    `cam_matrix`, `dist_coeffs`, `warp_matrices`, `mpp_conversion` (missing keys: the group's) -- for cameras that differ in
    intrinsics, distortion or mounting.  `img_size` / `warped_size` are the group's.  Entries whose arrays are equal byte for byte
    share one calibration set of the context (`calibration_count()`).

    `raw_setups` (keyword only, raw Bayer pixel formats): one entry per stream -- None for the group's own raw_lut / raw_ccm / raw_curve /
    raw_shading, or a mapping with any of those four keys (missing keys: the group's value; an explicit None: none for this camera) --
    for sensors that differ in white balance, colour matrix or lens.  Streams whose effective setups are equal byte for byte share one
    raw set of the context (`raw_set_count()`); `set_raw_lut` / `set_raw_color` / `set_raw_shading` with `stream=i` change one camera's,
    `raw_stats(frames, stream)` measures one camera's frames, and `trackers[i].raw_lut` ... read its own values.

    For every stream i, the annotated frame and the whole tracker state after every call equal, bit for bit, what a solo
    `LaneTracker.process()` leaves when fed the same frames; a stream whose frame is None does not move.  `trackers[i]` is
    stream i's tracker (read its attributes, `get_state()` / `set_state()` to hand a camera over).  Not thread-safe, like
    `LaneTracker`; groups on different threads share nothing."""

    def __init__(self, k, img_size, warped_size, cam_matrix, dist_coeffs, warp_matrices, mpp_conversion, n_fail=8, n_reset=4,
                 n_average=2, print_frame_count=False, device=0, *, pixel_format='rgb', yuv_matrix='bt601', calibrations=None,
                 input_size=None, raw_lut=None, raw_ccm=None, raw_curve=None, raw_shading=None, raw_setups=None):
        k = int(k)
        if k < 1:
            raise ValueError("a group needs at least one stream")
        self._ctx = None
        self.trackers = []
        cals = _stream_calibrations(calibrations, k, dict(cam_matrix=cam_matrix, dist_coeffs=dist_coeffs, warp_matrices=warp_matrices,
                                                          mpp_conversion=mpp_conversion))
        self.k = k
        self.img_size, self.warped_size = img_size, warped_size
        self.pixel_format, self.yuv_matrix = pixel_format, yuv_matrix
        self._frame_shape = _native.input_frame_shape(img_size, pixel_format)
        # one input size for all streams (LaneTracker's input_size): RGB frames of that size, resized on the device to img_size
        self.input_size = None if input_size is None else tuple(int(v) for v in input_size)
        self._resize_from = _native.checked_input_size(input_size, img_size, pixel_format)
        if self._resize_from is not None:
            self._frame_shape = (self._resize_from[1], self._resize_from[0], 3)
        self._raw_lut = _native.effective_raw_lut(raw_lut, pixel_format)       # the group's own raw table (LaneTracker's raw_lut): what raw_setups leaves out
        self._raw_ccm, self._raw_curve = _native.checked_raw_color(raw_ccm, raw_curve, pixel_format)     # ... and one colour stage
        self._raw_shading = _native.checked_raw_shading(raw_shading, pixel_format)      # ... and one lens-shading map
        # every stream's own setup (raw_setups), checked before any device call: set 0 of the context is the group's, one more for every
        # distinct setup among the streams
        setups = _stream_raw_setups(raw_setups, k, dict(raw_lut=self._raw_lut, raw_ccm=self._raw_ccm, raw_curve=self._raw_curve,
                                                       raw_shading=self._raw_shading), pixel_format)
        self._raw_ids, self._raw_sets_used = [0] * k, False
        self._ctx = _native.Context(img_size, warped_size, cam_matrix, dist_coeffs, warp_matrices[0], device=device, capacity=4 * k)
        self._tick = 0
        self._overlay_sets = set()           # the calibration sets whose overlay a member has configured
        try:
            if pixel_format != 'rgb':        # every stream of a group is a camera of the same kind
                self._ctx.set_input_format(pixel_format, yuv_matrix)
            if self._resize_from is not None:
                self._ctx.set_input_size(self._resize_from)
            if self._raw_lut is not None:
                self._ctx.set_raw_lut(self._raw_lut)
            if self._raw_ccm is not None or self._raw_curve is not None:
                self._ctx.set_raw_color(self._raw_ccm, self._raw_curve)
            if self._raw_shading is not None:
                self._ctx.set_raw_shading(self._raw_shading)
            raw_sets = {_raw_setup_key(dict(raw_lut=self._raw_lut, raw_ccm=self._raw_ccm, raw_curve=self._raw_curve, raw_shading=self._raw_shading)): 0}
            for i, s in enumerate(setups):
                key = _raw_setup_key(s)
                if key not in raw_sets:
                    raw_sets[key] = self._new_raw_set(s)
                self._raw_ids[i] = raw_sets[key]
            # the calibration sets of the context: 0 is the group's own, one more for every distinct calibration among the streams
            sets = {_table_key(dict(cam_matrix=cam_matrix, dist_coeffs=dist_coeffs, warp_matrices=warp_matrices)): 0}
            self._cal_ids = []
            for c in cals:
                key = _table_key(c)
                if key not in sets:
                    sets[key] = self._ctx.add_calibration(c["cam_matrix"], c["dist_coeffs"], c["warp_matrices"][0])
                self._cal_ids.append(sets[key])
            self._many_sets = len(sets) > 1
            for c, cal_id, rs in zip(cals, self._cal_ids, setups):
                self.trackers.append(_GroupMember(self, cal_id, img_size, warped_size, c["cam_matrix"], c["dist_coeffs"], c["warp_matrices"],
                                                  c["mpp_conversion"], n_fail=n_fail, n_reset=n_reset, n_average=n_average,
                                                  print_frame_count=print_frame_count, device=device,
                                                  pixel_format=pixel_format, yuv_matrix=yuv_matrix, input_size=input_size,
                                                  raw_lut=rs["raw_lut"], raw_ccm=rs["raw_ccm"], raw_curve=rs["raw_curve"],
                                                  raw_shading=rs["raw_shading"]))
        except BaseException:
            self.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- raw sets: one raw table, colour stage and shading map per camera -------------------------------------------------------------
    def _new_raw_set(self, setup):
        """A further raw set of the context holding `setup` (a copy of set 0, then every part written); returns its id."""
        ctx = self._ctx
        rid = ctx.add_raw_set()
        ctx.set_raw_lut(setup["raw_lut"], raw_set=rid)
        ctx.set_raw_color(setup["raw_ccm"], setup["raw_curve"], enable=setup["raw_ccm"] is not None or setup["raw_curve"] is not None, raw_set=rid)
        ctx.set_raw_shading(setup["raw_shading"], raw_set=rid)
        self._raw_sets_used = True
        return rid

    def _raw_targets(self, stream):
        """(raw set ids, trackers) a setter with `stream` changes: every set in use and every tracker (None), or stream i's own set --
        split off first where other streams share it -- and tracker i."""
        if stream is None:
            return sorted(set(self._raw_ids)), self.trackers
        i = int(stream)
        if not 0 <= i < self.k:
            raise ValueError("stream must be 0 .. %d, got %r" % (self.k - 1, stream))
        t = self.trackers[i]
        if self._raw_ids.count(self._raw_ids[i]) > 1:
            self._raw_ids[i] = self._new_raw_set(dict(raw_lut=t._raw_lut, raw_ccm=t._raw_ccm, raw_curve=t._raw_curve, raw_shading=t._raw_shading))
        return [self._raw_ids[i]], [t]

    @staticmethod
    def _of_set(rid):
        return dict(raw_set=rid) if rid else {}      # (set 0 through the calls a group always made)

    def raw_set_count(self):
        """The raw sets the group's streams use (1: every stream is conditioned with the same table, colour stage and shading map)."""
        return len(set(self._raw_ids))

    @property
    def raw_lut(self):
        """The group's raw table, u8 (4, 256), or None (`set_raw_lut`); a stream's own: `trackers[i].raw_lut`."""
        return None if self._raw_lut is None else self._raw_lut.copy()

    def set_raw_lut(self, lut, stream=None):
        """Another raw table for every stream of the group -- `stream=i`: for camera i alone, which gets a raw set of its own where it
        shared one -- or None for none, between `process()` calls (LaneTracker.set_raw_lut)."""
        lut = _native.effective_raw_lut(lut, self.pixel_format)
        if not _native.raw_bits(self.pixel_format):
            return
        ids, ts = self._raw_targets(stream)
        for rid in ids:
            self._ctx.set_raw_lut(lut, **self._of_set(rid))
        if stream is None:
            self._raw_lut = lut
        for t in ts:
            t._raw_lut = lut
            t._resident = None

    @property
    def raw_ccm(self):
        """The colour-correction matrix of the group's colour stage, int16 (3, 3) in Q10, or None (`set_raw_color`)."""
        return None if self._raw_ccm is None else self._raw_ccm.copy()

    @property
    def raw_curve(self):
        """The output curve of the group's colour stage, u8 (256,), or None (`set_raw_color`)."""
        return None if self._raw_curve is None else self._raw_curve.copy()

    def set_raw_color(self, ccm=None, curve=None, stream=None):
        """Another colour stage for every stream of the group -- `stream=i`: for camera i alone -- or (None, None) for none, between
        `process()` calls (LaneTracker.set_raw_color)."""
        ccm, curve = _native.checked_raw_color(ccm, curve, self.pixel_format)
        if not _native.raw_bits(self.pixel_format):
            return
        ids, ts = self._raw_targets(stream)
        for rid in ids:
            self._ctx.set_raw_color(ccm, curve, enable=ccm is not None or curve is not None, **self._of_set(rid))
        if stream is None:
            self._raw_ccm, self._raw_curve = ccm, curve
        for t in ts:
            t._raw_ccm, t._raw_curve = ccm, curve
            t._resident = None

    @property
    def raw_shading(self):
        """The group's lens-shading map, a utils.RawShading (a copy), or None (`set_raw_shading`)."""
        s = self._raw_shading
        return None if s is None else type(s)(s.mesh.copy(), s.black.copy())

    def set_raw_shading(self, shading, stream=None):
        """Another lens-shading map for every stream of the group -- `stream=i`: for camera i alone -- or None for none, between
        `process()` calls (LaneTracker.set_raw_shading)."""
        shading = _native.checked_raw_shading(shading, self.pixel_format)
        if not _native.raw_bits(self.pixel_format):
            return
        ids, ts = self._raw_targets(stream)
        for rid in ids:
            self._ctx.set_raw_shading(shading, **self._of_set(rid))
        if stream is None:
            self._raw_shading = shading
        for t in ts:
            t._raw_shading = shading
            t._resident = None

    def raw_stats(self, frames, stream, grid=(8, 8), rows=None, cols=None, lo=None, hi=None):
        """`LaneTracker.raw_stats` of camera `stream`'s frames -- one frame, a stack, or `DeviceFrames` --, behind that camera's shading
        map: what its auto-white-balance step measures (`set_raw_lut(utils.raw_lut(..., utils.awb_gains(s, black), ...), stream=i)`).
        Between `process()` calls; it runs in slots the group is not using and leaves every stream's state and counters untouched."""
        if self._ctx is None:
            raise RuntimeError("the group is closed")
        if not _native.raw_bits(self.pixel_format):
            raise ValueError("raw statistics are taken of raw Bayer frames: a %r group has none" % (self.pixel_format,))
        i = int(stream)
        if not 0 <= i < self.k:
            raise ValueError("stream must be 0 .. %d, got %r" % (self.k - 1, stream))
        base = (self._tick & 1) * self.k         # the slots the next tick's first tries take: their lists are fetched first, as process() does
        self._free_slots(base, base + self.k)
        if self._raw_sets_used:
            self._ctx.set_slot_raw_sets([self._raw_ids[i]] * self.k, first=base)
        return self.trackers[i]._raw_stats_in_slots(frames, base, self.k, grid, rows, cols, lo, hi)

    def calibration_count(self):
        """The calibration sets the group's context holds (1: every stream has the group's own calibration)."""
        return self._ctx.calibration_count() if self._many_sets else 1

    def close(self):
        for t in self.trackers:
            t.close()
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    # ------------------------------------------------------------------------------------------------------------------------
    def _free_slots(self, lo, hi):
        """Fetch every stream's lists that still lie in slots [lo, hi) before those slots take new frames."""
        for t in self.trackers:
            p, q = t._pending, t._pending_cent
            if (p is not None and lo <= p[1] < hi) or (q is not None and lo <= q[1] < hi):
                t._materialise_pending()

    def _search(self, ts, base, try_, diagnostics):
        """Search the masks in slots base, base + 1, ... -- one per tracker of `ts`, each in its own mode -- in one launch and
        collect the records into the trackers (what _search_uploaded leaves)."""
        items = np.zeros(len(ts), _native.SEARCH_ITEM_DTYPE)
        modes = []
        for j, t in enumerate(ts):
            items[j]["slot"] = base + j
            if t.last_detection > t.n_reset:                                  # lane_tracker.py:851
                modes.append('sws')
            else:
                modes.append('bs')
                items[j]["mode"] = 1
                items[j]["prev_coeffs"][:3] = np.asarray(t.last_left_coeffs, np.float64).reshape(3)
                items[j]["prev_coeffs"][3:] = np.asarray(t.last_right_coeffs, np.float64).reshape(3)
            if diagnostics:
                print("Using sliding window search." if modes[-1] == 'sws' else "Using band search.")
        q = try_
        sws = _native.search_params(window_width=q[9], window_height=q[10], search_range=q[11], mu=q[12], no_success_limit=q[13],
                                    start_slice=q[14], ignore_sides=q[15], ignore_bottom=q[16], partial=q[18])
        band = _native.search_params(bandwidth=q[17], ignore_bottom=q[16], partial=q[18])
        ctx = self._ctx
        ctx.search_fit_list(items, sws, band)
        recs = ctx.download_records(len(ts), first=base)
        for j, t in enumerate(ts):
            r = recs[j]
            t._collect_record(ctx, (r["left_coeffs"].copy(), r["right_coeffs"].copy(), bool(r["detected"]), int(r["fit_flags"])),
                              want_centroids=(modes[j] == 'sws'), slot=base + j, lazy=True)
            if diagnostics:
                print("Lane pixels found." if t.detected_pixels else "No lane pixels found.")

    def process(self, frames, annotate=True, out=None, out_yuv_matrix=None, **kwargs):
        """One frame per stream: `frames[i]` (a host array or a one-frame `DeviceFrames` of img_size in the group's pixel format) for
        stream i, or None -- stream i skips this call.  `kwargs` are
        `LaneTracker.process()`'s keywords (one set for the whole group; visualize_search / split_view are not available).
        Returns a list of k entries: stream i's annotated frame (views of one block), or None for a skipped stream and for
        every stream with `annotate=False` (the states are updated identically).
        `out`: a device sink -- a `DeviceFrames` of the group's `img_size` with k surfaces on the group's device, 'rgb', 'nv12' or
        'i420' at any pitch; surface i is stream i's.  The annotated frames of the active streams are drawn on their way into their
        surfaces by one kernel launch, whatever the streams' calibrations (lt_overlay_run_to_surfaces; 4:2:0 converted with
        `out_yuv_matrix`, None: 'bt601'), and no frame crosses the bus on the way out; the surfaces of skipped streams are not touched.
        Returns `out[i]` for active streams and None for skipped ones, final when the call returns.
        `out="inplace"`: every active frame is a writeable one-frame `DeviceFrames`, and lane and text are drawn INTO them by one
        launch (lt_overlay_run_inplace; `out_yuv_matrix=None`: the group's own `yuv_matrix`, which must then be a preset's name).
        Returns the frames handed in.  Both need `annotate=True`; states and attributes are those of the same call without `out`."""
        if self._ctx is None:
            raise RuntimeError("the group is closed")
        frames = list(frames)
        if len(frames) != self.k:
            raise ValueError("expected %d frames (None for a stream that skips this call), got %d" % (self.k, len(frames)))
        t0 = self.trackers[0]
        kw, first_try, fp = t0._batch_arguments(kwargs)
        if kw["visualize_search"] or kw["split_view"]:
            raise NotImplementedError("search visualisation / split view are not available for a group: use the streams' own trackers "
                                      "(process, process_batch, process_stream)")
        n_tries, diagnostics = kw["n_tries"], kw["diagnostics"]
        active = [i for i, f in enumerate(frames) if f is not None]
        # the destination of the annotated frames, checked before anything reaches the device
        t0._sink_keywords(out, annotate, kw)
        in_place = isinstance(out, str)
        sink = None
        if in_place:
            out_yuv_matrix = t0._inplace_matrix(out, out_yuv_matrix)
            for i in active:
                t0._check_inplace_source(frames[i])
        elif out is not None:
            sink = t0._check_sink(out, self.k, one_launch=True)
            out_yuv_matrix = 'bt601' if out_yuv_matrix is None else out_yuv_matrix
            _native.rgb2yuv_coeffs(out_yuv_matrix)
        outs = [None] * self.k
        if not active:
            return outs
        shape = self._frame_shape
        imgs = [frames[i] if isinstance(frames[i], DeviceFrames) else _native.frames_array(frames[i], self.pixel_format) for i in active]
        for img in imgs:
            if isinstance(img, DeviceFrames) and self._resize_from is not None:
                raise ValueError("a group with input_size takes host frames only: frames in device memory are not resized")
            if isinstance(img, DeviceFrames):        # a stream whose frame is already in device memory: attached, not uploaded
                img.check_for(self.img_size, self.pixel_format)
                if len(img) != 1:
                    raise ValueError("expected one frame per stream, got DeviceFrames of %d" % len(img))
            elif img.shape != shape:
                raise ValueError("expected frames of shape %r, got %r" % (shape, img.shape))
        ts = [self.trackers[i] for i in active]
        m, k, ctx = len(active), self.k, self._ctx
        r = self._tick & 1
        self._tick += 1
        base, spare = r * k, (2 + r) * k
        self._free_slots(base, base + m)

        # 1-3: camera rows of the m frames, one mask chain, one search launch
        if self._raw_sets_used:                                          # every slot with its stream's raw set, ahead of its frame
            ctx.set_slot_raw_sets([self._raw_ids[i] for i in active], first=base)
        keep = feed_rows_list(ctx, imgs, base)
        if self._many_sets:                                              # ... and with its stream's calibration set
            ctx.set_slot_calibrations([self._cal_ids[i] for i in active], first=base)
        ctx.mask_run(m, fp, first=base)
        keep_rest = None
        if annotate:
            if not in_place:                                             # (an in-place draw reads the surfaces themselves)
                keep_rest = feed_rest_list(ctx, imgs, base)              # (for the overlay, beside the mask chain)
            ts[0]._configure_overlay()                                   # (every member configured its set's overlay when it was built)
        for t in ts:                                                     # _step's opening
            t._open_frame()
            t._want_out = False
            t._device_lane = None
        self._search(ts, base, first_try, diagnostics)

        # 4: each stream's verdict on its first try (_step's pieces, run per stream on the records of the one launch)
        fits, partials, again = [None] * m, [first_try[-1]] * m, []
        for j, t in enumerate(ts):
            if t.detected_pixels:
                fits[j] = t._fit_and_check(diagnostics, "first")
            if t._needs_second_try(n_tries, diagnostics):
                again.append(j)

        # 5: the second parameter set over the frames that need it, in the spare slots (the first tries' slots stay untouched)
        if again:
            second = StreamPipeline._SECOND_TRY
            self._free_slots(spare, spare + len(again))
            if self._raw_sets_used:
                ctx.set_slot_raw_sets([self._raw_ids[active[j]] for j in again], first=spare)
            keep_again = feed_rows_list(ctx, [imgs[j] for j in again], spare)
            if self._many_sets:
                ctx.set_slot_calibrations([self._cal_ids[active[j]] for j in again], first=spare)
            ctx.mask_run(len(again), _native.filter_params(second[4], *second[:4], *second[5:9]), first=spare)
            self._search([ts[j] for j in again], spare, second, diagnostics)
            for j in again:
                t = ts[j]
                partials[j] = 1.0
                fits[j] = None
                if t.detected_pixels:
                    fits[j] = t._fit_and_check(diagnostics, "second")
            del keep_again

        # the outcomes (_step's ending, deferred pictures) ...
        deferred = []
        for j, t in enumerate(ts):
            if not t.valid_lane_lines:
                if diagnostics:
                    print("No success after all attempts.")
                t._record_failure()
            else:
                t._record_success(fits[j][0], fits[j][1], partials[j])
            if annotate:
                deferred.append(t._deferred_picture())
        # 6: ... drawn by one overlay launch and one download -- or, with `out`, by one launch into the sink's surfaces / into the
        # frames themselves (a second try attached its surface to a spare slot as well: the draw detaches every slot of a surface)
        if in_place:
            ts[0]._draw_in_place(deferred, base, out_yuv_matrix)
            ctx.store_wait()
            for i in active:
                outs[i] = frames[i]
        elif sink is not None:
            lines = [d[2] for d in deferred] if ts[0]._have_font else None
            ctx.overlay_run_to_surfaces_packed(*_pack_deferred(deferred), sink.select(active), first=base, lines=lines,
                                               origin=ts[0]._TEXT_ORIGIN, step=ts[0]._TEXT_STEP, matrix=out_yuv_matrix)
            ctx.store_wait()
            for i in active:
                outs[i] = sink[i]
        elif annotate:
            for i, picture in zip(active, ts[0]._render_window(deferred, base)):
                outs[i] = picture
        del keep_rest
        del keep
        return outs
