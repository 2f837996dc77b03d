"""The front end against the CPU oracle over (pixel format x source x table form x range shape): the undistorted rows, the R plane
and the Lab-b plane of every slot of a range, bit for bit, and nothing written outside the range.  front_matrix.py builds the cases
and the reference; test_front_matrix_cpu.py holds the inputs to what they are for.

One context of 72 slots per (format, size) with the four calibration sets of the size.  The ranges, each fed from the slots' own
frames ("slots"), from pitched surfaces in device memory ("surfaces") and from both in runs of 1, 2, 3, 1, 2, 3, ... slots inside
the one slice ("alternating"):

  row  sets of the slots                                     first, n          what only it reaches
  1    all set 0                                             (0, 1), (1, 3)    the one-table kernels, one frame per walk, an odd first slot
  2    all set 2                                             (1, 37)           the one-table kernels with another set's tables; four frames
                                                                               per walk: nine walks and a tail walk of one
  3    the id pattern                                        (1, 5)            the table-per-slot kernels, one chunk
  4    the id pattern                                        (3, 67)           their second chunk, undistortion and warp (64 + 3)
  5    two streams: slice [0, 36) all set 1, [36, 72) the    (0, 72)           one call that takes the one-table form on one slice and
       id pattern                                                              the table-per-slot form on the other

A slot that reads a surface holds the complement of its frame in its own staging memory, so a walk that reads the wrong source shows;
every range takes other frames of the pool than its slots held, so a slot that nothing wrote shows.

The undistorted rows: set 0 is the identity, so the rows of the context are the whole image, every set's table covers them and whole
frames are fed: all rows of a slot are defined by the code, not only the run its own bird's-eye view reads.  Both are compared, the
set's own run first."""
import numpy as np
import pytest

import front_matrix as FM
from lane_tracker_amd import _native

pytestmark = pytest.mark.gpu

N = FM.CAPACITY
HALF = N // 2
SOURCES = ("slots", "surfaces", "alternating")
ROWS = [("1", 0, 1, lambda n: [0] * n, 1), ("1", 1, 3, lambda n: [0] * n, 1), ("2", 1, 37, lambda n: [2] * n, 1),
        ("3", FM.FIRSTS[0], 5, FM.ids_pattern, 1), ("4", FM.FIRSTS[1], 67, FM.ids_pattern, 1),
        ("5", 0, N, lambda n: [1] * HALF + FM.ids_pattern(n - HALF), 2)]


def _context(fmt, size):
    sets = FM.calibration_sets(size)
    c = _native.Context(FM.SIZES[size], FM.SIZES[size], sets[0]["cam_matrix"], sets[0]["dist_coeffs"], sets[0]["M"], capacity=N)
    try:
        if fmt != "rgb":
            c.set_input_format(fmt, FM.yuv_matrix(size))
        for s, q in enumerate(sets[1:], 1):
            assert c.add_calibration(q["cam_matrix"], q["dist_coeffs"], q["M"]) == s
        c.set_streams(1)
    except BaseException:
        c.close()
        raise
    return c


def _differing(got, want):
    d = got != want
    return int((d.any(-1) if d.ndim == 3 else d).sum())


def _feed(ctx, fmt, size, frames, first, source, offset):
    """The frames into slots first, ...; -> the DeviceFrames that must outlive the run (or None)."""
    if source == "slots":
        ctx.upload_frames(frames, first=first)
        return None
    n = len(frames)
    runs = [(0, n, True)] if source == "surfaces" else FM.alternating_runs(n)
    staged = frames.copy()
    for a, b, attached in runs:
        if attached:
            staged[a:b] = ~frames[a:b]                      # the slot's own frame is not the one to read
    ctx.upload_frames(staged, first=first)
    dev = FM.device_surfaces(frames, fmt, size, offset)
    try:
        assert int(dev.surfaces["plane"][0, 0]) == dev.owner.ptr + offset
        for a, b, attached in runs:
            if attached:
                ctx.attach_device_frames(dev[a:b], first=first + a)
    except BaseException:
        dev.owner.close()
        raise
    return dev


@pytest.mark.parametrize("fmt,size", FM.cases(), ids=["%s-%s" % c for c in FM.cases()])
def test_front_end_equals_the_oracle(fmt, size):
    w, h = FM.SIZES[size]
    pool = FM.frame_pool(fmt, size)
    ctx = _context(fmt, size)
    try:
        info = ctx.info()
        assert (info.src_row0, info.src_row1) == (0, h)      # the identity's rows: the whole image (all of it is compared below)
        held_r = held_b = None

        def run(row, first, n, ids, source, shift, offset):
            """Slot first + i takes frame (first + i + shift) % 72 of the pool and set ids[i]; everything is compared."""
            nonlocal held_r, held_b
            where = "%s %s (%dx%d), source %s, row %s of the table, slots [%d, %d)" % (fmt, size, w, h, source, row, first, first + n)
            ks = [(first + i + shift) % N for i in range(n)]
            ctx.set_slot_calibrations(ids, first=first)
            assert list(ctx.slot_calibrations(n, first=first)) == list(ids)
            dev = _feed(ctx, fmt, size, pool[ks], first, source, offset)
            try:
                ctx.mask_run(n, first=first)
                und = ctx.download_undistorted(n, first=first)
                got_r, got_b = ctx.download_plane(0, N), ctx.download_plane(1, N)
                ctx.sync()
            finally:
                if dev is not None:
                    dev.owner.close()
            assert und.shape == (n, h, w, 3)
            for i, (k, s) in enumerate(zip(ks, ids)):
                slot = first + i
                want_u, want_r, want_b = FM.reference(fmt, size, s, k)
                r0, r1 = FM.source_rows(size, s)
                msg = "%s: slot %d, set %d (frame %d of the pool): " % (where, slot, s, k)
                assert np.array_equal(und[i, r0:r1], want_u[r0:r1]), \
                    msg + "%d undistorted pixels differ in the set's own rows [%d, %d)" % (_differing(und[i, r0:r1], want_u[r0:r1]), r0, r1)
                assert np.array_equal(und[i], want_u), msg + "%d undistorted pixels differ outside the set's own rows" % _differing(und[i], want_u)
                assert np.array_equal(got_r[slot], want_r), msg + "%d pixels of the R plane differ" % _differing(got_r[slot], want_r)
                assert np.array_equal(got_b[slot], want_b), msg + "%d pixels of the Lab-b plane differ" % _differing(got_b[slot], want_b)
            if held_r is not None:
                for slot in list(range(first)) + list(range(first + n, N)):
                    for name, got, held in (("R", got_r, held_r), ("Lab-b", got_b, held_b)):
                        assert np.array_equal(got[slot], held[slot]), \
                            "%s: slot %d outside the range, set %d: %d pixels of its %s plane changed" % (
                                where, slot, int(ctx.slot_calibrations(1, first=slot)[0]), _differing(got[slot], held[slot]), name)
            held_r, held_b = got_r, got_b

        # all 72 slots once, set 0: what the slots outside a range must keep (and nine frames per walk, eight walks)
        run("0 (the fill)", 0, N, [0] * N, "slots", 0, 0)
        case = 0
        for source in SOURCES:
            for row, first, n, ids_of, streams in ROWS:
                case += 1
                if streams != 1:
                    ctx.set_streams(streams)
                try:
                    run(row, first, n, ids_of(n), source, 5 * case + 1, case % 4)
                finally:
                    if streams != 1:
                        ctx.set_streams(1)
    finally:
        ctx.close()
