"""Host frames into slots, every entry point x every kind of ingest, at 64 x 48: the camera frame of a slot and the undistorted rows
behind it after each family of uploads, against definitions that are not the library's (front_matrix.to_rgb, the raw-packed suite's
NumPy reference, oracle.resize_linear, oracle.undistort).

Kinds (lt_ingest.cpp): direct -- plain RGB of the calibration's size, rows straight into the camera frame; staged -- every other pixel
format, rows into the slot's staging frame and yuv_rows_to_rgb behind them (one case per copy arithmetic: NV12, I420, UYVY, BGRA, an
8-bit Bayer pattern, a MIPI-packed RAW10 pattern); resized -- RGB of another size, source rows into staging and the resize behind them.

Geometry: set 2 of front_matrix size A, whose bird's-eye view reads a strict inner run of camera rows: the rows the path's upload
brings, a raw mosaic's widened run and the pieces of a `rest` above and below it are all non-empty.

Contexts: capacity 2 on one stream (LaneTracker.process()'s: lazy reader notes, and the direct kind may take the aperture) and capacity 6
on two streams with the range n = 3, first = 1 (a call spans two slices).  Every step writes slots the previous step filled with other
frames, and the steps run forwards and then backwards without a sync() between them."""
import functools

import numpy as np
import pytest

import bayer_reference as RB
import front_matrix as FM
from lane_tracker_amd import _native, utils
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIZE, SET = "A", 2
W, H = FM.SIZES[SIZE]
SRC = (96, 72)                                   # the resized kind's input size (Wi, Hi)
POOL = 12
BAYER8, RAW10P = "bayer_grbg", "bayer10p_gbrg"
KINDS = ("rgb", "nv12", "i420", "uyvy", "bgra", BAYER8, RAW10P, "resized")
CONTEXTS = ((2, 1, 0, 2), (6, 2, 1, 3))          # (capacity, streams, first, n)
ROW_FORMS = ("waited-for", "enqueue", "async", "list")


@functools.lru_cache(maxsize=None)
def material(kind):
    """-> (POOL frames as the caller hands them in, their RGB camera frames, their undistorted images); shared, never changed."""
    if kind == "resized":
        frames = np.random.default_rng(77).integers(0, 256, (POOL, SRC[1], SRC[0], 3), dtype=np.uint8)
        rgb = np.stack([O.resize_linear(f, (W, H)) for f in frames])
    elif kind == RAW10P:
        words = np.random.default_rng(78).integers(0, 1 << 10, (POOL, H, W), dtype=np.uint16)
        frames = utils.pack_raw(words, kind)
        wide = kind.replace("p_", "_", 1)
        rgb = RB.bayer_to_rgb(utils.apply_raw_lut(words, wide, utils.raw_lut(bits=10)), "bayer_" + kind[-4:])
    else:
        frames = FM.frame_pool(kind, SIZE)[:POOL]
        rgb = FM.to_rgb(frames, kind, FM.yuv_matrix(SIZE))
    oc = FM.oracle_calib(SIZE, SET)
    und = np.stack([O.undistort(oc, f) for f in rgb])
    out = (np.ascontiguousarray(frames), np.ascontiguousarray(rgb), und)
    assert out[1].shape == out[2].shape == (POOL, H, W, 3) and out[1].dtype == np.uint8
    for a in out:
        a.setflags(write=False)
    return out


def _context(kind, capacity, streams):
    q = FM.calibration_sets(SIZE)[SET]
    c = _native.Context((W, H), (W, H), q["cam_matrix"], q["dist_coeffs"], q["M"], capacity=capacity)
    try:
        if kind == "resized":
            c.set_input_size(SRC)
        elif kind != "rgb":
            c.set_input_format(kind, FM.yuv_matrix(SIZE))
        c.set_streams(streams)
        c.overlay_configure(np.linalg.inv(q["M"]))
    except BaseException:
        c.close()
        raise
    return c


def _read_back(c, n, first, rows=None):
    """The camera frames of slots [first, first + n) through the overlay with no points (a plain copy of the frame); with `rows` only
    those two runs of rows (the others zero).  No sync(): the row form waits for its own download only."""
    e = np.zeros(0, np.int64)
    if rows is None:
        c.overlay_run([(e, e, e, e)] * n, first=first)
        return np.array(c.download_overlay(n, first=first))
    c.overlay_run([(e, e, e, e)] * n, first=first, rows=rows.ctypes.data)
    out = _native.pinned_empty((n, H, W, 3))
    out[:] = 0
    c.download_overlay_async(out, first=first, rows=rows.ctypes.data)
    c.download_overlay_wait()
    return np.array(out)


def _differing(got, want):
    return int((got != want).any(-1).sum())


@pytest.mark.parametrize("capacity,streams,first,n", CONTEXTS, ids=["cap2-1stream", "cap6-2streams"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_upload_form_brings_the_frame(kind, capacity, streams, first, n):
    frames, rgb, und = material(kind)
    ctx = _context(kind, capacity, streams)
    keep = []                                    # what the enqueued and stream-ordered forms were handed: alive until the last sync
    try:
        info = ctx.info()
        u0, u1 = info.src_row0, info.src_row1
        c0, c1 = ctx.source_rows()
        assert c0 >= 4 and c1 <= H - 4 and c1 > c0, "the path's camera rows [%d, %d) leave no room in %d rows" % (c0, c1, H)
        assert (u0, u1) == tuple(FM.source_rows(SIZE, SET))
        # the run of rows of the caller's frame that a `rest` cuts out: the camera rows, or what a staged kind stages for them
        r0, r1 = (c0, c1) if kind == "resized" else ctx.input_rows()
        assert 0 < r0 <= c0 and c1 <= r1 < H and (kind not in (BAYER8, RAW10P) or (r0, r1) != (c0, c1))
        where = "%s, capacity %d on %d stream(s), slots [%d, %d)" % (kind, capacity, streams, first, first + n)
        turn = [0]

        def pick():
            """The next n frames of the pool: never the ones the previous step left in these slots."""
            ks = [(turn[0] * n + i) % POOL for i in range(n)]
            turn[0] += 1
            return ks

        def check_frame(ks, form):
            got = _read_back(ctx, n, first)
            assert np.array_equal(got, rgb[ks]), "%s: %s: %d pixels of the camera frames differ" % (where, form, _differing(got, rgb[ks]))

        def check_undistorted(ks, form):
            ctx.mask_run(n, first=first)
            got = ctx.download_undistorted(n, first=first)
            want = und[ks][:, u0:u1]
            assert np.array_equal(got, want), "%s: %s: %d undistorted pixels differ" % (where, form, _differing(got, want))

        def rows_by(form, f):
            if form == "waited-for":
                ctx.upload_frame_rows(f, first=first)
            elif form == "enqueue":
                keep.append(ctx.upload_frame_rows(f, first=first, enqueue=True))
            elif form == "async":
                keep.append(ctx.upload_frame_rows_async(f, first=first))
            else:
                keep.append(ctx.upload_frame_rows_list(list(f), first=first))

        def whole():
            ks = pick()
            ctx.upload_frames(frames[ks], first=first)
            check_frame(ks, "upload_frames")
            check_undistorted(ks, "upload_frames")

        def rows_then_rest(form, rest_list=False):
            def step():
                ks = pick()
                f = np.ascontiguousarray(frames[ks])
                rows_by(form, f)
                check_undistorted(ks, "upload_frame_rows, " + form)
                if rest_list:
                    keep.append(ctx.upload_frame_rest_list(list(f), first=first))
                else:
                    keep.append(ctx.upload_frame_rest(f, first=first))
                check_frame(ks, "upload_frame_rest%s after upload_frame_rows, %s" % ("_list" if rest_list else "", form))
            return step

        def rows_then_runs(runs):
            def step():
                assert 0 <= runs[0] <= runs[1] <= runs[2] <= runs[3] <= H, runs
                ks = pick()
                f = np.ascontiguousarray(frames[ks])
                rows = np.array(runs, np.int32)
                rows_by("enqueue", f)
                ctx.mask_run(n, first=first)
                keep.append(ctx.upload_frame_rest(f, first=first, rows=rows.ctypes.data))
                got = _read_back(ctx, n, first, rows=rows)
                for lo, hi in ((runs[0], runs[1]), (runs[2], runs[3])):
                    assert np.array_equal(got[:, lo:hi], rgb[ks][:, lo:hi]), "%s: upload_frame_rest(rows=%s): %d pixels of rows [%d, %d) differ" % (
                        where, runs, _differing(got[:, lo:hi], rgb[ks][:, lo:hi]), lo, hi)
            return step

        steps = [whole] + [rows_then_rest(form) for form in ROW_FORMS] + [rows_then_rest("enqueue", rest_list=True)]
        steps += [rows_then_runs(r) for r in ((2, r0 + 3, r1 - 2, H - 1), (0, 1, r0 - 3, r1 + 1), (r0 + 1, r0 + 2, H - 1, H))]
        for step in steps + steps[::-1]:
            step()
        ctx.sync()
    finally:
        ctx.close()
        del keep
