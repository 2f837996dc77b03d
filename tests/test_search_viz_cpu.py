"""The host logic of `visualize_search=True` / `split_view=True` in the stream pipeline, without a GPU: `LaneTracker` on a subclass of
`tests/fake_context.py` that paints `search_viz_run` / `split_panes_run` with `overlay.py` and `utils.resize_linear` from the fake
slot's mask and lists AT THE MOMENT OF THE CALL -- so a descriptor enqueued too late (after a second-try mask, a first-try search
run again, a speculative re-search over the slot) shows as a wrong picture.  What is checked is the driver: the per-frame descriptors
of `_step`, of the bulk commit of chained successes and of `_fail_group`, against the unchained route, which paints on the host as
`process()` does (reference lane_tracker.py:687-793, 1130-1137)."""
import numpy as np
import pytest

import fake_context
from lane_tracker_amd import _native, calib, overlay, synth, utils
from lane_tracker_amd.lane_tracker import LaneTracker
from oracle import oracle as O


class VizFakeContext(fake_context.FakeContext):
    kinds = None                     # optional list: the kind of every item painted, in call order

    def download_bev(self, n, first=0):
        return np.stack([O.warp(self.oc, O.undistort(self.oc, self._slot(first + k)["frame"])) for k in range(n)], 0)

    def split_panes_size(self):
        return _native.split_panes_size((self.img_w, self.img_h), (self.warp_w, self.warp_h))

    def search_viz_wait(self):
        pass

    def _paint(self, items, lists):
        at = [0, 0, 0, 0]
        out = []
        for it in items:
            s = self._slot(int(it["slot"]))
            mask = s["mask"]
            kind = int(it["kind"])
            if VizFakeContext.kinds is not None:
                VizFakeContext.kinds.append(kind)
            if kind == 0:
                out.append(np.repeat(mask[:, :, None], 3, axis=2))
                continue
            cut = []
            for c, field in enumerate(("n_fit_left", "n_fit_right", "n_band_left", "n_band_right")):
                m = int(it[field]) if (c < 2 or kind == 2) else 0
                cut.append(np.asarray(lists[c][at[c]:at[c] + m], np.int64).reshape(-1, 2) if m else np.zeros((0, 2), np.int64))
                at[c] += m
            fit = (cut[0][:, 0], cut[0][:, 1], cut[1][:, 0], cut[1][:, 1])
            ly, lx, ry, rx = s["pix"]
            if kind == 1:
                out.append(overlay.visualize_sliding_window_search(mask, s["cent"][0], s["cent"][1], (ly, lx), (ry, rx), fit,
                                                                   int(it["window_width"]), int(it["window_height"]), int(it["ignore_bottom"])))
            else:
                band = (cut[2][:, 0], cut[2][:, 1], cut[3][:, 0], cut[3][:, 1])
                out.append(overlay.visualize_band_search(mask, (ly, lx), (ry, rx), band, fit, int(it["bandwidth"])))
        return out

    def search_viz_run(self, items, fit_left=None, fit_right=None, band_left=None, band_right=None, out=None):
        pics = self._paint(items, (fit_left, fit_right, band_left, band_right))
        out[:] = np.stack(pics, 0)
        return out

    def split_panes_run(self, items, fit_left=None, fit_right=None, band_left=None, band_right=None, out=None):
        sw, sh, x2 = self.split_panes_size()
        pics = self._paint(items, (fit_left, fit_right, band_left, band_right))
        for q, (it, pic) in enumerate(zip(items, pics)):
            bev = self.download_bev(1, first=int(it["slot"]))[0]
            out[q] = utils.create_split_view((self.img_w, sh), [bev, pic], [(0, 0), (x2, 0)], [(sw, sh), (sw, sh)])
        return out


@pytest.fixture()
def fake(monkeypatch):
    monkeypatch.setattr(_native, "Context", VizFakeContext)
    monkeypatch.setattr(_native, "pinned_empty", lambda shape, dtype=np.uint8: np.empty(shape, dtype))
    VizFakeContext.kinds = []
    yield VizFakeContext
    VizFakeContext.kinds = None


@pytest.fixture(scope="module")
def stream():
    a = synth.stream_lanes(3, seed=101)
    b = synth.stream_lanes(3, seed=202)
    noise, black = synth.frame_uniform(4001), np.zeros_like(a[0])
    mirrored, shifted = np.ascontiguousarray(a[1][:, ::-1]), np.roll(a[2], 200, axis=1)
    return np.stack([noise, a[0], a[1], mirrored, a[2], black, noise, a[1], shifted, a[0], black, black, black, black, black, noise,
                     b[0], b[1]], 0)


# per frame of the stream: 0 bare mask, 1 sliding windows, 2 band (default keywords)
KINDS = [1, 1, 2, 2, 2, 0, 2, 2, 0, 2, 0, 0, 0, 0, 0, 1, 1, 2]


@pytest.fixture(scope="module")
def unchained(stream):
    """The yardstick, computed once: the frame-by-frame route with host painting -> (pictures, states after each frame)."""
    import unittest.mock as mock
    with mock.patch.object(_native, "Context", VizFakeContext):
        seq = LaneTracker(**calib.reference_calibration())
        seq.chain_searches = False
        pics, states = [], []
        for f in stream:
            (none, pic), = seq.process_batch(f[None], annotate=False, visualize_search=True)
            assert none is None
            pics.append(pic.copy())
            states.append(_state(seq))
    return pics, states


def _state(lt):
    b = lambda a: None if a is None else np.asarray(a).tobytes()
    return dict(detected=lt.detected_pixels, valid=lt.valid_lane_lines, last_detection=lt.last_detection, success=lt.success,
                counter=lt.counter, last_left=b(lt.last_left_coeffs), last_right=b(lt.last_right_coeffs),
                pix=(b(lt.left_y), b(lt.left_x), b(lt.right_y), b(lt.right_x)), cent=(lt.left_window_centroids, lt.right_window_centroids))


def _same(got, want, where):
    assert got.ndim == want.ndim and got.shape == want.shape, (where, got.shape, want.shape)
    assert np.array_equal(got, want), where


def test_the_stream_holds_every_kind(unchained):
    pics, states = unchained
    assert [p.ndim for p in pics] == [2 if k == 0 else 3 for k in KINDS]
    valid = [s["valid"] for s in states]
    assert not valid[0] and valid[1] and not valid[15] and valid[16] and valid[17]      # failed second tries at 0 and 15


@pytest.mark.parametrize("chunk,windows", [(None, (18,)), (4, (5, 13)), (2, (7, 4, 7))])
def test_process_batch_pictures_equal_the_unchained_route(fake, stream, unchained, chunk, windows):
    pics, states = unchained
    bat = LaneTracker(**calib.reference_calibration())
    bat.chain_chunk = chunk
    lo = 0
    for w in windows:
        out = bat.process_batch(stream[lo:lo + w], annotate=False, visualize_search=True)
        assert len(out) == w
        for q, (none, pic) in enumerate(out):
            assert none is None
            _same(pic, pics[lo + q], (windows, lo + q))
        assert _state(bat) == states[lo + w - 1], (windows, lo)
        lo += w
    assert fake.kinds == KINDS


def test_process_stream_pictures_equal_the_unchained_route(fake, stream, unchained):
    pics, states = unchained
    bat = LaneTracker(**calib.reference_calibration())
    bat.chain_chunk = 4
    wins = [stream[0:6], stream[6:12], stream[12:18]]
    for k, out in enumerate(bat.process_stream(wins, annotate=False, visualize_search=True)):
        for q, (none, pic) in enumerate(out):
            assert none is None
            _same(pic, pics[6 * k + q], (k, q))
        assert _state(bat) == states[6 * k + 5], k
    assert fake.kinds == KINDS


class BlindSecondTry(VizFakeContext):
    """The second parameter set ('neighborhood') sees nothing: a frame whose first try found pixels but no valid lane ends with the
    bare, empty second-try mask -- and `_fail_group` then runs that frame's first-try mask and search again, for the tracker's lists."""

    def mask_run(self, n, fp=None, first=0, reuse_front=False):
        super().mask_run(n, fp, first, reuse_front)
        if fp is not None and fp.filter_type == 1:
            for k in range(n):
                self._slot(first + k)["mask"] = np.zeros((self.warp_h, self.warp_w), np.uint8)


def test_an_outage_group_paints_before_it_runs_a_first_try_again(monkeypatch, stream):
    monkeypatch.setattr(_native, "Context", BlindSecondTry)
    monkeypatch.setattr(_native, "pinned_empty", lambda shape, dtype=np.uint8: np.empty(shape, dtype))
    off = np.roll(stream[4], 60, axis=1)          # the lane 60 columns aside: the band still finds pixels, the fit is not valid
    frames = np.stack([stream[1], stream[2], off, off, off, off, off, stream[4], off, stream[2]], 0)    # a whole group fails, and a lone frame
    seq, bat = (LaneTracker(n_reset=8, **calib.reference_calibration()) for _ in range(2))
    seq.chain_searches = False
    want = [seq.process_batch(f[None], annotate=False, visualize_search=True)[0][1] for f in frames]
    got = [p for _, p in bat.process_batch(frames, annotate=False, visualize_search=True)]
    assert want[2].ndim == 2 and not want[2].any() and seq.left_x.size        # the empty second-try mask; the first try's lists kept
    for q in range(len(frames)):
        _same(got[q], want[q], q)
    assert _state(bat) == _state(seq)


def test_split_view_needs_a_new_annotated_frame(fake, stream):
    lt = LaneTracker(**calib.reference_calibration())
    with pytest.raises(ValueError):
        lt.process_batch(stream[:2], annotate=False, split_view=True)
    with pytest.raises(ValueError):
        lt.process_batch(stream[:2], annotate="inplace", split_view=True)
    with pytest.raises(ValueError):
        next(lt.process_stream([stream[:2]], annotate=False, split_view=True))
    out = lt.process_batch(stream[:2], annotate=False, visualize_search=True, split_view=True)    # the pictures win, as upstream
    assert all(isinstance(o, tuple) and o[0] is None for o in out)


def test_fake_panes_are_the_lower_part_of_triple_split_view(fake, stream):
    """The stand-in's pane strip (what the GPU suite holds lt_split_panes_run to) is rows img_h .. of triple_split_view."""
    lt = LaneTracker(**calib.reference_calibration())
    ctx = lt._ctx
    ctx.upload_frame_rows(stream[1:2])
    ctx.mask_run(1)
    ctx.sws_fit_run(1)
    items = np.zeros(1, _native.VIZ_ITEM_DTYPE)
    items[0]["kind"], items[0]["window_width"], items[0]["window_height"], items[0]["ignore_bottom"] = 1, 30, 40, 30
    sw, sh, x2 = ctx.split_panes_size()
    strip = ctx.split_panes_run(items, out=np.empty((1, sh, ctx.img_w, 3), np.uint8))[0]
    pic = ctx.search_viz_run(items, out=np.empty((1, ctx.warp_h, ctx.warp_w, 3), np.uint8))[0]
    view = lt.triple_split_view([stream[1], ctx.download_bev(1)[0], pic])
    assert view.shape == (ctx.img_h + sh, ctx.img_w, 3) and np.array_equal(view[ctx.img_h:], strip)


@pytest.mark.parametrize("img,warp", [((1280, 720), (1080, 1100)), ((1281, 720), (1080, 1100)), ((1279, 719), (1081, 1099)), ((128, 72), (90, 71)),
                                      ((640, 480), (333, 777))])
def test_split_panes_size_is_triple_split_views_arithmetic(img, warp):
    sw, sh, x2 = _native.split_panes_size(img, warp)
    scale = warp[0] / (0.5 * img[0])
    assert (sw, sh, x2) == (round(warp[0] / scale), round(warp[1] / scale), round(0.5 * img[0]))
    if (img, warp) == ((1280, 720), (1080, 1100)):
        assert (sw, sh, x2) == (640, 652, 640)
