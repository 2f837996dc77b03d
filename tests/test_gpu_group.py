"""LaneTrackerGroup: K independent streams advanced one frame each per call in one batch.  For every stream the annotated frames
and the whole tracker state after every call equal those of a solo LaneTracker.process() fed the same frames -- with failures,
outages (sliding windows again after n_reset misses), second tries, skipped streams, hand-overs between the two, and the list
search entry point itself against the range forms slot by slot."""
import threading

import numpy as np
import pytest

from test_gpu_chain import _stream_with_failures
from test_gpu_process_tail import _full

pytestmark = pytest.mark.gpu


def _streams(k, n, cal, seed):
    """k different videos: drifting lanes with failures at different rates, each with an outage at its own place."""
    out = []
    for i in range(k):
        f = _stream_with_failures(n, 5 + 2 * i, seed=seed + 13 * i, cal=cal)
        a = 8 + 3 * i
        f[a:a + 6] = 0                  # an outage: sliding windows after n_reset misses (:851)
        out.append(f)
    return out


def _lockstep(group, solos, ticks, annotate=True, kw=None, on_tick=None):
    """Feed `ticks` (lists of k frames or None) to the group and each stream's frames to its solo tracker; compare after every tick."""
    kw = kw or {}
    for n, tick in enumerate(ticks):
        outs = group.process(tick, annotate=annotate, **kw)
        for i, f in enumerate(tick):
            t = group.trackers[i]
            if f is None:
                assert outs[i] is None
                continue
            want = solos[i].process(f, **kw)
            if annotate:
                assert outs[i] is not None and np.array_equal(outs[i], want), (n, i)
            else:
                assert outs[i] is None
            assert _full(t) == _full(solos[i]), (n, i)
            assert t.left_window_centroids == solos[i].left_window_centroids, (n, i)
            assert t.right_window_centroids == solos[i].right_window_centroids, (n, i)
        if on_tick is not None:
            on_tick(n, tick)


class _Modes:
    """What the ticks exercised: search modes per tick, and which streams needed the second try."""

    def __init__(self, group):
        self.mixed = self.partial_second = False
        self._g = group
        self._orig = group._search
        group._search = self._search

    def _search(self, ts, base, try_, diagnostics):
        modes = {t.last_detection > t.n_reset for t in ts}
        if base < 2 * self._g.k:        # a first try
            self.mixed |= len(modes) == 2
            self._first = len(ts)
        elif len(ts) < self._first:
            self.partial_second = True
        return self._orig(ts, base, try_, diagnostics)


def test_group_of_four_equals_four_solo_trackers():
    from lane_tracker_amd import LaneTrackerGroup, calib
    from lane_tracker_amd.lane_tracker import LaneTracker
    cal = calib.reference_calibration()
    k, n = 4, 48
    vids = _streams(k, n, cal, seed=41)
    g = LaneTrackerGroup(k, **cal)
    solos = [LaneTracker(**cal) for _ in range(k)]
    try:
        seen = _Modes(g)
        _lockstep(g, solos, [[v[t] for v in vids] for t in range(n)])
        assert seen.mixed, "no tick mixed sliding-window and band frames"
        assert seen.partial_second, "no tick where only some streams needed the second try"
        assert all(0 < s.success < n for s in solos)
    finally:
        g.close()
        for s in solos:
            s.close()


def test_group_of_eight_at_1080p_with_demo_settings():
    from lane_tracker_amd import LaneTrackerGroup, calib, settings
    from lane_tracker_amd.lane_tracker import LaneTracker
    cal = calib.scaled_calibration(1.5)
    k, n = 8, 24
    vids = _streams(k, n, cal, seed=7)
    g = LaneTrackerGroup(k, print_frame_count=True, **cal)
    solos = [LaneTracker(print_frame_count=True, **cal) for _ in range(k)]
    try:
        kw = {}
        for t in g.trackers + solos:
            kw = settings.apply(t, settings.DEMOS["demo1"])
        _lockstep(g, solos, [[v[t] for v in vids] for t in range(n)], kw=kw)
    finally:
        g.close()
        for s in solos:
            s.close()


@pytest.mark.parametrize("k", [1, 5])
def test_ragged_ticks_equal_each_stream_over_its_own_frames(k):
    from lane_tracker_amd import LaneTrackerGroup, calib
    from lane_tracker_amd.lane_tracker import LaneTracker
    cal = calib.reference_calibration()
    n = 30
    vids = _streams(k, n, cal, seed=3)
    rng = np.random.default_rng(5 + k)
    pos = [0] * k
    ticks = []
    for t in range(n):
        tick = []
        for i in range(k):
            skip = t == 6 or rng.random() < 0.3          # tick 6: every stream skips
            tick.append(None if skip else vids[i][pos[i]])
            pos[i] += 0 if skip else 1
        ticks.append(tick)
    g = LaneTrackerGroup(k, **cal)
    solos = [LaneTracker(**cal) for _ in range(k)]
    try:
        counters = []
        _lockstep(g, solos, ticks, on_tick=lambda n_, tick: counters.append([t.counter for t in g.trackers]))
        assert counters[6] == counters[5]
        assert [t.counter for t in g.trackers] == pos
    finally:
        g.close()
        for s in solos:
            s.close()


def test_annotate_false_leaves_the_same_states():
    from lane_tracker_amd import LaneTrackerGroup, calib
    cal = calib.reference_calibration()
    k, n = 3, 24
    vids = _streams(k, n, cal, seed=19)
    a, b = LaneTrackerGroup(k, **cal), LaneTrackerGroup(k, **cal)
    try:
        for t in range(n):
            tick = [v[t] for v in vids]
            outs = a.process(tick, annotate=False)
            assert outs == [None] * k
            b.process(tick)
            for i in range(k):
                assert _full(a.trackers[i]) == _full(b.trackers[i]), (t, i)
    finally:
        a.close()
        b.close()


def test_hand_over_between_solo_and_group_both_ways():
    from lane_tracker_amd import LaneTrackerGroup, calib
    from lane_tracker_amd.lane_tracker import LaneTracker
    cal = calib.reference_calibration()
    k, n, h = 4, 40, 20
    vids = _streams(k, n, cal, seed=23)
    g = LaneTrackerGroup(k, **cal)
    ref = LaneTracker(**cal)              # stream 2 from start to end, solo
    first = LaneTracker(**cal)            # its first half, solo, then handed to the group
    try:
        for t in range(h):
            ref.process(vids[2][t])
            first.process(vids[2][t])
            g.process([vids[i][t] if i != 2 else None for i in range(k)])
        g.trackers[2].set_state(first.get_state())
        for t in range(h, n):
            want = ref.process(vids[2][t])
            got = g.process([v[t] for v in vids])[2]
            assert np.array_equal(got, want), t
            assert _full(g.trackers[2]) == _full(ref), t
        # and back: the group's stream 2 continues solo
        back = LaneTracker(**cal)
        back.set_state(g.trackers[2].get_state())
        extra = _stream_with_failures(12, 4, seed=77, cal=cal)
        for f in extra:
            assert np.array_equal(back.process(f), ref.process(f))
            assert _full(back) == _full(ref)
        back.close()
        with pytest.raises(RuntimeError):
            g.trackers[0].process(vids[0][0])
        with pytest.raises(RuntimeError):
            g.trackers[0].process_batch(vids[0][:2])
        with pytest.raises(NotImplementedError):
            g.process([v[0] for v in vids], visualize_search=True)
    finally:
        for t in (g, ref, first):
            t.close()


def test_search_list_equals_the_range_forms_slot_by_slot():
    from lane_tracker_amd import _native, calib, synth
    cal = calib.reference_calibration()
    n = 8
    frames = _stream_with_failures(n, 4, seed=11)
    frames[5] = synth.stream_lanes(1, seed=99)[0]
    prev = np.array([[1e-4, -0.05, 180.0, 1e-4, -0.05, 460.0]], np.float64) + np.linspace(0, 5, n)[:, None] * [0, 0, 1, 0, 0, 1]

    def ctx():
        c = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0],
                            device=0, capacity=n)
        c.upload_frames(frames)
        c.mask_run(n, _native.filter_params())
        return c

    for ww in (30, 80):                                  # 80: wider than the one-launch kernel takes -> slot by slot
        sws = _native.search_params(window_width=ww)
        band = _native.search_params(bandwidth=25)
        modes = [0, 1, 1, 0, 1, 0, 0, 1]
        order = [5, 2, 7, 0, 3, 6, 1]                    # shuffled, slot 4 left out
        a, b = ctx(), ctx()
        try:
            a.search_fit_list([(s, modes[s], prev[s] if modes[s] else None) for s in order], sws, band)
            for s in order:
                if modes[s] == 0:
                    b.sws_fit_run(1, sws, first=s)
                else:
                    b.band_fit_run(1, prev[s:s + 1], band, first=s)
            ra, rb = a.download_records(n), b.download_records(n)
            for s in order:
                assert ra[s].tobytes() == rb[s].tobytes(), (ww, s)
                for side in (0, 1):
                    for x, y in zip(a.download_pixels(s, side), b.download_pixels(s, side)):
                        assert np.array_equal(x, y), (ww, s, side)
                    if modes[s] == 0:
                        assert np.array_equal(a.download_centroids(s, side), b.download_centroids(s, side)), (ww, s, side)
            assert any(ra[s]["detected"] for s in order if modes[s] == 0) and any(ra[s]["detected"] for s in order if modes[s] == 1)
            LT_ERR_INVALID = -1
            for bad in ([(n, 0, None)], [(1, 2, None)], [(-1, 0, None)], [(1, 0, None), (1, 1, prev[1])]):
                items = np.zeros(len(bad), _native.SEARCH_ITEM_DTYPE)
                for i, (slot, mode, _) in enumerate(bad):
                    items[i]["slot"], items[i]["mode"] = slot, mode
                assert a.lib.lt_search_fit_list(a._h, len(items), items.ctypes.data, sws, band) == LT_ERR_INVALID, bad
            assert a.lib.lt_search_fit_list(a._h, -1, None, sws, band) == LT_ERR_INVALID
        finally:
            a.close()
            b.close()


def test_two_groups_on_two_threads_equal_each_alone():
    from lane_tracker_amd import LaneTrackerGroup, calib
    cal = calib.reference_calibration()
    k, n = 3, 20
    sets = [_streams(k, n, cal, seed=s) for s in (101, 202)]

    def run(vids, box):
        g = LaneTrackerGroup(k, **cal)
        try:
            res = []
            for t in range(n):
                outs = g.process([v[t] for v in vids])
                res.append(([o.copy() for o in outs], [_full(tr) for tr in g.trackers]))
            box.append(res)
        except BaseException as e:       # noqa: BLE001
            box.append(e)
        finally:
            g.close()

    alone = []
    for vids in sets:
        box = []
        run(vids, box)
        alone.append(box[0])
    boxes = [[], []]
    th = [threading.Thread(target=run, args=(sets[i], boxes[i])) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    for i in range(2):
        got = boxes[i][0]
        assert not isinstance(got, BaseException), got
        for (fa, sa), (fb, sb) in zip(got, alone[i]):
            assert all(np.array_equal(x, y) for x, y in zip(fa, fb))
            assert sa == sb


def test_device_memory_is_flat_over_ticks_and_returned_by_close():
    from lane_tracker_amd import LaneTrackerGroup, _native, calib, synth
    cal = calib.reference_calibration()
    k = 8
    vids = [synth.stream_lanes(40, seed=60 + i) for i in range(k)]
    before = _native.device_cache_stats()["live_bytes"]
    g = LaneTrackerGroup(k, **cal)
    try:
        for t in range(20):
            g.process([v[t % 40] if (t + i) % 7 else 0 * v[0] for i, v in enumerate(vids)])
        warm = _native.device_cache_stats()["live_bytes"]
        for t in range(200):
            g.process([v[t % 40] if (t + i) % 7 else 0 * v[0] for i, v in enumerate(vids)])
        assert _native.device_cache_stats()["live_bytes"] == warm
    finally:
        g.close()
    assert _native.device_cache_stats()["live_bytes"] == before


def test_back_to_back_list_searches_on_two_slot_streams():
    """Two list calls one behind the other with nothing waited for in between, over slots of different slot streams (the
    second call's list must not reach the device while the first call's search still reads its own): every slot equals the
    range forms."""
    from lane_tracker_amd import _native, calib
    cal = calib.reference_calibration()
    n = 8
    frames = _stream_with_failures(n, 3, seed=29)
    prev = np.array([[1e-4, -0.05, 180.0, 1e-4, -0.05, 460.0]], np.float64) + np.arange(n)[:, None] * [0, 0, 2.0, 0, 0, -2.0]
    sws, band = _native.search_params(window_width=30), _native.search_params(bandwidth=25)
    calls = ([(0, 0, None), (1, 1, prev[1]), (2, 0, None), (3, 1, prev[3])],       # slots of the first slot stream
             [(6, 1, prev[6]), (4, 0, None), (7, 0, None), (5, 1, prev[5])])       # ... and of the second, other modes

    def ctx():
        c = _native.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0],
                            device=0, capacity=n)
        c.set_streams(2)
        c.upload_frames(frames)
        c.mask_run(n, _native.filter_params())
        return c

    a, b = ctx(), ctx()
    try:
        for _ in range(3):
            for items in calls:
                a.search_fit_list(items, sws, band)
            for items in calls:
                for s, mode, p in items:
                    if mode == 0:
                        b.sws_fit_run(1, sws, first=s)
                    else:
                        b.band_fit_run(1, p[None], band, first=s)
            ra, rb = a.download_records(n), b.download_records(n)
            for s in range(n):
                assert ra[s].tobytes() == rb[s].tobytes(), s
                for side in (0, 1):
                    for x, y in zip(a.download_pixels(s, side), b.download_pixels(s, side)):
                        assert np.array_equal(x, y), (s, side)
            assert ra["detected"].any()
    finally:
        a.close()
        b.close()
