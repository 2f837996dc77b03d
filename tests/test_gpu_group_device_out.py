"""LaneTrackerGroup.process(out=...): the annotated frames of a tick written into device sinks by one launch, or drawn into the
DeviceFrames handed in.  Three cameras of different calibrations (A, B, E of calibration_cameras), six ticks, one stream that skips
every third tick and one whose every second frame fails its first try.  Everything is bit for bit against solo trackers; the sinks'
pitch padding and the surfaces of skipped streams keep their fill."""
import copy
import functools

import numpy as np
import pytest

import calibration_cameras as CC
import yuv_reference as R
from test_gpu_chain import _stream_with_failures
from test_gpu_group import _lockstep

pytestmark = pytest.mark.gpu

NAMES, K, N, FILL = "ABE", 3, 6, 0xC3
SKIPPER, FAILING = 1, 2                   # stream 1 skips ticks 1 and 4; stream 2's frames 1, 3, 5 are noise, grey, black


@functools.lru_cache(maxsize=None)
def _videos():
    """Per stream N + 1 RGB frames (the last one for a tick after the six)."""
    cams = CC.cameras()
    vids = [_stream_with_failures(N + 1, 2 if i == FAILING else 1000, seed=5 + 13 * i, cal=cams["A"]) for i in range(K)]
    vids[1] = CC.shifted(vids[1])
    for v in vids:
        v.setflags(write=False)
    return vids


def _ticks():
    """[(stream -> index of its frame or None)] for the six ticks."""
    pos, ticks = [0] * K, []
    for t in range(N):
        tick = []
        for i in range(K):
            skip = i == SKIPPER and t % 3 == 1
            tick.append(None if skip else pos[i])
            pos[i] += 0 if skip else 1
        ticks.append(tick)
    return ticks


def _as_input(frame, pixel_format):
    return frame if pixel_format == "rgb" else R.rgb_to_yuv420(frame, pixel_format)


def _group(pixel_format):
    from lane_tracker_amd import LaneTrackerGroup
    cams = CC.cameras()
    g = LaneTrackerGroup(K, **cams["A"], pixel_format=pixel_format, calibrations=[None, CC.overrides(cams["B"]), CC.overrides(cams["E"])])
    assert g.calibration_count() == 3
    return g


def _solos(pixel_format):
    from lane_tracker_amd.lane_tracker import LaneTracker
    cams = CC.cameras()
    return [LaneTracker(**cams[x], pixel_format=pixel_format) for x in NAMES]


@functools.lru_cache(maxsize=None)
def _reference(pixel_format):
    """The solo trackers over the ticks, once per input format: per tick and stream (annotated RGB frame, state), None where skipped."""
    solos = _solos(pixel_format)
    try:
        out = []
        for tick in _ticks():
            row = []
            for i, j in enumerate(tick):
                if j is None:
                    row.append(None)
                    continue
                want = np.array(solos[i].process(_as_input(_videos()[i][j], pixel_format)))
                row.append((want, copy.deepcopy(solos[i].get_state())))
            out.append(row)
        assert all(s.success > 0 for s in solos)
        return out
    finally:
        for s in solos:
            s.close()


class _SecondTries:
    """Counts the group's second-try searches (a condition of the tests)."""

    def __init__(self, group):
        self.count, self._k, self._orig = 0, group.k, group._search
        group._search = self._search

    def _search(self, ts, base, try_, diagnostics):
        self.count += base >= 2 * self._k
        return self._orig(ts, base, try_, diagnostics)


@pytest.mark.parametrize("feed", ["host-rgb", "device-nv12"])
@pytest.mark.parametrize("sink_format", ["rgb", "nv12", "i420"])
def test_a_tick_into_device_sinks(sink_format, feed):
    from lane_tracker_amd import utils
    from lane_tracker_amd.device import DeviceFrames, pack_host_frames
    pixel_format = "rgb" if feed == "host-rgb" else "nv12"
    ref = _reference(pixel_format)
    W, H = CC.cameras()["A"]["img_size"]
    pitch = (3 * W if sink_format == "rgb" else W) + 6
    g = _group(pixel_format)
    sink = DeviceFrames.empty(K, (W, H), sink_format, pitch=pitch, fill=FILL)
    held = np.full((K,) + ((H, W, 3) if sink_format == "rgb" else (H * 3 // 2, W)), FILL, np.uint8)   # what the surfaces hold
    try:
        seen = _SecondTries(g)
        for t, tick in enumerate(_ticks()):
            frames, keep = [], []
            for i, j in enumerate(tick):
                if j is None:
                    frames.append(None)
                elif feed == "host-rgb":
                    frames.append(_videos()[i][j])
                else:
                    keep.append(DeviceFrames.from_host(_as_input(_videos()[i][j], "nv12"), "nv12", pitch=W + 6))
                    frames.append(keep[-1])
            outs = g.process(frames, out=sink)
            assert g._ctx.last_overlay_launches() == 1, t
            for i, j in enumerate(tick):
                if j is None:
                    assert outs[i] is None
                    continue
                want, state = ref[t][i]
                held[i] = want if sink_format == "rgb" else utils.rgb_to_yuv(want, sink_format, "bt601")
                assert np.array_equal(outs[i].to_host(), held[i]), (t, i)
                assert g.trackers[i].get_state() == state, (t, i)
            # the whole block: skipped streams' surfaces and every byte of padding as they were
            assert np.array_equal(sink.owner.copy_to_host(), pack_host_frames(held, sink_format, pitch, fill=FILL)[0]), t
            for f in keep:
                f.owner.close()
        assert seen.count > 0, "no tick needed a second try"
    finally:
        g.close()
        sink.owner.close()


@pytest.mark.parametrize("pixel_format", ["rgb", "nv12"])
def test_a_tick_drawn_into_the_frames_handed_in(pixel_format):
    from lane_tracker_amd.device import DeviceFrames
    W, H = CC.cameras()["A"]["img_size"]
    pitch = (3 * W if pixel_format == "rgb" else W) + 6
    g, solos = _group(pixel_format), _solos(pixel_format)
    live = []
    try:
        # A group member's state is that of a solo process() (tests/test_gpu_group*.py).  process_batch() of one frame leaves the same
        # state except for the size of its NEXT speculative outage group, a scheduling hint that only its chained route adapts (4, 8,
        # .. while whole groups fail) and process() never touches.  With the knob off, a frame whose first try failed is handled
        # alone, as process() handles it, and the whole get_state() is comparable.
        for s in solos:
            s.outage_groups = False
        seen = _SecondTries(g)
        last = None
        for t, tick in enumerate(_ticks()):
            frames, twins = [], []
            for i, j in enumerate(tick):
                if j is None:
                    frames.append(None)
                    twins.append(None)
                    continue
                host = _as_input(_videos()[i][j], pixel_format)
                frames.append(DeviceFrames.from_host(host, pixel_format, pitch=pitch))
                twins.append(DeviceFrames.from_host(host, pixel_format, pitch=pitch))
                live += [frames[-1], twins[-1]]
            before = seen.count
            outs = g.process(frames, out="inplace")
            assert g._ctx.last_overlay_launches() == 1, t
            for i, j in enumerate(tick):
                if j is None:
                    assert outs[i] is None
                    continue
                assert outs[i] is frames[i]
                solos[i].process_batch(twins[i], out="inplace")
                assert np.array_equal(frames[i].owner.copy_to_host(), twins[i].owner.copy_to_host()), (t, i)
                assert g.trackers[i].get_state() == solos[i].get_state(), (t, i)
            last = (frames, seen.count > before)
        assert seen.count > 0 and last[1], "the last tick needed no second try"
        assert all(f is not None for f in last[0])
        # Nothing is left attached -- not the first tries' slots, not the spare slot of the second try: the surfaces the last tick
        # drew into are accepted as the sink of the next one.
        again = DeviceFrames(np.concatenate([f.surfaces for f in last[0]]), (W, H), pixel_format, owner=last[0])
        tick = [_as_input(v[N], pixel_format) for v in _videos()]
        outs = g.process(tick, out=again)
        assert g._ctx.last_overlay_launches() == 1
        from lane_tracker_amd import utils
        for i in range(K):
            want = np.array(solos[i].process(tick[i]))
            want = want if pixel_format == "rgb" else utils.rgb_to_yuv(want, pixel_format, "bt601")
            assert np.array_equal(outs[i].to_host(), want), i
            assert g.trackers[i].get_state() == solos[i].get_state(), i
    finally:
        g.close()
        for s in solos:
            s.close()
        for f in live:
            f.owner.close()


def test_without_out_a_mixed_group_still_equals_the_solo_trackers():
    g, solos = _group("rgb"), _solos("rgb")
    try:
        ticks = [[None if j is None else _videos()[i][j] for i, j in enumerate(tick)] for tick in _ticks()]
        _lockstep(g, solos, ticks)
        assert g._ctx.last_overlay_launches() == 1
    finally:
        g.close()
        for s in solos:
            s.close()
