"""LaneTrackerGroup(calibrations=...): every stream a camera of its own calibration.  For every stream the annotated frames and the
whole tracker state after every tick equal those of a solo LaneTracker built with that camera's calibration."""
import numpy as np
import pytest

import calibration_cameras as CC
import yuv_reference as R
from test_gpu_group import _lockstep, _streams

pytestmark = pytest.mark.gpu


def test_group_of_four_cameras_equals_four_solo_trackers():
    from lane_tracker_amd import LaneTrackerGroup
    from lane_tracker_amd.lane_tracker import LaneTracker
    cams = CC.cameras()
    names, k, n = "ABCD", 4, 24
    vids = _streams(k, n, cams["A"], seed=41)
    vids[1] = CC.shifted(vids[1])
    skipper = 2                                                   # this stream skips every third tick
    pos, ticks = [0] * k, []
    for t in range(n):
        tick = []
        for i in range(k):
            skip = i == skipper and t % 3 == 2
            tick.append(None if skip else vids[i][pos[i]])
            pos[i] += 0 if skip else 1
        ticks.append(tick)
    g = LaneTrackerGroup(k, **cams["A"], calibrations=[None] + [CC.overrides(cams[x]) for x in names[1:]])
    solos = [LaneTracker(**cams[x]) for x in names]
    try:
        assert g.calibration_count() == 4
        for t, s, x in zip(g.trackers, solos, names):
            assert np.array_equal(t.Minv, cams[x]["warp_matrices"][1]) and np.array_equal(t.cam_matrix, s.cam_matrix)
        _lockstep(g, solos, ticks)
        assert [t.counter for t in g.trackers] == pos
        # the streams are real lanes for their cameras: judged on the solo trackers
        assert all(0 < s.success for s in solos), [s.success for s in solos]
        good = 0
        for i, s in enumerate(solos):
            outage = len([j for j in range(8 + 3 * i, 8 + 3 * i + 6) if j < pos[i]])
            good += 2 * s.success >= pos[i] - outage
        assert good >= 3, [(s.success, p) for s, p in zip(solos, pos)]
    finally:
        g.close()
        for s in solos:
            s.close()


def test_group_of_three_nv12_cameras_in_device_memory():
    from lane_tracker_amd import LaneTrackerGroup
    from lane_tracker_amd.device import DeviceFrames
    from lane_tracker_amd.lane_tracker import LaneTracker
    cams = CC.cameras()
    names, k, n, layout = "ABE", 3, 6, "nv12"
    rgb = _streams(k, n, cams["A"], seed=5)
    rgb[1] = CC.shifted(rgb[1])
    vids = [np.stack([R.rgb_to_yuv420(f, layout) for f in v]) for v in rgb]
    W = cams["A"]["img_size"][0]
    dev = [DeviceFrames.from_host(v, layout, pitch=W + 6) for v in vids]
    g = LaneTrackerGroup(k, **cams["A"], pixel_format=layout, calibrations=[None, CC.overrides(cams["B"]), CC.overrides(cams["E"])])
    solos = [LaneTracker(**cams[x], pixel_format=layout) for x in names]
    try:
        assert g.calibration_count() == 3
        for t in range(n):
            outs = g.process([d[t] for d in dev])
            for i in range(k):
                want = solos[i].process(vids[i][t])
                assert np.array_equal(outs[i], want), (t, i)
                assert g.trackers[i].get_state() == solos[i].get_state(), (t, i)
        assert all(s.success > 0 for s in solos)
    finally:
        g.close()
        for s in solos:
            s.close()


def test_equal_calibrations_share_a_set_and_close_returns_the_memory():
    from lane_tracker_amd import LaneTrackerGroup, _native, synth
    cams = CC.cameras()
    k = 4
    vids = [synth.stream_lanes(8, seed=60 + i) for i in range(k)]
    before = _native.device_cache_stats()["live_bytes"]
    own = CC.overrides(cams["A"])
    g = LaneTrackerGroup(k, **cams["A"], calibrations=[None, own, dict(cam_matrix=cams["A"]["cam_matrix"].copy()), {}])
    try:
        assert g.calibration_count() == 1 and g._ctx.calibration_count() == 1
        g.process([v[0] for v in vids])
    finally:
        g.close()
    assert _native.device_cache_stats()["live_bytes"] == before
    # ... and a group that does hold several sets: two streams share camera C's
    g = LaneTrackerGroup(k, **cams["A"], calibrations=[CC.overrides(cams["C"]), None, CC.overrides(cams["C"]), CC.overrides(cams["D"])])
    try:
        assert g.calibration_count() == 3
        for t in range(4):
            g.process([v[t] if (t + i) % 3 else None for i, v in enumerate(vids)], annotate=bool(t % 2))
        warm = _native.device_cache_stats()["live_bytes"]
        for t in range(4, 8):
            g.process([v[t] if (t + i) % 3 else None for i, v in enumerate(vids)], annotate=bool(t % 2))
        assert _native.device_cache_stats()["live_bytes"] == warm
    finally:
        g.close()
    assert _native.device_cache_stats()["live_bytes"] == before
