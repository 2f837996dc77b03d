"""MI355X-native lane-tracker hot path (undistort -> warp -> filter_lane_points ->
sliding_window_search / band_search -> fit_poly) behind the reference's LaneTracker API."""
__version__ = "0.1.0"


def __getattr__(name):
    # LaneTrackerGroup (lane_tracker_amd/group.py) on first use: importing the package stays as light as before
    if name == "LaneTrackerGroup":
        from .group import LaneTrackerGroup
        return LaneTrackerGroup
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
