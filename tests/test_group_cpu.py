"""LaneTrackerGroup's boundary without a GPU: the package exports the class, the list item has the header's layout, and the
group's argument checks come before any device work."""
import ctypes as C

import pytest


def test_package_exports_the_group():
    import lane_tracker_amd
    from lane_tracker_amd.group import LaneTrackerGroup
    assert lane_tracker_amd.LaneTrackerGroup is LaneTrackerGroup


def test_search_item_layout():
    from lane_tracker_amd import _native
    assert C.sizeof(_native.SearchItem) == 64 and _native.SEARCH_ITEM_DTYPE.itemsize == 64
    assert _native.SearchItem.prev_coeffs.offset == 16 and _native.SEARCH_ITEM_DTYPE.fields["prev_coeffs"][1] == 16


def test_group_needs_a_stream():
    from lane_tracker_amd import LaneTrackerGroup, calib
    with pytest.raises(ValueError):
        LaneTrackerGroup(0, **calib.reference_calibration())
