"""Device sinks without a GPU: the layout `DeviceFrames.empty` gives a sink is the one `pack_host_frames` gives frames, the sink's
keyword rules, and the raw 4:2:0 files `video.FrameSink` writes are the ones `video.FrameSource` reads."""
import numpy as np
import pytest

import sink_reference as S
from lane_tracker_amd import _native, video
from lane_tracker_amd.device import _layout_block, pack_host_frames


@pytest.mark.parametrize("layout,pitch,cpitch,offset", [("rgb", None, None, 0), ("rgb", 3 * 18 + 7, None, 5), ("nv12", None, None, 0),
                                                       ("nv12", 18 + 5, 18 + 9, 3), ("i420", None, None, 0), ("i420", 18 + 6, 9 + 5, 1)])
def test_a_sink_is_laid_out_like_packed_frames(layout, pitch, cpitch, offset):
    w, h, n = 18, 4, 3
    rgb = np.random.default_rng(1).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    frames = rgb if layout == "rgb" else S.rgb_to_yuv420(rgb, layout)
    block, surf, size, _ = pack_host_frames(frames, layout, pitch, cpitch, offset)
    total, sink_surf, sizes = _layout_block(n, (w, h), layout, pitch, cpitch, offset)
    assert size == (w, h) and total == block.nbytes and np.array_equal(sink_surf, surf)
    last_rows, last_rb, last_pitch = sizes[-1]
    assert int(surf["plane"][-1, len(sizes) - 1]) + last_pitch * (last_rows - 1) + last_rb == total      # ends on the last byte of the last plane
    for bad in (dict(pitch=sizes[0][1] - 1), dict(offset=-1)) + ((dict(chroma_pitch=sizes[1][1] - 1),) if layout != "rgb" else ()):
        with pytest.raises(ValueError):
            _layout_block(n, (w, h), layout, **{**dict(pitch=None, chroma_pitch=None, offset=0), **bad})
    if layout != "rgb":
        with pytest.raises(ValueError):
            _layout_block(n, (w + 1, h), layout, None, None, 0)


def test_matrix_names_and_shapes():
    assert tuple(_native.rgb2yuv_coeffs("bt601")) == S.MATRICES["bt601"] and tuple(_native.rgb2yuv_coeffs("bt709")) == S.MATRICES["bt709"]
    assert tuple(_native.rgb2yuv_coeffs(S.CLAMPING)) == S.CLAMPING
    for bad in ("bt2020", (1, 2, 3, 4, 5)):
        with pytest.raises(ValueError):
            _native.rgb2yuv_coeffs(bad)
    for name in ("lt_rgb_to_surfaces", "lt_overlay_store_device", "lt_overlay_store_wait"):
        assert name in _native.exported_symbols()


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_frame_sink_writes_raw_420_files_the_source_reads(tmp_path, layout):
    w, h = 18, 4
    frames = S.rgb_to_yuv420(np.random.default_rng(2).integers(0, 256, (5, h, w, 3), dtype=np.uint8), layout)
    path = str(tmp_path / ("out." + layout))
    with video.FrameSink(path, (w, h), pixel_format=layout) as sink:
        sink.write(frames[:3])
        sink.write(frames[3])
        sink.write(frames[4:])
        with pytest.raises(ValueError):
            sink.write(np.zeros((h, w, 3), np.uint8))
    src = video.FrameSource(path, (w, h))
    assert src.pixel_format == layout and len(src) == 5 and np.array_equal(src.read(0, 5), frames)
    with pytest.raises(ValueError):
        video.FrameSink(str(tmp_path / "out.rgb"), (w, h), pixel_format=layout)
