"""What a camera surface must hold after lane and text have been drawn into it in place (lt_overlay_run_inplace), restated in NumPy
from four inputs: the surface's bytes, the annotated RGB frame A the existing route returns for it, tests/yuv_reference.py (the
front end's YUV -> RGB) and tests/sink_reference.py (the sinks' RGB -> YUV).  With C = the camera frame as RGB:

    changed = (A != C).any(-1)
    RGB     every changed pixel holds A, every other pixel its own bytes
    4:2:0   Y(p) = luma(A(p)) where changed(p), else the original byte;
            (U, V) of a 2 x 2 block = chroma(A(top-left pixel)) where that pixel changed, else the original bytes

YUV -> RGB -> YUV is not the identity (`round_trip`), so "kept the original bytes" and "converted the whole frame" differ -- on
noise at most of the bytes.  Test infrastructure."""
import numpy as np

import sink_reference as S
import yuv_reference as R


def camera_rgb(frame, layout, in_matrix="bt601"):
    """The camera frame as RGB: the surface itself, or the front end's conversion of it."""
    frame = np.asarray(frame)
    return frame if layout == "rgb" else R.yuv420_to_rgb(frame, layout, in_matrix)


def _join(y, u, v, layout):
    h, w = y.shape
    chroma = np.stack([u, v], -1).reshape(-1) if layout == "nv12" else np.concatenate([u.reshape(-1), v.reshape(-1)])
    return np.concatenate([y.reshape(-1), chroma]).reshape(h * 3 // 2, w)


def expected(frame, annotated, layout, in_matrix="bt601", out_matrix="bt601"):
    """One frame -- (H, W, 3) RGB or (H * 3 // 2, W) 4:2:0 -- and its annotated RGB frame -> (the frame after the in-place draw,
    the mask of changed pixels)."""
    frame, a = np.asarray(frame), np.asarray(annotated)
    c = camera_rgb(frame, layout, in_matrix)
    changed = (a != c).any(-1)
    if layout == "rgb":
        out = frame.copy()
        out[changed] = a[changed]
        return out, changed
    y, u, v = R.split_planes(frame, layout)
    yn, _, _ = S.forward_triples(a[..., 0], a[..., 1], a[..., 2], out_matrix)
    tl = a[0::2, 0::2]
    _, un, vn = S.forward_triples(tl[..., 0], tl[..., 1], tl[..., 2], out_matrix)
    ctl = changed[0::2, 0::2]
    return _join(np.where(changed, yn, y), np.where(ctl, un, u), np.where(ctl, vn, v), layout), changed


def round_trip(frame, layout, in_matrix="bt601", out_matrix="bt601"):
    """A 4:2:0 frame converted to RGB and back, whole: what an in-place draw must NOT do to the pixels it did not draw on."""
    return S.rgb_to_yuv420(R.yuv420_to_rgb(frame, layout, in_matrix), layout, out_matrix)


def block_expected(y4, u, v, lane4, alpha4, in_matrix="bt601", out_matrix="bt601", alpha=0.3):
    """2 x 2 blocks one by one, for the host build of the arithmetic (tests/inplace_arith_host.cpp): y4 (n, 4) -- top left, top right,
    bottom left, bottom right --, u, v (n,), the lane's value and the glyph's alpha per pixel (n, 4; 0: none)
    -> (y4, u, v after the draw, changed (n, 4) bool).  Lane: cv::addWeighted(img, 1, lane, alpha, 0) of the green byte in f32,
    rounded half to even; text: white over the frame, v + ((255 - v) * a + 127) // 255."""
    y4, lane4, alpha4 = np.asarray(y4, np.int64), np.asarray(lane4, np.int64), np.asarray(alpha4, np.int64)
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    c = R.convert_triples(y4, u[:, None].repeat(4, 1), v[:, None].repeat(4, 1), in_matrix).astype(np.int64)      # (n, 4, 3)
    a = c.copy()
    g = (a[..., 1].astype(np.float32) + (lane4.astype(np.float32) * np.float32(alpha)).astype(np.float32)).astype(np.float32)
    a[..., 1] = np.where(lane4 != 0, np.clip(np.rint(g), 0, 255).astype(np.int64), a[..., 1])
    over = a + ((255 - a) * alpha4[..., None] + 127) // 255
    a = np.where((alpha4 != 0)[..., None], over, a)
    changed = (a != c).any(-1)
    yn, un, vn = S.forward_triples(a[..., 0], a[..., 1], a[..., 2], out_matrix)
    return (np.where(changed, yn, y4).astype(np.uint8), np.where(changed[:, 0], un[:, 0], u).astype(np.uint8),
            np.where(changed[:, 0], vn[:, 0], v).astype(np.uint8), changed)
