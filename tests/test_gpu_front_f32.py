"""The front end's blend and Lab tail (lane_tracker_amd/csrc/front_arith.h) on the device, bit for bit against the oracle:
a quarter-scale geometry whose bird's-eye view has all three classes of k_warp_split4's quads (inside / none / border) over an
odd run of slots, every RGB triple through the Lab tail at an identity geometry, the reference geometry, and a 4:2:0 context
(the 4:2:0 walks share the undistortion's blend)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from lane_tracker_amd import _native
    _native.load()
    return _native


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (f"{what}: {bad.shape[0]} of {got.size} differ; first at {bad[:5].tolist()} "
                               f"got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}")


def check_front_end(c, oracle, oc, frames, first):
    n = frames.shape[0]
    c.upload_frames(frames, first=first)
    c.mask_run(n, first=first)
    und = c.download_undistorted(n, first=first)
    R, B = c.download_plane(0, n, first=first), c.download_plane(1, n, first=first)
    r0, r1 = oracle.warp_source_rows(oc)
    for k in range(n):
        assert_same(und[k], oracle.undistort(oc, frames[k])[r0:r1], f"undistorted rows, frame {k}")
        bev = oracle.front_end(oc, frames[k])
        assert_same(R[k], bev[:, :, 0], f"R plane, frame {k}")
        assert_same(B[k], oracle.lab_b(bev), f"Lab-b plane, frame {k}")


QUARTER = dict(img_size=(320, 180), warped=(272, 276))


def quarter_geometry():
    from lane_tracker_amd import calib
    S = np.diag([0.25, 0.25, 1.0])
    return S @ calib.CAM_MATRIX, calib.DIST_COEFFS, S @ calib.M @ np.diag([4.0, 4.0, 1.0])


def quad_classes(oracle, oc):
    """(inside, none, border) counts of the 4-pixel quads of the bird's-eye view, from the warp table, as k_warp_split4 sorts them."""
    xy, _ = oracle.warp_map(oc)
    r0, r1 = oracle.warp_source_rows(oc)
    sx, sy = xy[..., 0].astype(np.int64).reshape(-1, 4), xy[..., 1].astype(np.int64).reshape(-1, 4)
    inside = ((sx >= 0) & (sx + 1 < oc.img_w) & (sy >= r0) & (sy + 1 < r1) & (sy + 1 < oc.img_h)).all(axis=1)
    yin = lambda y: (y >= 0) & (y < oc.img_h) & (y >= r0) & (y < r1)
    xin = lambda x: (x >= 0) & (x < oc.img_w)
    none = (~((yin(sy) | yin(sy + 1)) & (xin(sx) | xin(sx + 1)))).all(axis=1)
    return int(inside.sum()), int((none & ~inside).sum()), int((~inside & ~none).sum())


def test_quarter_scale_all_quad_classes_odd_slot_run(nat, oracle):
    """Camera 320x180, bird's-eye 272x276 (a multiple of 4 wide: k_warp_split4), 19 frames in slots 1..19 of 20: an odd first
    slot, an odd count, more than the 16 slots of one walk."""
    K, D, M = quarter_geometry()
    oc = oracle.make_calib(QUARTER["img_size"], QUARTER["warped"], K, D, M)
    inside, none, border = quad_classes(oracle, oc)
    assert inside > 0 and none > 0 and border > 0, (inside, none, border)
    h, w = 180, 320
    rng = np.random.default_rng(31)
    frames = rng.integers(0, 256, (19, h, w, 3), dtype=np.uint8)
    frames[0] = 0
    frames[1] = 255
    yy, xx = np.mgrid[0:h, 0:w]
    frames[2] = (((yy + xx) & 1) * 255).astype(np.uint8)[..., None]                   # one-pixel 0 / 255 checkerboard
    sat = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (255, 255, 255), (0, 0, 0)], np.uint8)
    frames[3] = sat[((yy // 9) * 3 + xx // 16) % 8]                                   # saturated colour blocks
    frames[4] = np.where(((yy + xx) & 1)[..., None] == 1, sat[(xx // 5) % 8], 0)
    c = nat.Context(QUARTER["img_size"], QUARTER["warped"], K, D, M, device=0, capacity=20)
    try:
        check_front_end(c, oracle, oc, frames, first=1)
    finally:
        c.close()


def test_every_rgb_triple_through_the_lab_tail(nat, oracle):
    """Zero distortion, identity warp, camera = bird's-eye = 512x512: every fraction is 0, so each bird's-eye pixel is a camera
    pixel, and 64 frames enumerate all 2^24 RGB triples."""
    K = np.array([[500.0, 0.0, 256.0], [0.0, 500.0, 256.0], [0.0, 0.0, 1.0]])
    D, M = np.zeros(5), np.eye(3)
    size = (512, 512)
    oc = oracle.make_calib(size, size, K, D, M)
    wxy, wfr = oracle.warp_map(oc)
    uxy, ufr = oracle.undistort_map(oc)
    yy, xx = np.mgrid[0:512, 0:512]
    for xy, fr in ((wxy, wfr), (uxy, ufr)):
        assert not fr.any() and np.array_equal(xy[..., 0], xx) and np.array_equal(xy[..., 1], yy)
    v = (np.arange(64, dtype=np.uint32)[:, None, None] << 18) + (yy * 512 + xx).astype(np.uint32)[None]
    frames = np.stack([v & 255, (v >> 8) & 255, v >> 16], axis=-1).astype(np.uint8)
    assert np.unique(frames.reshape(-1, 3).astype(np.uint32) @ np.array([1, 256, 65536], np.uint32)).size == 1 << 24
    c = nat.Context(size, size, K, D, M, device=0, capacity=64)
    try:
        c.upload_frames(frames)
        c.mask_run(64)
        R, B = c.download_plane(0, 64), c.download_plane(1, 64)
        assert_same(R, frames[..., 0], "R plane")
        assert_same(B, oracle.lab_b(frames), "Lab-b plane")
        assert_same(c.download_undistorted(64), frames, "undistorted rows")
    finally:
        c.close()


def test_reference_geometry_scene_and_noise(nat, oracle, ref_calib):
    from lane_tracker_amd import calib, synth
    cal = calib.reference_calibration()
    rng = np.random.default_rng(77)
    noise = rng.integers(0, 256, (720, 1280, 3), dtype=np.uint8)
    noise[:, 300:340] = (255, 255, 255)
    noise[:, 620:660] = (255, 255, 0)
    noise[:, 900:940] = (0, 0, 255)
    noise[500:520] = (255, 0, 0)
    frames = np.stack([synth.SceneRenderer().render(1)[0], noise])
    c = nat.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0],
                    device=0, capacity=2)
    try:
        check_front_end(c, oracle, ref_calib, frames, first=0)
    finally:
        c.close()


def test_nv12_context_rows_equal_the_rgb_contexts(nat):
    """The 4:2:0 walks convert every tap and then run the same blend: their undistorted rows are those of an RGB context fed
    utils.yuv_to_rgb of the same frames."""
    from lane_tracker_amd import utils
    K, D, M = quarter_geometry()
    rng = np.random.default_rng(41)
    yuv = rng.integers(0, 256, (3, 270, 320), dtype=np.uint8)
    yuv[1, :180] = (((np.mgrid[0:180, 0:320].sum(axis=0)) & 1) * 255).astype(np.uint8)     # checkerboard luma under random chroma
    rgb = np.stack([utils.yuv_to_rgb(f, layout="nv12") for f in yuv])
    a = nat.Context(QUARTER["img_size"], QUARTER["warped"], K, D, M, device=0, capacity=3)
    b = nat.Context(QUARTER["img_size"], QUARTER["warped"], K, D, M, device=0, capacity=3)
    try:
        a.set_input_format("nv12")
        a.upload_frames(yuv)
        a.mask_run(3)
        b.upload_frames(rgb)
        b.mask_run(3)
        assert_same(a.download_undistorted(3), b.download_undistorted(3), "undistorted rows")
        assert_same(a.download_plane(1, 3), b.download_plane(1, 3), "Lab-b plane")
    finally:
        a.close()
        b.close()
