"""Dead tiles of the matrix-core thresholds (csrc/k_threshold_mma.hip): a verdict tile whose own pixels are all <= C is written as
"nothing passes" without its matrix products, and the horizontal tasks collect their words in LDS and write them in one sweep.
The first is exact (C >= 0, window sums >= 0), so every comparison here is for equality:
PLANE_MERGED against the NumPy prefix-sum formula on the oracle's top-hat planes, the masks against the oracle's.

The inputs are built so that the top-hat planes hold chosen values: on a flat grey background a small structure of R + d has R
top-hat value d, and one of blue - BLUE_DELTA[v] has Lab-b top-hat value v.  Every test asserts on the oracle's planes that its
input is what it claims before it looks at the GPU.  Tiles are the kernel's own: 32 x 32 for the horizontal tasks, 32 rows x 128
columns for the vertical ones."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_walk import _bilateral_np
from test_gpu_threshold_mma import _ctx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lane_tracker_amd", "csrc")
EXP_LIB = os.path.join(ROOT, "lane_tracker_amd", "liblane_tracker_amd_exp.so")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (w, h): one 128-column strip and a remainder; the two vertical segments; five 128-column trips and a remainder
SHAPES = [(132, 70), (72, 650), (644, 130)]
PARAMS = [(15, 8, 35, 5), (35, 0, 15, 12)]       # (ksize_r, C_r, ksize_b, C_b)
GREY = 100
BLUE_DELTA = {0: 0, 1: 1, 5: 9, 6: 10, 12: 21, 13: 22}      # blue - d on grey 100 -> that Lab-b top-hat value (asserted below)
BRIGHT = 60                                      # channel offset of a bright blob: far above every C here in either plane


def _kc(params, plane):
    return params[0:2] if plane == "r" else params[2:4]


def _put(img, ys, xs, plane, value):
    """top-hat value `value` of `plane` at img[ys, xs]"""
    if plane == "r":
        img[ys, xs, 0] = GREY + value
    else:
        img[ys, xs, 2] = GREY - BLUE_DELTA[value]


def _put_bright(img, ys, xs, plane):
    img[ys, xs, 0 if plane == "r" else 2] = GREY + BRIGHT if plane == "r" else GREY - BRIGHT


def _vseg_len(h):
    """rows of the first vertical segment: the kernel splits the rows of a strip in two above 640, on a 32-row boundary"""
    return h if h <= 640 else (((h + 1) // 2 + 31) & ~31)


def _tile_max(plane, th, tw):
    h, w = plane.shape
    return np.array([[plane[y:y + th, x:x + tw].max() for x in range(0, w, tw)] for y in range(0, h, th)])


# ---------------------------------------------------------------------------------------------------------------------------
# the inputs (deterministic, no oracle, no GPU: the child processes of the switch test build the same ones)

def isolated_pixels(w, h, params, plane):
    """-> bev, the (y, x) of the C + 1 pixels, the (y, x) of the pixels of exactly C (none for C = 0)"""
    C = _kc(params, plane)[1]
    img = np.full((h, w, 3), GREY, np.uint8)
    hot = [(0, 0), (31, 31), (32, 32), (h - 1, w - 1)]
    if w > 128:
        hot += [(40, 127), (50, 128)]
    if h > 640:
        hot += [(_vseg_len(h) - 1, 10), (_vseg_len(h), 20)]
    taken = {(y // 32, x // 32) for y, x in hot}
    free = [(ty, tx) for ty in range((h + 31) // 32) for tx in range((w + 31) // 32) if (ty, tx) not in taken]
    cold = []
    if C > 0:
        for ty, tx in free[::max(1, len(free) // 6)]:
            cold.append((min(32 * ty + 13, h - 1), min(32 * tx + 17, w - 1)))
    for y, x in hot:
        _put(img, y, x, plane, C + 1)
    for y, x in cold:
        _put(img, y, x, plane, C)
    return img, hot, cold


def noise_and_blobs(w, h, params, plane, seed):
    """background noise of top-hat amplitude <= C (none for C = 0) and about one bright blob of at least 6 x 8 per nine tiles"""
    C = _kc(params, plane)[1]
    rng = np.random.default_rng(seed)
    img = np.full((h, w, 3), GREY, np.uint8)
    if C > 0:
        if plane == "r":
            img[:, :, 0] = GREY + rng.integers(0, C + 1, (h, w))
        else:
            img[:, :, 2] = GREY - rng.integers(0, BLUE_DELTA[C] + 1, (h, w))
    ntiles = ((h + 31) // 32) * ((w + 31) // 32)
    for _ in range(max(1, round(ntiles / 9))):
        bh, bw = int(rng.integers(6, 9)), int(rng.integers(8, 11))
        y, x = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
        _put_bright(img, slice(y, y + bh), slice(x, x + bw), plane)
    return img


H_RUNS = [1, 0, 0, 1, 0, 1, 0, 0]                # liveness of the eight 32 x 32 tiles of trips 0 and 1 of one row group
V_RUNS = [[1, 0, 0, 1], [0, 1, 0, 0]]            # liveness of tiles 0 .. 3 down the 128-column strips 0 and 1


def _fill_tile(img, y0, x0, th, tw, plane, C, live):
    """a live tile: C + 1 in its corners and a bright blob; a dead one: the same structures with value C (nothing for C = 0)"""
    h, w = img.shape[:2]
    y1, x1 = min(y0 + th, h) - 1, min(x0 + tw, w) - 1
    v = C + 1 if live else C
    if v == 0:
        return
    for y, x in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
        _put(img, y, x, plane, v)
    ys, xs = slice(y0 + 12, y0 + 18), slice(x0 + 10, x0 + 18)
    if live:
        _put_bright(img, ys, xs, plane)
    else:
        _put(img, ys, xs, plane, v)


def runs_in_a_trip(w, h, params, plane):
    """-> two frames: live / dead runs along one row group (rows 32 .. 63); the same down two 128-column strips"""
    C = _kc(params, plane)[1]
    assert w >= 256 and h >= 128
    a = np.full((h, w, 3), GREY, np.uint8)
    for t, live in enumerate(H_RUNS):
        _fill_tile(a, 32, 32 * t, 32, 32, plane, C, live)
    b = np.full((h, w, 3), GREY, np.uint8)
    for s, col in enumerate(V_RUNS):
        for t, live in enumerate(col):
            _fill_tile(b, 32 * t, 128 * s, 32, 128, plane, C, live)
    return a, b


def all_inputs():
    """every input of this file as (name, (w, h), params, frames): what the switch test runs under both settings"""
    out = []
    for pi, params in enumerate(PARAMS):
        for w, h in SHAPES:
            frames = []
            for plane in "rb":
                frames += [isolated_pixels(w, h, params, plane)[0], noise_and_blobs(w, h, params, plane, 1000 * pi + w + h)]
                if w >= 256 and h >= 128:
                    frames += list(runs_in_a_trip(w, h, params, plane))
            out.append(("%dx%d_p%d" % (w, h, pi), (w, h), params, frames))
    return out


# ---------------------------------------------------------------------------------------------------------------------------

def _oracle(bev, params):
    """-> the oracle's R and Lab-b top-hat planes, the merged verdicts the formula gives on them, the oracle's mask"""
    from oracle import oracle as O
    kr, cr, kb, cb = params
    fp = O.filter_params(ksize_r=kr, C_r=cr, ksize_b=kb, C_b=cb)
    mask, planes = O.filter_lane_points(bev, fp, want_planes=True)
    return planes[2], planes[3], _bilateral_np(planes[2], kr, cr) | _bilateral_np(planes[3], kb, cb), mask


def _gpu_equals(shape, params, frames, oracles):
    from lane_tracker_amd import _native
    w, h = shape
    kr, cr, kb, cb = params
    n = len(frames)
    ctx = _ctx(w, h, capacity=n)
    try:
        ctx.upload_bev(np.stack(frames, 0))
        ctx.filter_run(n, _native.filter_params(ksize_r=kr, C_r=cr, ksize_b=kb, C_b=cb))
        assert ctx.last_threshold_form() == 2, "the matrix-core form did not take these parameters"
        merged = ctx.download_plane(_native.PLANE_MERGED, n)
        masks = ctx.download_masks(n)
    finally:
        ctx.close()
    for i, (_, _, expect, mask) in enumerate(oracles):
        diff = (merged[i] > 0) != expect
        assert not diff.any(), (shape, params, i, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        assert np.array_equal(masks[i], mask), (shape, params, i)
    return merged


def _other(plane):
    return "b" if plane == "r" else "r"


@pytest.mark.gpu
@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_isolated_pixels_just_above_c_pass_and_those_at_c_do_not(shape, params):
    """Single pixels of C + 1 in the corners of the image, of the tiles, of the 128-column strips and of the vertical segments, and
    single pixels of exactly C in other tiles: exactly the former appear in PLANE_MERGED.  One frame for each plane."""
    w, h = shape
    frames, oracles, hots = [], [], []
    for plane in "rb":
        C = _kc(params, plane)[1]
        bev, hot, cold = isolated_pixels(w, h, params, plane)
        o = _oracle(bev, params)
        th = o[0] if plane == "r" else o[1]
        want = np.zeros((h, w), np.uint8)
        for y, x in hot:
            want[y, x] = C + 1
        for y, x in cold:
            want[y, x] = C
        assert np.array_equal(th, want), (plane, np.argwhere(th != want)[:4].tolist())
        assert (o[1] if plane == "r" else o[0]).max() <= _kc(params, _other(plane))[1]       # the other plane passes nothing
        assert sorted(map(tuple, np.argwhere(o[2]).tolist())) == sorted(hot)
        assert not set((y // 32, x // 32) for y, x in hot) & set((y // 32, x // 32) for y, x in cold)
        frames.append(bev); oracles.append(o); hots.append(hot)
    merged = _gpu_equals(shape, params, frames, oracles)
    for i, hot in enumerate(hots):
        assert sorted(map(tuple, np.argwhere(merged[i] > 0).tolist())) == sorted(hot)


@pytest.mark.gpu
@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_dead_tiles_that_hold_nonzero_pixels_leave_their_live_neighbours_alone(shape, params):
    """Noise of amplitude <= C everywhere and a few bright blobs: few tiles are live, the dead ones are full of non-zero pixels that
    the sums of their live neighbours need.  For C = 0 a dead tile is an all-zero tile."""
    w, h = shape
    frames, oracles = [], []
    for pi, plane in enumerate("rb"):
        C = _kc(params, plane)[1]
        bev = noise_and_blobs(w, h, params, plane, 1000 * PARAMS.index(params) + w + h)
        o = _oracle(bev, params)
        th = o[0] if plane == "r" else o[1]
        live = _tile_max(th, 32, 32) > C
        share = float(live.mean())
        dead_px = np.repeat(np.repeat(~live, 32, 0), 32, 1)[:h, :w]
        nonzero = float((th[dead_px] > 0).mean())
        print(shape, params, plane, "live share %.3f, non-zero share of the pixels in dead tiles %.3f" % (share, nonzero))
        assert 0.05 <= share <= 0.6, share
        if C > 0:
            assert nonzero > 0.25, nonzero
        else:
            assert nonzero == 0.0
        assert o[2].any()
        frames.append(bev); oracles.append(o)
    _gpu_equals(shape, params, frames, oracles)


@pytest.mark.gpu
@pytest.mark.parametrize("params", PARAMS)
def test_runs_of_live_and_dead_tiles_inside_one_trip(params):
    """live, dead, dead, live and dead, live, dead, dead along one row group and down a 128-column strip, in either plane"""
    shape = w, h = 644, 130
    frames, oracles = [], []
    for plane in "rb":
        C = _kc(params, plane)[1]
        a, b = runs_in_a_trip(w, h, params, plane)
        oa, ob = _oracle(a, params), _oracle(b, params)
        tha, thb = (oa[0], ob[0]) if plane == "r" else (oa[1], ob[1])
        live_h = (_tile_max(tha, 32, 32) > C).astype(int)
        assert live_h[1, :8].tolist() == H_RUNS and live_h.sum() == sum(H_RUNS), live_h.tolist()
        live_v = (_tile_max(thb, 32, 128) > C).astype(int)
        assert live_v[:4, 0].tolist() == V_RUNS[0] and live_v[:4, 1].tolist() == V_RUNS[1] and live_v.sum() == 3, live_v.tolist()
        if C > 0:                                # the dead tiles of the runs are not empty
            assert all(_tile_max(tha, 32, 32)[1, t] == C for t in range(8) if not H_RUNS[t])
            assert all(_tile_max(thb, 32, 128)[t, s] == C for s in range(2) for t in range(4) if not V_RUNS[s][t])
        assert oa[2].any() and ob[2].any()
        frames += [a, b]; oracles += [oa, ob]
    _gpu_equals(shape, params, frames, oracles)


_CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
from lane_tracker_amd import _native
import test_gpu_threshold_skip as T
out = {}
for name, (w, h), (kr, cr, kb, cb), frames in T.all_inputs():
    n = len(frames)
    ctx = T._ctx(w, h, capacity=n)
    ctx.upload_bev(np.stack(frames, 0))
    ctx.filter_run(n, _native.filter_params(ksize_r=kr, C_r=cr, ksize_b=kb, C_b=cb))
    assert ctx.last_threshold_form() == 2, ctx.last_threshold_form()
    out["merged_" + name] = ctx.download_plane(_native.PLANE_MERGED, n)
    out["masks_" + name] = ctx.download_masks(n)
    ctx.close()
np.savez(sys.argv[1], **out)
print("ok")
'''


@pytest.mark.gpu
def test_skipping_and_not_skipping_write_identical_planes(tmp_path):
    """One child process per setting with the experiments library: PLANE_MERGED and the masks of every input of this file are
    byte-identical between "every block counts as live" (LT_THRESHOLD_SKIP=0) and the dead-tile test (unset), and between the
    horizontal tasks' words stored trip by trip (LT_THRESHOLD_STAGE=0, also the route of rows too wide for LDS) and collected in
    LDS (unset), in every combination."""
    if not os.path.exists(EXP_LIB):
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j8", "EXPERIMENTS=1"])
    code = _CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    files = {}
    for setting in ((None, None), ("0", None), (None, "0"), ("0", "0")):
        env = dict(os.environ, LANE_TRACKER_AMD_LIB=EXP_LIB)
        for name, value in zip(("LT_THRESHOLD_SKIP", "LT_THRESHOLD_STAGE"), setting):
            env.pop(name, None)
            if value is not None:
                env[name] = value
        env.pop("LT_THRESHOLD_MMA", None)
        files[setting] = str(tmp_path / ("skip_%s_stage_%s.npz" % setting))
        r = subprocess.run([sys.executable, "-c", code, files[setting]], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
    a = np.load(files[(None, None)])
    assert len(a.files) == 2 * len(PARAMS) * len(SHAPES) and any(a[name].any() for name in a.files)
    for setting in list(files)[1:]:
        b = np.load(files[setting])
        assert sorted(a.files) == sorted(b.files)
        for name in a.files:
            assert a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), (setting, name)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_generated_code_keeps_two_waves_per_simd_and_the_matrix_cores():
    """CPU only (hipcc cross-compiles): at most 256 VGPRs for each of the three window sizes, nothing spills, no scratch access before
    a kernel's end, and the i8 32x32x32 MFMA is still there."""
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                        "-I", CSRC, os.path.join(CSRC, "k_threshold_mma.hip"), "-o", "-"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = r.stdout
    assert "v_mfma_i32_32x32x32_i8" in text
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = [k for k in meta.split("\n  - ")[1:] if "k_bilateral_mma_hv" in k]
    assert len(kernels) == 3
    field = lambda k, name: int(k.split(name)[1].split()[0])
    for k in kernels:
        assert field(k, ".vgpr_count:") <= 256, k[-400:]
        assert field(k, ".vgpr_spill_count:") == 0 and field(k, ".private_segment_fixed_size:") == 0, k[-400:]
    for body in text.split(".end_amdhsa_kernel")[:-1]:
        for code in body.split("s_endpgm")[:-1]:
            assert "scratch_" not in code
