"""The 5x5 open on 64-pixel bit-plane words (csrc/k_threshold.hip), its three kernel forms, at every word layout, against the oracle.

`Chain::open()` (csrc/lt_mask_chain.cpp) picks a form by the frame count of the slice -- `last_open_form` tells which:
  2  k_or_open5_small<NP>   up to 4 frames: 8 output rows per workgroup through two LDS stages
  0  the separate kernels   5 .. 15 frames, and every plane that arrives merged (NP = 1) from 5 frames: k_or4_bits, k_erode5_bits,
                            k_dilate5_bits; with a u8 mask out (filter_lane_points) k_dilate5_mask is the dilate
  1  k_merge_open5<NP>      from 16 frames: a wave holds G = 64 / wpr frames side by side (lane = g * wpr + j), row neighbours are
                            whole-wave DPP shifts, rows are cut into bands with four halo rows on each side
NP, the merge arity: 4 = the bilateral walks' partial planes, 6 = those AND the greenery mask's two, 2 = the two planes of the box
walk ('neighborhood'), 1 = a plane that is merged already.

The shapes are the smallest at which each mechanism of the wave walk exists (SHAPES below); every shape runs at 4, 5, 15 and 16
frames, and at G + 1 frames where that makes a second group of one frame.  Everything goes through the context's own chain
(upload_bev, filter_run, download_plane(PLANE_MERGED), download_masks) on one stream, every frame is distinct, and every
comparison is for equality:
  (a) merged == the NumPy restatement of the thresholds on the oracle's planes,
  (b) mask   == oracle.morph_open(downloaded merged, 5),
  (c) mask   == oracle.filter_lane_points,
so that a threshold bug cannot hide an open bug, nor the other way round.  A case must not pass vacuously: judged from the oracle
alone, the expected masks of its slots are neither all empty nor all set, and the open changes the merged plane of some slot.

NP = 2 runs on designed bit patterns (`_pattern`): with ksize 63 and C 0 a pixel of the R plane is set exactly when it is 255 on a 0
background (unless its window is all but full), so a bird's-eye image coloured magenta where a pattern A is set yields A as the R
verdict plane; green pixels put a second pattern B into the Lab-b plane (black 128, magenta 67, green 211, yellow 223; C_b = 40).
The test asserts that encoding from the oracle's planes before it uses it.

The experiments build puts band boundaries of the wave walk everywhere (LT_OPEN5_BAND_ROWS = 1, 5, 9) and sends 4 and 16 frames
through the separate kernels (LT_OPEN5_SEPARATE=1 with LT_OPEN_SMALL=0: k_or4_bits at every wpr), one child process per setting
that computes every such case once; planes and masks must equal the unforced routes' byte for byte, and the oracle's."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_adaptive import adaptive_np
from test_gpu_walk import _bev, _bilateral_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lane_tracker_amd", "csrc")
EXP_LIB = os.path.join(ROOT, "lane_tracker_amd", "liblane_tracker_amd_exp.so")

# (w, h): wpr, G, what exists there first
SHAPES = [(8, 5),         # 1, 64: h = 5
          (64, 3),        # 1, 64: an exact word, h < 5
          (68, 24),       # 2, 32: 4 valid bits in the last word
          (128, 48),      # 2, 32: an exact word, two bands of 24
          (132, 70),      # 3, 21: lane 63 idle, two bands of 35
          (320, 49),      # 5, 12: 4 idle lanes, two bands of 25
          (1088, 26),     # 17, 3: the reference wpr
          (1348, 50),     # 22, 2: 20 idle lanes
          (2052, 24),     # 33, 1: 31 idle lanes
          (4096, 24)]     # 64, 1: every lane active, an exact word
ODD_SHAPE = (70, 30)      # w % 4 != 0: no walks, no box walk, the generic k_bits_to_u8
ARITIES = [4, 6, 2, 1]
BAND_ROWS = [1, 5, 9]


def _wpr(w):
    return (w + 63) // 64


def frame_counts(w):
    """4: the small form; 5, 15: the separate kernels; 16: the wave walk; G + 1 where that is a second group of one frame"""
    g1 = 64 // _wpr(w) + 1
    return [4, 5, 15, 16] + ([g1] if 16 < g1 <= 65 else [])


def expected_form(n, np_):
    return 2 if n <= 4 else 1 if n >= 16 and np_ > 1 else 0


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _tinted(rng, h, w):
    """shades of grey with a yellow / blue tint: Lab-b values around the greenery mask's threshold (test_gpu_walk.py)"""
    tint, grey = rng.integers(-40, 41, (h, w)), rng.integers(60, 200, (h, w))
    return np.clip(np.stack([grey + tint, grey + tint, grey - tint], -1), 0, 255).astype(np.uint8)


def _image(rng, h, w, kind):
    return _tinted(rng, h, w) if kind == 3 else _bev(rng, h, w, kind)


# Image kinds per slot (cycled), chosen per arity from the oracle's masks alone so that no case is vacuous: a random 8-bit image
# gives a few per cent of merged pixels and an empty mask at the small shapes, the block and the structure images keep a mask.
KINDS = {4: (2, 1, 0, 2), 6: (2, 1, 3, 2), 1: (2, 1, 0, 2)}

ELLIPSE = np.array([[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]], bool)   # the 17 taps


def _stamp(a, cy, cx, without=0):
    """the ellipse centred on (cy, cx); without = -1 / +1: its top / bottom tap missing (16 pixels, which the open removes)"""
    h, w = a.shape
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if ELLIPSE[dy + 2, dx + 2] and 0 <= cy + dy < h and 0 <= cx + dx < w and dy != 2 * without:
                a[cy + dy, cx + dx] = True


def _pattern(i, h, w):
    """-> (A, B) of slot i.  A holds what the open must keep (exact 17-pixel ellipses, 6-wide stripes, 5- and 3-wide edge stripes),
    what it must remove (4- and 2-wide stripes, 2-wide edge stripes, 2-row bars, specks), structures across every 64-column
    boundary, in rows 0 .. 2 and h - 3 .. h - 1, and on every row of h/2 - 6 .. h/2 + 6 the centre of an ellipse, of one without its
    top tap and of one without its bottom tap (spread over the slots where the width does not hold 39), so that a band boundary
    is covered wherever it falls: the outermost taps are what the fourth halo row of a band is for -- a walk with a halo of three
    rows takes the missing top tap for set and keeps a pixel of the 16-pixel shape.
    The edge stripes are 3 wide in the lower half of the image (and all of one below 8 rows): of a 5-wide stripe the erode keeps a
    column that does not need the border, and the dilate restores the rest, whatever came in across the edge; of a 3-wide one
    it keeps the edge column alone, and only because the border counts as set.
    The edge columns go by i % 3 -- 0: right edge set, left empty; 1: both empty; 2: both set -- so that slots i, i + 1 (lane
    neighbours of the wave walk: the last word of frame g beside the first word of frame g + 1) meet as (right set, left empty)
    and as (right empty, left set), the two cases in which a word leaking across the frame boundary changes the erode (a leaked
    0 where the border counts as set) or the dilate (a leaked eroded word where the border counts as clear); with two frames per
    wave (wpr 22) the pairs (0,1), (2,3), (4,5) still go through all three meetings.  A plain alternation of the two edge patterns
    would only ever meet as (set, set) and (empty, empty), which a leak does not change.
    B: ellipses and specks away from the borders (None where the image is too small to keep them there)."""
    rng = np.random.default_rng(1000003 * w + 1009 * h + i)
    a = np.zeros((h, w), bool)
    c, wide, edge = i % 3, (5 if w >= 16 else 3), (8 if w >= 32 else 3)
    # stripes across every word boundary: 6, 4, 2 wide by boundary and slot, not over the full height in every slot
    y0 = (i % 4) if h >= 8 else 0
    for k in range(1, _wpr(w)):
        half = (3, 2, 1)[(k + i) % 3]
        if 64 * k + half <= w - edge:
            a[y0:, 64 * k - half:64 * k + half] = True
    # an ellipse centred on every row around the middle
    rows = sorted({min(max(y, 0), h - 1) for y in range(h // 2 - 6, h // 2 + 7)})
    stamps = [(y, without) for without in (0, -1, 1) for y in rows]
    x0 = 12 if w >= 32 else w // 2
    per = max(1, min(len(stamps), (w - x0 - edge) // 8))
    turns = (len(stamps) + per - 1) // per
    for k, (y, without) in enumerate(stamps):
        if k // per == i % turns:
            _stamp(a, y, x0 + 8 * (k % per), without)
    # rows 0 .. 2 and h - 3 .. h - 1: a bar the open keeps at the top, a 2-row bar it removes at the bottom (and the other way round)
    if w >= 64:
        top, bot = (3, 2) if i % 2 == 0 else (2, 3)
        if h < 6:
            top, bot = min(top, 2), 1
        xa, xb = 20 + 3 * (i % 5), 44 + 2 * (i % 7)
        a[:top, xa:xa + 9] = True
        a[h - bot:, xb:xb + 9] = True
    # specks: single pixels and 2 x 2 blocks
    for _ in range(max(2, h * w // 400)):
        y, x = int(rng.integers(0, h)), int(rng.integers(edge, max(edge + 1, w - edge)))
        a[y:y + int(rng.integers(1, 3)), x:min(x + int(rng.integers(1, 3)), w - edge)] = True
    # the edge columns
    a[:, :edge] = False
    a[:, w - edge:] = False
    ysplit = h // 2 if h >= 8 else 0        # 5 wide above, 3 wide from there down
    if c in (0, 2):
        a[:ysplit, w - wide:] = True
        a[ysplit:, w - 3:] = True
    if c == 2:
        a[:ysplit, :wide] = True
        a[ysplit:, :3] = True
        if w < 16:
            a[:, wide:w - wide] = False     # (8 columns: both edges are most of the image, and a full window is not set)
    if c == 1 and h >= 6:
        a[:h // 3, w - 2:] = True           # the 2-wide stripe on the right edge; the rows below keep the edge empty
    b = None
    if h >= 24 and w >= 64:
        b = np.zeros((h, w), bool)
        for _ in range(max(2, w // 48)):
            _stamp(b, int(rng.integers(6, h - 6)), int(rng.integers(10, w - 10)))
        for _ in range(max(2, w // 32)):
            b[int(rng.integers(4, h - 4)), int(rng.integers(10, w - 10))] = True
    return a, b


def _colour(a, b):
    img = np.zeros(a.shape + (3,), np.uint8)
    img[a] = (255, 0, 255)                   # magenta: R 255, Lab-b 67
    if b is not None:
        img[b & ~a] = (0, 255, 0)            # green: R 0, Lab-b 211
        img[b & a] = (255, 255, 0)           # yellow: R 255, Lab-b 223
    return img


def filter_kw(np_, w, h):
    if np_ == 4:
        return dict(ksize_r=15, C_r=8, ksize_b=35, C_b=5)
    if np_ == 6:
        return dict(ksize_r=15, C_r=8, ksize_b=35, C_b=5, mask_noise=True)
    if np_ == 2:
        return dict(filter_type="neighborhood", ksize_r=63, C_r=0, ksize_b=63, C_b=40 if (h >= 24 and w >= 64) else 255)
    return dict(ksize_r=25, C_r=6, ksize_b=31, C_b=4)      # windows the walks do not have: the tile kernel merges (NP = 1)


def frames_of(w, h, np_, n=None):
    """the bird's-eye images of a case: a function of the shape and the arity alone (the children compute the same)"""
    n = n or max(frame_counts(w))
    if np_ == 2:
        return np.stack([_colour(*_pattern(i, h, w)) for i in range(n)], 0)
    rng = np.random.default_rng(7919 * w + 31 * h + np_)
    kinds = KINDS[np_]
    return np.stack([_image(rng, h, w, kinds[i % len(kinds)]) for i in range(n)], 0)


def _predict(planes, kw):
    """the merged plane from the oracle's planes (R, Lab-b, top-hat R, top-hat b), NumPy"""
    kr, cr, kb, cb = kw.get("ksize_r", 15), kw.get("C_r", 8), kw.get("ksize_b", 35), kw.get("C_b", 5)
    if kw.get("filter_type") == "neighborhood":
        m = adaptive_np(planes[0], kr, cr) | adaptive_np(planes[1], kb, cb)
    else:
        m = _bilateral_np(planes[2], kr, cr) | _bilateral_np(planes[3], kb, cb)
    if kw.get("mask_noise"):
        m &= ~(planes[1] >= kw.get("noise_thresh", 140)) | _bilateral_np(planes[1], kw.get("ksize_noise", 65), kw.get("C_noise", 10))
    return m


@functools.lru_cache(maxsize=None)
def oracle_case(w, h, np_, key=None):
    """-> (bev, want masks, predicted merged planes) of every slot, computed once and shared; key: another filter of ODD_SHAPE"""
    from oracle import oracle as O
    kw = dict(key) if key else filter_kw(np_, w, h)
    bev = frames_of(w, h, np_, 16 if key else None)
    want, merged = [], []
    for i in range(len(bev)):
        m, planes = O.filter_lane_points(bev[i], O.filter_params(**kw), want_planes=True)
        want.append(m)
        merged.append(_predict(planes, kw))
        if np_ == 2 and not key:                # the encoding itself: the verdict planes are the patterns
            a, b = _pattern(i, h, w)
            assert np.array_equal(adaptive_np(planes[0], kw["ksize_r"], kw["C_r"]), a), ((w, h), i, "pattern A does not encode")
            assert np.array_equal(adaptive_np(planes[1], kw["ksize_b"], kw["C_b"]), b if b is not None else np.zeros_like(a)), \
                ((w, h), i, "pattern B does not encode")
    for a in (bev, *want, *merged):
        a.setflags(write=False)
    return bev, want, merged


def assert_not_vacuous(want, merged, n, tag):
    """from the oracle alone: the masks of slots [0, n) are neither all empty nor all set, and the open changes some merged plane"""
    ones, total = sum(int((m > 0).sum()) for m in want[:n]), sum(m.size for m in want[:n])
    assert 0 < ones < total, (tag, ones, total)
    assert any(not np.array_equal(want[i] > 0, merged[i]) for i in range(n)), (tag, "the open changes nothing")


def _context(w, h, capacity):
    from lane_tracker_amd import _native, calib
    cal = calib.reference_calibration()
    ctx = _native.Context(cal["img_size"], (w, h), cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], device=0, capacity=capacity)
    ctx.set_walk_min_frames(0)                             # these small calls would take the tile kernel by default
    return ctx


def assert_routes(ctx, np_, n, tag):
    assert ctx.last_open_form() == expected_form(n, np_), (tag, ctx.last_open_form())
    if np_ in (4, 6):
        assert ctx.last_threshold_path() == 1, (tag, "the walking kernels did not take these parameters")
        assert ctx.last_threshold_form() in (1, 2), tag
    elif np_ == 2:
        assert ctx.last_adaptive_path() == 1, (tag, "the box walk did not take these parameters")
    else:
        assert ctx.last_threshold_path() == 0, (tag, "NP = 1 is the tile kernel's merged plane")


def check_slots(got, merged_gpu, want, merged, tag):
    """(a), (b), (c) on every slot"""
    from oracle import oracle as O
    for i in range(len(got)):
        t = tag + (i,)
        diff = (merged_gpu[i] > 0) != merged[i]
        assert not diff.any(), (t, "merged plane", int(diff.sum()), np.argwhere(diff)[:4].tolist())
        assert np.array_equal(got[i], O.morph_open(np.ascontiguousarray(merged_gpu[i]), 5)), (t, "mask != open(downloaded merged)")
        diff = got[i] != want[i]
        assert not diff.any(), (t, "mask", int(diff.sum()), np.argwhere(diff)[:4].tolist())


# ---- the release routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("np_", ARITIES, ids=lambda v: "np%d" % v)
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_open_forms_match_the_oracle_at_every_word_layout(size, np_):
    from lane_tracker_amd import _native
    w, h = size
    kw = filter_kw(np_, w, h)
    bev, want, merged = oracle_case(w, h, np_)
    counts = frame_counts(w)
    ctx = _context(w, h, max(counts))
    try:
        assert ctx.last_open_form() == -1
        for n in counts:
            tag = (size, np_, n)
            assert_not_vacuous(want, merged, n, tag)
            ctx.upload_bev(bev[:n])
            ctx.filter_run(n, _native.filter_params(**kw))
            assert_routes(ctx, np_, n, tag)
            check_slots(ctx.download_masks(n), ctx.download_plane(_native.PLANE_MERGED, n), want, merged, tag)
    finally:
        ctx.close()


ODD_FILTERS = [dict(), dict(mask_noise=True), dict(filter_type="neighborhood", ksize_r=15, C_r=5, ksize_b=35, C_b=5)]


@pytest.mark.gpu
@pytest.mark.parametrize("kw", ODD_FILTERS, ids=["bilateral", "mask_noise", "neighborhood"])
def test_a_width_that_is_no_multiple_of_four_reaches_the_open_merged(kw):
    """(70, 30): no walks and no box walk, so every filter leaves one merged plane (NP = 1): the small form at 4 frames, the separate
    kernels from 5 -- at 16 too, as the route table says -- and the generic k_bits_to_u8 behind them."""
    from lane_tracker_amd import _native
    w, h = ODD_SHAPE
    np_ = 6 if kw.get("mask_noise") else 4          # (the image kinds of that arity; the merge arity is 1 for all three)
    bev, want, merged = oracle_case(w, h, np_, tuple(sorted(kw.items())))
    ctx = _context(w, h, 16)
    try:
        for n in (4, 5, 15, 16):
            tag = (ODD_SHAPE, tuple(kw), n)
            assert_not_vacuous(want, merged, n, tag)
            ctx.upload_bev(bev[:n])
            ctx.filter_run(n, _native.filter_params(**kw))
            assert ctx.last_open_form() == expected_form(n, 1), (tag, ctx.last_open_form())
            if kw.get("filter_type") == "neighborhood":
                assert ctx.last_adaptive_path() == 0, tag
            else:
                assert ctx.last_threshold_path() == 0, tag
            check_slots(ctx.download_masks(n), ctx.download_plane(_native.PLANE_MERGED, n), want, merged, tag)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("np_", [4, 2], ids=lambda v: "np%d" % v)
def test_a_range_of_slots_leaves_the_slots_outside_it_alone(np_):
    """first = 3 in a context of 24 slots: 16 frames through the wave walk at slots 3 .. 18 (then 4 and 5 frames), whose groups and
    idle lanes are counted from the range's first slot; the slots before and behind keep the masks of an earlier run."""
    from lane_tracker_amd import _native
    w, h = 132, 70
    kw = filter_kw(np_, w, h)
    bev, want, merged = oracle_case(w, h, np_)
    ctx = _context(w, h, 24)
    try:
        order = np.arange(24)[::-1] % len(bev)             # the earlier run: other frames in every slot
        ctx.upload_bev(bev[order])
        ctx.filter_run(24, _native.filter_params(**kw))
        before = ctx.download_masks(24)
        for k in range(24):
            assert np.array_equal(before[k], want[order[k]]), k
        for n in (16, 4, 5):
            ctx.upload_bev(bev[:n], first=3)
            ctx.filter_run(n, _native.filter_params(**kw), first=3)
            assert_routes(ctx, np_, n, (np_, n))
            check_slots(ctx.download_masks(n, first=3), ctx.download_plane(_native.PLANE_MERGED, n, first=3), want, merged, (np_, n))
            after = ctx.download_masks(24)
            for k in list(range(3)) + list(range(19, 24)):
                assert np.array_equal(after[k], before[k]), (n, k, "a slot outside the range changed")
    finally:
        ctx.close()


# ---- the u8 route: lt_filter_lane_points, k_erode5_bits + k_dilate5_mask -------------------------------------------------------------
U8_SHAPES = [(3, 64), (5, 8), (17, 66), (33, 4096), (16, 4092), (40, 200)]      # (h, w); h = 40 crosses a DR = 16 block of the dilate
U8_FILTERS = [dict(), dict(mask_noise=True), dict(filter_type="neighborhood", ksize_r=63, C_r=0, ksize_b=63, C_b=255)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", U8_SHAPES, ids=lambda s: "%dx%d" % s)
def test_u8_mask_route_matches_the_oracle(size):
    from lane_tracker_amd import _native
    from oracle import oracle as O
    h, w = size
    ctx = _context(8, 5, 1)
    rng = np.random.default_rng(977 * w + h)
    try:
        for kw in U8_FILTERS:
            nonempty = changed = False
            for kind in ((0, 1) if kw.get("filter_type") else (2, 1, 3 if kw.get("mask_noise") else 0)):
                img = _colour(_pattern(kind, h, w)[0], None) if kw.get("filter_type") else _image(rng, h, w, kind)
                want, planes = O.filter_lane_points(img, O.filter_params(**kw), want_planes=True)
                got = ctx.filter_lane_points(img, _native.filter_params(**kw))
                diff = got != want
                assert not diff.any(), (size, kw, kind, int(diff.sum()), np.argwhere(diff)[:4].tolist())
                nonempty |= bool(want.any()) and not bool(want.all())
                changed |= not np.array_equal(want > 0, _predict(planes, kw))
            assert nonempty and changed, (size, kw, "a vacuous case: choose other images")
    finally:
        ctx.close()


# ---- the experiments build -------------------------------------------------------------------------------------------------------------
SETTINGS = {"release": {}, "separate": {"LT_OPEN5_SEPARATE": "1", "LT_OPEN_SMALL": "0"},
            **{"band%d" % r: {"LT_OPEN5_BAND_ROWS": str(r)} for r in BAND_ROWS}}


def exp_cases(setting):
    """(w, h, np, n) a setting runs; "release" runs them all without a switch"""
    sep = [(w, h, np_, n) for (w, h) in SHAPES for np_ in (2, 4, 6) for n in (4, 16)]
    band = [(w, h, np_, 16) for (w, h) in SHAPES if h >= 24 for np_ in (2, 4, 6)]
    return sep if setting == "separate" else band if setting.startswith("band") else sorted(set(sep + band))


def _child(setting, path):
    sys.path.insert(0, ROOT)
    from lane_tracker_amd import _native
    out = {}
    for (w, h) in SHAPES:
        mine = [c for c in exp_cases(setting) if c[:2] == (w, h)]
        if not mine:
            continue
        ctx = _context(w, h, 16)
        try:
            for (_, _, np_, n) in mine:
                ctx.upload_bev(frames_of(w, h, np_, n))
                ctx.filter_run(n, _native.filter_params(**filter_kw(np_, w, h)))
                name = "%d_%d_%d_%d" % (w, h, np_, n)
                out["form_" + name] = np.array([ctx.last_open_form(), ctx.last_threshold_path(), ctx.last_adaptive_path()])
                out["merged_" + name] = np.packbits(ctx.download_plane(_native.PLANE_MERGED, n) > 0)
                masks = ctx.download_masks(n)
                assert np.isin(masks, (0, 255)).all(), name
                out["masks_" + name] = np.packbits(masks > 0)
        finally:
            ctx.close()
    np.savez(path, **out)
    print("ok")


@pytest.fixture(scope="module")
def exp_runs(tmp_path_factory):
    """one child process per setting, each with the experiments library: -> {setting: its planes}"""
    if not os.path.exists(EXP_LIB):
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j8", "EXPERIMENTS=1"])
    d = tmp_path_factory.mktemp("open_stage")
    runs = {}
    for setting, switches in SETTINGS.items():
        env = dict(os.environ, LANE_TRACKER_AMD_LIB=EXP_LIB)
        for name in ("LT_OPEN5_SEPARATE", "LT_OPEN_SMALL", "LT_OPEN5_BAND_ROWS"):
            env.pop(name, None)
        env.update(switches)
        path = str(d / (setting + ".npz"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", setting, path], cwd=ROOT, capture_output=True, text=True,
                           env=env, timeout=300)
        assert r.returncode == 0 and "ok" in r.stdout, (setting, r.stdout[-1000:] + r.stderr[-2000:])
        runs[setting] = dict(np.load(path))
    return runs


@pytest.mark.gpu
@pytest.mark.parametrize("setting", [s for s in SETTINGS if s != "release"])
def test_forced_open_routes_write_the_planes_of_the_release_routes(exp_runs, setting):
    run, release = exp_runs[setting], exp_runs["release"]
    cases = exp_cases(setting)
    assert len(run) == 3 * len(cases)
    for (w, h, np_, n) in cases:
        name = "%d_%d_%d_%d" % (w, h, np_, n)
        form, tpath, apath = (int(v) for v in run["form_" + name])
        assert form == (0 if setting == "separate" else 1), (setting, name, form)
        assert int(release["form_" + name][0]) == expected_form(n, np_), name
        assert (apath if np_ == 2 else tpath) == 1, (setting, name)
        for what in ("merged_", "masks_"):
            assert run[what + name].tobytes() == release[what + name].tobytes(), (setting, what + name)
        _, want, merged = oracle_case(w, h, np_)
        assert_not_vacuous(want, merged, n, name)
        assert np.array_equal(run["merged_" + name], np.packbits(np.stack(merged[:n], 0))), (setting, name, "merged plane != the prediction")
        assert np.array_equal(run["masks_" + name], np.packbits(np.stack(want[:n], 0) > 0)), (setting, name, "masks != the oracle's")


if __name__ == "__main__" and "--child" in sys.argv:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    _child(sys.argv[sys.argv.index("--child") + 1], sys.argv[sys.argv.index("--child") + 2])
