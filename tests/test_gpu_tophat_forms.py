"""Every walk form of csrc/k_tophat.hip against the definition (tests/morph_reference.py) on designed planes, for equality.

One case = one geometry (k, h, forced bands, w, frames) run through the test hook lt_morph_planes, which makes ONE launcher call on
planes given by value in buffers of its own and says which kernel family ran.  A case names the report it expects: a form that
silently stops being chosen fails.  What is compared: the eroded plane, the dilated plane (the batch instantiations <DIL, !TH> no
product call reaches), the top-hat with a dense and with a 64-byte padded destination, the top-hat's eroded intermediate, and for k = 55
the top-hat that copies its minuend.  Guards: the destination, the intermediate and the copy plane are n + 2 planes of 0xA5 and the
work goes to planes 1 .. n -- planes 0 and n + 1 and the pitch padding must come back untouched.

Planes of a case (frames of one call all differ, so swapped frames of a PAIR wave show): uniform noise; noise with 2 % zeros and 2 %
255s; constant 0 and 255; the ramps x, y, x + y, 255 - (x + y) (mod 256: every adjacent pair of the 256 values meets under min and max
-- the walks order them as f16 bit patterns, denormals included); and delta planes -- single zeros on 255 for the erosion, single 255s
on 0 for the dilation, both kinds for the top-hats -- with a delta at every combination of the rows {0, h - 1} and b * band_rows + d,
d in {-R - 1, -R, -1, 0, 1, R - 1, R}, for every band boundary b (the first and the last one when there are more than four bands), and
the columns {0, 63, 64, 127, 128, w - 1}; deltas of one plane are more than K apart.

Which pairs run (not the cross product).  Split-band form and its refusals: every (h, bands) of SPLIT at the widths 64, 132 and 196
with 3 frames; the three-band geometry also at every other WIDE width, and with 4 and 5 frames at 64, 132, 196.  Halo form
(k_morph_runs2), 3 frames: forced bands of 1, 2, 3, R and 2R + 1 rows, five bands where four would split, and the heights 1, 2, 7, R,
R + 1 under the launcher's own rule, each at 64, 132, 196; the three-row-band geometry also at every other width, the narrow ones
included, and with 4 and 5 frames.  k_morph_one (one and two frames): every WIDE width at h = 61 under the launcher's rule (the test
repeats `one_frame_bands` from the CU count) and with two forced bands; the narrow widths take k_morph_runs2's narrow form there.
k_morph_one_pair: the top-hat at (150, 260), (61, 132), (9, 64), (300, 516) with one and two frames, the launcher's bands and forced
ones, dense and padded, plane pairs from different families (a quarter of the planes at the largest size); its erosion and its
dilation alone at (61, 132) and (9, 64); width 130 is refused.  The experiments build's Q = 8 forms and the one-row kernel run once each in child processes at (61, 132), which also
carry the two chain cases: a slot range that does not start at 0, and two streams."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import morph_reference as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP_LIB = os.path.join(ROOT, "lane_tracker_amd", "liblane_tracker_amd_exp.so")

RADIUS = {29: 14, 55: 27}
ZONE = {29: 28, 55: 56}                                # rows of a boundary zone of the split-band form
WIDE_WIDTHS = [4, 64, 68, 128, 132, 192, 196, 260]
NARROW_WIDTHS = [1, 3, 67, 130]
PAIR_WIDTHS = {4, 64, 132, 192, 260}                   # the last strip is at most 64 columns wide: a PAIR strip
MAIN_WIDTHS = [64, 132, 196]
GUARD = 0xA5

# (h, bands) -> the family that must run, with a zone scratch at hand (3 frames and more)
SPLIT = {29: [((56, 1), "split"), ((56, 2), "split"), ((57, 2), "split"), ((86, 3), "split"), ((112, 4), "split"), ((85, 3), "runs2")],
         55: [((56, 1), "split"), ((112, 2), "split"), ((113, 2), "split"), ((170, 3), "split"), ((224, 4), "split"), ((111, 2), "runs2")]}
SPLIT_ALL_WIDTHS = {29: (86, 3), 55: (170, 3)}         # the middle band has a zone on both sides


def _halo(k):
    """(h, bands) of the halo cases: band_rows of 1, 2, 3, R; five bands where four split; bands 0 = the launcher's rule.  (band_rows
    of 2R + 1 with a last band the split form refuses are SPLIT's (85, 3) and the (109, 2) added here for 55x55.)"""
    r = RADIUS[k]
    out = [(20, 20), (20, 10), (21, 7), (3 * r, 3), (4 * ZONE[k], 5)] + [(h, 0) for h in (1, 2, 7, r, r + 1)]
    return out + ([(109, 2)] if k == 55 else [])


HALO_ALL_WIDTHS = (21, 7)


def _cases():
    cases = []

    def add(kind, k, h, bands, w, n, family):
        cases.append(pytest.param(kind, k, h, bands, w, n, family, id="%s-k%d-h%d-b%d-w%d-n%d" % (kind, k, h, bands, w, n)))
    for k in (29, 55):
        for (h, bands), family in SPLIT[k]:
            for w in MAIN_WIDTHS:
                add("split", k, h, bands, w, 3, family)
        h, bands = SPLIT_ALL_WIDTHS[k]
        for w in WIDE_WIDTHS:
            if w not in MAIN_WIDTHS:
                add("split", k, h, bands, w, 3, "split")
        for n in (4, 5):
            for w in MAIN_WIDTHS:
                add("split", k, h, bands, w, n, "split")
        for h, bands in _halo(k):
            for w in MAIN_WIDTHS:
                add("halo", k, h, bands, w, 3, "runs2")
        h, bands = HALO_ALL_WIDTHS
        for w in WIDE_WIDTHS + NARROW_WIDTHS:
            if w not in MAIN_WIDTHS:
                add("halo", k, h, bands, w, 3, "runs2")
        for n in (4, 5):
            for w in MAIN_WIDTHS:
                add("halo", k, h, bands, w, n, "runs2")
        for n in (1, 2):
            for w in WIDE_WIDTHS:
                add("one", k, 61, 0, w, n, "one")
                add("one", k, 61, 2, w, n, "one")
            for w in NARROW_WIDTHS:
                add("one", k, 61, 0, w, n, "runs2")
    return cases


# ---- planes -------------------------------------------------------------------------------------------------------------------
def common_planes(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    sparse = rng.integers(0, 256, (h, w), dtype=np.uint8)
    u = rng.random((h, w))
    sparse[u < 0.02] = 0
    sparse[u > 0.98] = 255
    ramps = [x & 255, y & 255, (x + y) & 255, 255 - ((x + y) & 255)]
    return [rng.integers(0, 256, (h, w), dtype=np.uint8), sparse, np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)] + \
        [r.astype(np.uint8) for r in ramps]


def delta_positions(k, h, w, band_rows, nbands):
    r = RADIUS[k]
    bounds = list(range(1, nbands))
    if nbands > 4:
        bounds = [1, nbands - 1]
    rows = {0, h - 1}
    for b in bounds:
        rows |= {b * band_rows + d for d in (-r - 1, -r, -1, 0, 1, r - 1, r)}
    cols = {0, 63, 64, 127, 128, w - 1}
    return [(y, x) for y in sorted(rows) if 0 <= y < h for x in sorted(cols) if 0 <= x < w]


def delta_planes(k, h, w, band_rows, nbands, background, value):
    """As few planes as keep the deltas of one plane more than K apart (Chebyshev), filled first fit."""
    groups = []
    for (y, x) in delta_positions(k, h, w, band_rows, nbands):
        for g in groups:
            if all(max(abs(y - yy), abs(x - xx)) > k for (yy, xx) in g):
                g.append((y, x))
                break
        else:
            groups.append([(y, x)])
    out = []
    for g in groups:
        a = np.full((h, w), background, np.uint8)
        for (y, x) in g:
            a[y, x] = value
        out.append(a)
    return out


def distinct(planes, n, seed):
    """The planes without repeats (a 1 x 1 ramp is a constant), at least n of them."""
    seen, out = set(), []
    for a in planes:
        key = a.tobytes()
        if key not in seen:
            seen.add(key)
            out.append(a)
    rng = np.random.default_rng(seed)
    while len(out) < n:
        a = rng.integers(0, 256, planes[0].shape, dtype=np.uint8)
        if a.tobytes() not in seen:
            seen.add(a.tobytes())
            out.append(a)
    return out


def calls_of(planes, n):
    """The planes in calls of n frames; a short last call is filled up from the front of the list (still n different planes)."""
    out = []
    for i in range(0, len(planes), n):
        chunk = planes[i:i + n]
        j = 0
        while len(chunk) < n:
            chunk.append(planes[j])
            j += 1
        out.append(np.stack(chunk, 0))
    return out


_REF = {}


def reference(a, k, op):
    """erode / dilate / tophat of one plane by the definition, computed once per (plane, k) in this module."""
    key = (k, op, a.shape, hashlib.blake2b(a.tobytes(), digest_size=16).digest())
    if key not in _REF:
        if op == "tophat":
            er = reference(a, k, "erode")
            opened = reference(er, k, "dilate")
            assert (opened <= a).all()
            _REF[key] = a - opened
        else:
            _REF[key] = MR.erode(a, k) if op == "erode" else MR.dilate(a, k)
        _REF[key].setflags(write=False)
    return _REF[key]


# ---- one hook call against the definition -----------------------------------------------------------------------------------------
def check_guards(name, buf, n, w, what):
    """buf: (n + 2, h, pitch), the whole allocation."""
    assert (buf[0] == GUARD).all(), "%s: a store into the plane in front of %s" % (name, what)
    assert (buf[n + 1] == GUARD).all(), "%s: a store into the plane behind %s (frame n of a PAIR wave?)" % (name, what)
    assert (buf[:, :, w:] == GUARD).all(), "%s: a store into the pitch padding of %s" % (name, what)


def first_diff(got, want):
    idx = np.argwhere(got != want)
    f, y, x = idx[0]
    return "%d pixels differ, first at frame %d row %d column %d: got %d, want %d" % (len(idx), f, y, x, got[f, y, x], want[f, y, x])


def check_call(ctx, frames, k, op, bands, padded, expect, name):
    """frames: (n, h, w).  expect: the report's fields that must hold."""
    n, h, w = frames.shape
    r = ctx.morph_planes(frames, k, op, bands=bands, padded=padded)
    rep = r["report"]
    name = "%s %s%s" % (name, op, " padded" if padded else "")
    assert r["launched"], name + ": the launcher refused"
    for key, v in expect.items():
        assert rep[key] == v, "%s: report %s = %r, expected %r (%r)" % (name, key, rep[key], v, rep)
    assert rep["nbands"] == -(-h // rep["band_rows"]), (name, rep)
    base = "tophat" if op == "tophat_copy" else op
    want = np.stack([reference(f, k, base) for f in frames], 0)
    check_guards(name, r["dst"], n, w, "the destination")
    got = r["dst"][1:n + 1, :, :w]
    assert np.array_equal(got, want), "%s: %s" % (name, first_diff(got, want))
    if base == "tophat":
        check_guards(name, r["mid"], n, w, "the intermediate")
        want_mid = np.stack([reference(f, k, "erode") for f in frames], 0)
        assert np.array_equal(r["mid"][1:n + 1], want_mid), "%s, eroded intermediate: %s" % (name, first_diff(r["mid"][1:n + 1], want_mid))
    if op == "tophat_copy":
        check_guards(name, r["copy"], n, w, "the copy plane")
        assert np.array_equal(r["copy"][1:n + 1, :, :w], frames), "%s, minuend copy: %s" % (name, first_diff(r["copy"][1:n + 1, :, :w], frames))
    else:
        assert (r["copy"] == GUARD).all(), name + ": a store into the copy plane of a launch that has none"
    return rep


def one_frame_cut(h, w, n, target, bands):
    """k_morph_one's bands (one_frame_bands): about `target` workgroups, bands even and at least 8 rows long."""
    nstrips = (w + 127) // 128
    nb = bands if bands > 0 else max(1, target // max(1, n * nstrips))
    rows = max(-(-h // nb), 8)
    rows = (rows + 1) & ~1
    return rows, -(-h // rows)


def run_geometry(ctx, kind, k, h, bands, w, n, family, cus):
    """Every operation of one geometry.  Returns the number of hook calls."""
    wide = w % 4 == 0
    expect = dict(family=family, wide=int(wide))
    if family == "one":
        rows, nbands = one_frame_cut(h, w, n, 2 * cus, bands)
        expect.update(band_rows=rows, nbands=nbands, pair_strip=0, q=4)
    else:
        expect.update(pair_strip=int(wide and w in PAIR_WIDTHS), q=0)
        if bands > 0:
            rows = -(-h // bands)
            expect.update(band_rows=rows, nbands=-(-h // rows))
        else:   # the launcher's rule (it depends on the device): ask it, on zeros, and design the deltas for what it says
            probe = ctx.morph_planes(np.zeros((n, h, w), np.uint8), k, "erode")["report"]
            rows = probe["band_rows"]
            expect.update(band_rows=rows, nbands=probe["nbands"])
    nbands = expect["nbands"]
    seed = 100000 * k + 100 * h + w
    common = common_planes(h, w, seed)
    zeros_on_255 = delta_planes(k, h, w, rows, nbands, 255, 0)
    ones_on_0 = delta_planes(k, h, w, rows, nbands, 0, 255)
    name = "%s k=%d h=%d bands=%d w=%d n=%d" % (kind, k, h, bands, w, n)
    calls = 0
    plan = [("erode", False, common + zeros_on_255), ("dilate", False, common + ones_on_0),
            ("tophat", False, common + zeros_on_255 + ones_on_0), ("tophat", True, common + zeros_on_255 + ones_on_0)]
    if k == 55 and wide:   # the minuend copy rides on the dword store of the WIDE 55x55 top-hat; narrow rows have none (refusal below)
        plan.append(("tophat_copy", True, common + zeros_on_255 + ones_on_0))
    for op, padded, planes in plan:
        exp = dict(expect)
        if op == "tophat_copy" and family == "one":   # k_morph_one has no copy form: the batch kernel takes the call, without a zone
            exp = dict(family="runs2", wide=1, pair_strip=int(w in PAIR_WIDTHS), q=0)
            if bands > 0:
                exp.update(band_rows=-(-h // bands), nbands=-(-h // -(-h // bands)))
        for frames in calls_of(distinct(planes, n, seed), n):
            check_call(ctx, frames, k, op, bands, padded, exp, name)
            calls += 1
    if k == 55 and not wide:
        r = ctx.morph_planes(np.stack(distinct(common, n, seed)[:n], 0), k, "tophat_copy", bands=bands, padded=True)
        assert not r["launched"] and r["report"]["family"] == "none", name + ": a minuend copy on narrow rows must be refused"
        assert (r["dst"] == GUARD).all() and (r["copy"] == GUARD).all()
    return calls


@pytest.fixture(scope="module")
def hook():
    from lane_tracker_amd import _native, calib
    cal = calib.reference_calibration()
    ctx = _native.Context(cal["img_size"], (64, 64), cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], device=0, capacity=1)
    try:
        yield ctx, int(ctx.info().cu_count)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,k,h,bands,w,n,family", _cases())
def test_form_equals_the_definition(hook, kind, k, h, bands, w, n, family):
    ctx, cus = hook
    calls = run_geometry(ctx, kind, k, h, bands, w, n, family, cus)
    print(kind, k, h, bands, w, n, family, "hook calls:", calls)


def test_the_split_cases_are_the_predicates_edge():
    """The table above against lt_tophat_split_form, and against the rule it states: WIDE, at most four bands, every band a zone long.
    (Host code only: runs without a GPU.)"""
    from lane_tracker_amd import _native
    lib = _native.load()
    for k in (29, 55):
        for (h, bands), family in SPLIT[k]:
            rows = -(-h // bands)
            nb = -(-h // rows)
            rule = nb <= 4 and rows >= ZONE[k] and h - (nb - 1) * rows >= ZONE[k]
            assert rule == (family == "split"), (k, h, bands)
            for w in WIDE_WIDTHS:
                assert bool(lib.lt_tophat_split_form(h, w, k, bands)) == rule, (k, h, bands, w)
        for h, bands in _halo(k):
            if bands:
                assert not lib.lt_tophat_split_form(h, 132, k, bands), (k, h, bands)


# ---- k_morph_one_pair ---------------------------------------------------------------------------------------------------------------
PAIR_SIZES = [(150, 260), (61, 132), (9, 64), (300, 516)]


def pair_planes(h, w, n, bands, cus, variant):
    """(2, n, h, w): the 55x55 chain's planes and the 29x29 chain's, from different families, with deltas at each chain's own bands."""
    rows55, nb55 = one_frame_cut(h, w, n, cus, bands)
    rows29, nb29 = one_frame_cut(h, w, n, cus + cus // 2, bands)
    common = common_planes(h, w, 7 * h + w + variant)
    d55 = delta_planes(55, h, w, rows55, nb55, 255, 0) + delta_planes(55, h, w, rows55, nb55, 0, 255)
    d29 = delta_planes(29, h, w, rows29, nb29, 255, 0) + delta_planes(29, h, w, rows29, nb29, 0, 255)
    sets = []
    for i in range(max(len(d55), len(d29), len(common))):
        p55 = [common[(i + j) % len(common)] if j % 2 == variant % 2 else d55[(i + j) % len(d55)] for j in range(n)]
        p29 = [d29[(i + j) % len(d29)] if j % 2 == variant % 2 else common[(i + j + 3) % len(common)] for j in range(n)]
        sets.append(np.stack([np.stack(p55, 0), np.stack(p29, 0)], 0))
    return sets, dict(family="one_pair", wide=1, q=4, band_rows=rows55, nbands=nb55, band_rows29=rows29, nbands29=nb29, pair_strip=0)


@pytest.mark.gpu
@pytest.mark.parametrize("bands", [0, 2])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("size", PAIR_SIZES)
def test_one_pair_equals_the_definition(hook, size, n, bands):
    ctx, cus = hook
    h, w = size
    if bands and size == (300, 516):
        bands = 3
    calls = 0
    for variant in (0, 1):
        sets, expect = pair_planes(h, w, n, bands, cus, variant)
        if size == (300, 516):
            sets = sets[::4]            # a quarter of the planes at the largest size (the definition's time)
        for planes in sets:
            check_pair_call(ctx, planes, bands, bool(variant), expect, "one_pair h=%d w=%d n=%d bands=%d" % (h, w, n, bands))
            calls += 1
    print(size, n, bands, "hook calls:", calls)


def check_pair_call(ctx, planes, bands, padded, expect, name, op="tophat"):
    _, n, h, w = planes.shape
    r = ctx.morph_planes(planes, 55, op, bands=bands, padded=padded, route=1)
    assert r["launched"], name + ": refused"
    for key, v in expect.items():
        assert r["report"][key] == v, "%s: report %s = %r, expected %r (%r)" % (name, key, r["report"][key], v, r["report"])
    assert (r["copy"] == GUARD).all()
    for c, k in enumerate((55, 29)):
        tag = "%s %s, %dx%d chain%s" % (name, op, k, k, " padded" if padded else "")
        check_guards(tag, r["dst"][c], n, w, "the destination")
        want = np.stack([reference(f, k, op) for f in planes[c]], 0)
        got = r["dst"][c][1:n + 1, :, :w]
        if op == "tophat":
            check_guards(tag, r["mid"][c], n, w, "the intermediate")
            want_mid = np.stack([reference(f, k, "erode") for f in planes[c]], 0)
            got_mid = r["mid"][c][1:n + 1]
            assert np.array_equal(got_mid, want_mid), "%s, eroded plane: %s" % (tag, first_diff(got_mid, want_mid))
        assert np.array_equal(got, want), "%s: %s" % (tag, first_diff(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["erode", "dilate"])
@pytest.mark.parametrize("n", [1, 2])
def test_one_pair_erode_and_dilate_alone(hook, n, op):
    """The pair launch's dilation without a minuend has no product caller (the chain always passes one); its erosion is the
    top-hat's first launch, here into a padded destination of its own."""
    ctx, cus = hook
    for (h, w) in [(61, 132), (9, 64)]:
        for variant in (0, 1):
            sets, expect = pair_planes(h, w, n, 0, cus, variant)
            for planes in sets:
                check_pair_call(ctx, planes, 0, bool(variant), expect, "one_pair h=%d w=%d n=%d" % (h, w, n), op=op)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2])
def test_one_pair_refuses_rows_that_are_not_dwords(hook, n):
    ctx, _ = hook
    planes = np.random.default_rng(130 + n).integers(0, 256, (2, n, 61, 130), dtype=np.uint8)
    for op in ("erode", "dilate", "tophat"):
        r = ctx.morph_planes(planes, 55, op, route=1)
        assert not r["launched"] and r["report"]["family"] == "none"
        assert (r["dst"] == GUARD).all() and (r["copy"] == GUARD).all() and (r["mid"] is None or (r["mid"] == GUARD).all())


# ---- the experiments build's forms and the chain cases, in child processes -------------------------------------------------------
EXP_SIZE = (61, 132)                                     # a full strip plus a four-column PAIR strip
CHAIN_SIZE = (236, 188)
CHAIN_BANDS = 4


def _exp_hook_cases(ctx, cases):
    """cases: (label, frames, route, expected family, expected q) at EXP_SIZE -> {label: "ok" or what failed}"""
    h, w = EXP_SIZE
    out = {}
    for label, n, route, expect_family, q in cases:
        common = common_planes(h, w, 61132 + n)
        try:
            if route == 0:
                rows = one_frame_cut(h, w, n, 2 * int(ctx.info().cu_count), 0) if expect_family == "one" else None
                d = delta_planes(29, h, w, rows[0], rows[1], 255, 0) + delta_planes(29, h, w, rows[0], rows[1], 0, 255) if rows else []
                for k in (29, 55):
                    for op in ("erode", "dilate", "tophat"):
                        for frames in calls_of(distinct(common + d, n, 1), n):
                            exp = dict(family=expect_family, q=q)
                            check_call(ctx, frames, k, op, 0, op == "tophat", exp, label)
            else:
                planes = np.stack([np.stack(common[:n], 0), np.stack(common[4:4 + n], 0)], 0)
                r = ctx.morph_planes(planes, 55, "tophat", route=1)
                assert r["launched"] and r["report"]["family"] == expect_family and r["report"]["q"] == q, r["report"]
                for c, k in enumerate((55, 29)):
                    check_guards(label, r["dst"][c], n, w, "the destination")
                    check_guards(label, r["mid"][c], n, w, "the intermediate")
                    for i in range(n):
                        assert np.array_equal(r["mid"][c][1 + i], reference(planes[c][i], k, "erode")), (label, k, i, "eroded plane")
                        assert np.array_equal(r["dst"][c][1 + i], reference(planes[c][i], k, "tophat")), (label, k, i, "top-hat")
            out[label] = "ok"
        except AssertionError as e:
            out[label] = "FAILED: " + str(e)[:600]
    return out


def _chain_cases(_native, cal):
    """Through the chain at CHAIN_SIZE, four bands: a slot range that does not start at 0; then two streams."""
    h, w = CHAIN_SIZE
    out = {}
    rng = np.random.default_rng(236188)

    def bev(n):
        a = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        rows = -(-h // CHAIN_BANDS)
        for i in range(1, n, 2):        # every other frame: mid grey with sparse extremes near the band boundaries and the image's ends
            near = np.zeros(h, bool)
            for y in [0, h - 1] + [b * rows for b in range(1, CHAIN_BANDS)]:
                near[max(y - 27, 0):min(y + 28, h)] = True
            hit = (rng.random((h, w)) < 0.04) & near[:, None]
            a[i][~hit] = 128
        return a

    def definition(ctx, slots):
        # the chain's own inputs, as they lie in the arena: the case is about the top-hats alone
        r_pl, b_pl = ctx.download_plane(_native.PLANE_R, 7), ctx.download_plane(_native.PLANE_LAB_B, 7)
        return ({i: reference(r_pl[i], 29, "tophat") for i in slots}, {i: reference(b_pl[i], 55, "tophat") for i in slots})

    ctx = _native.Context(cal["img_size"], (w, h), cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], device=0, capacity=7)
    try:
        ctx.set_walk_min_frames(0)
        fp = _native.filter_params()
        ctx.upload_bev(bev(7))
        ctx.filter_run(7, fp)
        path0 = ctx.last_tophat_path()
        th_r0, th_b0 = ctx.download_plane(_native.PLANE_TOPHAT_R, 7), ctx.download_plane(_native.PLANE_TOPHAT_B, 7)
        want_r, want_b = definition(ctx, range(7))
        first_ok = all(np.array_equal(th_r0[i], want_r[i]) and np.array_equal(th_b0[i], want_b[i]) for i in range(7))
        ctx.upload_bev(bev(5), first=1)
        ctx.filter_run(5, fp, first=1)
        path1 = ctx.last_tophat_path()
        th_r1, th_b1 = ctx.download_plane(_native.PLANE_TOPHAT_R, 7), ctx.download_plane(_native.PLANE_TOPHAT_B, 7)
        want_r, want_b = definition(ctx, range(1, 6))
        out["slot_range"] = dict(
            path_all=path0, path_range=path1, first_run_equals_definition=first_ok,
            wrong_r=[i for i in range(1, 6) if not np.array_equal(th_r1[i], want_r[i])],
            wrong_b=[i for i in range(1, 6) if not np.array_equal(th_b1[i], want_b[i])],
            changed_outside=[i for i in (0, 6) if th_r1[i].tobytes() != th_r0[i].tobytes() or th_b1[i].tobytes() != th_b0[i].tobytes()],
            planes_differ=bool((th_r1[1:6] != th_r0[1:6]).any() and (th_b1[1:6] != th_b0[1:6]).any()))
        ctx.set_streams(2)
        ctx.upload_bev(bev(7))
        ctx.filter_run(7, fp)
        th_r2, th_b2 = ctx.download_plane(_native.PLANE_TOPHAT_R, 7), ctx.download_plane(_native.PLANE_TOPHAT_B, 7)
        want_r, want_b = definition(ctx, range(7))
        out["two_streams"] = dict(path=ctx.last_tophat_path(),
                                  wrong_r=[i for i in range(7) if not np.array_equal(th_r2[i], want_r[i])],
                                  wrong_b=[i for i in range(7) if not np.array_equal(th_b2[i], want_b[i])])
    finally:
        ctx.close()
    return out


MIXED_BANDS = {"LT_MORPH_NB_29E": 2, "LT_MORPH_NB_29D": 4, "LT_MORPH_NB_55E": 3, "LT_MORPH_NB_55D": 4}


def _mixed_bands_case(_native, cal):
    """One chain whose erosions and dilations are cut differently (2 | 4 bands for 29x29, 3 | 4 for 55x55: all split at 236 rows):
    the zones of a slot are shared by its four launches, each with its own boundaries."""
    h, w = CHAIN_SIZE
    n = 4
    ctx = _native.Context(cal["img_size"], (w, h), cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], device=0, capacity=n)
    try:
        ctx.set_walk_min_frames(0)
        ctx.upload_bev(np.random.default_rng(2434).integers(0, 256, (n, h, w, 3), dtype=np.uint8))
        ctx.filter_run(n, _native.filter_params())
        th_r, th_b = ctx.download_plane(_native.PLANE_TOPHAT_R, n), ctx.download_plane(_native.PLANE_TOPHAT_B, n)
        r_pl, b_pl = ctx.download_plane(_native.PLANE_R, n), ctx.download_plane(_native.PLANE_LAB_B, n)
        return dict(path=ctx.last_tophat_path(),
                    wrong_r=[i for i in range(n) if not np.array_equal(th_r[i], reference(r_pl[i], 29, "tophat"))],
                    wrong_b=[i for i in range(n) if not np.array_equal(th_b[i], reference(b_pl[i], 55, "tophat"))])
    finally:
        ctx.close()


def _child(which):
    sys.path.insert(0, ROOT)
    from lane_tracker_amd import _native, calib
    cal = calib.reference_calibration()
    if which == "mixed":
        print("REPORT " + json.dumps(dict(mixed=_mixed_bands_case(_native, cal))))
        return
    ctx = _native.Context(cal["img_size"], (64, 64), cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], device=0, capacity=1)
    try:
        if which == "q8":
            report = _exp_hook_cases(ctx, [("one_q8_n1", 1, 0, "one", 8), ("one_q8_n2", 2, 0, "one", 8), ("one_pair_q8", 2, 1, "one_pair", 8)])
        else:
            report = _exp_hook_cases(ctx, [("one_row", 3, 0, "one_row", 0)])
    finally:
        ctx.close()
    if which == "q8":
        report.update(_chain_cases(_native, cal))
    print("REPORT " + json.dumps(report))


def _run_child(which, extra_env):
    if not os.path.exists(EXP_LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "lane_tracker_amd", "csrc"), "-s", "-j8", "EXPERIMENTS=1"])
    env = dict(os.environ, LANE_TRACKER_AMD_LIB=EXP_LIB, **extra_env)
    path = os.pathsep.join([os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    env["PYTHONPATH"] = path
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which], cwd=ROOT, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("REPORT ")]
    assert line, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(line[-1][len("REPORT "):])


@pytest.fixture(scope="module")
def q8_report():
    env = {"LT_MORPH_ONE": "8", "LT_PAIR_Q": "8"}
    for name in ("LT_MORPH_NB_29E", "LT_MORPH_NB_29D", "LT_MORPH_NB_55E", "LT_MORPH_NB_55D"):
        env[name] = str(CHAIN_BANDS)
    return _run_child("q8", env)


@pytest.mark.gpu
@pytest.mark.parametrize("label", ["one_q8_n1", "one_q8_n2", "one_pair_q8"])
def test_eight_waves_per_task_equal_the_definition(q8_report, label):
    assert q8_report[label] == "ok", q8_report[label]


@pytest.mark.gpu
def test_one_row_kernel_equals_the_definition():
    report = _run_child("one_row", {"LT_MORPH_ONE_ROW": "1"})
    assert report["one_row"] == "ok", report["one_row"]


@pytest.mark.gpu
def test_chain_slot_range_that_does_not_start_at_zero(q8_report):
    got = q8_report["slot_range"]
    print(got)
    assert got["path_all"] == 3 and got["path_range"] == 3, "the batch walks did not take the split-band form"
    assert got["first_run_equals_definition"]
    assert got["planes_differ"], "the second upload did not change the planes: the case checks nothing"
    assert got["wrong_r"] == [] and got["wrong_b"] == [], "slots 1 .. 5 differ from the definition"
    assert got["changed_outside"] == [], "slots outside the range changed"


@pytest.mark.gpu
def test_chain_on_two_streams(q8_report):
    got = q8_report["two_streams"]
    print(got)
    assert got["path"] == 3, "the batch walks did not take the split-band form"
    assert got["wrong_r"] == [] and got["wrong_b"] == [], "slots differ from the definition"


@pytest.mark.gpu
def test_chain_with_other_band_counts_for_erode_and_dilate():
    got = _run_child("mixed", {k: str(v) for k, v in MIXED_BANDS.items()})["mixed"]
    print(got)
    assert got["path"] == 3, "the batch walks did not take the split-band form"
    assert got["wrong_r"] == [] and got["wrong_b"] == [], "slots differ from the definition"


if __name__ == "__main__" and "--child" in sys.argv:
    _child(sys.argv[sys.argv.index("--child") + 1])
