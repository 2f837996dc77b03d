"""Every route into solve_poly2 (csrc/k_search.hip) against exact rational least squares (tests/exact_fit.py).

For each route: upload or produce the mask, run the search, download the pixel lists the search itself kept, take the exact fit OF
THOSE LISTS, and hold the record to it: fit_flags says "rank deficient" exactly where a side has fewer than 3 distinct rows, and the
coefficients pass helpers.coeff_close (1e-4 relative, the BASELINE tolerance).  The masks are the ones the normal equations about
the image centre cancel on (a few adjacent rows at the top or bottom edge) and the tall images on which sum dy^4 passes 2^63.

Which kernel ran is read from the record where the ABI says so -- `_pad`, the pixel-block format: 1 = k_sws_fit2, 2 = k_band_fit2 /
k_band_chain2 / k_band_chain3, 0 = the first-formulation k_sws_fit / k_band_fit -- and follows the launchers' rules (k_search.hip):
  sws2_eligible:  w % 4 == 0, 2 * int(window_width / 2) <= 64, window_height * 255 <= 65535, h <= 8192, w >= 16, its LDS layout
                  (16 bytes per window row of both sides, 2 bytes per level and column, ...) <= 150 KB; ND = 9 for 2 * hw <= 32, else 17
  band2_eligible: w % 4 == 0, 2 * bandwidth + 2 <= 64, h <= 8192, w >= 16, 32 bytes of LDS per band row <= 150 KB
A search the first-formulation kernels cannot hold in LDS is refused with LT_ERR_INVALID (ValueError) before anything is launched.

`_pad` does not tell the u8 variant of a *2 kernel from its bit-plane variant, nor k_search_list from the slot-by-slot fall-back;
those follow from the rules of lt_api.cpp, which the bit-plane tests at the end of this file arrange for:
  slot_reads_bits:       masks_have_bits(slots) && sws_fit_takes_bits / band_fit_takes_bits (= sws2_eligible / band2_eligible)
                         -- a slot has a bit plane after lt_mask_run / lt_filter_run (mark_masks(.., bits 1, u8 0)) and loses it
                         with lt_upload_masks (bits 0, u8 1); lt_download_masks only adds the u8 copy (ensure_u8_masks), so the
                         searches behind it still read the bit plane
  one k_search_list launch: every listed slot has a bit plane && search_list_supported = both geometries take bit planes
  k_band_chain3:         bit planes && h <= 8192 (launch_band_chain; launch_band_fit_one for n = 1 with coefficients by value)
The bit planes of the tests at the end of this file come from the mask chain, at the reference 1100 x 1080, where sum dy^4 stays below
2^53.  The tall designs of this file run through the bit-plane *2 kernels and k_band_chain3 -- sum dy^4 above 2^63 -- in
tests/test_gpu_search_bits.py (test_tall_sliding_window_from_bit_planes, test_tall_band_and_chain_from_bit_planes), on masks
uploaded as bit planes (lt_upload_mask_bits; lt_last_search_source tells the variants apart where `_pad` does not)."""
import ctypes as C
from fractions import Fraction as F

import numpy as np
import pytest

import exact_fit as E
from helpers import coeff_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from lane_tracker_amd import _native
    _native.load()
    return _native


@pytest.fixture(scope="module")
def ctxs(nat):
    cache = {}

    def get(h, w):
        if (h, w) not in cache:
            cache[(h, w)] = nat.Context((2, 2), (w, h), np.eye(3), np.zeros(5), np.eye(3), device=0, capacity=2)
        return cache[(h, w)]
    yield get
    for c in cache.values():
        c.close()


class Worst:
    """worst curve error and worst |delta| / limit seen, printed by the test that collected them"""
    def __init__(self):
        self.err, self.ratio, self.where, self.n = 0.0, 0.0, "", 0

    def add(self, got, fr, fl, h, where):
        err, ratio = float(E.curve_error(got, fr, h)), E.coeff_ratio(got, fl, h)
        if err >= self.err:
            self.err, self.where = err, where
        self.ratio = max(self.ratio, ratio)
        self.n += 1

    def __str__(self):
        return f"{self.n} fits: worst curve error {self.err:.3e} px ({self.where}), worst |delta| / limit {self.ratio:.3e}"


def check_slot(c, slot, rec, h, what, worst, min_rows=3):
    """The record of one slot against the exact fit of the slot's own pixel lists.  min_rows: what the mask was designed to leave
    on each side (so that no case passes by finding nothing)."""
    assert int(rec["detected"]) == 1, f"{what}: not detected"
    for side, key in ((0, "left_coeffs"), (1, "right_coeffs")):
        ys, xs = c.download_pixels(slot, side)
        assert ys.size == int(rec["n_left" if side == 0 else "n_right"])
        rows = np.unique(ys).size
        assert rows >= min_rows, f"{what}, side {side}: the search kept {rows} rows, the mask was made for {min_rows}"
        flagged = bool((int(rec["fit_flags"]) >> side) & 1)
        assert flagged == (rows < 3), f"{what}, side {side}: fit_flags {int(rec['fit_flags'])} with {rows} distinct rows"
        if rows < 3:
            continue
        fr, fl = E.exact_polyfit2(ys, xs)
        got = np.array(rec[key], np.float64)
        worst.add(got, fr, fl, h, f"{what}, side {side}")
        assert coeff_close(got, fl, h), (f"{what}, side {side}: {got.tolist()} against the exact {fl.tolist()}: "
                                         f"|delta| / limit {E.coeff_ratio(got, fl, h):.3g}, curve error {float(E.curve_error(got, fr, h)):.3g} px")


def sws_params(nat, h, w, window_width, mask, window_height=None):
    """A sliding-window search that reaches every row of the mask it is given: windows that tile the rows from the bottom (the rows
    above the last full window are not searched, so the tiling starts at the image's last row or one remainder below it, whichever
    keeps the mask's pixels), no give-up limit, the start slice's 25 %."""
    wh = window_height or {1100: 44, 720: 40}.get(h, 8)
    rem = h % wh
    ignore_bottom = 0 if rem == 0 or mask[h - rem:].any() else rem
    return nat.search_params(window_width=window_width, window_height=wh, no_success_limit=1000, ignore_sides=360 if w >= 1000 else 0,
                             ignore_bottom=ignore_bottom)


def min_rows_of(mask, lo=0, hi=None):
    hi = mask.shape[0] if hi is None else hi
    half = mask.shape[1] // 2
    return min(int(mask[lo:hi, :half].any(axis=1).sum()), int(mask[lo:hi, half:].any(axis=1).sum()))


SEARCH_MASKS = E.search_masks()


def masks_of(h, w):
    return [m for m in SEARCH_MASKS if (m["h"], m["w"]) == (h, w)]


# ---- sliding window -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,window_width,pad", [(1100, 1080, 30, 1), (1100, 1080, 64, 1), (1100, 1080, 66, 0), (720, 1280, 30, 1),
                                                  (97, 64, 10, 1), (97, 64, 34, 1), (97, 66, 10, 0)],
                         ids=["sws2_9", "sws2_17", "sws1_wide", "sws2_9_720", "sws2_9_small", "sws2_17_small", "sws1_w_not_4"])
def test_sliding_window_routes(nat, ctxs, h, w, window_width, pad):
    c = ctxs(h, w)
    worst = Worst()
    if (h, w) == (97, 66):                    # a width that is no multiple of 4: the first-formulation kernel, byte loads
        rng = np.random.default_rng(66)
        masks = [dict(name=f"edge_w66_r{r0}", mask=E.lane_mask(h, w, range(r0, r0 + 4), range(r0, r0 + 3), rng)) for r0 in (0, 3, h - 10, h - 4)]
    else:
        masks = masks_of(h, w)
    for m in masks:
        sp = sws_params(nat, h, w, window_width, m["mask"])
        c.upload_masks(m["mask"][None])
        c.sws_fit_run(1, sp)
        rec = c.download_records(1)[0]
        assert int(rec["_pad"]) == pad, f"{m['name']}: pixel-block format {int(rec['_pad'])}, expected {pad}"
        lo = (h - sp.ignore_bottom) % sp.window_height
        check_slot(c, 0, rec, h, f"sws {window_width} {m['name']}", worst, min(3, min_rows_of(m["mask"], lo, h - sp.ignore_bottom)))
    print(f"\nsliding window {h}x{w}, width {window_width}: {worst}")
    assert worst.n >= len(masks)


# ---- band search --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,bandwidth,pad", [(1100, 1080, 30, 2), (1100, 1080, 32, 0), (720, 1280, 30, 2), (97, 64, 6, 2), (97, 64, 32, 0)],
                         ids=["band2", "band1", "band2_720", "band2_small", "band1_small"])
def test_band_routes(nat, ctxs, h, w, bandwidth, pad):
    c = ctxs(h, w)
    worst = Worst()
    masks = masks_of(h, w)
    sp = nat.search_params(bandwidth=bandwidth, ignore_bottom=0, partial=1.0)
    prev = np.array([0.0, 0.0, int(w * 0.4) + 0.5, 0.0, 0.0, int(w * 0.6) + 0.5])
    for k in range(0, len(masks), 2):          # n = 2: two slots per launch
        pair = [masks[k], masks[(k + 1) % len(masks)]]
        c.upload_masks(np.stack([m["mask"] for m in pair]))
        c.band_fit_run(2, np.stack([prev, prev]), sp)
        recs = c.download_records(2)
        for slot, m in enumerate(pair):
            assert int(recs[slot]["_pad"]) == pad and int(recs[slot]["mode"]) == 1
            check_slot(c, slot, recs[slot], h, f"band {bandwidth} {m['name']}", worst, min(3, min_rows_of(m["mask"])))
    print(f"\nband search {h}x{w}, bandwidth {bandwidth}: {worst}")


# ---- chained band search ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r0,nrows", [(1090, 5), (1097, 3), (0, 5), (3, 4)], ids=["bottom5", "bottom3", "top5", "top4"])
def test_chain_searches_the_next_frame_around_the_exact_curve(nat, ctxs, oracle, r0, nrows):
    """k_band_chain2 over two slots.  Slot 0: a plain dash, 6 pixels wide, in a few edge rows -- its exact fit is the vertical line
    through the dash's middle column + 0.5.  Slot 1: full-height lines on the last columns inside the band around that line and
    on the first columns outside it, half a pixel from the band's edge each: a curve that is half a pixel off anywhere in the
    image keeps another pixel set.  The chain must search slot 1, and keep exactly what the band search around the EXACT curve
    of slot 0 keeps (oracle.band_search)."""
    h, w, bw = 1100, 1080, 30
    c = ctxs(h, w)
    xl, xr = 430, 646
    m0 = np.zeros((h, w), np.uint8)
    m0[r0:r0 + nrows, xl:xl + 6] = 255
    m0[r0:r0 + nrows, xr:xr + 6] = 255
    m1 = np.zeros((h, w), np.uint8)
    for x0 in (xl, xr):                        # band (x0 + 2.5 - 30, x0 + 2.5 + 30): columns x0 - 27 .. x0 + 32
        m1[:, [x0 - 28, x0 - 27, x0 + 32, x0 + 33]] = 255
    sp = nat.search_params(bandwidth=bw, ignore_bottom=0, partial=1.0)
    seed = np.array([0.0, 0.0, xl + 2.5, 0.0, 0.0, xr + 2.5])
    c.upload_masks(np.stack([m0, m1]))
    c.band_fit_chain_run(2, seed, sp, first=0)
    recs = c.band_fit_chain_collect(2)
    worst = Worst()
    assert [int(r["mode"]) for r in recs] == [1, 1] and [int(r["_pad"]) for r in recs] == [2, 2], "slot 1 was not searched"
    check_slot(c, 0, recs[0], h, "chain slot 0", worst, nrows)
    exact0 = [E.exact_polyfit2(*c.download_pixels(0, side)) for side in (0, 1)]
    assert exact0[0][0] == (0, 0, xl + 2.5) and exact0[1][0] == (0, 0, xr + 2.5)
    want = oracle.band_search(m1, exact0[0][1], exact0[1][1], oracle.search_params(bandwidth=bw, ignore_bottom=0, partial=1.0))
    assert want["left_y"].size == 2 * h and want["right_y"].size == 2 * h
    for side, ky, kx in ((0, "left_y", "left_x"), (1, "right_y", "right_x")):
        ys, xs = c.download_pixels(1, side)
        assert np.array_equal(ys, want[ky]) and np.array_equal(xs, want[kx]), \
            f"slot 1, side {side}: searched around {recs[0]['left_coeffs' if side == 0 else 'right_coeffs'].tolist()}, not the exact curve"
    check_slot(c, 1, recs[1], h, "chain slot 1", worst, h)
    print(f"\nchain, dash rows {r0}..{r0 + nrows - 1}: {worst}")


# ---- explicit lists -----------------------------------------------------------------------------------------------
def fit_list(c, ys, xs, h, w):
    """lt_fit_poly2 with the image size given (Context.fit_poly2 passes the context's own) -> (rc, coefficients, flag)"""
    ys, xs = np.ascontiguousarray(ys, np.int32), np.ascontiguousarray(xs, np.int32)
    coef, bad = (C.c_double * 3)(), C.c_int(0)
    rc = c.lib.lt_fit_poly2(c._h, ys.ctypes.data, xs.ctypes.data, int(ys.size), int(h), int(w), coef, C.byref(bad))
    return rc, np.array(coef[:], np.float64), bad.value


def test_fit_list_on_every_case(nat, ctxs):
    """k_fit_list on every generated list.  The figures printed here are the ones DESIGN.md quotes."""
    c = ctxs(97, 64)
    gpu, ref = Worst(), Worst()
    bad = []
    for case in E.generate_cases():
        fr, fl = E.exact_polyfit2(case["ys"], case["xs"])
        rc, got, flag = fit_list(c, case["ys"], case["xs"], case["h"], case["w"])
        assert rc == 0 and flag == 0, f"{case['name']}: rc {rc}, rank-deficient flag {flag} on {np.unique(case['ys']).size} rows"
        gpu.add(got, fr, fl, case["h"], case["name"])
        ref.add(np.polyfit(case["ys"], case["xs"], 2), fr, fl, case["h"], case["name"])
        if not coeff_close(got, fl, case["h"]):
            bad.append((case["name"], E.coeff_ratio(got, fl, case["h"])))
    print(f"\nk_fit_list:  {gpu}\nnp.polyfit:  {ref}")
    assert not bad, f"{len(bad)} of {gpu.n} outside coeff_close, worst {max(bad, key=lambda t: t[1])}"


def test_fit_list_rank_deficient_lists_are_flagged(nat, ctxs):
    c = ctxs(97, 64)
    for ys, xs in (([5, 5, 5], [1, 2, 3]), ([0, 96, 96, 0], [3, 4, 5, 6]), ([65535], [65535])):
        rc, _, flag = fit_list(c, ys, xs, 97, 64)
        assert rc == 0 and flag == 1


@pytest.mark.parametrize("h", [2, 16384, 131072, 200001, 2 ** 30])
def test_fit_list_rows_at_the_end_of_the_coordinate_range(nat, ctxs, h):
    """Rows in [65000, 65535] whatever the image size says: |y - h / 2| ^ 4 alone passes 2^63 at h = 2; from h = 131072 on the
    image centre itself lies outside the coordinate range (the sums are taken about a point kept inside it).  The width follows
    the height from 131072 on."""
    c = ctxs(97, 64)
    rng = np.random.default_rng(h)
    for k, n in enumerate((3, 40, 2000)):
        ys = np.sort(rng.integers(65000, 65536, n))
        ys[0], ys[-1] = 65000, 65535
        if n == 3:
            ys[1] = 65300
        xs = rng.integers(0, 65536, n)
        fr, fl = E.exact_polyfit2(ys, xs)
        rc, got, flag = fit_list(c, ys, xs, h, 64 if h < 131072 else h)
        assert rc == 0 and flag == 0, (rc, flag)
        # (coeff_close scales a and b by the image height; a list's rows end at 65535 however tall the image is said to be)
        assert coeff_close(got, fl, min(h, 65536)), (n, got.tolist(), fl.tolist(), E.coeff_ratio(got, fl, min(h, 65536)))
        # ... and the curve inside the rows that hold the pixels (at h = 2 coeff_close's h^2 and h say little about a and b).
        # 1e-3 px: the three coefficients are f64 roundings of terms up to a y^2 < 2^35, 1e-5 px together; the rest is the solve's.
        shifted = (fr[0], fr[1] + 2 * fr[0] * 65000, (fr[0] * 65000 + fr[1]) * 65000 + fr[2])
        a, b, cc = [float(v) for v in got]
        gshift = (F(a), F(b) + 2 * F(a) * 65000, (F(a) * 65000 + F(b)) * 65000 + F(cc))
        assert E.curve_error(gshift, shifted, 536) < 1e-3, float(E.curve_error(gshift, shifted, 536))


def test_fit_list_hundred_thousand_pixels_far_from_the_centre(nat, ctxs):
    """100 000 pixels at |y - h / 2| ~ 8000: sum dy^4 ~ 4e20."""
    c = ctxs(97, 64)
    rng = np.random.default_rng(8000)
    h, w = 16384, 4096
    ys = np.repeat(np.arange(150, 250), 1000)
    xs = np.concatenate([np.sort(rng.choice(w, size=1000, replace=False)) for _ in range(100)])
    fr, fl = E.exact_polyfit2(ys, xs)
    rc, got, flag = fit_list(c, ys, xs, h, w)
    assert rc == 0 and flag == 0
    assert coeff_close(got, fl, h), (got.tolist(), fl.tolist(), E.coeff_ratio(got, fl, h))


# ---- tall images --------------------------------------------------------------------------------------------------
def tall_mask(h, lane_width):
    """Two full-height lanes `lane_width` wide -> (mask, the lanes' first columns).  Width 64 needs an image of 144 columns (each
    half must hold its lane and the window around it must start at a column >= 0): 2.4 MB at 16384 rows."""
    w = 144 if lane_width == 64 else 64
    xl, xr = (4, 76) if lane_width == 64 else (18 - lane_width // 2, 46 - lane_width // 2)
    m = np.zeros((h, w), np.uint8)
    m[:, xl:xl + lane_width] = 255
    m[:, xr:xr + lane_width] = 255
    m[::7, xl] = 0                             # not a plain rectangle: the fit has all three coefficients to find
    m[::5, xr + lane_width - 1] = 0
    return m, xl, xr


BAND1_MAX_ROWS = 9590          # k_band_fit: 16 bytes of LDS per image row + 160, at most 150 KB (lane_tracker_amd.h)


TALL = [6600, 8192, 8193, 12000, 16384]


def tall_lane_widths(h):
    """4, 20 and 64 pixels at every height: sum dy^4 of a full-height lane passes 2^63 from 6600 rows at width 64, from 8192 at
    width 20, at 16384 at any width; 64 pixels at 16384 rows is the largest the searches can make, 2^70"""
    return (4, 20, 64)


@pytest.mark.parametrize("h", TALL)
def test_tall_sliding_window(nat, ctxs, h):
    """Full-height lanes on tall images, 64-row windows: k_sws_fit2 up to 8192 rows, k_sws_fit above.  At 8192 / 8193 the lower
    75 % are searched (k_sws_fit2's LDS holds 16 bytes per searched row: the two heights differ in the kernel alone)."""
    worst = Worst()
    for lane_width in tall_lane_widths(h):
        mask, xl, xr = tall_mask(h, lane_width)
        c = ctxs(h, mask.shape[1])
        c.upload_masks(mask[None])
        sp = nat.search_params(window_width=64 if lane_width == 64 else 30, window_height=64, no_success_limit=1000, ignore_sides=0,
                               ignore_bottom=0, partial=0.75 if h in (8192, 8193) else 1.0)
        c.sws_fit_run(1, sp)
        rec = c.download_records(1)[0]
        assert int(rec["_pad"]) == (1 if h <= 8192 else 0), f"h {h}, width {lane_width}: pixel-block format {int(rec['_pad'])}"
        check_slot(c, 0, rec, h, f"tall sws h {h} lane {lane_width}", worst, 1000)
    print(f"\ntall sliding window, h {h}: {worst}")


@pytest.mark.parametrize("h", TALL)
def test_tall_band_is_solved_or_refused(nat, ctxs, h):
    """Band searches with bandwidth 30 and 40 around full-height lanes.  Each either solves -- record within coeff_close of the
    exact fit of its own lists, no flag -- or is refused with LT_ERR_INVALID before anything is launched; which of the two is
    fixed here by the documented limit, so a refusal where the limit allows the search fails as well.  From 8192 rows on the
    lower half is searched (k_band_fit2's LDS holds 32 bytes per band row: 4096 rows, and 8192 / 8193 differ in the kernel alone)."""
    worst = Worst()
    for lane_width in tall_lane_widths(h):
        mask, xl, xr = tall_mask(h, lane_width)
        c = ctxs(h, mask.shape[1])
        c.upload_masks(mask[None])
        prev = np.array([[0.0, 0.0, xl + lane_width / 2, 0.0, 0.0, xr + lane_width / 2]])
        for bandwidth in (30, 40):
            bp = nat.search_params(bandwidth=bandwidth, ignore_bottom=0, partial=0.5 if h >= 8192 else 1.0)
            if h > BAND1_MAX_ROWS:
                with pytest.raises(ValueError, match=str(BAND1_MAX_ROWS)):
                    c.band_fit_run(1, prev, bp)
                continue
            c.band_fit_run(1, prev, bp)        # (uploaded masks: k_band_fit2 / k_band_fit, not the one-frame chain kernel)
            rec = c.download_records(1)[0]
            second = bandwidth == 30 and h == 8192
            assert int(rec["_pad"]) == (2 if second else 0), f"h {h}, bandwidth {bandwidth}: pixel-block format {int(rec['_pad'])}"
            check_slot(c, 0, rec, h, f"tall band {bandwidth} h {h} lane {lane_width}", worst, 1000)
    print(f"\ntall band search, h {h}: {worst}")


# ---- bit-plane variants -------------------------------------------------------------------------------------------
# k_sws_fit2<ND, true>, k_band_fit2<true>, k_band_chain3 and k_search_list only see masks the mask chain made (an uploaded u8 mask
# has no bit plane): the slots get theirs from lt_upload_bev + lt_filter_run on dark bird's-eye images with bright marks.
BEV_H, BEV_W = 1100, 1080
DASH_XL, DASH_XR = 426, 642               # first columns of the 12-pixel-wide dashes; their middle: + 5.5


def dash_bev(r0, r1, slant=0):
    """Two bright dashes over rows [r0, r1) (at least 5: the 5 x 5 opening removes less), `slant` rows per column of drift."""
    b = np.full((BEV_H, BEV_W, 3), 20, np.uint8)
    for y in range(r0, r1):
        d = (y - r0) // slant if slant else 0
        b[y, DASH_XL + d:DASH_XL + d + 12] = 255
        b[y, DASH_XR - d:DASH_XR - d + 12] = 255
    return b


def bars_bev(bandwidth):
    """Full-height bars 6 pixels wide across the edges of the band around the dashes' middle columns: three columns inside, three
    outside, the edge itself half a pixel from either."""
    b = np.full((BEV_H, BEV_W, 3), 20, np.uint8)
    for x0 in (DASH_XL, DASH_XR):
        mid = x0 + 5.5
        for a in (int(mid - bandwidth - 0.5) - 2, int(mid + bandwidth + 0.5) - 3):
            b[:, a:a + 6] = 255
    return b


@pytest.fixture(scope="module")
def bev_ctx(nat):
    """a context of the reference calibration (bird's-eye 1080 x 1100), as the mask chain is used everywhere else"""
    from lane_tracker_amd import calib
    cal = calib.reference_calibration()
    assert tuple(cal["warped_size"]) == (BEV_W, BEV_H)
    c = nat.Context(cal["img_size"], cal["warped_size"], cal["cam_matrix"], cal["dist_coeffs"], cal["warp_matrices"][0], device=0, capacity=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bev_designs(oracle):
    """The images and the masks the CPU filter makes of them (computed once)."""
    bevs = dict(dash12=dash_bev(1088, 1100), dash7=dash_bev(1092, 1099), slant=dash_bev(1089, 1099, slant=3), bars=bars_bev(30))
    return {k: (b, oracle.filter_lane_points(b)) for k, b in bevs.items()}


def assert_short_bottom_dash(c, slot, what):
    """the condition the design is for, on the pixels the search itself kept: each side at most 12 rows, inside the last 5 %"""
    for side in (0, 1):
        ys, _ = c.download_pixels(slot, side)
        assert ys.size and ys.min() >= BEV_H - BEV_H // 20 and ys.max() - ys.min() + 1 <= 12 and np.unique(ys).size >= 3, \
            f"{what}, slot {slot}, side {side}: rows {ys.min() if ys.size else None} .. {ys.max() if ys.size else None}"


def load_bevs(c, designs, names):
    c.upload_bev(np.stack([designs[k][0] for k in names]))
    c.filter_run(len(names))
    got = c.download_masks(len(names))
    for k, name in enumerate(names):
        assert np.array_equal(got[k], designs[name][1]), f"{name}: the mask chain's mask is not the CPU filter's"


@pytest.mark.parametrize("names", [("dash12", "dash7"), ("slant", "dash12")], ids=["dash12_dash7", "slant_dash12"])
def test_bit_plane_searches_on_short_bottom_dashes(nat, bev_ctx, bev_designs, names):
    """k_sws_fit2<9, true>, k_sws_fit2<17, true>, k_band_fit2<true> (two slots per launch), k_band_chain3 as the one-frame band
    search, and k_search_list with one sliding-window and one band item, all on bit planes of the mask chain."""
    c = bev_ctx
    worst = Worst()
    load_bevs(c, bev_designs, names)
    for ww in (30, 64):
        sp = nat.search_params(window_width=ww, window_height=44, no_success_limit=1000, ignore_bottom=0)
        c.sws_fit_run(2, sp)
        recs = c.download_records(2)
        for slot in (0, 1):
            assert int(recs[slot]["_pad"]) == 1
            check_slot(c, slot, recs[slot], BEV_H, f"bits sws {ww} {names[slot]}", worst)
            assert_short_bottom_dash(c, slot, f"bits sws {ww}")
    bp = nat.search_params(bandwidth=30, ignore_bottom=0, partial=1.0)
    prev = np.array([0.0, 0.0, DASH_XL + 5.5, 0.0, 0.0, DASH_XR + 5.5])
    c.band_fit_run(2, np.stack([prev, prev + np.array([0, 0, 1.0, 0, 0, 1.0])]), bp)   # unlike coefficients: read from device memory
    recs = c.download_records(2)
    for slot in (0, 1):
        assert int(recs[slot]["_pad"]) == 2 and int(recs[slot]["mode"]) == 1
        check_slot(c, slot, recs[slot], BEV_H, f"bits band {names[slot]}", worst)
        assert_short_bottom_dash(c, slot, "bits band")
    for slot in (0, 1):                                         # one frame per call: a chain of one (launch_band_fit_one)
        c.band_fit_run(1, prev[None], bp, first=slot)
        rec = c.download_records(1, first=slot)[0]
        assert int(rec["_pad"]) == 2 and int(rec["mode"]) == 1
        check_slot(c, slot, rec, BEV_H, f"bits band, one frame, {names[slot]}", worst)
        assert_short_bottom_dash(c, slot, "bits band, one frame")
    sws = nat.search_params(window_width=30, window_height=44, no_success_limit=1000, ignore_bottom=0)
    for order in ([(0, 0, None), (1, 1, prev)], [(1, 0, None), (0, 1, prev)]):
        c.search_fit_list(order, sws, bp)
        recs = c.download_records(2)
        for slot, mode, _ in order:
            assert int(recs[slot]["mode"]) == mode and int(recs[slot]["_pad"]) == (2 if mode else 1)
            check_slot(c, slot, recs[slot], BEV_H, f"bits list, mode {mode}, {names[slot]}", worst)
            assert_short_bottom_dash(c, slot, "bits list")
    print(f"\nbit planes {names}: {worst}")


@pytest.mark.parametrize("first", ["dash12", "dash7"])
def test_bit_plane_chain_searches_the_next_frame_around_the_exact_curve(nat, bev_ctx, oracle, bev_designs, first):
    """k_band_chain3 over two slots: a short bottom dash, then the bars across the edges of the band around the dash's exact curve
    (a vertical line through a half-integer column: a curve half a pixel off anywhere keeps another set)."""
    c = bev_ctx
    worst = Worst()
    load_bevs(c, bev_designs, (first, "bars"))
    bp = nat.search_params(bandwidth=30, ignore_bottom=0, partial=1.0)
    seed = np.array([0.0, 0.0, DASH_XL + 5.5, 0.0, 0.0, DASH_XR + 5.5])
    c.band_fit_chain_run(2, seed, bp, first=0)
    recs = c.band_fit_chain_collect(2)
    assert [int(r["mode"]) for r in recs] == [1, 1] and [int(r["_pad"]) for r in recs] == [2, 2], "slot 1 was not searched"
    check_slot(c, 0, recs[0], BEV_H, "bits chain slot 0", worst)
    assert_short_bottom_dash(c, 0, "bits chain")
    exact0 = [E.exact_polyfit2(*c.download_pixels(0, side)) for side in (0, 1)]
    assert exact0[0][0] == (0, 0, DASH_XL + 5.5) and exact0[1][0] == (0, 0, DASH_XR + 5.5)
    want = oracle.band_search(bev_designs["bars"][1], exact0[0][1], exact0[1][1], oracle.search_params(bandwidth=30, ignore_bottom=0, partial=1.0))
    assert want["left_y"].size == 6 * BEV_H and want["right_y"].size == 6 * BEV_H      # three columns of either bar
    for side, ky, kx in ((0, "left_y", "left_x"), (1, "right_y", "right_x")):
        ys, xs = c.download_pixels(1, side)
        assert np.array_equal(ys, want[ky]) and np.array_equal(xs, want[kx]), f"slot 1, side {side}: not searched around the exact curve of slot 0"
    check_slot(c, 1, recs[1], BEV_H, "bits chain slot 1", worst, BEV_H)
    print(f"\nbit-plane chain behind {first}: {worst}")
