"""The bit-plane searches (csrc/k_search.hip: k_band_sums_bits, k_sws_fit2<9|17, true>, k_band_fit2<true>, k_band_chain3,
k_search_list) on masks of any kind, uploaded as bit planes (lt_upload_mask_bits) -- not only on what the mask chain leaves at
1100 x 1080.  Every comparison is equality with the CPU oracle (oracle.sliding_window_search, oracle.band_search) or with the
fixtures the reference made (tests/golden/); coefficients are held to the exact rational fit of the lists (tests/exact_fit.py) within
helpers.coeff_close.  lt_last_search_source says whether the bit-plane kernels ran; a test that expects them asserts it.

The searches from bit planes of the fixtures, the fuzz and the kernel-limit cases are the `_bits` tests of tests/test_gpu_parity.py."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import exact_fit as E
from helpers import FIXTURE_BITS_SOURCE, coeff_close, golden_files, params_of, unpack_mask
from lane_tracker_amd import utils
from test_gpu_fit_exact import Worst, check_slot, tall_mask

SIDES = (("left_y", "left_x"), ("right_y", "right_x"))


# ---- a. the packing, no GPU -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 63, 64, 65, 68, 1080, 4100])
def test_pack_mask_bits_is_packbits_little_on_rows_padded_to_64_columns(w):
    rng = np.random.default_rng(w)
    for shape in ((3, w), (2, 5, w)):
        m = ((rng.random(shape) < 0.5) * rng.integers(1, 256, shape)).astype(np.uint8)       # non-zero bytes of every value
        m[..., 0, w - 1] = 7
        m[..., -1, 0] = 1
        padded = np.zeros(shape[:-1] + ((w + 63) // 64 * 64,), np.uint8)
        padded[..., :w] = m != 0
        want = np.packbits(padded, axis=-1, bitorder="little")
        got = utils.pack_mask_bits(m)
        assert got.dtype == np.uint64 and got.shape == shape[:-1] + ((w + 63) // 64,)
        assert got.astype("<u8").tobytes() == want.tobytes()
        assert np.array_equal(utils.pack_mask_bits(m != 0), got)                             # bool masks
        assert np.array_equal(utils.unpack_mask_bits(got, w), (m != 0) * np.uint8(255))
        assert np.array_equal(utils.unpack_mask_bits(got, w, value=1), (m != 0).astype(np.uint8))
        dirty = got.copy()
        if w % 64:
            dirty[..., -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(w % 64)             # bits at columns >= w are dropped
        assert np.array_equal(utils.unpack_mask_bits(dirty, w), (m != 0) * np.uint8(255))
    with pytest.raises(ValueError):
        utils.unpack_mask_bits(np.zeros((2, 2), np.uint64), 64)


# ---- the device tests -----------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from lane_tracker_amd import _native
    _native.load()
    return _native


@pytest.fixture(scope="module")
def ctxs(nat):
    """one context of three slots per image size"""
    cache = {}

    def get(h, w):
        if (h, w) not in cache:
            cache[(h, w)] = nat.Context((2, 2), (w, h), np.eye(3), np.zeros(5), np.eye(3), device=0, capacity=3)
        return cache[(h, w)]
    yield get
    for c in cache.values():
        c.close()


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: {got.shape[0]} entries, the oracle has {want.shape[0]}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: {got[bad[0]]} for {want[bad[0]]}"


def hold(c, slot, rec, want, h, what, centroids=False):
    """The record and the lists of a slot against the oracle's search of the slot's mask; the coefficients against the exact fit
    of those lists."""
    assert bool(rec["detected"]) == want["detected"], f"{what}: detected {int(rec['detected'])}"
    for side, (ky, kx) in enumerate(SIDES):
        y, x = c.download_pixels(slot, side)
        assert_same(y, want[ky], f"{what}: {ky}")
        assert_same(x, want[kx], f"{what}: {kx}")
    if centroids:
        assert c.download_centroids(slot, 0) == want["left_centroids"], f"{what}: left centroids"
        assert c.download_centroids(slot, 1) == want["right_centroids"], f"{what}: right centroids"
    if not want["detected"]:
        return
    assert (int(rec["n_left"]), int(rec["n_right"])) == (want["left_y"].size, want["right_y"].size), what
    for side, key in enumerate(("left_coeffs", "right_coeffs")):
        ys, xs = want[SIDES[side][0]], want[SIDES[side][1]]
        rows = np.unique(ys).size
        assert bool((int(rec["fit_flags"]) >> side) & 1) == (rows < 3), f"{what}, side {side}: fit_flags {int(rec['fit_flags'])}, {rows} rows"
        if rows >= 3:
            fl = E.exact_polyfit2(ys, xs)[1]
            got = np.array(rec[key], np.float64)
            assert coeff_close(got, fl, h), f"{what}, side {side}: {got.tolist()} for the exact {fl.tolist()}"


# ---- d. small shapes around the word boundaries ---------------------------------------------------------------------
SHAPES = [(64, 16), (40, 64), (40, 68), (130, 124), (130, 128), (130, 132), (96, 4096), (96, 4100)]
# k_band_sums_bits sums at most 64 words of a row: 4096 columns.  No plane is wider: lt_create refuses a bird's-eye width above 4096
# (the mask chain's limit as well), which is what the tests pin at 4100 columns -- no search runs there, on bit planes or on bytes.
MAX_WIDTH = 4096


def ctx_or_refusal(ctxs, h, w):
    """the context of the size, or None once the refusal of a size no context can have has been seen"""
    if w <= MAX_WIDTH:
        return ctxs(h, w)
    with pytest.raises(ValueError, match="bird's-eye width in \\[2, 4096\\]"):
        ctxs(h, w)
    return None


def shape_masks(h, w):
    """random at three densities; full columns 0, 63, 64, w - 1 and full rows 0, h - 1; all ones"""
    rng = np.random.default_rng(h * 10007 + w)
    masks = [((rng.random((h, w)) < d) * 255).astype(np.uint8) for d in (1e-3, 0.05, 0.5)]
    edges = np.zeros((h, w), np.uint8)
    edges[:, [x for x in (0, 63, 64, w - 1) if x < w]] = 255
    edges[[0, h - 1], :] = 255
    return masks + [edges, np.full((h, w), 255, np.uint8)]


def slot_triples(masks):
    """the five masks three per launch: (0, 1, 2), then (3, 4, 0)"""
    return [(0, 1, 2), (3, 4, 0)]


def sws_param_sets(h, w):
    for ww, wh, sides, bottom, start, partial in itertools.product((4, 20, 31, 64), (7, 25), (0, w // 4), (0, 7), (0.25, 1.0), (1.0, 0.5)):
        yield dict(window_width=ww, window_height=wh, ignore_sides=sides, ignore_bottom=bottom, start_slice=start, partial=partial,
                   search_range=8 if w < 200 else 20)


def band_curves(h, w):
    """previous curves through columns 0.5, 63.5 and w - 1.5 (vertical, and slanted through them at row 0), and off the image"""
    on = [0.5, 63.5, w - 1.5]
    vertical = [[0.0, 0.0, c] for c in on]
    slanted = [[1e-3, -0.05, c] for c in on]
    off = [0.0, 0.0, w + 70.5]
    return [vertical[0] + vertical[1], vertical[1] + vertical[2], vertical[2] + vertical[0], slanted[0] + slanted[2],
            slanted[1] + slanted[0], vertical[1] + off, off + [0.0, 0.0, -40.5]]


@gpu
@pytest.mark.parametrize("h,w", SHAPES, ids=lambda v: str(v))
def test_sliding_window_search_from_bit_planes_around_the_word_boundaries(nat, ctxs, oracle, h, w):
    c = ctx_or_refusal(ctxs, h, w)
    if c is None:
        return
    masks = shape_masks(h, w)
    n_cases = n_detected = n_refused = 0
    for triple in slot_triples(masks):
        c.upload_mask_bits(np.stack([masks[k] for k in triple]))
        for p in sws_param_sets(h, w):
            if 2 * (p["window_width"] // 2) > w:           # the reference's window wraps round the image edge: refused
                with pytest.raises(ValueError, match="wider than the image"):
                    c.sws_fit_run(3, nat.search_params(**p))
                n_refused += 1
                continue
            c.sws_fit_run(3, nat.search_params(**p))
            assert c.last_search_source() == 1, p
            recs = c.download_records(3)
            for slot, k in enumerate(triple):
                want = oracle.sliding_window_search(masks[k], oracle.search_params(**p))
                hold(c, slot, recs[slot], want, h, f"{h}x{w} mask {k} slot {slot} {p}", centroids=True)
                n_cases += 1
                n_detected += want["detected"]
    print(f"\nsliding window {h}x{w} from bit planes: {n_cases} searches, {n_detected} detected, {n_refused} launches refused")
    assert n_detected >= n_cases // 8          # the designs are searched, not all empty
    assert n_refused == (2 * 96 if w == 16 else 0)     # windows of 20, 31 and 64 columns in 16


@gpu
@pytest.mark.parametrize("h,w", SHAPES, ids=lambda v: str(v))
def test_band_search_from_bit_planes_around_the_word_boundaries(nat, ctxs, oracle, h, w):
    """Three slots per launch, each around its own curves (k_band_fit2<true>, coefficients from device memory), and slot 1 alone
    (k_band_chain3 as a chain of one, coefficients by value)."""
    c = ctx_or_refusal(ctxs, h, w)
    if c is None:
        return
    masks = shape_masks(h, w)
    curves = band_curves(h, w)
    n_cases = n_detected = 0
    for triple in slot_triples(masks):
        c.upload_mask_bits(np.stack([masks[k] for k in triple]))
        for bandwidth, bottom, partial, q in itertools.product((0, 5, 31), (0, 7), (1.0, 0.5), range(len(curves))):
            p = dict(bandwidth=bandwidth, ignore_bottom=bottom, partial=partial)
            prev = np.array([curves[(q + slot) % len(curves)] for slot in range(3)])
            c.band_fit_run(3, prev, nat.search_params(**p))
            assert c.last_search_source() == 1, p
            recs = c.download_records(3)
            for slot, k in enumerate(triple):
                want = oracle.band_search(masks[k], prev[slot, :3], prev[slot, 3:], oracle.search_params(**p))
                assert int(recs[slot]["mode"]) == 1 and int(recs[slot]["_pad"]) == 2
                hold(c, slot, recs[slot], want, h, f"{h}x{w} mask {k} slot {slot} {p} around {prev[slot].tolist()}")
                n_cases += 1
                n_detected += want["detected"]
            c.band_fit_run(1, prev[1:2], nat.search_params(**p), first=1)
            assert c.last_search_source() == 1, p
            rec = c.download_records(1, first=1)[0]
            want = oracle.band_search(masks[triple[1]], prev[1, :3], prev[1, 3:], oracle.search_params(**p))
            assert int(rec["mode"]) == 1 and int(rec["_pad"]) == 2
            hold(c, 1, rec, want, h, f"{h}x{w} mask {triple[1]} alone {p} around {prev[1].tolist()}")
    print(f"\nband search {h}x{w} from bit planes: {n_cases} searches of three, {n_detected} detected")
    assert n_detected >= n_cases // 16


# ---- b. round trip, and the neighbours' u8 masks ----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("h,w", SHAPES, ids=lambda v: str(v))
def test_bit_plane_upload_round_trip_leaves_the_neighbour_slots_alone(nat, ctxs, oracle, h, w):
    c = ctx_or_refusal(ctxs, h, w)
    if c is None:
        return
    rng = np.random.default_rng(h + w)
    a, b = [((rng.random((h, w)) < 0.05) * 255).astype(np.uint8) for _ in range(2)]
    m = ((rng.random((h, w)) < 0.3) * rng.integers(1, 256, (h, w))).astype(np.uint8)         # a bit is "byte != 0"
    m[0, w - 1] = m[h - 1, 0] = 1
    c.upload_masks(np.stack([a, b, a]))
    c.upload_masks(b[None], first=2)
    c.upload_mask_bits(m[None], first=1)
    got = c.download_masks(3)
    assert np.array_equal(got[1], (m != 0) * np.uint8(255)), "slot 1 is not the mask that was uploaded as a bit plane"
    assert np.array_equal(got[0], a) and np.array_equal(got[2], b), "a neighbour's u8 mask changed"
    p = dict(window_width=min(20, w), window_height=7, ignore_sides=0, ignore_bottom=0, search_range=8)
    m = got[1]                                             # (the u8 kernels sum byte values: the oracle gets the mask the slot holds)
    for slot, mask, source in ((0, a, 0), (2, b, 0), (1, m, 1)):
        c.sws_fit_run(1, nat.search_params(**p), first=slot)
        assert c.last_search_source() == source, f"slot {slot}"
        hold(c, slot, c.download_records(1, first=slot)[0], oracle.sliding_window_search(mask, oracle.search_params(**p)), h,
             f"{h}x{w} slot {slot}", centroids=True)
    c.sws_fit_run(3, nat.search_params(**p))               # one slot of the range holds bytes only: the range is searched as bytes
    assert c.last_search_source() == 0
    recs = c.download_records(3)
    for slot, mask in enumerate((a, m, b)):
        hold(c, slot, recs[slot], oracle.sliding_window_search(mask, oracle.search_params(**p)), h, f"{h}x{w} range, slot {slot}", centroids=True)
    assert np.array_equal(c.download_masks(3), got)


# ---- bits at columns >= w ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("h,w", [(40, 68), (1100, 1080)], ids=lambda v: str(v))
def test_bits_beyond_the_last_column_are_cleared_on_upload(nat, ctxs, oracle, h, w):
    """Words with every bit at a column >= w set, through the C entry point itself: masks, searches and the visualisation's plane
    are those of the mask."""
    from lane_tracker_amd import synth
    c = ctxs(h, w)
    if w == 1080:
        m = synth.synth_mask(3, noise=5e-3)[0]
        m[:, w - 14:] = 255                                # a lane on the last columns, next to the dead bits
        sp = dict(window_width=30, window_height=40, ignore_sides=0, ignore_bottom=0)
        prev = [0.0, 0.0, 439.5, 0.0, 0.0, w - 1.5]
    else:
        m = shape_masks(h, w)[1]
        m[:, w - 3:] = 255
        sp = dict(window_width=20, window_height=7, ignore_sides=0, ignore_bottom=0, search_range=8)
        prev = [0.0, 0.0, 20.5, 0.0, 0.0, w - 1.5]
    bits = utils.pack_mask_bits(m[None])
    bits[..., -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(w % 64)
    bits = np.ascontiguousarray(bits)
    rc = c.lib.lt_upload_mask_bits(c._h, bits.ctypes.data_as(C.c_void_p), 1, 1)
    assert rc == 0
    assert np.array_equal(c.download_masks(1, first=1)[0], m)
    c.sws_fit_run(1, nat.search_params(**sp), first=1)
    assert c.last_search_source() == 1
    hold(c, 1, c.download_records(1, first=1)[0], oracle.sliding_window_search(m, oracle.search_params(**sp)), h, f"{h}x{w} sws", centroids=True)
    for n in (1, 2):                                       # k_band_chain3 (one frame), k_band_fit2 (slots 1 and 2)
        if n == 2:
            assert c.lib.lt_upload_mask_bits(c._h, bits.ctypes.data_as(C.c_void_p), 2, 1) == 0
        bp = dict(bandwidth=31, ignore_bottom=0, partial=1.0)
        c.band_fit_run(n, np.array([prev] * n), nat.search_params(**bp), first=1)
        assert c.last_search_source() == 1
        recs = c.download_records(n, first=1)
        want = oracle.band_search(m, prev[:3], prev[3:], oracle.search_params(**bp))
        for k in range(n):
            hold(c, 1 + k, recs[k], want, h, f"{h}x{w} band, {n} per launch, slot {1 + k}")
    items = np.zeros(1, nat.VIZ_ITEM_DTYPE)
    items[0]["slot"], items[0]["kind"] = 1, 0              # the bare mask, read from the bit plane
    pic = c.search_viz_run(items)
    assert np.array_equal(pic[0], np.repeat(m[:, :, None], 3, axis=2))


# ---- c. two fixtures per launch -------------------------------------------------------------------------------------
@gpu
def test_two_fixtures_per_launch_in_slots_1_and_2(nat, ctxs, oracle):
    """Slots (1, 2) hold two different fixtures of one shape and are searched by one launch with the first one's parameters: frame
    indexing in k_band_sums_bits and in the two-workgroup launches.  Slot 1 is held to the fixture, both to the oracle."""
    sws = [p for p in golden_files("sws_") if tuple(np.load(p)["mask_shape"]) == (1100, 1080)]
    band = golden_files("band")
    c = ctxs(1100, 1080)
    for files, kind in ((sws, "sws"), (band, "band")):
        loaded = [np.load(p) for p in files]
        masks = [unpack_mask(d) for d in loaded]
        for k, path in enumerate(files):
            name, j = os.path.basename(path), (k + 1) % len(files)
            d, p = loaded[k], params_of(loaded[k])
            c.upload_mask_bits(np.stack([masks[k], masks[j]]), first=1)
            if kind == "sws":
                c.sws_fit_run(2, nat.search_params(**p), first=1)
                want = [oracle.sliding_window_search(m, oracle.search_params(**p)) for m in (masks[k], masks[j])]
            else:
                prev = np.stack([np.concatenate([e["prev_left"], e["prev_right"]]) for e in (d, loaded[j])])
                c.band_fit_run(2, prev, nat.search_params(**p), first=1)
                want = [oracle.band_search(m, pv[:3], pv[3:], oracle.search_params(**p)) for m, pv in zip((masks[k], masks[j]), prev)]
            assert c.last_search_source() == FIXTURE_BITS_SOURCE[name], name
            recs = c.download_records(2, first=1)
            for q in (0, 1):
                hold(c, 1 + q, recs[q], want[q], 1100, f"{name} in slot 1, slot {1 + q}", centroids=kind == "sws")
            assert bool(recs[0]["detected"]) == bool(d["detected"]), name
            if bool(d["detected"]):
                for side, (ky, kx) in enumerate(SIDES):
                    y, x = c.download_pixels(1, side)
                    assert_same(y, d[ky], f"{name}: {ky}")
                    assert_same(x, d[kx], f"{name}: {kx}")
                assert coeff_close(recs[0]["left_coeffs"], d["left_coeffs"]) and coeff_close(recs[0]["right_coeffs"], d["right_coeffs"]), name


# ---- e. k_search_list and k_band_chain3 on arbitrary masks ----------------------------------------------------------
@pytest.fixture(scope="module")
def noisy_lanes():
    """three masks of one pair of lanes: salt noise 5e-3, 0.05, and the first shifted by three columns"""
    from lane_tracker_amd import synth
    m0, lc, rc = synth.synth_mask(31, noise=5e-3)
    m1 = synth.synth_mask(31, noise=0.05)[0]
    return [m0, m1, np.roll(m0, 3, axis=1)], np.concatenate([lc + np.array([0, 0, 0.4]), rc + np.array([0, 0, -0.6])])


@gpu
def test_search_list_on_noisy_bit_planes(nat, ctxs, oracle, noisy_lanes):
    masks, prev = noisy_lanes
    c = ctxs(1100, 1080)
    c.upload_mask_bits(np.stack(masks))
    sp, bp = dict(window_width=30, window_height=40, ignore_sides=200), dict(bandwidth=25, ignore_bottom=30, partial=1.0)

    def run(items, source):
        c.search_fit_list([(slot, mode, prev if mode else None) for slot, mode in items], nat.search_params(**sp), nat.search_params(**bp))
        assert c.last_search_source() == source, items
        recs = c.download_records(3)
        for slot, mode in items:
            want = oracle.band_search(masks[slot], prev[:3], prev[3:], oracle.search_params(**bp)) if mode else \
                oracle.sliding_window_search(masks[slot], oracle.search_params(**sp))
            assert int(recs[slot]["mode"]) == mode and int(recs[slot]["_pad"]) == (2 if mode else 1), (items, slot)
            assert want["detected"], "the design is two lanes in noise"
            hold(c, slot, recs[slot], want, 1100, f"list {items}, slot {slot}", centroids=mode == 0)

    for items in ([(0, 0), (2, 1)], [(2, 1), (0, 0)], [(2, 0), (0, 1)], [(1, 1), (2, 0), (0, 0)], [(0, 1), (1, 0), (2, 1)], [(1, 0)], [(1, 1)]):
        run(items, 1)
    # slot 1 as bytes: the list is no longer one launch over bit planes; slot by slot, each from the form it holds
    c.upload_masks(masks[1][None], first=1)
    run([(0, 0), (1, 1)], 0)
    run([(1, 0), (2, 1)], 0)
    run([(0, 0), (2, 1)], 1)


@gpu
def test_band_chain_over_three_noisy_bit_planes(nat, ctxs, oracle, noisy_lanes):
    """k_band_chain3: every slot is searched around the record the chain left in the slot before it (the first around the seed)."""
    masks, seed = noisy_lanes
    c = ctxs(1100, 1080)
    c.upload_mask_bits(np.stack(masks))
    for bp in (dict(bandwidth=25, ignore_bottom=30, partial=1.0), dict(bandwidth=31, ignore_bottom=0, partial=0.5)):
        c.band_fit_chain_run(3, seed, nat.search_params(**bp), first=0)
        assert c.last_search_source() == 1
        recs = c.band_fit_chain_collect(3)
        prev = seed
        for slot in range(3):
            want = oracle.band_search(masks[slot], prev[:3], prev[3:], oracle.search_params(**bp))
            assert int(recs[slot]["mode"]) == 1 and int(recs[slot]["_pad"]) == 2 and want["detected"], slot
            hold(c, slot, recs[slot], want, 1100, f"chain {bp}, slot {slot}")
            prev = np.concatenate([recs[slot]["left_coeffs"], recs[slot]["right_coeffs"]])


# ---- f. tall images -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("h", [6600, 8192])
def test_tall_sliding_window_from_bit_planes(nat, ctxs, oracle, h):
    """test_gpu_fit_exact.py's full-height lanes through k_band_sums_bits + k_sws_fit2<9|17, true>: sum dy^4 of a side passes 2^63
    at width 64 (6600 rows) and at width 20 (8192 rows)."""
    worst = Worst()
    for lane_width in (4, 20, 64):
        mask, xl, xr = tall_mask(h, lane_width)
        c = ctxs(h, mask.shape[1])
        c.upload_mask_bits(mask[None])
        p = dict(window_width=64 if lane_width == 64 else 30, window_height=64, no_success_limit=1000, ignore_sides=0, ignore_bottom=0,
                 partial=0.75 if h == 8192 else 1.0)
        c.sws_fit_run(1, nat.search_params(**p))
        assert c.last_search_source() == 1
        rec = c.download_records(1)[0]
        assert int(rec["_pad"]) == 1
        hold(c, 0, rec, oracle.sliding_window_search(mask, oracle.search_params(**p)), h, f"tall sws h {h} lane {lane_width}", centroids=True)
        check_slot(c, 0, rec, h, f"tall sws from bits, h {h} lane {lane_width}", worst, 1000)
    print(f"\ntall sliding window from bit planes, h {h}: {worst}")


@gpu
@pytest.mark.parametrize("h", [6600, 8192])
def test_tall_band_and_chain_from_bit_planes(nat, ctxs, oracle, h):
    """Bandwidth 30 around the full-height lanes, lower half (k_band_fit2's LDS holds 32 bytes per band row): two slots per launch
    (k_band_fit2<true>), one frame (k_band_chain3 as a chain of one), a chain of two (k_band_chain3).  At 8192 rows and width 64
    sum dy^4 of a side is 1.4e19: above 2^63, so a total read as a signed word gives another parabola."""
    worst = Worst()
    for lane_width in (4, 20, 64):
        mask, xl, xr = tall_mask(h, lane_width)
        c = ctxs(h, mask.shape[1])
        c.upload_mask_bits(np.stack([mask, mask]))
        prev = np.array([0.0, 0.0, xl + lane_width / 2, 0.0, 0.0, xr + lane_width / 2])
        bp = dict(bandwidth=30, ignore_bottom=0, partial=0.5)
        want = oracle.band_search(mask, prev[:3], prev[3:], oracle.search_params(**bp))
        nudged = prev + np.array([0, 0, 0.25, 0, 0, -0.25])          # unlike coefficients: read from device memory
        want_nudged = oracle.band_search(mask, nudged[:3], nudged[3:], oracle.search_params(**bp))

        def check(recs, what, wants=(want, want)):
            assert c.last_search_source() == 1, what
            for slot, rec in enumerate(recs):
                assert int(rec["mode"]) == 1 and int(rec["_pad"]) == 2, what
                hold(c, slot, rec, wants[slot], h, f"{what}, slot {slot}")
                check_slot(c, slot, rec, h, f"{what}, slot {slot}", worst, 1000)

        c.band_fit_run(2, np.stack([prev, nudged]), nat.search_params(**bp))
        check(c.download_records(2), f"tall band h {h} lane {lane_width}, two per launch", (want, want_nudged))
        c.band_fit_run(1, prev[None], nat.search_params(**bp))
        check(c.download_records(1), f"tall band h {h} lane {lane_width}, one frame")
        c.band_fit_chain_run(1, prev, nat.search_params(**bp), first=0)
        check(c.band_fit_chain_collect(1), f"tall chain of one h {h} lane {lane_width}")
        # a chain of two: slot 1 is searched around the fit the chain left in slot 0
        c.band_fit_chain_run(2, prev, nat.search_params(**bp), first=0)
        recs = c.band_fit_chain_collect(2)
        fit0 = np.concatenate([recs[0]["left_coeffs"], recs[0]["right_coeffs"]])
        want1 = oracle.band_search(mask, fit0[:3], fit0[3:], oracle.search_params(**bp))
        assert [int(r["mode"]) for r in recs] == [1, 1] and c.last_search_source() == 1
        hold(c, 0, recs[0], want, h, f"tall chain of two h {h} lane {lane_width}, slot 0")
        hold(c, 1, recs[1], want1, h, f"tall chain of two h {h} lane {lane_width}, slot 1")
        for slot in (0, 1):
            check_slot(c, slot, recs[slot], h, f"tall chain of two h {h} lane {lane_width}, slot {slot}", worst, 1000)
    print(f"\ntall band searches from bit planes, h {h}: {worst}")
