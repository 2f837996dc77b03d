"""Exact least-squares parabola through integer pixels, and the lane-pixel cases the fit is held to.

The device solves x = a y^2 + b y + c from integer moments in f64.  The reference here does the same job with no rounding at all:
moments as Python ints (from per-row counts and per-row column sums, so that a 16384-row list costs 16384 steps, not one per
pixel), the 3x3 normal equations in `fractions.Fraction`.  NumPy and the standard library only."""
from fractions import Fraction

import numpy as np


def row_sums(ys, xs):
    """-> (rows, counts, column sums) of the distinct rows, as Python ints."""
    ys = np.asarray(ys, np.int64).ravel()
    xs = np.asarray(xs, np.int64).ravel()
    if ys.size != xs.size:
        raise ValueError("ys and xs differ in length")
    rows, inv = np.unique(ys, return_inverse=True)
    cnt = np.bincount(inv, minlength=rows.size)
    sx = np.zeros(rows.size, np.int64)
    np.add.at(sx, inv, xs)                      # |x| < 2^16 and < 2^31 pixels: exact in int64
    return [int(v) for v in rows], [int(v) for v in cnt], [int(v) for v in sx]


def exact_polyfit2(ys, xs):
    """np.polyfit(ys, xs, 2) in exact arithmetic -> ((a, b, c) as Fractions, np.array of their floats).
    Raises ValueError on fewer than 3 distinct rows (the parabola is not determined)."""
    rows, cnt, sx = row_sums(ys, xs)
    if len(rows) < 3:
        raise ValueError(f"{len(rows)} distinct rows: a parabola needs 3")
    S = [0] * 5
    T = [0] * 3
    for y, n, s in zip(rows, cnt, sx):
        p = 1
        for k in range(5):
            S[k] += n * p
            if k < 3:
                T[k] += s * p
            p *= y
    # [S4 S3 S2; S3 S2 S1; S2 S1 S0] [a b c]' = [T2 T1 T0]', by Cramer's rule on integers
    def det3(m):
        return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
                + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
    G = [[S[4], S[3], S[2]], [S[3], S[2], S[1]], [S[2], S[1], S[0]]]
    rhs = [T[2], T[1], T[0]]
    d = det3(G)
    if d == 0:
        raise ValueError("singular normal equations")
    sol = []
    for j in range(3):
        M = [[rhs[i] if k == j else G[i][k] for k in range(3)] for i in range(3)]
        sol.append(Fraction(det3(M), d))
    return tuple(sol), np.array([float(v) for v in sol], np.float64)


def _as_fractions(c):
    return [v if isinstance(v, Fraction) else Fraction(float(v)) for v in c]


def curve_error(c, exact, h):
    """max over rows 0 .. h-1 of |x_c(y) - x_exact(y)|, in Fractions (a float is an exact rational).  The difference of two
    parabolas is a parabola: its extreme values over the integer rows lie at row 0, row h-1 or next to its vertex."""
    da, db, dc = [p - q for p, q in zip(_as_fractions(c), _as_fractions(exact))]
    cand = {0, h - 1}
    if da != 0:
        v = -db / (2 * da)
        for y in (int(v) - 1, int(v), int(v) + 1):
            if 0 <= y < h:
                cand.add(y)
    return max(abs((da * y + db) * y + dc) for y in cand)


def coeff_ratio(got, want, h, tol=1e-4):
    """The largest of helpers.coeff_close's three quantities over its limit: <= 1 is what coeff_close(got, want, h) accepts."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    lim = tol * max(1.0, abs(float(want[2])))
    return max(abs(got[0] - want[0]) * h * h, abs(got[1] - want[1]) * h, abs(got[2] - want[2])) / lim


# ---- the cases ---------------------------------------------------------------------------------------------------
# A case is one lane's pixel list inside an h x w image: dict(name, h, w, ys, xs), rows ascending, columns ascending in a row
# (the order of nonzero()).  Columns stay inside the 64-column strip [x0, x0 + 64), x0 = 300 in the wide images.
HEIGHTS = ((1100, 1080), (720, 1280), (97, 64))


def _strip(w):
    return 300 if w >= 400 else 0


def _case(name, h, w, rows, cols_of_row):
    ys, xs = [], []
    for y, cols in zip(rows, cols_of_row):
        cols = sorted(int(v) for v in cols)
        ys += [int(y)] * len(cols)
        xs += cols
    return dict(name=name, h=h, w=w, ys=np.array(ys, np.int64), xs=np.array(xs, np.int64))


def edge_row_cases(h, w, count, rng):
    """3 to 5 adjacent rows at the top or bottom edge (first row 0, 3, h - 10, h - 4 or h - 3: 1090, 1096, 1097 at h = 1100),
    1 to 29 pixels per row, columns uniform in the 64-column strip."""
    out = []
    starts = (0, 3, h - 10, h - 4, h - 3)
    for i in range(count):
        r0 = starts[i % len(starts)]
        nrows = min(int(rng.integers(3, 6)), h - r0)
        rows = list(range(r0, r0 + nrows))
        cols = [_strip(w) + rng.choice(64, size=int(rng.integers(1, 30)), replace=False) for _ in rows]
        out.append(_case(f"edge_h{h}_r{r0}_{i}", h, w, rows, cols))
    return out


def dash_cases(h, w, rng):
    """Plain dashes, 6 pixels wide, of 3, 4, 5 and 10 rows at the top edge, the bottom edge and the centre: straight and slanted
    (one column every two rows); with one pixel per row as well."""
    out = []
    for nrows in (3, 4, 5, 10):
        for where, r0 in (("top", 0), ("bottom", h - nrows), ("centre", h // 2 - nrows // 2)):
            rows = list(range(r0, r0 + nrows))
            x0 = _strip(w) + 20
            out.append(_case(f"dash_h{h}_{where}_{nrows}", h, w, rows, [range(x0, x0 + 6) for _ in rows]))
            out.append(_case(f"slant_h{h}_{where}_{nrows}", h, w, rows, [range(x0 + k // 2, x0 + k // 2 + 6) for k in range(nrows)]))
            out.append(_case(f"thin_h{h}_{where}_{nrows}", h, w, rows, [[x0 + int(rng.integers(0, 8))] for _ in rows]))
    return out


def sparse_cases(h, w, rng):
    """Rows {0, 1, h - 1}: one pixel per row, and many."""
    x0 = _strip(w)
    rows = [0, 1, h - 1]
    return [_case(f"rows01last_one_h{h}", h, w, rows, [[x0 + 10], [x0 + 12], [x0 + 40]]),
            _case(f"rows01last_many_h{h}", h, w, rows, [x0 + rng.choice(64, size=29, replace=False) for _ in rows])]


def full_height_cases(h, w, rng):
    """A lane over every row: a gentle parabola 1, 20 and 64 pixels wide (clipped to the strip), and random pixels in every row."""
    x0 = _strip(w)
    out = []
    for width in (1, 20, 64):
        cols = []
        for y in range(h):
            c = x0 + 32 + 20.0 * ((y / h) - 0.5) ** 2 * 4 - 10
            a = int(round(c - width / 2))
            cols.append([x for x in range(a, a + width) if x0 <= x < x0 + 64])
        out.append(_case(f"full_h{h}_w{width}", h, w, range(h), cols))
    out.append(_case(f"full_random_h{h}", h, w, range(h), [x0 + rng.choice(64, size=int(rng.integers(1, 30)), replace=False) for _ in range(h)]))
    return out


def generate_cases(seed=20240229):
    """The whole set, the same on every call (seeded): the CPU test checks the references on it, the GPU test the kernels."""
    rng = np.random.default_rng(seed)
    out = []
    for (h, w), n_edge in zip(HEIGHTS, (150, 50, 50)):
        out += edge_row_cases(h, w, n_edge, rng)
        out += dash_cases(h, w, rng)
        out += sparse_cases(h, w, rng)
        out += full_height_cases(h, w, rng)
    return out


def lane_mask(h, w, rows_left, rows_right, rng, half=None):
    """A {0, 255} search mask with one lane per side: in each given row a random non-empty set of the columns within `half` of
    int(0.4 w) (left) and int(0.6 w) (right) -- the columns where a sliding-window search without a start-slice hit looks."""
    half = half or (12 if w >= 400 else 4)
    m = np.zeros((h, w), np.uint8)
    for rows, c in ((rows_left, int(w * 0.4)), (rows_right, int(w * 0.6))):
        for y in rows:
            cols = c - half + rng.choice(2 * half, size=int(rng.integers(1, 2 * half + 1)), replace=False)
            m[int(y), cols] = 255
    return m


def search_masks(seed=20240301):
    """Masks for the search routes, per image size: both lanes a dash of 3 to 5 rows at each edge-row start, a 10-row dash at
    the centre, left and right dashes at opposite edges, rows {0, 1, h - 1} and a full-height lane."""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in HEIGHTS:
        for r0 in (0, 3, h - 10, h - 4, h - 3):
            n = min(int(rng.integers(3, 6)), h - r0)
            out.append(dict(name=f"edge_h{h}_r{r0}", h=h, w=w, mask=lane_mask(h, w, range(r0, r0 + n), range(r0, r0 + n), rng)))
        out.append(dict(name=f"centre_h{h}", h=h, w=w, mask=lane_mask(h, w, range(h // 2 - 5, h // 2 + 5), range(h // 2 - 4, h // 2 + 6), rng)))
        out.append(dict(name=f"opposite_h{h}", h=h, w=w, mask=lane_mask(h, w, range(0, 4), range(h - 5, h), rng)))
        out.append(dict(name=f"rows01last_h{h}", h=h, w=w, mask=lane_mask(h, w, (0, 1, h - 1), (0, 1, h - 1), rng)))
        out.append(dict(name=f"full_h{h}", h=h, w=w, mask=lane_mask(h, w, range(h), range(h), rng)))
    return out
