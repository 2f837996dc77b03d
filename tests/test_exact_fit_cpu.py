"""The exact reference of the parabola fit (tests/exact_fit.py) against closed forms, and the references the suite has used so far
-- np.polyfit and the oracle's long-double QR -- against it on the case set the GPU test runs (tests/test_gpu_fit_exact.py): a
case on which a reference leaves its own tolerance would not be a test of the kernel, so that is a condition of the set."""
from fractions import Fraction

import numpy as np
import pytest

import exact_fit as E
from helpers import coeff_close


def test_integer_parabola_is_recovered_exactly():
    ys = np.repeat(np.arange(0, 40), 3)
    for a, b, c in ((2, -7, 11), (0, 3, 5), (1, 0, 0), (-3, 100, 65000)):
        xs = a * ys * ys + b * ys + c
        fr, fl = E.exact_polyfit2(ys, xs)
        assert fr == (a, b, c)
        assert fl.tolist() == [float(a), float(b), float(c)]


def test_vertical_line():
    ys = np.array([5, 5, 9, 200, 200, 1099])
    fr, _ = E.exact_polyfit2(ys, np.full(ys.size, 437))
    assert fr == (0, 0, 437)


def test_fewer_than_three_rows_raise():
    with pytest.raises(ValueError):
        E.exact_polyfit2([4, 4, 9, 9, 9], [1, 2, 3, 4, 5])
    with pytest.raises(ValueError):
        E.exact_polyfit2([], [])


def test_translations_map_the_coefficients_exactly():
    rng = np.random.default_rng(5)
    ys = np.sort(rng.integers(0, 300, 200))
    xs = rng.integers(100, 164, 200)
    (a, b, c), _ = E.exact_polyfit2(ys, xs)
    for dx in (1, -100, 40000):
        assert E.exact_polyfit2(ys, xs + dx)[0] == (a, b, c + dx)
    for dy in (1, 797, 65000):                       # x = a (y - dy)^2 + b (y - dy) + c
        assert E.exact_polyfit2(ys + dy, xs)[0] == (a, b - 2 * a * dy, a * dy * dy - b * dy + c)


def test_curve_error():
    exact = (Fraction(1, 1000), Fraction(-1, 2), Fraction(300))
    assert E.curve_error(exact, exact, 1100) == 0
    assert E.curve_error((Fraction(1, 1000), Fraction(-1, 2), Fraction(301)), exact, 1100) == 1
    assert E.curve_error((Fraction(1, 1000), Fraction(-1, 2) + Fraction(1, 100), Fraction(300)), exact, 1100) == Fraction(1099, 100)
    # a difference with its vertex inside the image: d(y) = (y - 500)^2 / 250000 - 2, largest at the vertex
    d = (Fraction(1, 250000), Fraction(-1000, 250000), Fraction(250000, 250000) - 2)
    assert E.curve_error([p + q for p, q in zip(exact, d)], exact, 1100) == 2
    assert E.curve_error(np.array([0.001, -0.5, 300.0]), (0.001, -0.5, 300.0), 1100) == 0


def test_case_generator_is_deterministic_and_complete():
    a, b = E.generate_cases(), E.generate_cases()
    assert [c["name"] for c in a] == [c["name"] for c in b]
    assert all(np.array_equal(p["ys"], q["ys"]) and np.array_equal(p["xs"], q["xs"]) for p, q in zip(a, b))
    names = [c["name"] for c in a]
    assert len(set(names)) == len(names)
    for h, w in ((1100, 1080), (720, 1280), (97, 64)):
        mine = [c for c in a if (c["h"], c["w"]) == (h, w)]
        starts = {int(c["ys"].min()) for c in mine if c["name"].startswith("edge_")}
        assert starts == {0, 3, h - 10, h - 4, h - 3}
        for c in mine:
            if c["name"].startswith("edge_"):
                rows = np.unique(c["ys"])
                assert 3 <= rows.size <= 5 and rows[-1] - rows[0] == rows.size - 1
                assert 1 <= np.bincount(c["ys"] - rows[0]).min() and np.bincount(c["ys"] - rows[0]).max() <= 29
        for tag in ("dash", "slant", "thin"):
            for where in ("top", "bottom", "centre"):
                for n in (3, 4, 5, 10):
                    c = [c for c in mine if c["name"] == f"{tag}_h{h}_{where}_{n}"][0]
                    assert np.unique(c["ys"]).size == n
        assert any(np.array_equal(np.unique(c["ys"]), [0, 1, h - 1]) and c["ys"].size == 3 for c in mine)
        assert any(np.array_equal(np.unique(c["ys"]), [0, 1, h - 1]) and c["ys"].size > 3 for c in mine)
        assert sum(np.unique(c["ys"]).size == h for c in mine) >= 4
        for c in mine:
            assert c["ys"].min() >= 0 and c["ys"].max() < h and c["xs"].min() >= 0 and c["xs"].max() < w
            assert np.all(np.diff(c["ys"] * 65536 + c["xs"]) > 0), "nonzero() order, no pixel twice"
    m1, m2 = E.search_masks(), E.search_masks()
    assert [m["name"] for m in m1] == [m["name"] for m in m2] and all(np.array_equal(p["mask"], q["mask"]) for p, q in zip(m1, m2))


def test_references_stay_inside_their_tolerance_on_every_case(oracle):
    worst = {"np.polyfit": (0, 0.0, ""), "oracle.polyfit2": (0, 0.0, "")}
    bad = []
    for c in E.generate_cases():
        fr, fl = E.exact_polyfit2(c["ys"], c["xs"])
        for name, got in (("np.polyfit", np.polyfit(c["ys"], c["xs"], 2)), ("oracle.polyfit2", oracle.polyfit2(c["ys"], c["xs"]))):
            err, ratio = E.curve_error(got, fr, c["h"]), E.coeff_ratio(got, fl, c["h"])
            if float(err) >= worst[name][0]:
                worst[name] = (float(err), max(ratio, worst[name][1]), c["name"])
            else:
                worst[name] = (worst[name][0], max(ratio, worst[name][1]), worst[name][2])
            if not coeff_close(got, fl, c["h"]):
                bad.append((name, c["name"], ratio))
    for name, (err, ratio, where) in worst.items():
        print(f"{name}: worst curve error {err:.3e} px (case {where}), worst |delta| / limit {ratio:.3e}")
    assert not bad, bad
