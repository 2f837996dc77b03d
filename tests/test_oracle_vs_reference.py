"""Fuzz: the CPU oracle against the reference's own NumPy methods on seeded random cases.  The reference's answers
are stored in tests/golden/fuzz_reference.npz (tests/gen_golden.py --only fuzz) as SHA-256 digests of its pixel and
centroid arrays, so the oracle is held to them bit for bit wherever the suite runs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gen  # noqa: E402
from helpers import GOLDEN  # noqa: E402


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "fuzz_reference.npz"))


def test_sliding_window_search_fuzz(oracle, ref):
    cases = gen.fuzz_sws_cases()
    assert len(cases) == len(ref["sws_detected"])
    n_det = 0
    for i, (m, p) in enumerate(cases):
        r = oracle.sliding_window_search(m, oracle.search_params(**p))
        assert r["detected"] == bool(ref["sws_detected"][i]), (i, p)
        if r["detected"]:
            n_det += 1
            got = [gen.digest(r[f]) for f in gen.FUZZ_FIELDS]
            assert got == list(ref["sws_digests"][i]), (i, p)
    assert n_det > 40


def test_band_search_fuzz(oracle, ref):
    cases = gen.fuzz_band_cases()
    assert len(cases) == len(ref["band_detected"])
    for i, (m, lc, rc, p) in enumerate(cases):
        r = oracle.band_search(m, lc, rc, oracle.search_params(**p))
        assert r["detected"] == bool(ref["band_detected"][i]), (i, p)
        if r["detected"]:
            got = [gen.digest(r[f]) for f in gen.FUZZ_FIELDS[:4]]
            assert got == list(ref["band_digests"][i][:4]), (i, p)
