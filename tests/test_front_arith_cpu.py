"""The front end's blend and Lab-b arithmetic (lane_tracker_amd/csrc/front_arith.h) on the CPU: tests/front_arith_host.cpp is
the same header compiled with the system C++ compiler, so these are the very expressions k_frontend.hip runs.

  blend     both forms (24-bit integer multiplies, fp32 fma chain) against (sum_i w_i p_i + 512) >> 10 in int64: every pair of
            fractions, tap channels from {0, 1, 2, 127, 128, 254, 255}^4 plus 2000 random sets, every pattern of taps outside the
            frame (weight 0) -- zero mismatches
  Lab b     all 2^24 RGB triples against the oracle -- zero mismatches, with and without the clamp of the table index
  clamp     the predicate that lets the kernel drop the clamp: true for the shipped tables, false for a matrix whose row sums
            to 7000, for which the clamped form is still exact on the triples that reach the clamp"""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no C++ compiler")


@pytest.fixture(scope="module")
def fa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("front_arith") / "libfront_arith_host.so")
    subprocess.check_call([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "lane_tracker_amd", "csrc"), os.path.join(ROOT, "tests", "front_arith_host.cpp"),
                           "-o", out])
    lib = C.CDLL(out)
    lib.fa_blend_all.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint, C.c_void_p]
    lib.fa_blend_all.restype = None
    lib.fa_lab_clamp_is_dead.argtypes = [C.c_int, C.c_void_p]
    lib.fa_lab_clamp_is_dead.restype = C.c_int
    lib.fa_lab_b.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.fa_lab_b.restype = None
    return lib


def tap_sets(n_random, seed):
    """(n, 4 taps, 3 channels) u8: the 7^4 extreme combinations (each channel walks them in another order) + random sets."""
    ext = np.array(list(itertools.product((0, 1, 2, 127, 128, 254, 255), repeat=4)), np.uint8)          # (2401, 4)
    rng = np.random.default_rng(seed)
    sets = np.stack([ext, np.roll(ext, 777, axis=0), ext[::-1]], axis=2)                                 # (2401, 4, 3)
    return np.concatenate([sets, rng.integers(0, 256, (n_random, 4, 3), dtype=np.uint8)], axis=0)


def blend_reference(sets, m):
    """[fy][fx][n][3]: (sum_i w_i p_i + 512) >> 10 in int64, w = {gx gy, fx gy, gx fy, fx fy}, 0 for a tap outside the frame."""
    f = np.arange(32, dtype=np.int64)
    fy, fx = np.meshgrid(f, f, indexing="ij")
    w = np.stack([(32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy], axis=-1)            # (32, 32, 4)
    w = w * np.array([(m >> i) & 1 for i in range(4)], np.int64)
    s = np.einsum("yxt,ntc->yxnc", w, sets.astype(np.int64))
    return ((s + 512) >> 10).astype(np.uint8)


def run_blend(fa, form, sets, m):
    x = np.zeros(sets.shape[:2] + (4,), np.uint8)
    x[:, :, :3] = sets                                               # RGBX, X = 0 as the undistortion writes it
    taps = np.ascontiguousarray(x).view(np.uint32).reshape(-1, 4)
    out = np.empty((32, 32, sets.shape[0], 3), np.uint8)
    fa.fa_blend_all(form, taps.ctypes.data, sets.shape[0], m, out.ctypes.data)
    return out


@pytest.mark.parametrize("form", [0, 1], ids=["int24", "fp32"])
def test_blend_is_the_integer_blend(fa, form):
    sets = tap_sets(2000, 5)
    assert sets.shape[0] == 2401 + 2000
    got, want = run_blend(fa, form, sets, 15), blend_reference(sets, 15)
    assert int((got != want).sum()) == 0
    # taps outside the frame: every pattern, on the extremes' corners and a slice of the random sets
    some = np.concatenate([sets[:2401:7], sets[2401:2401 + 300]], axis=0)
    for m in range(15):
        got, want = run_blend(fa, form, some, m), blend_reference(some, m)
        assert int((got != want).sum()) == 0, "mask pattern %d" % m


@pytest.fixture(scope="module")
def all_rgb():
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.empty((4096, 4096, 3), np.uint8)
    rgb[..., 0] = (v & 255).reshape(4096, 4096)
    rgb[..., 1] = ((v >> 8) & 255).reshape(4096, 4096)
    rgb[..., 2] = (v >> 16).reshape(4096, 4096)
    return rgb


def run_lab_b(fa, rgb, tables, clamp):
    g, c, k = (np.ascontiguousarray(t) for t in tables)
    flat = np.ascontiguousarray(rgb).reshape(-1, 3)
    out = np.empty(flat.shape[0], np.uint8)
    fa.fa_lab_b(flat.ctypes.data, flat.shape[0], g.ctypes.data, c.ctypes.data, k.ctypes.data, clamp, out.ctypes.data)
    return out.reshape(rgb.shape[:-1])


def test_lab_b_of_every_rgb_triple(fa, oracle, all_rgb):
    tables = oracle.lab_tables()
    want = oracle.lab_b(all_rgb)
    for clamp in (0, 1):
        assert int((run_lab_b(fa, all_rgb, tables, clamp) != want).sum()) == 0, "clamp=%d" % clamp


def lab_b_numpy(rgb, tables):
    g, c, k = tables
    k = k.astype(np.int64)
    R, G, B = (g[rgb[..., i]].astype(np.int64) for i in range(3))
    iy = np.minimum((R * k[3] + G * k[4] + B * k[5] + 2048) >> 12, 3071)
    iz = np.minimum((R * k[6] + G * k[7] + B * k[8] + 2048) >> 12, 3071)
    v = (200 * (c[iy].astype(np.int64) - c[iz].astype(np.int64)) + 128 * (1 << 15) + (1 << 14)) >> 15
    return np.clip(v, 0, 255).astype(np.uint8), np.maximum(iy, iz)


def test_clamp_elision_predicate(fa, oracle):
    g, c, k = oracle.lab_tables()
    gmax = int(g.max())
    assert gmax == 2040
    assert fa.fa_lab_clamp_is_dead(gmax, k.ctypes.data) == 1
    # a made-up matrix whose Y row sums to 7000: (2040 * 7000 + 2048) >> 12 = 3486 > 3071
    bad = k.copy()
    bad[3:6] = (3000, 3000, 1000)
    assert fa.fa_lab_clamp_is_dead(gmax, bad.ctypes.data) == 0
    neg = k.copy()
    neg[7] = -1
    assert fa.fa_lab_clamp_is_dead(gmax, neg.ctypes.data) == 0
    # ... and the clamped form is still exact for it, on triples that reach the clamp (bright ones) among others
    rng = np.random.default_rng(9)
    rgb = np.concatenate([rng.integers(200, 256, (60000, 3), dtype=np.uint8), rng.integers(0, 256, (60000, 3), dtype=np.uint8),
                          np.array([[255, 255, 255], [255, 255, 0], [0, 255, 255]], np.uint8)], axis=0)
    want, top = lab_b_numpy(rgb, (g, c, bad))
    unclamped = (g[rgb[:, 0]].astype(np.int64) * 3000 + g[rgb[:, 1]].astype(np.int64) * 3000 + g[rgb[:, 2]].astype(np.int64) * 1000 + 2048) >> 12
    assert int((unclamped > 3071).sum()) > 1000 and int(top.max()) == 3071
    assert int((run_lab_b(fa, rgb[None], (g, c, bad), 1)[0] != want).sum()) == 0
    # the same reference agrees with the oracle on the shipped tables
    assert np.array_equal(lab_b_numpy(rgb, (g, c, k))[0], oracle.lab_b(rgb[None])[0])
