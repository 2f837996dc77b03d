"""The device sinks' RGB -> YUV 4:2:0 arithmetic (lane_tracker_amd/csrc/sink_arith.h) on the CPU: tests/sink_arith_host.cpp is the
same header compiled with the system C++ compiler, so these are the very expressions k_sink.hip runs.

  formulas    all 2^24 colours against the NumPy restatement (tests/sink_reference.py), for bt601, bt709 and a matrix whose
              clamps act at both ends -- zero mismatches
  round trip  the existing inverse (tests/yuv_reference.convert_triples) brings every colour back within 2 / 1 / 2 levels
  matrices    the BT.709 integers are round(c * 2^20); both matrices stay within one level of their float formula
  limits      coefficient sets at and just past both limits, through the host-only validation
  OpenCV      cross-check where cv2 imports; until then: UNVERIFIED vs OpenCV"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import sink_reference as S
import yuv_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no C++ compiler")


@pytest.fixture(scope="module")
def sa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sink_arith") / "libsink_arith_host.so")
    subprocess.check_call([CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", os.path.join(ROOT, "lane_tracker_amd", "csrc"),
                           os.path.join(ROOT, "tests", "sink_arith_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.sa_forward.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.sa_forward.restype = None
    lib.sa_coeffs_ok.argtypes = [C.c_void_p]
    lib.sa_coeffs_ok.restype = C.c_int
    lib.sa_matrix.argtypes = [C.c_int, C.c_void_p]
    lib.sa_matrix.restype = None
    return lib


@pytest.fixture(scope="module")
def colours():
    r, g, b = S.all_colours()
    return r, g, b, np.ascontiguousarray(np.stack([r, g, b], -1).astype(np.uint8))


def host_forward(sa, rgb_u8, matrix):
    k = np.array(S.coeffs(matrix), np.int32)
    out = np.empty_like(rgb_u8)
    sa.sa_forward(rgb_u8.ctypes.data, rgb_u8.shape[0], k.ctypes.data, out.ctypes.data)
    return out


def header_matrix(sa, which):
    k = np.zeros(8, np.int32)
    sa.sa_matrix(which, k.ctypes.data)
    return tuple(int(v) for v in k)


@pytest.mark.parametrize("matrix", ["bt601", "bt709", S.CLAMPING], ids=["bt601", "bt709", "clamping"])
def test_header_equals_the_restatement_on_all_colours(sa, colours, matrix):
    r, g, b, rgb = colours
    got = host_forward(sa, rgb, matrix)
    want = np.stack(S.forward_triples(r, g, b, matrix), -1)
    assert np.array_equal(got, want)
    if matrix is S.CLAMPING:             # the clamps act at both ends of every component
        assert sa.sa_coeffs_ok(np.array(matrix, np.int32).ctypes.data) == 1
        for ch in range(3):
            assert want[:, ch].min() == 0 and want[:, ch].max() == 255
        cry, cgy, cby, cru, cgu, cbu, cgv, cbv = matrix
        raw = lambda c, r_, g_, b_, off: (c[0] * r_ + c[1] * g_ + c[2] * b_ + (1 << 19) + (off << 20)) >> 20
        assert raw((cry, cgy, cby), 255, 255, 0, 16) > 255 and raw((cry, cgy, cby), 0, 0, 255, 16) < 0
        assert raw((cru, cgu, cbu), 255, 255, 0, 128) < 0 and raw((cru, cgu, cbu), 0, 0, 255, 128) > 255
        assert raw((cbu, cgv, cbv), 0, 255, 0, 128) < 0 and raw((cbu, cgv, cbv), 255, 0, 255, 128) > 255


def test_header_matrices_are_the_documented_ones(sa):
    assert header_matrix(sa, 0) == S.MATRICES["bt601"]
    assert header_matrix(sa, 1) == S.MATRICES["bt709"]
    assert S.MATRICES["bt709"] == tuple(int(round(c * (1 << 20))) for c in S.FLOAT_MATRICES["bt709"])
    from lane_tracker_amd import _native
    assert {k: tuple(v) for k, v in _native.RGB2YUV_MATRICES.items()} == S.MATRICES
    text = open(os.path.join(ROOT, "include", "lane_tracker_amd.h")).read()
    for name, m in (("LT_RGB2YUV_BT601", "bt601"), ("LT_RGB2YUV_BT709", "bt709")):
        assert "#define %s {%s}" % (name, ", ".join(str(v) for v in S.MATRICES[m])) in text


@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_ranges_and_float_formula(colours, matrix):
    r, g, b, _ = colours
    y, u, v = S.forward_triples(r, g, b, matrix)
    assert (y.min(), y.max()) == (16, 235) and (u.min(), u.max()) == (16, 240) and (v.min(), v.max()) == (16, 240)
    c = S.FLOAT_MATRICES[matrix]
    fy = 16 + c[0] * r + c[1] * g + c[2] * b
    fu = 128 + c[3] * r + c[4] * g + c[5] * b
    fv = 128 + c[5] * r + c[6] * g + c[7] * b
    for got, want in ((y, fy), (u, fu), (v, fv)):
        assert np.abs(got - want).max() <= 1.0
    k = S.coeffs(matrix)                 # the validation's bound on every row, sum |c| * 255 + 2^19 + (128 << 20), is inside int32
    bound = max(sum(abs(c_) for c_ in row) * 255 + (1 << 19) + (128 << 20) for row in (k[0:3], k[3:6], k[5:8]))
    assert bound < 1 << 31
    if matrix == "bt601":
        assert bound == 369507001


def test_round_trip_through_the_existing_inverse(colours):
    r, g, b, rgb = colours
    y, u, v = S.forward_triples(r, g, b, "bt601")
    back = R.convert_triples(y, u, v, "bt601").astype(np.int64)
    err = np.abs(back - rgb.astype(np.int64)).max(0)
    print("round trip bt601, largest |error| per channel (R, G, B):", err.tolist())
    assert err[0] <= 2 and err[1] <= 1 and err[2] <= 2


def test_validation_limits(sa):
    ok = lambda k: sa.sa_coeffs_ok(np.array(k, np.int32).ctypes.data) == 1
    lim = 1 << 23
    assert ok(S.MATRICES["bt601"]) and ok(S.MATRICES["bt709"]) and ok(S.CLAMPING) and ok((0,) * 8)
    # row sums: sum |c| * 255 + 2^19 + (128 << 20) <= 2^31 - 1  <=>  sum |c| <= 7893104.  That is below 2^23, so the row rule is
    # the one that binds: a lone coefficient is taken up to `top`, and both 2^23 - 1 and 2^23 are refused, either sign
    top = ((1 << 31) - 1 - (1 << 19) - (128 << 20)) // 255
    assert top * 255 + (1 << 19) + (128 << 20) <= (1 << 31) - 1 < (top + 1) * 255 + (1 << 19) + (128 << 20) and top < lim
    for i in range(8):
        for sign in (1, -1):
            for value, verdict in ((top, True), (top + 1, False), (lim - 1, False), (lim, False)):
                k = [0] * 8
                k[i] = sign * value
                assert ok(k) == verdict, (i, sign, value)
    a, b_ = top // 2, top - top // 2
    for at in ((0, 1), (3, 4), (6, 7)):  # the Y, U and V rows (V shares CBU = k[5], left at 0 here)
        for signs in ((1, 1), (-1, -1), (1, -1)):
            k = [0] * 8
            k[at[0]], k[at[1]] = signs[0] * a, signs[1] * b_
            assert ok(k), (at, signs)
            k[at[1]] += signs[1]
            assert not ok(k), (at, signs)
    k = [0] * 8                          # CBU counts in both chroma rows
    k[5], k[6] = a, -b_
    assert ok(k)
    k[5] += 1
    assert not ok(k)


def test_restatement_is_opencv():
    cv2 = None
    try:
        import cv2
    except Exception:
        print("UNVERIFIED vs OpenCV (cv2 absent)")
    cv2 = pytest.importorskip("cv2")
    rgb = np.random.default_rng(11).integers(0, 256, (720, 1280, 3), dtype=np.uint8)
    assert np.array_equal(S.rgb_to_yuv420(rgb, "i420", "bt601"), cv2.cvtColor(rgb, cv2.COLOR_RGB2YUV_I420))
