"""What a raw Bayer context is conditioned with, without a GPU: csrc/raw_setup.h -- the value the setters edit, the bytes a raw kernel stages
for it and what a launch is given -- compiled with the system compiler (tests/raw_setup_host.cpp), plain and under ASan / UBSan, for all
eight states (table x stage x map) of an 8-bit, a 10- and a 12-bit layout and of their MIPI-packed forms, against the Python definitions:
utils.raw_lut(bits=..) for the default table, the identity, the caller's table, the curve in front.  And that the walk of
tests/test_gpu_raw_setup_walk.py covers what it says it covers."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_gpu_raw_setup_walk as WALK
from lane_tracker_amd import _native, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
LAYOUTS = (("bayer_grbg", 8, -1), ("bayer10_grbg", 10, -1), ("bayer10p_bggr", 10, 0), ("bayer12_rggb", 12, -1), ("bayer12p_gbrg", 12, 1))


def staged_bytes(bits, table, curve, shaded):
    """What a raw kernel stages, from the Python definitions: nothing for 8-bit frames with nothing set; else the curve where there is a
    stage, then the caller's table, the 8-bit identity or the 10- / 12-bit default."""
    if bits == 8 and table is None and curve is None and not shaded:
        return b""
    default = np.tile(np.arange(256, dtype=np.uint8), (4, 1)) if bits == 8 else utils.raw_lut(bits=bits)
    assert default.shape == (4, 1 << bits) and default.dtype == np.uint8
    return (b"" if curve is None else curve.tobytes()) + (default if table is None else table).tobytes()


@pytest.mark.skipif(CXX is None, reason="no C++ compiler")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_staged_bytes_and_launch_fields_of_every_state(tmp_path, flags):
    exe = str(tmp_path / "raw_setup_host")
    subprocess.run([CXX, "-std=c++17", "-Wall", *flags, "-I", os.path.join(ROOT, "lane_tracker_amd", "csrc"), os.path.join(ROOT, "tests", "raw_setup_host.cpp"),
                    "-o", exe], check=True, capture_output=True, timeout=300)
    rng = np.random.default_rng(31)
    blob, cases = b"", 0
    for name, bits, pack in LAYOUTS:
        for table, stage, shaded in itertools.product((0, 1), repeat=3):
            lut = rng.integers(0, 256, (4, 1 << bits), dtype=np.uint8)
            ccm, curve = rng.integers(-32768, 32768, 9).astype("<i2"), rng.integers(0, 256, 256, dtype=np.uint8)
            black, mesh = rng.integers(0, 1 << bits, 4).astype("<i4"), rng.integers(0, 65536, (4, 2, 3)).astype("<u2")
            want = staged_bytes(bits, lut if table else None, curve if stage else None, bool(shaded))
            assert len(want) == (0 if bits == 8 and not (table or stage or shaded) else (256 if stage else 0) + (4 << bits))
            head = np.array([_native.pixel_format_id(name), table, stage, shaded, bits, pack, len(want)], "<i4")
            blob += head.tobytes() + lut.tobytes() + ccm.tobytes() + curve.tobytes() + black.tobytes() + mesh.tobytes() + want
            cases += 1
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        fh.write(blob)
    r = subprocess.run([exe, path], capture_output=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-900:])
    assert r.stdout.split() == [b"ok", b"%d" % cases] and cases == 8 * len(LAYOUTS)


def test_the_walk_covers_every_edge_and_every_replacement():
    walk, states = WALK.WALK, WALK.states()
    assert 36 <= len(walk) <= 44 and all(len(s) == 2 and s[0] in "TSM" and s[1] in "012" for s in walk)
    on = lambda s: tuple(int(v > 0) for v in s)
    edges, replaced = set(), set()
    for step, before, after in zip(walk, [(0, 0, 0)] + states[:-1], states):
        k = "TSM".index(step[0])
        assert all(before[i] == after[i] for i in range(3) if i != k)
        if on(before) != on(after):
            edges.add((on(before), on(after)))
        elif before[k] and before[k] != after[k] and all(after[i] for i in range(3) if i != k):
            replaced.add(step[0])
    cube = list(itertools.product((0, 1), repeat=3))
    assert edges == {(a, b) for a in cube for b in cube if sum(x != y for x, y in zip(a, b)) == 1} and len(edges) == 24
    assert replaced == set("TSM")
    assert states[-1] == (0, 0, 0)
