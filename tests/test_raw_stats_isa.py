"""The budget of the raw-statistics kernels -- k_raw_stats<ENC, BITS, SURF, SHADE> (k_raw_stats.hip), DESIGN.md section 4 -- on the generated
gfx950 code (hipcc cross-compiles; no GPU needed), through tools/isa_split.py like the other budget files: every one of them uses no scratch
memory and at most 65536 bytes of LDS.  Nothing else is pinned: nobody has tuned these kernels yet."""
import re

import pytest

import test_isa_guards as G

pytestmark = G.needs_hipcc

LDS_MAX = 65536
# (ENC, BITS) of stats_arith.h: bytes, 16-bit words at 10 / 12 bits, RAW10, RAW12; each from surfaces or staging, with or without a map
FORMS = [(0, 8), (1, 10), (1, 12), (2, 10), (3, 12)]
NAMES = sorted("k_raw_stats<%d, %d, %s, %s>" % (enc, bits, surf, shade) for enc, bits in FORMS for surf in ("false", "true") for shade in ("false", "true"))


def _listing():
    return G._isa(G.os.path.join(G.CSRC, "k_raw_stats.hip"))


def _descriptors(split, isa):
    """kernel name -> {directive: value} of its .amdhsa_kernel block."""
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", isa, flags=re.S):
        out[split.kernel_name(m.group(1))] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\b", m.group(2))}
    return out


def test_raw_stats_kernels_use_no_scratch_and_fit_the_lds():
    split, isa = G._isa_split(), _listing()
    table, desc = split.table(isa), _descriptors(split, isa)
    ours = sorted(n for n in table if "k_raw_stats" in n)
    assert ours == NAMES and len(ours) == 20, ours
    assert sorted(n for n in desc if "k_raw_stats" in n) == NAMES
    for n in ours:
        d = desc[n]
        print(n, table[n], d["group_segment_fixed_size"], d["private_segment_fixed_size"])
        assert table[n]["scratch"] == 0 and d["private_segment_fixed_size"] == 0, "%s uses scratch memory" % n
        assert 0 < d["group_segment_fixed_size"] <= LDS_MAX, "%s: %d bytes of LDS" % (n, d["group_segment_fixed_size"])
