#!/usr/bin/env python3
"""Per-kernel instruction streams of a gfx950 assembly listing (hipcc -S --cuda-device-only), and the counts the front end's
instruction budget is stated in (tests/test_isa_guards.py holds the undistortion walks to them).

    tools/isa_split.py FILE.s [FILE.s ...] [--match SUBSTRING]

prints, per kernel: a hash of the instruction stream, instructions, v_mul_lo_u32, vector-memory instructions, scalar loads,
scratch instructions, SGPRs, VGPRs, and the VALU instructions inside the innermost loop that stores through a buffer
resource (the per-frame loop of the undistortion walks; '-' where a kernel has none)."""
import hashlib
import re
import sys

VMEM = re.compile(r"^(buffer_|global_|flat_|scratch_)")


def kernels(text):
    """mangled name -> {'insts': [instruction or 'label:'], 'sgpr': int, 'vgpr': int}; comments and directives dropped."""
    out, cur, last = {}, None, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = last = out[m.group(1)] = {"insts": [], "sgpr": None, "vgpr": None}
            continue
        m = re.match(r"^; (?:TotalNum|Num)([SV])gprs: (\d+)", line)      # the register summary follows the kernel descriptor
        if m and last is not None:
            last["sgpr" if m.group(1) == "S" else "vgpr"] = int(m.group(2))
        if cur is None:
            continue
        s = line.split(";")[0].strip()
        if s.startswith(".end_amdhsa_kernel"):
            cur = None
        elif s and (not s.startswith(".") or re.match(r"^\.LBB\w+:$", s)):
            cur["insts"].append(re.sub(r"\s+", " ", s))
    return out


def kernel_name(mangled):
    """k_name or k_name<true / false / N, ...> of an Itanium-mangled kernel symbol (the project's kernels are all named k_*, with bool
    and int template arguments only: k_undistort_rows<5, 1, false>); the symbol itself where that does not fit.  (No demangler is called: ROCm's llvm/bin has
    none, and a guard test should not hang on binutils being installed.)"""
    m = re.search(r"(?:_GLOBAL__N_1)?(\d+)k_", mangled)
    if not m:
        return mangled
    # (the length prefix follows the anonymous namespace's "_GLOBAL__N_1", whose own 1 is not part of it -- a long symbol can have an 'E' at
    # that distance too; elsewhere: take the digits that make the name end at 'E' / 'I')
    start, digits = m.end(1), m.group(1)
    n = next((int(digits[i:]) for i in range(len(digits)) if mangled[start + int(digits[i:]):start + int(digits[i:]) + 1] in ("E", "I")), None)
    if n is None:
        return mangled
    name, rest = mangled[start:start + n], mangled[start + n:]
    t = re.match(r"I((?:L[bi]\d+E)+)E", rest)
    if t:
        name += "<%s>" % ", ".join(("false", "true")[int(v)] if c == "b" else v for c, v in re.findall(r"L([bi])(\d+)E", t.group(1)))
    elif rest.startswith("I"):
        return mangled
    return name


def store_loop(insts):
    """The instructions of the innermost loop (label ... backward branch to it) that holds a buffer store, or None."""
    pos = {s[:-1]: i for i, s in enumerate(insts) if s.endswith(":")}
    best = None
    for i, s in enumerate(insts):
        m = re.match(r"s_cbranch_\w+ (\.LBB\w+)$", s) or re.match(r"s_branch (\.LBB\w+)$", s)
        if m and m.group(1) in pos and pos[m.group(1)] < i:
            body = insts[pos[m.group(1)]:i + 1]
            if any(b.startswith("buffer_store") for b in body) and (best is None or len(body) < len(best)):
                best = body
    return best


def stats(k):
    ins = [s for s in k["insts"] if not s.endswith(":")]
    loop = store_loop(k["insts"])
    return {
        "hash": hashlib.sha1("\n".join(ins).encode()).hexdigest()[:12],
        "insts": len(ins),
        "mul_lo": sum(s.startswith("v_mul_lo_u32") for s in ins),
        "vmem": sum(bool(VMEM.match(s)) for s in ins),
        "sload": sum(s.startswith("s_load_") or s.startswith("s_buffer_load_") for s in ins),
        "scratch": sum(s.startswith("scratch_") for s in ins),
        "sgpr": k["sgpr"],
        "vgpr": k["vgpr"],
        "loop_valu": None if loop is None else sum(s.startswith("v_") for s in loop),
    }


def table(text, match=""):
    ks = kernels(text)
    return {kernel_name(n): stats(k) for n, k in ks.items() if match in kernel_name(n)}


if __name__ == "__main__":
    args = sys.argv[1:]
    match = args.pop(args.index("--match") + 1) if "--match" in args else ""
    cols = ["hash", "insts", "mul_lo", "vmem", "sload", "scratch", "sgpr", "vgpr", "loop_valu"]
    for p in [a for a in args if a != "--match"]:
        print("# %s\n# %s  kernel" % (p, " ".join(cols)))
        for name, st in table(open(p).read(), match).items():
            print(" ".join("-" if st[c] is None else str(st[c]) for c in cols), name)
