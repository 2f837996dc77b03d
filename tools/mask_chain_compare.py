#!/usr/bin/env python3
"""Two rocprofv3 kernel traces (CSV) of tools/mask_chain_routes.py, one per build of the library: are the launches the same?
Compares the ordered list of (kernel name, grid, workgroup, dynamic LDS) and prints a short report (what profiles/ keeps).

  mask_chain_compare.py PARENT_kernel_trace.csv NEW_kernel_trace.csv [label_parent label_new]
"""
import collections, csv, sys


def launches(path):
    rows = list(csv.DictReader(open(path, newline="")))
    key = "Dispatch_Id" if rows and "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[key]))
    dims = lambda r, what: "x".join(r.get("%s_%s" % (what, a), "?") for a in "XYZ")
    return [(r["Kernel_Name"], dims(r, "Grid_Size"), dims(r, "Workgroup_Size"), r.get("LDS_Block_Size", "?")) for r in rows]


def short(name):
    return name.replace("lt::(anonymous namespace)::", "").replace("void ", "").split("(")[0]


def main():
    a, b = launches(sys.argv[1]), launches(sys.argv[2])
    la, lb = (sys.argv[3], sys.argv[4]) if len(sys.argv) > 4 else ("parent", "new")
    print("launches: %s %d, %s %d" % (la, len(a), lb, len(b)))
    diff = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    same = len(a) == len(b) and not diff
    print("ordered list of (kernel, grid, workgroup, dynamic LDS): %s" % ("EQUAL" if same else "DIFFERENT"))
    for i in diff[:20]:
        print("  #%d  %s: %s   %s: %s" % (i, la, (short(a[i][0]),) + a[i][1:], lb, (short(b[i][0]),) + b[i][1:]))
    count = collections.Counter(short(x[0]) for x in b)
    print("kernels of %s, launches each:" % lb)
    for name, k in sorted(count.items()):
        print("  %5d  %s" % (k, name))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
