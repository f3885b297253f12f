#!/usr/bin/env python3
"""Sum rocprofv3 --pmc counter CSVs (all dispatches, all instances) per counter name.
    python3 tools/pmc_summary.py [--by-kernel] <glob>...
--by-kernel: one block per kernel name, each counter as its mean per dispatch."""
import collections, csv, glob, sys

args = sys.argv[1:]
by_kernel = "--by-kernel" in args
args = [a for a in args if a != "--by-kernel"]
tot = collections.defaultdict(float)
disp = collections.defaultdict(set)
for pat in args:
    for f in glob.glob(pat, recursive=True):
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"] if by_kernel else ""
            tot[(k, r["Counter_Name"])] += float(r["Counter_Value"])
            disp[(k, r["Counter_Name"])].add((f, r["Dispatch_Id"]))
last = None
for k, c in sorted(tot):
    if by_kernel and k != last:
        print(f"== {k[:150]}")
        last = k
    v = tot[(k, c)] / len(disp[(k, c)]) if by_kernel else tot[(k, c)]
    print(f"{c:34s} {v:18.0f}" + (f"  (mean of {len(disp[(k, c)])} dispatches)" if by_kernel else ""))
