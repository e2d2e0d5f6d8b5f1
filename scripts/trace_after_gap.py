#!/usr/bin/env python3
"""The dispatches of a rocprofv3 --kernel-trace CSV that follow its longest idle gap (scripts/verify_mode_times.py --trace pauses
between the prove and the verification), in start order: time, start relative to the first of them, grid. Then the totals.
--last-gap-ms G: cut at the LAST idle gap longer than G ms instead (a longer idle stretch comes earlier, e.g. while
scripts/verify_batch_times.py --trace synthesises its witnesses).
Usage: trace_after_gap.py <kernel_trace.csv> [--last-gap-ms G]"""
import csv
import sys

rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
ts = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows]
last_gap = float(sys.argv[3]) * 1e6 if len(sys.argv) > 3 and sys.argv[2] == "--last-gap-ms" else None
cut, gap, busy_until = 0, -1, ts[0][1]
for i in range(1, len(ts)):
    g = ts[i][0] - busy_until
    if (last_gap is None and g > gap) or (last_gap is not None and g > last_gap):
        cut, gap = i, g
    busy_until = max(busy_until, ts[i][1])
sel = rows[cut:]
t0 = int(sel[0]["Start_Timestamp"])
print(f"{len(sel)} dispatches after a {gap / 1e6:.1f} ms gap ({cut} before it)")
print(f"{'kernel':40s} {'time us':>9s} {'at us':>9s}   grid")
busy = 0.0
for r in sel:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    busy += (e - s) / 1e3
    name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").split("::")[-1].split("<")[0]
    grid = "x".join(r.get(f"Grid_Size_{d}", r.get(f"Grid_{d}", "?")) for d in "XYZ")
    print(f"{name:40s} {(e - s) / 1e3:9.1f} {(s - t0) / 1e3:9.1f}   {grid}")
end = max(int(r["End_Timestamp"]) for r in sel)
print(f"span {(end - t0) / 1e3:.1f} us, kernel time {busy:.1f} us")
