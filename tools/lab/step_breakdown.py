#!/usr/bin/env python3
"""Per-step kernel shares from a rocprofv3 kernel trace of bench.py: the dispatches between the
starts of the 2nd and the last advection launch, summed by kernel (sweep-loop kernels by grid size).
usage: step_breakdown.py <dir with *_kernel_trace.csv or *_results.db> [name of the once-per-step kernel]
(a rocprofv3 that writes its database by default: the same columns from the `kernels` view of *_results.db)"""
import collections
import csv
import glob
import sqlite3
import sys

f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)
mark = sys.argv[2] if len(sys.argv) > 2 else "advect3"
if f:
    rows = list(csv.DictReader(open(f[0])))
else:
    db = sqlite3.connect(glob.glob(sys.argv[1] + "/**/*_results.db", recursive=True)[0])
    cols = ("Kernel_Name", "Start_Timestamp", "End_Timestamp", "Grid_Size_X")
    rows = [dict(zip(cols, r)) for r in db.execute("select name, start, end, grid_x from kernels")]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
adv = [i for i, r in enumerate(rows) if mark in r["Kernel_Name"]]
if len(adv) < 3:
    sys.exit("fewer than 3 launches of %s" % mark)
a, b = adv[1], adv[min(len(adv) - 1, 5)]
ns = min(len(adv) - 1, 5) - 1
t0, t1 = int(rows[a]["Start_Timestamp"]), int(rows[b]["Start_Timestamp"])
print("%d steps, wall %.3f ms/step" % (ns, (t1 - t0) / ns / 1e6))
tot, cnt = collections.Counter(), collections.Counter()
for r in rows[a:b]:
    k = r["Kernel_Name"].split("(")[0][:64]
    if "loop_kernel" in r["Kernel_Name"] or "relax" in r["Kernel_Name"]:
        k += " g%s" % r["Grid_Size_X"]
    tot[k] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    cnt[k] += 1
print("busy %.3f ms/step" % (sum(tot.values()) / ns / 1e6))
for k, v in tot.most_common(40):
    print("%-80s %6.1f/step %8.1f us/step  avg %7.1f us" % (k, cnt[k] / ns, v / ns / 1e3, v / cnt[k] / 1e3))
