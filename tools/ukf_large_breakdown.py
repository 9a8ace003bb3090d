#!/usr/bin/env python3
"""Steady-state kernel time per callback of the large-state UKF chain from a rocprofv3 kernel trace of tools/ukf_large_rate.py:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ukfl -- python tools/ukf_large_rate.py --landmarks 512 --batches 64 --steps 20 --no-oracle
    python tools/ukf_large_breakdown.py DIR/.../ukfl_kernel_trace.csv [launches_per_callback=76] [callbacks=20]

The stats file of such a run covers the warm-up replay too (smaller states); this takes the last `callbacks` callbacks only
(profiles/ukf_large_steady_breakdown.txt)."""
import collections
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows = [r for r in rows if "aslam::" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
per_cb = int(sys.argv[2]) if len(sys.argv) > 2 else 76
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
last = rows[-per_cb * steps:]
assert "frontend" in last[0]["Kernel_Name"], last[0]["Kernel_Name"]
acc = collections.OrderedDict()
for r in last:
    k = r["Kernel_Name"].split("(")[0].replace("void ", "")
    a = acc.setdefault(k, [0, 0])
    a[0] += 1
    a[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
tot = sum(v[1] for v in acc.values())
span = int(last[-1]["End_Timestamp"]) - int(last[0]["Start_Timestamp"])
print(f"steady state: last {steps} callbacks of the run ({per_cb} launches each); kernel time {tot/steps/1e6:.3f} ms per callback, span {span/steps/1e6:.3f} ms per callback")
for k, (c, ns) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
    print(f"{k:50s} calls/callback {c/steps:5.1f}  ms/callback {ns/steps/1e6:8.3f}  share {100*ns/tot:5.1f} %")
# the three products separately (in launch order: P, S+, Tc)
w = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in last if "ukf_large_wabt" in r["Kernel_Name"]]
for i, name in enumerate(("P = D W D^T + Q", "S+ = DZ W DZ^T + R", "Tc = D W DZ^T")):
    print(f"ukf_large_wabt {name:22s} ms/launch {sum(w[i::3])/len(w[i::3])/1e6:.3f}")
