#!/usr/bin/env python3
"""What the sighted-only EKF update (aslam_sighted_update_enable) costs -- numbers to record, not targets, and not part of bench.py.

Two shapes: the single-CU EKF at 64 landmarks (n = 131) with 64 filters, and the large-state EKF at 512 landmarks (n = 1027), binary32
products, 256 filters.  Each runs one trajectory in every filter, on a trace whose sensor range is cut (trace.limit_range) to the median
range behind the warm-up, so that about half the landmarks are in view.  The map is grown with the mode off, that state is kept as a device
snapshot, and then, alternating in ONE process, `--reps` rounds of

    restore the snapshot -> mode off -> device-event time of one aslam_replay over --steps callbacks
    restore the snapshot -> mode on  -> the same replay

after one untimed round of both.  Per shape one JSON line: the filter-steps/s of every round, their medians, the spread (max - min) / median
of each mode and the ratio on / off of the medians.

    python tools/sighted_rate.py [--steps 24] [--reps 5] [--out profiles/sighted_rate.json]

There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("ekf64_single_cu", 64, 64, "f64"), ("ekf512_f32", 512, 256, "f32"))
WARM = 42  # the three growth stages of make_traces end here


def measure(name, L, B, dtype, steps, reps):
    import numpy as np
    import torch

    from awesomeslam_amd import trace as tg
    from awesomeslam_amd.core import Core, F32, F64

    full = tg.make_traces(L, WARM + steps, B=1, seed=71)
    seen = full.obs[0, WARM:, :, 0]
    r = float(np.median(seen[seen > 0]))
    tr = tg.limit_range(full, r, WARM).select([0] * B)
    core = Core("ekf", tg.dim_cap(L), batch=B, max_obs=tr.max_obs, max_wait=2048 if L > 64 else 256, dtype=F32 if dtype == "f32" else F64)
    core.set_trace(tr)
    core.replay(0, WARM)
    torch.cuda.synchronize()
    n = core.dim(0)
    assert n == tg.full_dim(L), (n, tg.full_dim(L))
    blob = torch.empty(core.snapshot_bytes(), dtype=torch.uint8, device="cuda")
    core.snapshot(out=blob)
    torch.cuda.synchronize()
    slots = list(range(B))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rates, kernels, status, in_view = {False: [], True: []}, {}, {}, None
    for rep in range(-1, reps):
        for on in (False, True):
            core.restore(blob, slots, slots)
            core.sighted_only(on)
            torch.cuda.synchronize()
            e0.record()
            core.replay(WARM, steps)
            e1.record()
            torch.cuda.synchronize()
            status[on] = sorted({core.status(b) for b in (0, B - 1)})
            assert core.dim(B - 1) == n, (name, on, core.dim(B - 1), n)
            kernels[on] = core.kernel_info()["name"]
            in_view = float(core.sighted(0).mean())
            if rep >= 0:
                rates[on].append(B * steps / (e0.elapsed_time(e1) * 1e-3))
    med = {on: float(np.median(v)) for on, v in rates.items()}
    rec = {"workload": name, "landmarks": L, "n": n, "batch": B, "dtype": dtype, "steps": steps, "reps": reps, "sensor_range_m": r,
           "sighted_fraction_last_callback": in_view,
           "filter_steps_per_s_off": rates[False], "filter_steps_per_s_on": rates[True],
           "median_off": med[False], "median_on": med[True],
           "spread_off": (max(rates[False]) - min(rates[False])) / med[False], "spread_on": (max(rates[True]) - min(rates[True])) / med[True],
           "time_ratio_on_over_off": med[False] / med[True],
           "status_bits_off": status[False], "status_bits_on": status[True],
           "kernel_off": kernels[False], "kernel_on": kernels[True], "launches_per_callback": core.launch_info()["launches_per_callback"],
           "timing": "device events around one aslam_replay, alternating off / on in one process, measured"}
    core.close()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("sighted_rate: no GPU (there is no CPU fallback)")
    lines = []
    for name, L, B, dtype in SHAPES:
        lines.append(measure(name, L, B, dtype, a.steps, a.reps))
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
