#!/usr/bin/env python3
"""What the Mahalanobis gate inside the replay seam (aslam_set_replay_gate) costs -- numbers to record, not targets, and not part of bench.py.

Three shapes: the single-CU EKF at 64 landmarks (n = 131) with 256 filters, and the large-state EKF at 512 landmarks (n = 1027), binary32
products, with 256 filters and with 1.  Each runs one trajectory in every filter with the default parameters.  The map is grown with the
gate off, that state is kept as a device snapshot, and then, alternating in ONE process and ONE context, `--reps` rounds of

    restore the snapshot -> every gate 0    -> device-event time of one aslam_replay over --steps callbacks
    restore the snapshot -> every gate 9.21 -> the same replay

after one untimed round of both.  With every gate at 0 the context launches the ungated kernels, with 9.21 the GATED instantiations: the ratio
is that of the two front ends, on the same trace and the same state.  Per shape one JSON line: the time per callback (us, the whole batch) of
every round, the medians, the spread (max - min) / median of each setting, the ratio on / off of the medians, and what the gate decided.

    python tools/gated_replay_rate.py [--steps 24] [--reps 5] [--shape NAME] [--out profiles/gated_replay.json] [--md profiles/gated_replay.md]
                                      [--frontend-stats DIR] [--build-seconds BEFORE AFTER]

--frontend-stats: a directory with the kernel trace (CSV) of a SEPARATE run of this tool under a kernel-trace profiler; the mean duration
of the large-state front-end launches over the measured window, gate 0 against 9.21, is read from it into the record.  --build-seconds: wall seconds of a full
build of libaslam_core.so before and with the gated instantiations, measured by whoever runs the tool.
There is no CPU fallback: without a GPU the tool fails."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("ekf64_single_cu_b256", 64, 256, "f64"), ("ekf512_f32_b256", 512, 256, "f32"), ("ekf512_f32_b1", 512, 1, "f32"))
WARM = 42  # the three growth stages of make_traces end here
GATE = 9.21


def measure(name, L, B, dtype, steps, reps):
    import numpy as np
    import torch

    from awesomeslam_amd import trace as tg
    from awesomeslam_amd.core import Core, F32, F64

    tr = tg.make_traces(L, WARM + steps, B=1, seed=71).select([0] * B)
    core = Core("ekf", tg.dim_cap(L), batch=B, max_obs=tr.max_obs, max_wait=2048 if L > 64 else 256, dtype=F32 if dtype == "f32" else F64)
    core.set_trace(tr)
    core.replay(0, WARM)
    torch.cuda.synchronize()
    n = core.dim(0)
    blob = torch.empty(core.snapshot_bytes(), dtype=torch.uint8, device="cuda")
    core.snapshot(out=blob)
    torch.cuda.synchronize()
    slots = list(range(B))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us, kernels, status, dims, rejected, lds = {0.0: [], GATE: []}, {}, {}, {}, {}, {}
    for rep in range(-1, reps):
        for g in (0.0, GATE):
            core.restore(blob, slots, slots)
            core.set_replay_gate(g)
            torch.cuda.synchronize()
            e0.record()
            core.replay(WARM, steps)
            e1.record()
            torch.cuda.synchronize()
            status[g] = sorted({core.status(b) for b in (0, B - 1)})
            dims[g], rejected[g] = core.dim(B - 1), core.assoc_rejected(B - 1)
            info = core.kernel_info()
            kernels[g], lds[g] = info["name"], info["lds_bytes"]
            if rep >= 0:
                us[g].append(e0.elapsed_time(e1) * 1e3 / steps)
    med = {g: float(np.median(v)) for g, v in us.items()}
    rec = {"workload": name, "landmarks": L, "n_at_start": n, "batch": B, "dtype": dtype, "steps": steps, "reps": reps, "gate": GATE,
           "observations_per_callback": int(tr.n_obs[0, WARM:].mean()),
           "us_per_callback_off": us[0.0], "us_per_callback_on": us[GATE], "median_off": med[0.0], "median_on": med[GATE],
           "spread_off": (max(us[0.0]) - min(us[0.0])) / med[0.0], "spread_on": (max(us[GATE]) - min(us[GATE])) / med[GATE],
           "time_ratio_on_over_off": med[GATE] / med[0.0], "us_per_callback_added": med[GATE] - med[0.0],
           "n_end_off": dims[0.0], "n_end_on": dims[GATE], "rejected_on": rejected[GATE], "rejected_off": rejected[0.0],
           "status_bits_off": status[0.0], "status_bits_on": status[GATE], "kernel_off": kernels[0.0], "kernel_on": kernels[GATE],
           "lds_bytes_off": lds[0.0], "lds_bytes_on": lds[GATE], "launches_per_callback": core.launch_info()["launches_per_callback"],
           "timing": "device events around one aslam_replay, alternating gate 0 / 9.21 in one process and one context, measured"}
    core.close()
    return rec


def frontend_stats(directory):
    """Mean duration (us) of the large-state front-end launches, gated and ungated, over the SAME window, from the kernel trace (CSV) a profiler
    left under `directory` of a run of this tool.  Such a run launches the ungated front end for the warm-up and then for as many callbacks as
    the gated one (the rounds alternate), so the window's ungated launches are the last len(gated) of them in time: like for like."""
    launches = {"gated": [], "ungated": []}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace*.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name") or row.get("KernelName") or ""
                if "large_frontend_kernel" not in name:
                    continue
                t0, t1 = float(row["Start_Timestamp"]), float(row["End_Timestamp"])
                key = "gated" if name.split("(")[0].rstrip().rstrip(">").rstrip().endswith("true") else "ungated"
                launches[key].append((t0, t1 - t0))
    k = len(launches["gated"])
    if k == 0 or len(launches["ungated"]) < k:
        return {}
    window = {"gated": launches["gated"], "ungated": sorted(launches["ungated"])[-k:]}
    return {key: {"calls": len(v), "mean_us": sum(d for _, d in v) / len(v) / 1e3} for key, v in window.items()}


def markdown(lines, extra):
    md = ["# The gate inside the replay seam: what it costs", "",
          "Written by `tools/gated_replay_rate.py` on an MI355X; numbers to record, not targets.  Time per callback of the whole batch (device events",
          "around one `aslam_replay`), gate 0 (the ungated kernels) against gate 9.21 (the GATED instantiations) in every filter, alternating in one",
          "context on the same trace and the same restored state; default parameters.", "",
          "| shape | n | filters | obs / callback | us / callback off | on | spread off / on | on / off | added us |", "|---|---|---|---|---|---|---|---|---|"]
    for r in lines:
        md.append(f"| {r['workload']} | {r['n_at_start']} | {r['batch']} | {r['observations_per_callback']} | {r['median_off']:.1f} | {r['median_on']:.1f} | "
                  f"{r['spread_off']:.3f} / {r['spread_on']:.3f} | {r['time_ratio_on_over_off']:.3f} | {r['us_per_callback_added']:.1f} |")
    md.append("")
    for r in lines:
        md.append(f"- `{r['workload']}`: `{r['kernel_on']}`, {r['lds_bytes_on']} bytes of LDS ({r['lds_bytes_off']} ungated); the gate dropped {r['rejected_on']} observations of the last filter.")
    if extra.get("frontend"):
        md += ["", "Front-end launch of the large-state chain, from the kernel trace of a separate profiling run: mean over the launches of the same",
               "window of callbacks, gate 0 against 9.21 (the warm-up launches are left out):", ""]
        md += [f"- {k}: {v['mean_us']:.1f} us over {v['calls']} launches" for k, v in sorted(extra["frontend"].items())]
    if extra.get("build_seconds"):
        b, a = extra["build_seconds"]
        md += ["", f"A full build of `libaslam_core.so` (both translation units, guards included) took {b:.0f} s before the gated instantiations and {a:.0f} s with them."]
    return "\n".join(md) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default=None, choices=[s[0] for s in SHAPES])
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--frontend-stats", default=None)
    ap.add_argument("--build-seconds", type=float, nargs=2, default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("gated_replay_rate: no GPU (there is no CPU fallback)")
    lines = []
    for name, L, B, dtype in SHAPES:
        if a.shape in (None, name):
            lines.append(measure(name, L, B, dtype, a.steps, a.reps))
            print(json.dumps(lines[-1]), flush=True)
    extra = {}
    if a.frontend_stats:
        extra["frontend"] = frontend_stats(a.frontend_stats)
    if a.build_seconds:
        extra["build_seconds"] = a.build_seconds
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
            if extra:
                f.write(json.dumps({"extra": extra}) + "\n")
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(lines, extra))


if __name__ == "__main__":
    main()
