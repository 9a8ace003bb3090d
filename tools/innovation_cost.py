#!/usr/bin/env python3
"""What the innovation statistics cost: aslam_replay against aslam_replay_stats (all three arrays) on the same context, timed with device
events, at bench.py's three shapes (ekf512: 256 filters, fp32 products; ekf64, ukf64: 256 filters, fp64) and at the large-state UKF shape
(256 landmarks, 64 filters).  Prints one JSON record per shape: ms per launch both ways, the ratio, launches per callback both ways.

    python tools/innovation_cost.py [--reps 5] [--shapes ekf512,ekf64,ukf64,ukf256] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROLOGUE = 64  # bench.py: the warm-up in which the state grows to its full dimension
SHAPES = {
    # name: (filter, landmarks, batch, callbacks per launch, binary32 products, large-state UKF)
    "ekf512": ("ekf", 512, 256, 20, True, False),
    "ekf64": ("ekf", 64, 256, 500, False, False),
    "ukf64": ("ukf", 64, 256, 200, False, False),
    "ukf256": ("ukf", 256, 64, 4, False, True),
}


def measure(name, reps):
    import numpy as np
    import torch
    from awesomeslam_amd import trace as tg
    from awesomeslam_amd.core import CFG_UKF_LARGE, Core, F32, F64

    kind, L, B, C, f32, ukf_large = SHAPES[name]
    T = PROLOGUE + (2 * reps + 2) * C
    tr = tg.make_traces(L, T, B=B, seed=1)
    large = f32 or ukf_large
    core = Core(kind, tg.dim_cap(L), batch=B, max_obs=tr.max_obs, max_wait=min(2048 if large else 512, 2 * L + 64), dtype=F32 if f32 else F64,
                flags=CFG_UKF_LARGE if ukf_large else 0)
    core.set_trace(tr)
    del tr
    dev = "cuda"
    poses = torch.zeros((B, max(C, PROLOGUE), 3), dtype=torch.float64, device=dev)
    nis = torch.zeros((B, C), dtype=torch.float64, device=dev)
    logdet = torch.zeros((B, C), dtype=torch.float64, device=dev)
    pcov = torch.zeros((B, C, 6), dtype=torch.float64, device=dev)
    core.replay(0, PROLOGUE, poses.data_ptr(), None)
    torch.cuda.synchronize()
    assert core.dim(0) == tg.full_dim(L) and core.status(0) == 0, (core.dim(0), core.status(0))
    t = PROLOGUE
    ms = {"replay": [], "replay_stats": []}
    launches = {}
    # one untimed launch each way first, then alternate: both see the same drift of clocks and of the trajectory
    for rep in range(-1, reps):
        for how in ("replay", "replay_stats"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if how == "replay":
                core.replay(t, C, poses.data_ptr(), None)
            else:
                core.replay_stats(t, C, poses.data_ptr(), None, nis.data_ptr(), logdet.data_ptr(), pcov.data_ptr())
            b.record()
            torch.cuda.synchronize()
            launches[how] = core.launch_info()["launches_per_callback"]
            if rep >= 0:
                ms[how].append(a.elapsed_time(b))
            t += C
    assert core.status(0) == 0 and bool(torch.isfinite(nis).all()) and bool(torch.isfinite(logdet).all())
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rec = {"shape": name, "filter": kind, "landmarks": L, "state_dim": tg.full_dim(L), "batch": B, "callbacks_per_launch": C, "reps": reps,
           "kernel": core.kernel_info()["name"], "ms_per_launch": med, "ms_all": ms,
           "stats_over_plain": med["replay_stats"] / med["replay"],
           "us_per_callback_added": (med["replay_stats"] - med["replay"]) * 1e3 / C,
           "launches_per_callback": launches}
    core.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    recs = []
    for name in args.shapes.split(","):
        rec = measure(name, args.reps)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
