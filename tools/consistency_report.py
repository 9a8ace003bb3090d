#!/usr/bin/env python3
"""Monte-Carlo consistency of the filters on synthetic traces with ground truth: a batch of seeded trajectories per filter kind and landmark
count is replayed with aslam_replay_stats, and the statistics are reduced the way a consistency experiment reads them:

    NIS / dof   y^T S^-1 y over the state dimension of that callback -- 1 on average for a consistent filter
    pose NEES   e^T P_pose^-1 e of the pose against the truth        -- 3 on average for a consistent filter

Callbacks of the survey lap (the state still grows) are left out.  Prints one JSON document; --out writes it to a file.

    python tools/consistency_report.py [--batch 16] [--steps 200] [--landmarks 8,64] [--out profiles/consistency_report.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(kind, L, B, T, seed):
    import numpy as np
    import torch
    from awesomeslam_amd import consistency as cs
    from awesomeslam_amd import trace as tg
    from awesomeslam_amd.core import CFG_UKF_LARGE, Core

    tr = tg.make_traces(L, T, B=B, seed=seed)
    cap = tg.dim_cap(L)
    large = cap > 144
    core = Core(kind, cap, batch=B, max_obs=tr.max_obs, max_wait=min(2048 if large else 512, 2 * L + 64),
                flags=CFG_UKF_LARGE if kind == "ukf" and large else 0)
    core.set_trace(tr)
    dev = "cuda"
    poses = torch.zeros((B, T, 3), dtype=torch.float64, device=dev)
    dims = torch.zeros((B, T), dtype=torch.int32, device=dev)
    nis = torch.zeros((B, T), dtype=torch.float64, device=dev)
    logdet = torch.zeros((B, T), dtype=torch.float64, device=dev)
    pcov = torch.zeros((B, T, 6), dtype=torch.float64, device=dev)
    core.replay_stats(0, T, poses.data_ptr(), dims.data_ptr(), nis.data_ptr(), logdet.data_ptr(), pcov.data_ptr())
    torch.cuda.synchronize()
    poses, dims, nis, logdet, pcov = (a.cpu().numpy() for a in (poses, dims, nis, logdet, pcov))
    status = [core.status(b) for b in range(B)]
    core.close()
    steady = np.zeros((B, T), bool)
    steady[:, max(tr.warmup, 1):] = True
    steady &= np.isfinite(nis) & (dims == tg.full_dim(L))
    per_dof = np.where(steady, nis / np.maximum(dims, 1), np.nan)
    nees = np.where(steady, cs.pose_nees(poses, pcov, tr.truth), np.nan)
    ll = np.where(steady, cs.log_likelihood(nis, logdet, dims), np.nan)
    return {"filter": kind, "landmarks": L, "state_dim": tg.full_dim(L), "batch": B, "callbacks": T, "seed": seed,
            "callbacks_counted": int(steady.sum()), "filters_with_status_bits": int(sum(s != 0 for s in status)),
            "nis_per_dof_mean": float(np.nanmean(per_dof)), "nis_per_dof_median": float(np.nanmedian(per_dof)),
            "pose_nees_mean": float(np.nanmean(nees)), "pose_nees_median": float(np.nanmedian(nees)),
            "log_likelihood_mean": float(np.nanmean(ll)),
            "nis_per_dof_mean_per_filter": [float(v) for v in np.nanmean(per_dof, axis=1)],
            "pose_nees_mean_per_filter": [float(v) for v in np.nanmean(nees, axis=1)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--landmarks", default="8,64")
    ap.add_argument("--filters", default="ekf,ukf")
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    recs = []
    for kind in args.filters.split(","):
        for L in (int(v) for v in args.landmarks.split(",")):
            rec = run(kind, L, args.batch, args.steps, args.seed)
            print(f"{kind} L={L}: mean NIS/dof {rec['nis_per_dof_mean']:.3g} (consistent: 1), mean pose NEES {rec['pose_nees_mean']:.3g} (consistent: 3), "
                  f"{rec['callbacks_counted']} callbacks of {args.batch} filters", file=sys.stderr)
            recs.append(rec)
    doc = {"what": "tools/consistency_report.py: synthetic traces (awesomeslam_amd.trace.make_traces), sensor noise 0.02 / 0.002 against the reference's R = 0.2 I",
           "expected_if_consistent": {"nis_per_dof": 1.0, "pose_nees": 3.0}, "runs": recs}
    print(json.dumps(doc, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
