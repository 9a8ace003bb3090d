#!/usr/bin/env python3
"""What the sighting records and the forgetting policy cost (aslam_get_sightings / aslam_select_stale, csrc/small_common.h, csrc/prune.h).

    python tools/forget_rate.py [--reps 10] [--filters 256] [--landmarks 512] [--bench-this a.json b.json c.json --bench-parent d.json ...]
                                [--out profiles/forget_rate.json] [--md profiles/forget.md]

Prune cost.  One EKF fp32 context, 512 landmarks (n = 1027) x 256 filters, every filter at its full dimension with the robot at the origin:
the even landmarks stand on a near grid, the odd ones on a far one.  One callback of a hand-made trace observes exactly the even landmarks, so
the odd ones have age 1 and `select_stale(0)` selects what `select_beyond(between the grids)` selects.  Timed between two device events on the
default stream, the context restored from a device snapshot and stepped through that callback (both untimed) before every repetition:
    stale    aslam_select_stale + aslam_remove_landmarks, device mask
    beyond   aslam_select_beyond + aslam_remove_landmarks, device mask: the same landmarks, the same run
Each interval includes the host round trip inside aslam_remove_landmarks (see tools/prune_rate.py).

Headline rate.  The front end writes the records in every callback, so the question is whether `python bench.py` (default workload) moved.
The tool does not check out commits: it takes the JSON result lines of bench.py runs of this commit and of its parent, made alternately on one
device in one session (--bench-this / --bench-parent: files holding one result line each), and records both ranges and whether they overlap.
No figure is a pass/fail condition anywhere; the files record what was measured."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from awesomeslam_amd import core as C  # noqa: E402
from awesomeslam_amd import snapshot  # noqa: E402
from awesomeslam_amd import trace as tg  # noqa: E402


def world(L):
    """landmark positions [L, 2]: even ones on a grid 3 .. 40 m from the origin, odd ones on the same grid pushed out by 100 m; every pair of
    landmarks is at least 1 m apart (assoc_dist is 0.5 m)"""
    side = int(np.ceil(np.sqrt(L / 2)))
    gx, gy = np.meshgrid(np.arange(side), np.arange(side))
    grid = np.stack([3.0 + 1.5 * gx.reshape(-1), 3.0 + 1.5 * gy.reshape(-1)], 1)[: (L + 1) // 2]
    lm = np.zeros((L, 2))
    lm[0::2] = grid[: len(lm[0::2])]
    lm[1::2] = grid[: len(lm[1::2])] + 100.0
    return lm


def measure(L, B, reps):
    import torch

    n = tg.full_dim(L)
    lm = world(L)
    rb = np.stack([np.hypot(lm[:, 0], lm[:, 1]), np.arctan2(lm[:, 1], lm[:, 0])], 1)
    near = np.arange(0, L, 2)
    max_obs, max_wait = len(near), 16
    core = C.Core("ekf", tg.dim_cap(L), batch=B, max_obs=max_obs, max_wait=max_wait, dtype=C.F32)
    X = np.concatenate([np.zeros(3), lm.reshape(-1)])
    Z = np.concatenate([np.zeros(3), rb.reshape(-1)])
    rec = dict(n=n, flags=0, status=0, A=np.array([1.0, 0.0]), X=X, Z=Z, P=np.eye(n) * 0.01,
               sens=np.zeros((0, 2), np.float32), wait_rb=np.zeros((0, 2), np.float32), wait_cnt=np.zeros(0, np.uint32))
    core.restore(snapshot.pack([rec], "ekf"), records=[0] * B, trajs=list(range(B)))
    # one callback: the robot at rest at the origin, a sensor message with the even landmarks
    odom = np.zeros((B, 1, 8))
    odom[:, :, 2] = 1.0  # qw
    obs = np.broadcast_to(rb[near].astype(np.float32), (B, 1, max_obs, 2)).copy()
    tr = tg.Trace(odom, np.full((B, 1), 0.1, np.float32), np.ones((B, 1), np.uint8), np.full((B, 1), max_obs, np.int32), obs,
                  np.broadcast_to(lm, (B, L, 2)).copy(), None)
    core.set_trace(tr)
    full = torch.empty(core.snapshot_bytes(), dtype=torch.uint8, device="cuda")
    core.snapshot(out=full)
    ld = (core.landmark_capacity() + 15) // 16 * 16
    mask = torch.zeros((B, ld), dtype=torch.uint8, device="cuda")
    radius = 80.0  # between the grids
    out = {"filters": B, "landmarks": L, "n": n, "padded_dim": core.layout()[0], "reps": reps, "removed_per_filter": L // 2}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    masks = {}
    for name in ("stale", "beyond"):
        ms = []
        for r in range(-2, reps):
            core.restore(full, records=list(range(B)))
            core.replay(0, 1)
            torch.cuda.synchronize()
            e0.record()
            if name == "stale":
                core.select_stale(0, mask.data_ptr(), ld)
            else:
                core.select_beyond(radius, mask.data_ptr(), ld)
            core.remove_landmarks_ptr(mask.data_ptr(), ld, True)
            e1.record()
            torch.cuda.synchronize()
            if r >= 0:
                ms.append(e0.elapsed_time(e1))
        masks[name] = mask.cpu().numpy().copy()
        assert [core.dim(b) for b in (0, B - 1)] == [n - 2 * (L // 2)] * 2 and core.status(0) == 0, (name, core.dim(0), core.status(0))
        seen, hits, clk = core.sightings(B - 1)
        assert clk == 1 and (seen == 1).all() and (hits == 1).all()  # the survivors are the landmarks the callback sighted
        out[name] = {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms))}
    want = np.zeros(ld, np.uint8)
    want[1:L:2] = 1
    assert all(np.array_equal(masks[k][b], want) for k in masks for b in (0, B - 1))  # both selectors chose the odd landmarks
    out["stale"]["ratio_to_beyond"] = out["stale"]["ms_median"] / out["beyond"]["ms_median"]
    core.close()
    return out


def bench_ranges(this, parent):
    def values(paths):
        v = []
        for p in paths:
            lines = [ln for ln in open(p).read().splitlines() if ln.startswith("{")]
            v.append(float(json.loads(lines[-1])["value"]))
        return v

    a, b = values(this), values(parent)
    return {"unit": "filter-steps/s", "this_commit": a, "parent_commit": b, "this_range": [min(a), max(a)], "parent_range": [min(b), max(b)],
            "ranges_overlap": bool(min(a) <= max(b) and min(b) <= max(a)), "this_median_over_parent_median": float(np.median(a) / np.median(b))}


def write_md(path, res):
    s = res["prune"]
    txt = f"""# Sighting records and forgetting: what they cost

Written by `tools/forget_rate.py` ({res['device']}); the numbers are in `forget_rate.json`.

## A prune by age beside a prune by range

EKF fp32, {s['landmarks']} landmarks (n = {s['n']}, padded {s['padded_dim']}) x {s['filters']} filters; every filter loses the same {s['removed_per_filter']}
landmarks in one call, device mask.  Median of {s['reps']} repetitions between two device events on the default stream; the context is restored
and stepped through one callback (untimed) before each.

| what | ms (median) | ms (min) |
|---|---|---|
| select_stale + remove_landmarks | {s['stale']['ms_median']:.2f} | {s['stale']['ms_min']:.2f} |
| select_beyond + remove_landmarks, the same landmarks | {s['beyond']['ms_median']:.2f} | {s['beyond']['ms_min']:.2f} |

Ratio stale / beyond: {s['stale']['ratio_to_beyond']:.2f}.  The two calls differ in the selector (one wave per filter either way: 4 bytes per landmark
read instead of 16) and in nothing else: both prunes run prune_map, prune_pack, snapshot_unpack and sight_compact.  See `prune.md` for what a
prune costs beside a snapshot.
"""
    b = res.get("bench")
    if b:
        fmt = lambda v: ", ".join(f"{x:.0f}" for x in v)  # noqa: E731
        txt += f"""
## The headline rate with the records written in every callback

`python bench.py` (default workload), this commit and its parent alternately on one device in one session, {b['unit']}:

| | runs | range |
|---|---|---|
| this commit | {fmt(b['this_commit'])} | {b['this_range'][0]:.0f} .. {b['this_range'][1]:.0f} |
| parent commit | {fmt(b['parent_commit'])} | {b['parent_range'][0]:.0f} .. {b['parent_range'][1]:.0f} |

The ranges {'overlap' if b['ranges_overlap'] else 'DO NOT overlap'}; median over median {b['this_median_over_parent_median']:.4f}.  The front end adds one 4-byte load and at most two
4-byte stores per sighted landmark per callback.
"""
    with open(path, "w") as f:
        f.write(txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--filters", type=int, default=256)
    ap.add_argument("--landmarks", type=int, default=512)
    ap.add_argument("--bench-this", nargs="*", default=[])
    ap.add_argument("--bench-parent", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forget_rate.json"))
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "forget.md"))
    a = ap.parse_args()
    import torch

    res = {"tool": "tools/forget_rate.py", "device": torch.cuda.get_device_name(0),
           "timing": "device events around select + aslam_remove_landmarks (device mask, default stream), median of reps after 2 warm-up rounds",
           "prune": measure(a.landmarks, a.filters, a.reps)}
    if a.bench_this and a.bench_parent:
        res["bench"] = bench_ranges(a.bench_this, a.bench_parent)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    write_md(a.md, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
