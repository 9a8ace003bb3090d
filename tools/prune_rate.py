#!/usr/bin/env python3
"""What removing landmarks costs (aslam_remove_landmarks, csrc/prune.h), beside the snapshot pack + unpack pair that moves the same filters.

    python tools/prune_rate.py [--reps 10] [--filters 256] [--out profiles/prune_rate.json] [--md profiles/prune.md]

One EKF fp32 context, 512 landmarks (n = 1027) x 256 filters, every filter at its full dimension.  Timed between two device events on the
default stream, the context restored from a device snapshot (untimed) before every repetition:
    one    aslam_remove_landmarks with a device mask that removes landmark 256 of every filter
    half   ... that removes every second landmark of every filter
The call holds one small device-to-host copy and one stream synchronisation between its map launch and its pack + unpack launches, so the
interval includes that host round trip: it is the time the stream is busy with the call, which is what a caller waits for.
    pack + unpack   aslam_debug_snapshot_rate on the same context in the same run: the two launches aslam_snapshot / aslam_restore enqueue
No rate is a pass/fail condition anywhere; the files record what was measured."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from awesomeslam_amd import core as C  # noqa: E402
from awesomeslam_amd import snapshot  # noqa: E402
from awesomeslam_amd import trace as tg  # noqa: E402


def measure(L, B, reps):
    import torch

    n = tg.full_dim(L)
    max_obs, max_wait = 16, 16
    core = C.Core("ekf", tg.dim_cap(L), batch=B, max_obs=max_obs, max_wait=max_wait, dtype=C.F32)
    rng = np.random.default_rng(L)
    A = rng.normal(size=(n, n)) * 0.02
    rec = dict(n=n, flags=0, status=0, A=np.array([1.0, 0.0]), X=rng.normal(size=n), Z=rng.normal(size=n), P=A @ A.T + np.eye(n) * 0.01,
               sens=rng.normal(size=(max_obs, 2)).astype(np.float32), wait_rb=rng.normal(size=(max_wait, 2)).astype(np.float32),
               wait_cnt=np.ones(max_wait, np.uint32))
    core.restore(snapshot.pack([rec], "ekf"), records=[0] * B, trajs=list(range(B)))
    blob_bytes = core.snapshot_bytes()
    buf = torch.empty(2 * blob_bytes, dtype=torch.uint8, device="cuda")
    full = torch.empty(blob_bytes, dtype=torch.uint8, device="cuda")
    core.snapshot(out=full)
    ld = (core.landmark_capacity() + 15) // 16 * 16
    drops = {"one": [L // 2], "half": list(range(0, L, 2))}
    out = {"filters": B, "landmarks": L, "n": n, "padded_dim": core.layout()[0], "blob_bytes": blob_bytes, "reps": reps}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, drop in drops.items():
        m = np.zeros((B, ld), np.uint8)
        m[:, drop] = 1
        mask = torch.from_numpy(m).cuda()
        ms = []
        for r in range(-2, reps):
            core.restore(full, records=list(range(B)))
            torch.cuda.synchronize()
            e0.record()
            core.remove_landmarks_ptr(mask.data_ptr(), ld, True)
            e1.record()
            torch.cuda.synchronize()
            if r >= 0:
                ms.append(e0.elapsed_time(e1))
        n_new = n - 2 * len(drop)
        assert [core.dim(b) for b in (0, B - 1)] == [n_new, n_new]
        got = snapshot.parse(core.snapshot(trajs=[B - 1]))[0]
        keep = np.delete(np.arange(n), [3 + 2 * i + j for i in drop for j in (0, 1)])
        assert np.array_equal(got["P"], rec["P"][np.ix_(keep, keep)]) and np.array_equal(got["X"], rec["X"][keep])
        rec_new = snapshot.record_bytes(n_new, max_obs, max_wait)
        out[name] = {"removed_per_filter": len(drop), "n_new": n_new, "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)),
                     "record_bytes_written": B * rec_new}
    # the yardstick, same context, same run: the filters back at full dimension
    core.restore(full, records=list(range(B)))
    ms = np.zeros((3, reps), np.float32)
    info = (ctypes.c_int64 * 3)()
    lib = C.core_lib()
    lib.aslam_debug_snapshot_rate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    C._chk(lib.aslam_debug_snapshot_rate(core._h, buf.data_ptr(), buf.numel(), reps, ms.ctypes.data, info))
    med = [float(np.median(ms[i])) for i in range(3)]
    out["snapshot"] = {"pack_ms_median": med[0], "unpack_ms_median": med[1], "copy_ms_median": med[2], "pack_plus_unpack_ms": med[0] + med[1]}
    for name in drops:
        out[name]["ratio_to_pack_plus_unpack"] = out[name]["ms_median"] / (med[0] + med[1])
    core.close()
    return out


def write_md(path, res):
    s, snap = res["shape"], res["shape"]["snapshot"]
    rows = "\n".join(f"| remove {k} ({s[k]['removed_per_filter']} per filter, n -> {s[k]['n_new']}) | {s[k]['ms_median']:.2f} | {s[k]['ms_min']:.2f} | "
                     f"{s[k]['ratio_to_pack_plus_unpack']:.2f} |" for k in ("one", "half"))
    txt = f"""# Removing landmarks: what a call costs

Written by `tools/prune_rate.py` ({res['device']}); the numbers are in `prune_rate.json`.

EKF fp32, {s['landmarks']} landmarks (n = {s['n']}, padded {s['padded_dim']}) x {s['filters']} filters, every filter pruned in one call, device
mask.  Median of {s['reps']} repetitions between two device events on the default stream; the context is restored (untimed) before each.

| what | ms (median) | ms (min) | / (pack + unpack) |
|---|---|---|---|
{rows}
| snapshot_pack + snapshot_unpack of the same filters | {snap['pack_plus_unpack_ms']:.2f} | | 1.00 |
| (pack {snap['pack_ms_median']:.2f}, unpack {snap['unpack_ms_median']:.2f}, device-to-device copy of the blob {snap['copy_ms_median']:.2f}) | | | |

How to read it.  A prune is prune_map (one wave per filter), one 16-byte-per-filter copy to the host with a stream synchronisation, prune_pack
and the unchanged snapshot_unpack.  prune_pack writes what snapshot_pack writes but reads P element by element through the survivor list
(8-byte loads at gathered columns, two per 16-byte store) instead of 16-byte loads of contiguous rows; snapshot_unpack rewrites the WHOLE padded
slot and clears the slot's scratch whatever the new dimension is, so removing half the landmarks saves pack time but no unpack time.  The
interval also holds the host round trip in the middle of the call, which the pack + unpack pair (two back-to-back launches) does not have.
This is a maintenance call, not a per-callback one; no figure here is a bar.
"""
    with open(path, "w") as f:
        f.write(txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--filters", type=int, default=256)
    ap.add_argument("--landmarks", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_rate.json"))
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "prune.md"))
    a = ap.parse_args()
    import torch

    res = {"tool": "tools/prune_rate.py", "device": torch.cuda.get_device_name(0),
           "timing": "device events around aslam_remove_landmarks (device mask, default stream), median of reps after 2 warm-up rounds; "
                     "aslam_debug_snapshot_rate in the same run", "shape": measure(a.landmarks, a.filters, a.reps)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    write_md(a.md, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
