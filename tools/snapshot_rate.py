#!/usr/bin/env python3
"""How fast whole filters move in and out of a context (include/aslam_snapshot.h): the pack and the unpack launch, timed with device events
beside a plain device-to-device hipMemcpyAsync of the blob's byte count, all three alternating in ONE call after a warm-up
(aslam_debug_snapshot_rate: the launches aslam_snapshot / aslam_restore enqueue, without their host side).

    python tools/snapshot_rate.py [--reps 20] [--out profiles/snapshot_rate.json]

Two shapes: EKF fp32 with 512 landmarks x 64 filters (few large records), EKF fp64 with 64 landmarks x 1024 filters (many small ones), every
filter at its full dimension.  Bytes are computed from the shapes, not counted:
    pack    reads the blob's bytes out of the padded layout and writes them           2 x blob
    unpack  reads the blob and writes the WHOLE padded slot plus the scratch it clears blob + padded + cleared
    copy    the yardstick                                                              2 x blob
No rate is a pass/fail condition anywhere; the file records what was measured."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from awesomeslam_amd import core as C  # noqa: E402
from awesomeslam_amd import snapshot  # noqa: E402
from awesomeslam_amd import trace as tg  # noqa: E402

SHAPES = (("ekf-f32-L512-B64", C.F32, 512, 64), ("ekf-f64-L64-B1024", C.F64, 64, 1024))


def measure(name, dtype, L, B, reps):
    import torch

    n = tg.full_dim(L)
    max_obs, max_wait = 16, 16
    core = C.Core("ekf", tg.dim_cap(L), batch=B, max_obs=max_obs, max_wait=max_wait, dtype=dtype)
    # one filter at full dimension, forked into every slot
    rng = np.random.default_rng(L)
    A = rng.normal(size=(n, n)) * 0.02
    rec = dict(n=n, flags=0, status=0, A=np.array([1.0, 0.0]), X=rng.normal(size=n), Z=rng.normal(size=n), P=A @ A.T + np.eye(n) * 0.01,
               sens=rng.normal(size=(max_obs, 2)).astype(np.float32), wait_rb=rng.normal(size=(max_wait, 2)).astype(np.float32),
               wait_cnt=np.ones(max_wait, np.uint32))
    core.restore(snapshot.pack([rec], "ekf"), records=[0] * B, trajs=list(range(B)))
    blob_bytes = core.snapshot_bytes()
    buf = torch.empty(2 * blob_bytes, dtype=torch.uint8, device="cuda")
    ms = np.zeros((3, reps), np.float32)
    info = (ctypes.c_int64 * 3)()
    lib = C.core_lib()
    lib.aslam_debug_snapshot_rate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_void_p]
    C._chk(lib.aslam_debug_snapshot_rate(core._h, buf.data_ptr(), buf.numel(), reps, ms.ctypes.data, info))
    assert info[0] == blob_bytes
    # the round trip is the identity: what the timed launches left in the context is what went in
    back = snapshot.parse(core.snapshot(trajs=[0, B - 1]))
    assert all(snapshot.records_equal(r, rec) for r in back)
    NP = core.layout()[0]
    padded, cleared = int(info[1]), int(info[2])  # from the shapes: B x (P, X, Z, the lists at their capacity), B x the scratch a reset zeroes
    assert padded == B * (8 * NP * NP + 2 * 8 * NP + 8 * max_obs + 12 * max_wait)
    moved = {"pack": 2 * blob_bytes, "unpack": blob_bytes + padded + cleared, "copy": 2 * blob_bytes}
    med = {k: float(np.median(ms[i])) for i, k in enumerate(("pack", "unpack", "copy"))}
    out = {"shape": name, "filters": B, "landmarks": L, "n": n, "padded_dim": NP, "blob_bytes": blob_bytes, "reps": reps}
    for k in ("pack", "unpack", "copy"):
        out[k] = {"ms_median": med[k], "ms_min": float(ms[("pack", "unpack", "copy").index(k)].min()), "bytes_moved": moved[k],
                  "GBps": moved[k] / med[k] / 1e6}
    # time per blob byte against the yardstick's (1.0 = as fast as a plain copy of the blob)
    out["pack"]["copy_time_ratio"] = med["copy"] / med["pack"]
    out["unpack"]["copy_time_ratio"] = med["copy"] / med["unpack"]
    core.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "snapshot_rate.json"))
    a = ap.parse_args()
    import torch

    res = {"tool": "tools/snapshot_rate.py", "device": torch.cuda.get_device_name(0), "timing": "device events around each launch, median of reps after 3 warm-up rounds, pack / unpack / copy alternating",
           "shapes": [measure(*s, a.reps) for s in SHAPES]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
