#!/usr/bin/env python3
"""What Mahalanobis-gated association costs (aslam_gate_observations, csrc/assoc.h): the call beside one callback of the same context, and
the host mirror's callbacks per second with the gate on against off.

    python tools/assoc_rate.py [--reps 20] [--out profiles/assoc_rate.json] [--md profiles/assoc.md] [--err-over-bar X]
    python tools/assoc_rate.py --from-json profiles/assoc_rate.json      (rewrite the .md from recorded numbers, no GPU)

Three shapes, 16 observations per filter, every filter at its full dimension (restored from one packed record, untimed):
    64 landmarks (n = 131, EKF fp64 single-CU kernels) x 256 filters
    512 landmarks (n = 1027, EKF fp32 chain; P is binary64) x 256 filters, and x 1 filter
Timed between two device events on the default stream, median of `reps` after 3 warm-up rounds:
    gate   aslam_gate_observations with a device obs array (its two small host-to-device copies of n_obs and gate included)
    step   one aslam_ekf_step_batch callback of the same context: existing code on the same tree
and the ratio gate / step.  Then the node: trace(8) of tests/test_gpu_snapshot.py's generator driven through core.Node, wall clock, with the
gate off (the behaviour of the parent commit) and at 9.21.
No rate is a pass/fail condition anywhere; the files record what was measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_OBS = 16
GATE = 9.21


def measure(L, B, dtype, reps):
    import torch

    from awesomeslam_amd import core as C
    from awesomeslam_amd import snapshot
    from awesomeslam_amd import trace as tg

    n = tg.full_dim(L)
    max_obs, max_wait = 16, 16
    core = C.Core("ekf", tg.dim_cap(L), batch=B, max_obs=max_obs, max_wait=max_wait, dtype=C.F32 if dtype == "f32" else C.F64)
    rng = np.random.default_rng(L)
    A = rng.normal(size=(n, n)) * 0.02
    X = np.concatenate([[0.0, 0.0, 0.0], rng.uniform(-20, 20, 2 * L)])
    lm = X[3:].reshape(-1, 2)
    Z = X.copy()  # the pose, then every landmark's own predicted reading: a callback that has little to correct
    Z[3::2], Z[4::2] = np.hypot(lm[:, 0], lm[:, 1]), np.arctan2(lm[:, 1], lm[:, 0])
    rec = dict(n=n, flags=0, status=0, A=np.array([1.0, 0.0]), X=X, Z=Z, P=A @ A.T + np.eye(n) * 0.01,
               sens=rng.normal(size=(max_obs, 2)).astype(np.float32), wait_rb=rng.normal(size=(max_wait, 2)).astype(np.float32),
               wait_cnt=np.ones(max_wait, np.uint32))
    core.restore(snapshot.pack([rec], "ekf"), records=[0] * B, trajs=list(range(B)))
    k = rng.integers(L, size=N_OBS)
    obs = np.stack([Z[3 + 2 * k] + 0.1 * rng.normal(size=N_OBS), Z[4 + 2 * k] + 0.01 * rng.normal(size=N_OBS)], axis=1).astype(np.float32)
    dev = torch.from_numpy(np.tile(obs, (B, 1, 1))).cuda()
    assert dev.is_contiguous() and dev.shape == (B, N_OBS, 2)
    assoc = torch.empty((B, N_OBS), dtype=torch.int32, device="cuda")
    mdist = torch.empty((B, N_OBS), dtype=torch.float64, device="cuda")
    n_obs = np.full(B, N_OBS, np.int32)
    vx, az, dt = (np.full(B, v, np.float32) for v in (0.0, 0.0, 0.05))
    Zb = np.ascontiguousarray(np.broadcast_to(Z, (B, n)))
    a00, a10 = np.ones(B), np.zeros(B)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(f):
        ms = []
        for r in range(-3, reps):
            torch.cuda.synchronize()
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            if r >= 0:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms))

    g_med, g_min = timed(lambda: core.gate_observations_ptr(dev.data_ptr(), N_OBS, True, n_obs, GATE, assoc.data_ptr(), mdist.data_ptr()))
    got = assoc.cpu().numpy()
    assert (got == got[0]).all() and (got >= -1).all() and (got < L).all()  # the same filter B times: the same answer B times
    s_med, s_min = timed(lambda: core.step_batch(vx, az, dt, Zb, a00, a10))
    out = {"landmarks": L, "n": n, "filters": B, "dtype": dtype, "observations": N_OBS, "reps": reps, "kernel": core.kernel_info()["name"],
           "associated": int((got[0] >= 0).sum()), "to_their_own_landmark": int((got[0] == k).sum()), "status_after": [core.status(b) for b in (0, B - 1)],
           "gate_ms_median": g_med, "gate_ms_min": g_min, "step_ms_median": s_med, "step_ms_min": s_min, "gate_over_step": g_med / s_med}
    core.close()
    return out


def measure_node(T):
    from awesomeslam_amd import core as C
    from awesomeslam_amd import trace as tg

    tr = tg.make_traces(8, T, B=1, seed=2, sensor_every=2, dt_mode="random")[0]
    out = {"trace": "make_traces(8, T, B=1, seed=2, sensor_every=2, dt_mode='random')", "callbacks": T}
    for name, gate in (("off", 0.0), ("on", GATE)):
        best = None
        for _ in range(3):
            node = C.Node("ekf", tg.dim_cap(8))
            node.set_assoc_gate(gate)
            t0 = time.perf_counter()
            node.replay(tr)
            t = time.perf_counter() - t0
            best = t if best is None else min(best, t)
            out[name] = {"gate": gate, "seconds": best, "callbacks_per_s": T / best, "final_dim": node.N, "rejected": node.assoc_rejected()}
            node.close()
    out["on_over_off_time"] = out["on"]["seconds"] / out["off"]["seconds"]
    return out


def write_md(path, res):
    rows = "\n".join(f"| {s['landmarks']} (n = {s['n']}, {s['dtype']}) | {s['filters']} | {1e3 * s['gate_ms_median']:.1f} | {1e3 * s['gate_ms_min']:.1f} | "
                     f"{1e3 * s['step_ms_median']:.1f} | {s['gate_over_step']:.4f} |" for s in res["shapes"])
    nd = res["node"]
    ratio = res.get("err_over_bar")
    ratio_txt = (f"The worst error / bar seen on the GPU over every case of `tests/test_gpu_assoc.py` is **{ratio:.3f}** (`mdist` against the long-double "
                 "reference as |m_dev - m_ld| / max(m_ld, 1); bar = max(32 x the binary64-versus-long-double spread of the reference on the same input, "
                 "64 x 2^-52)).") if ratio is not None else "The worst error / bar of the GPU tests was not recorded with this run."
    txt = f"""# Mahalanobis-gated association: what a call costs

Written by `tools/assoc_rate.py` ({res['device']}); the numbers are in `assoc_rate.json`.

`aslam_gate_observations`, {res['shapes'][0]['observations']} observations per filter, a device `obs` array, every filter at its full dimension; beside it one
`aslam_ekf_step_batch` callback of the same context (existing code, the same tree).  Median of {res['shapes'][0]['reps']} repetitions between two device
events on the default stream after 3 warm-up rounds.

| landmarks | filters | gate call, us (median) | gate call, us (min) | one callback, us (median) | gate / callback |
|---|---|---|---|---|---|
{rows}

How to read it.  The call is one launch, one workgroup of 4 waves per filter: 15 lower-triangle entries of P, a `sqrt`, an `atan2` and a
25-product congruence per landmark into LDS (6 doubles each), then a wave per observation over the landmarks with one IEEE `remainder` per
pair and a wave-level arg-min.  The interval also holds the call's two small host-to-device copies (`n_obs`, `gate`) and the launch itself;
at one filter that is most of it.  Nothing of P leaves the device.

The host mirror (`core.Node`, EKF, 8 landmarks, {nd['callbacks']} callbacks, wall clock, best of 3): gate off {nd['off']['callbacks_per_s']:.0f} callbacks/s (the
behaviour of the parent commit), gate at 9.21 {nd['on']['callbacks_per_s']:.0f} callbacks/s ({nd['on_over_off_time']:.2f} x the time): with the gate on every callback with a
landmark mapped makes one more call and one 4-byte-per-observation copy back, each a host round trip.  Final dimension {nd['off']['final_dim']} / {nd['on']['final_dim']},
observations dropped by the gate {nd['on']['rejected']}.  The two runs do not map the same landmarks: with the default `r_range = r_bearing = 0.2` the gate at
9.21 reaches about 1.4 m in range and 1.4 rad in bearing around a landmark's predicted reading, far beyond `assoc_dist`, so it is no
substitute for a noise model that describes the sensor (INTEGRATION.md §2i); which observations went where was not examined.

{ratio_txt}

No figure here is a bar.
"""
    with open(path, "w") as f:
        f.write(txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--node-callbacks", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assoc_rate.json"))
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "assoc.md"))
    ap.add_argument("--err-over-bar", type=float, default=None, help="worst error / bar printed by tests/test_gpu_assoc.py (-s), recorded as given")
    ap.add_argument("--from-json", default=None)
    a = ap.parse_args()
    if a.from_json:
        res = json.load(open(a.from_json))
    else:
        import torch

        res = {"tool": "tools/assoc_rate.py", "device": torch.cuda.get_device_name(0),
               "timing": "device events around aslam_gate_observations (device obs, default stream) and around aslam_ekf_step_batch, median of reps "
                         "after 3 warm-up rounds; the node by wall clock, best of 3",
               "shapes": [measure(64, 256, "f64", a.reps), measure(512, 256, "f32", a.reps), measure(512, 1, "f32", a.reps)],
               "node": measure_node(a.node_callbacks)}
    if a.err_over_bar is not None:
        res["err_over_bar"] = a.err_over_bar
    with open(a.from_json or a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    write_md(a.md, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
