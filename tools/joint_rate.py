#!/usr/bin/env python3
"""What the joint-compatibility test costs (aslam_joint_compat, csrc/joint.h): the chain gate -> joint, in place on one device array, beside
aslam_gate_observations alone on the same inputs.

    python tools/joint_rate.py [--reps 20] [--out profiles/joint_rate.json] [--md profiles/joint.md] [--err-over-bar X] [--parent-json F]
    python tools/joint_rate.py --gate-only --root OTHER_TREE --out F     (the gate alone with the package of another checkout, e.g. the parent commit)
    python tools/joint_rate.py --from-json profiles/joint_rate.json      (rewrite the .md from recorded numbers, no GPU)

Three shapes, 256 filters each, every filter at its full dimension (restored from one packed record, untimed):
    512 landmarks (n = 1027, EKF fp32 chain; P is binary64), 24 observations
    64 landmarks (n = 131, EKF fp64 single-CU kernels), 16 observations, and 64 observations (the cap)
Every observation is a landmark's own predicted reading plus noise, distinct landmarks as far as there are any.  Timed by wall clock around the
calls and a stream synchronisation (the issue of both launches, their small host-to-device copies and the kernels), median of `reps` after 3
warm-up rounds:
    gate    aslam_gate_observations with a device obs array
    chain   aslam_gate_observations, then aslam_joint_compat in place on its output, at 0.99
No rate is a pass/fail condition anywhere; the files record what was measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

GATE, PROB = 9.21, 0.99
SHAPES = ((512, "f32", 24), (64, "f64", 16), (64, "f64", 64))
FILTERS = 256


def measure(L, dtype, n_obs, reps, gate_only):
    import torch

    from awesomeslam_amd import core as C
    from awesomeslam_amd import snapshot
    from awesomeslam_amd import trace as tg

    B, n = FILTERS, tg.full_dim(L)
    max_obs, max_wait = 16, 16
    core = C.Core("ekf", tg.dim_cap(L), batch=B, max_obs=max_obs, max_wait=max_wait, dtype=C.F32 if dtype == "f32" else C.F64)
    rng = np.random.default_rng(L)
    A = rng.normal(size=(n, n)) * 0.02
    X = np.concatenate([[0.0, 0.0, 0.0], rng.uniform(-20, 20, 2 * L)])
    lm = X[3:].reshape(-1, 2)
    Z = X.copy()
    Z[3::2], Z[4::2] = np.hypot(lm[:, 0], lm[:, 1]), np.arctan2(lm[:, 1], lm[:, 0])
    rec = dict(n=n, flags=0, status=0, A=np.array([1.0, 0.0]), X=X, Z=Z, P=A @ A.T + np.eye(n) * 0.01,
               sens=rng.normal(size=(max_obs, 2)).astype(np.float32), wait_rb=rng.normal(size=(max_wait, 2)).astype(np.float32),
               wait_cnt=np.ones(max_wait, np.uint32))
    core.restore(snapshot.pack([rec], "ekf"), records=[0] * B, trajs=list(range(B)))
    k = rng.permutation(L)[:n_obs]
    obs = np.stack([Z[3 + 2 * k] + 0.1 * rng.normal(size=n_obs), Z[4 + 2 * k] + 0.01 * rng.normal(size=n_obs)], axis=1).astype(np.float32)
    dev = torch.from_numpy(np.tile(obs, (B, 1, 1))).cuda()
    assoc = torch.empty((B, n_obs), dtype=torch.int32, device="cuda")
    incr = torch.empty((B, n_obs), dtype=torch.float64, device="cuda")
    joint = torch.empty((B, 2), dtype=torch.float64, device="cuda")
    count = torch.empty((B, 2), dtype=torch.int32, device="cuda")
    cnt = np.full(B, n_obs, np.int32)

    def timed(f):
        ms = []
        for r in range(-3, reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if r >= 0:
                ms.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    def gate():
        core.gate_observations_ptr(dev.data_ptr(), n_obs, True, cnt, GATE, assoc.data_ptr(), None)

    out = {"landmarks": L, "n": n, "filters": B, "dtype": dtype, "observations": n_obs, "reps": reps}
    out["gate_ms_median"], out["gate_ms_min"], out["gate_ms_max"] = timed(gate)
    gated = assoc.cpu().numpy()
    assert (gated == gated[0]).all()  # the same filter B times: the same answer B times
    out["gated"] = int((gated[0] >= 0).sum())
    if not gate_only:
        tab = C.joint_gates(PROB, n_obs)

        def chain():
            gate()
            core.joint_compat_ptr(dev.data_ptr(), n_obs, True, cnt, assoc.data_ptr(), tab, assoc.data_ptr(), incr.data_ptr(), joint.data_ptr(), count.data_ptr())

        out["chain_ms_median"], out["chain_ms_min"], out["chain_ms_max"] = timed(chain)
        got, c = assoc.cpu().numpy(), count.cpu().numpy()
        assert (got == got[0]).all() and (c == c[0]).all()
        out.update(accepted=int(c[0, 0]), refused=int(c[0, 1]), D2=float(joint.cpu().numpy()[0, 0]),
                   joint_ms_by_difference=out["chain_ms_median"] - out["gate_ms_median"])
    core.close()
    return out


def write_md(path, res):
    parent = {(s["landmarks"], s["observations"]): s for s in res.get("parent_gate", {}).get("shapes", [])}

    def row(s):
        p = parent.get((s["landmarks"], s["observations"]))
        ptxt = f"{1e3 * p['gate_ms_median']:.0f} ({1e3 * p['gate_ms_min']:.0f} .. {1e3 * p['gate_ms_max']:.0f})" if p else "not measured"
        return (f"| {s['landmarks']} (n = {s['n']}, {s['dtype']}) | {s['observations']} | {s['gated']} / {s['accepted']} / {s['refused']} | "
                f"{1e3 * s['gate_ms_median']:.0f} ({1e3 * s['gate_ms_min']:.0f} .. {1e3 * s['gate_ms_max']:.0f}) | {ptxt} | "
                f"{1e3 * s['chain_ms_median']:.0f} ({1e3 * s['chain_ms_min']:.0f} .. {1e3 * s['chain_ms_max']:.0f}) | {1e3 * s['joint_ms_by_difference']:.0f} |")

    rows = "\n".join(row(s) for s in res["shapes"])
    ratio = res.get("err_over_bar")
    ratio_txt = (f"The worst error / bar seen on the GPU over every case of `tests/test_gpu_joint.py` is **{ratio:.3f}** (D2 and each increment against "
                 "the long-double reference as |dev - ld| / max(ld, 1), log det as |dev - ld| / max(|ld|, 1); bar = max(32 x spread, 64 x 2^-52), spread "
                 "the larger binary64-versus-long-double difference of the reference's bordering and dense forms on the same input)."
                 ) if ratio is not None else "The worst error / bar of the GPU tests was not recorded with this run."
    txt = f"""# Joint compatibility: what the chain gate -> joint costs

Written by `tools/joint_rate.py` ({res['device']}); the numbers are in `joint_rate.json`.

{res['shapes'][0]['filters']} filters, every filter at its full dimension, a device `obs` array; every observation is a landmark's own predicted reading plus noise.
Wall clock around the calls and a synchronisation, median (min .. max) of {res['shapes'][0]['reps']} repetitions after 3 warm-up rounds, in microseconds.  "gate" is
`aslam_gate_observations` alone; "chain" is the gate and then `aslam_joint_compat` in place on its output at 0.99; "gate at the parent commit" is
the same measurement of the gate with the library built from the parent commit, in the same session.

| landmarks | observations | gated / accepted / refused | gate, us | gate at the parent commit, us | chain, us | chain - gate, us |
|---|---|---|---|---|---|---|
{rows}

How to read it.  `joint_compat` is one launch, one workgroup of 256 threads per filter.  Phases 0 to 2 are parallel (a 2 x 2 congruence of 25
entries of P per candidate pair); phase 3 is one wave doing the bordering, about 2m dependent steps (a cross-lane read, a division, a fused
multiply-add) for the candidate behind m accepted pairings, so its time grows with the square of the message length and does not depend on
the state dimension.  The filters run side by side, one workgroup per CU.  The "chain - gate" column also holds the second call's host side
(its synchronisation of the context, two small host-to-device copies, the launch).  Before this measurement the kernel's cost was an estimate
(a few tens of microseconds at 16 observations, a few hundred at 64); the table is the record.

{ratio_txt}

No figure here is a bar.
"""
    with open(path, "w") as f:
        f.write(txt)


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--root", default=here, help="the checkout whose awesomeslam_amd package (and built libraries) is measured")
    ap.add_argument("--gate-only", action="store_true", help="aslam_gate_observations alone (a tree without the joint test)")
    ap.add_argument("--out", default=os.path.join(here, "profiles", "joint_rate.json"))
    ap.add_argument("--md", default=os.path.join(here, "profiles", "joint.md"))
    ap.add_argument("--err-over-bar", type=float, default=None, help="worst error / bar printed by tests/test_gpu_joint.py (-s), recorded as given")
    ap.add_argument("--parent-json", default=None, help="a --gate-only result of the parent commit, recorded beside this tree's")
    ap.add_argument("--from-json", default=None)
    a = ap.parse_args()
    if a.from_json:
        res = json.load(open(a.from_json))
    else:
        sys.path.insert(0, os.path.abspath(a.root))
        import torch

        res = {"tool": "tools/joint_rate.py", "device": torch.cuda.get_device_name(0), "gate_only": a.gate_only,
               "timing": "wall clock around the calls and a synchronisation, median of reps after 3 warm-up rounds",
               "shapes": [measure(L, dtype, n_obs, a.reps, a.gate_only) for L, dtype, n_obs in SHAPES]}
    if a.err_over_bar is not None:
        res["err_over_bar"] = a.err_over_bar
    if a.parent_json:
        res["parent_gate"] = json.load(open(a.parent_json))
    with open(a.from_json or a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if not res.get("gate_only"):
        write_md(a.md, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
