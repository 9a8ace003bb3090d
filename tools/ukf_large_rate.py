#!/usr/bin/env python3
"""Rate of the large-state UKF chain (ukf_large.h; ASLAM_CFG_UKF_LARGE) -- a number to record, not a target, and not part of bench.py.

Per shape (UKF fp64 at 142, 256 and 512 landmarks = state dimension 287, 515, 1027; batch 1 and 64): device-event time of ONE aslam_replay
over `--steps` steady-state callbacks (every landmark mapped) after a warm-up replay that grows the map and has launched every kernel; one
JSON line with filter-steps/s, ms per callback, the chain's floating-point operations AS BUILT (counted from the shapes below, tile by tile
the way the kernels skip work -- not the reference's operation count), that over the fp64 MFMA peak (78.6 TFLOP/s), and
the CPU oracle's slam() rate on one core of the same machine for scale.

    python tools/ukf_large_rate.py [--steps 24] [--landmarks 142 256 512] [--batches 1 64] [--out profiles/ukf_large_rate.json] [--no-oracle]
    python tools/ukf_large_rate.py --flops-only        # the operation counts alone: needs no GPU

There is no CPU fallback: without a GPU the timing path fails."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F64_TFLOPS = 78.6  # 256 CU x 4 SIMD x 16 FMA/clk x 2 x 2.4 GHz, v_fma_f64 and v_mfma_f64 alike
LB, TB = 64, 128


def chain_flops(n):
    """floating-point operations of one callback of one filter of dimension n, per kernel family, as the kernels are built"""
    nb = (n + 2 + LB - 1) // LB        # active 64-blocks: n state rows + z^T + the innovation
    na = nb * LB
    m = 2 * n + 5
    K = (m + 15) // 16 * 16            # sigma points, padded to the slab of ukf_large_wabt

    def subtiles(first, width=64):     # 16-row subtiles of a 64-row quadrant that hold a valid row (nu / nv of the kernels)
        return max(0, min(width // 16, (n - first + 15) // 16))

    def quadrant_products(sym, depth):  # 128x128 tiles of 2x2 quadrants, lower tiles (and lower quadrants of diagonal tiles) when symmetric
        f = 0
        nt = (na + TB - 1) // TB
        for rt in range(nt):
            for jt in range(rt + 1 if sym else nt):
                for wr in (0, 64):
                    for wc in (0, 64):
                        if sym and rt == jt and wc > wr:
                            continue
                        f += subtiles(rt * TB + wr) * subtiles(jt * TB + wc) * 16 * 16 * depth * 2
        return f

    wabt = 2 * quadrant_products(True, K) + quadrant_products(False, K)   # P, S+ (symmetric), Tc (full)
    syrk = quadrant_products(True, na)                                    # P -= W W^T, K loop over na columns

    def panels(s_only):
        f = 0
        for k0 in range(nb):
            blocks = (nb if s_only else 2 * nb) - k0 - 1  # 64-row blocks below the diagonal block (S, then all of G)
            wgs = (blocks + 1) // 2                       # a workgroup takes two blocks; a missing second one is computed and dropped
            sblocks = nb - k0 - 1
            f += wgs * 128 * 64 * (64 * k0) * 2           # left-looking update
            f += wgs * 128 * 64 * 64 * 2                  # X = C Linv^T
            f += ((sblocks + 1) // 2) * 128 * 64 * 64 * 2  # S(rt, rt) -= X X^T in the workgroups that hold blocks of S
        return f

    potrf = 2 * nb * (64 ** 3 // 3 + 64 ** 3 // 3)        # factor + inverse of a 64x64 diagonal block, twice per callback
    vectors = 8 * n * n + 3 * n * n + 60 * m * (n // 2) + 40 * m  # gain (4 FMAs / entry), rank-1, sigma points (two entries, h, the sums)
    parts = {"ukf_large_wabt": wabt, "large_update_panel": panels(True) + panels(False), "large_syrk": syrk, "large_potrf_inv_tiles": potrf,
             "vector_kernels": vectors}
    parts["total"] = sum(parts.values())
    return parts


def oracle_rate(state, cap, steps):
    """slam() calls per second of the CPU oracle (one core) from the steady state the GPU filter reached: one untimed call, then `steps` timed"""
    from oracle.c_oracle import CFilter

    X, Z, P = state
    o = CFilter("ukf", cap)
    o.set_state(len(X), X, Z, P)
    o.slam(0.2, 0.1, 0.1)
    t0 = time.perf_counter()
    for _ in range(steps):
        o.slam(0.2, 0.1, 0.1)
    return steps / (time.perf_counter() - t0)


def measure(L, B, steps, with_oracle, oracle_steps):
    import torch

    from awesomeslam_amd import trace as tg
    from awesomeslam_amd.core import CFG_UKF_LARGE, Core

    warm = 42  # three growth stages of make_traces end here (tests: 512 landmarks mapped after 42 callbacks)
    tr1 = tg.make_traces(L, warm + steps, B=1, seed=71)
    tr = tr1.select([0] * B)
    cap = tg.dim_cap(L)
    core = Core("ukf", cap, batch=B, max_obs=tr.max_obs, max_wait=2048, flags=CFG_UKF_LARGE)
    core.set_trace(tr)
    core.replay(0, warm)
    torch.cuda.synchronize()
    n = core.dim(0)
    assert n == tg.full_dim(L), (n, tg.full_dim(L))
    state = core.state(0) if with_oracle else None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    core.replay(warm, steps)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    assert all(core.status(b) == 0 for b in range(B)) and core.dim(B - 1) == n
    fl = chain_flops(n)
    rate = B * steps / (ms * 1e-3)
    rec = {"workload": "ukf_large_f64", "landmarks": L, "n": n, "batch": B, "steps": steps, "warmup_callbacks": warm,
           "ms_per_callback": ms / steps, "filter_steps_per_s": rate, "flops_per_filter_callback_as_built": fl["total"],
           "flops_by_kernel": fl, "achieved_tflops": rate * fl["total"] / 1e12, "peak_f64_tflops": PEAK_F64_TFLOPS,
           "fraction_of_f64_mfma_peak": rate * fl["total"] / 1e12 / PEAK_F64_TFLOPS,
           "launches_per_callback": core.launch_info()["launches_per_callback"], "kernel": core.kernel_info()["name"],
           "hbm_bytes": core.layout()[1], "timing": "device events around one aslam_replay, measured"}
    if with_oracle:
        r = oracle_rate(state, cap, oracle_steps)
        rec["oracle_filter_steps_per_s_one_core"] = r
        rec["speedup_over_oracle_one_core"] = rate / r
    core.close()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--landmarks", type=int, nargs="+", default=[142, 256, 512])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--oracle-steps", type=int, default=2, help="oracle callbacks timed per shape (2.3 s each at 512 landmarks)")
    ap.add_argument("--flops-only", action="store_true")
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps must be at least 20 steady-state callbacks")
    if a.flops_only:
        for L in a.landmarks:
            print(json.dumps({"landmarks": L, "n": 3 + 2 * L, "flops_by_kernel": chain_flops(3 + 2 * L)}))
        return
    import torch

    if not torch.cuda.is_available():
        sys.exit("ukf_large_rate: no GPU (there is no CPU fallback)")
    lines = []
    for L in a.landmarks:
        for i, B in enumerate(a.batches):
            rec = measure(L, B, a.steps, with_oracle=not a.no_oracle and i == 0, oracle_steps=a.oracle_steps)
            if i > 0 and "oracle_filter_steps_per_s_one_core" in lines[-i]:
                rec["oracle_filter_steps_per_s_one_core"] = lines[-i]["oracle_filter_steps_per_s_one_core"]
                rec["speedup_over_oracle_one_core"] = rec["filter_steps_per_s"] / rec["oracle_filter_steps_per_s_one_core"]
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
