#!/usr/bin/env python
"""bench.py -- filter-steps/s of the MI355X-native EKF/UKF-SLAM core on synthetic trajectories.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload ekf512|ekf64|ukf64|ekf8] [--batch B] [--chunk C]
                    [--scaling weak|strong --trajectories M] [--dump-outputs DIR] [--full [--no-sub] [--no-legs] [--cpu-sample S]]

Default workload: BASELINE.json configs[3] -- EKF, 512 landmarks (n = 1027), fp32 MFMA products, 256 trajectories per GPU
(the north-star configuration; the largest one that fits a single GPU).

A plain run sets up, warms up, times the K steps and prints the headline line (value, ms_per_step, the roofline of the timed
launches).  --full adds what the headline does not need: the check of the ekf512 fp32 filters against the fp64 path
(`parity_check`), the batch-1 latency and PCIe-inclusive legs, the configs[1] (ekf64) and configs[2] (ukf64) measurements as
sub-records (one GPU, each with its own roofline) and the CPU-oracle baselines.

--dump-outputs DIR: after the timed steps, what the timed path computed is written as DIR/<name>.npy (float64, at most 64 MB
in all): `poses` = the pose stream of the last timed step [filters, C, 3], `X` / `Z` = the final state vector and its landmark
ids per filter, `P` = the final covariance of a seeded sample of filters; `<name>_filters` lists the filters of an array that is
a sample.  The inputs are generated from --seed, so two runs with the same arguments see the same data.  Under --gpus N > 1
the dump holds rank 0's filters (trajectories 0 .. B-1).

One bench "step" = one replay launch = `chunk` consecutive callbacks (sensor message + odom message: association, growth
bookkeeping, predict, update) for each of the `batch` independent trajectories held by a GPU.  The trace is already resident
in HBM when the timed region starts.

--gpus N: one process per GPU.  Under torch.distributed.run the ranks are taken from the environment; started plainly
(`python bench.py --gpus N`, WORLD_SIZE unset) this process spawns the N rank processes itself, before it touches the GPU.
--scaling weak (default): every rank owns `batch` trajectories of its own.  --scaling strong --trajectories M: M trajectories
in total (configs[4]: 8), dealt to the ranks in contiguous blocks.  Either way the only communication is one all_gather of the
pose streams at the end of the timed region (RCCL over xGMI).

Prints ONE JSON line (rank 0).  The CPU oracle is used for the `cpu_baseline` leg (--full) and for nothing else.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (filter, landmarks, BASELINE.json config it corresponds to)
    "ekf512": ("ekf", 512, "configs[3]: EKF, 512 landmarks (n=1027), fp32 MFMA products, multi-workgroup launch chain"),
    "ekf64": ("ekf", 64, "configs[1]: EKF, 64 landmarks (n=131), fp64"),
    "ukf64": ("ukf", 64, "configs[2]: UKF, 64 landmarks (n=131), fp64"),
    "ekf8": ("ekf", 8, "configs[0] geometry on the GPU: EKF, 8 landmarks (n=19), fp64"),
}
# fp32 MFMA peak (MI355X_MICROARCH.md: 157.3 TFLOP/s, v_mfma_f32_16x16x4_f32 at the vector rate)
PEAK_F32_TFLOPS = 157.3
# fp64 peak: 256 CU x 4 SIMD x 16 FMA/clk x 2 x 2.4 GHz = 78.6 TFLOP/s, for v_fma_f64 and v_mfma_f64 alike
# (= half of the 157.3 TFLOP/s FP32 row of MI355X_MICROARCH.md, which lists no fp64 row of its own)
PEAK_F64_TFLOPS = 78.6
# binary32 products formed on the bf16 matrix pipe as six v_mfma_f32_16x16x32_bf16 per 16x16x32 product ("bf16x3"): the guide's dense bf16
# peak (2.5 PFLOP/s, 16 cycles per 16x16x32 instruction) / 6 = fp32-equivalent FLOP/s; tools/ubench/mfma_bf16x3.hip measures 308 T
PEAK_BF16X3_TFLOPS = 2516.6 / 6.0
# which pipe each third of the chain's 2.33 n^3 runs on (fractions of n^3): Cholesky of S, V = G L^-T, P -= V V^T
# (the library's kernel_info names the kernels of the chain it launches: `large_chol_bf16` / `large_trsm_bf16` are the bf16x3 forms)
EKF512_FLOPS_N3 = {"chol": 1.0 / 3.0, "trsm": 1.0, "syrk": 1.0}


def ekf512_pipes(kernel_name):
    pipe = lambda bf: "bf16x3" if bf else "fp32"
    return {"chol": (EKF512_FLOPS_N3["chol"], pipe("large_chol_bf16" in kernel_name)),
            "trsm": (EKF512_FLOPS_N3["trsm"], pipe("large_trsm_bf16" in kernel_name)),
            "syrk": (EKF512_FLOPS_N3["syrk"], pipe("large_syrk_bf16x3" in kernel_name))}
PEAK_HBM_GBPS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s peak (about 6.3 TB/s achievable)
UKF_MAX_CALLBACKS = 3000  # the reference UKF stays positive definite for a few thousand callbacks at n = 131
PROLOGUE = 64  # callbacks: the 42-callback warm-up in which the state grows to its full dimension, rounded up


def algorithmic_flops(kind, n):
    """reference-equivalent minimum per callback."""
    return (2.0 + 1.0 / 3.0) * n ** 3 if kind == "ekf" else 10.7 * n ** 3


def executed_flops(workload, n):
    """Flops the kernels actually issue per callback (padded tiles, structure-blind products), from the launch geometry."""
    if workload == "ekf512":
        # round-2 chain (binary32 products): large_chol_resident + large_trsm_pipe + large_syrk_bf16x3
        nb = (n + 1 + 63) // 64  # 64-blocks (row n of G carries Y^T)
        hist = 2.0 * 64 ** 3  # one history block: 4 waves x 64 MFMAs x 2048 flop
        close = hist * 10.0 / 16.0  # one closing block: the product with the lower-triangular (in 16-tiles) Linv_k, 40 MFMAs per wave
        f = (nb - 1) * nb * (nb + 1) / 6.0 * hist + nb * (nb - 1) / 2.0 * close  # Cholesky of S: block row I = I (I + 1) / 2 history blocks (incl. the diagonal chain) + I closing blocks
        f += nb * 2.0 * 64 ** 3 * (1.0 / 3.0 + 1.0 / 3.0)  # 64x64 diagonal factorisations + inverses
        f += nb * (nb * (nb - 1) / 2.0 * hist + nb * close)  # V = G L^-T: nb row blocks x (136 history + 17 closing blocks)
        nt = (nb * 64 + 127) // 128
        kend = min(nb * 64, (n + 31) // 32 * 32)
        f += (nt * (nt + 1) // 2 - nt * 0.25) * 2.0 * 128 * 128 * kend  # syrk lower tiles (upper quadrant of diagonal ones idle), K loop up to n
        return f
    np_ = 16 * ((n + 15) // 16)
    if workload in ("ekf64", "ekf8"):
        return 1.0 * np_ ** 3  # Cholesky + inverse of L + L^-T L^-1 on 16x16 tiles, n^3/3 each
    return algorithmic_flops("ukf", np_)  # the UKF kernel exploits the same structure the survey's figure assumes


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start the N rank processes (fresh children, nothing in this process has
    touched the GPU), relay rank 0's line, exit with the worst return code."""
    port = free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    deadline = time.time() + 3000
    pending = list(procs)
    while pending:
        for p in list(pending):
            code = p.poll()
            if code is not None:
                pending.remove(p)
                rc = rc or code
        if rc or time.time() > deadline:
            for p in pending:  # a rank failed: the others would wait in a collective for ever
                p.kill()
            rc = rc or 1
            break
        time.sleep(0.05)
    return rc


def cpu_baseline(kind, L, seed, sample):
    """The C++ oracle (Eigen-free restatement of the reference node, -O2, one core) on a bounded sample of the
    same workload: trajectory 0, `sample` steady-state callbacks after the warm-up prologue."""
    from oracle.cpu_bench import run

    r = run(kind, L, seed, 0, PROLOGUE, sample)
    el = r["t1"] - r["t0"]
    if L >= 256:
        what = (f"{sample} slam() calls (after one untimed call) on a synthetic state of the same dimension N={r['N']}; "
                f"oracle/aslam_oracle.cpp = the as-coded 18 n^3 dense algebra in fp64 as NAIVE TRIPLE LOOPS (an Eigen-free restatement, "
                f"not Eigen: the reference's own Eigen build would be several times faster), g++ -O2 (no auto-vectorisation), 1 thread, "
                f"{el:.1f} s; cpu_baseline_all_cores times further calls (SURVEY 8d asks for >= 20 in all)")
    else:
        what = (f"trajectory 0 of the same seed, {sample} steady-state callbacks after a {PROLOGUE}-callback "
                f"warm-up, N={r['N']}; oracle/aslam_oracle.cpp (as-coded 18 n^3 algebra), g++ -O2, 1 thread, {el:.1f} s")
    return {"value": sample / el, "unit": "filter-steps/s", "cores": 1, "kind": "port", "sample": what}


def cpu_baseline_all_cores(kind, L, seed, sample):
    """the reference node is single-threaded, so "all cores" = one trajectory per host core, one oracle
    process each (oracle/cpu_bench.py), same bounded sample per process; value = sum of the per-process rates."""
    if L >= 256:
        sample = max(2, sample // 4)  # n = 1027: seconds per call; 16 processes x 2 calls and the one-core leg's 8 make 40 timed calls
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    cores = max(1, min(cores, 16))  # a one-GPU box's CPU share is 16 cores, whatever the affinity mask says
    cmd = [sys.executable, "-m", "oracle.cpu_bench", "--kind", kind, "--landmarks", str(L), "--seed", str(seed),
           "--prologue", str(PROLOGUE), "--sample", str(sample)]
    procs = [subprocess.Popen(cmd + ["--traj", str(b)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
             for b in range(cores)]
    res = []
    for p_ in procs:
        out, _ = p_.communicate(timeout=600)
        if p_.returncode == 0 and out.strip():
            res.append(json.loads(out.strip().splitlines()[-1]))
    if not res:
        return None
    rate = sum(r["steps"] / (r["t1"] - r["t0"]) for r in res)
    span = max(r["t1"] for r in res) - min(r["t0"] for r in res)
    overlap = min(r["t1"] for r in res) - max(r["t0"] for r in res)
    return {"value": rate, "unit": "filter-steps/s", "cores": len(res), "kind": "port",
            "sample": f"{len(res)} oracle processes side by side, one trajectory each (trajectories 0..{len(res) - 1} of the same "
                      f"seed), {sample} callbacks per process; value = sum of per-process rates; timed sections span {span:.1f} s "
                      f"and overlap for {max(overlap, 0.0):.1f} s"}


def sub_records(seed):
    """configs[1] (ekf64) and configs[2] (ukf64) on the same clock as the default line, as sub-records with fixed shapes
    (whatever --steps/--warmup say; the UKF stays within the callbacks the reference UKF survives).  Each runs in a fresh
    process of its own, like a stand-alone `bench.py --workload ...`: measured in-process after the 5 GB configs[3] context the
    UKF launch took twice as long (profiles/r02_experiments.md)."""
    subs = {}
    for sw, sC, sK, sW in (("ekf64", 500, 4, 1), ("ukf64", 200, 10, 2)):
        cmd = [sys.executable, os.path.abspath(__file__), "--workload", sw, "--chunk", str(sC), "--steps", str(sK), "--warmup", str(sW),
               "--seed", str(seed), "--full", "--cpu-sample", "0", "--no-sub"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1200)
        if r.returncode != 0:
            raise SystemExit(f"bench sub-record {sw} failed:\n{r.stderr[-2000:]}")
        line = json.loads(r.stdout.strip().splitlines()[-1])
        subs[sw] = {"value": line["value"], "unit": line["unit"], "dtype": line["dtype"], "workload": line["config"]["workload"],
                    "trajectories_per_gpu": line["config"]["trajectories_per_gpu"], "callbacks_per_step": line["config"]["callbacks_per_step"],
                    "steps": line["steps"], "warmup": line["warmup"], "ms_per_step": line["ms_per_step"], "kernel": line["config"]["kernel"],
                    "roofline": line["roofline"], "single_trajectory": line.get("single_trajectory"),
                    "pcie_step_batch": line.get("pcie_step_batch")}
    return subs


def make_core(workload, B, tr, local):
    from awesomeslam_amd import trace as tg
    from awesomeslam_amd.core import Core, F32, F64

    kind, L, _ = WORKLOADS[workload]
    large = workload == "ekf512"
    return Core(kind, tg.dim_cap(L), batch=B, max_obs=tr.max_obs, max_wait=min(2048 if large else 512, 2 * L + 64), device=local,
                dtype=F32 if large else F64)


def pcie_step_batch(workload, seed, B, calls, local, dev):
    """The PCIe-inclusive rate of the per-callback seam: the host keeps association and growth and hands
    vx, az, dt, Z[n], A(0,0), A(1,0) of all `B` filters over per callback (aslam_*_step_batch: host arrays in, X[n] back, one
    launch chain, no synchronisation inside); `calls` back-to-back callbacks, one synchronisation at the end.  The filters are
    brought to their steady state through the replay seam first; the inputs are the same every call (the arithmetic does not
    depend on the values).  Never the headline `value`."""
    import numpy as np
    import torch
    from awesomeslam_amd import trace as tg

    kind, L, _ = WORKLOADS[workload]
    tr = tg.make_traces(L, PROLOGUE, B=B, seed=seed)
    core = make_core(workload, B, tr, local)
    core.set_trace(tr)
    scratch = torch.zeros((B, PROLOGUE, 3), dtype=torch.float64, device=dev)
    core.replay(0, PROLOGUE, scratch.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n = core.dim(0)
    pin = lambda a: torch.from_numpy(a).pin_memory().numpy()  # noqa: E731  (page-locked: the copies really are asynchronous)
    Z = np.zeros((B, n))
    a00, a10 = np.zeros(B), np.zeros(B)
    for b in range(B):
        Z[b] = core.state(b, with_P=False)[1][:n]
        a00[b], a10[b] = core.A(b)
    Z, a00, a10 = pin(Z), pin(a00), pin(a10)
    vx, az, dt = pin(np.full(B, 0.12, np.float32)), pin(np.full(B, 0.05, np.float32)), pin(np.full(B, 1.0, np.float32))
    X = pin(np.zeros((B, n)))
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        core.step_batch(vx, az, dt, Z, a00, a10, X_out=X, stream=stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        core.step_batch(vx, az, dt, Z, a00, a10, X_out=X, stream=stream)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    ok = bool(np.isfinite(X).all()) and core.status(0) == 0
    core.close()
    return {"value": B * calls / el, "unit": "filter-steps/s", "trajectories": B, "calls": calls, "us_per_call": el / calls * 1e6,
            "host_bytes_per_call": int(B * (3 * 4 + 8 * n + 16 + 8 * n)), "finite": ok,
            "what": "aslam_%s_step_batch: host arrays (pinned) -> HBM, one launch chain for all filters, X back; PCIe and launch cost included" % kind}


def single_trajectory_latency(workload, seed, C1, local, dev):
    """batch 1 is reported with every number (it is also the shape configs[4] runs at with one trajectory per
    GPU).  One filter alone on the GPU, `C1` steady-state callbacks in one launch (replay seam), HIP events on the launch
    stream; the second of two launches is reported."""
    import torch
    from awesomeslam_amd import trace as tg

    kind, L, _ = WORKLOADS[workload]
    tr = tg.make_traces(L, PROLOGUE + 2 * C1, B=1, seed=seed)
    core = make_core(workload, 1, tr, local)
    core.set_trace(tr)
    stream = torch.cuda.current_stream().cuda_stream
    scratch = torch.zeros((1, max(C1, PROLOGUE), 3), dtype=torch.float64, device=dev)
    core.replay(0, PROLOGUE, scratch.data_ptr(), None, stream)
    ms = []
    for w in range(2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        core.replay(PROLOGUE + w * C1, C1, scratch.data_ptr(), None, stream)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ok = core.dim(0) == tg.full_dim(L) and core.status(0) == 0
    core.close()
    return {"trajectories": 1, "callbacks_per_launch": C1, "us_per_callback": ms[1] * 1e3 / C1,
            "filter_steps_per_s": C1 / (ms[1] * 1e-3), "steady_state": bool(ok)}


DUMP_BUDGET = {"poses": 16 << 20, "X": 8 << 20, "Z": 8 << 20, "P": 32 << 20}  # bytes per array, 64 MB in all
DUMP_SEED = 20260101  # the fixed sample of filters an array is cut to when it exceeds its budget


def dump_filters(name, B, row_bytes):
    """The filters whose rows of array `name` are written: all of them when they fit DUMP_BUDGET[name], else a fixed seeded sample."""
    import numpy as np

    k = max(1, min(B, DUMP_BUDGET[name] // row_bytes))
    if k == B:
        return np.arange(B)
    return np.sort(np.random.default_rng(DUMP_SEED).choice(B, k, replace=False))


def dump_outputs(path, core, last_poses, n_full):
    """--dump-outputs: the last timed step's pose stream and the final filter states, as float64 .npy files under `path`."""
    import numpy as np

    os.makedirs(path, exist_ok=True)
    B = last_poses.shape[0]
    out = {}
    ids = dump_filters("poses", B, last_poses[0].nbytes)
    out["poses"] = (last_poses[ids], ids)
    ids = dump_filters("X", B, 8 * n_full)
    X, Z = np.full((len(ids), n_full), np.nan), np.full((len(ids), n_full), np.nan)
    for i, b in enumerate(ids):
        x, z, _ = core.state(int(b), with_P=False)
        X[i, :len(x)], Z[i, :len(z)] = x, z
    out["X"], out["Z"] = (X, ids), (Z, ids)
    ids = dump_filters("P", B, 8 * n_full * n_full)
    P = np.full((len(ids), n_full, n_full), np.nan)
    for i, b in enumerate(ids):
        p = core.state(int(b))[2]
        P[i, :p.shape[0], :p.shape[1]] = p
    out["P"] = (P, ids)
    for name, (a, ids) in out.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, np.float64))
        if len(ids) < B:
            np.save(os.path.join(path, name + "_filters.npy"), ids.astype(np.float64))


def measure(workload, B, C, K, W, seed, first_traj, rank, world, local, dev, full=False, dump=None):
    """W untimed + exactly K timed replay launches of `C` callbacks for this rank's `B` trajectories; barrier + synchronize on
    both sides of the timed region, one all_gather of the pose streams at its end, max over ranks of the elapsed time.
    full: the ekf512 fp32 filters are checked against the fp64 path afterwards.  dump: directory for --dump-outputs (rank 0).
    Returns (elapsed_s, mean launch duration by HIP events in s, kernel info, trace_gen_s)."""
    import numpy as np
    import torch
    from awesomeslam_amd import dist as adist
    from awesomeslam_amd import trace as tg

    kind, L, _ = WORKLOADS[workload]
    n_full = tg.full_dim(L)
    T = PROLOGUE + (W + K) * C
    t_gen = time.time()
    tr = tg.make_traces(L, T, B=B, seed=seed, first_traj=first_traj)
    t_gen = time.time() - t_gen
    core = make_core(workload, B, tr, local)
    core.set_trace(tr)
    # filters whose final state is compared with the fp64 path after the timed region (ekf512): one inside the first stream group, one
    # with an index >= 8 inside a later group, the last one of the batch
    check_ids = sorted({min(3, B - 1), min(B - 1, B // 4 + 13), B - 1}) if workload == "ekf512" and full else []
    check_tr = tr.select(check_ids) if check_ids else None
    del tr
    stream = torch.cuda.current_stream().cuda_stream
    poses = torch.zeros((K, B, C, 3), dtype=torch.float64, device=dev)
    scratch = torch.zeros((B, max(C, PROLOGUE), 3), dtype=torch.float64, device=dev)

    core.replay(0, PROLOGUE, scratch.data_ptr(), None, stream)
    torch.cuda.synchronize()
    probe = range(0, B, max(1, B // 8))
    for b in probe:
        if core.dim(b) != n_full or core.status(b) != 0:
            raise SystemExit(f"trajectory {b}: N={core.dim(b)} (want {n_full}), status={core.status(b)} after the warm-up")
    for w in range(W):
        core.replay(PROLOGUE + w * C, C, scratch.data_ptr(), None, stream)
    adist.gather_poses(scratch[:, :1])  # the collective once, untimed: communicator and buffers exist when the clock starts
    torch.cuda.synchronize()

    # ---- timed region: exactly K steps, barrier + synchronize on both sides
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(K)]
    adist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(K):
        ev[k][0].record()
        core.replay(PROLOGUE + (W + k) * C, C, poses[k].data_ptr(), None, stream)
        ev[k][1].record()
    all_poses = adist.gather_poses(poses.permute(1, 0, 2, 3).reshape(B, K * C, 3))  # the one collective: poses, at the end
    torch.cuda.synchronize()
    adist.barrier()
    el = time.perf_counter() - t0
    el = adist.max_over_ranks(el, dev if world > 1 else "cpu")
    kernel_s = float(np.mean([a.elapsed_time(b) for a, b in ev])) * 1e-3

    ok = all(core.dim(b) == n_full and core.status(b) == 0 for b in probe)
    finite = bool(torch.isfinite(all_poses).all().item())
    if not (ok and finite):
        raise SystemExit(f"bench {workload}: a filter left its steady state (dimension/status/non-finite pose)")
    info = core.kernel_info()
    info["launch"] = core.launch_info()
    if dump and rank == 0:
        dump_outputs(dump, core, poses[K - 1].cpu().numpy(), n_full)
    finals = {b: core.state(b) for b in check_ids}
    core.close()
    del poses, scratch, all_poses
    torch.cuda.empty_cache()
    info["parity_check"] = parity_check(workload, check_ids, check_tr, finals, T, local) if check_ids else None
    return el, kernel_s, info, t_gen


PARITY_BAR = 1e-6  # the north-star tolerance: X, and P norm-wise
PARITY_BAR_BLOCK = 1e-6  # P block-wise (tests/util.py::block_rel_err: pose 3x3, cross, landmark block, each against its own maximum) = F32_DRIFT_TOL of tests/test_gpu_large.py


def parity_check(workload, ids, tr, finals, T, local):
    """After the timed region: the final X and P of a few of the benchmarked fp32 filters against the SAME trajectories replayed through the
    fp64 large path of this library (itself within 1e-13 of the CPU oracle at n = 1027: tests/test_gpu_large.py).  The benchmark fails
    if a filter that the timed launches should have advanced was skipped, mis-indexed or came out beyond the bar."""
    import numpy as np
    import torch
    from awesomeslam_amd import trace as tg
    from awesomeslam_amd.core import Core, F64

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from util import block_rel_err, rel_err

    kind, L, _ = WORKLOADS[workload]
    ref = Core(kind, tg.dim_cap(L), batch=len(ids), max_obs=tr.max_obs, max_wait=min(2048, 2 * L + 64), device=local, dtype=F64)
    ref.set_trace(tr)
    ref.replay(0, T, None, None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    worst_x = worst_p = worst_blk = 0.0
    for i, b in enumerate(ids):
        Xr, Zr, Pr = ref.state(i)
        X, Z, P = finals[b]
        if X.shape != Xr.shape or not np.array_equal(Z, Zr):
            raise SystemExit(f"bench parity check: filter {b} has dimension {X.shape[0]} / Z differs from the fp64 path ({Xr.shape[0]})")
        worst_x, worst_p, worst_blk = max(worst_x, rel_err(X, Xr)), max(worst_p, rel_err(P, Pr)), max((worst_blk,) + block_rel_err(P, Pr))
    ref.close()
    torch.cuda.empty_cache()
    ok = bool(worst_x < PARITY_BAR and worst_p < PARITY_BAR and worst_blk < PARITY_BAR_BLOCK)
    return {"filters": ids, "callbacks": int(T), "x_rel_err": worst_x, "p_rel_err": worst_p, "p_block_rel_err": worst_blk,
            "bar": PARITY_BAR, "bar_block": PARITY_BAR_BLOCK, "ok": ok,
            "against": "the same trajectories through this library's fp64 large path (checked against the CPU oracle at 1e-6 in tests/test_gpu_large.py); "
                       "p_rel_err norm-wise, p_block_rel_err the worst of the pose 3x3, pose-landmark and landmark blocks, each against its own maximum"}


def roofline(workload, B, C, kernel_s, kernel_name=""):
    from awesomeslam_amd import trace as tg

    kind, L, _ = WORKLOADS[workload]
    n = tg.full_dim(L)
    large = workload == "ekf512"
    peak = PEAK_F32_TFLOPS if large else PEAK_F64_TFLOPS
    achieved = algorithmic_flops(kind, n) * B * C / kernel_s / 1e12
    executed = executed_flops(workload, n) * B * C / kernel_s / 1e12
    # PMC traffic is a stored measurement (profiles/pmc_traffic.json, separate --pmc passes): it is reported only when the entry was taken on
    # the SAME kernel chain this run launched (the entry's "kernel" must equal aslam_kernel_info's name); otherwise traffic is null
    traffic, traffic_note = None, None
    tj = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(tj):
        try:
            ent = json.load(open(tj)).get(workload, {})
            if ent.get("kernel") != kernel_name:
                traffic_note = f"profiles/pmc_traffic.json[{workload}] was measured on kernel {ent.get('kernel')!r}, this run launched {kernel_name!r}: not reported"
            else:
                traffic = ent.get("hbm_bytes_per_launch")
                if traffic is not None and ent.get("trajectories") and ent.get("callbacks_per_launch"):
                    # the PMC passes are per launch of the shape they were taken at: scale to this launch's callbacks x trajectories
                    traffic = traffic * (B * C) / (ent["trajectories"] * ent["callbacks_per_launch"])
        except Exception as e:  # noqa: BLE001
            traffic, traffic_note = None, f"profiles/pmc_traffic.json unreadable: {e}"
    mixed = None
    if large:
        # ADVICE / VERDICT round 2: `frac` divides fp32-equivalent flops by the fp32 MFMA peak although part of them runs on the (faster) bf16
        # pipe.  mixed_pipe_frac = the time the algorithmic flops would take at the peak of the pipe each part really uses / the measured time.
        pipes = ekf512_pipes(kernel_name)
        t_ideal = sum(f * n ** 3 / ((PEAK_F32_TFLOPS if pipe == "fp32" else PEAK_BF16X3_TFLOPS) * 1e12) for f, pipe in pipes.values())
        mixed = {"frac": t_ideal * B * C / kernel_s, "fp32_equivalent": True,
                 "pipes": {k: {"flops_n3": f, "pipe": pipe, "peak_tflops": PEAK_F32_TFLOPS if pipe == "fp32" else PEAK_BF16X3_TFLOPS}
                           for k, (f, pipe) in pipes.items()},
                 "note": "time of the 2.33 n^3 algorithmic flops at the peaks of the pipes they run on (fp32 MFMA 157.3 T; bf16x3 = dense bf16 "
                         "peak / 6 = 419 T fp32-equivalent, 308 T measured by tools/ubench/mfma_bf16x3.hip) / measured launch time"}
    return {"bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
            "executed_frac": executed / peak, "mixed_pipe_frac": None if mixed is None else mixed["frac"], "mixed_pipe": mixed, "traffic": traffic, "traffic_note": traffic_note,
            # the other roofline north_star asks for: PMC bytes at the L2's memory side per launch / launch time
            "hbm": None if traffic is None else {"achieved": traffic / kernel_s / 1e9, "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                                                 "frac": traffic / kernel_s / 1e9 / PEAK_HBM_GBPS},
            "kernel_ms": kernel_s * 1e3,
            "note": "achieved = SURVEY 8(d) algorithmic flops per callback (EKF 2.33 n^3, UKF 10.7 n^3: the reference-equivalent "
                    "minimum the survey defines) x callbacks x trajectories per launch / mean launch duration (HIP events on the "
                    "launch stream); executed_frac = the same with the flops the kernels really issue (padded tiles; the single-CU EKF "
                    "update needs only S^-1 since R = r I: about n^3); peak = dense " + ("fp32" if large else "fp64")
                    + " MFMA rate (MI355X_MICROARCH.md); traffic = PMC bytes at the L2's memory side (profiles/pmc_traffic.json)"
                    + ("; the products of the kernels mixed_pipe lists as bf16x3 (all 2.33 n^3 with the default chain) are binary32 products formed on the bf16 matrix pipe -- every float split "
                       "exactly into three bf16 pieces, six v_mfma_f32_16x16x32_bf16 per 16x16x32 product, fp32 accumulation: twice the fp32 MFMA "
                       "rate at a smaller error (tools/ubench/mfma_bf16x3.hip) -- and are counted as the fp32 flops they replace; the peak stays the "
                       "fp32 MFMA figure the path's arithmetic type names" if large else "")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="ekf512", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=None, help="trajectories per GPU (weak scaling; default 256)")
    ap.add_argument("--chunk", type=int, default=None,
                    help="callbacks per launch (= per bench step); default 20 (ekf512) / 500 (EKF) / 200 (UKF, capped so that a "
                         "run stays within the 3000 callbacks the reference UKF survives)")
    ap.add_argument("--scaling", default="weak", choices=("weak", "strong"))
    ap.add_argument("--trajectories", type=int, default=8, help="total trajectories under --scaling strong (configs[4]: 8)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--full", action="store_true",
                    help="also the fp32-vs-fp64 parity check, the batch-1 latency and PCIe-inclusive legs, the ekf64 / ukf64 sub-records "
                         "and the CPU-oracle baselines (a plain run does only what the headline figure needs)")
    ap.add_argument("--cpu-sample", type=int, default=None, help="with --full: callbacks timed on the CPU oracle (0 = skip)")
    ap.add_argument("--no-sub", action="store_true", help="with --full: skip the ekf64 / ukf64 sub-records")
    ap.add_argument("--no-legs", action="store_true",
                    help="with --full: skip the batch-1 latency and PCIe-inclusive legs (the timed steps are then the last launches)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's poses and the final filter states as DIR/<name>.npy (float64, <= 64 MB)")
    args = ap.parse_args()

    if args.gpus > 1 and os.environ.get("ASLAM_DIST_BACKEND") != "gloo":
        # one process per GPU over RCCL: more ranks than devices cannot work (two ranks on one device deadlock in the communicator set-up);
        # ASLAM_DIST_BACKEND=gloo is the rehearsal in which ranks share devices.  torch.cuda.device_count() does not initialise the GPU.
        import torch

        if torch.cuda.device_count() == 0:
            raise SystemExit("bench.py needs a GPU: the filter core has no CPU fallback")
        if args.gpus > torch.cuda.device_count():
            raise SystemExit(f"bench.py --gpus {args.gpus}: this node has {torch.cuda.device_count()} GPU(s); one rank per GPU over RCCL needs "
                             f"{args.gpus}.  (ASLAM_DIST_BACKEND=gloo rehearses the multi-process path with ranks sharing devices.)")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(args.gpus))

    subs = None
    if args.full and args.gpus == 1 and args.workload == "ekf512" and args.scaling == "weak" and not args.no_sub:
        subs = sub_records(args.seed)  # fresh processes, before this one touches the GPU

    import torch
    from awesomeslam_amd import dist as adist
    from awesomeslam_amd import trace as tg

    rank, world, local = adist.init()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the filter core has no CPU fallback")
    local = local % torch.cuda.device_count()  # ranks share devices only in the gloo rehearsal (ASLAM_DIST_BACKEND=gloo)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    wl = args.workload
    kind, L, cfg_name = WORKLOADS[wl]
    n_full = tg.full_dim(L)
    large = wl == "ekf512"
    K, W = args.steps, args.warmup
    C = args.chunk if args.chunk is not None else (20 if large else 200 if kind == "ukf" else 500)
    if kind == "ukf":
        C = max(1, min(C, (UKF_MAX_CALLBACKS - PROLOGUE) // (K + W)))
    if args.scaling == "strong":
        if args.trajectories % world:
            raise SystemExit(f"--trajectories {args.trajectories} does not divide over {world} ranks")
        B = args.trajectories // world
        cfg_name = cfg_name.replace("configs[3]", "configs[4]") + f"; {args.trajectories} trajectories in total"
    else:
        B = args.batch if args.batch is not None else 256
    first_traj = rank * B

    el, kernel_s, info, t_gen = measure(wl, B, C, K, W, args.seed, first_traj, rank, world, local, dev, full=args.full, dump=args.dump_outputs)

    if rank == 0:
        total_steps = world * B * C * K
        out = {
            "metric": "EKF/UKF filter-steps/s @ N_landmarks", "value": total_steps / el, "unit": "filter-steps/s",
            "n_gpus": world, "steps": K, "warmup": W, "ms_per_step": el / K * 1e3, "higher_is_better": True,
            "scaling": args.scaling, "vs_baseline": None, "dtype": "f32" if large else "f64", "data": "synthetic",
            "config": {"workload": f"{wl} = {cfg_name}", "landmarks": L, "state_dim": n_full,
                       "trajectories_per_gpu": B, "trajectories_total": world * B, "callbacks_per_step": C,
                       "parallelism": f"trajectory-sharded x{world}",
                       "kernel": info["name"], "grid": info["grid"], "block": info["block"], "lds_bytes": info["lds_bytes"],
                       "trace_gen_s": round(t_gen, 1)},
            "roofline": roofline(wl, B, C, kernel_s, info["name"]),
        }
        if info.get("launch"):
            out["config"]["launch"] = info["launch"]
        if info.get("parity_check") is not None:
            out["parity_check"] = info["parity_check"]
            if not info["parity_check"]["ok"]:
                print(json.dumps(out), flush=True)
                raise SystemExit("bench: fp32 filters beyond the parity bar against the fp64 path: " + json.dumps(info["parity_check"]))
        if world == 1 and args.full:
            if not args.no_legs:
                out["single_trajectory"] = single_trajectory_latency(wl, args.seed, min(C, 200), local, dev)
                out["pcie_step_batch"] = pcie_step_batch(wl, args.seed, min(B, 256), 10 if large else 100, local, dev)
            if subs:
                out["sub"] = subs
            sample = args.cpu_sample
            if sample is None:
                sample = {"ekf64": 1200, "ukf64": 1000, "ekf8": 20000, "ekf512": 8}[wl]
            if sample > 0:
                out["cpu_baseline"] = cpu_baseline(kind, L, args.seed, sample)
                allc = cpu_baseline_all_cores(kind, L, args.seed, sample)
                if allc:
                    out["cpu_baseline_all_cores"] = allc
        print(json.dumps(out), flush=True)
    adist.finalize()


if __name__ == "__main__":
    main()
