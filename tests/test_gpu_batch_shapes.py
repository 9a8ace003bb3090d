"""-m gpu: batches whose filters are NOT alike.  Every kernel of the large-state chain reads the dimension and the skip flag of its own filter
and stops at its own block count; the rest of the suite mostly runs batches whose filters share one dimension and one message timing, so a
kernel that took either from a neighbour would pass it.  Here:

  A. every state dimension of a capacity in ONE shuffled batch (large path, every binary32 chain and fp64), one step against NumPy;
  B. the same for the single-CU kernels (EKF and UKF, fp64), every dimension of the three tile counts;
  C. a replay in which each filter's first sensor message comes at a different callback (dropped callbacks next to active ones, dimensions
     that differ at most callbacks), started on a context that has run before;
  D. the benchmarked shape (256 filters, n = 1027, default chain) on DISTINCT trajectories against the fp64 chain;
  E. the status bits of the large path (wait-list overflow on both paths, refused growth, an over-long message).

The states of A and B are marginals of real filter states (one fp64 replay to n = 1087, one UKF replay to n = 143): every leading principal
block of an SPD covariance is SPD, so one replay gives a realistic state of every dimension.  A hand-over through aslam_set_state to a
SMALLER dimension leaves the scratch of the larger one behind, so each batch first runs one step with the assignment reversed."""
import numpy as np
import pytest

from awesomeslam_amd import trace as tg
from test_gpu_large import F32_TOL, chol_mode
from util import block_rel_err, cov_err, rel_err

pytestmark = pytest.mark.gpu

# fp64 bars: one callback from a handed-over state, and replays -- far below util.REL_TOL; the existing tests print <= 3e-14 (n = 1027)
STEP_TOL = 1e-10
REPLAY_TOL = 1e-9
# the chains of the large path, forced through the environment (test_gpu_large.chol_mode); "f32-resident" is the default of bench.py
LARGE_CHAINS = ["f64", "f32", "f32-left", "f32-resident-pipe0", "f32-resident-pipe1", "f32-resident-pipe2", "f32-resident"]
KNOBS = ("ASLAM_CHOL_RESIDENT", "ASLAM_RIGHT_STEP", "ASLAM_BF16_PIPE", "ASLAM_LARGE_GROUPS", "ASLAM_GS_TILES", "ASLAM_KEEP_L32", "ASLAM_SYRK_RUNNING")


def _sync():
    import torch

    torch.cuda.synchronize()


def expected_launch(dtype, B):
    """(stream groups, resident Cholesky) the library must report for `B` filters of chain `dtype` (ekf_large_launch.h: one group below 32 filters)"""
    return (1 if B < 32 else 3), (dtype.startswith("f32") and "-resident" in dtype)


def odd_dims(lo, hi):
    return list(range(lo | 1, hi + 1, 2))


def dims_1088():
    """every odd n <= 199, and the odd n from 64 k - 5 to 64 k + 3 (k = 4 .. 17) up to 1087: 167 filters"""
    dims = odd_dims(3, 199)
    for k in range(4, 18):
        dims += [n for n in range(64 * k - 5, 64 * k + 4, 2) if n <= 1087]
    return dims


# capacity (max_landmark_count) -> the dimensions of its batch.  NP = 1088 (17 blocks), 64 (one block: the 128-row syrk tile hangs over the
# end), 128.  66 admits every odd n <= 65: 32 filters, so 65 is there twice to keep the batch off a multiple of 8
LARGE_BATCHES = {1088: dims_1088(), 64: odd_dims(3, 63), 66: odd_dims(3, 65) + [65]}
SMALL_BATCHES = {32: odd_dims(3, 31), 80: odd_dims(3, 79), 144: odd_dims(3, 143)}  # NT = 2, 5, 9


def shuffled(dims, seed, last=None):
    """a fixed permutation; `last` (if given) goes to the last filter"""
    d = list(np.random.default_rng(seed).permutation(dims))
    if last is not None:
        d.remove(last)
        d.append(last)
    assert len(d) % 8, "the last stream group must be partial"
    return [int(n) for n in d]


def spd(P):
    np.linalg.cholesky(P)  # raises on a matrix that is not SPD
    return True


# ---------------------------------------------------------------------------------------------------- base states and references


@pytest.fixture(scope="module")
def ekf_base(built):
    """(X, Z, P, a00, a10) of one fp64 large-path replay to n = 1087; P symmetrised"""
    from awesomeslam_amd.core import Core, F64

    L = 542
    tr = tg.make_traces(L, 48, B=1)
    core = Core("ekf", tg.dim_cap(L), batch=1, max_obs=tr.max_obs, max_wait=2048, dtype=F64)
    core.set_trace(tr)
    core.replay(0, tr.T)
    _sync()
    assert core.dim(0) == 1087 and core.status(0) == 0
    X, Z, P = core.state(0)
    a00, a10 = core.A(0)
    core.close()
    return X, Z, (P + P.T) / 2, a00, a10


@pytest.fixture(scope="module")
def ukf_base(built):
    """(X, Z, P) of one UKF replay to n = 143 (the scenario of tests/test_gpu_ukf.py, L70-max); P symmetrised"""
    from awesomeslam_amd.core import Core

    L = 70
    tr = tg.make_traces(L, 80, B=1, seed=47)
    core = Core("ukf", tg.dim_cap(L), batch=1, max_obs=tr.max_obs, max_wait=256)
    core.set_trace(tr)
    core.replay(0, tr.T)
    _sync()
    assert core.dim(0) == 143 and core.status(0) == 0
    X, Z, P = core.state(0)
    core.close()
    return X, Z, (P + P.T) / 2


def ukf_synthetic(n):
    """the synthetic scenario of tests/test_gpu_ukf.py::test_single_slam_on_synthetic_state (landmarks east of the robot, small covariance)"""
    rng = np.random.default_rng(100 + n)
    L = (n - 3) // 2
    X = np.concatenate([[0.3, -0.2, 0.4], (np.array([25.0, 0.0]) + 4 * rng.normal(size=(L, 2))).ravel()])
    A = rng.normal(size=(n, n)) * 0.01
    P = A @ A.T + np.eye(n) * 0.002
    Z = X.copy()
    for i in range(L):
        dx, dy = X[3 + 2 * i] - X[0], X[4 + 2 * i] - X[1]
        Z[3 + 2 * i] = np.float32(np.hypot(dx, dy) + 0.01 * rng.normal())
        Z[4 + 2 * i] = np.float32(np.arctan2(dy, dx) - X[2] + 0.002 * rng.normal())
    return X, Z, P


def step_inputs(kind, dims, states, seed, steps=2):
    """per step: vx, az, dt [B] f32, a00, a10 [B] f64, Z [B, ldz] with ldz > every n and junk past each filter's n (only the first n
    entries of a row are the filter's, include/aslam_core.h); every filter gets inputs of its own"""
    rng = np.random.default_rng(seed)
    B = len(dims)
    ldz = max(dims) + 5
    out = []
    for s in range(steps):
        vx = (0.05 + 0.15 * rng.random(B)).astype(np.float32)
        az = ((rng.random(B) - 0.5) * (0.0 if s == 1 else 0.4)).astype(np.float32)  # the second step takes the straight-line branch
        dt = (0.2 + 0.8 * rng.random(B)).astype(np.float32)
        Z = np.empty((B, ldz))
        a00, a10 = np.empty(B), np.empty(B)
        for b, n in enumerate(dims):
            Zb = states[n][1].copy()
            if s:  # new readings for the second step (binary32 values, as the node stores them)
                Zb[3:] = (Zb[3:] + 0.01 * rng.normal(size=n - 3)).astype(np.float32)
            Z[b, :n] = Zb
            Z[b, n:] = 1e3 + np.arange(ldz - n)
            if kind == "ekf":
                a00[b] = states[n][3] * (1 + 0.2 * rng.random())
                a10[b] = states[n][4] * (1 + 0.2 * rng.random())
        out.append((vx, az, dt, a00, a10, np.ascontiguousarray(Z)))
    return out


def np_reference(kind, dims, states, inputs):
    """NumPy oracle (plain binary64 BLAS / LAPACK): set_state, then one slam() per step with that step's Z (and A); per filter the X after
    each step and the final (X, P)"""
    from oracle.np_oracle import NpFilter

    xs, finals = [[] for _ in inputs], []
    for b, n in enumerate(dims):
        X, Z, P = states[n][:3]
        f = NpFilter(kind, n + 1)
        f.set_state(n, X, Z, P, *((states[n][3], states[n][4]) if kind == "ekf" else ()))
        for s, (vx, az, dt, a00, a10, Zs) in enumerate(inputs):
            f.Z = Zs[b, :n].copy()
            if kind == "ekf":
                f.A[0, 0], f.A[1, 0] = a00[b], a10[b]
            f.slam(vx[b], az[b], dt[b])
            assert np.isfinite(f.X).all() and np.isfinite(f.P).all(), (n, s)
            if kind == "ukf":  # the reference UKF stays PD on these states (asserted: a comparison of NaNs proves nothing)
                assert np.linalg.eigvalsh((f.P + f.P.T) / 2).min() > 0, (n, s)
            xs[s].append(f.X.copy())
        finals.append((f.X.copy(), f.P.copy()))
    return xs, finals


class RefCache:
    """module-wide: states, inputs and NumPy results, computed once per (kind, capacity) and shared by every chain"""

    def __init__(self, ekf, ukf):
        self.base, self.cache = {"ekf": ekf, "ukf": ukf}, {}

    def states(self, kind, dims):
        X, Z, P = self.base[kind][:3]
        st = {}
        for n in sorted(set(dims)):
            st[n] = (X[:n].copy(), Z[:n].copy(), P[:n, :n].copy()) + tuple(self.base[kind][3:])
            assert spd(st[n][2]), (kind, n)
        return st

    def get(self, kind, cap, dims, seed):
        key = (kind, cap)
        if key not in self.cache:
            st = self.states(kind, dims)
            fallback = []
            while True:
                inp = step_inputs(kind, dims, st, seed)
                try:
                    ref = np_reference(kind, dims, st, inp)
                    break
                except AssertionError as e:  # (UKF) a dimension whose reference step leaves the PD cone takes the synthetic scenario
                    n = e.args[0][0] if kind == "ukf" and e.args and isinstance(e.args[0], tuple) else None
                    if n is None or n in fallback:
                        raise
                    st[n] = ukf_synthetic(n)
                    fallback.append(n)
            rev = step_inputs(kind, dims[::-1], st, seed + 1, steps=1)
            self.cache[key] = (st, rev, inp, ref, fallback)
        return self.cache[key]


@pytest.fixture(scope="module")
def refs(ekf_base, ukf_base):
    return RefCache(ekf_base, ukf_base)


def run_assignment(core, kind, dims, st, rev, inp):
    """one step with the assignment reversed (every filter's scratch then holds another dimension's data), set_state to the tested
    assignment, two steps; returns X_out of each step"""
    B = len(dims)
    for b, n in enumerate(dims[::-1]):
        core.set_state(b, n, *st[n][:3])
    vx, az, dt, a00, a10, Z = rev[0]
    core.step_batch(vx, az, dt, Z, a00, a10) if kind == "ekf" else core.step_batch(vx, az, dt, Z)
    _sync()
    for b, n in enumerate(dims):
        core.set_state(b, n, *st[n][:3])
    xs = []
    for vx, az, dt, a00, a10, Z in inp:
        X_out = np.zeros((B, Z.shape[1] + 2))
        core.step_batch(vx, az, dt, Z, a00, a10, X_out=X_out) if kind == "ekf" else core.step_batch(vx, az, dt, Z, X_out=X_out)
        _sync()
        xs.append(X_out)
    return xs


def check_batch(core, dims, xs, ref, tol, what):
    """X_out of both steps, X and P of every filter against the reference; status clear; returns the worst (X, P) figures"""
    ref_xs, finals = ref
    wx = wp = 0.0
    worst = None
    for b, n in enumerate(dims):
        for s in range(len(xs)):
            e = rel_err(xs[s][b, :n], ref_xs[s][b])
            wx = max(wx, e)
            assert e < tol, f"{what}: X_out of step {s}, filter {b} (n = {n}): {e:.2e}"
        assert core.dim(b) == n and core.status(b) == 0, (what, b, n, core.status(b))
        X, _, P = core.state(b)
        ex, ep = rel_err(X, finals[b][0]), cov_err(P, finals[b][1])
        if ep > wp:
            worst = (n, block_rel_err(P, finals[b][1]))
        wx, wp = max(wx, ex), max(wp, ep)
        assert ex < tol and ep < tol, f"{what}: filter {b} (n = {n}): X {ex:.2e} P {ep:.2e} (blocks {block_rel_err(P, finals[b][1])})"
    return wx, wp, worst


# ---------------------------------------------------------------------------------------------------- A


A_CASES = [(d, 1088) for d in LARGE_CHAINS] + [(d, cap) for cap in (64, 66) for d in LARGE_CHAINS if d != "f64"]  # binary32 only below 146


@pytest.mark.parametrize("dtype,cap", A_CASES, ids=[f"{d}-cap{c}" for d, c in A_CASES])
def test_every_dimension_in_one_batch(dtype, cap, refs, monkeypatch):
    """Every dimension of a capacity in ONE batch of the large path, shuffled (n = 1087 on the last filter of NP = 1088), after a step with
    the assignment reversed: one fp64 reference step per filter from NumPy, X_out of both steps, X and P (norm-wise and block-wise)."""
    from awesomeslam_amd.core import Core, F32, F64

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    dt = chol_mode(dtype, monkeypatch)
    dims = shuffled(LARGE_BATCHES[cap], seed=cap, last=1087 if cap == 1088 else None)
    st, rev, inp, ref, _ = refs.get("ekf", cap, dims, seed=7 + cap)
    core = Core("ekf", cap, batch=len(dims), max_obs=4, max_wait=4, dtype=F32 if dt == "f32" else F64)
    try:
        assert core.layout()[0] == {1088: 1088, 64: 64, 66: 128}[cap]
        xs = run_assignment(core, "ekf", dims, st, rev, inp)
        info = core.launch_info()
        groups, resident = expected_launch(dtype, len(dims))
        assert info["stream_groups"] == groups and info["chol_resident"] == resident, info
        tol = STEP_TOL if dt == "f64" else F32_TOL
        wx, wp, worst = check_batch(core, dims, xs, ref, tol, f"{dtype} cap {cap}")
        print(f"every dimension in one batch, {dtype} NP={core.layout()[0]} B={len(dims)}: worst rel err X {wx:.2e} P {wp:.2e} "
              f"(n = {worst[0]}: blocks pose/cross/landmark {worst[1][0]:.2e} {worst[1][1]:.2e} {worst[1][2]:.2e}); launch {info}")
    finally:
        core.close()


# ---------------------------------------------------------------------------------------------------- B


@pytest.mark.parametrize("cap", sorted(SMALL_BATCHES))
@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_every_dimension_small_kernels(kind, cap, refs):
    """The single-CU kernels (fp64) with every dimension their tile count admits in one shuffled batch (n = 31 under NT = 2, n = 79 under
    NT = 5 included), after a step with the assignment reversed: the scratch of the UKF (D, DZ, Tc, K) then holds rows of a larger state."""
    from awesomeslam_amd.core import Core

    dims = shuffled(SMALL_BATCHES[cap], seed=cap)
    st, rev, inp, ref, fallback = refs.get(kind, cap, dims, seed=11 + cap)
    core = Core(kind, cap, batch=len(dims), max_obs=4, max_wait=4)
    try:
        assert core.layout()[0] == cap // 16 * 16 and core.kernel_info()["name"].startswith(kind)
        xs = run_assignment(core, kind, dims, st, rev, inp)
        wx, wp, worst = check_batch(core, dims, xs, ref, STEP_TOL, f"{kind} cap {cap}")
        print(f"every dimension of the single-CU {kind} kernel, NP={core.layout()[0]} B={len(dims)}: worst rel err X {wx:.2e} P {wp:.2e} "
              f"(n = {worst[0]}: blocks {worst[1][0]:.2e} {worst[1][1]:.2e} {worst[1][2]:.2e})"
              + (f"; synthetic states at n = {fallback}" if fallback else ""))
    finally:
        core.close()


# ---------------------------------------------------------------------------------------------------- C


def delayed_trace(L, T, B, seed, rotate):
    """make_traces with filter b's first sensor message held back by k_b callbacks, k_b cycling through DELAYS (shifted by `rotate`)"""
    tr = tg.make_traces(L, T, B=B, seed=seed)
    delays = (0, 1, 2, 13, 14, 15, 40, T)
    ks = [delays[(b + rotate) % len(delays)] for b in range(B)]
    for b, k in enumerate(ks):
        tr.obs_new[b, :k] = 0
    return tr, ks


@pytest.fixture(scope="module")
def lag_oracles(built):
    """CFilter replays of the delayed trajectories, per filter index (trajectory b and its delay do not depend on the batch size)"""
    from oracle.c_oracle import CFilter

    cache = {}

    def get(L, T, B, seed, ids):
        tr, ks = delayed_trace(L, T, B, seed, 0)
        for b in ids:
            if b not in cache:
                o = CFilter("ekf", tg.dim_cap(L))
                po, do = o.replay(tr[b])
                cache[b] = (po, do, o.state(), o.wait_list())
                assert len(cache[b][3][0]) < 2048, "the scenario must stay within the wait-list capacity of the context"
        return tr, ks, {b: cache[b] for b in ids}

    return get


@pytest.mark.parametrize("dtype", LARGE_CHAINS)
def test_replay_with_skipped_and_lagging_filters(dtype, lag_oracles, monkeypatch):
    """Each filter's first sensor message at its own callback (k_b in {0, 1, 2, 13, 14, 15, 40, T}): callbacks dropped by the front end
    (skipped[b]) run next to active filters at every stage of growth, and the batch's dimensions differ at most callbacks.  The checked replay
    (two launches) starts on a context that has replayed other delays and been reset (stale planes, Y, Linv).  Bookkeeping bit-exact against
    the oracle, poses / X / P within the bars; a filter that never receives a message is exactly as initialize() left it."""
    import torch
    from awesomeslam_amd.core import Core, F32, F64

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    dt = chol_mode(dtype, monkeypatch)
    L, T, seed = 100, 80, 67
    B = 37 if "-resident" in dtype else 12  # 37: stream groups of 16, 16 and 5
    ids = list(range(B)) if B == 12 else [0, 1, 2, 3, 4, 5, 6, 15, 16, 31, 32, 36]  # every k_b, both ends of every group
    tr, ks, ref = lag_oracles(L, T, B, seed, ids)
    rot, _ = delayed_trace(L, T, B, seed, 1)
    core = Core("ekf", tg.dim_cap(L), batch=B, max_obs=tr.max_obs, max_wait=2048, dtype=F32 if dt == "f32" else F64)
    try:
        core.set_trace(rot)
        core.replay(0, T, None, None)
        _sync()
        core.reset()
        core.set_trace(tr)
        half = 37
        ph = torch.zeros((B, half, 3), dtype=torch.float64, device="cuda")
        dh = torch.zeros((B, half), dtype=torch.int32, device="cuda")
        core.replay(0, half, ph.data_ptr(), dh.data_ptr())
        rest = torch.zeros((B, T - half, 3), dtype=torch.float64, device="cuda")
        dr = torch.zeros((B, T - half), dtype=torch.int32, device="cuda")
        core.replay(half, T - half, rest.data_ptr(), dr.data_ptr())
        _sync()
        poses = np.concatenate([ph.cpu().numpy(), rest.cpu().numpy()], axis=1)
        dims = np.concatenate([dh.cpu().numpy(), dr.cpu().numpy()], axis=1)
        info = core.launch_info()
        groups, resident = expected_launch(dtype, B)
        assert info["stream_groups"] == groups and info["chol_resident"] == resident, info
        tol = REPLAY_TOL if dt == "f64" else F32_TOL
        # the delays really put different dimensions side by side (k = 40 and k = T both stay at n = 3)
        assert len({tuple(ref[b][1]) for b in ids}) >= 7
        worst = 0.0
        for b in ids:
            po, do, (Xo, Zo, Po), wo = ref[b]
            X, Z, P = core.state(b)
            assert np.array_equal(dims[b], do), f"filter {b} (k = {ks[b]}): state dimension per callback"
            assert np.array_equal(Z, Zo), f"filter {b} (k = {ks[b]}): Z"
            for a, c in zip(core.wait_list(b, cap=2048), wo):
                assert np.array_equal(a, c), f"filter {b} (k = {ks[b]}): wait-list"
            assert core.status(b) == 0, (b, core.status(b))
            if ks[b] == T:  # never a sensor message: initialize()'s state, zero poses
                assert (dims[b] == 3).all() and not poses[b].any() and not X.any() and not Z.any()
                assert np.array_equal(P, np.eye(3) * float(np.float32(0.001))) and len(wo[0]) == 0
                continue
            errs = rel_err(poses[b], po), rel_err(X, Xo), cov_err(P, Po)
            worst = max(worst, *errs)
            assert max(errs) < tol, f"filter {b} (k = {ks[b]}, N = {X.shape[0]}): rel err pose/X/P {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}"
        print(f"skipped / lagging filters {dtype} B={B}: worst rel err pose/X/P over {len(ids)} filters {worst:.2e}; launch {info}")
    finally:
        core.close()


# ---------------------------------------------------------------------------------------------------- D


def test_bench_shape_distinct_trajectories(built, monkeypatch):
    """bench.py's workload -- 256 filters of 512 landmarks (n = 1027), the library's default chain (three stream groups, resident bf16
    Cholesky and TRSM) -- on 256 DISTINCT trajectories, against the fp64 chain run on the same trajectories: on identical data a workgroup
    that reads a neighbour's planes, V or inputs gets the right numbers (test_gpu_large's bit-identity test); here it does not."""
    import torch
    from awesomeslam_amd.core import Core, F32, F64

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    L, T, B = 512, 104, 256
    ids = list(range(9)) + [87, 88, 95, 96, 175, 176, 183] + list(range(247, 256))  # every residue mod 8, both sides of each group boundary
    tr = tg.make_traces(L, T, B=B, seed=1)
    core = Core("ekf", tg.dim_cap(L), batch=B, max_obs=tr.max_obs, max_wait=2048, dtype=F32)
    poses = torch.zeros((B, T, 3), dtype=torch.float64, device="cuda")
    dims = torch.zeros((B, T), dtype=torch.int32, device="cuda")
    try:
        core.set_trace(tr)
        core.replay(0, T, poses.data_ptr(), dims.data_ptr())
        _sync()
        info = core.launch_info()
        assert info["stream_groups"] == 3 and info["chol_resident"] and "bf16" in core.kernel_info()["name"], (info, core.kernel_info())
        got = {b: (core.state(b), core.wait_list(b, cap=2048), core.status(b)) for b in ids}
    finally:
        core.close()
    poses, dims = poses.cpu().numpy(), dims.cpu().numpy()
    sub = tr.select(ids)
    ref = Core("ekf", tg.dim_cap(L), batch=len(ids), max_obs=tr.max_obs, max_wait=2048, dtype=F64)
    pr = torch.zeros((len(ids), T, 3), dtype=torch.float64, device="cuda")
    dr = torch.zeros((len(ids), T), dtype=torch.int32, device="cuda")
    try:
        ref.set_trace(sub)
        ref.replay(0, T, pr.data_ptr(), dr.data_ptr())
        _sync()
        pr, dr = pr.cpu().numpy(), dr.cpu().numpy()
        wx = wpose = 0.0
        wp = np.zeros(4)
        for i, b in enumerate(ids):
            (X, Z, P), w, status = got[b]
            Xr, Zr, Pr = ref.state(i)
            assert status == 0 and ref.status(i) == 0
            assert np.array_equal(dims[b], dr[i]) and dims[b, -1] == tg.full_dim(L) and np.array_equal(Z, Zr), f"filter {b}: bookkeeping"
            for a, c in zip(w, ref.wait_list(i, cap=2048)):
                assert np.array_equal(a, c), f"filter {b}: wait-list"
            ex, epose = rel_err(X, Xr), rel_err(poses[b], pr[i])
            ep = np.array((rel_err(P, Pr),) + block_rel_err(P, Pr))
            wx, wpose, wp = max(wx, ex), max(wpose, epose), np.maximum(wp, ep)
            assert ex < 1e-8 and epose < 1e-8 and ep.max() < F32_TOL, f"filter {b}: rel err X {ex:.2e} pose {epose:.2e} P (norm, blocks) {ep}"
        print(f"bench shape, {len(ids)} of {B} distinct trajectories against the fp64 chain: worst rel err pose {wpose:.2e} X {wx:.2e} "
              f"P {wp[0]:.2e} (blocks pose/cross/landmark {wp[1]:.2e} {wp[2]:.2e} {wp[3]:.2e})")
    finally:
        ref.close()


# ---------------------------------------------------------------------------------------------------- E


def replay_all(core, T, t0=0):
    import torch

    B = core.batch
    p = torch.zeros((B, T - t0, 3), dtype=torch.float64, device="cuda")
    d = torch.zeros((B, T - t0), dtype=torch.int32, device="cuda")
    core.replay(t0, T - t0, p.data_ptr(), d.data_ptr())
    _sync()
    return p.cpu().numpy(), d.cpu().numpy()


def assert_matches_oracle(core, b, poses, dims, o, po, do, tol, what):
    Xo, Zo, Po = o.state()
    X, Z, P = core.state(b)
    assert np.array_equal(dims, do) and np.array_equal(Z, Zo), f"{what}: dimensions / Z"
    for a, c in zip(core.wait_list(b, cap=2048), o.wait_list()):
        assert np.array_equal(a, c), f"{what}: wait-list"
    errs = rel_err(poses, po), rel_err(X, Xo), cov_err(P, Po)
    assert max(errs) < tol, f"{what}: rel err pose/X/P {errs}"
    return max(errs)


@pytest.mark.parametrize("path", ["small-f64", "large-f64", "large-f32"])
def test_status_bits_wait_overflow(path, built, monkeypatch):
    """ASLAM_ST_WAIT_OVERFLOW: a trace that fills the wait-list with junk (warm-up stops at different places) and a small max_wait.  The bit
    is clear up to the callback before the first one whose wait-list the oracle grows past max_wait, set from that callback on and until
    aslam_reset; the state just before it matches the oracle, and so does the whole trace with a large max_wait."""
    from awesomeslam_amd.core import Core, F32, F64, ST_WAIT_OVERFLOW
    from oracle.c_oracle import CFilter

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    L, T, max_wait = 8, 200, 24
    cap = 30 if path.startswith("small") else 200  # 200: the fp64 context takes the large path
    tr = tg.make_traces(L, T, B=1, seed=25, warm_hop=12, layout="ring", sensor_range=6.0)
    o = CFilter("ekf", cap)
    t0 = None
    for t in range(T):
        o.replay(tr[0].slice(t, t + 1))
        if len(o.wait_list()[0]) > max_wait:
            t0 = t
            break
    assert t0 is not None and t0 > 5, "the scenario must overflow the small wait-list, and not at once"
    dtype = F32 if path.endswith("f32") else F64
    core = Core("ekf", cap, batch=1, max_obs=tr.max_obs, max_wait=max_wait, dtype=dtype)
    big = Core("ekf", cap, batch=1, max_obs=tr.max_obs, max_wait=512, dtype=dtype)
    try:
        assert (core.layout()[0] > 144) == path.startswith("large")
        core.set_trace(tr)
        bits = []
        for t in range(t0 + 3):
            core.replay(t, 1, None, None)
            bits.append(bool(core.status(0) & ST_WAIT_OVERFLOW))
        assert bits == [False] * t0 + [True] * 3, f"first callback past max_wait: {t0} (oracle); bit per callback {bits}"
        assert core.status(0) == ST_WAIT_OVERFLOW
        replay_all(core, T, t0 + 3)
        assert core.status(0) == ST_WAIT_OVERFLOW, "the bit is sticky until aslam_reset"
        core.reset()
        assert core.status(0) == 0 and core.dim(0) == 3
        # the reset context up to the callback before the overflow, against the oracle
        p, d = replay_all(core, t0)
        oo = CFilter("ekf", cap)
        po, do = oo.replay(tr[0], T=t0)
        tol = REPLAY_TOL if dtype == F64 else F32_TOL
        e1 = assert_matches_oracle(core, 0, p[0], d[0], oo, po, do, tol, f"{path} up to callback {t0 - 1}")
        assert core.status(0) == 0
        # the whole trace with room on the wait-list
        big.set_trace(tr)
        p, d = replay_all(big, T)
        of = CFilter("ekf", cap)
        po, do = of.replay(tr[0])
        e2 = assert_matches_oracle(big, 0, p[0], d[0], of, po, do, tol, f"{path}, max_wait 512")
        assert big.status(0) == 0
        print(f"wait-list overflow {path}: bit from callback {t0} on; rel err before it {e1:.2e}, whole trace with max_wait 512 {e2:.2e}")
    finally:
        core.close()
        big.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_status_bits_growth_refused_large(dtype, built, monkeypatch):
    """ASLAM_ST_GROWTH_REFUSED on the large path: a capacity between the second (n = 137) and the third (n = 203) growth stage of a
    100-landmark trace; the oracle with the same capacity refuses the same landmarks (ekf.cpp:263-268)."""
    from awesomeslam_amd.core import Core, F32, F64, ST_GROWTH_REFUSED
    from oracle.c_oracle import CFilter

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    L, T, B, cap = 100, 80, 2, 150
    tr = tg.make_traces(L, T, B=B, seed=68)
    core = Core("ekf", cap, batch=B, max_obs=tr.max_obs, max_wait=2048, dtype=F32 if dtype == "f32" else F64)
    try:
        assert core.layout()[0] == 192
        core.set_trace(tr)
        poses, dims = replay_all(core, T)
        tol = REPLAY_TOL if dtype == "f64" else F32_TOL
        for b in range(B):
            o = CFilter("ekf", cap)
            po, do = o.replay(tr[b])
            assert do[-1] == 137 and 71 in do, "the third growth stage must be the refused one"
            e = assert_matches_oracle(core, b, poses[b], dims[b], o, po, do, tol, f"growth refused {dtype} b={b}")
            assert core.status(b) == ST_GROWTH_REFUSED, core.status(b)
            print(f"growth refused on the large path {dtype} b={b}: N={core.dim(b)}, rel err {e:.2e}")
    finally:
        core.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_status_bits_obs_overflow_large(dtype, built, monkeypatch):
    """ASLAM_ST_OBS_OVERFLOW on the large path: one message longer than max_obs flags that filter only; the other filters of the batch come
    out bit for bit as in the same replay without the long message."""
    from awesomeslam_amd.core import Core, F32, F64, ST_OBS_OVERFLOW
    from oracle.c_oracle import CFilter

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    L, T, B = 80, 50, 3
    clean = tg.make_traces(L, T, B=B, seed=69)
    bad = tg.make_traces(L, T, B=B, seed=69)
    bad.n_obs[1, 30] = bad.max_obs + 3
    out = []
    for tr in (clean, bad):
        core = Core("ekf", tg.dim_cap(L), batch=B, max_obs=tr.max_obs, max_wait=2048, dtype=F32 if dtype == "f32" else F64)
        try:
            assert core.layout()[0] > 144
            core.set_trace(tr)
            poses, dims = replay_all(core, T)
            out.append((poses, dims, [core.state(b) for b in range(B)], [core.status(b) for b in range(B)]))
        finally:
            core.close()
    (p0, d0, s0, st0), (p1, d1, s1, st1) = out
    assert st0 == [0] * B and st1[1] == ST_OBS_OVERFLOW and st1[0] == st1[2] == 0, (st0, st1)
    for b in (0, 2):
        assert np.array_equal(p0[b], p1[b]) and np.array_equal(d0[b], d1[b]), f"filter {b} changed"
        assert all(np.array_equal(x, y) for x, y in zip(s0[b], s1[b])), f"filter {b} changed"
    o = CFilter("ekf", tg.dim_cap(L))
    po, do = o.replay(clean[0])
    assert np.array_equal(d0[0], do) and d0[0, -1] == tg.full_dim(L)
    e = max(rel_err(p0[0], po), rel_err(s0[0][0], o.state()[0]), cov_err(s0[0][2], o.state()[2]))
    assert e < (REPLAY_TOL if dtype == "f64" else F32_TOL)
    print(f"message overflow on the large path {dtype}: flagged on filter 1 only, neighbours bit-identical; filter 0 rel err {e:.2e}")
