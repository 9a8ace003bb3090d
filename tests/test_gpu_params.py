"""-m gpu: the run-time noise and association parameters (aslam_set_params) of every kernel family against tests/params_ref.py -- the NumPy
oracle run with a parameter dict -- on the same inputs.

Bars: util.REL_TOL for the fp64 paths and test_gpu_large.F32_TOL for the binary32 chains, the project's own; errors are norm-wise per trajectory
as in tests/test_gpu_innovation.py.  Every scenario asserts that its oracle stays positive definite, and where a parameter set is meant to move
the result, that the oracle's final P moved by >= MOVED (util.cov_err against the default oracle): at 100 x the bar a kernel that ignored the
parameter cannot pass, and a change of the traces cannot hollow the test out unnoticed.
"""
import functools

import numpy as np
import pytest

from awesomeslam_amd import trace as tg
from params_ref import DEFAULTS, FIELDS, SETS, ParamFilter, full
from test_gpu_innovation import assert_pd, gpu_replay_stats, make_core
from util import REL_TOL, cov_err, rel_err

pytestmark = pytest.mark.gpu

MOVED = 1e-4  # 100 x REL_TOL
WAIT = 512  # the single-CU kernels' largest wait-list: the UKF under set D (assoc_dist 0.1) holds up to 307 entries at L = 5 and 465 at L = 8
LATE = 3


def key(params):
    return tuple(sorted(params.items()))


@functools.lru_cache(maxsize=None)
def trajectory(L, T, seed, b=0, late=0):
    """trajectory b of make_traces(L, T, seed); late: its first `late` sensor messages dropped (cbOdom returns early until then)"""
    tr = tg.make_traces(L, T, B=b + 1, seed=seed)
    if late:
        tr.obs_new[b, :late] = 0
    return tr.select([b])


def batch_of(trajs):
    """one trace from single-trajectory traces"""
    cat = lambda f: np.concatenate([getattr(t, f) for t in trajs])  # noqa: E731
    return tg.Trace(cat("odom"), cat("dt"), cat("obs_new"), cat("n_obs"), cat("obs"), cat("landmarks"), cat("truth"), trajs[0].warmup)


@functools.lru_cache(maxsize=None)
def reference(kind, L, T, seed, b, late, pkey):
    """ParamFilter's streams and final state for that trajectory under the parameters `pkey`; computed once, never modified"""
    o = ParamFilter(kind, tg.dim_cap(L), dict(pkey))
    out = o.replay_stats(trajectory(L, T, seed, b, late)[0])
    wait = tuple(np.array([w[i] for w in o.wait]) for i in range(3))
    res = out + (o.X.copy(), o.Z.copy(), o.P.copy(), wait)
    for a in res[:-1]:
        a.setflags(write=False)
    return res


def configure(core, sets):
    """filter b on sets[b] from its first callback on: p0_pose applies at aslam_reset, so the context is initialised again behind set_params
    (the oracle writes P = p0_pose I after initialize())"""
    for b, p in enumerate(sets):
        if p is not None:
            core.set_params(p, b)
    core.reset()


def check_filter(core, b, streams, ref, tol, what, wait_cap=WAIT):
    """filter b of a finished replay against its oracle; returns the errors"""
    poses, dims, nis, logdet, pcov = streams
    po, do, no, lo, co, ran, Xo, Zo, Po, wo = ref
    assert_pd(Po, what)
    assert ran.any() and np.array_equal(dims[b], do), (what, dims[b], do)
    assert np.array_equal(np.isnan(nis[b]), ~ran) and np.array_equal(np.isnan(logdet[b]), ~ran), what
    X, Z, P = core.state(b)
    errs = dict(nis=rel_err(nis[b][ran], no[ran]), logdet=rel_err(logdet[b][ran], lo[ran]), pose_cov=rel_err(pcov[b][ran], co[ran]),
                pose=rel_err(poses[b][ran], po[ran]), X=rel_err(X, Xo), P=cov_err(P, Po))
    print(f"{what} N={core.dim(b)}: rel err " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert np.array_equal(Z, Zo) and core.status(b) == 0, what
    wr, wb, wc = core.wait_list(b, cap=wait_cap)
    assert len(wr) == len(wo[0]) and np.array_equal(wr, wo[0].astype(np.float32)) and np.array_equal(wb, wo[1].astype(np.float32)) and \
        np.array_equal(wc, wo[2].astype(np.uint32)), what
    assert max(errs.values()) < tol, (what, errs)
    return errs


def assert_moved(ref, ref_default, what):
    assert ref[8].shape == ref_default[8].shape and cov_err(ref[8], ref_default[8]) >= MOVED, f"{what}: the parameters must move the oracle's P"


# ---- 1. the single-CU kernels, every instantiation: two tiles (n = 13), five (n = 43), nine (n = 131)
@pytest.mark.parametrize("pset", ["A", "B"])
@pytest.mark.parametrize("L,T,seed", [(5, 120, 41), (20, 100, 45), (64, 100, 46)])
@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_single_cu_kernels(kind, L, T, seed, pset, built):
    """B = 2, filter 1's first sensor message three callbacks late (as tests/test_gpu_innovation.check_replay).  Fails without the feature."""
    prm = SETS[pset]
    tr = batch_of([trajectory(L, T, seed, 0, 0), trajectory(L, T, seed, 1, LATE)])
    core = make_core(kind, tg.dim_cap(L), batch=2, max_obs=tr.max_obs, max_wait=WAIT)
    configure(core, [prm, prm])
    core.set_trace(tr)
    streams = gpu_replay_stats(core, T)
    for b in range(2):
        ref = reference(kind, L, T, seed, b, LATE if b else 0, key(prm))
        assert b == 0 or not ref[5][:LATE].any()
        check_filter(core, b, streams, ref, REL_TOL, f"{kind} L={L} set {pset} b={b}")
        assert core.dim(b) == tg.full_dim(L)
    assert_moved(reference(kind, L, T, seed, 0, 0, key(prm)), reference(kind, L, T, seed, 0, 0, ()), f"{kind} L={L} set {pset}")
    assert core.launch_info()["launches_per_callback"] == 1


# ---- 2. each parameter alone
@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_each_parameter_alone(kind, built):
    """one context of 11 filters on one trajectory, filter k with only parameter k changed (to its value in A; assoc_dist to D's): a parameter
    wired to the wrong row class passes the full sets only by luck, not this"""
    L, T, seed = 5, 120, 41
    singles = [{k: (SETS["D"] if k == "assoc_dist" else SETS["A"])[k]} for k in FIELDS]
    assert len(singles) == 11
    tr = trajectory(L, T, seed).select([0] * 11)
    core = make_core(kind, tg.dim_cap(L), batch=11, max_obs=tr.max_obs, max_wait=WAIT)
    configure(core, singles)
    core.set_trace(tr)
    streams = gpu_replay_stats(core, T)
    default = reference(kind, L, T, seed, 0, 0, ())
    for b, p in enumerate(singles):
        (name,) = p
        ref = reference(kind, L, T, seed, 0, 0, key(p))
        check_filter(core, b, streams, ref, REL_TOL, f"{kind} {name} alone")
        if name in ("promote_count", "assoc_dist"):
            assert not np.array_equal(ref[1], default[1]), f"{name}: the dimension stream must leave the default's"
        elif name == "var_a" and kind == "ekf":
            assert np.array_equal(ref[8], default[8])  # ignored by the EKF
        else:
            assert_moved(ref, default, f"{kind} {name} alone")


# ---- 3. a heterogeneous batch; the filter nobody touched
@pytest.fixture(scope="module")
def mixed(built):
    L, T, seed = 8, 120, 42
    names = ["default", "A", "B", "D"]
    out = {}
    for kind in ("ekf", "ukf"):
        tr = trajectory(L, T, seed).select([0] * 4)
        core = make_core(kind, tg.dim_cap(L), batch=4, max_obs=tr.max_obs, max_wait=WAIT)
        configure(core, [None] + [SETS[nm] for nm in names[1:]])  # filter 0: never set
        core.set_trace(tr)
        out[kind] = core, gpu_replay_stats(core, T), tr
    return L, T, seed, names, out


@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_mixed_batch_and_untouched_default(kind, mixed):
    L, T, seed, names, out = mixed
    core, streams, tr = out[kind]
    for b, nm in enumerate(names):
        check_filter(core, b, streams, reference(kind, L, T, seed, 0, 0, key(SETS[nm])), REL_TOL, f"{kind} mixed batch, {nm}")
        assert core.params(b).as_dict() == full(SETS[nm])  # the round trip through HBM
    # filter 0 against a context that never heard of parameters: bit for bit
    plain = make_core(kind, tg.dim_cap(L), batch=1, max_obs=tr.max_obs, max_wait=WAIT)
    plain.set_trace(tr.select([0]))
    ps = gpu_replay_stats(plain, T)
    for a, c in zip(streams, ps):
        assert np.array_equal(a[0], c[0], equal_nan=True)
    for a, c in zip(core.state(0) + core.wait_list(0), plain.state(0) + plain.wait_list(0)):
        assert np.array_equal(a, c)
    assert plain.params(0).as_dict() == DEFAULTS


def test_set_all_reset_and_p0_pose(mixed):
    L, T, seed, names, out = mixed
    core = make_core("ekf", tg.dim_cap(L), batch=3, max_obs=4, max_wait=16)
    core.set_params(SETS["B"])  # traj = -1
    assert all(core.params(b).as_dict() == full(SETS["B"]) for b in range(3))
    core.set_params(SETS["A"], 1)
    # p0_pose: not before the next reset
    assert all(np.array_equal(core.state(b)[2], np.eye(3) * DEFAULTS["p0_pose"]) for b in range(3))
    core.reset()
    assert core.params(0).as_dict() == full(SETS["B"]) and core.params(1).as_dict() == full(SETS["A"])  # reset keeps them
    assert np.array_equal(core.state(0)[2], np.eye(3) * SETS["B"]["p0_pose"]) and np.array_equal(core.state(1)[2], np.eye(3) * SETS["A"]["p0_pose"])
    from awesomeslam_amd.core import AslamError

    with pytest.raises(AslamError, match="aslam_params.r_yaw"):
        core.set_params(dict(r_yaw=0.0), 2)
    with pytest.raises(AslamError, match="out of range"):
        core.set_params({}, 3)
    assert core.params(2).as_dict() == full(SETS["B"])  # a refused call changes nothing


@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_reset_then_rerun_with_the_parameters(kind, mixed):
    """after aslam_reset the batch runs again under the same parameters -- p0_pose included, now from the start for both runs: bit for bit"""
    L, T, seed, names, out = mixed
    core, streams, tr = out[kind]
    before = [core.state(b) for b in range(4)]
    core.reset()
    again = gpu_replay_stats(core, T)
    for a, c in zip(streams, again):
        assert np.array_equal(a, c, equal_nan=True)
    for b in range(4):
        for a, c in zip(before[b], core.state(b)):
            assert np.array_equal(a, c)


def test_restore_leaves_the_parameters_alone(built):
    """fork: filter 0 (default parameters) into slot 1 (set A) -- the state moves, the destination's parameters stay"""
    L, T, seed = 5, 40, 41
    tr = trajectory(L, 120, seed).select([0, 0])
    core = make_core("ekf", tg.dim_cap(L), batch=2, max_obs=tr.max_obs, max_wait=WAIT)
    configure(core, [None, SETS["A"]])
    core.set_trace(tr)
    gpu_replay_stats(core, T)
    assert not np.array_equal(core.state(0)[0], core.state(1)[0])
    core.restore(core.snapshot([0]), records=[0], trajs=[1])
    assert core.params(1).as_dict() == full(SETS["A"]) and core.params(0).as_dict() == DEFAULTS
    for a, c in zip(core.state(0) + core.wait_list(0), core.state(1) + core.wait_list(1)):
        assert np.array_equal(a, c)


# ---- 4. the large-state paths at n = 163
LARGE = (80, 150, 61)


def large_pair(kind, pset, dtype, tol, what):
    """two filters on the trajectory: filter 0 on the defaults, filter 1 on `pset`; returns the worst error of each"""
    L, T, seed = LARGE
    tr = trajectory(L, T, seed).select([0, 0])
    core = make_core(kind, tg.dim_cap(L), batch=2, max_obs=tr.max_obs, max_wait=2048, dtype=dtype)
    configure(core, [None, SETS[pset]])
    core.set_trace(tr)
    streams = gpu_replay_stats(core, T)
    worst = []
    for b, p in enumerate(({}, SETS[pset])):
        errs = check_filter(core, b, streams, reference(kind, L, T, seed, 0, 0, key(p)), tol, f"{what} {'set ' + pset if b else 'defaults'}", wait_cap=2048)
        worst.append(max(errs.values()))
        assert core.dim(b) == tg.full_dim(L) == 163
    assert_moved(reference(kind, L, T, seed, 0, 0, key(SETS[pset])), reference(kind, L, T, seed, 0, 0, ()), what)
    assert core.launch_info()["launches_per_callback"] > 1  # the launch chains, not a single-CU kernel
    return worst + [core.launch_info()]


@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_large_fp64(kind, built):
    from awesomeslam_amd.core import F64

    large_pair(kind, "A", F64, REL_TOL, f"large {kind} fp64")


@pytest.mark.parametrize("dtype", ["f32", "f32-resident"])
def test_large_ekf_binary32(dtype, built, monkeypatch):
    """set C keeps S no worse conditioned than the defaults do (cond 5.6 against 7.1 on this trace), so the project's own bar applies; the
    default-parameter error of the same chain on the same trace is measured in the same launch (filter 0) and printed next to it"""
    from awesomeslam_amd.core import F32
    from test_gpu_large import F32_TOL, chol_mode

    assert chol_mode(dtype, monkeypatch) == "f32"
    d, c, info = large_pair("ekf", "C", F32, F32_TOL, f"large ekf {dtype}")
    assert info["chol_resident"] == ("-resident" in dtype), info  # the chain this spelling means (tests/test_gpu_large.py::test_replay_parity)
    print(f"large ekf {dtype}: worst rel err, defaults {d:.2e}, set C {c:.2e} (bar {F32_TOL:.0e})")


# ---- 5. the seams outside the replay
def synth13(kind, seed):
    from test_gpu_large import synth

    n = 13
    X, Z, P = synth(n, seed)
    if kind == "ukf":  # landmarks east of the robot, a small covariance (the scenario of tests/test_gpu_ukf.py)
        r2 = np.random.default_rng(seed)
        X = np.concatenate([[0.3, -0.2, 0.4], (np.array([25.0, 0.0]) + 4 * r2.normal(size=((n - 3) // 2, 2))).ravel()])
        A_ = r2.normal(size=(n, n)) * 0.01
        P = A_ @ A_.T + np.eye(n) * 0.002
        Z = X.copy()
        for i in range((n - 3) // 2):
            dx, dy = X[3 + 2 * i] - X[0], X[4 + 2 * i] - X[1]
            Z[3 + 2 * i] = np.float32(np.hypot(dx, dy) + 0.01 * r2.normal())
            Z[4 + 2 * i] = np.float32(np.arctan2(dy, dx) - X[2] + 0.002 * r2.normal())
    return X, Z, P


@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_step_batch_and_grow(kind, built):
    """aslam_*_step_batch and aslam_grow at n = 13 under set A (filter 0 stays on the defaults): a step, a growth to n = 15, a step"""
    import torch

    B, n = 3, 13
    core = make_core(kind, 30, batch=B, max_obs=4, max_wait=4)
    a = (0.07, -0.03)
    oracles = []
    for b in range(B):
        prm = SETS["A"] if b else {}
        if b:
            core.set_params(prm, b)
        X, Z, P = synth13(kind, 1300 + b)
        o = ParamFilter(kind, 30, prm)
        o.set_state(n, X, Z, P, *a)
        core.set_state(b, n, X, Z, P)
        oracles.append(o)
    vx, az, dt = (np.full(B, v, np.float32) for v in (0.2, 0.1, 1.0))
    a00, a10 = np.full(B, a[0]), np.full(B, a[1])

    def step():
        nn = oracles[0].N
        Zs = np.zeros((B, nn + 3))
        for b, o in enumerate(oracles):
            Zs[b, :nn] = o.Z
        Xout = np.zeros((B, nn))
        core.step_batch(vx, az, dt, Zs, a00, a10, X_out=Xout) if kind == "ekf" else core.step_batch(vx, az, dt, Zs, X_out=Xout)
        torch.cuda.synchronize()
        for b, o in enumerate(oracles):
            o.slam(vx[b], az[b], dt[b])
            assert_pd(o.P, f"{kind} step b={b}")
            X, _, P = core.state(b)
            e = max(rel_err(Xout[b], o.X), rel_err(X, o.X), cov_err(P, o.P))
            print(f"step_batch {kind} n={nn} b={b}: rel err {e:.2e}")
            assert e < REL_TOL and core.status(b) == 0, (b, e)

    step()
    for b, o in enumerate(oracles):
        o.grow([(np.float32(3.0 + b), np.float32(0.3))])
        assert o.N == 15 and o.P[13, 13] == o.P[14, 14] == full(o.prm)["p0_landmark"]
        core.grow(b, 15, o.X[13:], o.Z[13:])
        P = core.state(b)[2]
        assert np.array_equal(P[13:, 13:], o.P[13:, 13:]) and not P[13:, :13].any() and not P[:13, 13:].any()
    step()


@pytest.mark.parametrize("pset", ["A", "D"])
@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_host_mirror_node(kind, pset, built):
    """aslam::EKFSlam / UKFSlam with setParams: the mirror's own association and wait-list use assoc_dist and promote_count"""
    from awesomeslam_amd.core import Node

    L, T, seed = 5, 120, 41
    node = Node(kind, tg.dim_cap(L))
    node.set_params(SETS[pset])
    assert node.params().as_dict() == full(SETS[pset])
    pn, dn = node.replay(trajectory(L, T, seed)[0])
    po, do, no, lo, co, ran, Xo, Zo, Po, wo = reference(kind, L, T, seed, 0, 0, key(SETS[pset]))
    assert_pd(Po, f"node {kind} {pset}")
    X, Z, a00, a10 = node.state()
    assert np.array_equal(dn, do) and np.array_equal(Z, Zo)
    wr, wb, wc = node.wait_list()
    assert np.array_equal(wr, wo[0].astype(np.float32)) and np.array_equal(wb, wo[1].astype(np.float32)) and np.array_equal(wc, wo[2].astype(np.uint32))
    errs = rel_err(pn[ran], po[ran]), rel_err(X, Xo), cov_err(node.P(), Po)
    print(f"node {kind} set {pset}: rel err pose/X/P {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
    assert max(errs) < REL_TOL
    default = reference(kind, L, T, seed, 0, 0, ())
    assert not np.array_equal(do, default[1])  # both sets change the dimension stream (promote_count / assoc_dist)


# ---- 6. the sweep
def test_sweep(built):
    from awesomeslam_amd import consistency, tune

    L, T, seed = 8, 120, 42
    names = ["default", "A", "B", "C"]
    res = tune.sweep("ekf", trajectory(L, T, seed), [SETS[k] for k in names], tg.dim_cap(L))
    ll, npd = [], []
    for nm, r in zip(names, res):
        po, do, no, lo, co, ran, Xo, Zo, Po, wo = reference("ekf", L, T, seed, 0, 0, key(SETS[nm]))
        assert_pd(Po, f"sweep {nm}")
        ll.append(consistency.log_likelihood(no[ran], lo[ran], do[ran]).sum())
        npd.append((no[ran] / do[ran]).mean())
        assert r["params"] == full(SETS[nm]) and r["N"] == tg.full_dim(L) and r["status"] == 0 and r["callbacks"] == int(ran.sum())
        assert r["pose_nees"] is not None and np.isfinite(r["pose_nees"]) and r["pose_nees"] > 0
    got_ll, got_npd = [r["log_likelihood"] for r in res], [r["nis_per_dim"] for r in res]
    # a single trace.Trajectory instead of a Trace, with and without its ground truth: the same figures from the same launches
    import dataclasses

    tj = trajectory(L, T, seed)[0]
    for t2, nees in ((tj, True), (dataclasses.replace(tj, landmarks=None, truth=None), False)):
        r2 = tune.sweep("ekf", t2, [SETS["A"], SETS["B"]], tg.dim_cap(L))
        assert [r["log_likelihood"] for r in r2] == got_ll[1:3] and [r["N"] for r in r2] == [tg.full_dim(L)] * 2
        assert all((r["pose_nees"] is not None) == nees for r in r2) and (not nees or r2[0]["pose_nees"] == res[1]["pose_nees"])
    print("sweep log-likelihood", got_ll, "oracle", ll, "nis/dim", got_npd, "oracle", npd)
    assert rel_err(got_ll, ll) < REL_TOL and rel_err(got_npd, npd) < REL_TOL
    # pairwise different, by more than the comparison above could blur: 100 x the bar on the largest of them
    for v in (ll, got_ll):
        assert min(abs(a - b) for i, a in enumerate(v) for b in v[i + 1:]) > 100 * REL_TOL * max(map(abs, v)), v
