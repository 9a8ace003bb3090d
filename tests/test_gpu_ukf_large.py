"""-m gpu: the large-state UKF chain (ASLAM_CFG_UKF_LARGE: state dimensions 145 .. 1085, fp64; ukf_large.h) against the CPU oracle.

The project's usual bars: 1e-6 relative norm-wise AND block-wise on state and covariance (util.REL_TOL), bit-exact bookkeeping (dimensions, Z,
wait-list), status 0.  The reference UKF's central weight is (1 - N) / 3, so every case first asserts that the ORACLE's covariance is finite and
positive definite on its input (as tests/test_gpu_ukf.py does): a scenario that leaves the cone would be a wrong scenario, not a skip.  The
formulation the kernels use (Cholesky of S without the i = 0 term, forward-only Sherman-Morrison) agrees with the oracle to 1e-10 in NumPy
fp64 on these inputs: an error near 1e-6 here is a bug, not rounding."""
import numpy as np
import pytest

from awesomeslam_amd import trace as tg
from util import REL_TOL, cov_err, rel_err

pytestmark = pytest.mark.gpu


def synth(n, seed):
    """the synthetic state of tests/test_gpu_large.py"""
    rng = np.random.default_rng(seed)
    L = (n - 3) // 2
    X = np.concatenate([[0.3, -0.2, 0.4], (np.array([20.0, 0.0]) + 6 * rng.normal(size=(L, 2))).ravel()])
    A = rng.normal(size=(n, n)) * 0.02
    P = A @ A.T / n * 20 + np.eye(n) * 0.01
    Z = X.copy()
    for i in range(L):
        dx, dy = X[3 + 2 * i] - X[0], X[4 + 2 * i] - X[1]
        Z[3 + 2 * i] = np.float32(np.hypot(dx, dy) + 0.01 * rng.normal())
        Z[4 + 2 * i] = np.float32(np.arctan2(dy, dx) - X[2] + 0.002 * rng.normal())
    return X, Z, P


STEPS = ((0.2, 0.1, 1.0), (0.15, 0.0, 0.5), (0.0, 0.0, 1.0))


def assert_pd(P, what):
    assert np.isfinite(P).all() and np.linalg.eigvalsh((P + P.T) / 2).min() > 0, f"{what}: the scenario must keep the oracle positive definite"


def ukf_core(cap, **kw):
    from awesomeslam_amd.core import CFG_UKF_LARGE, Core

    return Core("ukf", cap, flags=CFG_UKF_LARGE, **kw)


def gpu_replay(tr, cap, T):
    import torch

    core = ukf_core(cap, batch=tr.B, max_obs=tr.max_obs, max_wait=2048)
    core.set_trace(tr)
    poses = torch.zeros((tr.B, T, 3), dtype=torch.float64, device="cuda")
    dims = torch.zeros((tr.B, T), dtype=torch.int32, device="cuda")
    core.replay(0, T, poses.data_ptr(), dims.data_ptr())
    torch.cuda.synchronize()
    return core, poses.cpu().numpy(), dims.cpu().numpy()


def assert_replay_parity(core, b, poses, dims, o, po, do, what):
    Xo, Zo, Po = o.state()
    X, Z, P = core.state(b)
    assert np.array_equal(dims, do) and np.array_equal(Z, Zo), what
    for a, c in zip(core.wait_list(b, cap=2048), o.wait_list()):
        assert np.array_equal(a, c), what
    errs = rel_err(poses, po), rel_err(X, Xo), cov_err(P, Po)
    print(f"{what} N={core.dim(b)}: rel err pose/X/P = {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
    assert max(errs) < REL_TOL and core.status(b) == 0, what
    return errs


# 189 / 191: n + 2 (state rows, z^T and the innovation) just fits / just overflows three 64-blocks; 1085 = the largest state the path takes
@pytest.mark.parametrize("n,steps", [(145, 3), (189, 3), (191, 3), (193, 3), (321, 3), (515, 3), (1085, 1)])
def test_single_slam_on_synthetic_state(n, steps, built):
    from oracle.c_oracle import CFilter

    X, Z, P = synth(n, n)
    o = CFilter("ukf", n + 2)
    o.set_state(n, X, Z, P)
    core = ukf_core(n + 2, batch=2, max_obs=4, max_wait=4)
    core.set_state(1, n, X, Z, P)
    for vx, az, dt in STEPS[:steps]:
        Xg = core.ukf_step(1, vx, az, dt, Z)
        o.slam(vx, az, dt)
        Xo, _, Po = o.state()
        assert_pd(Po, f"n={n}")
        ex = rel_err(Xg, Xo)
        print(f"ukf large n={n}: rel err X {ex:.2e}")
        assert ex < REL_TOL
    ep = cov_err(core.state(1)[2], Po)
    print(f"ukf large n={n}: rel err P {ep:.2e}")
    assert ep < REL_TOL
    assert core.status(1) == 0 and core.dim(0) == 3 and core.dim(1) == n


@pytest.mark.parametrize("L,T,kw", [(80, 150, dict(seed=61)), (100, 80, dict(seed=62, sensor_every=2, dt_mode="random"))])
def test_replay_parity(L, T, kw, built):
    """two launches (the state round-trips through HBM), then reset and one launch; and the launch shape of the chain"""
    import torch
    from oracle.c_oracle import CFilter
    from awesomeslam_amd.core import Core

    tr = tg.make_traces(L, T, B=2, **kw)
    cap = tg.dim_cap(L)
    with pytest.raises(Exception):
        Core("ukf", cap, batch=2, max_obs=tr.max_obs, max_wait=2048)  # without the flag the refusal stands
    core = ukf_core(cap, batch=2, max_obs=tr.max_obs, max_wait=2048)
    core.set_trace(tr)
    poses = torch.zeros((2, T, 3), dtype=torch.float64, device="cuda")
    dims = torch.zeros((2, T), dtype=torch.int32, device="cuda")
    half = T // 2
    core.replay(0, half, poses[:, :half].contiguous().data_ptr(), None)
    core.replay(half, T - half, None, None)
    torch.cuda.synchronize()
    first = [core.state(b) for b in range(2)]
    core.reset()
    core.replay(0, T, poses.data_ptr(), dims.data_ptr())
    torch.cuda.synchronize()
    for b in range(2):
        o = CFilter("ukf", cap)
        po, do = o.replay(tr[b])
        assert_pd(o.state()[2], f"L={L} b={b}")
        assert_replay_parity(core, b, poses.cpu().numpy()[b], dims.cpu().numpy()[b], o, po, do, f"ukf large replay L={L} b={b}")
        for a, c in zip(first[b], core.state(b)):
            assert np.array_equal(a, c), "two launches and one launch after a reset must agree bit for bit"
    # launch shape: what the last replay really launched is the count the design documents (4 NB + 8), on one stream
    NB = core.layout()[0] // 64
    info = core.launch_info()
    assert info["launches_per_callback"] == 4 * NB + 8 and info["stream_groups"] == 1 and not info["chol_resident"], info
    name = core.kernel_info()["name"]
    assert "ukf_large_wabt" in name and f"{4 * NB + 8}-launch" in name, name


def test_512_landmarks(built):
    from oracle.c_oracle import CFilter

    L, T = 512, 42
    tr = tg.make_traces(L, T, B=1, seed=71)
    o = CFilter("ukf", tg.dim_cap(L))
    po, do = o.replay(tr[0])
    assert o.N == 1027
    assert_pd(o.state()[2], "512 landmarks")
    core, poses, dims = gpu_replay(tr, tg.dim_cap(L), T)
    assert_replay_parity(core, 0, poses[0], dims[0], o, po, do, "ukf large 512 landmarks")


def test_indefinite_covariance_is_flagged(built):
    """chol(P) of a covariance with a negative landmark variance has no factor: the sticky ASLAM_ST_NOT_PD bit is raised (the reference goes on with
    the NaNs of llt(), ukf.cpp:280 -- so does the oracle, and only the bit is asserted), and the other filter of the batch is left alone."""
    from awesomeslam_amd.core import ST_NOT_PD
    from oracle.c_oracle import CFilter

    n = 203
    X, Z, P = synth(n, 7)
    bad = P.copy()
    bad[100, 100] = -50.0
    core = ukf_core(n + 2, batch=2, max_obs=4, max_wait=4)
    core.set_state(0, n, X, Z, P)
    core.set_state(1, n, X, Z, bad)
    Xg = core.ukf_step(0, 0.2, 0.1, 1.0, Z)
    core.ukf_step(1, 0.2, 0.1, 1.0, Z)
    assert core.status(0) == 0
    assert core.status(1) & ST_NOT_PD
    o = CFilter("ukf", n + 2)
    o.set_state(n, X, Z, P)
    o.slam(0.2, 0.1, 1.0)
    Xo, _, Po = o.state()
    assert_pd(Po, "filter 0")
    ex, ep = rel_err(Xg, Xo), cov_err(core.state(0)[2], Po)
    print(f"ukf large, good filter next to an indefinite one: rel err X {ex:.2e} P {ep:.2e}")
    assert max(ex, ep) < REL_TOL


def test_mixed_dimensions_in_one_batched_step(built):
    from oracle.c_oracle import CFilter

    ns = (145, 515, 321, 189)
    B, ld = len(ns), max(ns)
    core = ukf_core(ld + 2, batch=B, max_obs=4, max_wait=4)
    oracles, Zs = [], np.zeros((B, ld))
    for b, n in enumerate(ns):
        X, Z, P = synth(n, n)
        core.set_state(b, n, X, Z, P)
        o = CFilter("ukf", ld + 2)
        o.set_state(n, X, Z, P)
        oracles.append(o)
        Zs[b, :n] = Z
    Xg = np.zeros((B, ld))
    for vx, az, dt in STEPS:
        f = lambda v: np.full(B, v, np.float32)  # noqa: E731
        core.step_batch(f(vx), f(az), f(dt), Zs, X_out=Xg)
        core.sync()
        for b, n in enumerate(ns):
            oracles[b].slam(vx, az, dt)
            Xo, _, Po = oracles[b].state()
            assert_pd(Po, f"n={n}")
            assert rel_err(Xg[b, :n], Xo) < REL_TOL, n
    for b, n in enumerate(ns):
        Xo, _, Po = oracles[b].state()
        X, _, P = core.state(b)
        ex, ep = rel_err(X, Xo), cov_err(P, Po)
        print(f"ukf large mixed batch b={b} n={n}: rel err X {ex:.2e} P {ep:.2e}")
        assert core.dim(b) == n and core.status(b) == 0 and max(ex, ep) < REL_TOL


def test_skipped_and_lagging_filters_in_one_replay(built):
    """filters whose first sensor message arrives 0, 2, 14, 40 callbacks late or never: skipped callbacks, different dimensions side by side"""
    from oracle.c_oracle import CFilter

    L, T, B = 80, 70, 5
    tr = tg.make_traces(L, T, B=B, seed=65)
    ks = (0, 2, 14, 40, 70)
    for b, k in enumerate(ks):
        tr.obs_new[b, :k] = 0
    core, poses, dims = gpu_replay(tr, tg.dim_cap(L), T)
    finals = []
    for b in range(B):
        o = CFilter("ukf", tg.dim_cap(L))
        po, do = o.replay(tr[b])
        if o.N > 3:
            assert_pd(o.state()[2], f"b={b}")
        assert_replay_parity(core, b, poses[b], dims[b], o, po, do, f"ukf large lagging b={b} (first message at {ks[b]})")
        finals.append(o.N)
    assert finals == [163, 163, 163, 17, 3], finals


def test_batch_through_the_whole_chain(built):
    """40 copies of one trajectory: filter indices beyond 8 in every kernel of the chain; identical inputs must give identical pose streams"""
    from oracle.c_oracle import CFilter

    L, T, B = 80, 70, 40
    tr = tg.make_traces(L, T, seed=65).select([0] * B)
    core, poses, dims = gpu_replay(tr, tg.dim_cap(L), T)
    differing = [b for b in range(B) if not np.array_equal(poses[b], poses[0]) or not np.array_equal(dims[b], dims[0])]
    assert not differing, f"{len(differing)} of {B} identical trajectories left the pose stream of filter 0 (first: {differing[:5]})"
    o = CFilter("ukf", tg.dim_cap(L))
    po, do = o.replay(tr[0])
    assert o.N == 163
    assert_pd(o.state()[2], "batch 40")
    assert_replay_parity(core, 0, poses[0], dims[0], o, po, do, "ukf large batch 40, filter 0")
    X0, _, P0 = core.state(0)
    for b in (7, 8, 39):
        X, _, P = core.state(b)
        assert core.status(b) == 0 and np.array_equal(X, X0) and np.array_equal(P, P0), f"filter {b} differs from filter 0"
