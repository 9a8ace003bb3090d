"""-m gpu: the per-callback innovation statistics (aslam_replay_stats, aslam_innovation_enable / aslam_get_innovation) of every kernel family
against tests/innovation_ref.py -- the NumPy oracle with two taps -- on the same inputs.

Errors are norm-wise per trajectory (util.rel_err: max |a - b| / max |b| over the callbacks in which slam() ran): NIS is (next to) zero on the
callback that seeds X <- Z, so a per-entry ratio means nothing.  The bar is the project's 1e-6 (util.REL_TOL); S is well conditioned on these
inputs (smallest eigenvalue >= 0.2 = R), so an error near the bar is a bug, not rounding.  The binary32 chains are compared with the fp64
chain on the same inputs at F32_STATS_TOL (measured: profiles/innovation_stats.md)."""
import functools

import numpy as np
import pytest

from awesomeslam_amd import trace as tg
from innovation_ref import StatsFilter
from util import REL_TOL, cov_err, rel_err

pytestmark = pytest.mark.gpu

# nis and logdet of the binary32 chains (fp32 G, S, L; binary64 sums) against the fp64 chain at n = 1027: the worst norm-wise deviation measured
# over the cases of test_binary32_chains_against_the_fp64_chain is 1.08e-7 (nis, right-looking chain; profiles/innovation_stats.md section 1);
# the bar is that value rounded up to the next power of ten.  A bar above 1e-4 would have been a defect (a binary32 accumulation), not a bar.
F32_STATS_TOL = 1e-6
assert F32_STATS_TOL <= 1e-4


def assert_pd(P, what):
    assert np.isfinite(P).all() and np.linalg.eigvalsh((P + P.T) / 2).min() > 0, f"{what}: the scenario must keep the oracle positive definite"


def make_core(kind, cap, **kw):
    from awesomeslam_amd.core import CFG_UKF_LARGE, Core

    return Core(kind, cap, flags=CFG_UKF_LARGE if kind == "ukf" and cap > 144 else 0, **kw)


def gpu_replay_stats(core, T, stats=True, call="replay_stats"):
    """one launch over callbacks 0 .. T-1; returns poses, dims, nis, logdet, pose_cov as host arrays (None where not asked for)"""
    import torch

    B = core.batch
    poses = torch.zeros((B, T, 3), dtype=torch.float64, device="cuda")
    dims = torch.zeros((B, T), dtype=torch.int32, device="cuda")
    nis = torch.full((B, T), 7.0, dtype=torch.float64, device="cuda")
    logdet = torch.full((B, T), 7.0, dtype=torch.float64, device="cuda")
    pcov = torch.full((B, T, 6), 7.0, dtype=torch.float64, device="cuda")
    if call == "replay":
        core.replay(0, T, poses.data_ptr(), dims.data_ptr())
    elif stats:
        core.replay_stats(0, T, poses.data_ptr(), dims.data_ptr(), nis.data_ptr(), logdet.data_ptr(), pcov.data_ptr())
    else:
        core.replay_stats(0, T, poses.data_ptr(), dims.data_ptr(), None, None, None)
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (poses, dims, nis, logdet, pcov))


@functools.lru_cache(maxsize=None)
def reference(kind, L, T, b, late, kw):
    """the reference's streams for trajectory b of make_traces(L, T, B = b + 1, **kw) with `late` callbacks before the first sensor message"""
    tr = traces(L, T, b + 1, late, kw)
    o = StatsFilter(kind, tg.dim_cap(L))
    out = o.replay_stats(tr[b])
    return out + (o.X.copy(), o.Z.copy(), o.P.copy())


def traces(L, T, B, late, kw):
    tr = tg.make_traces(L, T, B=B, **dict(kw))
    if B > 1 and late:
        tr.obs_new[1, :late] = 0  # filter 1 hears its first sensor message `late` callbacks late: cbOdom returns early until then
    return tr


def check_replay(kind, L, T, kw, dtype=None, tol=REL_TOL):
    from awesomeslam_amd.core import F64

    late, B = 3, 2
    kw = tuple(sorted(kw.items()))
    tr = traces(L, T, B, late, kw)
    core = make_core(kind, tg.dim_cap(L), batch=B, max_obs=tr.max_obs, max_wait=2048 if tg.dim_cap(L) > 144 else 256, dtype=F64 if dtype is None else dtype)
    core.set_trace(tr)
    poses, dims, nis, logdet, pcov = gpu_replay_stats(core, T)
    worst = 0.0
    for b in range(B):
        po, do, no, lo, co, ran, Xo, Zo, Po = reference(kind, L, T, b, late if b else 0, kw)
        if kind == "ukf":
            assert_pd(Po, f"{kind} L={L} b={b}")
        assert ran.any() and (b == 0 or not ran[:late].any())
        assert np.array_equal(dims[b], do)
        # NaN exactly where the reference's odom_msg returned 0 -- in all three arrays --, pose 0.0 there as ever
        assert np.array_equal(np.isnan(nis[b]), ~ran) and np.array_equal(np.isnan(logdet[b]), ~ran), (kind, L, b)
        assert np.array_equal(np.isnan(pcov[b]).all(axis=1), ~ran) and np.array_equal(np.isnan(pcov[b]).any(axis=1), ~ran)
        assert (poses[b][~ran] == 0.0).all()
        X, Z, P = core.state(b)
        errs = dict(nis=rel_err(nis[b][ran], no[ran]), logdet=rel_err(logdet[b][ran], lo[ran]), pose_cov=rel_err(pcov[b][ran], co[ran]),
                    pose=rel_err(poses[b][ran], po[ran]), X=rel_err(X, Xo), P=cov_err(P, Po))
        print(f"{kind} L={L} b={b} N={core.dim(b)}: rel err " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert max(errs.values()) < tol and np.array_equal(Z, Zo) and core.status(b) == 0, (kind, L, b, errs)
        worst = max(worst, max(errs.values()))
    return core, worst


# L = 5, 8 -> the two-tile kernels (n <= 31), 20 -> five tiles (n = 43), 64 -> nine tiles (n = 131): all three instantiations of both kernels
@pytest.mark.parametrize("L,T,seed", [(5, 120, 41), (8, 120, 42), (20, 100, 45), (64, 100, 46)])
@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_replay_single_cu(kind, L, T, seed, built):
    core, _ = check_replay(kind, L, T, dict(seed=seed))
    assert core.launch_info()["launches_per_callback"] == 1


@pytest.mark.parametrize("L,T,kw", [(80, 150, dict(seed=61)), (512, 42, dict(seed=71))])
def test_replay_large_ekf_fp64(L, T, kw, built):
    """the fp64 chain at n = 163 and at n = 1027 (the 42-callback window of test_gpu_large.test_config4_512_landmarks): one launch more than without"""
    core, _ = check_replay("ekf", L, T, kw)
    NB = core.layout()[0] // 64
    assert core.dim(0) == tg.full_dim(L) and core.launch_info()["launches_per_callback"] == 4 + 2 * NB + 1, core.launch_info()


@pytest.mark.parametrize("L,T,kw", [(80, 150, dict(seed=61)), (100, 80, dict(seed=62, sensor_every=2, dt_mode="random"))])
def test_replay_large_ukf(L, T, kw, built):
    """N = 163 and 203 (the traces of tests/test_gpu_ukf_large.py)"""
    core, _ = check_replay("ukf", L, T, kw)
    NB = core.layout()[0] // 64
    assert core.dim(0) == tg.full_dim(L) and core.launch_info()["launches_per_callback"] == 4 * NB + 8 + 1, core.launch_info()


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


STEP = (0.2, 0.1, 1.0)


@pytest.mark.parametrize("kind,n", [("ekf", 145), ("ekf", 189), ("ekf", 1027), ("ekf", 1087), ("ukf", 145), ("ukf", 515)])
def test_single_steps_on_synthetic_states(kind, n, built):
    """aslam_*_step and aslam_*_step_batch with aslam_innovation_enable: aslam_get_innovation against the reference; ASLAM_ERR_STATE before the
    enable call; aslam_reset keeps the setting and clears the record"""
    from awesomeslam_amd.core import AslamError

    X, Z, P = synth(n, n)
    a00, a10 = (0.07, -0.03) if kind == "ekf" else (1.0, 0.0)
    o = StatsFilter(kind, n + 2)
    o.set_state(n, X, Z, P, a00, a10)
    o.slam(np.float32(STEP[0]), np.float32(STEP[1]), np.float32(STEP[2]))
    if kind == "ukf":
        assert_pd(o.P, f"ukf n={n}")
    assert np.linalg.eigvalsh((o.S + o.S.T) / 2).min() >= 0.2 * (1 - 1e-9) or kind == "ukf"
    B = 2
    core = make_core(kind, n + 1 if kind == "ekf" else n + 2, batch=B, max_obs=4, max_wait=4)  # (the caps of test_gpu_large / test_gpu_ukf_large)
    with pytest.raises(AslamError, match="-4"):  # ASLAM_ERR_STATE
        core.innovation(1)
    core.enable_innovation()
    assert all(np.isnan(v) for v in core.innovation(1))  # no callback yet
    # the step of one filter
    core.set_state(1, n, X, Z, P)
    if kind == "ekf":
        core.ekf_step(1, *STEP, Z, a00, a10)
    else:
        core.ukf_step(1, *STEP, Z)
    one = core.innovation(1)
    assert all(np.isnan(v) for v in core.innovation(0))  # the other filter has not stepped
    info_on = core.launch_info()["launches_per_callback"]
    # the batched step: both filters from the same state
    core.reset()
    assert all(np.isnan(v) for v in core.innovation(1))  # reset: values cleared, setting kept
    for b in range(B):
        core.set_state(b, n, X, Z, P)
    f = lambda v: np.full(B, v, np.float32)  # noqa: E731
    Zs = np.tile(Z, (B, 1))
    if kind == "ekf":
        core.step_batch(f(STEP[0]), f(STEP[1]), f(STEP[2]), Zs, np.full(B, a00), np.full(B, a10))
    else:
        core.step_batch(f(STEP[0]), f(STEP[1]), f(STEP[2]), Zs)
    core.sync()
    batch = [core.innovation(b) for b in range(B)]
    for what, (nis, ld) in (("step", one), ("step_batch b=0", batch[0]), ("step_batch b=1", batch[1])):
        en, el = abs(nis - o.nis) / abs(o.nis), abs(ld - o.logdet) / abs(o.logdet)
        print(f"{kind} n={n} {what}: nis {nis:.9g} (ref {o.nis:.9g}, rel err {en:.2e}) logdet {ld:.9g} (ref {o.logdet:.9g}, rel err {el:.2e})")
        assert max(en, el) < REL_TOL, (kind, n, what)
    assert cov_err(core.state(1)[2], o.P) < REL_TOL and core.status(0) == 0 and core.status(1) == 0
    # switched off again: the seam launches what it launched before, and the getter refuses
    core.enable_innovation(False)
    core.step_batch(*((f(STEP[0]), f(STEP[1]), f(STEP[2]), Zs) + ((np.full(B, a00), np.full(B, a10)) if kind == "ekf" else ())))
    core.sync()
    assert core.launch_info()["launches_per_callback"] == info_on - 1
    with pytest.raises(AslamError, match="-4"):
        core.innovation(0)


@functools.lru_cache(maxsize=None)
def fp64_chain_1027():
    """the 512-landmark trajectory (n = 1027, 42 callbacks) through the fp64 chain at batch 1, with statistics"""
    from awesomeslam_amd.core import Core, F64

    L, T = 512, 42
    tr = tg.make_traces(L, T, B=1, seed=71)
    core = Core("ekf", tg.dim_cap(L), batch=1, max_obs=tr.max_obs, max_wait=2048, dtype=F64)
    core.set_trace(tr)
    out = gpu_replay_stats(core, T)
    assert core.status(0) == 0 and core.dim(0) == 1027
    core.close()
    return tr, out


@pytest.mark.parametrize("B,chain", [(1, "right"), (40, "resident")])
def test_binary32_chains_against_the_fp64_chain(B, chain, built, monkeypatch):
    """n = 1027 in binary32 mode: batch 1 runs the right-looking few-filter chain, batch 40 the resident bf16-pipe chain in three stream groups
    (filter indices >= 8, shifted views) -- asserted from aslam_get_launch_info.  nis and logdet against the fp64 chain on the same inputs at
    F32_STATS_TOL; pose_cov against the oracle at the 1e-6 of that path (test_gpu_large.F32_TOL)."""
    from awesomeslam_amd.core import Core, F32

    for k in ("ASLAM_CHOL_RESIDENT", "ASLAM_LARGE_GROUPS", "ASLAM_RIGHT_STEP", "ASLAM_BF16_PIPE", "ASLAM_KEEP_L32"):
        monkeypatch.delenv(k, raising=False)
    L, T = 512, 42
    tr1, (p64, d64, n64, l64, c64) = fp64_chain_1027()
    tr = tr1.select([0] * B)
    core = Core("ekf", tg.dim_cap(L), batch=B, max_obs=tr.max_obs, max_wait=2048, dtype=F32)
    core.set_trace(tr)
    poses, dims, nis, logdet, pcov = gpu_replay_stats(core, T)
    info, name = core.launch_info(), core.kernel_info()["name"]
    NB = core.layout()[0] // 64
    if chain == "right":
        assert info["launches_per_callback"] == 5 + NB + 1 and not info["chol_resident"] and info["stream_groups"] == 1 and "large_right_step" in name, (info, name)
    else:
        assert info["launches_per_callback"] == 6 + 1 and info["chol_resident"] and info["stream_groups"] == 3 and "large_chol_bf16" in name and "large_trsm_bf16" in name, (info, name)
    co = reference("ekf", L, T, 0, 0, (("seed", 71),))[4]
    ran = ~np.isnan(n64[0])
    assert ran.all()
    for b in sorted({0, B - 1, min(8, B - 1), min(17, B - 1)}):
        assert np.array_equal(dims[b], d64[0]) and core.status(b) == 0
        en, el, ec = rel_err(nis[b], n64[0]), rel_err(logdet[b], l64[0]), rel_err(pcov[b], co)
        print(f"f32 {chain} chain n=1027 B={B} b={b}: nis {en:.2e} logdet {el:.2e} against the fp64 chain; pose_cov {ec:.2e} against the oracle")
        assert max(en, el) < F32_STATS_TOL and ec < REL_TOL, (chain, b, en, el, ec)


@pytest.mark.parametrize("kind,L,T,dtype", [("ekf", 8, 100, "f64"), ("ukf", 8, 100, "f64"), ("ekf", 80, 60, "f32"), ("ukf", 80, 60, "f64")])
def test_unused_means_unchanged(kind, L, T, dtype, built):
    """aslam_replay, aslam_replay_stats with three NULL pointers and aslam_replay_stats with all three set: bit-identical poses, X and P; the
    first two also report the same launch shape"""
    from awesomeslam_amd.core import F32, F64

    tr = tg.make_traces(L, T, B=2, seed=65)
    runs = {}
    for how in ("replay", "stats-null", "stats"):
        core = make_core(kind, tg.dim_cap(L), batch=2, max_obs=tr.max_obs, max_wait=2048 if L > 70 else 256, dtype=F32 if dtype == "f32" else F64)
        core.set_trace(tr)
        out = gpu_replay_stats(core, T, stats=how == "stats", call="replay" if how == "replay" else "replay_stats")
        runs[how] = (out, [core.state(b) for b in range(2)], core.launch_info())
        if how != "stats":
            assert (out[2] == 7.0).all() and (out[3] == 7.0).all() and (out[4] == 7.0).all()  # untouched
        core.close()
    base = runs["replay"]
    for how in ("stats-null", "stats"):
        out, states, info = runs[how]
        assert np.array_equal(out[0], base[0][0]) and np.array_equal(out[1], base[0][1]), how
        for b in range(2):
            for a, c in zip(states[b], base[1][b]):
                assert np.array_equal(a, c), (how, b)
    assert runs["stats-null"][2] == base[2]
    assert runs["stats"][2]["launches_per_callback"] == base[2]["launches_per_callback"] + (1 if L > 70 else 0)
    assert np.isfinite(runs["stats"][0][2]).all() and np.isfinite(runs["stats"][0][4]).all()


@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_host_mirror_innovation_follows_the_replay_seam(kind, built):
    """Node.innovation() after each of 30 callbacks against aslam_replay_stats's stream for the same trace: NaN in the same callbacks; the
    values agree to 1e-9 (the step and the replay instantiation of the kernel do the same binary64 arithmetic on a well-conditioned S, they
    are not the same instruction stream)"""
    from awesomeslam_amd.core import AslamError, Core, Node

    L, T = 8, 30
    trs = tg.make_traces(L, T, B=1, seed=3)
    trs.obs_new[0, :2] = 0
    tr = trs[0]
    core = Core(kind, tg.dim_cap(L), batch=1, max_obs=trs.max_obs, max_wait=256)
    core.set_trace(trs)
    core.enable_innovation()
    _, _, nis, logdet, _ = gpu_replay_stats(core, T)
    last = core.innovation(0)
    assert last == (nis[0, -1], logdet[0, -1])  # the record of aslam_replay's last callback is the stream's last entry
    node = Node(kind, tg.dim_cap(L))
    with pytest.raises(AslamError):
        node.innovation()
    node.enable_innovation()
    got = np.full((T, 2), np.nan)
    ran = np.zeros(T, bool)
    for t in range(T):
        if tr.obs_new[t]:
            k = int(tr.n_obs[t])
            node.sensor_msg(tr.obs[t, :k, 0], tr.obs[t, :k, 1])
        ran[t] = bool(node.odom_msg(tr.odom[t], tr.dt[t]))
        got[t] = node.innovation()
    assert not ran[:2].any() and ran[2:].all()
    assert np.array_equal(np.isnan(got[:, 0]), ~ran) and np.array_equal(np.isnan(got[:, 1]), ~ran) and np.array_equal(np.isnan(nis[0]), ~ran)
    en, el = rel_err(got[ran, 0], nis[0][ran]), rel_err(got[ran, 1], logdet[0][ran])
    print(f"host mirror {kind}: nis {en:.2e} logdet {el:.2e} against the replay seam")
    assert max(en, el) < 1e-9
