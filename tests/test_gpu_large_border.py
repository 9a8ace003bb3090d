"""-m gpu: the border of the binary32 resident chain (large_border, ekf_large.h).  A state of n = n0 + t with n0 a multiple of 64 and t = 1 or 3 is
factored over its n0 leading columns by large_chol_bf16 / large_trsm_bf16; the t x t tail is solved in binary64 by large_x_update_rows, which then runs in
front of the syrk.  Everything here runs fp32 `Core`s with the resident chain forced (ASLAM_CHOL_RESIDENT=1: what a batch >= 32 selects by itself) and
compares with the fp64 path on the same inputs at the bars test_gpu_large.py uses for that chain.

Sizes: 64 landmarks = n 131 (t = 3, one factored block row: the smallest n whose TRSM has a history block in front of the border -- in the last ROW block),
63 = n 129 (t = 1), 96 = n 195 (n0 = 192), 128 = n 259 (n0 = 256: two 128-row syrk tiles in front of the border), and the control 65 = n 133 (t = 5: no
border).  The replays start from an empty map and grow in four stages, three filters out of step with each other, so that filters with and without a
border share the launches."""
import numpy as np
import pytest

from awesomeslam_amd import trace as tg
from test_gpu_innovation import F32_STATS_TOL, gpu_replay_stats
from test_gpu_large import F32_DRIFT_TOL, F32_SYNTH_TOL, synth
from util import block_rel_err, cov_err, rel_err

pytestmark = pytest.mark.gpu

SIZES = [64, 63, 96, 128, 65]  # landmarks: n = 131, 129, 195, 259 (border) and 133 (none)


def border_width(n):
    """large_border() of ekf_large.h"""
    n0 = n // 64 * 64
    return n - n0 if n0 >= 64 and n - n0 in (1, 3) else 0


def resident(monkeypatch, border=None):
    monkeypatch.setenv("ASLAM_CHOL_RESIDENT", "1")
    for k in ("ASLAM_BF16_PIPE", "ASLAM_KEEP_L32", "ASLAM_GS_TILES", "ASLAM_SYRK_RUNNING", "ASLAM_RIGHT_STEP", "ASLAM_LARGE_GROUPS"):
        monkeypatch.delenv(k, raising=False)
    if border is None:
        monkeypatch.delenv("ASLAM_BORDER", raising=False)
    else:
        monkeypatch.setenv("ASLAM_BORDER", border)


def cap(L):
    """MAX_LANDMARK_COUNT of the contexts: what the trace needs, and beyond 144 so that the fp64 reference is the multi-workgroup fp64 chain too
    (the single-CU kernels hold 512 wait-list entries at most; the staggered growth needs more)"""
    return max(tg.dim_cap(L), 146)


def staggered_traces(L, T, seed):
    """three trajectories that grow out of step: the landmarks of a stage appear at callbacks 0, 14, 28, 42 (trace.STOP_STEPS); filters 1 and 2 get no
    new sensor message for the 5 / 9 callbacks after each of those, so every growth step reaches them that much later than filter 0"""
    tr = tg.make_traces(L, T, B=3, seed=seed, stages=4)
    for k in range(4):
        tr.obs_new[1, tg.STOP_STEPS * k : tg.STOP_STEPS * k + 5] = 0
        tr.obs_new[2, tg.STOP_STEPS * k : tg.STOP_STEPS * k + 9] = 0
    return tr


_replays = {}


def replay(L, dtype, border, monkeypatch):
    """(poses, dims, [(X, Z, P)], [status], kernel name, launch info) of the staggered replay; computed once per (L, chain)"""
    import torch
    from awesomeslam_amd.core import Core, F32, F64

    key = (L, dtype, border)
    if key not in _replays:
        T = 75
        tr = staggered_traces(L, T, 80 + L)
        resident(monkeypatch, border)
        if dtype.endswith("-tiles"):
            monkeypatch.setenv("ASLAM_GS_TILES", "1")
        core = Core("ekf", cap(L), batch=3, max_obs=tr.max_obs, max_wait=2048, dtype=F64 if dtype == "f64" else F32)
        core.set_trace(tr)
        poses = torch.zeros((3, T, 3), dtype=torch.float64, device="cuda")
        dims = torch.zeros((3, T), dtype=torch.int32, device="cuda")
        half = 31  # two launches: the state round-trips through HBM in mid-growth
        core.replay(0, half, poses[:, :half].contiguous().data_ptr(), None)
        core.replay(half, T - half, None, None)
        torch.cuda.synchronize()
        core.reset()
        core.replay(0, T, poses.data_ptr(), dims.data_ptr())
        torch.cuda.synchronize()
        _replays[key] = (poses.cpu().numpy(), dims.cpu().numpy(), [core.state(b) for b in range(3)], [core.status(b) for b in range(3)],
                         core.kernel_info()["name"], core.launch_info())
        core.close()
    return _replays[key]


@pytest.mark.parametrize("L", SIZES)
def test_replay_with_border_against_fp64(L, built, monkeypatch):
    """X, P (norm-wise and on every block) and the pose stream of the border chain against the fp64 path over a replay from an empty map."""
    p32, d32, s32, st32, name, info = replay(L, "f32", None, monkeypatch)
    p64, d64, s64, st64, _, _ = replay(L, "f64", None, monkeypatch)
    assert "+ border" in name and "large_chol_bf16" in name and "large_trsm_bf16" in name and "large_syrk_bf16x3" in name, name
    assert info["launches_per_callback"] == 6 and info["chol_resident"], info
    assert np.array_equal(d32, d64) and st32 == st64 == [0, 0, 0]
    assert d32[0, -1] == tg.full_dim(L)
    sizes = sorted(set(int(n) for n in d32.ravel() if n > 0))
    on = [n for n in sizes if border_width(n)]
    print(f"border replay L={L}: sizes visited {sizes}, with a border {on}")
    assert bool(border_width(tg.full_dim(L))) == (L != 65)
    # what the staged growth visits (the CPU oracle's dimensions, which d32 equals): the final size, 67 = 64 + 3 on the way where a stage ends there, and
    # sizes without a border in between -- not every odd n: the generator promotes a stage's landmarks together
    want = {64: [67, 131], 63: [67, 129], 96: [195], 128: [67, 131, 195, 259], 65: []}[L]
    assert on == want and len(sizes) > len(on), (sizes, on)
    # filters with and without a border inside one launch
    mixed = sum(1 for t in range(d32.shape[1]) if len({bool(border_width(int(n))) for n in d32[:, t] if n > 0}) == 2)
    if L != 65:
        assert mixed > 0, "the staggered filters never differed in having a border"
    for b in range(3):
        (X, Z, P), (Xo, Zo, Po) = s32[b], s64[b]
        eb = block_rel_err(P, Po)
        errs = rel_err(p32[b], p64[b]), rel_err(X, Xo), rel_err(P, Po)
        print(f"border replay L={L} b={b} N={d32[b, -1]}: rel err pose/X/P = {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}  "
              f"blocks pose/cross/landmark {eb[0]:.2e} {eb[1]:.2e} {eb[2]:.2e}")
        assert np.array_equal(Z, Zo)
        assert max(errs) < F32_DRIFT_TOL and cov_err(P, Po) < F32_DRIFT_TOL


@pytest.mark.parametrize("L", [64, 63, 96, 128])
def test_knob_agreement(L, built, monkeypatch):
    """ASLAM_BORDER=0 (every block row and column through the sweeps, the X update behind the syrk) and the default agree within the same bar."""
    p1, d1, s1, st1, name1, _ = replay(L, "f32", None, monkeypatch)
    p0, d0, s0, st0, name0, info0 = replay(L, "f32", "0", monkeypatch)
    assert "+ border" in name1 and "border" not in name0 and "large_chol_bf16" in name0 and "large_trsm_bf16" in name0, (name1, name0)
    assert info0["launches_per_callback"] == 6 and info0["chol_resident"], info0
    assert np.array_equal(d1, d0) and st1 == st0 == [0, 0, 0]
    for b in range(3):
        (X, Z, P), (Xo, Zo, Po) = s1[b], s0[b]
        errs = rel_err(p1[b], p0[b]), rel_err(X, Xo), cov_err(P, Po)
        print(f"border knob L={L} b={b}: default against ASLAM_BORDER=0: rel err pose/X/P = {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
        assert np.array_equal(Z, Zo) and max(errs) < F32_DRIFT_TOL


def test_tiled_GS_with_border_is_bit_identical(built, monkeypatch):
    """large_build_GS_tiles (ASLAM_GS_TILES=1) puts the same S21 rows and the same copies of G2 into the spare rows of G as large_build_GS: every
    later number agrees bit for bit, as in test_gpu_large.test_tiled_GS_is_bit_identical, here over sizes with a border (67 and 131)."""
    p0, d0, s0, st0, _, _ = replay(64, "f32", None, monkeypatch)
    p1, d1, s1, st1, name, _ = replay(64, "f32-tiles", None, monkeypatch)
    assert "+ border" in name and st0 == st1 == [0, 0, 0] and np.array_equal(d0, d1)
    assert np.array_equal(p0, p1), f"pose streams differ: max {np.abs(p0 - p1).max():.3e}"
    for b in range(3):
        for a, c, what in zip(s0[b], s1[b], "XZP"):
            assert np.array_equal(a, c), f"{what} of filter {b} differs: max {np.abs(a - c).max():.3e}"


@pytest.mark.parametrize("L", [64, 128])
def test_covariance_stays_symmetric(L, built, monkeypatch):
    """The X update writes the pose columns with their mirror image, the syrk the rest of the lower triangle with its: exactly symmetric outside the
    pose block, whose entries go through the two roundings of the predict (the bound test_fp32_drift_over_2000_callbacks uses)."""
    _, d32, s32, _, _, _ = replay(L, "f32", None, monkeypatch)
    for b in range(3):
        P = s32[b][2]
        A = np.abs(P - P.T)
        pose = A[:3, :3].max()
        A[:3, :3] = 0.0
        print(f"border symmetry L={L} b={b} N={d32[b, -1]}: max |P - P^T| outside the pose block {A.max():.1e}, inside {pose:.1e}")
        assert A.max() == 0.0 and pose <= 1e-18


@pytest.mark.parametrize("n", [129, 131, 133, 195, 259])
def test_single_step_on_synthetic_state(n, built, monkeypatch):
    """one slam() at exactly n on a dense synthetic covariance, against the oracle, at the bar of test_gpu_large.test_single_slam_on_synthetic_state"""
    from awesomeslam_amd.core import Core, F32
    from oracle.c_oracle import CFilter

    resident(monkeypatch)
    X, Z, P = synth(n, n)
    o = CFilter("ekf", n + 1)
    o.set_state(n, X, Z, P, 0.07, -0.03)
    core = Core("ekf", n + 1, batch=2, max_obs=4, max_wait=4, dtype=F32)
    core.set_state(1, n, X, Z, P)
    for vx, az, dt in ((0.2, 0.1, 1.0), (0.15, 0.0, 0.5), (0.0, 0.0, 1.0)):
        Xg = core.ekf_step(1, vx, az, dt, Z, 0.07, -0.03)
        o.slam(vx, az, dt)
    Xo, _, Po = o.state()
    Pg = core.state(1)[2]
    ex, ep = rel_err(Xg, Xo), cov_err(Pg, Po)
    print(f"border synthetic n={n} (t={border_width(n)}): rel err X {ex:.2e} P {ep:.2e}")
    assert core.launch_info()["chol_resident"] and "+ border" in core.kernel_info()["name"]
    assert max(ex, ep) < F32_SYNTH_TOL and core.status(1) == 0 and core.dim(0) == 3


def test_statistics_at_131(built, monkeypatch):
    """per-callback NIS and ln det S with the tail of L in the border (q2 in row n of V, diag(L22)^-1 in Linv) against the fp64 path"""
    from awesomeslam_amd.core import Core, F32, F64

    L, T = 64, 75
    tr = staggered_traces(L, T, 80 + L)
    resident(monkeypatch)
    out = {}
    for name, dt in (("f32", F32), ("f64", F64)):
        core = Core("ekf", cap(L), batch=3, max_obs=tr.max_obs, max_wait=2048, dtype=dt)
        core.set_trace(tr)
        out[name] = gpu_replay_stats(core, T)
        if name == "f32":
            assert core.launch_info()["launches_per_callback"] == 7 and "+ border" in core.kernel_info()["name"]
        core.close()
    (_, d32, n32, l32, c32), (_, d64, n64, l64, c64) = out["f32"], out["f64"]
    assert np.array_equal(d32, d64) and d32[0, -1] == 131
    for b in range(3):
        ran = ~np.isnan(n64[b])
        assert ran.any() and np.array_equal(np.isnan(n32[b]), ~ran) and np.array_equal(np.isnan(l32[b]), ~ran)
        at = ran & np.array([border_width(int(n)) > 0 for n in d32[b]])
        assert at.any()
        en, el, ec = rel_err(n32[b][ran], n64[b][ran]), rel_err(l32[b][ran], l64[b][ran]), rel_err(c32[b][ran], c64[b][ran])
        print(f"border statistics b={b}: nis {en:.2e} logdet {el:.2e} pose_cov {ec:.2e} against the fp64 path ({int(at.sum())} of {int(ran.sum())} callbacks with a border)")
        assert max(en, el) < F32_STATS_TOL and ec < F32_DRIFT_TOL


def test_indefinite_border_is_flagged(built, monkeypatch):
    """A covariance whose S has a positive definite S11 (the 128 leading rows, which large_chol_bf16 factors without complaint) and an indefinite Schur
    complement C = S22 - l l^T: the bad pivot falls in the border, and large_x_update_rows must raise ASLAM_ST_NOT_PD as the Cholesky does for its
    blocks.  Same construction as test_gpu_large.test_indefinite_innovation_covariance_is_flagged (a negative landmark variance), placed on the last
    landmark; the scenario is verified on the CPU with the NumPy oracle."""
    from awesomeslam_amd.core import Core, F32, ST_NOT_PD
    from oracle import np_oracle

    resident(monkeypatch)
    n = 131
    X, Z, P = synth(n, 7)
    bad = P.copy()
    bad[130, 130] = -50.0
    o = np_oracle.NpFilter("ekf", n + 1)
    o.set_state(n, X, Z, bad, 0.07, -0.03)
    o.X = np_oracle.state_transition(n, o.X, 0.2, 0.1, 1.0)
    o.P = o.A @ o.P @ o.A.T + o.Q
    o._update_h()
    S = o.H @ o.P @ o.H.T + o.R
    S11, S21, S22 = S[:128, :128], S[128:, :128], S[128:, 128:]
    # S11 must be safely positive definite for a binary32 factorisation on the bf16 pipe (products good to ~2^-24 of sum |a b|): its smallest eigenvalue
    # has to stand far above eps32 |S11|, so that large_chol_bf16 cannot be what raises the flag -- filter 0 below, whose S has the same S11 up to the
    # one entry, also shows that.  And the bad pivot of C has to be far from zero the other way.
    ev11 = np.linalg.eigvalsh((S11 + S11.T) / 2)
    margin = ev11.min() / (np.finfo(np.float32).eps * ev11.max())
    print(f"border not-PD scenario: S11 eigenvalues {ev11.min():.3e} .. {ev11.max():.3e} (smallest = {margin:.1e} eps32 |S11|)")
    assert ev11.min() > 0 and margin > 1e4
    C = S22 - S21 @ np.linalg.solve(S11, S21.T)
    evc = np.linalg.eigvalsh((C + C.T) / 2)
    print(f"border not-PD scenario: eigenvalues of C = S22 - S21 S11^-1 S21^T {evc}")
    assert evc.min() < -1e4 * np.finfo(np.float32).eps * np.abs(S22).max()
    core = Core("ekf", n + 1, batch=2, max_obs=4, max_wait=4, dtype=F32)
    core.set_state(0, n, X, Z, P)
    core.set_state(1, n, X, Z, bad)
    core.ekf_step(0, 0.2, 0.1, 1.0, Z, 0.07, -0.03)
    core.ekf_step(1, 0.2, 0.1, 1.0, Z, 0.07, -0.03)
    assert "+ border" in core.kernel_info()["name"]
    assert core.status(0) == 0
    assert core.status(1) & ST_NOT_PD
