"""-m gpu: the sighted-only EKF update (aslam_sighted_update_enable) in every EKF kernel family, against tests/sighted_ref.SightedFilter -- the
NumPy oracle with the row-selected update.

Bars (the project's own): util.REL_TOL = 1e-6 for fp64, norm- and block-wise through cov_err; test_gpu_large.F32_TOL = 1e-6 for binary32 products
against the fp64 model.  Bookkeeping is exact: Z, dimensions, wait-list, the mask against the model's, last_seen / hits.
The traces: the three limited-range traces of test_sighted_host.TABLE (contexts of capacity 12, 24 and 40 landmarks: the two-, five- and nine-tile
kernels; the limited range lets them map 5, 10 and 23), a 64-landmark trace (n = 131) cut to the median range after the warm-up, and for the launch chains the 80- and 96-landmark traces at 17 m / 18 m
(n = 163, and n = 195 = 3 x 64 + 3: the border).  Every model run is computed once per (trace, length) and shared."""
import functools

import numpy as np
import pytest

import prune_ref
from awesomeslam_amd import trace as tg
from sighted_ref import SightedFilter
from test_gpu_large import F32_TOL, chol_mode
from test_gpu_snapshot import final, run, same
from test_sighted_host import TABLE, table_trace
from util import REL_TOL, cov_err, rel_err

pytestmark = pytest.mark.gpu

T_SMALL = 150  # callbacks of a single-CU case
R64 = 15.9     # the median range of the 64-landmark trace behind its warm-up: 37 - 63 % of the landmarks sighted (asserted below)


@functools.lru_cache(maxsize=None)
def world(name):
    """name -> (trajectory, landmarks of the world)"""
    if name.startswith("table"):
        return table_trace(int(name[5:])), TABLE[int(name[5:])][0]
    if name == "L64":
        tr = tg.make_traces(64, 70, seed=5)[0]
        return tg.limit_range(tr, R64, tr.warmup), 64
    if name == "L80":
        return tg.limit_range(tg.make_traces(80, 62, seed=5)[0], 17.0, 42), 80
    if name == "L96":
        return tg.limit_range(tg.make_traces(96, 62, seed=5)[0], 18.0, 42), 96
    if name == "blind":  # trace 1 of the table with no observation at all from callback 60 on: an empty mask in every callback behind it
        return tg.limit_range(table_trace(0), 0.0, 60), 12
    if name == "open":   # everything in view
        return tg.make_traces(12, 120, seed=3)[0], 12
    raise KeyError(name)


def as_trace(trajs, max_obs=None):
    """trajectories of equal length as one Trace (observations padded to the widest message)"""
    mo = max_obs or max(t.max_obs for t in trajs)
    obs = np.zeros((len(trajs), trajs[0].T, mo, 2), np.float32)
    for b, t in enumerate(trajs):
        obs[b, :, : t.max_obs] = t.obs
    st = lambda k: np.stack([getattr(t, k) for t in trajs])  # noqa: E731
    return tg.Trace(st("odom"), st("dt"), st("obs_new"), st("n_obs"), obs, np.zeros((len(trajs), 0, 2)), None, trajs[0].warmup)


class Run:
    """the model on one trajectory, callback by callback: everything a test compares, frozen"""

    def __init__(self, name, T, cap, cut=None, drop=()):
        tr, _ = world(name)
        f = SightedFilter("ekf", cap)
        self.poses, self.dims, self.masks, self.nis, self.logdet, self.ran = np.zeros((T, 3)), np.zeros(T, np.int32), [], np.zeros(T), np.zeros(T), np.zeros(T, bool)
        for t in range(T):
            if t == cut:  # a prune between two callbacks
                import sightings_ref

                sightings_ref.compact(f, list(drop))
                f.mask = np.zeros(len(f.hits), np.uint8)
            n_before = f.init_z
            p, d = prune_ref.step_from(f, tr, t, t + 1)
            self.poses[t], self.dims[t] = p[0], d[0]
            self.ran[t] = not (n_before and not tr.obs_new[t])
            self.masks.append(f.mask.copy())
            self.nis[t], self.logdet[t] = (f.nis, f.logdet) if self.ran[t] else (np.nan, np.nan)
            if t + 1 in (T // 2, T):
                setattr(self, "half" if t + 1 == T // 2 else "end", (f.X.copy(), f.Z.copy(), f.P.copy(), f.sightings(), [np.array(c) for c in zip(*f.wait)] if f.wait else None))
        self.N = f.N
        for a in (self.poses, self.dims, self.nis, self.logdet):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def model(name, T, cap, cut=None, drop=()):
    return Run(name, T, cap, cut, drop)


def cap_of(name):
    """MAX_LANDMARK_COUNT of the contexts (and of the models) of a world; the two large worlds share the 96-landmark capacity: one batch"""
    return tg.dim_cap(96 if name in ("L80", "L96") else world(name)[1])


def make(trace, cap, dtype="f64", sighted=True, max_wait=None):
    from awesomeslam_amd.core import Core, F32, F64

    core = Core("ekf", cap, batch=trace.B, max_obs=trace.max_obs, max_wait=max_wait or (2048 if cap > 144 else 256), dtype=F32 if dtype == "f32" else F64)
    core.set_trace(trace)
    if sighted:
        core.sighted_only()
    return core


def check_state(core, b, ref, tol, what):
    """X, P at the bar; Z, the mask, the sighting record exact.  ref: (X, Z, P, sightings, wait), mask"""
    (Xo, Zo, Po, (seen, hits, clk), _), mask = ref
    X, Z, P = core.state(b)
    assert np.array_equal(Z, Zo), what
    assert np.array_equal(core.sighted(b), mask), (what, core.sighted(b), mask)
    s, h, c = core.sightings(b)
    assert c == clk and np.array_equal(s, seen) and np.array_equal(h, hits), what
    errs = rel_err(X, Xo), cov_err(P, Po)
    assert np.array_equal(P, P.T), what
    assert max(errs) < tol and core.status(b) == 0, (what, errs, core.status(b))
    return errs


# ---- 1. single-CU replay parity, every tile count -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,NP", [("table0", 32), ("table1", 80), ("table2", 144), ("L64", 144)])
def test_single_cu_replay_parity(name, NP, built):
    tr, L = world(name)
    T = min(T_SMALL, tr.T)
    m = model(name, T, tg.dim_cap(L))
    frac = [k.mean() for k in m.masks[tr.warmup:] if len(k)]
    if name == "L64":
        assert 0.25 <= min(frac) and max(frac) <= 0.75, (min(frac), max(frac))
    assert min(frac) < 1.0  # (landmarks do leave the view: the stale update is metres away on these traces)
    core = make(as_trace([tr]), tg.dim_cap(L))
    assert core.layout()[0] == NP and "true" in core.kernel_info()["name"]
    p0, d0 = run(core, 0, T // 2)  # two launches: the state and the mask round-trip through HBM
    e0 = check_state(core, 0, (m.half, m.masks[T // 2 - 1]), REL_TOL, (name, "half"))
    p1, d1 = run(core, T // 2, T - T // 2)
    e1 = check_state(core, 0, (m.end, m.masks[T - 1]), REL_TOL, (name, "end"))
    poses, dims = np.concatenate([p0[0], p1[0]]), np.concatenate([d0[0], d1[0]])
    ep = rel_err(poses, m.poses)
    assert np.array_equal(dims, m.dims) and ep < REL_TOL, (name, ep)
    if m.end[4] is not None:
        for a, c in zip(core.wait_list(0), m.end[4]):
            assert np.array_equal(a, c.astype(a.dtype))
    print(f"sighted single-CU {name} n={m.N} sighted {min(frac):.2f}-{max(frac):.2f}: rel err pose {ep:.2e}, X/P half {e0[0]:.2e} {e0[1]:.2e}, end {e1[0]:.2e} {e1[1]:.2e}")
    core.close()


# ---- 2. the empty mask and the full mask -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T", [("blind", 90), ("open", 120)])
def test_empty_and_full_mask(name, T, built):
    tr, L = world(name)
    m = model(name, T, tg.dim_cap(L))
    if name == "blind":
        assert all(not k.any() for k in m.masks[60:]) and m.N > 3  # landmarks mapped, none sighted: the pose rows alone
    else:
        assert all(k.all() for k in m.masks[tr.warmup + 1:]) and m.N == tg.full_dim(L)
    core = make(as_trace([tr]), tg.dim_cap(L))
    poses, dims = run(core, 0, T)
    e = check_state(core, 0, (m.end, m.masks[-1]), REL_TOL, name)
    ep = rel_err(poses[0], m.poses)
    print(f"sighted {name} n={m.N}: rel err pose {ep:.2e} X {e[0]:.2e} P {e[1]:.2e}")
    assert np.array_equal(dims[0], m.dims) and ep < REL_TOL
    core.close()


# ---- 3. statistics ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,T", [("table0", "f64", 150), ("table2", "f64", 150), ("L80", "f64", 62)])
def test_statistics_are_those_of_the_selected_rows(name, dtype, T, built):
    import torch

    tr, L = world(name)
    m = model(name, T, cap_of(name))
    core = make(as_trace([tr]), cap_of(name), dtype)
    nis = torch.zeros((1, T), dtype=torch.float64, device="cuda")
    logdet = torch.zeros((1, T), dtype=torch.float64, device="cuda")
    core.replay_stats(0, T, None, None, nis.data_ptr(), logdet.data_ptr(), None)
    torch.cuda.synchronize()
    nis, logdet = nis.cpu().numpy()[0], logdet.cpu().numpy()[0]
    assert np.array_equal(np.isnan(nis), ~m.ran) and np.array_equal(np.isnan(logdet), ~m.ran)
    en, el = rel_err(nis[m.ran], m.nis[m.ran]), rel_err(logdet[m.ran], m.logdet[m.ran])
    print(f"sighted statistics {name} {dtype} n={m.N}: rel err nis {en:.2e} logdet {el:.2e}")
    assert max(en, el) < REL_TOL and core.status(0) == 0
    check_state(core, 0, (m.end, m.masks[-1]), REL_TOL, name)
    core.close()


# ---- 4. the launch chains of the large-state path ---------------------------------------------------------------------------------------
LARGE_T = 62


@pytest.mark.parametrize("chain,B", [("f64", 1), ("f32", 2), ("f32-auto", 32)])
def test_large_state_parity(chain, B, built, monkeypatch):
    if chain == "f32-auto":  # the library's own choice at 32 filters: the resident bf16 Cholesky / TRSM, with the border
        for k in ("ASLAM_CHOL_RESIDENT", "ASLAM_RIGHT_STEP", "ASLAM_BF16_PIPE", "ASLAM_SYRK_RUNNING", "ASLAM_BORDER", "ASLAM_GS_TILES", "ASLAM_KEEP_L32"):
            monkeypatch.delenv(k, raising=False)
        dtype = "f32"
    else:
        dtype = chol_mode(chain, monkeypatch)
    names = ["L80", "L96"]
    cap = tg.dim_cap(96)
    trajs = [world(names[b % 2])[0] for b in range(B)]  # B = 1: n = 163 alone; else the two repeated: dimensions 163 and 195 in one batch
    core = make(as_trace(trajs, 96), cap, dtype)
    poses, dims = run(core, 0, LARGE_T)
    info, kname = core.launch_info(), core.kernel_info()["name"]
    NB = core.layout()[0] // 64
    if chain == "f64":
        assert info["launches_per_callback"] == 4 + 2 * NB and "large_update_panel<double>" in kname, (info, kname)
    elif chain == "f32":
        assert info["launches_per_callback"] == 5 + NB and not info["chol_resident"] and "large_right_step" in kname, (info, kname)
    else:
        assert info["chol_resident"] and info["launches_per_callback"] == 6 and "large_chol_bf16" in kname and "large_trsm_bf16" in kname and "border" in kname, (info, kname)
    assert "sighted" in kname
    tol = REL_TOL if dtype == "f64" else F32_TOL
    for b in sorted({0, 1, B - 2, B - 1} & set(range(B))):
        tr = trajs[b]
        m = model(names[b % 2], LARGE_T, cap)
        frac = [k.mean() for k in m.masks[42:]]
        assert (0.36 <= min(frac) and max(frac) <= 0.65) if b % 2 == 0 else (0.55 <= min(frac) and max(frac) <= 0.68), (b, min(frac), max(frac))
        assert m.N == (163, 195)[b % 2]
        e = check_state(core, b, (m.end, m.masks[-1]), tol, (chain, b))
        ep = rel_err(poses[b], m.poses)
        print(f"sighted large {chain} B={B} b={b} n={m.N}: rel err pose {ep:.2e} X {e[0]:.2e} P {e[1]:.2e}")
        assert np.array_equal(dims[b], m.dims) and ep < tol, (chain, b, ep)
    core.close()


# ---- 5. the per-callback seams ------------------------------------------------------------------------------------------------------------
def front_end(tr, f, t):
    """callback t of the model up to slam(): what a host that did the association hands to the seam (Z, A, the mask, slam()'s binary32 arguments)"""
    o = tr.odom[t]
    if tr.obs_new[t]:
        k = int(tr.n_obs[t])
        f.sensor_msg(tr.obs[t, :k, 0], tr.obs[t, :k, 1])
    assert not f.init_z and not f.init_x
    f._update_z(o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], tr.dt[t])
    return np.float32(o[6]), np.float32(o[7]), np.float32(tr.dt[t])


def test_batched_seam_with_masks_from_the_model(built):
    B, T0, T1 = 4, 60, 100
    tr, L = world("table0")
    cap = tg.dim_cap(L)
    trs = [tr, world("blind")[0], tr, world("blind")[0]]
    core = make(as_trace(trs), cap)
    models = []
    for b in range(B):
        f = SightedFilter("ekf", cap)
        prune_ref.step_from(f, trs[b], 0, T0 - b)  # (the filters of a batch are at different callbacks of their traces)
        models.append(f)
        core.set_state(b, f.N, f.X, f.Z, f.P)
    ld, NP = core.landmark_capacity(), core.layout()[0]
    for t in range(T0, T1):
        Z, mask = np.zeros((B, NP)), np.zeros((B, ld), np.uint8)
        vx, az, dt = (np.zeros(B, np.float32) for _ in range(3))
        a00, a10 = np.zeros(B), np.zeros(B)
        for b, f in enumerate(models):
            n0 = f.N
            vx[b], az[b], dt[b] = front_end(trs[b], f, t - b)
            if f.N > n0:  # a promotion: the host grows the filter, as the mirror does
                core.grow(b, f.N, f.X[n0:], f.Z[n0:])
            Z[b, : f.N], mask[b, : len(f.mask)], a00[b], a10[b] = f.Z, f.mask, f.A[0, 0], f.A[1, 0]
            f.slam(vx[b], az[b], dt[b])
        core.step_batch(vx, az, dt, Z, a00, a10, sighted=mask)
        core.sync()
    for b, f in enumerate(models):
        X, _, P = core.state(b)
        e = rel_err(X, f.X), cov_err(P, f.P)
        print(f"sighted batched seam b={b} n={f.N}: rel err X {e[0]:.2e} P {e[1]:.2e}")
        assert max(e) < REL_TOL and np.array_equal(core.sighted(b), f.mask) and core.status(b) == 0
    # the plain seam under the mode is the _sighted seam with all ones, bit for bit
    other = make(as_trace(trs), cap)
    for b, f in enumerate(models):
        other.set_state(b, f.N, *core.state(b))
    core.step_batch(vx, az, dt, Z, a00, a10)
    other.step_batch(vx, az, dt, Z, a00, a10, sighted=np.ones((B, ld), np.uint8))
    core.sync()
    for b in range(B):
        assert same(core.state(b), other.state(b)) and core.sighted(b).all() and other.sighted(b).all()
    core.close()
    other.close()


def test_single_seam_plain_equals_all_ones(built):
    tr, L = world("table0")
    cap = tg.dim_cap(L)
    f = SightedFilter("ekf", cap)
    prune_ref.step_from(f, tr, 0, 80)
    a, b = make(as_trace([tr]), cap), make(as_trace([tr]), cap)
    for c in (a, b):
        c.set_state(0, f.N, f.X, f.Z, f.P)
    Xa = a.ekf_step(0, 0.1, 0.05, 1.0, f.Z, 0.3, -0.2)
    Xb = b.ekf_step(0, 0.1, 0.05, 1.0, f.Z, 0.3, -0.2, sighted=np.ones(L, np.uint8))
    assert np.array_equal(Xa, Xb) and same(a.state(0), b.state(0)) and a.sighted(0).all() and b.sighted(0).all()
    # and a real mask changes the result
    m = np.ones(L, np.uint8)
    m[::2] = 0
    Xc = b.ekf_step(0, 0.1, 0.05, 1.0, f.Z, 0.3, -0.2, sighted=m)
    Xd = a.ekf_step(0, 0.1, 0.05, 1.0, f.Z, 0.3, -0.2)
    assert not np.array_equal(Xc, Xd) and np.array_equal(b.sighted(0), m[: (f.N - 3) // 2]) and f.N > 5
    a.close()
    b.close()


def test_node_with_sighted_only(built):
    from awesomeslam_amd.core import Node

    tr, L = world("table0")
    T = T_SMALL
    m = model("table0", T, tg.dim_cap(L))
    node = Node("ekf", tg.dim_cap(L))
    node.set_sighted_only(True)
    poses, dims = node.replay(tr, T)
    X, Z, _, _ = node.state()
    e = rel_err(poses, m.poses), rel_err(X, m.end[0]), cov_err(node.P(), m.end[2])
    print(f"sighted host mirror n={m.N}: rel err pose {e[0]:.2e} X {e[1]:.2e} P {e[2]:.2e}")
    assert np.array_equal(dims, m.dims) and np.array_equal(Z, m.end[1]) and max(e) < REL_TOL
    node.close()


# ---- 6. off means untouched ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("table0", "f64"), ("L80", "f32")])
def test_off_means_untouched(name, dtype, built, monkeypatch):
    if dtype == "f32":
        chol_mode("f32", monkeypatch)
    tr, L = world(name)
    T = 62
    cap = cap_of(name)
    trace = as_trace([tr, tr])
    never = make(trace, cap, dtype, sighted=False)
    name_off = never.kernel_info()["name"]
    p_never, d_never = run(never, 0, T)
    toggled = make(trace, cap, dtype, sighted=True)
    assert toggled.kernel_info()["name"] != name_off
    toggled.sighted_only(False)
    assert toggled.kernel_info()["name"] == name_off
    other = make(trace, cap, dtype, sighted=True)  # a second context with the mode on, running in between
    run(other, 0, T // 2)
    p_tog, d_tog = run(toggled, 0, T)
    run(other, T // 2, T - T // 2)
    assert np.array_equal(p_never, p_tog) and np.array_equal(d_never, d_tog)
    m = model(name, T, cap)
    for b in range(2):
        assert same(final(never, b), final(toggled, b))
        # the mask is written with the mode off as well.  The stale update associates as the model does only while their states agree: the mask
        # is compared right behind the warm-up (below), the final one only for its shape
        assert len(never.sighted(b)) == (never.dim(b) - 3) // 2
        assert not same(final(never, b), final(other, b))
    never.reset()
    run(never, 0, 44)
    assert np.array_equal(never.sighted(0), m.masks[43]) and m.masks[43].any(), (never.sighted(0), m.masks[43])
    for c in (never, toggled, other):
        c.close()


def test_ukf_contexts_refuse_the_mode(built):
    from awesomeslam_amd.core import AslamError, CFG_UKF_LARGE, Core

    for cap, flags in ((tg.dim_cap(8), 0), (tg.dim_cap(80), CFG_UKF_LARGE)):
        c = Core("ukf", cap, batch=1, max_obs=8, max_wait=2048 if flags else 64, flags=flags)
        with pytest.raises(AslamError, match="error -3"):  # ASLAM_ERR_UNSUPPORTED
            c.sighted_only()
        c.close()


# ---- 7. life cycle ----------------------------------------------------------------------------------------------------------------------------
def test_reset_keeps_the_mode_and_clears_the_mask(built):
    tr, L = world("table0")
    cap = tg.dim_cap(L)
    core = make(as_trace([tr]), cap)
    run(core, 0, 80)
    assert core.sighted(0).any()
    core.reset()
    assert core.dim(0) == 3 and len(core.sighted(0)) == 0 and "true" in core.kernel_info()["name"]
    run(core, 0, 80)
    m = model("table0", 80, cap)
    check_state(core, 0, (m.end, m.masks[-1]), REL_TOL, "after reset")
    core.close()


def test_prune_in_the_middle_zeroes_the_mask_and_parity_continues(built):
    tr, L = world("table0")
    cap = tg.dim_cap(L)
    cut, drop, T = 80, (1, 3), 140
    m = model("table0", T, cap, cut, drop)
    core = make(as_trace([tr]), cap)
    run(core, 0, cut)
    assert core.sighted(0).any()
    core.remove_landmarks(list(drop), traj=0)
    assert len(core.sighted(0)) == (m.dims[cut - 1] - 3) // 2 - len(drop) and not core.sighted(0).any()
    poses, dims = run(core, cut, T - cut)
    e = check_state(core, 0, (m.end, m.masks[-1]), REL_TOL, "after the prune")
    ep = rel_err(poses[0], m.poses[cut:])
    print(f"sighted prune at {cut}: n={m.N} rel err pose {ep:.2e} X {e[0]:.2e} P {e[1]:.2e}")
    assert np.array_equal(dims[0], m.dims[cut:]) and ep < REL_TOL
    core.close()


def test_restore_zeroes_the_mask_and_does_not_carry_the_mode(built):
    tr, L = world("table0")
    cap = tg.dim_cap(L)
    a = make(as_trace([tr]), cap)
    run(a, 0, 80)
    blob, n80 = a.snapshot(), a.dim(0)
    pa, da = run(a, 80, 40)
    b = make(as_trace([tr]), cap, sighted=False)  # the snapshot does not switch the mode on ...
    b.restore(blob)
    assert b.dim(0) == n80 and not b.sighted(0).any() and "true" not in b.kernel_info()["name"]
    b.sighted_only()  # ... and with the mode on the restored filter continues as the original did
    pb, db = run(b, 80, 40)
    assert np.array_equal(pa, pb) and np.array_equal(da, db) and same(a.state(0), b.state(0)) and np.array_equal(a.sighted(0), b.sighted(0))
    a.restore(blob)  # the mode of a context is its own: a restore keeps it
    assert a.dim(0) == n80 and not a.sighted(0).any() and "true" in a.kernel_info()["name"]
    a.close()
    b.close()
