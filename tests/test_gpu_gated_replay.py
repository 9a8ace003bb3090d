"""-m gpu: the Mahalanobis gate inside the replay seam (aslam_set_replay_gate) in all four kernel families, against tests/gated_ref.GatedFilter
and against the device's own aslam_gate_observations.

Bars (the project's own): util.REL_TOL = 1e-6 with cov_err for X, P and the poses of the fp64 families; everything the gate decides is exact --
Z, dimensions, the wait-list, the mask, last_seen / hits / clock and the rejected counter.  The closed-loop cases run on inputs whose every
decision is at least 1e-4 from flipping (asserted on the CPU in tests/test_gated_replay_host.py); the step-locked cases compare the front end
with aslam_gate_observations on the very same device state, callback by callback, and do not depend on accumulated rounding: that is the test
of the binary32-product chains.  Every model run is computed once and shared."""

import numpy as np
import pytest

import gated_ref
from awesomeslam_amd import trace as tg
from gated_ref import GATE, GatedFilter
from oracle.np_oracle import normalize_angle
from test_gpu_large import chol_mode
from test_gpu_sighted import as_trace
from test_gpu_snapshot import final, run, same
from util import REL_TOL, cov_err, rel_err

pytestmark = pytest.mark.gpu


def make(kind, trace, cap, dtype="f64", gate=None, params=None, large_ukf=False, max_wait=None):
    from awesomeslam_amd.core import CFG_UKF_LARGE, Core, F32, F64

    core = Core(kind, cap, batch=trace.B, max_obs=trace.max_obs, max_wait=max_wait or (2048 if cap > 145 or dtype == "f32" else 512),
                dtype=F32 if dtype == "f32" else F64, flags=CFG_UKF_LARGE if large_ukf else 0)
    if params:
        core.set_params(params)
        core.reset()
    core.set_trace(trace)
    if gate is not None:
        core.set_replay_gate(gate)
    return core


def check_exact(core, b, ref, what, ekf):
    """the bookkeeping of filter b against a frozen model state: exact"""
    X, Z, P = core.state(b)
    assert core.dim(b) == ref["N"] and np.array_equal(Z, ref["Z"]), what
    seen, hits, clk = ref["sightings"]
    s, h, c = core.sightings(b)
    assert c == clk and np.array_equal(s, seen) and np.array_equal(h, hits), what
    if ekf:
        assert np.array_equal(core.sighted(b), ref["mask"]), (what, core.sighted(b), ref["mask"])
    assert core.assoc_rejected(b) == ref["rejected"], (what, core.assoc_rejected(b), ref["rejected"])
    got = core.wait_list(b, cap=2048)
    if ref["wait"] is None:
        assert len(got[0]) == 0, what
    else:
        for a, m in zip(got, ref["wait"]):
            assert np.array_equal(a, m.astype(a.dtype)), what
    return X, P


def check_state(core, b, ref, what, ekf, tol=REL_TOL):
    X, P = check_exact(core, b, ref, what, ekf)
    errs = rel_err(X, ref["X"]), cov_err(P, ref["P"])
    assert np.array_equal(P, P.T), what
    assert max(errs) < tol and core.status(b) == 0, (what, errs, core.status(b))
    return errs


def two_launches(core, T):
    p0, d0 = run(core, 0, T // 2)
    return p0, d0, lambda: run(core, T // 2, T - T // 2)


# ---- 1. closed-loop parity against the model, fp64 families --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,NP", [("ekf-12", 32), ("ekf-24-limited", 80), ("ekf-64-limited", 144), ("ukf-24-limited", 80), ("ukf-12", 32)])
def test_single_cu_closed_loop(name, NP, built):
    kind, tr, cap, params = gated_ref.case_inputs(name)
    f, poses_m, dims_m, snaps = gated_ref.run_case(name)
    T = tr.T
    core = make(kind, as_trace([tr]), cap, gate=GATE, params=params)
    assert core.layout()[0] == NP and core.replay_gate(0) == GATE
    p0, d0, rest = two_launches(core, T)  # state, gate and counter round-trip through HBM; the second launch starts from the prefetch path
    e0 = check_state(core, 0, snaps[T // 2], (name, "half"), kind == "ekf")
    p1, d1 = rest()
    e1 = check_state(core, 0, snaps[T], (name, "end"), kind == "ekf")
    poses, dims = np.concatenate([p0[0], p1[0]]), np.concatenate([d0[0], d1[0]])
    ep = rel_err(poses, poses_m)
    print(f"gated {name} n={f.N} counts {f.counts()} rejected {f.rejected}: rel err pose {ep:.2e}, X/P half {e0[0]:.2e} {e0[1]:.2e}, end {e1[0]:.2e} {e1[1]:.2e}")
    assert np.array_equal(dims, dims_m) and ep < REL_TOL
    core.close()


@pytest.mark.parametrize("name", ["ukf-24-limited", "ukf-12"])
def test_single_cu_ukf_covariance_is_exactly_symmetric(name, built):
    """The single-CU UKF leaves every callback with an exactly symmetric P, with the gate and without it: its covariance update
    (gemm_wabt<GEMM_SUBTRACT_SYM>, ukf_small.h) mirrors the off-diagonal tiles and, since the change that added this test, the two halves of
    the diagonal tiles too (before it a few entries inside the diagonal 16x16 tiles differed from their mirror image in the last bit: 34 of
    1521 at n = 39, at most 3.1e-16 of max |P|, with the gate off as well)."""
    kind, tr, cap, params = gated_ref.case_inputs(name)
    T = tr.T
    for gate in (GATE, None):
        core = make(kind, as_trace([tr]), cap, gate=gate, params=params)
        run(core, 0, T)
        _, _, P = core.state(0)
        bad = np.argwhere(P != P.T)
        print(f"single-CU UKF {name} gate {gate}: {len(bad)} of {P.size} entries differ from their mirror image, max |P - P^T| / max |P| = "
              f"{np.abs(P - P.T).max() / np.abs(P).max():.2e}")
        core.close()
        assert np.array_equal(P, P.T), (name, gate)


def test_large_ekf_f64_closed_loop_two_trajectories_in_one_batch(built, monkeypatch):
    chol_mode("f64", monkeypatch)
    names = ["ekf-80-large", "ekf-96-large"]
    ins = [gated_ref.case_inputs(n) for n in names]
    cap, params, T = ins[0][2], ins[0][3], ins[0][1].T
    core = make("ekf", as_trace([i[1] for i in ins], 96), cap, gate=GATE, params=params)
    assert "gated" in core.kernel_info()["name"] and "large_update_panel<double>" in core.kernel_info()["name"]
    p0, d0, rest = two_launches(core, T)
    models = [gated_ref.run_case(n) for n in names]
    for b, (f, _, _, snaps) in enumerate(models):
        check_state(core, b, snaps[T // 2], (names[b], "half"), True)
    p1, d1 = rest()
    for b, (f, poses_m, dims_m, snaps) in enumerate(models):
        e = check_state(core, b, snaps[T], (names[b], "end"), True)
        ep = rel_err(np.concatenate([p0[b], p1[b]]), poses_m)
        print(f"gated large f64 {names[b]} n={f.N} counts {f.counts()}: rel err pose {ep:.2e} X {e[0]:.2e} P {e[1]:.2e}")
        assert np.array_equal(np.concatenate([d0[b], d1[b]]), dims_m) and ep < REL_TOL
    core.close()


# ---- 2. step-locked, device against device ---------------------------------------------------------------------------------------------------
def step_locked(core, kind, tr, cap, params, t_from, t_to, b=0):
    """Callbacks t_from .. t_to - 1 one launch at a time.  Before each: the device state seeds a model whose gate decisions are
    aslam_gate_observations' on that state (and whose Euclidean verdicts are the oracle's binary32 arithmetic on the device's own X); the model's
    _update_z then says what the callback must do to Z, the mask, the hits, the counter and the wait-list: compared exactly.
    Returns (accepted, dropped, waitlisted, differing) over the window."""
    B = core.batch
    f = GatedFilter(kind, cap, params=params, gate=core.replay_gate(b))
    stored = None
    for t in range(t_from):  # the stored message at t_from: the last new one (the front end keeps it with normalised bearings)
        if tr.obs_new[t]:
            stored = tr.obs[t, : int(tr.n_obs[t])]
    for t in range(t_from, t_to):
        if tr.obs_new[t]:
            stored = tr.obs[t, : int(tr.n_obs[t])]
        msg = np.array([[r, normalize_angle(bb)] for r, bb in stored], np.float32).reshape(-1, 2)
        n0 = core.dim(b)
        X, Z, P = core.state(b)
        seen0, hits0, clk0 = core.sightings(b)
        rej0 = core.assoc_rejected(b)
        wr, wb, wc = core.wait_list(b, cap=2048)
        k = len(msg)
        obs = np.zeros((B, max(k, 1), 2), np.float32)
        obs[b, :k] = msg
        assoc, _ = core.gate_observations(obs, [k if i == b else 0 for i in range(B)], f.gate)
        # seed the model with the device state
        acc = f.counts()
        f.set_state(n0, X, Z, P)
        f.accepted, f.dropped, f.waitlisted, f.differing = acc
        f.wait = [[np.float32(r), np.float32(bb), int(c)] for r, bb, c in zip(wr, wb, wc)]
        f.sensor = [[np.float32(r), np.float32(bb)] for r, bb in msg]
        f.last_seen, f.hits, f.clock = seen0.copy(), hits0.copy(), int(clk0)
        f.rejected = 0
        f.decide = lambda o, a=assoc[b, :k]: a
        o = tr.odom[t]
        with f._constants():
            f._update_z(o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], tr.dt[t])
        # the callback on the device
        run(core, t, 1)
        what = (kind, "callback", t)
        assert core.dim(b) == f.N, what
        _, Z1, _ = core.state(b)
        assert np.array_equal(Z1, f.Z), (what, np.flatnonzero(Z1 != f.Z))  # which entries were rewritten, and with what
        s1, h1, c1 = core.sightings(b)
        assert c1 == f.clock and np.array_equal(s1, f.last_seen) and np.array_equal(h1, f.hits), what  # the hit increments
        if kind == "ekf":
            assert np.array_equal(core.sighted(b), f.mask), what
        assert core.assoc_rejected(b) - rej0 == f.rejected, (what, core.assoc_rejected(b) - rej0, f.rejected)
        got = core.wait_list(b, cap=2048)
        want = [np.array(c) for c in zip(*f.wait)] if f.wait else [np.zeros(0)] * 3
        for a, m in zip(got, want):
            assert np.array_equal(a, m.astype(a.dtype)), what  # pushes and count changes
    return f.counts()


def test_step_locked_single_cu_ekf(built):
    kind, tr, cap, params = gated_ref.case_inputs("ekf-24-limited")
    core = make(kind, as_trace([tr]), cap, gate=GATE, params=params)
    t0 = tr.warmup
    run(core, 0, t0)
    counts = step_locked(core, kind, tr, cap, params, t0, t0 + 40)
    print(f"step-locked single-CU EKF callbacks {t0}..{t0 + 40}: accepted/dropped/wait-listed/differing {counts}")
    assert counts[0] > 0 and counts[1] + counts[2] > 0
    core.close()


@pytest.mark.parametrize("kind,r", [("ekf", 1e-3), ("ukf", 0.05)])
def test_step_locked_single_cu_nine_tiles(kind, r, built):
    """the 9-tile instantiations (NP = 144: the landmark table over sH next to 147 / 158 KB of LDS) of both single-CU kernels, on the 64-landmark
    limited-range trace, every callback behind the warm-up.  (UKF at r = 0.05: at 0.01 it loses positive definiteness on this trace.)"""
    _, tr, cap, _ = gated_ref.case_inputs("ekf-64-limited")
    params = dict(r_range=r, r_bearing=r)
    core = make(kind, as_trace([tr]), cap, gate=GATE, params=params)
    assert core.layout()[0] == 144 and "9,0" in core.kernel_info()["name"] and "true" in core.kernel_info()["name"]
    t0 = tr.warmup
    run(core, 0, t0)
    counts = step_locked(core, kind, tr, cap, params, t0, tr.T)
    print(f"step-locked single-CU {kind} NP=144 callbacks {t0}..{tr.T} n={core.dim(0)}: accepted/dropped/wait-listed/differing {counts}")
    assert counts[0] > 0 and counts[1] + counts[2] > 0 and core.status(0) == 0
    core.close()


@pytest.mark.parametrize("chain", ["f32-auto", "f32-resident-pipe0"])
def test_step_locked_binary32_chains(chain, built, monkeypatch):
    if chain == "f32-auto":  # the library's own choice from 32 filters on: the bf16 chain
        for k in ("ASLAM_CHOL_RESIDENT", "ASLAM_RIGHT_STEP", "ASLAM_BF16_PIPE", "ASLAM_SYRK_RUNNING", "ASLAM_BORDER", "ASLAM_GS_TILES", "ASLAM_KEEP_L32"):
            monkeypatch.delenv(k, raising=False)
        B = 32
    else:  # ASLAM_BF16_PIPE=0 below 32 filters: the fp32-MFMA pair
        chol_mode(chain, monkeypatch)
        B = 2
    kind, tr, cap, params = gated_ref.case_inputs("ekf-80-large")
    core = make("ekf", as_trace([tr] * B, 96), cap, dtype="f32", gate=GATE, params=params)
    kname = core.kernel_info()["name"]
    assert "gated" in kname and (("large_chol_bf16" in kname) if chain == "f32-auto" else ("large_chol_resident" in kname)), kname
    t0 = 42  # behind the warm-up: the range limit applies from here
    run(core, 0, t0)
    counts = step_locked(core, "ekf", tr, cap, params, t0, tr.T, b=B - 1)
    print(f"step-locked {chain} B={B} callbacks {t0}..{tr.T} n={core.dim(B - 1)}: accepted/dropped/wait-listed/differing {counts}")
    assert counts[0] > 0 and counts[1] + counts[2] > 0 and core.status(B - 1) == 0
    core.close()


def test_step_locked_large_ukf(built):
    """the ASLAM_CFG_UKF_LARGE chain: step-locked (its closed loop is not compared with the NumPy model here)"""
    kind, tr, cap, _ = gated_ref.case_inputs("ekf-80-large")
    params = dict(r_range=0.05, r_bearing=0.05)  # (at 0.01 the UKF loses positive definiteness on this trace, in the NumPy model too)
    core = make("ukf", as_trace([tr]), cap, gate=GATE, params=params, large_ukf=True)
    assert "gated" in core.kernel_info()["name"]
    t0 = 42
    run(core, 0, t0)
    counts = step_locked(core, "ukf", tr, cap, params, t0, tr.T)
    print(f"step-locked large UKF callbacks {t0}..{tr.T} n={core.dim(0)}: accepted/dropped/wait-listed/differing {counts}")
    assert counts[0] > 0 and counts[1] + counts[2] > 0 and core.status(0) == 0
    core.close()


# ---- 3. per-filter gates ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_per_filter_gates(kind, built):
    name = "ekf-24-limited" if kind == "ekf" else "ukf-24-limited"
    _, tr, cap, params = gated_ref.case_inputs(name)
    T = tr.T
    trace = as_trace([tr] * 3)
    core = make(kind, trace, cap, params=params)
    for b, g in enumerate((0.0, GATE, np.inf)):
        core.set_replay_gate(g, b)
    assert [core.replay_gate(b) for b in range(3)] == [0.0, GATE, np.inf]
    never = make(kind, trace, cap, params=params)
    pg, dg = run(core, 0, T)
    pn, dn = run(never, 0, T)
    # filter 0 of the gated launch is the filter of a context that never had a gate, bit for bit
    assert same(final(core, 0), final(never, 0)) and np.array_equal(pg[0], pn[0]) and np.array_equal(dg[0], dn[0])
    assert all(np.array_equal(a, c) for a, c in zip(core.sightings(0), never.sightings(0))) and core.assoc_rejected(0) == 0
    if kind == "ekf":
        assert np.array_equal(core.sighted(0), never.sighted(0))
    f, poses_m, dims_m, snaps = gated_ref.run_case(name)
    check_state(core, 1, snaps[T], (kind, "gate 9.21"), kind == "ekf")
    assert rel_err(pg[1], poses_m) < REL_TOL and np.array_equal(dg[1], dims_m)
    finf = GatedFilter(kind, cap, params=params, gate=np.inf)
    poses_i, dims_i, snaps_i = gated_ref.run_filter(finf, tr, T)
    assert finf.dropped == 0 and finf.waitlisted == 0 and finf.accepted > 0  # with +inf nothing is dropped or wait-listed while a landmark is valid
    check_state(core, 2, snaps_i[T], (kind, "gate inf"), kind == "ekf")
    assert core.assoc_rejected(2) == 0 and np.array_equal(dg[2], dims_i)
    core.close()
    never.close()


# ---- 4. composition ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ekf-12", "ukf-12"])
def test_replay_stats_with_the_gate(name, built):
    import torch

    kind, tr, cap, params = gated_ref.case_inputs(name)
    T = tr.T
    a = make(kind, as_trace([tr]), cap, gate=GATE, params=params)
    b = make(kind, as_trace([tr]), cap, gate=GATE, params=params)
    pa, da = run(a, 0, T)
    nis, logdet = (torch.zeros((1, T), dtype=torch.float64, device="cuda") for _ in range(2))
    pcov = torch.zeros((1, T, 6), dtype=torch.float64, device="cuda")
    poses = torch.zeros((1, T, 3), dtype=torch.float64, device="cuda")
    b.replay_stats(0, T, poses.data_ptr(), None, nis.data_ptr(), logdet.data_ptr(), pcov.data_ptr())
    torch.cuda.synchronize()
    assert same(final(a, 0), final(b, 0)) and np.array_equal(pa, poses.cpu().numpy()) and a.assoc_rejected(0) == b.assoc_rejected(0) > 0
    ran = ~np.isnan(pcov.cpu().numpy()[0]).any(axis=1)
    assert ran.sum() > T // 2 and np.isfinite(nis.cpu().numpy()[0][ran]).all() and np.isfinite(logdet.cpu().numpy()[0][ran]).all()
    a.close()
    b.close()


def test_sighted_only_with_the_gate(built):
    """the natural pair: the gate decides what is sighted, the update takes those rows alone"""
    import prune_ref

    kind, tr, cap, params = gated_ref.case_inputs("ekf-24-limited")
    T = tr.T
    f = gated_ref.GatedSightedFilter("ekf", cap, params, gate=GATE)
    poses_m, dims_m = prune_ref.step_from(f, tr, 0, T)
    core = make("ekf", as_trace([tr]), cap, gate=GATE, params=params)
    core.sighted_only()
    assert "true,true" in core.kernel_info()["name"]
    p, d = run(core, 0, T)
    X, Z, P = core.state(0)
    e = rel_err(X, f.X), cov_err(P, f.P), rel_err(p[0], poses_m)
    print(f"gate + sighted-only n={f.N}: rel err X {e[0]:.2e} P {e[1]:.2e} pose {e[2]:.2e}")
    assert np.array_equal(core.sighted(0), f.mask) and np.array_equal(Z, f.Z) and np.array_equal(d[0], dims_m)
    assert max(e) < REL_TOL and core.status(0) == 0 and core.assoc_rejected(0) == f.rejected
    core.close()


# ---- 5. life cycle and refusals ------------------------------------------------------------------------------------------------------------------
def test_nothing_mapped_and_empty_messages_are_the_ungated_run(built):
    tr = tg.make_traces(12, 150, seed=3)[0]
    T = 8  # promote_count is 10: nothing is mapped yet, N == 3 throughout
    cap = tg.dim_cap(12)
    a, b = make("ekf", as_trace([tr]), cap, gate=GATE), make("ekf", as_trace([tr]), cap)
    pa, da = run(a, 0, T)
    pb, db = run(b, 0, T)
    assert (da == 3).all() and same(final(a, 0), final(b, 0)) and np.array_equal(pa, pb) and a.assoc_rejected(0) == 0
    a.close()
    b.close()
    # a mapped filter that stops receiving observations: the stored message becomes empty (range limit 0 from callback 60 on)
    blind = tg.limit_range(tr, 0.0, 60)
    f = GatedFilter("ekf", cap, dict(r_range=0.01, r_bearing=0.01), gate=GATE)
    poses_m, dims_m, snaps = gated_ref.run_filter(f, blind, 90)
    c = make("ekf", as_trace([blind]), cap, gate=GATE, params=dict(r_range=0.01, r_bearing=0.01))
    pc, dc = run(c, 0, 90)
    assert f.N > 3 and not snaps[90]["mask"].any()
    check_state(c, 0, snaps[90], "blind", True)
    assert np.array_equal(dc[0], dims_m) and rel_err(pc[0], poses_m) < REL_TOL
    c.close()


def test_reset_restore_and_refusals(built):
    from awesomeslam_amd.core import AslamError

    kind, tr, cap, params = gated_ref.case_inputs("ekf-12")
    trace = as_trace([tr, tr])
    core = make(kind, trace, cap, params=params)
    name_off = core.kernel_info()["name"]
    core.set_replay_gate(GATE, 1)
    name_on = core.kernel_info()["name"]
    assert name_on != name_off and core.replay_gate(0) == 0.0 and core.replay_gate(1) == GATE
    run(core, 0, 100)
    r100 = core.assoc_rejected(1)
    assert r100 > 0 and core.assoc_rejected(0) == 0
    blob = core.snapshot()
    # refusals change nothing
    for bad_gate, bad_traj in ((-1.0, 0), (float("nan"), 0), (GATE, 2), (GATE, -2)):
        with pytest.raises(AslamError, match="error -1"):  # ASLAM_ERR_ARG
            core.set_replay_gate(bad_gate, bad_traj)
    with pytest.raises(AslamError, match="gate"):
        core.set_replay_gate(-1.0, 0)
    with pytest.raises(AslamError, match="traj"):
        core.set_replay_gate(GATE, 7)
    assert core.replay_gate(0) == 0.0 and core.replay_gate(1) == GATE and core.assoc_rejected(1) == r100 and core.kernel_info()["name"] == name_on
    # restore into a gated context: the gate stays, the counter of the restored slot starts at zero
    core.restore(blob, records=[1], trajs=[1])
    assert core.replay_gate(1) == GATE and core.assoc_rejected(1) == 0 and core.kernel_info()["name"] == name_on
    # reset keeps the gate and zeroes the counter; the run after it is the first run again
    core.reset()
    assert core.replay_gate(1) == GATE and core.assoc_rejected(1) == 0 and core.dim(1) == 3
    run(core, 0, 100)
    assert core.assoc_rejected(1) == r100
    # a snapshot does not carry the gate
    other = make(kind, trace, cap, params=params)
    other.restore(blob)
    assert other.replay_gate(1) == 0.0 and other.kernel_info()["name"] == name_off
    # switching every gate off brings the ungated kernels back
    core.set_replay_gate(0.0)
    assert core.kernel_info()["name"] == name_off
    core.close()
    other.close()


F64_CHAIN = "large_update_panel<double> (10-launch chain per callback, 3 stream groups)"
UKF_CHAIN = "ukf_large_wabt + large_update_panel<double> + large_syrk<double> (20-launch chain per callback, 1 stream)"
F32_CHAIN = "large_right_step + large_syrk_bf16x3 (6-launch chain per callback: one right-looking launch per block column)"
# context -> (kind, landmarks of the capacity, dtype, large UKF, NP, {state: (kernel_info name, dynamic LDS bytes)}): one context per family at its
# smallest shape, batch 1.  The names are keys (bench.py prices the chain from them, profiles/pmc_traffic.json is looked up by them) and the LDS
# sizes are what the host hands the launch: both recorded from the library before the front ends got one LDS layout and one variant rule
KERNEL_INFO = {
    "ekf-2": ("ekf", 12, "f64", False, 32, {"plain": ("ekf_small_kernel<2,0>", 31064), "sighted": ("ekf_small_kernel<2,0,false,true>", 31064),
                                            "gated": ("ekf_small_kernel<2,0,false,false,true>", 31064),
                                            "gated+sighted": ("ekf_small_kernel<2,0,false,true,true>", 31064)}),
    "ekf-5": ("ekf", 24, "f64", False, 80, {"plain": ("ekf_small_kernel<5,0>", 67448), "sighted": ("ekf_small_kernel<5,0,false,true>", 67448),
                                            "gated": ("ekf_small_kernel<5,0,false,false,true>", 67448),
                                            "gated+sighted": ("ekf_small_kernel<5,0,false,true,true>", 67448)}),
    "ekf-9": ("ekf", 64, "f64", False, 144, {"plain": ("ekf_small_kernel<9,0>", 146424), "sighted": ("ekf_small_kernel<9,0,false,true>", 146424),
                                             "gated": ("ekf_small_kernel<9,0,false,false,true>", 146424),
                                             "gated+sighted": ("ekf_small_kernel<9,0,false,true,true>", 146424)}),
    "ukf-2": ("ukf", 12, "f64", False, 32, {"plain": ("ukf_small_kernel<2,0>", 52336), "gated": ("ukf_small_kernel<2,0,false,true>", 52336)}),
    "ukf-5": ("ukf", 24, "f64", False, 80, {"plain": ("ukf_small_kernel<5,0>", 119824), "gated": ("ukf_small_kernel<5,0,false,true>", 119824)}),
    "ukf-9": ("ukf", 64, "f64", False, 144, {"plain": ("ukf_small_kernel<9,0>", 161936), "gated": ("ukf_small_kernel<9,0,false,true>", 161936)}),
    "ekf-large-f64": ("ekf", 80, "f64", False, 192, {"plain": (F64_CHAIN, 102808), "sighted": ("large_build_GS<T,sighted> + " + F64_CHAIN, 102808),
                                                     "gated": ("large_frontend_kernel<T,gated> + " + F64_CHAIN, 107416),
                                                     "gated+sighted": ("large_frontend_kernel<T,gated> + large_build_GS<T,sighted> + " + F64_CHAIN, 107416)}),
    "ukf-large": ("ukf", 80, "f64", True, 192, {"plain": (UKF_CHAIN, 102808), "gated": ("ukf_large_frontend_kernel<gated> + " + UKF_CHAIN, 107416)}),
    "ekf-f32-64": ("ekf", 12, "f32", False, 64, {"plain": (F32_CHAIN, 99992), "sighted": ("large_build_GS<T,sighted> + " + F32_CHAIN, 99992),
                                                 "gated": ("large_frontend_kernel<T,gated> + " + F32_CHAIN, 101528),
                                                 "gated+sighted": ("large_frontend_kernel<T,gated> + large_build_GS<T,sighted> + " + F32_CHAIN, 101528)}),
}


@pytest.mark.parametrize("ctx", list(KERNEL_INFO))
def test_kernel_names(ctx, built, monkeypatch):
    """kernel_info() in every state a context can be in, against the literals above; nothing is launched"""
    from awesomeslam_amd.core import CFG_UKF_LARGE, Core, F32, F64

    for k in ("ASLAM_LARGE_GROUPS", "ASLAM_CHOL_RESIDENT", "ASLAM_RIGHT_STEP", "ASLAM_BF16_PIPE", "ASLAM_KEEP_L32", "ASLAM_BORDER"):
        monkeypatch.delenv(k, raising=False)
    kind, L, dtype, large_ukf, NP, want = KERNEL_INFO[ctx]
    large = NP > 144 or dtype == "f32"
    c = Core(kind, tg.dim_cap(L), batch=1, max_obs=8, max_wait=2048 if large else 64, dtype=F32 if dtype == "f32" else F64,
             flags=CFG_UKF_LARGE if large_ukf else 0)
    assert c.layout()[0] == NP
    got = {}
    for state in ("plain", "sighted", "gated+sighted", "gated"):
        if state not in want:
            continue
        c.set_replay_gate(GATE if "gated" in state else 0.0)
        if kind == "ekf":
            c.sighted_only("sighted" in state)
        info = c.kernel_info()
        got[state] = (info["name"], info["lds_bytes"])
    assert got == want
    off, on = got["plain"], got["gated"]
    assert on[0] != off[0] and ("gated" in on[0] or "true" in on[0])
    assert on[1] == off[1] + (6 * 8 * (NP // 2) if large else 0)  # the single-CU kernels overlay sH
    assert on[1] <= 160 * 1024
    c.close()


# ---- 6. tune.sweep(gates=) ----------------------------------------------------------------------------------------------------------------------
def test_sweep_with_gates(built):
    from awesomeslam_amd import tune

    kind, tr, cap, params = gated_ref.case_inputs("ekf-12")
    plain = tune.sweep("ekf", tr, [params, params], cap)
    out = tune.sweep("ekf", tr, [params, params], cap, gates=[0, GATE])
    assert "gate" not in plain[0] and "rejected" not in plain[0]
    assert {k: v for k, v in out[0].items() if k not in ("gate", "rejected")} == plain[0] and out[0]["gate"] == 0.0 and out[0]["rejected"] == 0
    f, _, _, _ = gated_ref.run_case("ekf-12")
    assert out[1]["gate"] == GATE and out[1]["rejected"] == f.rejected and out[1]["N"] == f.N
    assert out[1]["log_likelihood"] != plain[1]["log_likelihood"]
    with pytest.raises(ValueError):
        tune.sweep("ekf", tr, [params], cap, gates=[0, GATE])
