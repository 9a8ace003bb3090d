"""-m gpu: the per-landmark sighting records (aslam_get_sightings), the selector on them (aslam_select_stale) and the forgetting policy
(Core.replay_forget, Node.remove_stale) in every kernel family.

The records are integers and are compared exactly with sightings_ref.SightFilter, the CPU oracle with a tap on its association walk.  The two
worlds, the policy (period 20, max_age 12) and the pinned schedule are those of test_forget_host.  The nine contexts: the single-CU EKF and
UKF at the capacities dim_cap(8), dim_cap(20), dim_cap(64) (the three tile counts the kernels are instantiated for) and the three launch
chains (EKF f64, EKF f32, large-state UKF) at dim_cap(80), which run here at n <= 39.  Against the oracle the bars are the ones the kernel
families already have: util.REL_TOL, test_gpu_large.F32_TOL for binary32 products."""
import functools

import numpy as np
import pytest

import prune_ref
import sightings_ref
from awesomeslam_amd import trace as tg
from test_forget_host import MAX_AGE, PERIOD, T, dims_after, trace
from test_gpu_large import F32_TOL
from test_gpu_snapshot import final, run, same
from util import REL_TOL, cov_err, rel_err

pytestmark = pytest.mark.gpu

NEVER = sightings_ref.NEVER
# name -> (filter, capacity in landmarks, dtype, flags, padded dimension)
CONTEXTS = {
    "ekf-c8": ("ekf", 8, "f64", 0, 32), "ekf-c20": ("ekf", 20, "f64", 0, 80), "ekf-c64": ("ekf", 64, "f64", 0, 144),
    "ukf-c8": ("ukf", 8, "f64", 0, 32), "ukf-c20": ("ukf", 20, "f64", 0, 80), "ukf-c64": ("ukf", 64, "f64", 0, 144),
    "ekf-c80-f64": ("ekf", 80, "f64", 0, 192), "ekf-c80-f32": ("ekf", 80, "f32", 0, 192), "ukf-c80-large": ("ukf", 80, "f64", 1, 192),
}
RUNS = [(c, L) for c in CONTEXTS for L in (8, 20) if CONTEXTS[c][1] >= L]  # a world runs in every context that can hold it
CUT = 80  # both worlds have stale landmarks here, and none was removed before


def make(ctx, tr, max_wait=512):
    from awesomeslam_amd.core import Core, F32, F64

    kind, cap, dtype, flags, NP = CONTEXTS[ctx]
    core = Core(kind, tg.dim_cap(cap), batch=tr.B, max_obs=tr.max_obs, max_wait=max_wait, dtype=F32 if dtype == "f32" else F64, flags=flags)
    assert core.layout()[0] == NP
    core.set_trace(tr)
    return core


def cap_of(ctx):
    """MAX_LANDMARK_COUNT of the context: the oracle it is compared with refuses growth at the same dimension"""
    return tg.dim_cap(CONTEXTS[ctx][1])


def tol(ctx):
    return F32_TOL if CONTEXTS[ctx][2] == "f32" else REL_TOL


@functools.lru_cache(maxsize=None)
def ref_pieces(kind, L, b, cap):
    """the oracle's uninterrupted run in pieces of 20: (dimension, last_seen, hits, clock, status) after each piece.  Computed once, never
    changed.  The L = 8 world promotes a ninth landmark near callback 130 (n = 21), which a context of capacity dim_cap(8) refuses: the status
    the device must then report is ASLAM_ST_GROWTH_REFUSED (1), and the record must not have gained an entry"""
    f = sightings_ref.SightFilter(kind, cap)
    out = []
    for t0 in range(0, T, PERIOD):
        prune_ref.step_from(f, trace(L)[b], t0, t0 + PERIOD)
        out.append((f.N,) + f.sightings() + (1 if f.growth_refused else 0,))
    return out


def ref_at(kind, L, b, upto, cap):
    """a fresh oracle stepped to callback `upto` (the caller may edit it)"""
    f = sightings_ref.SightFilter(kind, cap)
    prune_ref.step_from(f, trace(L)[b], 0, upto)
    return f


@functools.lru_cache(maxsize=None)
def ref_forget(kind, L, b, cap):
    f = sightings_ref.SightFilter(kind, cap)
    poses, dims, sched = sightings_ref.forget_run(f, trace(L)[b], T, PERIOD, MAX_AGE)
    assert not f.growth_refused
    return poses, dims, sched, f


def assert_sightings(core, b, want, what):
    seen, hits, clk = core.sightings(b)
    assert clk == want[2] and np.array_equal(seen, want[0]) and np.array_equal(hits, want[1]), (what, b, clk, want[2], seen, want[0], hits, want[1])


def assert_zero_tail(core, b):
    seen, hits, _ = core.sightings(b, padded=True)
    L = (core.dim(b) - 3) // 2
    assert len(seen) == core.landmark_capacity() and not seen[L:].any() and not hits[L:].any(), (b, L, seen, hits)


# ---- 1. the records, exact ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx,L", RUNS)
def test_records_are_exact(ctx, L, built):
    kind = CONTEXTS[ctx][0]
    core = make(ctx, trace(L))
    for b in range(3):
        assert_sightings(core, b, (np.zeros(0, np.uint32),) * 2 + (0,), "fresh")
    for i, t0 in enumerate(range(0, T, PERIOD)):
        run(core, t0, PERIOD)
        for b in range(3):
            n, seen, hits, clk, status = ref_pieces(kind, L, b, cap_of(ctx))[i]
            assert core.dim(b) == n and core.status(b) == status, (ctx, L, t0, b, core.dim(b), n, core.status(b), status)
            assert_sightings(core, b, (seen, hits, clk), (ctx, L, t0))
            assert_zero_tail(core, b)
    print(f"sightings {ctx} L={L}: clock {[core.sightings(b)[2] for b in range(3)]}, hits of filter 0 {core.sightings(0)[1].tolist()}")
    core.close()


# ---- 2. the selector ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx,L", [("ekf-c8", 8), ("ukf-c20", 20), ("ekf-c80-f32", 20)])
def test_select_stale(ctx, L, built):
    import torch

    kind = CONTEXTS[ctx][0]
    core = make(ctx, trace(L))
    run(core, 0, CUT)
    refs = [ref_at(kind, L, b, CUT, cap_of(ctx)) for b in range(3)]
    assert any(sightings_ref.stale(refs[b], MAX_AGE).any() for b in range(3))
    ld = (core.landmark_capacity() + 15) // 16 * 16 + 16
    for ages in ([0, MAX_AGE, NEVER], [MAX_AGE, NEVER, 0], [NEVER, 0, MAX_AGE]):
        mask = torch.full((3, ld), 7, dtype=torch.uint8, device="cuda")
        core.select_stale(ages, mask.data_ptr(), ld)
        torch.cuda.synchronize()
        got = mask.cpu().numpy()
        for b in range(3):
            exp = np.zeros(ld, np.uint8)
            w = sightings_ref.stale(refs[b], ages[b])
            exp[:w.size] = w
            assert np.array_equal(got[b], exp), (ctx, ages, b, got[b], exp)
            if ages[b] == NEVER:
                assert not got[b].any()
    # prune_stale: the counts, and the dimensions left
    want = [int(sightings_ref.stale(refs[b], MAX_AGE).sum()) for b in range(3)]
    before = [core.dim(b) for b in range(3)]
    assert core.prune_stale(MAX_AGE).tolist() == want and sum(want) > 0
    assert [core.dim(b) for b in range(3)] == [n - 2 * w for n, w in zip(before, want)]
    core.close()


def test_select_stale_refusals(built):
    import torch

    from awesomeslam_amd.core import AslamError

    core = make("ekf-c8", trace(8))
    run(core, 0, CUT)
    before = [final(core, b) + core.sightings(b) for b in range(3)]
    cap = core.landmark_capacity()
    dev = torch.ones(3 * cap + 64, dtype=torch.uint8, device="cuda")
    assert dev.data_ptr() % 16 == 0

    def refused(word, *args):
        with pytest.raises(AslamError, match=r"aslam_core error -1:.*aslam_select_stale.*" + word):
            core.select_stale(*args)

    refused("mask", 1, None, cap)
    refused("ld", 1, dev.data_ptr(), cap - 1)
    refused("aligned", 1, dev.data_ptr() + 8, cap)
    torch.cuda.synchronize()
    assert int(dev.min()) == 1  # a refused select wrote nothing
    for b in range(3):
        assert same(final(core, b) + core.sightings(b), before[b])
    core.close()


# ---- 3. a prune carries the record, a restore clears it ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx,L", [("ekf-c8", 8), ("ukf-c8", 8), ("ekf-c64", 20), ("ukf-c64", 20), ("ekf-c80-f64", 20), ("ekf-c80-f32", 20),
                                   ("ukf-c80-large", 20)])
def test_prune_carries_the_record(ctx, L, built):
    kind = CONTEXTS[ctx][0]
    core = make(ctx, trace(L))
    run(core, 0, CUT)
    refs = [ref_at(kind, L, b, CUT, cap_of(ctx)) for b in range(3)]
    nl = [(f.N - 3) // 2 for f in refs]
    assert min(nl) >= 3 and sightings_ref.stale(refs[0], MAX_AGE).any() and len(set(refs[0].last_seen.tolist())) > 1
    drops = [sorted({0, nl[0] - 1}), [], list(range(nl[2]))]  # first and last / nothing / everything
    untouched = final(core, 1) + core.sightings(1, padded=True)
    mask = np.zeros((3, core.landmark_capacity()), np.uint8)
    for b in range(3):
        mask[b, drops[b]] = 1
    dims = core.remove_landmarks(mask)
    for b in range(3):
        sightings_ref.compact(refs[b], drops[b])
        assert dims[b] == refs[b].N
        assert_sightings(core, b, refs[b].sightings(), (ctx, "after the prune"))  # survivors in order, the clock as it was
        assert_zero_tail(core, b)
    assert same(final(core, 1) + core.sightings(1, padded=True), untouched)
    # later callbacks keep counting from there
    _, dg = run(core, CUT, PERIOD)
    for b in range(3):
        _, do = prune_ref.step_from(refs[b], trace(L)[b], CUT, CUT + PERIOD)
        assert np.array_equal(dg[b], do) and core.status(b) == 0
        assert_sightings(core, b, refs[b].sightings(), (ctx, "20 callbacks on"))
        assert_zero_tail(core, b)
    core.close()


@pytest.mark.parametrize("ctx,L", [("ekf-c20", 20), ("ukf-c20", 20), ("ekf-c80-f64", 20), ("ukf-c80-large", 20)])
def test_restore_clears_the_record(ctx, L, built):
    kind = CONTEXTS[ctx][0]
    core = make(ctx, trace(L))
    run(core, 0, CUT)
    assert all(core.sightings(b)[2] > 0 and core.sightings(b)[1].any() for b in range(3))
    keep = core.sightings(2, padded=True)
    core.restore(core.snapshot([0, 1]), trajs=[1, 0])  # filters 0 and 1 change places; slot 2 is not restored
    refs = [ref_at(kind, L, b, CUT, cap_of(ctx)) for b in (1, 0)]
    for s in range(2):
        seen, hits, clk = core.sightings(s, padded=True)
        assert clk == 0 and not seen.any() and not hits.any() and core.dim(s) == refs[s].N
    assert same(core.sightings(2, padded=True), keep)
    # a run from there matches an oracle whose record was zeroed at the cut: every restored landmark had age 0
    for s in range(2):
        refs[s].clock = 0
        refs[s].last_seen[:] = 0
        refs[s].hits[:] = 0
    core.restore(core.snapshot([0, 1]), trajs=[1, 0])  # ... and back, so that every slot has its own trajectory's trace again
    run(core, CUT, PERIOD)
    for b in range(2):
        f = refs[1 - b]
        prune_ref.step_from(f, trace(L)[b], CUT, CUT + PERIOD)
        assert core.dim(b) == f.N and core.status(b) == 0
        assert_sightings(core, b, f.sightings(), (ctx, "after the restore"))
    core.close()


# ---- 4. the policy ----------------------------------------------------------------------------------------------------------------------
def forget_by_hand(core, T_, period, max_age):
    """what replay_forget is documented to be, written out: -> chunk-major poses and dims as flat arrays, the dimensions after each prune"""
    import torch

    poses, dims, after = [], [], []
    ld = (core.landmark_capacity() + 15) // 16 * 16
    mask = torch.zeros((core.batch, ld), dtype=torch.uint8, device="cuda")
    for t0 in range(0, T_, period):
        k = min(period, T_ - t0)
        p, d = run(core, t0, k)
        poses.append(p.reshape(-1))
        dims.append(d.reshape(-1))
        core.select_stale(max_age, mask.data_ptr(), ld)
        after.append(core.remove_landmarks(mask))
    return np.concatenate(poses), np.concatenate(dims), np.array(after)


def forget_by_call(core, T_, period, max_age):
    import torch

    poses = torch.zeros(core.batch * T_ * 3, dtype=torch.float64, device="cuda")
    dims = torch.zeros(core.batch * T_, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    after = core.replay_forget(0, T_, period, max_age, poses.data_ptr(), dims.data_ptr())
    torch.cuda.synchronize()
    return poses.cpu().numpy(), dims.cpu().numpy(), after


def chunk(flat, B, period, c, width):
    """chunk c of a chunk-major buffer of whole chunks: [B][period][width]"""
    return flat[B * period * width * c: B * period * width * (c + 1)].reshape(B, period, width)


@pytest.mark.parametrize("ctx,L", RUNS)
def test_policy(ctx, L, built):
    kind = CONTEXTS[ctx][0]
    a, b_ = make(ctx, trace(L)), make(ctx, trace(L))
    pa, da, after = forget_by_call(a, T, PERIOD, MAX_AGE)
    pb, db, after_b = forget_by_hand(b_, T, PERIOD, MAX_AGE)
    assert np.array_equal(pa, pb) and np.array_equal(da, db) and np.array_equal(after, after_b)
    for f in range(3):
        assert same(final(a, f) + a.sightings(f), final(b_, f) + b_.sightings(f)) and a.status(f) == 0
    assert after.shape == (T // PERIOD, 3) and np.array_equal(after, dims_after(kind, L)), (ctx, L, after.tolist())
    worst = 0.0
    for f in range(3):
        po, do, sched, ref = ref_forget(kind, L, f, cap_of(ctx))
        pg = np.concatenate([chunk(pa, 3, PERIOD, c, 3)[f] for c in range(T // PERIOD)])
        dg = np.concatenate([chunk(da, 3, PERIOD, c, 1)[f, :, 0] for c in range(T // PERIOD)])
        assert np.array_equal(dg, do), (ctx, L, f)
        X, Z, P = a.state(f)
        errs = rel_err(pg, po), rel_err(X, ref.X), cov_err(P, ref.P)
        print(f"forget vs oracle {ctx} L={L} b={f} N={a.dim(f)}: rel err pose/X/P = {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
        assert np.array_equal(Z, ref.Z) and max(errs) < tol(ctx), (ctx, L, f, errs)
        assert_sightings(a, f, ref.sightings(), (ctx, L, "end of the policy run"))
        worst = max(worst, *errs)
    print(f"forget {ctx} L={L}: dimensions after each prune {after.T.tolist()}, worst rel err {worst:.2e}")
    a.close()
    b_.close()


# the chains' and the single-CU kernels' own sizes, device against device (the oracle is finite and positive definite on these worlds too, but
# too slow to run here): L = 80 has n reach 123 and fall to 37 .. 59, across a 64-block boundary; L = 64 has n up to 83 and a wait-list <= 433
@pytest.mark.parametrize("ctx,L,seed,rng,T_,max_wait", [
    ("ekf-c80-f64", 80, 62, 18.0, 140, 1024), ("ekf-c80-f32", 80, 62, 18.0, 140, 1024), ("ukf-c80-large", 80, 62, 18.0, 140, 1024),
    ("ekf-c64", 64, 5, 16.0, 120, 512), ("ukf-c64", 64, 5, 16.0, 120, 512)])
def test_policy_at_the_kernels_own_sizes(ctx, L, seed, rng, T_, max_wait, built):
    tr = tg.make_traces(L, T_, B=3, seed=seed, sensor_every=2, dt_mode="fixed", sensor_range=rng)
    a, b_ = make(ctx, tr, max_wait), make(ctx, tr, max_wait)
    pa, da, after = forget_by_call(a, T_, PERIOD, MAX_AGE)
    pb, db, after_b = forget_by_hand(b_, T_, PERIOD, MAX_AGE)
    print(f"forget {ctx} L={L}: largest dimension {da.max()}, after each prune {after.T.tolist()}, status {[a.status(f) for f in range(3)]}")
    assert np.array_equal(pa, pb) and np.array_equal(da, db) and np.array_equal(after, after_b)
    for f in range(3):
        assert same(final(a, f) + a.sightings(f), final(b_, f) + b_.sightings(f)) and a.status(f) == 0
    last = np.array([chunk(da, 3, PERIOD, c, 1)[:, -1, 0] for c in range(T_ // PERIOD)])  # the dimensions each prune found
    assert ((last - after) > 0).sum() >= 2 and da.max() > 64 and after[-1].min() < 64  # the policy removed something, more than once
    a.close()
    b_.close()


# ---- 5. reset, set_state, grow ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx", ["ekf-c20", "ukf-c20", "ekf-c80-f64"])
def test_reset_set_state_grow(ctx, built):
    core = make(ctx, trace(8))
    run(core, 0, 40)
    seen, hits, clk = core.sightings(0)
    n = core.dim(0)
    assert n == 19 and clk > 0 and hits.any()
    other = final(core, 1) + core.sightings(1, padded=True)
    core.grow(0, n + 2, [1.0, 2.0], [3.0, 0.1])  # growth: last seen now, never sighted
    assert_sightings(core, 0, (np.append(seen, clk), np.append(hits, 0), clk), "grow")
    core.set_state(0, n + 6, X=np.arange(n + 6.0), Z=np.arange(n + 6.0), P=np.eye(n + 6))  # a higher dimension: growth too
    assert_sightings(core, 0, (np.concatenate([seen, [clk] * 3]), np.concatenate([hits, [0] * 3]), clk), "set_state up")
    core.set_state(0, n + 6, X=np.zeros(n + 6))  # the same dimension: nothing changes
    assert_sightings(core, 0, (np.concatenate([seen, [clk] * 3]), np.concatenate([hits, [0] * 3]), clk), "set_state same")
    core.set_state(0, 9, X=np.arange(9.0), Z=np.arange(9.0), P=np.eye(9))  # a lower one: the entries beyond become zero
    assert_sightings(core, 0, (seen[:3], hits[:3], clk), "set_state down")
    assert_zero_tail(core, 0)
    assert same(final(core, 1) + core.sightings(1, padded=True), other)
    core.reset()
    for b in range(3):
        s, h, c = core.sightings(b, padded=True)
        assert c == 0 and core.dim(b) == 3 and not s.any() and not h.any()
    run(core, 0, PERIOD)  # and a reset context counts like a fresh one
    for b in range(3):
        n, seen, hits, clk, _ = ref_pieces(CONTEXTS[ctx][0], 8, b, cap_of(ctx))[0]
        assert core.dim(b) == n
        assert_sightings(core, b, (seen, hits, clk), "after reset")
    core.close()


# ---- 6. the host mirror -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_node_forgets(kind, built):
    from awesomeslam_amd.core import Node

    tr = trace(8)[0]
    po, do, sched, ref = ref_forget(kind, 8, 0, tg.dim_cap(8))
    node = Node(kind, tg.dim_cap(8))
    poses = np.zeros((T, 3))
    dims = np.zeros(T, np.int32)
    for t in range(T):
        if tr.obs_new[t]:
            c = int(tr.n_obs[t])
            node.sensor_msg(tr.obs[t, :c, 0], tr.obs[t, :c, 1])
        if node.odom_msg(tr.odom[t], tr.dt[t]):
            poses[t] = node.state()[0][:3]
        dims[t] = node.N
        if (t + 1) % PERIOD == 0:
            before, gone, after = sched[t // PERIOD]
            assert node.N == before and node.remove_stale(MAX_AGE) == gone and node.N == after, (kind, t)
    X, Z, _, _ = node.state()
    errs = rel_err(poses, po), rel_err(X, ref.X), cov_err(node.P(), ref.P)
    print(f"node forget {kind}: schedule {[(n, g) for n, g, _ in sched]}, rel err pose/X/P = {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
    assert np.array_equal(dims, do) and np.array_equal(Z, ref.Z) and max(errs) < REL_TOL
    seen, hits, clk = node.sightings()
    want = ref.sightings()
    assert clk == want[2] and np.array_equal(seen, want[0]) and np.array_equal(hits, want[1])
    assert all(np.array_equal(g, o) for g, o in zip(node.wait_list(), prune_ref.wait_arrays(ref)))
    node.close()
