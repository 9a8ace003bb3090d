"""-m gpu: snapshot and restore of whole filters (include/aslam_snapshot.h) -- a restored filter continues the run it came from BIT FOR BIT,
in the same context configuration, in another slot or batch size, in a slot that held a larger filter before, and the record migrates
between the single-CU and the large-state kernels and between the dtypes.

All traces are make_traces(L, 60, B=3, seed=s, sensor_every=2, dt_mode="random") with (L, s) in {(8, 2), (20, 3), (64, 5), (80, 62)}: at the
cut k = 21 callback 21 carries no sensor message (the stored one is re-walked), the wait-list is in use (6 / 14 / 43 / 54 entries with
counts of 7 .. 11 on the CPU oracle, which the record must equal; it grows to 375 entries later, hence max_wait = 512) and n = 9 / 17 / 47 /
57 still has to grow to 19 / 43 / 131 / 163; at k = 49 n is final and the EKF's A has left the identity.  Every comparison asserts
status == 0 on the filters it compares.  Against the oracle the bars are the ones the kernel families already have: util.REL_TOL, and
test_gpu_large.F32_TOL for binary32 products."""
import functools

import numpy as np
import pytest

from awesomeslam_amd import snapshot
from awesomeslam_amd import trace as tg
from test_gpu_large import F32_TOL
from util import REL_TOL, cov_err, rel_err

pytestmark = pytest.mark.gpu

T = 60
SEEDS = {8: 2, 20: 3, 64: 5, 80: 62}
CUTS = (21, 49)
N_AT_21 = {8: 9, 20: 17, 64: 47, 80: 57}
N_FINAL = {8: 19, 20: 43, 64: 131, 80: 163}
MAX_WAIT = 512

# name -> (filter, L, dtype, flags): the three NT instantiations of the single-CU EKF, two of the UKF, the large-state chains
CASES = {
    "ekf-L8": ("ekf", 8, "f64", 0), "ekf-L20": ("ekf", 20, "f64", 0), "ekf-L64": ("ekf", 64, "f64", 0),
    "ukf-L8": ("ukf", 8, "f64", 0), "ukf-L64": ("ukf", 64, "f64", 0),
    "ekf-L80-f64": ("ekf", 80, "f64", 0), "ekf-L80-f32": ("ekf", 80, "f32", 0), "ukf-L80-large": ("ukf", 80, "f64", 1),
}


@functools.lru_cache(maxsize=None)
def trace(L, max_obs=None):
    tr = tg.make_traces(L, T, B=3, seed=SEEDS[L], sensor_every=2, dt_mode="random")
    if max_obs is not None and max_obs != tr.max_obs:
        # the same messages in a wider array (a context takes traces of its own max_obs only)
        obs = np.zeros(tr.obs.shape[:2] + (max_obs, 2), np.float32)
        obs[:, :, :tr.max_obs] = tr.obs
        tr = tg.Trace(tr.odom, tr.dt, tr.obs_new, tr.n_obs, obs, tr.landmarks, tr.truth, tr.warmup, dict(tr.meta))
    return tr


@functools.lru_cache(maxsize=None)
def oracle(kind, L, upto=T):
    """the CPU oracle's uninterrupted replay of callbacks 0 .. upto-1: per filter (poses, dims, X, Z, P, wait-list)"""
    from oracle.c_oracle import CFilter

    out = []
    for b in range(3):
        o = CFilter(kind, tg.dim_cap(L))
        po, do = o.replay(trace(L)[b], upto)
        out.append((po, do) + o.state() + (o.wait_list(),))
    return out


def make(case, batch=3, cap=None, max_obs=None, max_wait=MAX_WAIT):
    from awesomeslam_amd.core import Core, F32, F64

    kind, L, dtype, flags = CASES[case]
    return Core(kind, cap or tg.dim_cap(L), batch=batch, max_obs=max_obs or trace(L).max_obs, max_wait=max_wait,
                dtype=F32 if dtype == "f32" else F64, flags=flags)


def run(core, t0, k, stream=None):
    """replay(t0, k) -> poses [B, k, 3], dims [B, k] (synchronised)"""
    import torch

    poses = torch.zeros((core.batch, k, 3), dtype=torch.float64, device="cuda")
    dims = torch.zeros((core.batch, k), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    core.replay(t0, k, poses.data_ptr(), dims.data_ptr(), stream)
    torch.cuda.synchronize()
    return poses.cpu().numpy(), dims.cpu().numpy()


def final(core, b):
    """everything the getters say about filter b"""
    return (np.int64(core.dim(b)),) + core.state(b) + (np.array(core.A(b)),) + core.wait_list(b, cap=MAX_WAIT) + \
        (np.uint32(core.status(b)),) + core.landmarks(b)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


_REF = {}


def reference(case, k):
    """context A: replay(0, k), replay(k, 60 - k) without a snapshot in between.  Computed once per (case, k) and never changed:
    (poses of 0 .. k-1, poses of k .. 59, dims of k .. 59, final(b) for every b, the snapshot at the cut)"""
    if (case, k) not in _REF:
        core = make(case)
        core.set_trace(trace(CASES[case][1]))
        p0, _ = run(core, 0, k)
        blob = core.snapshot()
        p1, d1 = run(core, k, T - k)
        fin = [final(core, b) for b in range(3)]
        assert all(core.status(b) == 0 for b in range(3))
        core.close()
        for a in (p0, p1, d1, blob):
            a.setflags(write=False)
        _REF[case, k] = (p0, p1, d1, fin, blob)
    return _REF[case, k]


def assert_continues(core, case, k, rows=(0, 1, 2), slots=None):
    """`core` holds records `rows` of the cut at k in `slots` and has the matching trace bound: the rest of the run equals context A's"""
    _, p1, d1, fin, _ = reference(case, k)
    slots = range(len(rows)) if slots is None else slots
    pg, dg = run(core, k, T - k)
    for r, s in zip(rows, slots):
        assert core.status(s) == 0
        assert np.array_equal(pg[s], p1[r]) and np.array_equal(dg[s], d1[r]), (case, k, r, s)
        assert same(final(core, s), fin[r]), (case, k, r, s)
    return pg


# ---- 1. resume is bitwise ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", CUTS)
@pytest.mark.parametrize("case", list(CASES))
def test_resume_is_bitwise(case, k, built):
    kind, L, dtype, _ = CASES[case]
    tr = trace(L)
    assert tr.obs_new[:, k].max() == 0 and tr.obs_new[:, k - 1].min() == 1  # callback k re-walks the message stored at k - 1
    p0, p1, d1, fin, _ = reference(case, k)
    b_ctx = make(case)
    b_ctx.set_trace(tr)
    pb0, _ = run(b_ctx, 0, k)
    blob = b_ctx.snapshot()
    assert all(b_ctx.status(b) == 0 for b in range(3))
    b_ctx.close()
    assert np.array_equal(pb0, p0)
    recs = snapshot.parse(blob)
    if k == 21:  # the cut is where the module docstring says it is
        assert [r["n"] for r in recs] == [N_AT_21[L]] * 3
        for r, o in zip(recs, oracle(kind, L, 21)):  # a wait-list in use, with counts: the oracle's, entry for entry
            wr, wb, wc = o[5]
            assert len(wc) >= 6 and wc.min() > 0
            assert np.array_equal(r["wait_rb"][:, 0], wr) and np.array_equal(r["wait_rb"][:, 1], wb) and np.array_equal(r["wait_cnt"], wc)
    else:
        assert [r["n"] for r in recs] == [N_FINAL[L]] * 3
        if kind == "ekf":
            assert [bool(r["A"][0] != 1.0 or r["A"][1] != 0.0) for r in recs] == [not (L == 8 and b == 0) for b in range(3)]

    fresh = make(case)
    fresh.restore(blob)
    fresh.set_trace(tr)
    pg = assert_continues(fresh, case, k)
    if k == 21:  # once per case: the resumed run against the oracle's uninterrupted one
        tol = F32_TOL if dtype == "f32" else REL_TOL
        for b, (po, do, Xo, Zo, Po, _) in enumerate(oracle(kind, L)):
            X, Z, P = fresh.state(b)
            errs = rel_err(np.concatenate([pb0[b], pg[b]]), po), rel_err(X, Xo), cov_err(P, Po)
            print(f"snapshot resume {case} b={b} N={fresh.dim(b)}: rel err pose/X/P = {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
            assert max(errs) < tol and np.array_equal(Z, Zo) and fresh.dim(b) == do[-1] == N_FINAL[L]
    fresh.close()


# ---- 2. the record says what the getters say ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ekf-L8", "ukf-L64", "ekf-L80-f32", "ukf-L80-large"])
def test_record_equals_getters(case, built):
    L = CASES[case][1]
    tr = trace(L)
    core = make(case)
    core.set_trace(tr)
    run(core, 0, 21)
    blob = core.snapshot()
    recs = snapshot.parse(blob)
    assert len(recs) == 3 and blob.size == core.snapshot_bytes()
    for b, r in enumerate(recs):
        X, Z, P = core.state(b)
        wr, wb, wc = core.wait_list(b, cap=MAX_WAIT)
        assert core.status(b) == 0 and r["status"] == 0 and r["flags"] == 0
        assert r["n"] == core.dim(b) == N_AT_21[L]
        assert np.array_equal(r["X"], X) and np.array_equal(r["Z"], Z) and np.array_equal(r["P"], P)
        assert np.array_equal(r["A"], np.array(core.A(b)))
        assert np.array_equal(r["wait_rb"][:, 0], wr) and np.array_equal(r["wait_rb"][:, 1], wb) and np.array_equal(r["wait_cnt"], wc)
        assert tr.obs_new[b, 20] == 1 and np.array_equal(r["sens"], tr.obs[b, 20, :tr.n_obs[b, 20]])
    # a snapshot of some filters, in another order, holds the same records
    part = snapshot.parse(core.snapshot(trajs=[2, 0]))
    assert snapshot.records_equal(part[0], recs[2]) and snapshot.records_equal(part[1], recs[0])
    core.close()


# ---- 3. fork and permute -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ekf-L8", "ukf-L8"])
def test_fork_and_permute(case, built):
    tr = trace(8)
    blob = reference(case, 21)[4]
    rows = [2, 0, 2]
    core = make(case, batch=3)
    core.restore(blob, records=rows, trajs=[0, 1, 2])
    core.set_trace(tr.select(rows))
    assert_continues(core, case, 21, rows=rows)
    core.close()
    core = make(case, batch=5)
    core.restore(blob, records=[1], trajs=[3])
    core.set_trace(tr.select([0, 0, 0, 1, 0]))
    assert [core.dim(b) for b in range(5)] == [3, 3, 3, 9, 3]
    assert_continues(core, case, 21, rows=[1], slots=[3])
    core.close()


# ---- 4. dirty slots ----------------------------------------------------------------------------------------------------------------
# (case, L of the trace that dirties the slots, L of the trace they then run): the three large-state chains at n = 163 (NP = 192: more than one
# 64-block) and the two single-CU families
DIRTY = [("ekf-L64", 64, 8), ("ukf-L64", 64, 8), ("ekf-L80-f64", 80, 80), ("ekf-L80-f32", 80, 80), ("ukf-L80-large", 80, 80)]


@pytest.mark.parametrize("case,big,small", DIRTY)
def test_dirty_slots(case, big, small, built):
    """Slots that have run the big trace to its final n receive records of a SMALLER n (cut at k = 21 in a context of this configuration)
    and continue their trace exactly as a freshly created context restored from the same blob does."""
    mo = trace(big).max_obs
    tr_small = trace(small, mo)
    src = make(case)
    src.set_trace(tr_small)
    run(src, 0, 21)
    blob = src.snapshot()
    src.close()
    n_rec = [r["n"] for r in snapshot.parse(blob)]
    assert n_rec == [N_AT_21[small]] * 3

    def cont(dirty):
        core = make(case)
        if dirty:
            core.set_trace(trace(big))
            run(core, 0, T)
            assert [core.dim(b) for b in range(3)] == [N_FINAL[big]] * 3 and N_FINAL[big] > n_rec[0]
        core.restore(blob)
        assert [core.dim(b) for b in range(3)] == n_rec
        core.set_trace(tr_small)
        pg, dg = run(core, 21, T - 21)
        out = (pg, dg, [final(core, b) for b in range(3)], core.snapshot())
        assert all(core.status(b) == 0 for b in range(3))
        core.close()
        return out

    (pf, df, ff, sf), (pd, dd, fd, sd) = cont(False), cont(True)
    assert np.array_equal(pd, pf) and np.array_equal(dd, df)
    assert all(same(a, b) for a, b in zip(fd, ff)) and sd.tobytes() == sf.tobytes()
    assert df[:, -1].tolist() == [N_FINAL[small]] * 3
    if big == small:  # (the same configuration as test 1: the continuation is context A's, too)
        assert np.array_equal(pf, reference(case, 21)[1])


@pytest.mark.parametrize("case,big,small", DIRTY)
def test_reset_equals_a_fresh_context(case, big, small, built):
    """A context that has run the big trace to its final n and is reset() replays the small trace exactly as a freshly created context does:
    reset and create leave the same state AND the same scratch (one list of the arrays that must start zero serves both, and restore).
    Where big == small the second run takes the same trace in filter order [2, 0, 1], so every slot reruns with ANOTHER filter's stale
    scratch; a rerun of the same trace would find the values it is about to write."""
    tr_small = trace(small, trace(big).max_obs)
    if big == small:
        tr_small = tr_small.select([2, 0, 1])

    def replay_small(core):
        core.set_trace(tr_small)
        pg, dg = run(core, 0, T)
        out = (pg, dg, [final(core, b) for b in range(3)], core.snapshot())
        status = [core.status(b) for b in range(3)]
        core.close()
        return out + (status,)

    pf, df, ff, sf, stf = replay_small(make(case))
    core = make(case)
    core.set_trace(trace(big))
    run(core, 0, T)
    assert [core.dim(b) for b in range(3)] == [N_FINAL[big]] * 3
    core.reset()
    assert [core.dim(b) for b in range(3)] == [3] * 3
    pr, dr, fr, sr, st_r = replay_small(core)
    assert stf == [0] * 3 and st_r == [0] * 3
    assert np.array_equal(pr, pf) and np.array_equal(dr, df)
    assert all(same(a, b) for a, b in zip(fr, ff)) and sr.tobytes() == sf.tobytes()
    assert df[:, -1].tolist() == [N_FINAL[small]] * 3


# aslam_get_layout of the eight CASES at batch 3 (max_obs of the case's trace, max_wait 512): (padded dimension, HBM bytes).  The values are
# those of the commit before the arrays were allocated from one list per view; the list must allocate what the hand-written calls did.
LAYOUT = {
    "ekf-L8": (32, 45120), "ekf-L20": (80, 176736), "ekf-L64": (144, 524928), "ukf-L8": (32, 217152), "ukf-L64": (144, 3621504),
    "ekf-L80-f64": (192, 4369164), "ekf-L80-f32": (192, 3754764), "ukf-L80-large": (192, 8089164),
}


@pytest.mark.parametrize("case", list(CASES))
def test_allocation_is_unchanged(case, built):
    core = make(case)
    got = core.layout()
    core.close()
    print(f"layout {case}: {got}")
    assert got == LAYOUT[case]


# ---- 5. migration ------------------------------------------------------------------------------------------------------------------
def readback(core, b):
    return (np.int64(core.dim(b)),) + core.state(b) + (np.array(core.A(b)),) + core.wait_list(b, cap=MAX_WAIT) + (np.uint32(core.status(b)),)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_migration_small_to_large_and_back(dtype, built):
    from awesomeslam_amd.core import Core, F32, F64

    L, k = 64, 49
    tr = trace(L)
    small = make("ekf-L64")
    small.set_trace(tr)
    run(small, 0, k)
    blob = small.snapshot()
    want = [readback(small, b) for b in range(3)]
    assert [w[0] for w in want] == [131] * 3 and small.launch_info()["launches_per_callback"] == 1
    small.close()

    large = Core("ekf", tg.dim_cap(80), batch=3, max_obs=tr.max_obs, max_wait=MAX_WAIT, dtype=F32 if dtype == "f32" else F64)
    assert large.layout()[0] % 64 == 0 and large.layout()[0] >= 164
    large.restore(blob)
    for b in range(3):
        assert same(readback(large, b), want[b]) and large.status(b) == 0
    back_blob = large.snapshot()
    assert back_blob.tobytes() == blob.tobytes()  # the record does not know which context it came from
    large.set_trace(tr)
    pg, dg = run(large, k, 5)
    info = large.launch_info()
    assert info["launches_per_callback"] > 1 and "large" in large.kernel_info()["name"], info
    tol = F32_TOL if dtype == "f32" else REL_TOL
    for b, (po, do, Xo, Zo, Po, _) in enumerate(oracle("ekf", L, k + 5)):
        X, Z, P = large.state(b)
        errs = rel_err(pg[b], po[k:]), rel_err(X, Xo), cov_err(P, Po)
        print(f"snapshot migration small -> large {dtype} b={b}: rel err pose/X/P = {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
        assert max(errs) < tol and np.array_equal(Z, Zo) and np.array_equal(dg[b], do[k:]) and large.status(b) == 0

    # the reverse direction: what the large context holds now (n = 131) into single-CU slots, in another order and batch size
    want = [readback(large, b) for b in range(3)]
    blob = large.snapshot()
    large.close()
    small = make("ekf-L64", batch=4)
    small.restore(blob, records=[1, 2, 0], trajs=[3, 0, 2])
    for r, s in ((1, 3), (2, 0), (0, 2)):
        assert same(readback(small, s), want[r])
    assert small.dim(1) == 3
    small.close()


# ---- 6. refusals leave the context unchanged ---------------------------------------------------------------------------------------
def refused(core, code, *args, **kw):
    from awesomeslam_amd.core import AslamError

    with pytest.raises(AslamError, match=f"aslam_core error {code}:"):
        core.restore(*args, **kw)


def test_refusals_leave_the_context_unchanged(built):
    import torch

    core = make("ekf-L8")  # max_landmark_count 20, max_obs 8, max_wait 512
    core.set_trace(trace(8))
    run(core, 0, 21)
    before = core.snapshot()
    recs = snapshot.parse(before)
    good = dict(recs[1], X=recs[1]["X"] + 1.0)  # a valid record that differs from what the context holds: a half-applied request would show

    def grown(n):
        P = np.eye(n)
        P[:9, :9] = recs[0]["P"]
        return dict(recs[0], n=n, X=np.resize(recs[0]["X"], n), Z=np.resize(recs[0]["Z"], n), P=P)

    long_wait = dict(recs[0], wait_rb=np.ones((MAX_WAIT + 1, 2), np.float32), wait_cnt=np.ones(MAX_WAIT + 1, np.uint32))
    long_sens = dict(recs[0], sens=np.ones((9, 2), np.float32))
    UNSUPPORTED, ARG = -3, -1
    refused(core, UNSUPPORTED, snapshot.pack([good, grown(21)], "ekf"))   # n >= max_landmark_count (21 is what the next cap would take)
    refused(core, UNSUPPORTED, snapshot.pack([good, long_wait], "ekf"))  # wait_n > max_wait
    refused(core, UNSUPPORTED, snapshot.pack([good, long_sens], "ekf"))  # sens_n > max_obs
    refused(core, ARG, snapshot.pack([good, good], "ukf"))               # the other filter kind
    ok = snapshot.pack([good, good, good], "ekf")
    refused(core, ARG, ok, records=[0, 1], trajs=[1, 1])                 # a slot twice
    refused(core, ARG, ok, records=[0, 3], trajs=[0, 1])                 # a record index >= count
    refused(core, ARG, ok, records=[0, 1], trajs=[0, 3])                 # a slot index >= batch
    bad = torch.from_numpy(ok.copy()).cuda()
    bad[3] = ord("X")
    refused(core, ARG, bad, records=[0, 1, 2])                           # a corrupted magic in a device blob
    assert core.snapshot().tobytes() == before.tobytes()
    # the UKF refuses the EKF's blob
    ukf = make("ukf-L8")
    u_before = ukf.snapshot()
    refused(ukf, ARG, before)
    assert ukf.snapshot().tobytes() == u_before.tobytes()
    ukf.close()
    # ... and the request the refusals were variations of goes through, from the host and from the device
    core.restore(ok)
    assert all(np.array_equal(core.state(b)[0], good["X"]) for b in range(3))
    core.restore(torch.from_numpy(before.copy()).cuda(), records=[0, 1, 2])
    assert core.snapshot().tobytes() == before.tobytes()
    # a capacity below the size writes nothing
    small = torch.zeros(before.size - 64, dtype=torch.uint8, device="cuda")
    from awesomeslam_amd.core import AslamError
    with pytest.raises(AslamError, match="aslam_core error -1:"):
        core.snapshot(out=small)
    assert int(small.max()) == 0
    core.close()


# ---- 7. device blobs are asynchronous ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ekf-L8", "ekf-L80-f32", "ukf-L80-large"])
def test_device_blob_on_a_side_stream(case, built):
    """replay, snapshot into a device tensor and restore from it into a second context, all enqueued on one side stream: nothing between the
    two calls synchronises the host beyond what they document (snapshot: the context's last stream; restore: its own header reads)."""
    import torch

    kind, L, _, _ = CASES[case]
    tr, k = trace(L), 21
    a, b = make(case), make(case)
    a.set_trace(tr)
    b.set_trace(tr)
    s = torch.cuda.Stream()
    cap = 64 + 64 + 3 * ((snapshot.record_bytes(tg.dim_cap(L) - 1, tr.max_obs, MAX_WAIT) + 63) // 64 * 64)  # an upper bound: no size query
    buf = torch.empty(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    a.replay(0, k, None, None, s.cuda_stream)
    blob = a.snapshot(out=buf, stream=s.cuda_stream)
    b.restore(blob, records=[0, 1, 2], stream=s.cuda_stream)
    pg = assert_continues(b, case, k)
    assert blob.numel() == reference(case, k)[4].size and blob.cpu().numpy().tobytes() == reference(case, k)[4].tobytes()
    assert pg.shape == (3, T - k, 3)
    a.close()
    b.close()


# ---- 8. the record writer's edges ---------------------------------------------------------------------------------------------------
EDGE_CAP, EDGE_OBS, EDGE_WAIT = 24, 4, 6
# slot -> (n, sens_n, wait_n): sens_n in {0, 1, max_obs}, wait_n in {0, 1, 2, 5, max_wait}; the zeroed tail behind the nine records is
# 32, 28, 40, 0, 52, 48, 16, 56 and 4 bytes long
EDGE_SHAPES = [(3, 0, 0), (5, 1, 1), (17, EDGE_OBS, EDGE_WAIT), (3, EDGE_OBS, 0), (5, 0, 5), (17, 1, 2), (3, 1, EDGE_WAIT), (5, EDGE_OBS, 2), (17, 0, 1)]


@functools.lru_cache(maxsize=None)
def edge_records():
    """nine host records of random content; the n = 5 ones are not waiting for their first callback (a join needs that)"""
    rng = np.random.default_rng(41)
    out = []
    for i, (n, s, w) in enumerate(EDGE_SHAPES):
        F = rng.standard_normal((n, n))
        P = F @ F.T / n * 0.02 + 0.01 * np.eye(n)
        out.append(dict(n=n, flags=(3, 0, 2)[i % 3], status=(0, 1, 4, 16, 31)[i % 5], A=rng.standard_normal(2), X=0.5 * rng.standard_normal(n),
                        Z=rng.standard_normal(n), P=np.tril(P) + np.tril(P, -1).T, sens=rng.standard_normal((s, 2)).astype(np.float32),
                        wait_rb=rng.standard_normal((w, 2)).astype(np.float32), wait_cnt=rng.integers(1, 2 ** 32, w, dtype=np.uint32)))
    return out


@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_record_bytes_round_trip(kind, built):
    """Records whose lists are empty, hold one entry or are full, so that the zeroed tail behind a record takes nine lengths (0 included) and the
    offset table is padded or not: what the device writes equals snapshot.pack of the same records byte for byte -- as they were restored, after
    a prune (prune_ref on the host) and after a join (everything but the appended block, which is held to join_ref's bar)."""
    import torch

    import join_ref as jr
    import prune_ref
    from awesomeslam_amd.core import Core, core_lib
    from test_gpu_join import blob_of, check

    recs = edge_records()
    host = snapshot.pack(recs, kind)
    assert snapshot.pack(snapshot.parse(host), kind).tobytes() == host.tobytes()  # the reference writes what it reads
    sizes = [int(core_lib().aslam_snapshot_record_bytes(*shape)) for shape in EDGE_SHAPES]
    assert sizes == [snapshot.record_bytes(*shape) for shape in EDGE_SHAPES]
    tails = {-b % 64 for b in sizes}
    assert len(tails) == 9 and 0 in tails and all(t % 4 == 0 for t in tails)

    core = Core(kind, EDGE_CAP, batch=9, max_obs=EDGE_OBS, max_wait=EDGE_WAIT)
    core.restore(host)
    for count in (1, 8, 9):  # 8: no table padding; 9: the table is padded to 16 entries
        assert core.snapshot(trajs=list(range(count))).tobytes() == snapshot.pack(recs[:count], kind).tobytes(), count
    # from a device blob, into other slots
    perm = [4, 8, 0, 7, 2, 6, 1, 5, 3]
    core.restore(torch.from_numpy(host).cuda(), records=perm, trajs=list(range(9)))
    torch.cuda.synchronize()
    now = [recs[p] for p in perm]
    assert core.snapshot().tobytes() == snapshot.pack(now, kind).tobytes()
    assert core.snapshot(trajs=[8, 3]).tobytes() == snapshot.pack([now[8], now[3]], kind).tobytes()

    # after a prune: landmark 0 of the n = 17 slots
    mask = np.zeros((9, core.landmark_capacity()), np.uint8)
    mask[[b for b in range(9) if now[b]["n"] == 17], 0] = 1
    core.remove_landmarks(mask)
    now = [prune_ref.prune_record(r, [0]) if r["n"] == 17 else r for r in now]
    assert core.snapshot().tobytes() == snapshot.pack(now, kind).tobytes()

    # after a join of one landmark into an n = 5 slot, identity frame, zero covariance
    b = next(b for b in range(9) if now[b]["n"] == 5 and len(now[b]["wait_cnt"]) == 5)
    old = now[b]
    XB, PB = np.array([0.3, -0.2, 0.1, 12.0, -7.0]), jr.spd(5, np.random.default_rng(5))
    assert jr.clear_of(old["X"][:3], [XB[3:5]], [jr.identity()])
    assert core.join_maps(blob_of([(XB, PB)], kind), [0], [b]).tolist() == [1]
    Xg, Zg, Pg = check(core, b, (old["X"], old["Z"], old["P"], XB, PB), None, jr.identity(), f"edge {kind}", exact=True)
    new = dict(old, n=7, X=np.r_[old["X"], Xg[5:]], Z=np.r_[old["Z"], Zg[5:]], P=np.zeros((7, 7)))
    new["P"][:5, :5], new["P"][5:, 5:] = old["P"], Pg[5:, 5:]
    now[b] = new
    assert core.snapshot().tobytes() == snapshot.pack(now, kind).tobytes()
    core.close()
