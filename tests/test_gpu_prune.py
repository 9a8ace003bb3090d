"""-m gpu: removing landmarks from running filters (aslam_remove_landmarks / aslam_select_beyond, csrc/prune.h).

A pruned filter is, BIT FOR BIT, the filter one gets by taking a snapshot, deleting the landmarks from the record on the host
(prune_ref.prune_record) and restoring it into a fresh context -- right after the call and for the rest of the run, in every kernel family.
The traces, cuts and helpers are those of test_gpu_snapshot: at k = 21 the filters hold n = 9 / 17 / 47 / 57 and still grow to 19 / 43 / 131 /
163 (minus what was removed), i.e. into rows that were occupied before the prune; at k = 49 n is final.  Against the CPU oracle the bars are
the ones the kernel families already have (util.REL_TOL)."""
import numpy as np
import pytest

import prune_ref
from awesomeslam_amd import snapshot
from awesomeslam_amd import trace as tg
from test_gpu_snapshot import CASES, CUTS, MAX_WAIT, N_AT_21, N_FINAL, T, final, make, reference, run, same, trace
from util import REL_TOL, cov_err, rel_err

pytestmark = pytest.mark.gpu


def first_and_last(n):
    """landmark 0 (column 3: the odd half of a 16-byte pair) and the last one"""
    L = (n - 3) // 2
    return sorted({0, L - 1})


def everything(n):
    return list(range((n - 3) // 2))


def mask_of(core, drops):
    m = np.zeros((core.batch, core.landmark_capacity()), np.uint8)
    for b, d in enumerate(drops):
        m[b, list(d)] = 1
    return m


def edited_restore(case, k, drops):
    """context B: a fresh context restored from the reference snapshot at k, edited on the host"""
    recs = snapshot.parse(reference(case, k)[4])
    core = make(case)
    core.restore(snapshot.pack([prune_ref.prune_record(r, d) for r, d in zip(recs, drops)], CASES[case][0]))
    core.set_trace(trace(CASES[case][1]))
    return core


def pruned_run(case, k, drops, all_ones_for=()):
    """context A: replay(0, k), remove_landmarks"""
    core = make(case)
    core.set_trace(trace(CASES[case][1]))
    p0, _ = run(core, 0, k)
    assert np.array_equal(p0, reference(case, k)[0])
    m = mask_of(core, drops)
    for b in all_ones_for:  # entries at or beyond the filter's landmark count are ignored
        m[b, :] = 1
    dims = core.remove_landmarks(m)
    return core, dims


def assert_same_to_the_end(a, b, case, k, untouched=()):
    """both contexts hold the same filters now and after replay(k, 60 - k); `untouched` filters equal the uninterrupted reference run"""
    for f in range(3):
        assert same(final(a, f), final(b, f)), (case, k, f)
    pa, da = run(a, k, T - k)
    pb, db = run(b, k, T - k)
    assert np.array_equal(pa, pb) and np.array_equal(da, db), (case, k)
    for f in range(3):
        assert same(final(a, f), final(b, f)), (case, k, f)
        assert a.status(f) == b.status(f)
    _, p1, d1, fin, _ = reference(case, k)
    for f in untouched:
        assert np.array_equal(pa[f], p1[f]) and np.array_equal(da[f], d1[f]) and same(final(a, f), fin[f]), (case, k, f)
    return pa, da


# ---- 1. prune equals edit-and-restore, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", CUTS)
@pytest.mark.parametrize("case", list(CASES))
def test_prune_equals_edit_and_restore(case, k, built):
    L = CASES[case][1]
    n = N_AT_21[L] if k == 21 else N_FINAL[L]
    drops = [first_and_last(n), [], everything(n)]
    a, dims = pruned_run(case, k, drops, all_ones_for=(2,))
    assert dims.tolist() == [n - 2 * len(drops[0]), n, 3]
    b = edited_restore(case, k, drops)
    pa, da = assert_same_to_the_end(a, b, case, k, untouched=(1,))
    print(f"prune {case} k={k}: dims after the prune {dims.tolist()}, at callback 60 {da[:, -1].tolist()}, status {[a.status(f) for f in range(3)]}")
    if k == 21:
        # the promotions that were pending at the cut still happen: the filter grows past the rows it held before the prune
        assert da[0, -1] > n and np.all(np.diff(da[0]) >= 0)
        assert da[0, -1] == N_FINAL[L] - 2 * len(drops[0])
    a.close()
    b.close()


# ---- 2. the sizes where the large chain changes shape --------------------------------------------------------------------------------
# n = 163 (80 landmarks) at k = 49.  n_new = 131 / 129 / 127 and 67 / 65 / 63: the border tails t = 3 and t = 1 behind two 64-blocks and behind
# one, and one row below a block boundary.  Dropped from the end of the state, and from the middle (from landmark 5 on: every survivor behind
# moves, the pairs straddle)
@pytest.mark.parametrize("where", ["end", "middle"])
@pytest.mark.parametrize("sizes", [(131, 129, 127), (67, 65, 63)])
@pytest.mark.parametrize("case", ["ekf-L80-f64", "ekf-L80-f32", "ukf-L80-large"])
def test_large_chain_sizes(case, sizes, where, built):
    k, n = 49, 163
    drops = []
    for n_new in sizes:
        gone = (n - n_new) // 2
        drops.append(list(range(80 - gone, 80)) if where == "end" else list(range(5, 5 + gone)))
    a, dims = pruned_run(case, k, drops)
    assert dims.tolist() == list(sizes)
    b = edited_restore(case, k, drops)
    _, da = assert_same_to_the_end(a, b, case, k)
    print(f"prune {case} {where} -> {sizes}: dims at callback 60 {da[:, -1].tolist()}, status {[a.status(f) for f in range(3)]}")
    a.close()
    b.close()


# ---- 3. against the CPU oracle, independent of the snapshot code -----------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ekf-L8", "ekf-L20", "ukf-L8"])
def test_against_the_oracle(case, built):
    from oracle.np_oracle import NpFilter

    kind, L, _, _ = CASES[case]
    k, n = 21, N_AT_21[L]
    drops = [first_and_last(n), [1], everything(n)]
    core, dims = pruned_run(case, k, drops)
    pg, dg = run(core, k, T - k)
    for b in range(3):
        f = NpFilter(kind, tg.dim_cap(L))
        prune_ref.step_from(f, trace(L)[b], 0, k)
        assert f.N == n
        prune_ref.prune_npfilter(f, drops[b])
        assert dims[b] == f.N
        po, do = prune_ref.step_from(f, trace(L)[b], k, T)
        X, Z, P = core.state(b)
        errs = rel_err(pg[b], po), rel_err(X, f.X), cov_err(P, f.P)
        print(f"prune vs oracle {case} b={b} N={core.dim(b)}: rel err pose/X/P = {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
        assert np.array_equal(dg[b], do) and core.dim(b) == f.N and np.array_equal(Z, f.Z)
        assert all(np.array_equal(g, o) for g, o in zip(core.wait_list(b, cap=MAX_WAIT), prune_ref.wait_arrays(f)))
        assert max(errs) < REL_TOL and core.status(b) == 0
    core.close()


# ---- 4. the selector ------------------------------------------------------------------------------------------------------------------
def radius_between(X, lo_frac):
    """a radius whose square lies midway between two neighbouring squared distances of X (about lo_frac of them inside), and its margin"""
    d2 = np.sort(prune_ref.squared_distance(X))
    m = max(1, min(len(d2) - 1, int(lo_frac * len(d2))))
    r = float(np.sqrt((d2[m - 1] + d2[m]) / 2))
    return r, float(np.abs(prune_ref.squared_distance(X) - r * r).min() / (r * r))


@pytest.mark.parametrize("case", ["ekf-L20", "ekf-L80-f32"])
def test_select_beyond(case, built):
    import torch

    L = CASES[case][1]

    def at_49():
        core = make(case)
        core.set_trace(trace(L))
        run(core, 0, 49)
        core.remove_landmarks(everything(N_FINAL[L]), traj=2)  # a filter at n = 3
        return core

    core, twin = at_49(), at_49()
    assert [core.dim(b) for b in range(3)] == [N_FINAL[L], N_FINAL[L], 3]
    Xs = [core.state(b)[0] for b in range(3)]
    radii = []
    for b, frac in ((0, 0.3), (1, 0.6)):
        r, margin = radius_between(Xs[b], frac)
        assert margin > 1e-9, (b, margin)  # no landmark within rounding of the range: the comparison cannot go either way
        radii.append(r)
    radii.append(0.5)
    assert len(set(radii)) == 3
    want = [prune_ref.select_beyond(Xs[b], radii[b]) for b in range(3)]
    assert 0 < want[0].sum() < L and 0 < want[1].sum() < L and want[0].sum() != want[1].sum() and want[2].size == 0
    ld = (core.landmark_capacity() + 15) // 16 * 16 + 16
    mask = torch.full((3, ld), 7, dtype=torch.uint8, device="cuda")
    core.select_beyond(radii, mask.data_ptr(), ld)
    torch.cuda.synchronize()
    got = mask.cpu().numpy()
    for b in range(3):
        exp = np.zeros(ld, np.uint8)
        exp[:want[b].size] = want[b]
        assert np.array_equal(got[b], exp), (case, b)
    assert not got[2].any()
    # prune_beyond: the counts, and what remove_landmarks with that mask leaves
    counts = core.prune_beyond(radii)
    assert counts.tolist() == [int(w.sum()) for w in want]
    dims = twin.remove_landmarks(got)
    assert dims.tolist() == [N_FINAL[L] - 2 * int(want[0].sum()), N_FINAL[L] - 2 * int(want[1].sum()), 3]
    for b in range(3):
        assert same(final(core, b), final(twin, b)), (case, b)
        assert np.array_equal(final(core, b)[1][3:].reshape(-1, 2), Xs[b][3:].reshape(-1, 2)[~want[b]])
    core.close()
    twin.close()


# ---- 5. refusals leave the context unchanged -----------------------------------------------------------------------------------------
def test_refusals_leave_the_context_unchanged(built):
    import torch

    from awesomeslam_amd.core import AslamError

    core = make("ekf-L8")
    core.set_trace(trace(8))
    run(core, 0, 21)
    before = [final(core, b) for b in range(3)]
    blob = core.snapshot()
    cap = core.landmark_capacity()
    assert cap == (tg.dim_cap(8) - 3 + 1) // 2
    host = np.ones((3, cap), np.uint8)
    dev = torch.ones(3 * cap + 64, dtype=torch.uint8, device="cuda")
    assert dev.data_ptr() % 16 == 0

    def refused(word, f, *args):
        with pytest.raises(AslamError, match=r"aslam_core error -1:.*" + word):
            f(*args)

    refused("mask", core.remove_landmarks_ptr, None, cap, False)
    refused("mask", core.remove_landmarks_ptr, None, cap, True)
    refused("ld", core.remove_landmarks_ptr, host.ctypes.data, cap - 1, False)
    refused("ld", core.remove_landmarks_ptr, dev.data_ptr(), cap - 1, True)
    refused("aligned", core.remove_landmarks_ptr, dev.data_ptr() + 8, cap, True)
    refused("max_range", core.select_beyond, [1.0, -1.0, 1.0], dev.data_ptr(), cap)
    refused("max_range", core.select_beyond, [1.0, 1.0, float("nan")], dev.data_ptr(), cap)
    refused("max_range", core.select_beyond, float("inf"), dev.data_ptr(), cap)
    refused("max_range", core.select_beyond, 0.0, dev.data_ptr(), cap)
    refused("mask", core.select_beyond, 1.0, None, cap)
    refused("ld", core.select_beyond, 1.0, dev.data_ptr(), cap - 1)
    refused("aligned", core.select_beyond, 1.0, dev.data_ptr() + 8, cap)
    torch.cuda.synchronize()
    assert int(dev.min()) == 1  # a refused select wrote nothing
    for b in range(3):
        assert same(final(core, b), before[b])
    assert core.snapshot().tobytes() == blob.tobytes()
    # ... and the request the refusals were variations of goes through, from the device
    assert core.remove_landmarks(dev[:3 * cap].view(3, cap)).tolist() == [3, 3, 3]
    core.close()


# ---- 6. the host mirror ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_node_removes_landmarks(kind, built):
    from awesomeslam_amd.core import AslamError, Node
    from oracle.np_oracle import NpFilter

    tr = trace(8)[0]
    node = Node(kind, tg.dim_cap(8))
    ref = NpFilter(kind, tg.dim_cap(8))

    def drive(t0, t1):
        for t in range(t0, t1):
            if tr.obs_new[t]:
                c = int(tr.n_obs[t])
                node.sensor_msg(tr.obs[t, :c, 0], tr.obs[t, :c, 1])
            node.odom_msg(tr.odom[t], tr.dt[t])
        prune_ref.step_from(ref, tr, t0, t1)

    drive(0, 30)
    n = node.N
    assert n == ref.N == 15
    with pytest.raises(AslamError, match="out of range"):
        node.remove_landmarks([0, 6])
    assert node.N == n and np.array_equal(node.state()[1], ref.Z)
    assert node.remove_landmarks([0, 3]) == n - 4
    prune_ref.prune_npfilter(ref, [0, 3])
    assert np.array_equal(node.state()[1], ref.Z) and rel_err(node.state()[0], ref.X) < REL_TOL
    drive(30, T)
    X, Z, _, _ = node.state()
    errs = rel_err(X, ref.X), cov_err(node.P(), ref.P)
    print(f"node prune {kind}: N {n} -> {n - 4} -> {node.N}, rel err X/P = {errs[0]:.2e} {errs[1]:.2e}")
    assert node.N == ref.N and np.array_equal(Z, ref.Z)
    assert all(np.array_equal(g, o) for g, o in zip(node.wait_list(), prune_ref.wait_arrays(ref)))
    assert max(errs) < REL_TOL
    node.close()
