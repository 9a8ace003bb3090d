"""-m gpu: the HIP kernels against outputs recorded from the reference's own nodes (tests/golden/reference/, see
tests/test_reference_parity.py).  Fixtures only: nothing here needs the reference or oracle/_ref.

Bars: dimension per callback, Z, wait list, scan status and counts exact; poses, X and P (util.cov_err) within REL_TOL as in
test_golden of tests/test_gpu_ekf.py; scan range within 1e-5 relative and bearing within 1e-5 rad as in tests/test_scan.py."""
import os

import numpy as np
import pytest

import reference_cases as rc
from util import REL_TOL, cov_err, rel_err

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")
REPLAYS = [n for n in rc.FILTER_CASES if "_step_" not in n and "_clock_" not in n]
CLOCKS = [n for n in rc.FILTER_CASES if "_clock_" in n]


def load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("chunk", [None, 37], ids=["one-launch", "chunks-of-37"])
@pytest.mark.parametrize("name", REPLAYS)
def test_core_replay_against_reference(name, chunk, built):
    import torch
    from awesomeslam_amd.core import Core

    fx = load(name)
    kind, T = str(fx["kind"]), len(fx["dt"])
    tr = rc.script_trace(fx)
    core = Core(kind, 30, batch=1, max_obs=tr.max_obs, max_wait=512)
    if "init_X" in fx:
        core.set_state(0, int(fx["init_n"]), fx["init_X"], fx["init_Z"], fx["init_P"])
    core.set_trace(tr)
    poses, dims = np.zeros((T, 3)), np.zeros(T, np.int32)
    step = T if chunk is None else chunk
    for t0 in range(0, T, step):
        k = min(step, T - t0)
        p = torch.zeros((1, k, 3), dtype=torch.float64, device="cuda")
        d = torch.zeros((1, k), dtype=torch.int32, device="cuda")
        core.replay(t0, k, p.data_ptr(), d.data_ptr())
        torch.cuda.synchronize()
        poses[t0:t0 + k], dims[t0:t0 + k] = p.cpu().numpy()[0], d.cpu().numpy()[0]
    X, Z, P = core.state(0)
    assert np.array_equal(dims, fx["dims"]), "state dimension per callback must be bit-exact"
    assert np.array_equal(Z, fx["Z"]), "Z (association result) must be bit-exact"
    w = core.wait_list(0)
    for a, k in zip(w, ("wait_range", "wait_bearing", "wait_count")):
        assert np.array_equal(a, fx[k], equal_nan=True), k
    if kind == "ekf":  # A(0,0), A(1,0) come from double sin/cos: device libm vs glibc differ in the last ulp
        assert np.allclose(core.A(0), fx["A"], rtol=1e-13, atol=1e-16)
    assert core.status(0) & ~1 == 0, "wait-list / message capacity exceeded or a non-positive pivot"
    if "cap_refusal" in name:
        assert core.status(0) & 1
    errs = rel_err(poses, fx["poses"]), rel_err(X, fx["X"]), cov_err(P, fx["P"])
    print(f"{name}: kernel vs reference  poses {errs[0]:.2e}  X {errs[1]:.2e}  P {errs[2]:.2e}")
    assert max(errs) < REL_TOL, errs


@pytest.mark.parametrize("name", CLOCKS)
def test_node_clock_against_reference(name, built):
    """The host node derives delta_time from absolute clock values with its binary32 last_time; the reference did so from the
    same values when the fixture was recorded."""
    from awesomeslam_amd.core import Node

    fx = load(name)
    node = Node("ekf", 30, now_init=float(fx["now_init"]))
    out = rc.run_script(NodeAsFilter(node), fx)
    assert np.array_equal(out["dims"], fx["dims"]) and np.array_equal(out["Z"], fx["Z"])
    for k in ("wait_range", "wait_bearing", "wait_count"):
        assert np.array_equal(out[k], fx[k]), k
    _, _, a00, a10 = node.state()
    assert (a00, a10) == tuple(fx["A"])        # host libm on both sides
    errs = rel_err(out["poses"], fx["poses"]), rel_err(out["X"], fx["X"]), cov_err(out["P"], fx["P"])
    print(f"{name}: node vs reference  poses {errs[0]:.2e}  X {errs[1]:.2e}  P {errs[2]:.2e}")
    assert max(errs) < REL_TOL, errs


class NodeAsFilter:
    """awesomeslam_amd.core.Node behind the names rc.run_script uses"""

    def __init__(self, node):
        self.node = node
        self.sensor_msg, self.odom_msg_now, self.wait_list = node.sensor_msg, node.odom_msg_now, node.wait_list

    N = property(lambda self: self.node.N)
    X = property(lambda self: self.node.state()[0])
    Z = property(lambda self: self.node.state()[1])
    P = property(lambda self: self.node.P())


# ------------------------------------------------------------------------------------------------ scans
def assert_scan(i, n, rg, bg, st, fx, j, worst):
    """scan i of a kernel result against scan j of the fixture"""
    k = int(fx["n"][j])
    assert st[i] == fx["status"][j] and n[i] == k, (i, j, st[i], n[i], fx["status"][j], k)
    rr, rb = fx["range"][j, :k], fx["bearing"][j, :k]
    fin = np.isfinite(rr)
    assert np.array_equal(np.isfinite(rg[i, :k]), fin) and np.array_equal(np.isfinite(bg[i, :k]), np.isfinite(rb)), (i, j)
    if fin.any():
        er = float(np.max(np.abs(rg[i, :k][fin] - rr[fin]) / rr[fin]))
        eb = float(np.max(np.abs(bg[i, :k][fin] - rb[fin])))
        assert np.isfinite(er) and np.isfinite(eb)
        worst[0], worst[1] = max(worst[0], er), max(worst[1], eb)
    return k


def test_scan_kernel_against_reference(built):
    from awesomeslam_amd.core import scan_landmarks

    fx = load("scan")
    n, rg, bg, st = scan_landmarks(fx["ranges"], max_out=32)
    worst, tot = [0.0, 0.0], 0
    for i in range(len(fx["ranges"])):
        tot += assert_scan(i, n, rg, bg, st, fx, i, worst)
    print(f"scan kernel vs reference: {len(n)} scans, {int((st == 1).sum())} asserts, {tot} landmarks, worst range {worst[0]:.2e} "
          f"relative, worst bearing {worst[1]:.2e} rad")
    assert tot > 1000 and (st == 1).sum() == 2 and worst[0] < 1e-5 and worst[1] < 1e-5


def many_runs(fx):
    """the scan whose runs need three passes of the kernel's run loop, its index in the fixture, its landmarks' run indices"""
    j = int(fx["group_many_runs"][0])
    sc = fx["ranges"][j]
    assert np.array_equal(sc, rc.many_runs_scan())
    ends, at = rc.runs_of(sc)
    assert len(ends) > 128, len(ends)
    assert any(a < 64 for a in at) and any(64 <= a < 128 for a in at) and any(a >= 128 for a in at), at
    assert len(at) == fx["n"][j] == 5
    return sc, j, len(ends), at


def test_scan_run_loop_beyond_64_runs(built):
    """scan_landmarks_kernel takes its runs 64 at a time and carries the output count from pass to pass: a scan with more
    than 128 runs and landmarks in all three passes, alone and at the edges of a batch (first, 63, 64, last of 130)."""
    from awesomeslam_amd.core import scan_landmarks

    fx = load("scan")
    sc, j, nruns, at = many_runs(fx)
    print(f"many-runs scan: {nruns} runs, landmarks at run indices {at}")
    batch = fx["ranges"][:130].copy()                      # scans of the fixture's random group
    where = (0, 63, 64, 129)
    src = list(range(130))
    for i in where:
        batch[i], src[i] = sc, j
    n, rg, bg, st = scan_landmarks(batch, max_out=32)
    worst = [0.0, 0.0]
    for i in range(130):
        assert_scan(i, n, rg, bg, st, fx, src[i], worst)
    assert worst[0] < 1e-5 and worst[1] < 1e-5, worst
    for i in where:
        assert n[i] == 5 and st[i] == 0 and np.array_equal(rg[i, :5], rg[0, :5]) and np.array_equal(bg[i, :5], bg[0, :5])


@pytest.mark.parametrize("max_out", [5, 4, 1])
def test_scan_max_out_across_passes(max_out, built):
    """max_out = 5 holds the scan's five landmarks exactly (no overflow bit); with 4 and 1 the landmarks of the later passes are
    dropped, the bit is set and the first entries are those of the full result."""
    from awesomeslam_amd.core import SCAN_OVERFLOW, scan_landmarks

    fx = load("scan")
    sc, j, _, _ = many_runs(fx)
    guard = np.full((3, 360), np.inf, np.float32)          # neighbours in the batch: their output rows must stay empty
    guard[1] = sc
    n, rg, bg, st = scan_landmarks(guard, max_out=max_out)
    k = min(max_out, 5)
    assert n[1] == k and st[1] == (0 if max_out >= 5 else SCAN_OVERFLOW)
    rr, rb = fx["range"][j, :k], fx["bearing"][j, :k]
    assert np.max(np.abs(rg[1, :k] - rr) / rr) < 1e-5 and np.max(np.abs(bg[1, :k] - rb)) < 1e-5
    full = scan_landmarks(sc[None], max_out=32)
    assert np.array_equal(rg[1, :k], full[1][0, :k]) and np.array_equal(bg[1, :k], full[2][0, :k])
    assert list(n[[0, 2]]) == [0, 0] and list(st[[0, 2]]) == [0, 0] and not rg[[0, 2]].any() and not bg[[0, 2]].any()
