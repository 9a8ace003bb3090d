"""-m gpu: the tail rule of large_syrk_bf16x3 (large_syrk_tail, ekf_large.h).  With rl = (n - 1) // 128 the last row of 128x128 tiles that holds state rows
and no more than 16 of them in it, the tiles (rl, jt), jt < rl, return at once and the idle wave of every diagonal tile (jt, jt), jt < rl, forms rows
128 rl .. n-1 x the columns of tile jt from the B operands its workgroup has staged anyway.  Same operands, same products in the same order, same epilogue
arithmetic: every number of a replay must agree BIT FOR BIT with ASLAM_SYRK_TAIL=0, the kernel with that tile row.

Everything runs fp32 `Core`s with the resident chain forced (ASLAM_CHOL_RESIDENT=1: what a batch >= 32 selects by itself), as test_gpu_large_border.py
does.  Sizes (n = 3 + 2 L):

    n = 129 (63 landmarks)    one tail row
    n = 131 (64)              three tail rows
    n = 143 (70)              15 tail rows, the largest size at which the rule applies
    n = 259 (128)             two diagonal tiles carry a tail, and tile (2, 2) is the corner that stays
    n = 1027 (512)            the benchmark's size, three filters
    n = 145 (71)              17 tail rows: no rule, the tile row runs
    n = 127 (62)              no second tile row

The replays of one size put all landmarks out at callback 0 (stages = 1), so the filters spend some 30 of the 40 callbacks at the full size; the mixed
replay (128 landmarks in four stages, nine filters out of step) visits 67, 131, 195 and 259 with filters on both sides of the rule, and filters whose
callback is dropped, inside one launch.

Bit-equality of two paths cannot say that either path RAN, so each size is also compared with the fp64 chain at the bar test_gpu_large_border.py uses for
these replays: rows the syrk left out for 30 callbacks would miss it by orders of magnitude.  What a launch was is asserted from aslam_get_launch_info and aslam_get_syrk_tail (the flag the views of the last launch carried).
Contexts are 16 rows larger than the trace needs: handing a filter over to n + 16 afterwards (aslam_set_state without arrays changes the dimension alone)
reads back the rows and columns of P's padding that the 16-row MFMA tile of the tail hangs over."""
import numpy as np
import pytest

from awesomeslam_amd import trace as tg
from test_gpu_large import F32_DRIFT_TOL
from test_gpu_large_border import resident
from util import block_rel_err, cov_err, rel_err

pytestmark = pytest.mark.gpu

T = 40
LANDMARKS = {129: 63, 131: 64, 143: 70, 259: 128, 1027: 512, 145: 71, 127: 62}
SPARE = 16  # rows of capacity beyond the trace's full size


def tail_rows(n):
    """large_syrk_tail() of ekf_large.h: state rows in the last tile row when the rule holds, else 0"""
    rl = (n - 1) // 128
    t = n - 128 * rl
    return t if rl >= 1 and t <= 16 else 0


def capacity(L):
    return max(tg.full_dim(L) + 1 + SPARE, 146)


def run(tr, L, dtype, tail, monkeypatch, half=None):
    """(poses, dims, [(X, Z, P)], [status], kernel name, launch info, [P read back at n + SPARE]) of a replay; `half`: in two launches"""
    import torch
    from awesomeslam_amd.core import Core, F32, F64

    resident(monkeypatch)
    if tail is None:
        monkeypatch.delenv("ASLAM_SYRK_TAIL", raising=False)
    else:
        monkeypatch.setenv("ASLAM_SYRK_TAIL", tail)
    B, steps = tr.B, tr.T
    core = Core("ekf", capacity(L), batch=B, max_obs=tr.max_obs, max_wait=2048, dtype=F64 if dtype == "f64" else F32)
    core.set_trace(tr)
    poses = torch.zeros((B, steps, 3), dtype=torch.float64, device="cuda")
    dims = torch.zeros((B, steps), dtype=torch.int32, device="cuda")
    if half:
        p1, d1 = poses[:, :half].contiguous(), dims[:, :half].contiguous()
        p2, d2 = poses[:, half:].contiguous(), dims[:, half:].contiguous()
        core.replay(0, half, p1.data_ptr(), d1.data_ptr())
        core.replay(half, steps - half, p2.data_ptr(), d2.data_ptr())
        torch.cuda.synchronize()
        poses, dims = torch.cat([p1, p2], dim=1), torch.cat([d1, d2], dim=1)
    else:
        core.replay(0, steps, poses.data_ptr(), dims.data_ptr())
        torch.cuda.synchronize()
    states = [core.state(b) for b in range(B)]
    status = [core.status(b) for b in range(B)]
    name, info = core.kernel_info()["name"], dict(core.launch_info(), syrk_tail=core.syrk_tail())
    wide = []
    for b in range(B):  # the dimension alone: P as it lies in memory, SPARE rows and columns of padding included
        core.set_state(b, core.dim(b) + SPARE)
        wide.append(core.state(b)[2])
    core.close()
    return poses.cpu().numpy(), dims.cpu().numpy(), states, status, name, info, wide


_replays = {}


def replay(n, dtype, tail, monkeypatch):
    """three trajectories of LANDMARKS[n] landmarks, all out at callback 0; computed once per (size, chain)"""
    key = (n, dtype, tail)
    if key not in _replays:
        L = LANDMARKS[n]
        _replays[key] = run(tg.make_traces(L, T, B=3, seed=300 + L, stages=1), L, dtype, tail, monkeypatch)
    return _replays[key]


def assert_bit_equal(new, old, what):
    (p1, d1, s1, st1, _, _, w1), (p0, d0, s0, st0, _, _, w0) = new, old
    assert np.array_equal(d1, d0) and st1 == st0 == [0] * len(st1), (what, st1, st0)
    assert np.array_equal(p1, p0), f"{what}: pose streams differ: max {np.abs(p1 - p0).max():.3e}"
    for b in range(len(s1)):
        for a, c, name in zip(s1[b] + (w1[b],), s0[b] + (w0[b],), ("X", "Z", "P", "P with its padding")):
            assert np.array_equal(a, c), f"{what}: {name} of filter {b} differs from the ASLAM_SYRK_TAIL=0 run in {int((a != c).sum())} entries: max {np.abs(a - c).max():.3e}"


def assert_chain(name, info, tail):
    """the six launches of the resident chain, and whether the launch handed the syrk the rule (aslam_get_syrk_tail: what the views of the last
    launch carried, not the knob)"""
    assert "large_chol_bf16" in name and "large_trsm_bf16" in name and "large_syrk_bf16x3" in name, name
    assert info["launches_per_callback"] == 6 and info["chol_resident"] and info["stream_groups"] == 1, info
    assert info["syrk_tail"] == tail, info


def check_against_fp64(n, r32, r64):
    """X, P and the pose stream against the fp64 chain; the rows of the last tile row also on their own (printed)"""
    p32, d32, s32, _, _, _, _ = r32
    p64, d64, s64, st64, _, _, _ = r64
    assert np.array_equal(d32, d64) and st64 == [0] * len(st64)
    r0 = 128 * ((n - 1) // 128)
    for b in range(len(s32)):
        (X, Z, P), (Xo, Zo, Po) = s32[b], s64[b]
        assert np.array_equal(Z, Zo)
        errs = rel_err(p32[b], p64[b]), rel_err(X, Xo), cov_err(P, Po)
        eb = block_rel_err(P, Po)
        print(f"syrk tail n={n} b={b}: against fp64: rel err pose/X/P = {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}  blocks pose/cross/landmark "
              f"{eb[0]:.2e} {eb[1]:.2e} {eb[2]:.2e}  rows {r0} .. {n - 1} alone {rel_err(P[r0:], Po[r0:]):.2e}")
        assert max(errs) < F32_DRIFT_TOL


def at_full_size(dims, n):
    return min(int((dims[b] == n).sum()) for b in range(dims.shape[0]))


@pytest.mark.parametrize("n", [129, 131, 143, 259, 1027])
def test_bit_equal_to_the_tile_row(n, built, monkeypatch):
    """P, X, Z and the pose stream after 40 callbacks, some 30 of them at n: the default against ASLAM_SYRK_TAIL=0, bit for bit; and against the fp64 chain."""
    assert tail_rows(n) == {129: 1, 131: 3, 143: 15, 259: 3, 1027: 3}[n]
    new, old = replay(n, "f32", None, monkeypatch), replay(n, "f32", "0", monkeypatch)
    assert_chain(new[4], new[5], True)
    assert_chain(old[4], old[5], False)
    k = at_full_size(new[1], n)
    print(f"syrk tail n={n}: {k} of {T} callbacks at the full size; sizes visited {sorted(set(int(v) for v in new[1].ravel() if v > 0))}")
    assert k >= 20 and (new[1][:, -1] == n).all()
    assert_bit_equal(new, old, f"n = {n}")
    check_against_fp64(n, new, replay(n, "f64", None, monkeypatch))


@pytest.mark.parametrize("n", [145, 127])
def test_sizes_without_a_tail_run_the_tile_row(n, built, monkeypatch):
    """17 rows in the last tile row, or no second tile row: the rule does not hold, the launch is the same six kernels, the result is unchanged bit for
    bit -- and the last tile row was computed: X and P stand against the fp64 chain at the bar of the sizes with a tail."""
    assert tail_rows(n) == 0
    new, old = replay(n, "f32", None, monkeypatch), replay(n, "f32", "0", monkeypatch)
    assert_chain(new[4], new[5], True)  # the launch carries the rule; the kernel finds that it does not hold for this n
    assert_chain(old[4], old[5], False)
    k = at_full_size(new[1], n)
    assert k >= 20 and (new[1][:, -1] == n).all()
    assert_bit_equal(new, old, f"n = {n}")
    check_against_fp64(n, new, replay(n, "f64", None, monkeypatch))


B_MIXED, T_MIXED, L_MIXED = 9, 75, 128
LAGS = (0, 5, 9, 3, 7, 1, 8, 4, 6)  # callbacks without a sensor message after each stage's start, per filter
SKIPPED_UNTIL = 36  # first sensor message of the last filter: the others are at 67 and 131 by then


def mixed_traces():
    """nine trajectories of 128 landmarks in four stages (callbacks 0, 14, 28, 42: trace.STOP_STEPS), out of step with each other"""
    tr = tg.make_traces(L_MIXED, T_MIXED, B=B_MIXED, seed=340, stages=4)
    for k in range(4):
        for b, late in enumerate(LAGS):
            tr.obs_new[b, tg.STOP_STEPS * k : tg.STOP_STEPS * k + late] = 0
    tr.obs_new[B_MIXED - 1, :SKIPPED_UNTIL] = 0  # the last filter waits for its first sensor message: its callbacks are dropped (skipped[b]) until then
    return tr


def mixed(dtype, tail, monkeypatch):
    key = ("mixed", dtype, tail)
    if key not in _replays:
        _replays[key] = run(mixed_traces(), L_MIXED, dtype, tail, monkeypatch, half=31)
    return _replays[key]


def test_one_launch_mixes_filters(built, monkeypatch):
    """Nine filters (not a multiple of 8: the second slot of the grid is partly empty) that grow 67 -> 131 -> 195 -> ... 259 out of step, in two launches:
    callbacks whose launch holds filters with a tail (131, 259), filters without (67, 195) and a filter whose callback is dropped (the last one, before
    its first sensor message: dimension 3 and a zero pose in the record) at once.  Bit for bit against ASLAM_SYRK_TAIL=0, and against the fp64 chain."""
    new, old = mixed("f32", None, monkeypatch), mixed("f32", "0", monkeypatch)
    assert_chain(new[4], new[5], True)
    assert_chain(old[4], old[5], False)
    d = new[1]
    sizes = sorted(set(int(v) for v in d.ravel() if v > 0))
    on = [v for v in sizes if tail_rows(v)]
    print(f"syrk tail, mixed launch: sizes visited {sizes}, with a tail {on}")
    # (the filters that lag most promote the last stage's landmarks a few at a time and end between 195 and 259: more sizes without a tail in the mix)
    assert on == [131, 259] and 67 in sizes and 195 in sizes and d[0, -1] == 259 and int((d[:, -1] == 259).sum()) >= 3
    both = [t for t in range(T_MIXED) if {bool(tail_rows(int(v))) for v in d[:, t] if v > 0} == {True, False}]
    dropped = (d == 3) & (new[0] == 0.0).all(axis=2)
    assert dropped[-1, :SKIPPED_UNTIL].all() and not dropped[-1, SKIPPED_UNTIL:].any()
    all_three = [t for t in both if dropped[:, t].any()]
    print(f"syrk tail, mixed launch: {len(both)} callbacks mix filters with and without a tail, {len(all_three)} of them with a dropped filter besides")
    assert both and all_three
    assert_bit_equal(new, old, "mixed launch")
    r64 = mixed("f64", None, monkeypatch)
    check_against_fp64(259, new, r64)


@pytest.mark.parametrize("n", [131, 143, 259])
def test_symmetry_padding_and_the_x_updates_entries(n, built, monkeypatch):
    """P is exactly symmetric outside the pose block (whose entries go through the two roundings of the predict: the bound of
    test_gpu_large_border.test_covariance_stays_symmetric); the SPARE rows and columns past n -- the part of P's padding under the tail's 16-row MFMA
    tile -- hold what the ASLAM_SYRK_TAIL=0 run leaves there, zeros; the entries the X update owns (pose rows and columns, diagonal) are bit-equal to
    that run's."""
    new, old = replay(n, "f32", None, monkeypatch), replay(n, "f32", "0", monkeypatch)
    for b in range(3):
        P, P0, W, W0 = new[2][b][2], old[2][b][2], new[6][b], old[6][b]
        assert P.shape == (n, n) and W.shape == (n + SPARE, n + SPARE) and np.array_equal(W[:n, :n], P)
        A = np.abs(P - P.T)
        pose = A[:3, :3].max()
        A[:3, :3] = 0.0
        pad = max(np.abs(W[n:, :]).max(), np.abs(W[:, n:]).max())
        print(f"syrk tail symmetry n={n} b={b}: max |P - P^T| outside the pose block {A.max():.1e}, inside {pose:.1e}; max |padding| {pad:.1e}")
        assert A.max() == 0.0 and pose <= 1e-18
        assert np.array_equal(W[n:, :], W0[n:, :]) and np.array_equal(W[:, n:], W0[:, n:]) and pad == 0.0
        assert np.array_equal(P[:3, :], P0[:3, :]) and np.array_equal(P[:, :3], P0[:, :3]) and np.array_equal(np.diag(P), np.diag(P0))
