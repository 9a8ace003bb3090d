"""-m gpu: joining maps (aslam_join_maps of include/aslam_snapshot.h) -- the landmarks of a snapshot record, with their covariance block, behind
the state of a running filter.

Arithmetic is held to join_ref.spread_and_bar: bar = max(32 x spread, 64 x 2^-52), spread the error of the binary64 reference against the same
function in np.longdouble on the very input -- from the two references alone.  Everything that is not arithmetic (the old part of X, Z and P,
the zero cross blocks, symmetry, untouched filters, the lists, flags, sighting records, and with identity frames the new block itself) is
compared bit for bit.  Source blobs are built on the host with awesomeslam_amd.snapshot.pack; the strict upper triangle of their P holds
junk (join_ref.synthetic), which the join must not read.

Layouts: the single-CU contexts of test_gpu_merge.LAYOUTS accept dimensions up to 141, so n_A = 125 + 17 landmarks = 159 runs on the three
large-state contexts; the two small ones cross column 128 with 125 + 8 landmarks = 141, the last dimension they accept, and column 64 with
61 + 3 = 67."""
import numpy as np
import pytest

import join_ref as jr
import merge_ref as mr
from awesomeslam_amd import mapjoin, snapshot
from awesomeslam_amd import trace as tg
from test_gpu_merge import LAYOUTS
from test_gpu_snapshot import final, make, run, same, trace
from util import cov_err, rel_err

pytestmark = pytest.mark.gpu

WORST = {"ratio": 0.0}
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = -1, -3, -4


def record(X, P, Z=None):
    n = len(X)
    return dict(n=n, flags=0, status=0, A=np.array([1.0, 0.0]), X=X, Z=np.zeros(n) if Z is None else Z, P=P, sens=np.zeros((0, 2), np.float32),
                wait_rb=np.zeros((0, 2), np.float32), wait_cnt=np.zeros(0, np.uint32))


def blob_of(sources, kind="ekf"):
    """one record per (XB, PB)"""
    return snapshot.pack([record(X, P) for X, P in sources], kind)


def mask_of(sels, ld):
    m = np.zeros((len(sels), ld), np.uint8)
    for i, s in enumerate(sels):
        m[i, :ld if s is None else len(s)] = 1 if s is None else s
    return m


def check(core, b, case, sel, frame, what, exact):
    """filter b of `core`, which held case = (XA, ZA, PA, XB, PB), after the join: the reference at the bar, the rest bit for bit"""
    XA, ZA, PA, XB, PB = case
    spread, bar, (Xr, Zr, Pr) = jr.spread_and_bar(XA, ZA, PA, XB, PB, sel, frame)
    Xg, Zg, Pg = core.state(b)
    n, nA = len(Xr), len(XA)
    assert core.dim(b) == n == len(Xg) and Pg.shape == (n, n), what
    assert np.array_equal(Pg[nA:, nA:], Pg[nA:, nA:].T), what  # (the old block is what it was: a UKF's own P is not exactly symmetric)
    assert np.array_equal(Pg, Pg.T) or not np.array_equal(PA, PA.T), what
    assert np.array_equal(Xg[:nA], XA) and np.array_equal(Zg[:nA], ZA) and np.array_equal(Pg[:nA, :nA], PA), what
    assert not Pg[:nA, nA:].any() and not np.signbit(Pg[:nA, nA:]).any() and not np.signbit(Pg[nA:, :nA]).any(), what
    if exact:
        assert np.array_equal(Xg, Xr) and np.array_equal(Pg, Pr), what
    ex, ez, ep = rel_err(Xg, Xr), rel_err(Zg, Zr), cov_err(Pg, Pr)
    ratio = max(ex, ez, ep) / bar
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"join {what} n_A={nA} m={(n - nA) // 2}: X {ex:.2e} Z {ez:.2e} P {ep:.2e} spread {spread:.2e} bar {bar:.2e} err/bar {ratio:.3f} "
          f"(worst so far {WORST['ratio']:.3f})")
    assert max(ex, ez, ep) <= bar, what
    return Xg, Zg, Pg


def untouched(core, b, X, Z, P):
    Xg, Zg, Pg = core.state(b)
    return core.dim(b) == len(X) and np.array_equal(Xg, X) and np.array_equal(Zg, Z) and np.array_equal(Pg, P)


def everything(core):
    """what the getters and a snapshot say about every filter, sighting records included"""
    out = []
    for b in range(core.batch):
        out.append(final(core, b) + core.sightings(b, padded=True)[:2] + (np.uint32(core.sightings(b)[2]),))
    return out, core.snapshot().tobytes()


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------------------
SHAPES = {0: (3, 1, None), 2: (13, 6, [1, 0, 1, 0, 1, 0]), 4: (29, 9, None)}  # slot -> (n_A, L_B, selection)


@pytest.mark.parametrize("frames", ["identity", "general"])
def test_shapes(frames, built):
    from awesomeslam_amd.core import Core

    core = Core("ekf", 48, batch=5, max_obs=8, max_wait=16)
    cases = {b: jr.synthetic(nA, LB, seed=100 + b) for b, (nA, LB, _) in SHAPES.items()}
    cases[1], cases[3] = jr.synthetic(13, 1, seed=101), jr.synthetic(47, 1, seed=103)
    for b, (XA, ZA, PA, _, _) in cases.items():
        core.set_state(b, len(XA), XA, ZA, PA)
    blob = blob_of([cases[b][3:] for b in SHAPES])
    frame = jr.identity() if frames == "identity" else jr.general_frame()
    sel = mask_of([s for _, _, s in SHAPES.values()], 9)
    joined = core.join_maps(blob, trajs=list(SHAPES), frames=None if frames == "identity" else [frame] * 3, select=sel)
    assert joined.tolist() == [1, 3, 9]
    assert [core.dim(b) for b in range(5)] == [5, 13, 19, 47, 47]
    for b, (_, _, s) in SHAPES.items():
        check(core, b, cases[b], s, frame, f"shapes {frames} slot {b}", exact=frames == "identity")
    for b in (1, 3):
        assert untouched(core, b, *cases[b][:3])
    assert all(core.status(b) == 0 for b in range(5))
    core.close()


# ---- 2. layouts -----------------------------------------------------------------------------------------------------------------------------
def layout_joins(layout):
    return [(125, 17), (145, 3)] if LAYOUTS[layout][1] > 143 else [(125, 8), (61, 3)]


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layouts(layout, built):
    from awesomeslam_amd.core import Core, F32, F64

    kind, cap, dtype, flags, _ = LAYOUTS[layout]
    for nA, m in layout_joins(layout):
        core = Core(kind, cap, batch=2, max_obs=8, max_wait=16, dtype=F32 if dtype == "f32" else F64, flags=flags)
        case = jr.synthetic(nA, m + 2, seed=nA)
        other = jr.synthetic(nA, 1, seed=nA + 1)
        core.set_state(0, nA, *case[:3])
        core.set_state(1, nA, *other[:3])
        sel = [1] * m + [0, 0]
        frame = jr.general_frame()
        assert core.join_maps(blob_of([case[3:]], "ukf"), [0], [0], [frame], mask_of([sel], m + 2)).tolist() == [m]
        check(core, 0, case, sel, frame, f"{layout} {nA}+{m}", exact=False)
        assert untouched(core, 1, *other[:3]) and core.status(0) == 0
        core.close()


# ---- 3. blob forms --------------------------------------------------------------------------------------------------------------------------
def test_blob_forms(built):
    import torch

    from awesomeslam_amd.core import Core, F32

    case = jr.synthetic(145, 9, seed=3)
    XA, ZA, PA, XB, PB = case
    src = Core("ukf", 30, batch=1, max_obs=8, max_wait=16)
    src.set_state(0, len(XB), XB, np.zeros(len(XB)), PB)
    host = src.snapshot()
    buf = torch.zeros(src.snapshot_bytes() + 64, dtype=torch.uint8, device="cuda")
    dev = src.snapshot(out=buf)
    torch.cuda.synchronize()
    assert bytes(dev.cpu().numpy()) == host.tobytes() and snapshot.blob_info(host)[0] == 1  # a UKF record
    core = Core("ekf", 170, batch=4, max_obs=8, max_wait=16, dtype=F32)
    for b in range(4):
        core.set_state(b, 145, XA, ZA, PA)
    gen = jr.general_frame()
    assert core.join_maps(host, [0], [0], [gen]).tolist() == [9]
    assert core.join_maps(dev, [0], [1], [gen]).tolist() == [9]
    assert core.join_maps((dev.data_ptr(), dev.numel()), [0, 0], [3, 2], [gen, jr.identity()]).tolist() == [9, 9]  # one record, two slots
    torch.cuda.synchronize()
    s0 = check(core, 0, case, None, gen, "host blob", exact=False)
    for b in (1, 3):
        assert same(core.state(b), s0), b
    check(core, 2, case, None, jr.identity(), "device blob, identity", exact=True)
    src.close()
    core.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_unchanged(built):
    from awesomeslam_amd.core import AslamError, Core

    core = Core("ekf", 48, batch=3, max_obs=8, max_wait=16)
    a, b = jr.synthetic(29, 10, seed=41), jr.synthetic(13, 3, seed=42)
    core.set_state(0, 29, *a[:3])
    core.set_state(1, 13, *b[:3])  # filter 2 stays fresh from reset(): init_x is set
    blob = blob_of([a[3:], b[3:]])
    before = everything(core)
    gen = jr.general_frame()

    def refused(code, word, *args, **kw):
        with pytest.raises(AslamError, match=rf"aslam_core error {code}:.*{word}"):
            core.join_maps(*args, **kw)
        now = everything(core)
        assert all(same(x, y) for x, y in zip(now[0], before[0])) and now[1] == before[1], word

    def framed(**kw):
        tx, ty, phi, cov = gen
        cov = cov.copy()
        for k, v in kw.pop("cov", {}).items():
            cov[k] = v
        return (kw.get("tx", tx), ty, phi, cov)

    refused(ERR_ARG, r"trajs\[1\].*twice", blob, [1, 1], [1, 1])
    refused(ERR_ARG, r"records\[0\].*out of range", blob, [2], [1])
    refused(ERR_ARG, r"trajs\[0\].*out of range", blob, [1], [3])
    refused(ERR_ARG, "truncated", blob[:len(blob) - 64], [1], [1])
    refused(ERR_ARG, r"ld .*entry 0", blob, [0], [1], select=np.ones((1, 9), np.uint8))
    refused(ERR_ARG, r"frames\[1\]\.tx", blob, [1, 1], [0, 1], frames=[gen, framed(tx=float("nan"))])
    refused(ERR_ARG, r"frames\[0\]\.cov.*symmetric", blob, [1], [1], frames=[framed(cov={(0, 1): 1e-9})])
    refused(ERR_ARG, r"frames\[0\]\.cov\[0\].*negative", blob, [1], [1], frames=[framed(cov={(0, 0): -1e-12})])
    refused(ERR_STATE, "filter 2", blob, [1, 1], [1, 2])
    refused(ERR_UNSUPPORTED, "filter 0", blob, [1, 0], [1, 0])  # 29 + 20 = 49 >= 48, beside a valid entry
    assert all(core.status(k) == 0 for k in range(3))
    # the request the refusals were variations of goes through; an entry that selects nothing leaves its slot alone
    assert core.join_maps(blob, [1, 0], [1, 0], select=mask_of([None, [0] * 10], 10)).tolist() == [3, 0]
    assert untouched(core, 0, *a[:3])
    check(core, 1, b, None, jr.identity(), "after the refusals", exact=True)
    core.close()


# ---- 5. what is kept ------------------------------------------------------------------------------------------------------------------------
def test_everything_else_is_kept(built):
    core = make("ekf-L8", cap=tg.dim_cap(8) + 6)
    core.enable_innovation()
    core.set_trace(trace(8))
    run(core, 0, 21)
    before = [final(core, b) for b in range(3)]
    recs = snapshot.parse(core.snapshot())
    sight = [core.sightings(b) for b in range(3)]
    params = [bytes(core.params(b)) for b in range(3)]
    innov = [core.innovation(b) for b in range(3)]
    assert len(recs[1]["wait_cnt"]) > 0 and len(recs[1]["sens"]) > 0 and recs[1]["n"] == 9
    case = (before[1][1], before[1][2], before[1][3]) + jr.synthetic(9, 3, seed=5)[3:]
    assert core.join_maps(blob_of([case[3:]]), [0], [1]).tolist() == [3]
    check(core, 1, case, None, jr.identity(), "a replayed filter", exact=True)
    after = snapshot.parse(core.snapshot())
    for k in ("flags", "status", "A", "sens", "wait_rb", "wait_cnt"):
        assert np.asarray(after[1][k]).tobytes() == np.asarray(recs[1][k]).tobytes(), k
    assert bytes(core.params(1)) == params[1]
    seen, hits, clock = core.sightings(1)
    assert clock == sight[1][2] > 0 and np.array_equal(seen[:3], sight[1][0]) and np.array_equal(hits[:3], sight[1][1])
    assert seen[3:].tolist() == [clock] * 3 and hits[3:].tolist() == [0] * 3
    assert all(np.isnan(v) for v in core.innovation(1))
    assert len(core.sighted(1)) == 6 and not core.sighted(1).any()
    for b in (0, 2):
        assert same(final(core, b), before[b]) and same(core.sightings(b), sight[b])
        assert np.array_equal(core.innovation(b), innov[b], equal_nan=True)
        assert snapshot.records_equal(after[b], recs[b])
    core.close()


# ---- 6. continuation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,k,steps", [("ekf-L8", 20, 40), ("ukf-L8", 20, 40), ("ekf-L80-f32", 49, 8)])
def test_the_joined_slot_runs_on(case, k, steps, built):
    """slot 0: joined on the device; slot 1: the same filter built on the host (the pre-join snapshot with join_ref's X, Z, P and the
    device's own new Z entries) and restored.  Both replay the same trajectory."""
    from test_gpu_snapshot import CASES

    L = CASES[case][1]
    tr = trace(L).select([0, 0])
    core = make(case, batch=2, cap=tg.dim_cap(L) + 6)
    core.set_trace(tr)
    run(core, 0, k)
    XA, ZA, PA = core.state(0)
    nA = len(XA)
    assert same(core.state(1), (XA, ZA, PA)) and (case != "ekf-L80-f32" or nA >= 145)
    pre = snapshot.parse(core.snapshot([0]))[0]
    _, _, _, XB, PB = jr.synthetic(nA, 3, seed=6)
    assert core.join_maps(blob_of([(XB, PB)]), [0], [0]).tolist() == [3]
    Xg, Zg, Pg = core.state(0)
    Xr, Zr, Pr = jr.join(XA, ZA, PA, XB, PB, None, jr.identity())
    assert np.array_equal(Xg, Xr) and np.array_equal(Pg, Pr) and np.array_equal(Zg[:nA], ZA)
    Zr[nA:] = Zg[nA:]
    pre.update(n=nA + 6, X=Xr, Z=Zr, P=Pr)
    core.restore(snapshot.pack([pre], CASES[case][0]), [0], [1])
    poses, dims = run(core, k, steps)
    assert np.array_equal(poses[0], poses[1]) and np.array_equal(dims[0], dims[1])
    assert same(final(core, 0), final(core, 1)) and core.status(0) == core.status(1) == 0
    assert core.dim(0) >= nA + 6
    core.close()


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------------------
def test_fuse_is_join_then_merge(built):
    from awesomeslam_amd.core import Core

    case = jr.fusion_case(displace=0.05)
    XA, ZA, PA, XB, PB = case
    X, Z, P = jr.join(XA, ZA, PA, XB, PB, None, jr.identity())
    assert mr.pairs_of(mr.select_ref(X, P, 9.21, 0.5)) == jr.FUSION_PAIRS  # the reference selector picks exactly the six twins
    core = Core("ekf", 48, batch=2, max_obs=8, max_wait=16)
    core.set_state(0, 15, XA, ZA, PA)
    core.set_state(1, 15, XA, ZA, PA)
    joined, merged = mapjoin.fuse(core, blob_of([(XB, PB)]), [0], [0], None, 9.21, 0.5)
    assert joined.tolist() == [8] and merged.tolist() == [6, 0] and core.dim(0) == 15 + 4
    spread, bar, (Xr, Pr) = mr.spread_and_bar(X, P, jr.FUSION_PAIRS)
    Xg, Zg, Pg = core.state(0)
    ex, ep = rel_err(Xg, Xr), cov_err(Pg, Pr)
    print(f"fuse: X {ex:.2e} P {ep:.2e} spread {spread:.2e} bar {bar:.2e} err/bar {max(ex, ep) / bar:.3f}")
    assert max(ex, ep) <= bar and np.array_equal(Pg, Pg.T)
    # A's landmarks keep their index and their Z, the two unshared ones follow with the Z the join seeded (a device sqrt / atan2)
    assert np.array_equal(Zg[:15], ZA) and rel_err(Zg[15:], Z[27:]) <= 64 * jr.EPS
    assert untouched(core, 1, XA, ZA, PA)
    core.close()


# ---- 8. the host mirror ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_node_joins_like_the_core(kind, built):
    from awesomeslam_amd.core import AslamError, Core, Node

    tr = trace(8)[0]
    node = Node(kind, tg.dim_cap(8))
    _, _, _, XB, PB = jr.synthetic(15, 3, seed=8)
    blob = blob_of([(XB, PB)])
    with pytest.raises(AslamError, match="filter 0"):
        node.join_map(blob)  # before the first callback: refused by the core
    for t in range(30):
        if tr.obs_new[t]:
            c = int(tr.n_obs[t])
            node.sensor_msg(tr.obs[t, :c, 0], tr.obs[t, :c, 1])
        node.odom_msg(tr.odom[t], tr.dt[t])
    n = node.N
    assert n == 15
    X, Z, _, _ = node.state()
    P = node.P()
    seen, hits, clock = node.sightings()
    twin = Core(kind, tg.dim_cap(8), batch=1, max_obs=8, max_wait=16)
    twin.set_state(0, n, X, Z, P)
    with pytest.raises(AslamError, match="max_landmark_count"):
        node.join_map(blob)  # 15 + 6 = 21 >= 20
    assert node.N == n and np.array_equal(node.state()[0], X)
    gen = jr.general_frame()
    assert node.join_map(blob, 0, gen, [1, 0, 1]) == 2
    assert twin.join_maps(blob, [0], [0], [gen], np.array([[1, 0, 1]])).tolist() == [2]
    Xt, Zt, Pt = twin.state(0)
    Xn, Zn, _, _ = node.state()
    assert node.N == n + 4 and np.array_equal(Xn, Xt) and np.array_equal(Zn, Zt) and np.array_equal(node.P(), Pt)
    check(twin, 0, (X, Z, P, XB, PB), [1, 0, 1], gen, f"node {kind}", exact=False)
    sn, hn, cn = node.sightings()
    assert cn == clock and np.array_equal(sn, np.concatenate([seen, [clock] * 2])) and np.array_equal(hn, np.concatenate([hits, [0] * 2]))
    node.close()
    twin.close()
