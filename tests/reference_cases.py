"""The cases on which the oracles and the kernels are pinned to the reference's own nodes (oracle/_ref, oracle/ref_oracle.py).

Shared by tests/golden/make_reference_golden.py (records tests/golden/reference/*.npz from the reference), by
tests/test_reference_parity.py (CPU) and by tests/test_gpu_reference.py.  A filter case is a *script*: a message-level trace
(the arrays of awesomeslam_amd.trace.Trajectory), optionally a state handed over first (orc_set), optionally the absolute
clock values at which the odom messages arrive, optionally bare slam() calls at the end.  run_script() plays a script through
anything with the CFilter interface -- CFilter, NpFilter, RefFilter."""
import numpy as np

from awesomeslam_amd import trace as tg
from oracle import scan_oracle as so

F = np.float32


# ------------------------------------------------------------------------------------------------ filter scripts
def _from_trace(kind, tr, **extra):
    sc = dict(kind=kind, cap=30, odom=tr.odom, dt=tr.dt.astype(F), obs_new=tr.obs_new.astype(np.uint8),
              n_obs=tr.n_obs.astype(np.int32), obs=tr.obs.astype(F))
    sc.update(extra)
    return sc


def _seeded(kind, L, T, **kw):
    return lambda: _from_trace(kind, tg.make_traces(L, T, B=1, **kw)[0])


def _edge_messages():
    """tests/test_gpu_ekf.py::test_edge_messages: odom before the first sensor message, empty sensor messages"""
    tr = tg.make_traces(5, 60, B=1, seed=35)
    tr.obs_new[0, :3] = 0
    tr.n_obs[0, 20:23] = 0
    return _from_trace("ekf", tr[0])


def _association_corners(kind):
    """tests/test_gpu_ekf.py::test_association_ties_collisions_and_non_finite_readings: the same state and messages"""
    def make():
        lm = np.array([[12.0, 0.0], [12.0, 0.0], [13.0, -2.0], [14.0, 3.0], [14.0, 3.0], [15.0, 1.0]])
        n = 3 + 2 * len(lm)
        X = np.concatenate([[0.0, 0.0, 0.0], lm.ravel()])
        rng = np.random.default_rng(7)
        A = rng.normal(size=(n, n)) * 0.01
        P = A @ A.T + np.diag([1e-3] * 3 + [2e-2] * (n - 3))
        rb = lambda p: (F(np.hypot(*p)), F(np.arctan2(p[1], p[0])))
        Z = X.copy()
        for i, p in enumerate(lm):
            Z[3 + 2 * i], Z[4 + 2 * i] = rb(p)
            Z[3 + 2 * i] += F(0.01)
        T, max_obs = 12, 16
        nan, inf = F("nan"), F("inf")
        msg = [rb(lm[0]), rb(lm[2] + [0.02, -0.01]), rb(lm[3]), rb(lm[5] + [0.05, 0.0]), rb(lm[5] + [-0.03, 0.02]),
               (inf, F(0.1)), (nan, F(0.2)), (F(5.0), nan), (F(8.0), F(0.5)), (F(8.05), F(0.5))]
        obs = np.zeros((T, max_obs, 2), F)
        obs[:, :len(msg)] = np.array(msg, F)
        obs[1::2, 3], obs[1::2, 4] = obs[1::2, 4].copy(), obs[1::2, 3].copy()
        odom = np.zeros((T, 8))
        odom[:, 2] = 1.0
        return dict(kind=kind, cap=30, odom=odom, dt=np.full(T, 0.25, F), obs_new=np.ones(T, np.uint8),
                    n_obs=np.full(T, len(msg), np.int32), obs=obs, init_n=n, init_X=X, init_Z=Z, init_P=P)
    return make


def _clock(now_init):
    """tests/test_gpu_ekf.py::test_node_clock_delta_time, continued past its 40 callbacks at rest into the drive: odom messages
    at absolute clock values.  The reference derives delta_time from `nows` itself; delta_time enters its outputs only through
    the twist (stateTransitionFunction, A(0,0), A(1,0)), so the 28 callbacks with vx != 0 and wz != 0 are what makes it visible.
    `dt` is our reading of ekf.cpp:80-81 -- min(now - last_time, 1.0) with a binary32 last_time (ekf.h:98) -- worked out in
    Python for the filters that take delta_time as an argument; `reading` gives the dt of three other readings, which
    tests/test_reference_parity.py shows NOT to reproduce what the reference recorded.  70 callbacks span 62.9 s: at the epoch
    stamp (binary32 spacing 128 s) last_time stays at 1.7e9 throughout."""
    def make():
        tr = tg.make_traces(5, 70, B=1, seed=34)[0]
        assert np.count_nonzero((tr.odom[:, 6] != 0) & (tr.odom[:, 7] != 0)) >= 20
        now, last = now_init + 0.25, F(now_init)
        dts, nows = [], []
        for t in range(tr.T):
            now += 0.37 if t % 3 else 1.9
            dts.append(F(min(now - float(last), 1.0)))
            last = F(now)
            nows.append(now)
        return _from_trace("ekf", tr, dt=np.array(dts, F), obs_new=np.ones(tr.T, np.uint8), now_init=float(now_init),
                           nows=np.array(nows))
    return make


def _single_step(kind, n):
    """one slam() on a handed-over state of dimension n (the construction of test_single_slam_on_synthetic_state)"""
    def make():
        rng = np.random.default_rng(1000 + n)
        L = (n - 3) // 2
        X = np.concatenate([[0.3, -0.2, 0.4], (12 + 3 * rng.normal(size=(L, 2))).ravel()])
        A = rng.normal(size=(n, n)) * 0.05
        P = A @ A.T + np.eye(n) * 0.01
        Z = X.copy()
        for i in range(L):
            dx, dy = X[3 + 2 * i] - X[0], X[4 + 2 * i] - X[1]
            Z[3 + 2 * i] = F(np.hypot(dx, dy) + 0.01 * rng.normal())
            Z[4 + 2 * i] = F(np.arctan2(dy, dx) - X[2] + 0.01 * rng.normal())
        return dict(kind=kind, cap=30, odom=np.zeros((0, 8)), dt=np.zeros(0, F), obs_new=np.zeros(0, np.uint8),
                    n_obs=np.zeros(0, np.int32), obs=np.zeros((0, 4, 2), F), init_n=n, init_X=X, init_Z=Z, init_P=P,
                    steps=np.array([[0.2, 0.1, 1.0]], F))
    return make


def clock_dt(sc, reading):
    """delta_time per callback of a clock script under another reading of ekf.cpp:80-81 than ours:
    "double" -- last_time kept in binary64; "unclamped" -- no min(..., 1.0); "stored_first" -- last_time stored before the
    subtraction (delta_time 0)."""
    last, out = F(sc["now_init"]), []
    prev = float(sc["now_init"])
    for now in sc["nows"]:
        now = float(now)
        out.append({"double": min(now - prev, 1.0), "unclamped": now - float(last), "stored_first": min(now - float(F(now)), 1.0)}[reading])
        last, prev = F(now), now
    return np.array(out, F)


FILTER_CASES = {
    # the cap-30 cases of tests/test_oracle_cross.py
    "ekf_cross1": _seeded("ekf", 5, 250, seed=1),
    "ekf_cross2": _seeded("ekf", 8, 250, seed=2, sensor_every=3, dt_mode="random"),
    "ekf_cross3": _seeded("ekf", 13, 200, seed=3, stages=4),
    "ekf_cross4": _seeded("ekf", 8, 200, seed=4, warm_hop=12, layout="ring", sensor_range=6.0),
    "ekf_L14_cap_refusal": _seeded("ekf", 14, 100, seed=26, stages=2),         # tests/test_gpu_ekf.py
    "ekf_edge_messages": _edge_messages,
    "ekf_association_corners": _association_corners("ekf"),
    "ekf_clock_0": _clock(0.0),
    "ekf_clock_100": _clock(100.0),
    "ekf_clock_epoch": _clock(1_700_000_000.0),
    "ukf_cross5": _seeded("ukf", 5, 200, seed=5),
    "ukf_cross6": _seeded("ukf", 8, 200, seed=6, sensor_every=2),
    "ukf_cross7": _seeded("ukf", 13, 120, seed=7),
    "ukf_L8_rewalk_randomdt": _seeded("ukf", 8, 200, seed=44, sensor_every=2, dt_mode="random"),  # tests/test_gpu_ukf.py, 300 there
    "ukf_L13_4stages": _seeded("ukf", 13, 200, seed=43, stages=4),                               # 300 there
}
for _kind in ("ekf", "ukf"):
    for _n in (3, 5, 13, 29):
        FILTER_CASES[f"{_kind}_step_n{_n}"] = _single_step(_kind, _n)


def wait_of(f):
    if hasattr(f, "wait_list"):
        return f.wait_list()
    w = f.wait                                            # NpFilter: a list of (range, bearing, count)
    return (np.array([x[0] for x in w], F), np.array([x[1] for x in w], F), np.array([x[2] for x in w], np.uint32))


def run_script(f, sc, on_step=None):
    """Play a script through a filter; returns the recorded outputs.  A filter that has odom_msg_now() (the reference, which
    reads a clock) gets the absolute times of a clock case, the others the `dt` worked out for them."""
    T = len(sc["dt"])
    if "init_X" in sc:
        f.set_state(int(sc["init_n"]), sc["init_X"], sc["init_Z"], sc["init_P"])
    clocked = "nows" in sc and hasattr(f, "odom_msg_now")
    poses, dims = np.zeros((T, 3)), np.zeros(T, np.int32)
    for t in range(T):
        if sc["obs_new"][t]:
            k = int(sc["n_obs"][t])
            f.sensor_msg(sc["obs"][t, :k, 0], sc["obs"][t, :k, 1])
        o = sc["odom"][t]
        ran = f.odom_msg_now(o, sc["nows"][t]) if clocked else f.odom_msg(*o, sc["dt"][t])
        if ran:
            poses[t] = np.asarray(f.X)[:3]
        dims[t] = f.N
        if on_step is not None:
            on_step(t, f)
    for vx, az, dt in sc.get("steps", ()):
        f.slam(F(vx), F(az), F(dt))
        if on_step is not None:
            on_step(T, f)
    wr, wb, wc = wait_of(f)
    return dict(poses=poses, dims=dims, X=np.array(f.X), Z=np.array(f.Z), P=np.array(f.P), wait_range=wr, wait_bearing=wb,
                wait_count=wc)


def script_trace(sc):
    """the trace of a script as a one-trajectory awesomeslam_amd.trace.Trace (for Core.set_trace)"""
    T = len(sc["dt"])
    return tg.Trace(sc["odom"][None], sc["dt"][None], sc["obs_new"][None], sc["n_obs"][None], sc["obs"][None],
                    np.zeros((1, 1, 2)), np.zeros((1, T, 3)))


# ------------------------------------------------------------------------------------------------ scans
def cylinder_scan(cyls, noise=0.0, seed=0):
    """exact ray casting of 1-degree beams against circles (cx, cy, r); inf = no return"""
    rng = np.random.default_rng(seed)
    th = np.deg2rad(np.arange(360.0))
    dx, dy = np.cos(th), np.sin(th)
    best = np.full(360, np.inf)
    for cx, cy, r in cyls:
        bq = dx * cx + dy * cy
        disc = bq * bq - (cx * cx + cy * cy - r * r)
        t = np.where((disc > 0) & (bq > 0), bq - np.sqrt(np.maximum(disc, 0)), np.inf)
        best = np.minimum(best, t)
    best = np.where(np.isfinite(best), best + rng.normal(0, noise, 360), np.inf)
    return best.astype(F)


def polar(r, deg):
    return r * np.cos(np.deg2rad(deg)), r * np.sin(np.deg2rad(deg))


def many_runs_scan():
    """More runs than one pass of the kernel's run loop takes (64): pairs of beams alternating between 2 m and 4 m (each
    pair a run of its own, too short to be a cluster), five cylinders pasted over them so that landmarks fall in the first,
    second and third pass.  Beam 0 is at 2 m and beam 359 at 4 m: not linked."""
    sc = np.where((np.arange(360) // 2) % 2 == 0, 2.0, 4.0).astype(F)
    cyl = cylinder_scan([polar(3.0, a) + (0.3,) for a in (30.0, 150.0, 200.0, 262.0, 335.0)])
    return np.where(np.isfinite(cyl), cyl, sc).astype(F)


def runs_of(ranges):
    """the kernel's view of a scan whose beams 0 and 359 are not linked: (ends of the runs of linked beams that stop before
    beam 359, in beam order; for each fitted cluster the index of its run)"""
    p = so.points_of(ranges)
    assert not so.dist(p[0], p[359]) < so.MIN_DIST_THRESH
    linked = [False] + [bool(so.dist(p[t - 1], p[t]) < so.MIN_DIST_THRESH) for t in range(1, 360)]
    ends = [t for t in range(1, 359) if linked[t] and not linked[t + 1]]
    _, _, _, fitted = so.scan(ranges, detail=True)
    return ends, [ends.index(e) for _, e in fitted]


def constructed_scans():
    """name -> scan: the constructed scans of tests/test_scan.py and the corners of the walk that starts the callback"""
    out = {}
    out["dead_ahead"] = cylinder_scan([(2.0, 0.0, 0.3)])                      # beams 0 and 359 linked, no return beside it
    c = polar(2.0, 353.0)
    sc = cylinder_scan([(c[0], c[1], 0.25)])
    sc[0:3] = np.inf
    out["cluster_up_to_359"] = sc
    out["small_cluster"] = cylinder_scan([(6.0 * np.cos(1.0), 6.0 * np.sin(1.0), 0.12)])
    wall = np.full(360, np.inf, F)
    wall[60:120] = (2.0 / np.cos(np.deg2rad(np.arange(60, 120) - 90.0))).astype(F)
    out["wall"] = wall
    out["empty"] = np.full(360, np.inf, F)
    out["all_nan"] = np.full(360, np.nan, F)
    out["ring_all_finite"] = np.full(360, 2.0, F)                             # the walk reaches beam 360: the assert fails
    for k in (356, 357, 358):                                                 # the first beam without a return: assert(theta < 359) at k + 1
        sc = np.full(360, 2.0, F)
        sc[k] = np.inf
        out[f"ring_open_at_{k}"] = sc
    # dead ahead, other cylinders around, and a cluster that beam 359 itself breaks: the reference joins it with first_cluster
    sc = cylinder_scan([(2.0, 0.0, 0.3)] + [polar(2.5, a) + (0.3,) for a in (60.0, 170.0, 250.0)])
    far = cylinder_scan([polar(3.5, 354.0) + (0.3,)])
    take = np.isfinite(far) & (np.arange(360) <= 358) & (np.arange(360) > 340)
    sc[take] = far[take]
    out["dead_ahead_joined"] = sc
    out["dead_ahead_with_others"] = cylinder_scan([(1.5, 0.0, 0.2)] + [polar(2.5, a) + (0.3,) for a in (45.0, 135.0, 300.0)])
    sc = np.where(np.arange(360) % 2 == 0, 6.0, 7.0).astype(F)                # finite everywhere but one beam: a long first walk
    sc[200] = np.nan                                                          # (neighbours 1 m apart: the background links nothing)
    cyl = cylinder_scan([polar(2.0, 260.0) + (0.3,), polar(2.0, 100.0) + (0.3,)])
    out["walk_to_nan_at_200"] = np.where(np.isfinite(cyl), cyl, sc).astype(F)
    return out


def noise_free_cylinders():
    """one scan per (range, radius): three cylinders of that size at that range, away from beam 0"""
    scans = []
    for d in (0.6, 1.0, 2.0, 3.5, 5.0, 7.5):
        for r in (0.12, 0.2, 0.35, 0.5):
            scans.append(cylinder_scan([polar(d, a) + (r,) for a in (37.0, 161.5, 283.0)]))
    return np.array(scans, F)


def scan_cases():
    """-> (ranges [count, 360] binary32, {group name: slice}, [names of the constructed scans])"""
    con = constructed_scans()
    groups = [("random", so.make_scans(200, seed=3)), ("constructed", np.array(list(con.values()), F)),
              ("cylinders", noise_free_cylinders()), ("many_runs", many_runs_scan()[None])]
    at, where = 0, {}
    for name, a in groups:
        where[name] = slice(at, at + len(a))
        at += len(a)
    return np.concatenate([a for _, a in groups]).astype(F), where, list(con.keys())
