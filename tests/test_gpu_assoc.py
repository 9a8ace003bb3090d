"""-m gpu: Mahalanobis-gated data association on the device (aslam_gate_observations of include/aslam_core.h).

`assoc` is compared exactly with the long-double reference (assoc_ref.gate_ref); that comparison means something only where no decision is
a coin toss, so every case first asserts FROM THE REFERENCE that each finite best m is more than 1e-6 (relative) away from the gate and each
second-best more than 1e-6 above the best.  `mdist` is compared as |m_dev - m_ld| / max(m_ld, 1) against a bar computed from the references
alone on the very input: bar = max(32 x spread, 64 x 2^-52), spread the binary64-versus-long-double difference of gate_ref in the same measure
(32, as the merge tests use: a 25-product congruence in another order, and a device sqrt / atan2 that may differ from NumPy's by a few ulp).
Every case prints err / bar.  Synthetic states are merge_ref.synthetic(N, []) written in through Core.set_state."""
import numpy as np
import pytest

import assoc_ref as ar
import merge_ref as mr
from awesomeslam_amd import trace as tg
from test_gpu_merge import LAYOUTS
from test_gpu_snapshot import final, make, run, same, trace

pytestmark = pytest.mark.gpu

GATE = ar.GATE
WORST = {"ratio": 0.0}
PAT_I, PAT_D = 12345, 777.0


@pytest.fixture(scope="module")
def cases():
    """(N, n_obs) -> (X, P, obs): computed once, never changed"""
    out = {}
    for N, n_obs in ((3, 4), (5, 1), (5, 5), (17, 5), (17, 0), (131, 9), (133, 64), (141, 16), (163, 16), (1027, 24)):
        X, P = mr.synthetic(N, [])
        out[(N, n_obs)] = (X, P, ar.observations(X, n_obs, 100 + N))
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return out


def put(core, b, X, P):
    core.set_state(b, len(X), X, np.zeros(len(X)), P)


def packed(per_filter, ldo):
    """obs [batch, ldo, 2] float32 (rows beyond a filter's count hold junk that must not be read as observations), n_obs [batch]"""
    obs = np.full((len(per_filter), ldo, 2), 3.0e4, np.float32)
    for b, o in enumerate(per_filter):
        obs[b, :len(o)] = o
    return obs, np.array([len(o) for o in per_filter], np.int32)


def check(X, P, obs, assoc, mdist, what, gate=GATE, rr=ar.R_DEFAULT, rb=ar.R_DEFAULT, need_margins=True):
    """one filter's row of outputs against the reference: decisions exactly, distances at the bar, -1 / +inf behind the observations"""
    obs = np.asarray(obs, np.float32).reshape(-1, 2)
    k = len(obs)
    a_ld, m_ld = ar.gate_ref(X, P, obs, rr, rb, gate, np.longdouble)
    if need_margins:
        g, s = ar.margins(X, P, obs, rr, rb, gate)
        assert g > 1e-6 and s > 1e-6, (what, g, s)  # the conditions of the exact comparison, from the reference, no case left out
    err, spread, bar = ar.err_and_bar(mdist[:k], X, P, obs, rr, rb)
    ratio = err / bar
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"assoc {what} n={len(X)} n_obs={k}: associated {(a_ld >= 0).sum()}/{k} err {err:.2e} spread {spread:.2e} bar {bar:.2e} "
          f"err/bar {ratio:.3f} (worst so far {WORST['ratio']:.3f})")
    assert assoc.dtype == np.int32 and mdist.dtype == np.float64
    assert np.array_equal(assoc[:k], a_ld), what
    assert (assoc[k:] == -1).all() and np.isposinf(mdist[k:]).all(), what
    assert err <= bar, what
    return a_ld


# ---- 1. shapes: filters of different dimensions and observation counts side by side ---------------------------------------------------------
SHAPES = {
    "a": ([(3, 4), (5, 1), (17, 5), (131, 9), (133, 64)], 64),  # ldo = the largest count
    "b": ([(5, 5), (133, 64), (3, 4), (17, 0), (131, 9)], 72),   # ldo beyond every count, a filter without observations
}
ASSOCIATED = {(3, 4): 0, (5, 1): 1, (5, 5): 4, (17, 5): 4, (17, 0): 0, (131, 9): 8, (133, 64): 57, (163, 16): 15, (1027, 24): 21}


@pytest.mark.parametrize("which", list(SHAPES))
def test_shapes(which, cases, built):
    from awesomeslam_amd.core import Core

    shapes, ldo = SHAPES[which]
    core = Core("ekf", 144, batch=5, max_obs=8, max_wait=16)
    for b, key in enumerate(shapes):
        put(core, b, cases[key][0], cases[key][1])
    obs, n_obs = packed([cases[key][2] for key in shapes], ldo)
    assoc, mdist = core.gate_observations(obs, n_obs, GATE)
    assert assoc.shape == mdist.shape == (5, ldo)
    for b, key in enumerate(shapes):
        X, P, o = cases[key]
        a = check(X, P, o, assoc[b], mdist[b], f"shapes {which} b={b}")
        assert (a >= 0).sum() == ASSOCIATED[key]
        if key[0] == 3:
            assert (assoc[b] == -1).all() and np.isposinf(mdist[b]).all()  # no landmark: nothing to associate with
    core.close()


# ---- 2. layouts: every kind of context keeps one binary64 P ------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layouts(layout, cases, built):
    from awesomeslam_amd.core import Core, F32, F64

    kind, cap, dtype, flags, N = LAYOUTS[layout]
    core = Core(kind, cap, batch=2, max_obs=8, max_wait=16, dtype=F32 if dtype == "f32" else F64, flags=flags)
    keys = [(N, 16), (17, 5)]
    for b, key in enumerate(keys):
        put(core, b, cases[key][0], cases[key][1])
    obs, n_obs = packed([cases[key][2] for key in keys], 16)
    assoc, mdist = core.gate_observations(obs, n_obs, [GATE, GATE])
    for b, key in enumerate(keys):
        a = check(*cases[key], assoc[b], mdist[b], f"{layout} b={b}")
        assert key not in ASSOCIATED or (a >= 0).sum() == ASSOCIATED[key]
    core.close()


def test_n1027_f32_context(cases, built):
    from awesomeslam_amd.core import Core, F32

    core = Core("ekf", 1028, batch=2, max_obs=8, max_wait=16, dtype=F32)
    keys = [(1027, 24), (133, 64)]
    for b, key in enumerate(keys):
        put(core, b, cases[key][0], cases[key][1])
    obs, n_obs = packed([cases[key][2] for key in keys], 64)
    assoc, mdist = core.gate_observations(obs, n_obs, GATE)
    for b, key in enumerate(keys):
        a = check(*cases[key], assoc[b], mdist[b], f"n1027 f32 ctx b={b}")
        assert (a >= 0).sum() == ASSOCIATED[key]
    core.close()


# ---- 3. crafted cases ------------------------------------------------------------------------------------------------------------------------
def test_crafted_cases(built):
    from awesomeslam_amd.core import Core

    crafted = ar.crafted()
    names = list(crafted)
    core = Core("ekf", 30, batch=len(names), max_obs=8, max_wait=16)
    for b, name in enumerate(names):
        put(core, b, crafted[name]["X"], crafted[name]["P"])
    obs, n_obs = packed([np.asarray(crafted[k]["obs"], np.float32) for k in names], 9)
    assoc, mdist = core.gate_observations(obs, n_obs, [crafted[k]["gate"] for k in names])
    for b, name in enumerate(names):
        c = crafted[name]
        k = len(c["obs"])
        check(c["X"], c["P"], c["obs"], assoc[b], mdist[b], f"crafted {name}", gate=c["gate"], need_margins=False)
        if c["assoc"] is None:
            assert (assoc[b, :k] >= 0).all(), name  # an infinite gate associates every observation that has a valid landmark
        else:
            assert assoc[b, :k].tolist() == c["assoc"], name
        assert np.isposinf(mdist[b, :k]).astype(int).tolist() == c["inf"], name
    core.close()


def test_params_are_the_filters_own(cases, built):
    from awesomeslam_amd.core import Core

    X, P, o = cases[(17, 5)]
    core = Core("ekf", 30, batch=2, max_obs=8, max_wait=16)
    put(core, 0, X, P)
    put(core, 1, X, P)
    obs, n_obs = packed([o, o], 5)
    a0, m0 = core.gate_observations(obs, n_obs, np.inf)
    assert np.array_equal(m0[0], m0[1])
    core.set_params(dict(r_range=1e-4, r_bearing=1e-4), traj=1)
    a1, m1 = core.gate_observations(obs, n_obs, np.inf)
    assert np.array_equal(m1[0], m0[0]) and np.array_equal(a1[0], a0[0])  # the other filter: bit for bit what it was
    assert (m1[1] > m0[1]).all()                                          # less noise in S: every distance grows
    check(X, P, o, a1[1], m1[1], "r = 1e-4", gate=np.inf, rr=1e-4, rb=1e-4)
    check(X, P, o, a1[0], m1[0], "beside it", gate=np.inf)
    core.close()


# ---- 4. a real covariance ----------------------------------------------------------------------------------------------------------------------
def test_a_real_covariance(built):
    """ekf-L20 after 49 callbacks: every filter's own predicted readings plus offsets, a whole turn on every third; the bar from that input"""
    core = make("ekf-L20")
    core.set_trace(trace(20))
    run(core, 0, 49)
    states = [core.state(b) for b in range(3)]
    per_filter = []
    for X, _, _ in states:
        L = (len(X) - 3) // 2
        assert L >= 8
        o = [(ar.predicted(X, k)[0] + 0.05 * (k % 3 - 1), ar.predicted(X, k)[1] + 0.02 * (k % 5 - 2) + 2 * np.pi * (k % 3 - 1)) for k in range(L)]
        per_filter.append(np.array(o + [(7.5, 0.3), (0.7, -2.0)], np.float32))
    ldo = max(len(o) for o in per_filter)
    obs, n_obs = packed(per_filter, ldo)
    assoc, mdist = core.gate_observations(obs, n_obs, GATE)
    for b, (X, _, P) in enumerate(states):
        a = check(X, P, per_filter[b], assoc[b], mdist[b], f"ekf-L20 k=49 b={b}")
        assert (a >= 0).sum() >= len(per_filter[b]) // 2
    core.close()


# ---- 5. the call reads and does not write -------------------------------------------------------------------------------------------------------
def test_the_call_is_read_only(built):
    import torch

    core = make("ekf-L8")
    core.enable_innovation()
    core.set_trace(trace(8))
    run(core, 0, 49)

    def everything():
        out = []
        for b in range(3):
            out += list(final(core, b)) + list(core.sightings(b)[:2]) + [np.uint32(core.sightings(b)[2]), core.sighted(b),
                                                                          np.array(core.innovation(b)).view(np.uint64)]
        return out

    before, blob = everything(), core.snapshot()
    per_filter = [np.array([ar.predicted(core.state(b)[0], k) for k in range(4)] + [(9.0, 1.0)], np.float32) for b in range(3)]
    obs, n_obs = packed(per_filter, 8)
    a_host, m_host = core.gate_observations(obs, n_obs, GATE)
    dev = torch.from_numpy(obs).cuda()
    assert dev.data_ptr() % 16 == 0
    a_dev, m_dev = core.gate_observations(dev, n_obs, GATE)
    assert np.array_equal(a_host, a_dev) and np.array_equal(m_host, m_dev)  # a device obs and a host obs: equal outputs
    assert (a_host[:, :4] == np.arange(4)).all()
    assert same(everything(), before) and core.snapshot().tobytes() == blob.tobytes()
    assert [core.status(b) for b in range(3)] == [0, 0, 0]
    core.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(cases, built):
    import torch

    from awesomeslam_amd.core import AslamError, Core

    core = Core("ekf", 30, batch=3, max_obs=8, max_wait=16)
    X, P, o = cases[(17, 5)]
    for b in range(3):
        put(core, b, X, P)
    ldo = 8
    obs, n_obs = packed([o, o, o], ldo)
    dev = torch.from_numpy(np.concatenate([obs.reshape(-1), np.zeros(4, np.float32)])).cuda()
    assoc = torch.full((3 * ldo + 4,), PAT_I, dtype=torch.int32, device="cuda")
    mdist = torch.full((3 * ldo + 2,), PAT_D, dtype=torch.float64, device="cuda")
    assert dev.data_ptr() % 16 == 0 and assoc.data_ptr() % 16 == 0 and mdist.data_ptr() % 16 == 0

    def refused(word, obs_ptr=dev.data_ptr(), ld=ldo, is_device=True, k=n_obs, g=GATE, a=assoc.data_ptr(), m=mdist.data_ptr()):
        with pytest.raises(AslamError, match=r"aslam_core error -1: aslam_gate_observations: .*" + word):
            core.gate_observations_ptr(obs_ptr, ld, is_device, k, g, a, m)

    refused("null obs", obs_ptr=None)
    refused("null obs", obs_ptr=None, is_device=False)
    refused("null n_obs", k=None)
    refused("null gate", g=None)
    refused("null assoc_dev", a=None)
    refused("ldo", ld=0)
    refused("ldo", ld=-3)
    refused(r"n_obs\[1\].*filter 1", k=[5, ldo + 1, 5])
    refused(r"n_obs\[2\].*filter 2", k=[5, 5, -1])
    for bad in (0.0, -1.0, float("nan"), float("-inf")):
        refused(r"gate\[2\].*filter 2", g=[GATE, float("inf"), bad])
    refused("obs.*aligned", obs_ptr=dev.data_ptr() + 4)
    refused("assoc_dev.*aligned", a=assoc.data_ptr() + 4)
    refused("mdist_dev.*aligned", m=mdist.data_ptr() + 8)
    torch.cuda.synchronize()
    assert (assoc == PAT_I).all() and (mdist == PAT_D).all()  # a refused call launches nothing
    # the request the refusals were variations of goes through: from the device, with an infinite gate among the gates, mdist left out
    core.gate_observations_ptr(dev.data_ptr(), ldo, True, n_obs, [GATE, float("inf"), GATE], assoc.data_ptr(), None)
    core.gate_observations_ptr(obs.ctypes.data, ldo, False, n_obs, GATE, assoc.data_ptr(), mdist.data_ptr())
    torch.cuda.synchronize()
    a, m = assoc.cpu().numpy(), mdist.cpu().numpy()
    assert (a[3 * ldo:] == PAT_I).all() and (m[3 * ldo:] == PAT_D).all()  # nothing beyond [batch][ldo]
    for b in range(3):
        check(X, P, o, a[b * ldo:(b + 1) * ldo], m[b * ldo:(b + 1) * ldo], f"after the refusals b={b}")
    core.close()


# ---- 7. the host mirror --------------------------------------------------------------------------------------------------------------------------
def yaw_msg(X, vx, wz):
    """an odometry message whose pose is the filter's own estimate"""
    return np.array([X[0], X[1], np.cos(X[2] / 2), 0.0, 0.0, np.sin(X[2] / 2), vx, wz])


def reading(X, point):
    """(range, bearing in (-pi, pi)) of a world point from the pose in X"""
    dx, dy = point[0] - X[0], point[1] - X[1]
    return np.hypot(dx, dy), float(ar.ieee_remainder(np.float64(np.arctan2(dy, dx) - X[2]), np.float64(2 * np.pi)))


def world(pose, rb):
    return np.array([pose[0] + rb[0] * np.cos(pose[2] + rb[1]), pose[1] + rb[0] * np.sin(pose[2] + rb[1])])


def around(X, P, centre, dist):
    """the reading `dist` from the world point `centre` whose distance m in the reference (r = 1e-4, long double) is the largest, over 24 directions"""
    best = None
    for deg in range(0, 360, 15):
        o = np.array([reading(X, centre + dist * np.array([np.cos(np.radians(deg)), np.sin(np.radians(deg))]))], np.float32)
        m = float(ar.gate_ref(X, P, o, 1e-4, 1e-4, GATE, np.longdouble)[1][0])
        if best is None or m > best[0]:
            best = (m, deg, o[0])
    return best


@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_node_associates_by_the_gate(kind, built):
    """trace(8), 30 callbacks with the gate off (N = 15), then r_range = r_bearing = 1e-4 and the gate at 9.21, and one sensor message.

    The reading "0.3 m from landmark 0, beyond the gate but within assoc_dist" does not exist on this state: on the circle of 0.3 m around
    landmark 0 the reference's m is 6.62 at the most (EKF; 6.02 for the UKF -- the landmark's own variance after 20 sightings at R = 0.2 is
    about 0.0135 m^2), below 9.21 in every direction.  So the message holds FOUR observations: the 0.3 m reading, with the decision the
    reference gives for it (it passes the gate and goes to landmark 0), and beside it a reading 0.45 m from landmark 0 in the direction of
    the largest m (12.6 / 12.1), which is what the case is about -- beyond the gate, within assoc_dist = 0.5, dropped and counted.  Every
    expected decision is asserted from gate_ref with its margins before the node sees the message."""
    from awesomeslam_amd.core import AslamError, Node

    tr = trace(8)[0]
    node = Node(kind, tg.dim_cap(8))
    assert node.assoc_rejected() == 0
    for t in range(30):
        if tr.obs_new[t]:
            c = int(tr.n_obs[t])
            node.sensor_msg(tr.obs[t, :c, 0], tr.obs[t, :c, 1])
        node.odom_msg(tr.odom[t], tr.dt[t])
    assert node.N == 15
    for bad in (-1.0, float("nan")):
        with pytest.raises(AslamError, match="gate"):
            node.set_assoc_gate(bad)
    node.set_params(dict(r_range=1e-4, r_bearing=1e-4))
    node.set_assoc_gate(GATE)
    X, Z, _, _ = node.state()
    P = node.P()
    lm = X[3:].reshape(-1, 2)
    assoc_dist = node.params().assoc_dist
    wr, wb, wc = node.wait_list()
    # (a) the exact predicted reading of landmark 2; (b) 0.3 m behind landmark 0 along its ray; (b') 0.45 m from landmark 0 where the
    # reference's m is largest; (c) far from every landmark and wait-list entry
    m_far, deg, o_far = around(X, P, lm[0], 0.45)
    m_03 = around(X, P, lm[0], 0.3)[0]
    obs = np.array([reading(X, lm[2]), (reading(X, lm[0])[0] + 0.3, reading(X, lm[0])[1]), o_far, (60.0, 0.25)], np.float32)
    assert np.abs(obs[:, 1]).max() < 3.14  # (the mirror's binary32 normalisation leaves them as they are)
    a_ref, m_ref = ar.gate_ref(X, P, obs, 1e-4, 1e-4, GATE, np.longdouble)
    g, s = ar.margins(X, P, obs, 1e-4, 1e-4, GATE)
    print(f"node {kind}: reference decisions {a_ref.tolist()} distances {[float(f'{v:.3g}') for v in m_ref]} gate margin {g:.2g} second-best {s:.2g}; "
          f"largest m at 0.3 m from landmark 0 {m_03:.2f}, at 0.45 m {m_far:.2f} ({deg} degrees)")
    assert m_03 < GATE < m_far
    assert a_ref.tolist() == [2, 0, -1, -1] and g > 1e-6 and s > 1e-6
    # the Euclidean verdicts, as the mirror forms them: the observation projected from the pose of the odometry message
    msg = yaw_msg(X, tr.odom[30][6], tr.odom[30][7])
    pose = X[:3]
    d_b, d_far, d_c = (np.hypot(*(lm - world(pose, o)).T) for o in obs[1:])
    assert d_b.argmin() == 0 and abs(d_b.min() - 0.3) < 1e-3
    assert d_far.argmin() == 0 and abs(d_far.min() - 0.45) < 1e-3 and d_far.min() < assoc_dist - 0.04
    assert d_c.min() > assoc_dist + 1.0
    assert all(np.hypot(*(world(pose, (r, b)) - world(pose, obs[3]))) > assoc_dist + 1.0 for r, b in zip(wr, wb))
    seen, hits, clock = node.sightings()
    node.sensor_msg(obs[:, 0].astype(np.float64), obs[:, 1].astype(np.float64))
    assert node.odom_msg(msg, tr.dt[30]) == 1
    X1, Z1, _, _ = node.state()
    wr1, wb1, wc1 = node.wait_list()
    seen1, hits1, clock1 = node.sightings()
    assert node.N == 15 and clock1 == clock + 1
    assert Z1[7] == obs[0, 0] and Z1[8] == obs[0, 1]                                   # (a) went to landmark 2,
    assert Z1[3] == obs[1, 0] and Z1[4] == obs[1, 1]                                   # (b) through the gate to landmark 0,
    assert hits1.tolist() == [h + (k in (0, 2)) for k, h in enumerate(hits)] and seen1[2] == seen1[0] == clock1
    assert np.array_equal(Z1[[5, 6] + list(range(9, 15))], Z[[5, 6] + list(range(9, 15))])  # (b') to none: the rest of Z is what it was,
    assert node.assoc_rejected() == 1                                                  # it is dropped and counted,
    assert len(wr1) == len(wr) + 1 and np.array_equal(wc1[:-1], wc) and np.array_equal(wr1[:-1], wr)  # and the wait-list gains (c) alone,
    assert wc1[-1] == 1 and wr1[-1] == obs[3, 0] and wb1[-1] == obs[3, 1]              # with count 1
    # the gate off again: the same construction of (b') associates by the Euclidean rule
    node.set_assoc_gate(0)
    X, Z, _, _ = node.state()
    lm = X[3:].reshape(-1, 2)
    ob = np.array([reading(X, lm[0] + 0.45 * np.array([np.cos(np.radians(deg)), np.sin(np.radians(deg))]))], np.float32)
    assert abs(ob[0, 1]) < 3.14
    node.sensor_msg(ob[:, 0].astype(np.float64), ob[:, 1].astype(np.float64))
    assert node.odom_msg(yaw_msg(X, tr.odom[31][6], tr.odom[31][7]), tr.dt[31]) == 1
    Z2 = node.state()[1]
    assert Z2[3] == ob[0, 0] and Z2[4] == ob[0, 1] and node.assoc_rejected() == 1
    assert node.sightings()[1][0] == hits1[0] + 1 and len(node.wait_list()[0]) == len(wr1)
    node.close()

