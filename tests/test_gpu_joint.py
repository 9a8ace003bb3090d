"""-m gpu: joint compatibility of the gated pairings on the device (aslam_joint_compat of include/aslam_core.h).

The decisions (assoc, accepted, refused) are compared exactly with the long-double reference (joint_ref.sequential); that comparison means
something only where no decision is a coin toss, so every case first asserts FROM THE REFERENCE that every attempted D2 + dd is more than 1e-6
(relative) away from its bound and every pivot (T00, d) more than 1e-9 of its C_jj entry away from 0.  The distances (D2, each finite incr) are
compared as |dev - ld| / max(ld, 1), logdet as |dev - ld| / max(|ld|, 1), against a bar computed from the references alone on the very input:
bar = max(32 x spread, 64 x 2^-52), spread the larger of two binary64-versus-long-double differences of the reference, the bordering form's and
the dense form's -- two legitimate binary64 evaluation orders; the device's is a third.  Every case prints err / bar.  Synthetic states are
merge_ref.synthetic(N, []) written in through Core.set_state; the candidates are gate_ref's at 9.21 unless a case says otherwise."""
import numpy as np
import pytest

import assoc_ref as ar
import joint_ref as jr
import merge_ref as mr
from awesomeslam_amd import trace as tg
from test_gpu_assoc import packed, put, reading, yaw_msg
from test_gpu_merge import LAYOUTS
from test_gpu_snapshot import final, make, run, same, trace

pytestmark = pytest.mark.gpu

GATE, PROB = ar.GATE, 0.99
WORST = {"ratio": 0.0}
PAT_I, PAT_D = 12345, 777.0


@pytest.fixture(scope="module")
def cases():
    """(N, n_obs) -> (X, P, obs, cand): computed once, never changed"""
    out = {}
    for N, n_obs in ((3, 4), (5, 1), (5, 5), (17, 5), (17, 0), (131, 9), (133, 64), (141, 16), (163, 16), (1027, 24)):
        X, P = mr.synthetic(N, [])
        obs = ar.observations(X, n_obs, 100 + N)
        out[(N, n_obs)] = (X, P, obs, ar.gate_ref(X, P, obs, gate=GATE, dtype=np.longdouble)[0])
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return out


def rows(per_filter, ldo, fill=777):
    """cand [batch, ldo] int32; the entries beyond a filter's count hold junk that must not be read as candidates"""
    out = np.full((len(per_filter), ldo), fill, np.int32)
    for b, c in enumerate(per_filter):
        out[b, :len(c)] = c
    return out


def check(X, P, obs, cand, got, b, what, ldo, prob=PROB, r=ar.R_DEFAULT):
    """filter b's row of the outputs of Core.joint_compat against the reference: decisions exactly, numbers at the bar, -1 / +inf behind the
    observations.  Returns the long-double result."""
    from awesomeslam_amd.core import joint_gates

    assoc, incr, D2, logdet, accepted, refused = (a[b] for a in got)
    obs = np.asarray(obs, np.float32).reshape(-1, 2)
    k = len(obs)
    tab = None if prob is None else joint_gates(prob, ldo)
    g, t = jr.margins(X, P, obs, cand, r, r, tab)
    assert g > 1e-6 and t > 1e-9, (what, g, t)  # the conditions of the exact comparison, from the reference, no case left out
    ld, res = jr.err_and_bar((D2, logdet, incr[:k]), X, P, obs, cand, r, r, tab)
    ratio = max(e / bar for e, _, bar in res.values())
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"joint {what} n={len(X)} n_obs={k}: accepted {ld.accepted} refused {ld.refused} D2 {float(ld.D2):.6g} logdet {float(ld.logdet):.6g} "
          f"margins {g:.2g} {t:.2g}; " + "; ".join(f"{n} err {e:.2e} spread {s:.2e} bar {bar:.2e}" for n, (e, s, bar) in res.items()) +
          f"; err/bar {ratio:.3f} (worst so far {WORST['ratio']:.3f})")
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64
    assert np.array_equal(assoc[:k], ld.assoc), what
    assert (accepted, refused) == (ld.accepted, ld.refused), what
    assert (assoc[k:] == -1).all() and np.isposinf(incr[k:]).all(), what
    for n, (e, _, bar) in res.items():
        assert e <= bar, (what, n)
    ld.bars = {n: bar for n, (_, _, bar) in res.items()}
    return ld


# ---- 1. shapes: filters of different dimensions and observation counts side by side ---------------------------------------------------------
SHAPES = {"a": [(3, 4), (5, 5), (17, 5), (131, 9), (133, 64)], "b": [(133, 64), (17, 0), (5, 1), (3, 4), (131, 9)]}
ACCEPTED = {(3, 4): 0, (5, 5): 4, (17, 5): 4, (131, 9): 8, (133, 64): 57, (17, 0): 0, (5, 1): 1, (141, 16): 14, (163, 16): 15, (1027, 24): 21}


@pytest.mark.parametrize("which", list(SHAPES))
def test_shapes(which, cases, built):
    from awesomeslam_amd.core import Core

    shapes, ldo = SHAPES[which], 64
    core = Core("ekf", 144, batch=5, max_obs=8, max_wait=16)
    for b, key in enumerate(shapes):
        put(core, b, cases[key][0], cases[key][1])
    obs, n_obs = packed([cases[key][2] for key in shapes], ldo)
    got = core.joint_compat(obs, n_obs, cand=rows([cases[key][3] for key in shapes], ldo), prob=PROB)
    assert got[0].shape == got[1].shape == (5, ldo) and all(a.shape == (5,) for a in got[2:])
    for b, key in enumerate(shapes):
        ld = check(*cases[key], got, b, f"shapes {which} b={b}", ldo)
        assert (ld.accepted, ld.refused) == (ACCEPTED[key], 0)
        if ld.accepted == 0:
            assert got[2][b] == 0.0 and got[3][b] == 0.0  # an empty hypothesis
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
    got = core.joint_compat(obs, n_obs, cand=rows([cases[key][3] for key in keys], 16), prob=PROB)
    for b, key in enumerate(keys):
        assert check(*cases[key], got, b, f"{layout} b={b}", 16).accepted == ACCEPTED[key]
    core.close()


def test_n1027_f32_context(cases, built):
    from awesomeslam_amd.core import Core, F32

    core = Core("ekf", 1028, batch=2, max_obs=8, max_wait=16, dtype=F32)
    keys = [(1027, 24), (133, 64)]
    for b, key in enumerate(keys):
        put(core, b, cases[key][0], cases[key][1])
    obs, n_obs = packed([cases[key][2] for key in keys], 64)
    got = core.joint_compat(obs, n_obs, cand=rows([cases[key][3] for key in keys], 64), prob=PROB)
    for b, key in enumerate(keys):
        assert check(*cases[key], got, b, f"n1027 f32 ctx b={b}", 64).accepted == ACCEPTED[key]
    core.close()


# ---- 4, 5. crafted cases, one filter each in one batch; the reordered message among them -------------------------------------------------------
def test_crafted_cases(built):
    from awesomeslam_amd.core import Core

    crafted = jr.crafted()
    for prob in (PROB, None):  # (one table serves a batch: the evaluate-mode cases are a call of their own)
        names = [k for k in crafted if crafted[k]["prob"] == prob]
        core = Core("ekf", 30, batch=len(names), max_obs=8, max_wait=16)
        for b, name in enumerate(names):
            put(core, b, crafted[name]["X"], crafted[name]["P"])
            core.set_params(dict(r_range=crafted[name]["r"], r_bearing=crafted[name]["r"]), traj=b)
        ldo = 6
        obs, n_obs = packed([np.asarray(crafted[k]["obs"], np.float32).reshape(-1, 2) for k in names], ldo)
        got = core.joint_compat(obs, n_obs, cand=rows([crafted[k]["cand"] for k in names], ldo), prob=prob)
        for b, name in enumerate(names):
            c = crafted[name]
            k = len(c["obs"])
            ld = check(c["X"], c["P"], c["obs"], c["cand"], got, b, f"crafted {name}", ldo, prob=prob, r=c["r"])
            if c["assoc"] is not None:
                assert got[0][b, :k].tolist() == c["assoc"] and (got[4][b], got[5][b]) == (c["accepted"], c["refused"]), name
            assert np.isposinf(got[1][b, :k]).astype(int).tolist() == c["inf"], name
            if name == "common-shift":
                assert abs(got[2][b] - 8.939) < 1e-3
                shift = got[0][b, :k] >= 0
            if name == "common-shift-reordered":  # 5. the order of the message decides: observation 1 at the front is accepted, and takes others out
                back = [c["cand"].index(i) for i in range(5)]
                assert [bool(got[0][b, j] >= 0) for j in back] != shift.tolist() and got[0][b, 0] == 1
            if name == "one-observation":  # D2 of one pairing is the individual gate's m, as the device computes that
                _, mdist = core.gate_observations(obs, n_obs, np.inf)
                assert np.isfinite(mdist[b, 0]) and float(ld.D2) > 1
                assert abs(got[2][b] - mdist[b, 0]) <= ld.bars["D2"] * max(mdist[b, 0], 1)
        core.close()


def test_the_cap_of_64_usable_candidates(built):
    from awesomeslam_amd.core import Core

    X, P, obs, cand = jr.cap64()
    core = Core("ekf", 144, batch=2, max_obs=8, max_wait=16)
    put(core, 0, X, P)
    put(core, 1, X, P)
    o, n_obs = packed([obs, obs[:63]], 64)
    got = core.joint_compat(o, n_obs, cand=rows([cand, cand[:63]], 64), prob=PROB)
    ld = check(X, P, obs, cand, got, 0, "cap 64", 64)
    assert ld.verdicts.count("unusable") == 0 and ld.accepted >= 60
    check(X, P, obs[:63], cand[:63], got, 1, "cap 63", 64)
    core.close()


# ---- 6. the device chain ---------------------------------------------------------------------------------------------------------------------
def test_the_device_chain_runs_in_place(cases, built):
    import torch

    from awesomeslam_amd.core import Core, joint_gates

    keys = [(131, 9), (17, 5), (133, 64)]
    core = Core("ekf", 144, batch=3, max_obs=8, max_wait=16)
    for b, key in enumerate(keys):
        put(core, b, cases[key][0], cases[key][1])
    ldo = 64
    obs, n_obs = packed([cases[key][2] for key in keys], ldo)
    # two steps through host arrays
    cand, _ = core.gate_observations(obs, n_obs, GATE)
    want = core.joint_compat(obs, n_obs, cand=cand, prob=PROB)
    for b, key in enumerate(keys):
        check(*cases[key], want, b, f"chain b={b}", ldo)
    # the chain: the gate writes a tensor, the joint test runs in place on it, on one stream
    st = torch.cuda.Stream()
    dev = torch.from_numpy(obs).cuda()
    a = torch.full((3, ldo), PAT_I, dtype=torch.int32, device="cuda")
    incr = torch.full((3, ldo), PAT_D, dtype=torch.float64, device="cuda")
    joint = torch.full((3, 2), PAT_D, dtype=torch.float64, device="cuda")
    count = torch.full((3, 2), PAT_I, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    core.gate_observations_ptr(dev.data_ptr(), ldo, True, n_obs, GATE, a.data_ptr(), None, st.cuda_stream)
    core.joint_compat_ptr(dev.data_ptr(), ldo, True, n_obs, a.data_ptr(), joint_gates(PROB, ldo), a.data_ptr(), incr.data_ptr(), joint.data_ptr(),
                          count.data_ptr(), st.cuda_stream)
    st.synchronize()
    got = (a.cpu().numpy(), incr.cpu().numpy(), joint.cpu().numpy()[:, 0], joint.cpu().numpy()[:, 1], count.cpu().numpy()[:, 0], count.cpu().numpy()[:, 1])
    assert all(np.array_equal(x, y) for x, y in zip(got, want))  # bit for bit
    assert all(np.array_equal(x, y) for x, y in zip(core.joint_compat(dev, n_obs, prob=PROB, ic_gate=GATE), want))  # cand=None: the same chain
    core.close()


# ---- 7. the call reads and does not write -------------------------------------------------------------------------------------------------------
def test_the_call_is_read_only(built):
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
    states = [core.state(b) for b in range(3)]
    per_filter = [np.array([ar.predicted(X, k) for k in range(4)] + [(9.0, 1.0)], np.float32) for X, _, _ in states]
    obs, n_obs = packed(per_filter, 8)
    got = core.joint_compat(obs, n_obs, prob=PROB)
    ev = core.joint_compat(obs, n_obs, prob=None)
    for b, (X, _, P) in enumerate(states):
        cand = ar.gate_ref(X, P, per_filter[b], gate=GATE, dtype=np.longdouble)[0]
        assert cand[:4].tolist() == [0, 1, 2, 3]
        check(X, P, per_filter[b], cand, got, b, f"ekf-L8 k=49 b={b}", 8)
        check(X, P, per_filter[b], cand, ev, b, f"ekf-L8 k=49 b={b} evaluate", 8, prob=None)
    assert same(everything(), before) and core.snapshot().tobytes() == blob.tobytes()
    assert [core.status(b) for b in range(3)] == [0, 0, 0]
    core.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(cases, built):
    import torch

    from awesomeslam_amd.core import AslamError, Core, joint_gates

    core = Core("ekf", 30, batch=3, max_obs=8, max_wait=16)
    X, P, o, c = cases[(17, 5)]
    for b in range(3):
        put(core, b, X, P)
    ldo = 8
    obs, n_obs = packed([o, o, o], ldo)
    dev = torch.from_numpy(np.concatenate([obs.reshape(-1), np.zeros(4, np.float32)])).cuda()
    cand = torch.from_numpy(np.concatenate([rows([c, c, c], ldo).reshape(-1), np.full(4, PAT_I, np.int32)])).cuda()
    assoc = torch.full((3 * ldo + 4,), PAT_I, dtype=torch.int32, device="cuda")
    incr = torch.full((3 * ldo + 2,), PAT_D, dtype=torch.float64, device="cuda")
    joint = torch.full((3 * 2 + 2,), PAT_D, dtype=torch.float64, device="cuda")
    count = torch.full((3 * 2 + 4,), PAT_I, dtype=torch.int32, device="cuda")
    cand0 = cand.clone()
    tab = joint_gates(PROB, ldo)
    assert all(t.data_ptr() % 16 == 0 for t in (dev, cand, assoc, incr, joint, count))

    def call(obs_ptr=dev.data_ptr(), ld=ldo, is_device=True, k=n_obs, cd=cand.data_ptr(), g=tab, a=assoc.data_ptr(), i=incr.data_ptr(),
             jt=joint.data_ptr(), ct=count.data_ptr()):
        core.joint_compat_ptr(obs_ptr, ld, is_device, k, cd, g, a, i, jt, ct)

    def refused(word, code=-1, **kw):
        with pytest.raises(AslamError, match=rf"aslam_core error {code}: aslam_joint_compat: .*" + word):
            call(**kw)

    def table(m, v):
        t = tab.copy()
        t[m] = v
        return t

    refused("null obs", obs_ptr=None)
    refused("null obs", obs_ptr=None, is_device=False)
    refused("null n_obs", k=None)
    refused("null cand_dev", cd=None)
    refused("null assoc_dev", a=None)
    refused("null joint_dev", jt=None)
    refused("null count_dev", ct=None)
    refused("ldo", ld=0, g=None)
    refused("ldo", ld=-3, g=None)
    refused("ldo.*ASLAM_JC_MAX_OBS", code=-3, ld=65, g=None)
    refused(r"n_obs\[1\].*filter 1", k=[5, ldo + 1, 5])
    refused(r"n_obs\[2\].*filter 2", k=[5, 5, -1])
    for bad in (0.0, -1.0, float("nan"), float("-inf")):
        refused(r"gate_tab\[3\]", g=table(3, bad))
        refused(r"gate_tab\[8\]", g=table(ldo, bad))
    refused("obs.*aligned", obs_ptr=dev.data_ptr() + 4)
    refused("cand_dev.*aligned", cd=cand.data_ptr() + 4)
    refused("assoc_dev.*aligned", a=assoc.data_ptr() + 4)
    refused("incr_dev.*aligned", i=incr.data_ptr() + 8)
    refused("joint_dev.*aligned", jt=joint.data_ptr() + 8)
    refused("count_dev.*aligned", ct=count.data_ptr() + 4)
    refused("cand_dev and assoc_dev overlap", a=cand.data_ptr() + 16)
    refused("cand_dev and assoc_dev overlap", cd=assoc.data_ptr() + 16)
    refused("assoc_dev and incr_dev overlap", i=assoc.data_ptr())
    refused("obs and assoc_dev overlap", a=dev.data_ptr() + 32)
    refused("incr_dev and joint_dev overlap", jt=incr.data_ptr() + 16)
    refused("joint_dev and count_dev overlap", ct=joint.data_ptr() + 32)
    torch.cuda.synchronize()
    assert (assoc == PAT_I).all() and (incr == PAT_D).all() and (joint == PAT_D).all() and (count == PAT_I).all()  # a refused call launches nothing
    assert torch.equal(cand, cand0)
    # the request the refusals were variations of goes through: entry 0 of the table is ignored, infinity is a bound, incr may be left out ...
    call(g=table(0, -5.0), i=None)
    call(g=table(ldo, float("inf")), i=None)
    torch.cuda.synchronize()
    assert (incr == PAT_D).all()
    # ... from the host, and in place
    call(obs_ptr=obs.ctypes.data, is_device=False)
    inplace = cand.clone()
    incr2 = torch.full_like(incr, PAT_D)
    call(cd=inplace.data_ptr(), a=inplace.data_ptr(), i=incr2.data_ptr())
    torch.cuda.synchronize()
    a, i, jt, ct = assoc.cpu().numpy(), incr.cpu().numpy(), joint.cpu().numpy(), count.cpu().numpy()
    assert (a[3 * ldo:] == PAT_I).all() and (i[3 * ldo:] == PAT_D).all() and (jt[6:] == PAT_D).all() and (ct[6:] == PAT_I).all()  # nothing beyond
    assert torch.equal(cand, cand0)                                                       # cand is read only ...
    assert torch.equal(inplace, assoc) and torch.equal(incr2, incr)                       # ... unless it is assoc, with the same result
    got = (a[:3 * ldo].reshape(3, ldo), i[:3 * ldo].reshape(3, ldo), jt[:6].reshape(3, 2)[:, 0], jt[:6].reshape(3, 2)[:, 1],
           ct[:6].reshape(3, 2)[:, 0], ct[:6].reshape(3, 2)[:, 1])
    for b in range(3):
        check(X, P, o, c, got, b, f"after the refusals b={b}", ldo)
    core.close()


# ---- 9. the host mirror --------------------------------------------------------------------------------------------------------------------------
def near_landmark(X, P, centre, lo, hi):
    """a reading near landmark 1 (the world point `centre`) that the individual gate gives to landmark 1 and whose distance m (r = 1e-4, long double) lies inside (lo, hi), the one nearest the
    middle over 24 directions and distances of 0.04 .. 1.48 m: (m, o)"""
    best = None
    for dist in np.arange(0.04, 1.5, 0.04):
        for deg in range(0, 360, 15):
            o = np.array([reading(X, centre + dist * np.array([np.cos(np.radians(deg)), np.sin(np.radians(deg))]))], np.float32)
            a, m = ar.gate_ref(X, P, o, 1e-4, 1e-4, GATE, np.longdouble)
            m = float(m[0])
            if a[0] == 1 and lo < m < hi and (best is None or abs(m - (lo + hi) / 2) < abs(best[0] - (lo + hi) / 2)):
                best = (m, o[0])
    return best


def replayed_node(kind):
    from awesomeslam_amd.core import Node

    tr = trace(8)[0]
    node = Node(kind, tg.dim_cap(8))
    for t in range(30):
        if tr.obs_new[t]:
            c = int(tr.n_obs[t])
            node.sensor_msg(tr.obs[t, :c, 0], tr.obs[t, :c, 1])
        node.odom_msg(tr.odom[t], tr.dt[t])
    assert node.N == 15
    node.set_params(dict(r_range=1e-4, r_bearing=1e-4))
    node.set_assoc_gate(GATE)
    return node, tr


@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_node_drops_what_the_joint_test_refuses(kind, built):
    """trace(8), 30 callbacks with both gates off (N = 15), then r_range = r_bearing = 1e-4, the gate at 9.21 and the joint test at 0.5 (bounds
    1.39, 3.36, 5.35 for one, two, three pairings), and one sensor message: a reading near landmark 1 whose individual m lies between 3 and 9.21
    -- the gate accepts it, the joint test refuses it -- and the exact readings of landmarks 2 and 0.  The near reading comes FIRST, where its
    bound is the 1.39 of one pairing and D2 is its individual m, so that every m above 3 is refused; behind the two exact ones its bound would
    be the 5.35 of three pairings (the rule depends on the order).  Every expected decision is asserted from the references, with margins,
    before the node sees the message."""
    from awesomeslam_amd.core import AslamError, joint_gates

    node, tr = replayed_node(kind)
    assert node.joint_rejected() == 0
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(AslamError, match="probability"):
            node.set_joint_prob(bad)
    node.set_joint_prob(0.5)
    X, Z, _, _ = node.state()
    P = node.P()
    lm = X[3:].reshape(-1, 2)
    m_near, o_near = near_landmark(X, P, lm[1], 3.0, GATE)
    obs = np.array([o_near, reading(X, lm[2]), reading(X, lm[0])], np.float32)
    assert np.abs(obs[:, 1]).max() < 3.14  # (the mirror's binary32 normalisation leaves them as they are)
    tab = joint_gates(0.5, 3)
    assert abs(tab[1] - 1.39) < 0.005
    a_ic, m_ic = ar.gate_ref(X, P, obs, 1e-4, 1e-4, GATE, np.longdouble)
    g_ic, s_ic = ar.margins(X, P, obs, 1e-4, 1e-4, GATE)
    ld = jr.sequential(X, P, obs, a_ic, 1e-4, 1e-4, tab, np.longdouble)
    g, t = jr.margins(X, P, obs, a_ic, 1e-4, 1e-4, tab)
    print(f"node {kind}: individual decisions {a_ic.tolist()} m {[float(f'{v:.3g}') for v in m_ic]} margins {g_ic:.2g} {s_ic:.2g}; joint decisions "
          f"{ld.assoc.tolist()} incr {[float(f'{v:.3g}') for v in ld.incr]} D2 {float(ld.D2):.3g} margins {g:.2g} {t:.2g}")
    assert a_ic.tolist() == [1, 2, 0] and 3.0 < m_near < GATE and g_ic > 1e-6 and s_ic > 1e-6
    assert ld.assoc.tolist() == [-1, 2, 0] and (ld.accepted, ld.refused) == (2, 1) and g > 1e-6 and t > 1e-9
    msg = yaw_msg(X, tr.odom[30][6], tr.odom[30][7])
    wr, wb, wc = node.wait_list()
    seen, hits, clock = node.sightings()
    node.sensor_msg(obs[:, 0].astype(np.float64), obs[:, 1].astype(np.float64))
    assert node.odom_msg(msg, tr.dt[30]) == 1
    X1, Z1, _, _ = node.state()
    wr1, wb1, wc1 = node.wait_list()
    seen1, hits1, clock1 = node.sightings()
    assert node.N == 15 and clock1 == clock + 1
    assert Z1[7] == obs[1, 0] and Z1[8] == obs[1, 1] and Z1[3] == obs[2, 0] and Z1[4] == obs[2, 1]  # Z took the two accepted readings;
    assert np.array_equal(Z1[[5, 6] + list(range(9, 15))], Z[[5, 6] + list(range(9, 15))])          # the refused one left Z
    assert np.array_equal(wr1, wr) and np.array_equal(wb1, wb) and np.array_equal(wc1, wc)          # and the wait-list alone,
    assert node.joint_rejected() == 1 and node.assoc_rejected() == 0                                # is counted where it belongs,
    assert hits1.tolist() == [h + (k in (0, 2)) for k, h in enumerate(hits)] and seen1[2] == seen1[0] == clock1 and seen1[1] == seen[1]  # a drop
    node.close()
    # the joint test switched off again: the same message on the same state associates all three
    node, tr = replayed_node(kind)
    node.set_joint_prob(0.5)
    node.set_joint_prob(0)
    assert np.array_equal(node.state()[0], X) and np.array_equal(node.P(), P)
    hits = node.sightings()[1]
    node.sensor_msg(obs[:, 0].astype(np.float64), obs[:, 1].astype(np.float64))
    assert node.odom_msg(msg, tr.dt[30]) == 1
    Z2 = node.state()[1]
    assert [Z2[i] for i in (5, 6, 7, 8, 3, 4)] == [obs[0, 0], obs[0, 1], obs[1, 0], obs[1, 1], obs[2, 0], obs[2, 1]]
    assert node.joint_rejected() == 0 and node.assoc_rejected() == 0
    assert node.sightings()[1].tolist() == [h + (k in (0, 1, 2)) for k, h in enumerate(hits)]
    node.close()
