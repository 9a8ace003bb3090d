"""-m gpu: stream ordering of the entry points that take a `stream` (the STREAMS paragraph of include/aslam_core.h).

Method, the same everywhere.  A test never compares against numbers of its own: it compares with the SAME call sequence on the null stream
behind torch.cuda.synchronize() -- the same kernels on the same inputs, so the comparison is bit for bit -- which is what the rest of the suite
pins to the oracles.  To make a wrong order visible rather than lucky, every device input starts out holding a DECOY, a different and fully
valid input of the same shape (another seed's trace, an all-zero mask, an all -1 `into` / `cand`, another message's observations, the blob of
another cut, other scans).  On a side stream s the test enqueues a delay, a copy of the real input over the decoy and the call under test;
outputs go into buffers pre-filled with a sentinel on s, a clone() of them is enqueued on s right behind the call, and s alone is synchronised
(Core.sync(stream), never the device).  A launch or copy that is not on s reads the decoy, or is overtaken by the clone.  Every test also
computes the decoy's result and asserts that it differs from the real one.

The delay is torch.cuda._sleep (a chain of fp64 matmuls where that is not usable), calibrated once to DELAY_MS = 80 ms of device time.  It has
to outlast the host's enqueueing of what follows, and the tests check that themselves: for every entry that promises not to synchronise
`stream` (step_batch, replay, replay_stats, select_beyond / select_stale / select_duplicates, gate_observations, joint_compat, scan_landmarks
on device arrays) s.query() must be False when the call returns, else the test FAILS ("the premise did not hold").  Exempt, because their
documentation says they synchronise `stream` inside: the one-trajectory steps, remove_landmarks, merge_landmarks, join_maps, snapshot (the
counts of the batch), restore of a device blob (the headers), scan_landmarks on host arrays; and a call chained behind another one of the SAME
context on s ("synchronises the context first": it waits for its predecessor, hence for the delay) -- there the premise is checked on the
first call of the chain.  Measured on the MI355X: smallest margin 75.5 ms of 80 (MARGIN below).

The limit of the method: it is one-sided.  Streams share hardware queues, so a mis-streamed launch can land behind the delay by accident and
pass; a failure is always real.

Shapes: the single-CU kernels at 8 landmarks (n = 19), batch 3; the three launch chains at capacity dim_cap(80) (the multi-workgroup path) on
a 12-landmark trace (n <= 27), batch 40 = three stream groups of 16 / 16 / 8 filters for the EKF chains (the large-state UKF runs one group).
"""
import functools
import time

import numpy as np
import pytest

from awesomeslam_amd import trace as tg

pytestmark = pytest.mark.gpu

# MARGIN: with DELAY_MS = 80 the slowest call seen on the MI355X (replay_stats of 48 callbacks of the binary64 chain in three stream groups)
# returned 4.5 ms after the delay was enqueued, the smallest margin of the 41 premise checks being 75.5 ms; the single-CU calls return within
# 0.3 ms.  Every check prints its own figure ("premise ...").  Before the host arguments of select_* / gate / joint went through stage_host
# (a blocking null-stream copy then), those calls returned 79.5 .. 79.8 ms after the delay wherever the null stream shared a hardware queue
# with s: margins of 0.2 .. 0.5 ms, which is how the premise check found them.
DELAY_MS = 80.0

T = 48  # three birth stages of trace.STOP_STEPS callbacks, then six callbacks of driving
K = 30  # the cut of the maintenance tests: two stages promoted, one to come
K2 = 44  # "another cut": everything promoted
KNOBS = ("ASLAM_CHOL_RESIDENT", "ASLAM_RIGHT_STEP", "ASLAM_BF16_PIPE", "ASLAM_LARGE_GROUPS", "ASLAM_GS_TILES", "ASLAM_KEEP_L32", "ASLAM_SYRK_RUNNING",
         "ASLAM_SYRK_TAIL")
# name -> (filter, dtype, flags, landmarks of the trace, batch, capacity in landmarks, stream groups)
CTX = {
    "ekf": ("ekf", "f64", 0, 8, 3, 10, 0), "ukf": ("ukf", "f64", 0, 8, 3, 10, 0),
    "ekf-large-f64": ("ekf", "f64", 0, 12, 40, 80, 3), "ekf-large-f32": ("ekf", "f32", 0, 12, 40, 80, 3), "ukf-large": ("ukf", "f64", 1, 12, 40, 80, 1),
}
ALL = list(CTX)
EKF_LARGE = ["ekf-large-f64", "ekf-large-f32"]
GROUPS = ((0, 16), (16, 32), (32, 40))
EDGE_FILTERS = (0, 15, 16, 31, 32, 39)
SENT_I, SENT_F = -7, 12345.0


@pytest.fixture(autouse=True)
def _no_knobs(built, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


# ---- traces, contexts, read-back ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trace(L, B, seed):
    return tg.make_traces(L, T, B=B, seed=seed, sensor_every=2, dt_mode="random")


def traces(name):
    """(the real trace, the decoy: another seed's, of the same shape)"""
    L, B = CTX[name][3], CTX[name][4]
    real, decoy = trace(L, B, 2), trace(L, B, 7)
    assert real.max_obs == decoy.max_obs
    return real, decoy


@functools.lru_cache(maxsize=None)
def ranged(name):
    """the real trace with half of filter 0's first-stage landmarks out of range from callback 20 on: by K they are 10 callbacks stale"""
    tr = traces(name)[0]
    r = float(np.median(tr.obs[0, 5, : tr.n_obs[0, 5], 0]))
    return tg.limit_range(tr, r, t_from=20)


def make(name, max_wait=128):
    from awesomeslam_amd.core import Core, F32, F64

    kind, dtype, flags, L, B, cap, _ = CTX[name]
    core = Core(kind, tg.dim_cap(cap), batch=B, max_obs=traces(name)[0].max_obs, max_wait=max_wait, dtype=F32 if dtype == "f32" else F64, flags=flags)
    assert (core.layout()[0] >= 164) == (cap == 80)
    return core


def assert_launch(core, name):
    """the launch shape the test means to exercise"""
    info = core.launch_info()
    assert info["stream_groups"] == CTX[name][6], (name, info)
    if name == "ekf-large-f32":
        assert info["chol_resident"], (name, info)
    assert (info["launches_per_callback"] > 1) == (CTX[name][5] == 80), (name, info)


def readback(core):
    """everything the getters say about every filter (the first getter synchronises the context's last stream)"""
    return [(np.int64(core.dim(b)),) + core.state(b) + (np.array(core.A(b)),) + core.wait_list(b) + (np.uint32(core.status(b)),) for b in range(core.batch)]


def eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def same(a, b):
    return len(a) == len(b) and all(eq(x, y) for x, y in zip(a, b))


def differing(got, want):
    """the filters whose read-back differs"""
    return [b for b, (g, w) in enumerate(zip(got, want)) if not same(g, w)]


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pinned(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().numpy()


def dev_trace(tr):
    """the narrowed arrays of aslam_trace on the device, in the order set_trace_device takes them"""
    from awesomeslam_amd.core import narrow_odom

    pose, yaw, twist = narrow_odom(tr.odom)
    return [dev(a) for a in (pose, yaw, twist, tr.dt.astype(np.float32), tr.obs_new.astype(np.uint8), tr.n_obs.astype(np.int32), tr.obs.astype(np.float32))]


# ---- the delay and its premise -----------------------------------------------------------------------------------------------------------
_DELAY = None


def delay():
    """DELAY_MS of device time on the current stream; returns the host time at which it was enqueued"""
    import torch

    global _DELAY
    if _DELAY is None:
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        try:
            probe = 1_000_000
            torch.cuda._sleep(probe)
            e0.record()
            torch.cuda._sleep(probe)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if not 0.05 < ms < 1000.0:  # (a counter this probe cannot calibrate: no guess, the matmuls)
                raise RuntimeError(f"torch.cuda._sleep({probe}) took {ms} ms")
            _DELAY = ("sleep", int(probe * DELAY_MS / ms), None)
        except (AttributeError, RuntimeError):
            a = torch.ones((1536, 1536), dtype=torch.float64, device="cuda")
            b = torch.empty_like(a)
            torch.mm(a, a, out=b)
            e0.record()
            torch.mm(a, a, out=b)
            e1.record()
            e1.synchronize()
            _DELAY = ("mm", min(4000, int(DELAY_MS / max(e0.elapsed_time(e1), 1e-3)) + 1), (a, b))
        print(f"delay: {_DELAY[0]} x {_DELAY[1]} for {DELAY_MS} ms")
    kind, k, ab = _DELAY
    t0 = time.perf_counter()
    if kind == "sleep":
        torch.cuda._sleep(k)
    else:
        for _ in range(k):
            torch.mm(ab[0], ab[0], out=ab[1])
    return t0


def premise(s, what, t0):
    """the call has returned: the delay must still be running, or the test proves nothing"""
    busy = not s.query()
    ms = (time.perf_counter() - t0) * 1e3
    print(f"premise {what}: returned {ms:.1f} ms after the delay of {DELAY_MS:.0f} ms was enqueued (margin {DELAY_MS - ms:.1f} ms)")
    assert busy, f"the premise did not hold: the stream was idle when {what} returned, {ms:.1f} ms after a delay of {DELAY_MS} ms was enqueued"


def side_streams(n=1):
    import torch

    return [torch.cuda.Stream() for _ in range(n)]


# ---- 1, 2. replay honours the stream; fork and join of the stream groups ---------------------------------------------------------------
def replay_once(name, mode, stats=False):
    """replay(0, T) [replay_stats] on a device-bound trace.  mode "ref" / "decoy": the null stream behind full synchronisation, on the real /
    the decoy trace.  mode "side": the arrays hold the decoy; on s the delay, the copy of the real trace, the call, the clones.
    Returns (outputs, their clones or None, the read-back of every filter)."""
    import torch

    real, decoy = traces(name)
    core = make(name)
    B = core.batch
    bound = dev_trace(real if mode == "ref" else decoy)
    core.set_trace_device(T, *(a.data_ptr() for a in bound))
    f64, i32 = torch.float64, torch.int32
    outs = {"poses": torch.empty((B, T, 3), dtype=f64, device="cuda"), "dims": torch.empty((B, T), dtype=i32, device="cuda")}
    if stats:
        outs.update(nis=torch.empty((B, T), dtype=f64, device="cuda"), logdet=torch.empty((B, T), dtype=f64, device="cuda"),
                    pose_cov=torch.empty((B, T, 6), dtype=f64, device="cuda"))

    def prefill():
        outs["poses"].fill_(float("nan"))
        outs["dims"].fill_(-1)
        for k in ("nis", "logdet", "pose_cov"):  # (NaN is a value these take: a finite sentinel)
            if k in outs:
                outs[k].fill_(SENT_F)

    def call(st):
        ptr = [outs[k].data_ptr() for k in outs]
        core.replay_stats(0, T, *ptr, stream=st) if stats else core.replay(0, T, *ptr, stream=st)

    clones = None
    if mode == "side":
        src = dev_trace(real)
        (s,) = side_streams()
        with torch.cuda.stream(s):
            prefill()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            t0 = delay()
            for d, r in zip(bound, src):
                d.copy_(r, non_blocking=True)
        call(s.cuda_stream)
        premise(s, f"{'replay_stats' if stats else 'replay'} [{name}]", t0)
        with torch.cuda.stream(s):
            clones = {k: v.clone() for k, v in outs.items()}
        core.sync(s.cuda_stream)
        clones = {k: v.cpu().numpy() for k, v in clones.items()}
    else:
        prefill()
        torch.cuda.synchronize()
        call(None)
        torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    state = readback(core)
    assert_launch(core, name)
    core.close()
    return got, clones, state


@functools.lru_cache(maxsize=None)
def replay_ref(name, mode="ref", stats=False):
    return replay_once(name, mode, stats)


def assert_decoy_differs(name, stats=False):
    (want, _, state), (dec, _, dstate) = replay_ref(name, "ref", stats), replay_ref(name, "decoy", stats)
    assert all(not eq(want[k][b], dec[k][b]) for k in want if k != "dims" for b in range(len(state))), name
    assert len(differing(dstate, state)) == len(state), name


@pytest.mark.parametrize("name", ALL)
def test_replay_honours_the_stream(name):
    """On the two EKF chains this is the FORK test: filters 16 .. 39 run on the auxiliary streams and see the real trace only if ev_fork
    ordered them behind the copy."""
    want, _, wstate = replay_ref(name)
    assert want["dims"][:, -1].tolist() == [3 + 2 * CTX[name][3]] * CTX[name][4] and all(w[-1] == 0 for w in wstate)  # all promoted, status 0
    assert_decoy_differs(name)
    got, _, state = replay_once(name, "side")
    bad = sorted(set(differing(state, wstate)) | {b for b in range(len(state)) if not all(eq(got[k][b], want[k][b]) for k in want)})
    assert not bad, (f"{name}: filters {bad} differ from the null-stream run (the caller's stream carries filters 0 .. 15 of a large EKF batch, the "
                     f"auxiliary streams 16 .. 31 and 32 .. 39; edge filters {EDGE_FILTERS}: {[b for b in EDGE_FILTERS if b in bad]})")


@pytest.mark.parametrize("stats", [False, True], ids=["replay", "replay_stats"])
@pytest.mark.parametrize("name", EKF_LARGE)
def test_groups_join_the_callers_stream(name, stats):
    """The JOIN: a clone enqueued on s behind the call, with no host synchronisation in between, holds every group's rows."""
    want, _, _ = replay_ref(name, "ref", stats)
    assert_decoy_differs(name, stats)
    got, clones, _ = replay_once(name, "side", stats)
    for k in want:
        for lo, hi in GROUPS:
            c = clones[k][lo:hi]
            sentinel = (c == -1) if k == "dims" else np.isnan(c) if k == "poses" else (c == SENT_F)
            assert not sentinel.any(), f"{name} {k}: the clone of filters {lo} .. {hi - 1} was taken before their group had written"
            assert eq(c, want[k][lo:hi]) and eq(got[k][lo:hi], want[k][lo:hi]), (name, k, lo, hi)


# ---- 3. a change of stream between two calls ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def state_at(name, k):
    """the read-back after replay(0, k) on the null stream"""
    import torch

    core = make(name)
    core.set_trace(traces(name)[0])
    core.replay(0, k)
    torch.cuda.synchronize()
    out = readback(core)
    core.close()
    return out


def step_inputs(name, k, j, trajs=None):
    """Host inputs of a batched step behind replay(0, k): twist and dt of callback k + j, Z the filter's own with every range moved by j + 1 cm
    (valid, and not what the device holds).  Pinned, so that the copies are really asynchronous."""
    from awesomeslam_amd.core import narrow_odom

    tr = traces(name)[0]
    _, _, twist = narrow_odom(tr.odom)
    st = state_at(name, k)
    ldz = max(int(s[0]) for s in st)
    Z = np.zeros((len(st), ldz))
    for b, s in enumerate(st):
        Z[b, : s[0]] = s[2]
        Z[b, 3: s[0]: 2] += 0.01 * (j + 1)
    kw = dict(vx=twist[:, k + j, 0].astype(np.float32), az=twist[:, k + j, 1].astype(np.float32), dt=tr.dt[:, k + j].astype(np.float32), Z=Z)
    if CTX[name][0] == "ekf":
        kw.update(a00=np.ones(len(st)), a10=np.zeros(len(st)))
    return {k_: pinned(v) for k_, v in kw.items()}


@pytest.mark.parametrize("name", ALL)
def test_replay_across_a_change_of_stream(name):
    """replay(0, k) on s1 (behind the delay) and replay(k, T - k) on s2 with nothing in between, then the read-backs: one null-stream replay."""
    import torch

    want, _, wstate = replay_ref(name)
    core = make(name)
    core.set_trace(traces(name)[0])
    B, k = core.batch, 20
    p = [torch.full((B, n, 3), float("nan"), dtype=torch.float64, device="cuda") for n in (k, T - k)]
    d = [torch.full((B, n), -1, dtype=torch.int32, device="cuda") for n in (k, T - k)]
    s1, s2 = side_streams(2)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        delay()
    core.replay(0, k, p[0].data_ptr(), d[0].data_ptr(), s1.cuda_stream)
    core.replay(k, T - k, p[1].data_ptr(), d[1].data_ptr(), s2.cuda_stream)
    state = readback(core)  # (waits for s2, the context's last stream, alone)
    poses, dims = np.concatenate([x.cpu().numpy() for x in p], 1), np.concatenate([x.cpu().numpy() for x in d], 1)
    assert_launch(core, name)
    core.close()
    bad = sorted(set(differing(state, wstate)) | {b for b in range(B) if not (eq(poses[b], want["poses"][b]) and eq(dims[b], want["dims"][b]))})
    assert not bad, f"{name}: filters {bad} differ from one null-stream replay"


def step_pair(name, side):
    import torch

    k = 20
    core = make(name)
    core.set_trace(traces(name)[0])
    core.replay(0, k)
    torch.cuda.synchronize()
    ins = [step_inputs(name, k, j) for j in (0, 1)]
    X = [pinned(np.full(ins[0]["Z"].shape, SENT_F)) for _ in ins]
    st = [None, None]
    if side:
        s1, s2 = side_streams(2)
        st = [s1.cuda_stream, s2.cuda_stream]
        with torch.cuda.stream(s1):
            delay()
    for i in (0, 1):
        core.step_batch(X_out=X[i], stream=st[i], **ins[i])
    state = readback(core)
    assert_launch(core, name)
    core.close()
    return [x.copy() for x in X], state


@pytest.mark.parametrize("name", ALL)
def test_step_batch_across_a_change_of_stream(name):
    (X, state), (Xw, wstate) = step_pair(name, True), step_pair(name, False)
    n = int(wstate[0][0])
    assert not eq(Xw[0][:, :n], Xw[1][:, :n]) and not (Xw[1][:, :n] == SENT_F).any()
    assert eq(X[0], Xw[0]) and eq(X[1], Xw[1]) and not differing(state, wstate), (name, differing(state, wstate))


def replay_then_step(name, side):
    """replay up to and including the callback that grows filter 0, then ONE step of filter 0 on another stream: the n that step reads"""
    import torch

    dims = replay_ref(name)[0]["dims"][0]
    kg = int(np.flatnonzero(np.diff(dims) > 0)[0]) + 1  # callback kg grows the filter: the first birth stage (trace.STOP_STEPS callbacks at rest)
    assert kg < tg.STOP_STEPS and dims[kg] > dims[kg - 1] == 3
    ins = step_inputs(name, kg + 1, 0)
    core = make(name)
    core.set_trace(traces(name)[0])
    st = [None, None]
    torch.cuda.synchronize()
    if side:
        s1, s2 = side_streams(2)
        st = [s1.cuda_stream, s2.cuda_stream]
        with torch.cuda.stream(s1):
            delay()
    core.replay(0, kg + 1, stream=st[0])
    assert_launch(core, name)
    n = int(dims[kg])
    arg = (0, ins["vx"][0], ins["az"][0], ins["dt"][0], ins["Z"][0, :n].copy())
    X = core.ekf_step(*arg, 1.0, 0.0, stream=st[1]) if CTX[name][0] == "ekf" else core.ukf_step(*arg, stream=st[1])
    state = readback(core)
    core.close()
    return X, state, n


@pytest.mark.parametrize("name", ALL)
def test_one_step_behind_a_growing_replay_on_another_stream(name):
    (X, state, n), (Xw, wstate, _) = replay_then_step(name, True), replay_then_step(name, False)
    assert wstate[0][0] == n == len(Xw) and eq(X, Xw) and not differing(state, wstate), (name, n, differing(state, wstate))


@pytest.mark.parametrize("name", ALL)
def test_an_unchanged_stream_adds_nothing(name):
    """Two replays on ONE side stream: the second neither waits for the first (the stream is still busy with the delay when it returns) nor
    launches anything else than it launches on the null stream."""
    import torch

    want, _, wstate = replay_ref(name)
    null = make(name)
    null.set_trace(traces(name)[0])
    null.replay(0, 20)
    null.replay(20, T - 20)
    torch.cuda.synchronize()
    winfo = (null.launch_info(), null.kernel_info())
    null.close()
    core = make(name)
    core.set_trace(traces(name)[0])
    (s,) = side_streams()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        t0 = delay()
    core.replay(0, 20, stream=s.cuda_stream)
    info0 = (core.launch_info(), core.kernel_info())
    core.replay(20, T - 20, stream=s.cuda_stream)
    premise(s, f"the second replay on one stream [{name}]", t0)
    info1 = (core.launch_info(), core.kernel_info())
    assert_launch(core, name)
    state = readback(core)
    core.close()
    assert info0 == info1 == winfo, (info0, info1, winfo)
    assert not differing(state, wstate)


# ---- 4. the per-callback seam ----------------------------------------------------------------------------------------------------------------
SEAM = [("ekf", "ekf_step"), ("ekf", "ekf_step_sighted"), ("ekf", "step_batch"), ("ekf", "step_batch_sighted"), ("ukf", "ukf_step"), ("ukf", "step_batch"),
        ("ekf-large-f32", "step_batch"), ("ekf-large-f32", "ekf_step"), ("ukf-large", "step_batch")]


def seam(name, variant, side):
    import torch

    k = 20
    core = make(name)
    core.set_trace(traces(name)[0])
    core.replay(0, k)
    assert_launch(core, name)  # (of the replay: a one-trajectory step of a large context is one group by design)
    torch.cuda.synchronize()
    ins = step_inputs(name, k, 0)
    B, ldz = ins["Z"].shape
    n = int(state_at(name, k)[0][0])
    mask = pinned((np.add.outer(np.arange(B), np.arange(ldz // 2 + 1)) % 2).astype(np.uint8))
    st, t0 = None, None
    if side:
        (s,) = side_streams()
        st = s.cuda_stream
        with torch.cuda.stream(s):
            t0 = delay()
    if variant.startswith("step_batch"):
        X = pinned(np.full((B, ldz), SENT_F))
        core.step_batch(X_out=X, stream=st, sighted=mask if variant.endswith("sighted") else None, **ins)
        if side:
            premise(s, f"{variant} [{name}]", t0)
    else:  # (the one-trajectory steps synchronise `stream` inside: no premise)
        arg = (1, ins["vx"][1], ins["az"][1], ins["dt"][1], ins["Z"][1, :n].copy())
        if variant == "ukf_step":
            X = core.ukf_step(*arg, stream=st)
        else:
            X = core.ekf_step(*arg, 1.0, 0.0, stream=st, sighted=mask[1] if variant.endswith("sighted") else None)
    core.sync(st)
    X = np.array(X)
    sighted = [core.sighted(b) for b in range(B)] if CTX[name][0] == "ekf" else []
    state = readback(core)
    core.close()
    return X, sighted, state


@pytest.mark.parametrize("name,variant", SEAM)
def test_per_callback_seam_on_a_side_stream(name, variant):
    (X, sighted, state), (Xw, wsighted, wstate) = seam(name, variant, True), seam(name, variant, False)
    before = state_at(name, 20)
    assert differing(wstate, before) and not (Xw[..., :3] == SENT_F).any()  # the step did something
    if variant.endswith("sighted"):
        assert any(m.any() for m in wsighted)
    assert eq(X, Xw) and same(sighted, wsighted) and not differing(state, wstate), (name, variant, differing(state, wstate))


# ---- 5. the maintenance entries ----------------------------------------------------------------------------------------------------------
def mask_ld(core):
    return (max(core.landmark_capacity(), 1) + 15) // 16 * 16


class Op:
    """One maintenance entry (or a chain of two through one device array).  inputs(core, name) -> (real, decoy) host arrays of the device
    input; outputs(core) -> device output tensors; call(core, name, inp, outs, st, check) -> host results, check(what) once after the first
    call that promises not to synchronise `st`."""
    trace = "plain"
    chained = False

    def outputs(self, core):
        return []


class RemoveMask(Op):
    def inputs(self, core, name):
        real = np.zeros((core.batch, mask_ld(core)), np.uint8)
        real[:, 1] = 1
        return real, np.zeros_like(real)

    def call(self, core, name, inp, outs, st, check):  # (synchronises `st` inside: no premise)
        core.remove_landmarks_ptr(inp.data_ptr(), inp.shape[1], True, st)
        return []


class SelectBeyond(Op):
    """select_beyond + remove_landmarks through one device mask, which starts out all zero"""
    chained = True

    def inputs(self, core, name):
        z = np.zeros((core.batch, mask_ld(core)), np.uint8)
        return z, z

    def max_range(self, name):
        X = state_at(name, K)[0][1]
        return float(np.median(np.hypot(X[3::2] - X[0], X[4::2] - X[1])))

    def call(self, core, name, inp, outs, st, check, select=True):
        if select:
            core.select_beyond(self.max_range(name), inp.data_ptr(), inp.shape[1], st)
            check("select_beyond")
        core.remove_landmarks_ptr(inp.data_ptr(), inp.shape[1], True, st)
        return []


class SelectStale(SelectBeyond):
    trace = "ranged"

    def call(self, core, name, inp, outs, st, check, select=True):
        if select:
            core.select_stale(5, inp.data_ptr(), inp.shape[1], st)
            check("select_stale")
        core.remove_landmarks_ptr(inp.data_ptr(), inp.shape[1], True, st)
        return []


class MergeInto(Op):
    def inputs(self, core, name):
        real = np.full((core.batch, mask_ld(core)), -1, np.int32)
        real[:, 1] = 0
        return real, np.full_like(real, -1)

    def call(self, core, name, inp, outs, st, check):  # (synchronises `st` inside: no premise)
        return [core.merge_landmarks_ptr(inp.data_ptr(), inp.shape[1], True, 0.01, st)]


class SelectDuplicates(Op):
    """select_duplicates + merge_landmarks through one device array, which starts out all -1"""
    chained = True

    def inputs(self, core, name):
        z = np.full((core.batch, mask_ld(core)), -1, np.int32)
        return z, z

    def call(self, core, name, inp, outs, st, check, select=True):
        if select:
            core.select_duplicates(float("inf"), 1.0e3, inp.data_ptr(), inp.shape[1], st)
            check("select_duplicates")
        return [core.merge_landmarks_ptr(inp.data_ptr(), inp.shape[1], True, 0.01, st)]


class GateJoint(Op):
    """gate_observations on a device message, joint_compat in place on its output"""

    def inputs(self, core, name):
        tr = traces(name)[0]
        return tr.obs[:, K - 1].astype(np.float32), tr.obs[:, 5].astype(np.float32)  # the stored message; another message

    def outputs(self, core):
        import torch

        B, ldo = core.batch, core.max_obs
        return [torch.empty((B, ldo), dtype=torch.int32, device="cuda"), torch.empty((B, ldo), dtype=torch.float64, device="cuda"),
                torch.empty((B, ldo), dtype=torch.float64, device="cuda"), torch.empty((B, 2), dtype=torch.float64, device="cuda"),
                torch.empty((B, 2), dtype=torch.int32, device="cuda")]

    def call(self, core, name, inp, outs, st, check):
        from awesomeslam_amd.core import joint_gates

        n_obs, ldo = traces(name)[0].n_obs[:, K - 1], core.max_obs
        assoc, mdist, incr, joint, count = outs
        core.gate_observations_ptr(inp.data_ptr(), ldo, True, n_obs, 9.21, assoc.data_ptr(), mdist.data_ptr(), st)
        check("gate_observations")
        core.joint_compat_ptr(inp.data_ptr(), ldo, True, n_obs, assoc.data_ptr(), joint_gates(0.99, ldo), assoc.data_ptr(), incr.data_ptr(),
                              joint.data_ptr(), count.data_ptr(), st)
        return []


class JointCand(Op):
    """joint_compat on device candidates: the pairings the chain above accepted, against all -1"""

    def inputs(self, core, name):
        real = maintenance(name, "gate+joint", "cand")
        assert (real >= 0).any()
        self.obs = dev(traces(name)[0].obs[:, K - 1].astype(np.float32))  # (uploaded here: a blocking copy behind the delay would wait for it)
        return real, np.full_like(real, -1)

    def outputs(self, core):
        return GateJoint.outputs(self, core)[:1] + GateJoint.outputs(self, core)[2:]

    def call(self, core, name, inp, outs, st, check):
        from awesomeslam_amd.core import joint_gates

        tr, ldo = traces(name)[0], core.max_obs
        assoc, incr, joint, count = outs
        core.joint_compat_ptr(self.obs.data_ptr(), ldo, True, tr.n_obs[:, K - 1], inp.data_ptr(), joint_gates(0.99, ldo), assoc.data_ptr(), incr.data_ptr(),
                              joint.data_ptr(), count.data_ptr(), st)
        check("joint_compat")
        return []


@functools.lru_cache(maxsize=None)
def blob_at(name, k):
    """the host snapshot of a null-stream run cut at k"""
    import torch

    core = make(name)
    core.set_trace(traces(name)[0])
    core.replay(0, k)
    torch.cuda.synchronize()
    blob = core.snapshot()
    core.close()
    blob.setflags(write=False)
    return blob


def two_blobs(name, k_real, k_decoy):
    """two blobs in arrays of one length (a blob says itself how long it is)"""
    a, b = blob_at(name, k_real), blob_at(name, k_decoy)
    n = (max(a.size, b.size) + 63) // 64 * 64
    out = np.zeros((2, n), np.uint8)
    out[0, : a.size], out[1, : b.size] = a, b
    return out[0], out[1]


class JoinMaps(Op):
    """join_maps of a device blob: landmark 0 of every record of the cut at K2 (decoy: of the cut at K), moved 50 m away"""

    def inputs(self, core, name):
        return two_blobs(name, K2, K)

    def call(self, core, name, inp, outs, st, check):  # (synchronises `st` inside: no premise)
        B = core.batch
        sel = np.zeros((B, mask_ld(core)), np.uint8)
        sel[:, 0] = 1
        idx = np.arange(B, dtype=np.int32)
        return [core.join_maps_ptr(idx, idx, B, inp.data_ptr(), inp.numel(), True, [(50.0, 50.0, 0.0, None)] * B, sel.ctypes.data, sel.shape[1], st)]


class Restore(Op):
    """restore of a device blob into the running context: the cut at K itself (the run goes on as if nothing had happened) against the cut at
    K2.  What the snapshot test below cannot see, because aslam_snapshot waits out its delay: the header gather and the unpack behind a copy."""

    def inputs(self, core, name):
        return two_blobs(name, K, K2)

    def call(self, core, name, inp, outs, st, check):  # (synchronises `st` inside, for the headers: no premise)
        core.restore(inp, records=list(range(core.batch)), stream=st)
        return []


OPS = {"restore": Restore(), "remove": RemoveMask(), "select_beyond+remove": SelectBeyond(), "select_stale+remove": SelectStale(), "merge": MergeInto(),
       "select_duplicates+merge": SelectDuplicates(), "gate+joint": GateJoint(), "joint": JointCand(), "join_maps": JoinMaps()}
_MAINT = {}


def maintenance(name, op_name, mode):
    """replay(0, K) on the null stream, the entry, replay(K, T - K).  mode "ref" / "decoy": all on the null stream behind full
    synchronisation, the device input holding the real / the decoy array; "side": the input holds the decoy, on s the delay, the copy of the
    real array and the entry, then the rest of the trace on ANOTHER stream.  "cand": the gate's output of the "ref" run.
    Returns (host results, device outputs, the read-back at the end)."""
    import torch

    if mode == "cand":
        return maintenance(name, op_name, "ref")[1][0]
    if mode != "side" and (name, op_name, mode) in _MAINT:
        return _MAINT[name, op_name, mode]
    op = OPS[op_name]
    core = make(name)
    core.set_trace(ranged(name) if op.trace == "ranged" else traces(name)[0])
    core.replay(0, K)
    torch.cuda.synchronize()
    real, decoy = op.inputs(core, name)
    outs = op.outputs(core)

    def prefill():
        for o in outs:
            o.fill_(SENT_F if o.is_floating_point() else SENT_I)

    if mode == "side":
        inp, src = dev(decoy), dev(real)
        s, s2 = side_streams(2)
        with torch.cuda.stream(s):
            prefill()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            t0 = delay()
            inp.copy_(src, non_blocking=True)
        host = op.call(core, name, inp, outs, s.cuda_stream, lambda what: premise(s, f"{what} [{name}]", t0))
        with torch.cuda.stream(s):
            clones = [o.clone() for o in outs]
        core.replay(K, T - K, stream=s2.cuda_stream)
        assert_launch(core, name)
        core.sync(s.cuda_stream)
        got = [o.cpu().numpy() for o in outs]
        assert all(eq(c.cpu().numpy(), g) for c, g in zip(clones, got)), (name, op_name)
        state = readback(core)  # (waits for s2)
    else:
        inp = dev(real if mode == "ref" else decoy)
        prefill()
        torch.cuda.synchronize()
        kw = {"select": False} if mode == "decoy" and op.chained else {}  # (the decoy of a chain: the array as it starts out, no selector)
        host = op.call(core, name, inp, outs, None, lambda what: None, **kw)
        torch.cuda.synchronize()
        core.replay(K, T - K)
        assert_launch(core, name)
        torch.cuda.synchronize()
        got = [o.cpu().numpy() for o in outs]
        state = readback(core)
    core.close()
    res = ([np.array(h) for h in host], got, state)
    if mode != "side":
        _MAINT[name, op_name, mode] = res
    return res


# every entry on the single-CU EKF and UKF, the large f32 chain and the large-state UKF; the binary64 chain once more for a chained selector
MAINT = [(n, o) for o in OPS for n in ("ekf", "ukf", "ekf-large-f32", "ukf-large")] + [("ekf-large-f64", "select_beyond+remove")]


@pytest.mark.parametrize("name,op", MAINT)
def test_maintenance_entry_behind_the_delay(name, op):
    want, dec = maintenance(name, op, "ref"), maintenance(name, op, "decoy")
    assert not all(same(a, b) for a, b in zip(want[:2], dec[:2])) or differing(dec[2], want[2]), (name, op, "the decoy gives the same result")
    assert differing(dec[2], want[2]) or op in ("gate+joint", "joint"), (name, op)  # (the two association calls write nothing a filter owns)
    got = maintenance(name, op, "side")
    assert same(got[0], want[0]), (name, op, got[0], want[0])  # merged / joined counts
    assert same(got[1], want[1]), (name, op)  # assoc, mdist, incr, joint, count
    assert not differing(got[2], want[2]), (name, op, differing(got[2], want[2]))


@pytest.mark.parametrize("name", ["ekf", "ukf", "ekf-large-f32", "ukf-large"])
def test_snapshot_and_restore_through_a_device_blob(name):
    """snapshot(out = device buffer) of context a and restore from it into context b, both on s behind the delay; the buffer starts out
    holding the blob of another cut.  b then runs the rest of the trace on another stream.  (Both calls synchronise s inside -- the counts,
    the headers -- so there is no premise to check, and aslam_snapshot waits out the delay before it enqueues its pack: what is tested is
    that pack, unpack and the continuation are in order on an idle stream.  The "restore" entry of the maintenance test above puts
    aslam_restore of a device blob behind a delay and a copy.)"""
    import torch

    want, _, wstate = replay_ref(name)
    B = CTX[name][4]
    real, decoy = two_blobs(name, K, K2)
    assert blob_at(name, K).size != blob_at(name, K2).size
    a, b = make(name), make(name)
    a.set_trace(traces(name)[0])
    b.set_trace(traces(name)[0])
    a.replay(0, K)
    buf = dev(decoy)
    s, s2 = side_streams(2)
    poses = torch.full((B, T - K, 3), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay()
    blob = a.snapshot(out=buf, stream=s.cuda_stream)
    b.restore(blob, records=list(range(B)), stream=s.cuda_stream)
    with torch.cuda.stream(s):
        clone = blob.clone()
    b.replay(K, T - K, poses.data_ptr(), None, s2.cuda_stream)
    state = readback(b)
    a.sync(s.cuda_stream)
    assert clone.cpu().numpy().tobytes() == blob_at(name, K).tobytes() == blob.cpu().numpy().tobytes()
    assert eq(poses.cpu().numpy(), want["poses"][:, K:]) and not differing(state, wstate), (name, differing(state, wstate))
    assert_launch(b, name)
    a.close()
    b.close()


# ---- 6. the scan front end -------------------------------------------------------------------------------------------------------------------
def test_scan_front_end_on_a_side_stream():
    """130 scans: positions 0 / 63 / 64 / 129 of a launch are in it"""
    import torch

    from awesomeslam_amd.core import scan_landmarks, scan_landmarks_device
    from oracle import scan_oracle as so

    N, MO = 130, 32
    real, decoy = so.make_scans(N, seed=3).astype(np.float32), so.make_scans(N, seed=5).astype(np.float32)

    def outs():
        return [torch.full((N,), SENT_I, dtype=torch.int32, device="cuda"), torch.full((N, MO), SENT_F, dtype=torch.float32, device="cuda"),
                torch.full((N, MO), SENT_F, dtype=torch.float32, device="cuda"), torch.full((N,), 77, dtype=torch.int32, device="cuda")]

    def call(inp, o, st):
        scan_landmarks_device(inp.data_ptr(), N, MO, o[1].data_ptr(), o[2].data_ptr(), o[0].data_ptr(), o[3].data_ptr(), 0, st)

    res = {}
    for which, arr in (("real", real), ("decoy", decoy)):
        inp, o = dev(arr), outs()
        torch.cuda.synchronize()
        call(inp, o, None)
        torch.cuda.synchronize()
        res[which] = [x.cpu().numpy() for x in o]
    want = res["real"]
    assert want[0].min() >= 0 and want[0].max() > 0 and not all(eq(x, y) for x, y in zip(want, res["decoy"]))
    host = scan_landmarks(real, max_out=MO)  # n, range, bearing, status: the host form on the null stream
    assert eq(host[0], want[0]) and eq(host[3].astype(np.int32), want[3])
    for i in range(N):
        assert eq(host[1][i, : host[0][i]], want[1][i, : host[0][i]]) and eq(host[2][i, : host[0][i]], want[2][i, : host[0][i]]), i

    inp, src = dev(decoy), dev(real)
    (s,) = side_streams()
    with torch.cuda.stream(s):
        o = outs()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        t0 = delay()
        inp.copy_(src, non_blocking=True)
    call(inp, o, s.cuda_stream)
    premise(s, "scan_landmarks on device arrays", t0)
    with torch.cuda.stream(s):
        clones = [x.clone() for x in o]
    s.synchronize()
    for pos in (0, 63, 64, 129):
        assert all(eq(x.cpu().numpy()[pos], w[pos]) for x, w in zip(o, want)), f"scan {pos}"
    assert all(eq(x.cpu().numpy(), w) for x, w in zip(o, want)) and all(eq(x.cpu().numpy(), w) for x, w in zip(clones, want))
    # the host-array form on s (it synchronises s inside), behind the delay
    with torch.cuda.stream(s):
        delay()
    again = scan_landmarks(real, max_out=MO, stream=s.cuda_stream)
    assert same(again, host)


# ---- 7. read-backs after side-stream work ----------------------------------------------------------------------------------------------------
GETTERS = {
    "dim": lambda c: c.dim(1), "state": lambda c: c.state(1), "landmarks": lambda c: c.landmarks(1), "wait_list": lambda c: c.wait_list(1),
    "status": lambda c: c.status(1), "innovation": lambda c: c.innovation(1), "sighted": lambda c: c.sighted(1), "sightings": lambda c: c.sightings(1),
    "params": lambda c: tuple(c.params(1).as_dict().values()), "replay_gate": lambda c: c.replay_gate(1), "assoc_rejected": lambda c: c.assoc_rejected(1),
}


def flat(v):
    return [np.asarray(x) for x in (v if isinstance(v, tuple) else (v,))]


@pytest.mark.parametrize("name", ["ekf", "ekf-large-f32"])
def test_every_read_back_waits_for_the_side_stream(name):
    """Each getter as the FIRST host call behind an un-synchronised replay on s (behind the delay): they promise to synchronise the context's
    last stream.  So that a getter which did not wait (and returned what reset() left) is seen, the run is made to change what each one says:
    the innovation record is on; the Mahalanobis gate is 1e-6, so observations are dropped and assoc_rejected counts (R is 0.2 on range and
    bearing against readings noisy by 0.02 m and 0.002 rad, so m is of the order 1e-3 and below: a gate of 1.0 drops nothing, this one
    passes only a reading within half a millimetre and half a milliradian of the prediction); max_wait is 3, below the landmarks of one birth stage plus the next, so the wait-list is in use and
    ASLAM_ST_WAIT_OVERFLOW is set.  params and replay_gate are written by no replay: their two cases check that the call works behind
    side-stream work and returns the constants, nothing more."""
    import torch

    def run(getter, side):
        core.reset()
        torch.cuda.synchronize()
        st = None
        if side:
            with torch.cuda.stream(s):
                delay()
            st = s.cuda_stream
        core.replay(0, T, stream=st)
        if not side:
            torch.cuda.synchronize()
        out = flat(GETTERS[getter](core))
        assert_launch(core, name)
        return out

    core = make(name, max_wait=3)
    core.set_trace(traces(name)[0])
    core.enable_innovation()
    core.set_replay_gate(1.0e-6)
    (s,) = side_streams()
    fresh = {g: flat(GETTERS[g](core)) for g in GETTERS}
    for g in GETTERS:
        want = run(g, False)
        if g not in ("params", "replay_gate"):
            assert not same(want, fresh[g]), (g, "says the same before and after the run", want)
        got = run(g, True)
        assert same(got, want), (name, g, got, want)
    core.close()
