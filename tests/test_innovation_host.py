"""The innovation statistics without a GPU: the ABI (new functions declared and exported, struct and version untouched, argument errors),
the Sherman-Morrison forms the UKF kernels evaluate against the direct values of the oracle's S, and awesomeslam_amd.consistency."""
import ctypes
import math
import os
import re

import numpy as np

from awesomeslam_amd import consistency as cs
from awesomeslam_amd import core
from awesomeslam_amd import trace as tg
from innovation_ref import StatsFilter, sherman_morrison_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CORE = ("aslam_replay_stats", "aslam_innovation_enable", "aslam_get_innovation")
NEW_NODE = ("aslam_node_enable_innovation", "aslam_node_innovation")


def header(path):
    txt = open(os.path.join(ROOT, path)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"//[^\n]*", "", txt)


def test_header_declares_the_new_functions_and_the_symbol_lists_agree(built):
    h = header("include/aslam_core.h")
    names = sorted(set(re.findall(r"\b(aslam_[A-Za-z_0-9]+)\s*\(", h)))
    assert sorted(core.CORE_SYMBOLS) == names
    lib = ctypes.CDLL(os.path.join(ROOT, "awesomeslam_amd", "csrc", "libaslam_core.so"))
    for n in NEW_CORE:
        assert n in names and n in core.CORE_SYMBOLS and hasattr(lib, n), n
    hn = header("awesomeslam_amd/csrc/host/aslam_node.h")
    node_names = sorted(n for n in set(re.findall(r"\b(aslam_[A-Za-z_0-9]+)\s*\(", hn)) if n.startswith(("aslam_node", "aslam_host")))
    assert sorted(core.NODE_SYMBOLS) == node_names
    nlib = core.node_lib()
    for n in NEW_NODE:
        assert n in node_names and hasattr(nlib, n), n
    # the argument list of the replay seam with statistics: aslam_replay's, then the three arrays, then the stream
    m = re.search(r"int\s+aslam_replay_stats\s*\(([^)]*)\)", h)
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "t0", "nsteps", "poses_out", "dims_out", "nis_out", "logdet_out", "pose_cov_out", "stream"]
    assert all(args[i].startswith("double *") for i in (5, 6, 7))


def test_abi_version_and_config_are_unchanged(built):
    h = header("include/aslam_core.h")
    assert re.search(r"#define\s+ASLAM_ABI_VERSION\s+1\b", h) and core.core_lib().aslam_abi_version() == 1
    m = re.search(r"typedef struct\s*\{([^}]*)\}\s*aslam_config;", h)
    fields = re.findall(r"int32_t\s+(\w+);", m.group(1))
    assert fields == ["filter", "dtype", "max_landmark_count", "batch", "max_obs", "max_wait", "device", "flags"]
    assert [f for f, _ in core.Config._fields_] == fields and ctypes.sizeof(core.Config) == 32
    # no new configuration bit: ASLAM_CFG_UKF_LARGE stays the only one
    assert re.findall(r"\b(ASLAM_CFG_\w+)\s*=", h) == ["ASLAM_CFG_UKF_LARGE"]


def test_null_context_is_an_argument_error(built):
    lib = core.core_lib()
    a, b = ctypes.c_double(), ctypes.c_double()
    assert lib.aslam_replay_stats(None, 0, 1, None, None, None, None, None, None) == -1
    assert lib.aslam_innovation_enable(None, 1) == -1
    assert lib.aslam_get_innovation(None, 0, ctypes.byref(a), ctypes.byref(b)) == -1
    assert b"null" in lib.aslam_last_error()


def direct_and_sherman_morrison(o):
    """(direct nis, sign, ln|det|) of the oracle's S and the same three from the factor of S+ = S + z z^T, z = sqrt(-w_0) dz_0"""
    w0 = float(o.weights[0])
    assert w0 < 0.0
    z = math.sqrt(-w0) * o.dz0
    S_plus = o.S + np.outer(z, z)
    assert np.linalg.eigvalsh((S_plus + S_plus.T) / 2).min() > 0.0
    return (o.nis, o.sign, o.logdet), sherman_morrison_stats(S_plus, z, o.y)


def test_sherman_morrison_forms_on_oracle_states_of_a_trace():
    """NIS = t.t + (q.t)^2 / (1 - q.q) and det S = det S+ (1 - q.q) against solve / slogdet on the oracle's own S, every callback of a trace"""
    L, T = 8, 60
    tr = tg.make_traces(L, T, B=1, seed=3)[0]
    o = StatsFilter("ukf", tg.dim_cap(L))
    checked = 0
    for t in range(T):
        if tr.obs_new[t]:
            k = int(tr.n_obs[t])
            o.sensor_msg(tr.obs[t, :k, 0], tr.obs[t, :k, 1])
        if not o.odom_msg(*tr.odom[t], tr.dt[t]) or o.N == 3:
            continue  # (N = 3 has w_0 = -2/3 as well, but nothing of interest: the callbacks with landmarks are the case)
        (nis, sign, ld), (nis_sm, sign_sm, ld_sm) = direct_and_sherman_morrison(o)
        assert sign == sign_sm
        assert abs(nis_sm - nis) <= 1e-10 * max(abs(nis), 1e-300) or abs(nis) < 1e-25, (t, nis, nis_sm)
        assert abs(ld_sm - ld) <= 1e-10 * abs(ld), (t, ld, ld_sm)
        checked += 1
    assert checked >= 30 and o.N == 2 * L + 3


def test_sherman_morrison_forms_with_an_indefinite_S():
    """A state whose sigma-point headings straddle +-pi: the central column of Zsig - Zpred is large, S = S+ - z z^T is indefinite and
    1 - q.q < 0.  The signed quadratic form and ln |det S| must still be those of numpy on the oracle's S."""
    # heading 3.13 with a pose-landmark covariance that is strongly correlated: some sigma points pass +pi and are wrapped, the others are not,
    # so the bearings of Zsig are 2 pi apart and the central column of Zsig - Zpred is of order one against a weight of (1 - N) / 3
    n, nl = 9, 3
    rng = np.random.default_rng(3)
    X = np.concatenate([[0.5, -0.3, 3.13], (np.array([3.0, 0.0]) + 2 * rng.normal(size=(nl, 2))).ravel()])
    A = rng.normal(size=(n, n)) * 0.4
    P = A @ A.T / n + np.eye(n) * 0.01
    Z = X.copy()
    for i in range(nl):
        dx, dy = X[3 + 2 * i] - X[0], X[4 + 2 * i] - X[1]
        Z[3 + 2 * i] = np.float32(math.hypot(dx, dy) + 0.01)
        Z[4 + 2 * i] = np.float32(math.atan2(dy, dx) - X[2] + 0.002)
    o = StatsFilter("ukf", n + 2)
    o.set_state(n, X, Z, P)
    o.slam(np.float32(0.2), np.float32(0.1), np.float32(1.0))
    (nis, sign, ld), (nis_sm, sign_sm, ld_sm) = direct_and_sherman_morrison(o)
    assert sign < 0 and sign_sm < 0, "the construction must make det S negative (1 - q.q < 0)"
    assert np.linalg.eigvalsh((o.S + o.S.T) / 2).min() < 0.0
    assert abs(nis_sm - nis) <= 1e-10 * abs(nis), (nis, nis_sm)
    assert abs(ld_sm - ld) <= 1e-10 * abs(ld), (ld, ld_sm)


def test_reference_helper_on_both_filters():
    """the taps see one inverse per step and an innovation of the state's length; S of the EKF is positive definite"""
    for kind in ("ekf", "ukf"):
        L, T = 8, 40
        trs = tg.make_traces(L, T, B=1, seed=3)
        trs.obs_new[0, :2] = 0  # two callbacks before the first sensor message: cbOdom returns early
        tr = trs[0]
        o = StatsFilter(kind, tg.dim_cap(L))
        poses, dims, nis, logdet, pcov, ran = o.replay_stats(tr)
        assert not ran[:2].any() and ran[2:].all()
        po, do = StatsFilter(kind, tg.dim_cap(L)).replay(tr)
        assert np.array_equal(poses, po) and np.array_equal(dims, do)
        assert np.isnan(nis[~ran]).all() and np.isnan(logdet[~ran]).all() and np.isnan(pcov[~ran]).all()
        assert np.isfinite(nis[ran]).all() and np.isfinite(logdet[ran]).all() and ran.any() and not ran.all()
        assert abs(nis[np.argmax(ran)]) < 1e-9  # the callback that seeds X <- Z: the innovation is what one prediction moved the pose
        if kind == "ekf":
            assert (nis[ran] >= 0).all()


def test_log_likelihood():
    # one dimension, S = 4, y = 2: -1/2 (1 + ln 4 + ln 2 pi)
    assert math.isclose(cs.log_likelihood(1.0, math.log(4.0), 1), -0.5 * (1.0 + math.log(4.0) + math.log(2 * math.pi)), rel_tol=1e-15)
    ll = cs.log_likelihood([0.0, 3.0, np.nan], [0.0, -1.0, 2.0], [3, 5, 7])
    assert math.isclose(ll[0], -1.5 * math.log(2 * math.pi), rel_tol=1e-15)
    assert math.isclose(ll[1], -0.5 * (3.0 - 1.0 + 5 * math.log(2 * math.pi)), rel_tol=1e-15)
    assert np.isnan(ll[2])


def test_pose_nees():
    # diagonal covariance: the sum of squared errors over the variances
    cov = [4.0, 0.0, 1.0, 0.0, 0.0, 0.25]
    assert math.isclose(cs.pose_nees([1.0, 2.0, 0.5], cov, [0.0, 0.0, 0.0]), 1.0 / 4 + 4.0 / 1 + 0.25 / 0.25, rel_tol=1e-14)
    # the heading error is wrapped: 3.1 against -3.1 is 2 pi - 6.2, not 6.2
    e = 2 * math.pi - 6.2
    assert math.isclose(cs.pose_nees([0.0, 0.0, -3.1], cov, [0.0, 0.0, 3.1]), e * e / 0.25, rel_tol=1e-12)
    # a full matrix, by hand: P = [[2, 1, 0], [1, 2, 0], [0, 0, 1]], e = (1, 0, 0): e^T P^-1 e = 2 / 3
    assert math.isclose(cs.pose_nees([1.0, 0.0, 0.0], [2.0, 1.0, 2.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]), 2.0 / 3.0, rel_tol=1e-14)
    # batched, with a NaN row passing through
    poses = np.array([[1.0, 2.0, 0.5], [0.0, 0.0, 0.0]])
    covs = np.array([cov, [np.nan] * 6])
    out = cs.pose_nees(poses, covs, np.zeros((2, 3)))
    assert math.isclose(out[0], 5.25, rel_tol=1e-14) and np.isnan(out[1])
    assert np.array_equal(cs.pose_cov_matrix(cov), np.diag([4.0, 1.0, 0.25]))
