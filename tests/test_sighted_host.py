"""The sighted-only EKF update without a GPU: the ABI (four new functions declared and exported, version untouched), the model of
tests/sighted_ref.py against the oracle where they must agree and where they must not, the information form the single-CU kernel evaluates
against the row-selected update, and awesomeslam_amd.trace.limit_range."""
import ctypes
import os
import re

import numpy as np
import pytest

from awesomeslam_amd import core
from awesomeslam_amd import trace as tg
from oracle.np_oracle import NpFilter, measurement, normalize_angle, state_transition
from sighted_ref import SightedFilter, info_form_update, limit_range_ref
from util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CORE = ("aslam_sighted_update_enable", "aslam_get_sighted", "aslam_ekf_step_sighted", "aslam_ekf_step_batch_sighted")
# the three limited-range traces of INTEGRATION.md section 2l: (L, T, sensor_range, layout), seed 3
TABLE = ((12, 300, 5.0, "ring"), (24, 400, 6.0, "ring"), (40, 300, 14.0, "field"))


def header(path):
    txt = open(os.path.join(ROOT, path)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"//[^\n]*", "", txt)


def table_trace(i):
    L, T, r, layout = TABLE[i]
    return tg.make_traces(L, T, seed=3, sensor_range=r, layout=layout)[0]


def test_header_and_binding_declare_and_export_the_new_functions(built):
    h = header("include/aslam_core.h")
    names = set(re.findall(r"\b(aslam_[A-Za-z_0-9]+)\s*\(", h))
    lib = ctypes.CDLL(os.path.join(ROOT, "awesomeslam_amd", "csrc", "libaslam_core.so"))
    for n in NEW_CORE:
        assert n in names and n in core.CORE_SYMBOLS and hasattr(lib, n), n
    assert re.search(r"#define\s+ASLAM_ABI_VERSION\s+1\b", h) and core.core_lib().aslam_abi_version() == 1
    # the seams are the existing ones with one more argument (the batch form: and its row stride) behind Z
    for name, plain, extra in (("aslam_ekf_step_sighted", "aslam_ekf_step", ["sighted"]),
                               ("aslam_ekf_step_batch_sighted", "aslam_ekf_step_batch", ["sighted", "ld"])):
        arg = lambda f: [a.split()[-1].lstrip("*") for a in re.search(r"int\s+%s\s*\(([^)]*)\)" % f, h).group(1).split(",")]  # noqa: E731
        a, b = arg(name), arg(plain)
        k = b.index("ldz" if "batch" in plain else "Z") + 1
        assert a == b[:k] + extra + b[k:], (a, b)
    assert re.search(r"const\s+uint8_t\s*\*\s*sighted", h)
    assert lib.aslam_sighted_update_enable(None, 1) == -1 and lib.aslam_get_sighted(None, 0, None, 0, None) == -1


def test_model_with_everything_sighted_is_the_oracle():
    """unlimited range.  Through the promotions the two differ by design (a landmark promoted in a callback is not sighted in it, the oracle
    uses its row at once), so the model runs them with the oracle's update; past them every landmark is sighted in every callback and the
    row selection selects everything"""
    import prune_ref

    tr = tg.make_traces(12, 120, seed=3)[0]
    m, o = SightedFilter("ekf", tg.dim_cap(12)), NpFilter("ekf", tg.dim_cap(12))
    m.sighted_only = False
    t0 = tr.warmup + 1
    prune_ref.step_from(m, tr, 0, t0)
    prune_ref.step_from(o, tr, 0, t0)
    assert m.N == o.N == tg.full_dim(12) and np.array_equal(m.X, o.X) and np.array_equal(m.P, o.P)
    m.sighted_only = True
    pm, po = np.zeros((tr.T - t0, 3)), np.zeros((tr.T - t0, 3))
    for t in range(t0, tr.T):
        pm[t - t0] = prune_ref.step_from(m, tr, t, t + 1)[0][0]
        po[t - t0] = prune_ref.step_from(o, tr, t, t + 1)[0][0]
        assert m.mask.all() and m.N == o.N
    errs = rel_err(m.X, o.X), rel_err(m.P, o.P), rel_err(pm, po)
    print("everything sighted, model against the oracle: X %.2e P %.2e poses %.2e" % errs)
    assert max(errs) < 1e-12 and np.array_equal(m.Z, o.Z)


class Probe(SightedFilter):
    """compares every callback's row-selected update with the information form on the same predicted state"""

    worst = 0.0
    cond = 0.0

    def _slam_ekf(self, vx, az, dt):
        X0, P0 = self.X.copy(), self.P.copy()
        super()._slam_ekf(vx, az, dt)
        N = self.N
        Xp = state_transition(N, X0, vx, az, dt)
        Xp[2] = float(normalize_angle(Xp[2]))
        Pp = self.A @ P0 @ self.A.T + self.Q
        Y = self.Z - measurement(N, Xp)
        self._wrap_even(Y)
        dX, Pn = info_form_update(Pp, self.H, self.R, Y, self.mask)
        self.worst = max(self.worst, rel_err(Xp + dX, self.X), rel_err(Pn, self.P))
        self.cond = max(self.cond, float(np.linalg.cond(self.H @ Pp @ self.H.T)))


@pytest.mark.parametrize("i", range(len(TABLE)))
def test_information_form_is_the_row_selected_update(i):
    tr = table_trace(i)
    m = Probe("ekf", tg.dim_cap(TABLE[i][0]))
    m.replay(tr)
    print(f"trace {TABLE[i]}: information form against the row-selected update {m.worst:.2e}, cond(Pt) <= {m.cond:.2e}")
    assert 0.0 < m.worst < 1e-10


def test_sighted_only_stays_on_the_truth_where_the_stale_update_leaves_it():
    tr = table_trace(0)
    cap = tg.dim_cap(TABLE[0][0])
    pm, _ = SightedFilter("ekf", cap).replay(tr)
    po, _ = NpFilter("ekf", cap).replay(tr)
    w = tr.warmup
    em = np.hypot(*(pm[w:, :2] - tr.truth[w:, :2]).T).max()
    eo = np.hypot(*(po[w:, :2] - tr.truth[w:, :2]).T).max()
    print(f"worst pose error against the truth: sighted-only {em:.3f} m, stale {eo:.3f} m")
    assert em < 0.1 and eo > 1.0


def test_limit_range_compacts_and_round_trips(tmp_path):
    full = tg.make_traces(12, 60, B=2, seed=3, layout="ring")
    lim = tg.limit_range(full, 5.0, 45)
    assert lim.max_obs == full.max_obs and np.array_equal(lim.odom, full.odom) and lim.obs is not full.obs
    assert np.array_equal(lim.obs[:, :45], full.obs[:, :45]) and (lim.n_obs[:, 45:] < full.n_obs[:, 45:]).any()
    for b in range(2):
        ref = limit_range_ref(full[b], 5.0, 45)
        one = tg.limit_range(full[b], 5.0, 45)
        for got in (lim[b], one):
            assert np.array_equal(got.obs, ref.obs) and np.array_equal(got.n_obs, ref.n_obs)
    assert (lim.obs[:, 45:, :, 0] <= 5.0).all()
    p = str(tmp_path / "lim.asltrc")
    lim.to_file(p)
    back = tg.Trace.from_file(p)
    for k in ("odom", "dt", "obs_new", "n_obs", "obs", "landmarks", "truth"):
        assert np.array_equal(getattr(back, k), getattr(lim, k)), k
    assert back.warmup == lim.warmup
