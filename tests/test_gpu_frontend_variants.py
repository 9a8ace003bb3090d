"""-m gpu: every launchable flag combination of a front-end family -- statistics x sighted-only update x replay gate for the EKF (single-CU and
the fp64 large chain), statistics x gate for the UKF -- selects the kernel that computes what the combination means.

For each combination, on the cases of tests/gated_ref.py:
  * aslam_replay_stats and aslam_replay from the same start give bit-equal pose and dimension streams and bit-equal final X, Z, P (what
    test_gpu_innovation.py::test_unused_means_unchanged asserts for the plain kernels);
  * the streams and the final state match the NumPy model of the combination -- GatedFilter, GatedSightedFilter (gate 0: the ungated rule of
    the very same classes) -- at the bars of test_gpu_gated_replay.py: util.REL_TOL with cov_err for X, P and the poses, Z and the dimensions exact.
Every model run and every plain replay is computed once and shared."""
import functools

import numpy as np
import pytest

import gated_ref
import prune_ref
from gated_ref import GATE, GatedFilter, GatedSightedFilter
from test_gpu_gated_replay import make
from test_gpu_large import chol_mode
from test_gpu_sighted import as_trace
from test_gpu_snapshot import run
from util import REL_TOL, cov_err, rel_err

pytestmark = pytest.mark.gpu

FAMILIES = ["ekf-12", "ukf-12", "ekf-96-large"]  # single-CU EKF, single-CU UKF, the fp64 large chain at dim_cap(96)
COMBOS = [(name, stats, sighted, gated) for name in FAMILIES for sighted in ((False, True) if name.startswith("ekf") else (False,))
          for gated in (False, True) for stats in (False, True)]


@functools.lru_cache(maxsize=None)
def model(name, sighted, gated):
    """(final filter, poses, dims) of the NumPy model of one combination; leave it unchanged"""
    if gated and not sighted:
        f, poses, dims, _ = gated_ref.run_case(name)
        return f, poses, dims
    kind, tr, cap, params = gated_ref.case_inputs(name)
    f = (GatedSightedFilter if sighted else GatedFilter)(kind, cap, params, gate=GATE if gated else 0.0)
    poses, dims = prune_ref.step_from(f, tr, 0, tr.T)
    return f, poses, dims


def launch(name, sighted, gated, stats):
    """one context, one launch over the whole trace: (poses [T, 3], dims [T], X, Z, P, kernel name)"""
    import torch

    kind, tr, cap, params = gated_ref.case_inputs(name)
    T = tr.T
    core = make(kind, as_trace([tr]), cap, gate=GATE if gated else None, params=params)
    if sighted:
        core.sighted_only()
    kname = core.kernel_info()["name"]
    if stats:
        # 7.0 everywhere: a launch that picked an instantiation without statistics would leave it there
        nis, logdet = (torch.full((1, T), 7.0, dtype=torch.float64, device="cuda") for _ in range(2))
        pcov = torch.full((1, T, 6), 7.0, dtype=torch.float64, device="cuda")
        poses = torch.zeros((1, T, 3), dtype=torch.float64, device="cuda")
        dims = torch.zeros((1, T), dtype=torch.int32, device="cuda")
        core.replay_stats(0, T, poses.data_ptr(), dims.data_ptr(), nis.data_ptr(), logdet.data_ptr(), pcov.data_ptr())
        torch.cuda.synchronize()
        p, d = poses.cpu().numpy(), dims.cpu().numpy()
        n_, l_, c_ = nis.cpu().numpy()[0], logdet.cpu().numpy()[0], pcov.cpu().numpy()[0]
        ran = ~np.isnan(c_).any(axis=1)  # (a callback without slam() writes NaN)
        assert ran.sum() > T // 2 and np.isfinite(n_[ran]).all() and np.isfinite(l_[ran]).all()
        assert (n_ != 7.0).all() and (l_ != 7.0).all() and (c_ != 7.0).all()  # every entry was written: the STATS instantiation ran
        assert (n_[ran] >= 0.0).all() and (c_[ran][:, [0, 2, 5]] > 0.0).all()  # y^T S^-1 y and the pose variances
    else:
        p, d = run(core, 0, T)
    out = (p[0], d[0]) + core.state(0) + (kname,)
    assert core.status(0) == 0
    core.close()
    return out


@functools.lru_cache(maxsize=None)
def plain_replay(name, sighted, gated):
    return launch(name, sighted, gated, False)


@pytest.mark.parametrize("name,stats,sighted,gated", COMBOS)
def test_every_flag_combination(name, stats, sighted, gated, built, monkeypatch):
    if "large" in name:
        chol_mode("f64", monkeypatch)
    base = plain_replay(name, sighted, gated)
    got = launch(name, sighted, gated, True) if stats else base
    kname = got[5]  # (of the replay seam without statistics: what kernel_info reports)
    if "small_kernel" in kname:  # <NT, MODE, STATS, SIGHTED, GATED> (EKF) / <NT, MODE, STATS, GATED> (UKF), trailing defaults left out
        args = (kname[kname.index("<") + 1:-1].split(",")[2:] + ["false"] * 3)[:3]
        named = (args[1] == "true", args[2] == "true") if name.startswith("ekf") else (False, args[1] == "true")
    else:
        named = ("sighted" in kname, "gated" in kname)
    assert named == (sighted, gated), kname
    for a, b in zip(got[:5], base[:5]):  # replay_stats against replay: bit for bit
        assert np.array_equal(a, b), (name, stats, sighted, gated)
    f, poses_m, dims_m = model(name, sighted, gated)
    poses, dims, X, Z, P = got[:5]
    e = rel_err(poses, poses_m), rel_err(X, f.X), cov_err(P, f.P)
    print(f"{name} stats={stats} sighted={sighted} gated={gated} n={f.N} ({kname}): rel err pose {e[0]:.2e} X {e[1]:.2e} P {e[2]:.2e}")
    assert np.array_equal(dims, dims_m) and np.array_equal(Z, f.Z) and max(e) < REL_TOL
