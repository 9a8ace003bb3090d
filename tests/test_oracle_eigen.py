"""Compile-gated verbatim-Eigen check of the oracle.  `make -C oracle eigen` builds oracle/aslam_oracle.cpp a second
time with its matrix products, `inverse()` and `llt().matrixL()` evaluated by Eigen itself (the library the reference links:
ekf.cpp:297,300-301,309-310; ukf.cpp:280,378,391) -- only where <eigen3/Eigen/Dense> exists; elsewhere the test SKIPS.  The
reference's own text is held against the oracle without Eigen, over a header shim (tests/test_reference_parity.py, DESIGN.md
section 3); this test adds Eigen's own blocked kernels on a box that has them.  It replays the same seeded traces through both
builds in separate processes and compares state, covariance, dimensions and pose stream."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIGEN_LIB = os.path.join(ROOT, "oracle", "libaslam_oracle_eigen.so")

CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from awesomeslam_amd import trace as tg
from oracle.c_oracle import CFilter
kind, L, T, seed, out = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[6]
tr = tg.make_traces(L, T, B=1, seed=seed)
o = CFilter(kind, tg.dim_cap(L))
poses, dims = o.replay(tr[0])
X, Z, P = o.state()
np.savez(out, poses=poses, dims=dims, X=X, Z=Z, P=P)
"""


def replay(lib, kind, L, T, seed, tmp_path, tag):
    out = str(tmp_path / f"{tag}.npz")
    env = dict(os.environ)
    if lib:
        env["ASLAM_ORACLE_LIB"] = lib
    else:
        env.pop("ASLAM_ORACLE_LIB", None)
    subprocess.check_call([sys.executable, "-c", CHILD, ROOT, kind, str(L), str(T), str(seed), out], env=env)
    return np.load(out)


@pytest.mark.parametrize("kind,L,T", [("ekf", 8, 200), ("ekf", 24, 120), ("ukf", 8, 200), ("ukf", 13, 120)])
def test_restatement_against_eigen(kind, L, T, tmp_path):
    subprocess.call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "eigen"])
    if not os.path.exists(EIGEN_LIB):
        pytest.skip("no <eigen3/Eigen/Dense>: the Eigen-gated oracle build does not exist (tests/test_reference_parity.py pins the oracle without it)")
    a = replay(None, kind, L, T, 5, tmp_path, "plain")
    b = replay(EIGEN_LIB, kind, L, T, 5, tmp_path, "eigen")
    assert np.array_equal(a["dims"], b["dims"]) and np.array_equal(a["Z"], b["Z"])
    for k in ("poses", "X", "P"):
        err = np.abs(a[k] - b[k]).max() / max(np.abs(b[k]).max(), 1e-300)
        print(f"{kind} L={L} {k}: restatement vs Eigen {err:.2e}")
        assert err < 1e-9  # summation order differs (Eigen's blocked GEMM / LU), the algorithms do not
