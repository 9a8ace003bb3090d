"""The formulation of the large-state UKF chain against the as-coded oracle, in NumPy binary64 (no GPU).

tests/test_gpu_ukf_large.py claims in its docstring that the chain's update (Cholesky of S without the i = 0 term, forward-only
Sherman-Morrison: tests/ukf_large_ref.py::chain_step) agrees with the reference's K = Tc S^-1 on that file's synthetic states; here it is
asserted.  Bar 1e-12; measured here: first step <= 5.8e-15, second step (each side from its own first) <= 1.7e-13, both worst at n = 255."""
import numpy as np
import pytest

from oracle.np_oracle import NpFilter
from test_gpu_ukf_large import STEPS, synth
from ukf_large_ref import chain_step, recorded_den
from util import cov_err, rel_err

FORMULATION_TOL = 1e-12
DEN_TOL = 1e-10


@pytest.mark.parametrize("n", [5, 31, 145, 255])
def test_chain_formulation_agrees_with_the_oracle(n):
    X, Z, P = synth(n, n)
    ref, chain = NpFilter("ukf", n + 1), NpFilter("ukf", n + 1)
    ref.set_state(n, X, Z, P)
    chain.set_state(n, X, Z, P)
    for s, (vx, az, dt) in enumerate(STEPS[:2]):  # an arc, then the straight-line branch
        ref.slam(vx, az, dt)
        den = chain_step(chain, vx, az, dt)
        assert np.isfinite(ref.P).all() and np.linalg.eigvalsh((ref.P + ref.P.T) / 2).min() > 0, (n, s)
        ex, ep = rel_err(chain.X, ref.X), cov_err(chain.P, ref.P)
        print(f"chain formulation n={n} step {s}: rel err X {ex:.2e} P {ep:.2e}; den {den:.6f}, as coded {ref.sm_den:.6f}")
        assert ex < FORMULATION_TOL and ep < FORMULATION_TOL, (n, s, ex, ep)
        # 1 - z^T S+^-1 z = 1 / (1 + z^T S^-1 z), the right-hand side from the S the oracle inverts
        assert 0.0 < den <= 1.0 and abs(den - ref.sm_den) < DEN_TOL, (n, s, den, ref.sm_den)


def test_recorded_den_taps_every_step_and_restores():
    X, Z, P = synth(5, 5)
    slam = NpFilter.slam
    with recorded_den() as dens:
        f = NpFilter("ukf", 6)
        f.set_state(5, X, Z, P)
        f.slam(*STEPS[0])
        f.slam(*STEPS[1])
        e = NpFilter("ekf", 6)
        e.set_state(5, X, Z, P)
        e.slam(*STEPS[0])
    assert NpFilter.slam is slam
    assert [n for n, _ in dens] == [5, 5] and dens[1][1] == f.sm_den and all(0.0 < d <= 1.0 for _, d in dens)
