"""Reference for the large-state UKF chain (a helper of tests/test_ukf_large_ref_host.py, tests/test_gpu_ukf_large_shapes.py and
tests/manual/ukf_reference_spread.py, not a conftest).

chain_step() is oracle.np_oracle.NpFilter._slam_ukf with the update written the way csrc/ukf_large.h carries it out (DESIGN.md section 4,
"Negative central weight"): the central sigma point's weight w0 = (1 - N) / 3 is negative, so S is not a sum of squares; the chain factors

    S+ = sum_{i >= 1} w_i dz_i dz_i^T + R        (positive definite)           S = S+ - z z^T,  z = sqrt(-w0) dz_0

and takes S^-1 from the factor of S+ by Sherman-Morrison.  With L = chol(S+), W = Tc L^-T, q = L^-1 z, t = L^-1 (Z - Zpred), g = W q and
den = 1 - q.q:

    K (Z - Zpred) = W t + g (q.t) / den          K S K^T = W W^T + g g^T / den

den = 1 - z^T S+^-1 z = 1 / (1 + z^T S^-1 z) measures how close S is to singular; the as-coded oracle records the right-hand side as
NpFilter.sm_den.  recorded_den() collects that figure from every slam() of a block of code that builds its filters itself.
"""
import contextlib
import math

import numpy as np

from oracle.np_oracle import NpFilter, measurement, normalize_angle, state_transition, f32, UKF_STD_A, UKF_STD_YAW


def chain_step(f, vx, az, dt):
    """one slam() of the UKF `f` (an NpFilter("ukf")) in the chain's formulation, plain binary64; updates f.X and f.P, returns den"""
    N = f.N
    M = 2 * N + 5
    # ---- prediction: as NpFilter._slam_ukf (ukf.cpp:260-375), every binary32 rounding point kept
    Xaug = np.zeros(N + 2)
    Xaug[:N] = f.X
    Paug = np.zeros((N + 2, N + 2))
    Paug[:N, :N] = f.P
    Paug[N, N] = float(f32(UKF_STD_A * UKF_STD_A))
    Paug[N + 1, N + 1] = float(f32(UKF_STD_YAW * UKF_STD_YAW))
    L = np.linalg.cholesky(Paug)
    w = float(f32(np.sqrt(f32(f32(f.lam + f32(N)) + f32(2)))))
    Xsig = np.empty((N + 2, M))
    Xsig[:, 0] = Xaug
    Xsig[:, 1 : N + 3] = Xaug[:, None] + w * L
    Xsig[:, N + 3 :] = Xaug[:, None] - w * L
    Xp = np.empty((N, M))
    for i in range(M):
        col = state_transition(N, Xsig[:, i], vx, az, dt)
        col[2] = float(normalize_angle(col[2]))
        Xp[:, i] = col
    W = f.weights
    Xbar = Xp @ W
    D = Xp - Xbar[:, None]
    for i in range(M):
        D[2, i] = float(normalize_angle(D[2, i]))
    Pm = (D * W) @ D.T + f.Q
    Zs = np.empty((N, M))
    for i in range(M):
        Zs[:, i] = measurement(N, Xp[:, i])
    Zpred = Zs @ W
    f._wrap_even(Zpred)
    DZ = Zs - Zpred[:, None]
    for i in range(M):
        f._wrap_even(DZ[:, i])
    Tc = (D * W) @ DZ.T
    Zdiff = f.Z - Zpred
    f._wrap_even(Zdiff)
    # ---- update: the chain's (ukf_large.h: ukf_large_wabt, the stacked factorisation, ukf_large_gain, large_syrk, ukf_large_rank1)
    assert W[0] < 0.0
    Sp = (DZ[:, 1:] * W[1:]) @ DZ[:, 1:].T + f.R
    z = math.sqrt(-W[0]) * DZ[:, 0]
    Ls = np.linalg.cholesky(Sp)
    Wm = np.linalg.solve(Ls, Tc.T).T
    q = np.linalg.solve(Ls, z)
    t = np.linalg.solve(Ls, Zdiff)
    g = Wm @ q
    den = 1.0 - q @ q
    f.X = Xbar + Wm @ t + g * ((q @ t) / den)
    f.P = Pm - Wm @ Wm.T - np.outer(g, g) / den
    return float(den)


@contextlib.contextmanager
def recorded_den():
    """within the block, every NpFilter("ukf").slam() appends (N, sm_den) to the list this yields, in call order"""
    out = []
    slam = NpFilter.slam

    def tap(self, vx, az, dt):
        slam(self, vx, az, dt)
        if self.kind == "ukf":
            out.append((self.N, self.sm_den))

    NpFilter.slam = tap
    try:
        yield out
    finally:
        NpFilter.slam = slam
