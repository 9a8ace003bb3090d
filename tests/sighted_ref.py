"""Test-side reference for the sighted-only EKF update (aslam_sighted_update_enable), NumPy only.

    SightedFilter(kind, cap)        a sightings_ref.SightFilter whose slam() updates with the rows of the pose and of the landmarks sighted in the
                                    callback alone: M = {0, 1, 2} + {3 + 2k, 4 + 2k : k sighted},
                                        S = H_M P H_M^T + R_M,  K = P H_M^T S^-1,  X += K Y_M,  P = (I - K H_M) P
                                    predict, updateH, the wrapping and all bookkeeping are the oracle's.  `mask` is the mask of the last callback,
                                    `nis` / `logdet` are Y_M^T S_M^-1 Y_M and ln det S_M of it.
    info_form_update(P, H, R, Y, m) the same update in the information form the single-CU kernel uses (measurement coordinates, two inversions)
    limit_range_ref(trace, r, t0)   what awesomeslam_amd.trace.limit_range must return, written as plain loops

The mask comes from the hits increments of SightFilter's own tap of _update_z: landmark k is sighted iff the association walk gave it an
observation in this callback; entries a growth appends are 0 (a landmark promoted now was initialised from that very reading)."""
import copy

import numpy as np

from oracle.np_oracle import measurement, normalize_angle, state_transition
from sightings_ref import SightFilter


def rows_of(mask, N):
    """The row set M of a state of dimension N for a landmark mask [(N - 3) / 2]."""
    m = np.zeros(N, bool)
    m[:3] = True
    k = np.flatnonzero(np.asarray(mask)[: (N - 3) // 2])
    m[3 + 2 * k] = True
    m[4 + 2 * k] = True
    return m


class SightedFilter(SightFilter):
    sighted_only = True  # False: the oracle's update with every row (the mask is still kept)

    def initialize(self):
        super().initialize()
        self.mask = np.zeros(0, np.uint8)
        self.nis = float("nan")
        self.logdet = float("nan")

    def _update_z(self, *args):
        before = self.hits.copy()
        super()._update_z(*args)
        L0 = len(before)
        self.mask = np.zeros(len(self.hits), np.uint8)
        self.mask[:L0] = self.hits[:L0] != before  # (one increment per callback at most)

    def _slam_ekf(self, vx, az, dt):
        if not self.sighted_only:
            return super()._slam_ekf(vx, az, dt)
        N = self.N
        self.X = state_transition(N, self.X, vx, az, dt)
        self.X[2] = float(normalize_angle(self.X[2]))
        self.P = self.A @ self.P @ self.A.T + self.Q
        self._update_h()
        Y = self.Z - measurement(N, self.X)
        self._wrap_even(Y)
        M = rows_of(self.mask, N)
        H, R, Y = self.H[M], self.R[np.ix_(M, M)], Y[M]
        S = H @ self.P @ H.T + R
        Si = np.linalg.inv(S)
        K = self.P @ H.T @ Si
        self.X = self.X + K @ Y
        self.P = (self.I - K @ H) @ self.P
        self.nis = float(Y @ Si @ Y)
        self.logdet = float(np.linalg.slogdet(S)[1])


def info_form_update(P, H, R, Y, mask):
    """(X increment, new P) of the row-selected update by the information form: Pt = H P H^T, D = diag(1 / r_i on M, 0 elsewhere),
    Pt_new = (Pt^-1 + D)^-1, u = Pt_new (D Y); back through H^-1.  Exact in real arithmetic."""
    N = P.shape[0]
    M = rows_of(mask, N)
    D = np.where(M, 1.0 / np.diag(R), 0.0)
    Pt = H @ P @ H.T
    Ptn = np.linalg.inv(np.linalg.inv(Pt) + np.diag(D))
    Hi = np.linalg.inv(H)
    return Hi @ (Ptn @ (D * Y)), Hi @ Ptn @ Hi.T


def limit_range_ref(trace, r, t_from):
    """awesomeslam_amd.trace.limit_range on one Trajectory, as loops."""
    out = copy.copy(trace)
    out.obs = np.zeros_like(trace.obs)
    out.n_obs = np.zeros_like(trace.n_obs)
    for t in range(trace.T):
        k = 0
        for j in range(int(trace.n_obs[t])):
            if t < t_from or trace.obs[t, j, 0] <= np.float32(r):
                out.obs[t, k] = trace.obs[t, j]
                k += 1
        out.n_obs[t] = k
    return out
