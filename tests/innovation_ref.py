"""Reference for the innovation statistics (a helper of tests/test_innovation_host.py and tests/test_gpu_innovation.py, not a conftest).

StatsFilter is oracle.np_oracle.NpFilter with two taps and no arithmetic of its own: it records the argument of the step's single
np.linalg.inv call (that is S: ekf.cpp:300, ukf.cpp:378) and the vector of the step's last _wrap_even call (Y of the EKF, Zdiff of the
UKF).  From those:  nis = y . solve(S, y),  logdet = slogdet(S)[1].
"""
import numpy as np

from oracle.np_oracle import NpFilter


class StatsFilter(NpFilter):
    def __init__(self, kind, max_landmark_count=30):
        self.S = self.y = self.dz0 = None
        self._wrapped = []
        self.nis = self.logdet = float("nan")
        self.sign = 0.0
        super().__init__(kind, max_landmark_count)

    def _wrap_even(self, v):
        super()._wrap_even(v)
        self._wrapped.append(v)  # (wrapped in place; the last one of a step is the innovation)

    def slam(self, vx, az, dt):
        seen = []
        self._wrapped = []
        inv = np.linalg.inv

        def tap(a):
            seen.append(np.array(a, dtype=np.float64))
            return inv(a)

        np.linalg.inv = tap
        try:
            super().slam(vx, az, dt)
        finally:
            np.linalg.inv = inv
        assert len(seen) == 1, "a step inverts exactly one matrix: S"
        self.S, self.y = seen[0], np.array(self._wrapped[-1], dtype=np.float64)
        # UKF (ukf.cpp:326-339): Zpred is wrapped first, then the columns of Zsig - Zpred in order, then Zdiff -- the second one is the central column
        self.dz0 = np.array(self._wrapped[1], dtype=np.float64) if self.kind == "ukf" else None
        assert self.y.shape == (self.N,) and self.S.shape == (self.N, self.N)
        self.nis = float(self.y @ np.linalg.solve(self.S, self.y))
        self.sign, self.logdet = (float(v) for v in np.linalg.slogdet(self.S))

    def pose_cov(self):
        P = self.P
        return np.array([P[0, 0], P[1, 0], P[1, 1], P[2, 0], P[2, 1], P[2, 2]])

    def replay_stats(self, trace, T=None):
        """NpFilter.replay with the statistics of every callback: poses [T,3], dims [T], nis [T], logdet [T], pose_cov [T,6], ran [T] (bool:
        odom_msg returned 1); NaN where slam() did not run"""
        T = trace.T if T is None else T
        poses, dims = np.zeros((T, 3)), np.zeros(T, dtype=np.int32)
        nis, logdet, pcov = np.full(T, np.nan), np.full(T, np.nan), np.full((T, 6), np.nan)
        ran = np.zeros(T, dtype=bool)
        for t in range(T):
            if trace.obs_new[t]:
                k = int(trace.n_obs[t])
                self.sensor_msg(trace.obs[t, :k, 0], trace.obs[t, :k, 1])
            o = trace.odom[t]
            if self.odom_msg(o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], trace.dt[t]):
                ran[t] = True
                poses[t] = self.X[:3]
                nis[t], logdet[t], pcov[t] = self.nis, self.logdet, self.pose_cov()
            dims[t] = self.N
        return poses, dims, nis, logdet, pcov, ran


def sherman_morrison_stats(S_plus, z, y):
    """The statistics of S = S_plus - z z^T from the Cholesky factor of S_plus alone, as the UKF kernels form them:
        q = L^-1 z, t = L^-1 y:   y^T S^-1 y = t.t + (q.t)^2 / (1 - q.q),   det S = det S_plus (1 - q.q)
    returns (nis, sign of det S, ln |det S|)"""
    L = np.linalg.cholesky(S_plus)
    q, t = np.linalg.solve(L, z), np.linalg.solve(L, y)
    den = 1.0 - q @ q
    return float(t @ t + (q @ t) ** 2 / den), float(np.sign(den)), float(2.0 * np.log(np.diag(L)).sum() + np.log(abs(den)))
