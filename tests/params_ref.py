"""Reference for the run-time parameters (a helper of tests/test_params_host.py and tests/test_gpu_params.py, not a conftest).

ParamFilter is innovation_ref.StatsFilter -- oracle.np_oracle.NpFilter with the two taps -- run with a parameter dict instead of the reference's
constants, without a line of oracle/ changed: the matrices the reference builds from constants (P at initialize(), the diagonals of R and Q, the
new P diagonal of a growth) are rewritten right after the oracle has built them, and the three constants the oracle reads while it runs
(MIN_DIST_THRESH, MIN_LANDMARK_OCC, UKF_STD_A) are swapped in np_oracle's module globals for the duration of every call and put back after it.

The parameter sets of the tests live here too (SETS), with the defaults.
"""
import contextlib

import numpy as np

from innovation_ref import StatsFilter
from oracle import np_oracle

f32 = np.float32

# aslam_params_default: the widened binary32 constants of config.h
DEFAULTS = dict(r_xy=float(f32(0.2)), r_yaw=float(f32(0.2)), r_range=float(f32(0.2)), r_bearing=float(f32(0.2)), q_xy=float(f32(0.001)),
                q_yaw=float(f32(0.001)), p0_pose=float(f32(0.001)), p0_landmark=1.0, var_a=float(f32(f32(0.2) * f32(0.2))),
                assoc_dist=0.5, promote_count=10)
FIELDS = tuple(DEFAULTS)


def var_of(s):
    """var_a for a binary32 standard deviation s: the binary32 product the reference forms (ukf.cpp:276)"""
    return float(f32(f32(s) * f32(s)))


SETS = {
    "default": {},
    "A": dict(r_xy=.05, r_yaw=.02, r_range=.1, r_bearing=.05, q_xy=.002, q_yaw=.0005, p0_pose=.002, p0_landmark=.5, var_a=var_of(.3), assoc_dist=.6,
              promote_count=6),
    "B": dict(r_xy=.4, r_yaw=.3, r_range=.3, r_bearing=.1, q_xy=.0005, q_yaw=.002, p0_pose=.0005, p0_landmark=2.0, var_a=var_of(.1), assoc_dist=.4,
              promote_count=14),
    "C": dict(r_xy=.3, r_yaw=.25, r_range=.3, r_bearing=.25, q_xy=.0015, q_yaw=.0008, p0_landmark=.8, promote_count=8),
    "D": dict(assoc_dist=.1),
}


def full(params):
    """the defaults with `params` on top; assoc_dist as the binary32 value the structure holds"""
    assert set(params) <= set(DEFAULTS), set(params) - set(DEFAULTS)
    p = dict(DEFAULTS, **params)
    p["assoc_dist"] = float(f32(p["assoc_dist"]))
    p["promote_count"] = int(p["promote_count"])
    return p


def std_a_of(var_a):
    """the binary32 s with f32(s * s) == var_a (the oracle squares UKF_STD_A itself)"""
    s = f32(np.sqrt(var_a))
    for c in (s, np.nextafter(s, f32(0)), np.nextafter(s, f32(1))):
        if float(f32(c * c)) == var_a:
            return c
    raise ValueError(f"var_a = {var_a!r} is not the binary32 square of a binary32 value")


def r_diag(p, N):
    r = np.empty(N)
    r[:2], r[2] = p["r_xy"], p["r_yaw"]
    r[3::2], r[4::2] = p["r_range"], p["r_bearing"]
    return r


class ParamFilter(StatsFilter):
    def __init__(self, kind, max_landmark_count=30, params=None):
        self.prm = full(params or {})
        self._std_a = std_a_of(self.prm["var_a"])
        super().__init__(kind, max_landmark_count)

    @contextlib.contextmanager
    def _constants(self):
        keep = np_oracle.MIN_DIST_THRESH, np_oracle.MIN_LANDMARK_OCC, np_oracle.UKF_STD_A
        np_oracle.MIN_DIST_THRESH, np_oracle.MIN_LANDMARK_OCC, np_oracle.UKF_STD_A = f32(self.prm["assoc_dist"]), self.prm["promote_count"], self._std_a
        try:
            yield
        finally:
            np_oracle.MIN_DIST_THRESH, np_oracle.MIN_LANDMARK_OCC, np_oracle.UKF_STD_A = keep

    def _noise(self):
        N = self.N
        self.R = np.diag(r_diag(self.prm, N))
        self.Q = np.zeros((N, N))
        self.Q[0, 0] = self.Q[1, 1] = self.prm["q_xy"]
        self.Q[2, 2] = self.prm["q_yaw"]

    def initialize(self):
        super().initialize()
        self.P = np.eye(self.N) * self.prm["p0_pose"]
        self._noise()

    def _grow(self, new):
        n0 = self.N
        super()._grow(new)
        if self.N > n0:
            i = np.arange(n0, self.N)
            self.P[i, i] = self.prm["p0_landmark"]
            self._noise()

    def set_state(self, N, X, Z, P, a00=1.0, a10=0.0):
        super().set_state(N, X, Z, P, a00, a10)
        self._noise()

    def odom_msg(self, *a):
        with self._constants():
            return super().odom_msg(*a)

    def slam(self, vx, az, dt):
        with self._constants():
            super().slam(vx, az, dt)

    def grow(self, new):
        """the matrix part of updateNewLandmark for [(range, bearing), ...] (aslam_grow)"""
        with self._constants():
            self._grow(new)
