"""Test-side reference for the sighting records (aslam_get_sightings / aslam_select_stale) and the forgetting policy on them, NumPy only.

    SightFilter(kind, cap)                     an oracle.np_oracle.NpFilter that also keeps (clock, last_seen, hits), by tapping _update_z
    stale(f, max_age)                          bool [L]: clock - last_seen > max_age in unsigned 32-bit arithmetic
    compact(f, drop)                           prune_ref.prune_npfilter and the records moved with their landmarks
    forget_run(f, trace, T, period, max_age)   the policy of Core.replay_forget on the oracle

The tap changes no line of the oracle.  NpFilter._update_z reads Z[0:3] only and writes Z(3 + 2k), Z(4 + 2k) exactly when it associates an
observation with landmark k, so: save Z[3:N], overwrite it with NaN, call the oracle, and the entries that are no longer NaN are this
callback's hits; the saved values go back into the rest.  Entries appended by a growth get (clock, 0)."""
import numpy as np

import prune_ref
from oracle.np_oracle import NpFilter

U32 = np.uint32
NEVER = 0xFFFFFFFF


class SightFilter(NpFilter):
    def initialize(self):
        super().initialize()
        self.clock = 0
        self.last_seen = np.zeros(0, U32)
        self.hits = np.zeros(0, U32)
        self.growth_refused = False  # (the oracle drops the landmarks silently: ASLAM_ST_GROWTH_REFUSED on the device)

    def _grow(self, new):
        n0 = self.N
        super()._grow(new)
        self.growth_refused = self.growth_refused or self.N == n0

    def _update_z(self, *args):
        n0 = self.N
        saved = self.Z[3:n0].copy()
        self.Z[3:n0] = np.nan
        super()._update_z(*args)
        body = self.Z[3:n0]  # (a view: a growth copies the old entries, NaN included, into the new vector first)
        hit = ~np.isnan(body[0::2])
        assert np.array_equal(hit, ~np.isnan(body[1::2]))
        rest = np.isnan(body)
        body[rest] = saved[rest]
        self.clock += 1
        self.last_seen[hit] = self.clock
        self.hits[hit] += 1
        grown = (self.N - n0) // 2
        self.last_seen = np.concatenate([self.last_seen, np.full(grown, self.clock, U32)])
        self.hits = np.concatenate([self.hits, np.zeros(grown, U32)])

    def sightings(self):
        return self.last_seen.copy(), self.hits.copy(), self.clock


def ages(f):
    with np.errstate(over="ignore"):
        return (U32(f.clock & NEVER) - f.last_seen.astype(U32)).astype(U32)


def stale(f, max_age):
    return ages(f) > U32(max_age)


def compact(f, drop):
    keep = np.ones(len(f.last_seen), bool)
    keep[list(drop)] = False
    prune_ref.prune_npfilter(f, drop)
    f.last_seen, f.hits = f.last_seen[keep], f.hits[keep]
    return f


def forget_run(f, trace, T, period, max_age):
    """-> poses [T, 3], dims [T], and per prune (dimension before it, landmarks removed, dimension after it)"""
    poses, dims, sched = [], [], []
    for t0 in range(0, T, period):
        t1 = min(T, t0 + period)
        p, d = prune_ref.step_from(f, trace, t0, t1)
        poses.append(p)
        dims.append(d)
        drop = np.flatnonzero(stale(f, max_age)).tolist()
        before = f.N
        compact(f, drop)
        sched.append((before, len(drop), f.N))
    return np.concatenate(poses), np.concatenate(dims), sched
