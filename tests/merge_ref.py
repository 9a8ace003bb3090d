"""NumPy references of aslam_merge_landmarks / aslam_select_duplicates (include/aslam_core.h).

  merge_joint      the rounds of 8 pairs, each jointly through chol(S), in binary64
  merge_seq_ld     one pair at a time in np.longdouble with closed-form 2x2 inverses
  merge_seq        the same pair-by-pair evaluation in binary64
  select_ref       the selector, operation by operation: bit for bit what the device writes
  fuse_sightings   the rule of the sighting records
  synthetic        the inputs of the tests: any SPD P is a valid joint covariance, so arbitrary pairs are a valid constraint
  bar              the bar a third evaluation order is held to, from the references' own spread

Pairs are (i, j) with i < j: landmark j is merged into landmark i and removed.  All references return (X, P) of the SURVIVORS, in order."""
import numpy as np

MERGE_ROUND = 8
EPS = 2.0 ** -52


def rows(l):
    return [3 + 2 * l, 4 + 2 * l]


def ordered(pairs):
    return sorted(((int(i), int(j)) for i, j in pairs), key=lambda p: p[1])


def drop(X, P, gone):
    keep = [0, 1, 2] + [r for l in range((len(X) - 3) // 2) if l not in gone for r in rows(l)]
    return X[keep], P[np.ix_(keep, keep)]


def merge_joint(X, P, pairs, noise=0.0, rounds=None):
    """rounds: apply the first `rounds` rounds only (the pairs of the others stay in the state)"""
    X, P = np.array(X, np.float64), np.array(P, np.float64)
    pairs = ordered(pairs)
    gone = set()
    for r, p0 in enumerate(range(0, len(pairs), MERGE_ROUND)):
        if rounds is not None and r >= rounds:
            break
        grp = pairs[p0:p0 + MERGE_ROUND]
        a = [q for i, _ in grp for q in rows(i)]
        c = [q for _, j in grp for q in rows(j)]
        Wt = P[a, :] - P[c, :]
        S = Wt[:, a] - Wt[:, c] + noise * np.eye(len(a))
        d = X[a] - X[c]
        Lc = np.linalg.cholesky(np.tril(S) + np.tril(S, -1).T)
        V = np.linalg.solve(Lc, Wt)
        y = np.linalg.solve(Lc, d)
        X = X - V.T @ y
        P = P - V.T @ V
        P = np.tril(P) + np.tril(P, -1).T
        gone |= {j for _, j in grp}
    return drop(X, P, gone)


def _seq(X, P, pairs, noise, dtype):
    X, P = np.array(X, dtype), np.array(P, dtype)
    noise = dtype(noise)
    gone = set()
    for i, j in ordered(pairs):
        a, c = rows(i), rows(j)
        W = P[:, a] - P[:, c]
        S = W[a, :] - W[c, :]
        s00, s11, s10 = S[0, 0] + noise, S[1, 1] + noise, (S[1, 0] + S[0, 1]) / dtype(2)
        det = s00 * s11 - s10 * s10
        Si = np.array([[s11, -s10], [-s10, s00]], dtype) / det
        d = X[a] - X[c]
        X = X - W @ (Si @ d)
        P = P - W @ Si @ W.T
        P = (P + P.T) / dtype(2)
        gone.add(j)
    return drop(X, P, gone)


def merge_seq_ld(X, P, pairs, noise=0.0):
    return _seq(X, P, pairs, noise, np.longdouble)


def merge_seq(X, P, pairs, noise=0.0):
    return _seq(X, P, pairs, noise, np.float64)


def select_ref(X, P, gate, max_dist):
    """into [L] i32 of one filter; binary64, each operation rounded on its own, lower-triangle entries only (aslam_core.h)"""
    X, P = np.asarray(X, np.float64), np.asarray(P, np.float64)
    L = (len(X) - 3) // 2
    gate, maxd2 = np.float64(gate), np.float64(max_dist) * np.float64(max_dist)
    partner = np.full(L, -1, np.int32)
    with np.errstate(all="ignore"):
        for j in range(1, L):
            i = np.arange(j)
            a0, a1, c0, c1 = 3 + 2 * i, 4 + 2 * i, 3 + 2 * j, 4 + 2 * j
            dx, dy = X[a0] - X[c0], X[a1] - X[c1]
            r2 = dx * dx + dy * dy
            s00 = ((P[a0, a0] + P[c0, c0]) - P[c0, a0]) - P[c0, a0]
            s11 = ((P[a1, a1] + P[c1, c1]) - P[c1, a1]) - P[c1, a1]
            s10 = ((P[a1, a0] + P[c1, c0]) - P[c1, a0]) - P[c0, a1]
            det = s00 * s11 - s10 * s10
            t1 = (s10 * dx) * dy
            num = (((s11 * dx) * dx) - (t1 + t1)) + ((s00 * dy) * dy)
            m = num / det
            ok = (r2 <= maxd2) & (s00 > 0) & (det > 0) & (m < gate)
            if ok.any():
                partner[j] = int(np.argmin(np.where(ok, m, np.inf)))  # (argmin: the first of equal minima, i.e. the smaller i)
                if not ok[partner[j]]:  # (every candidate at +inf cannot happen: m < gate <= inf is strict)
                    partner[j] = int(np.flatnonzero(ok)[0])
    into = np.full(L, -1, np.int32)
    for j in range(L):
        if partner[j] >= 0 and partner[partner[j]] == -1:
            into[j] = partner[j]
    return into


def pairs_of(into):
    return [(int(i), j) for j, i in enumerate(into) if i >= 0]


def fuse_sightings(seen, hits, clock, pairs):
    """records of the survivors after merging `pairs`: hits add up, the younger last_seen stays (age = clock - seen, unsigned 32-bit)"""
    seen, hits = np.array(seen, np.uint32), np.array(hits, np.uint32)
    clock = np.uint32(clock)
    gone = set()
    with np.errstate(over="ignore"):
        for i, j in ordered(pairs):
            hits[i] = hits[i] + hits[j]
            if np.uint32(clock - seen[j]) < np.uint32(clock - seen[i]):
                seen[i] = seen[j]
            gone.add(j)
    keep = [l for l in range(len(seen)) if l not in gone]
    return seen[keep], hits[keep]


def synthetic(N, pairs, ridge=0.01):
    """P = M M^T / N * 0.02 + ridge I, M standard normal from default_rng(N); X = 5 normal, each leaf's X its root's plus 0.05 normal"""
    rng = np.random.default_rng(N)
    M = rng.standard_normal((N, N))
    P = M @ M.T / N * 0.02 + ridge * np.eye(N)
    P = (P + P.T) / 2
    X = 5.0 * rng.standard_normal(N)
    for i, j in ordered(pairs):
        X[rows(j)] = X[rows(i)] + 0.05 * rng.standard_normal(2)
    return X, P


def crafted_states():
    """name -> (X, P, gate, max_dist, expected into): the selector's edge cases, shared by the host and the GPU test"""
    def state(points, var=0.01):
        n = 3 + 2 * len(points)
        X = np.concatenate([[0.5, -0.25, 0.1], np.asarray(points, np.float64).reshape(-1)])
        return X, var * np.eye(n)

    out = {}
    # a ~ b ~ c: m(a, b) = m(b, c) = 0.09 / 0.02 = 4.5, m(a, c) = 18: c's partner b is itself merged, so c waits
    X, P = state([[0.0, 0.0], [0.3, 0.0], [0.6, 0.0]])
    out["chain"] = (X, P, 5.99, 1.0, [-1, 0, -1])
    # landmark 2 half way between 0 and 1 (m = 0.0625 / 0.02 both, bit for bit); 0 and 1 are 12.5 apart
    X, P = state([[-0.25, 1.0], [0.25, 1.0], [0.0, 1.0]])
    out["tie"] = (X, P, 5.99, 1.0, [-1, -1, 0])
    # the same, with max_dist below the distance: nothing
    out["far"] = (X, P, 5.99, 0.2, [-1, -1, -1])
    X, P = state([[1.0, 2.0]])
    out["one-landmark"] = (X, P, 5.99, 1.0, [-1])
    X, P = state([])
    out["no-landmark"] = (X, P, 5.99, 1.0, [])
    # S = 0 exactly: the two landmarks have identical rows of P
    X, P = state([[1.0, 2.0], [1.0, 2.0]])
    P[5:7, 3:5] = P[3:5, 5:7] = 0.01 * np.eye(2)
    out["s-zero"] = (X, P, 1e300, 1.0, [-1, -1])
    # s00 > 0 but det S < 0 (a cross block no covariance has): not a candidate, whatever the gate
    X, P = state([[1.0, 2.0], [1.01, 2.0]])
    P[5:7, 3:5] = [[0.0, 0.02], [0.02, 0.0]]
    P[3:5, 5:7] = P[5:7, 3:5].T
    out["s-indefinite"] = (X, P, 1e300, 1.0, [-1, -1])
    return out


def spread_and_bar(X, P, pairs, noise=0.0):
    """(spread, bar, (Xj, Pj)): spread = the larger of joint-vs-long-double and sequential-vs-long-double (util.rel_err on X, util.cov_err on
    P) on this very input; bar = max(32 spread, 64 * 2^-52): sums of up to 16 products plus a 16 x 16 triangular solve in another order."""
    from util import cov_err, rel_err

    Xl, Pl = merge_seq_ld(X, P, pairs, noise)
    Xl, Pl = np.asarray(Xl, np.float64), np.asarray(Pl, np.float64)
    Xj, Pj = merge_joint(X, P, pairs, noise)
    Xs, Ps = merge_seq(X, P, pairs, noise)
    spread = max(rel_err(Xj, Xl), cov_err(Pj, Pl), rel_err(Xs, Xl), cov_err(Ps, Pl))
    return spread, max(32 * spread, 64 * EPS), (Xj, Pj)


def two_per_root(L, k):
    """k pairs, two leaves on every root: roots 0, 0, 1, 1, ..., leaves from the back"""
    return [(p // 2, L - 1 - p) for p in range(k)]


# the (N, pairs) cases the references were compared on; the first four are the shapes of the GPU test
def ref_cases():
    return [(7, pair_set(2, 1)), (17, pair_set(7, 3, True)), (37, pair_set(17, 8, True)), (47, pair_set(22, 9, True)),
            (163, two_per_root(80, 16)), (1027, pair_set(512, 8)), (1027, two_per_root(512, 40))]


def pair_set(L, k, two_leaves=False):
    """k pairs among L landmarks: roots from the front, leaves from the back (the last landmark is a leaf); landmark 6, whose columns 15 and 16
    straddle a 16-tile, is a leaf where L allows; with two_leaves the first root takes two."""
    leaves = list(range(L - 1, L - 1 - k, -1))
    if L > 6 + 1 and 6 not in leaves and 6 >= k:
        leaves[-1] = 6
    roots = list(range(k))
    if two_leaves and k >= 2:
        roots[1] = roots[0]
    assert max(roots) < min(leaves)
    return [(i, j) for i, j in zip(roots, leaves)]
