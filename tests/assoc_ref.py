"""NumPy reference of aslam_gate_observations (include/aslam_core.h): the Mahalanobis gate of every observation against every landmark.

  landmark_part    rh, bh, s00, s10, s11, det and the validity of every landmark of one filter (the 5 x 5 form)
  dense_S          S = H P H^T with the dense 2 x n Jacobian: what the 5 x 5 form is a shortcut of
  gate_matrix      m [n_obs, L]: +inf where the landmark is invalid or m is NaN
  gate_ref         (assoc, mdist) of one filter
  margins          how far the decisions are from flipping: best-vs-gate and second-best-vs-best, relative
  observations     the observations of the GPU test's shapes; crafted(): the edge cases, shared by the host and the GPU test
  err_and_bar      the device's mdist against the long-double reference, and the bar from the references' own spread

Every function takes `dtype` (np.float64 or np.longdouble) and does all arithmetic in it; 2 pi is the binary64 constant in both."""
import numpy as np

EPS = 2.0 ** -52
GATE = 9.21  # the 99 % point of chi-square with 2 degrees of freedom
R_DEFAULT = float(np.float32(0.2))  # r_range = r_bearing of the default table (aslam_core.h)


def ieee_remainder(x, y):
    """x - n y with n = x / y rounded to the nearest integer, ties to even: exact, through fmod (np.remainder is the floored modulus)"""
    with np.errstate(all="ignore"):
        r = np.fmod(x, y)
        half = y / type(y)(2)
        odd = np.fmod(np.trunc(x / y), 2) != 0
        over = (np.abs(r) > half) | ((np.abs(r) == half) & odd)
        return np.where(over, r - np.copysign(y, r), r)


def landmark_part(X, P, r_range, r_bearing, dtype=np.float64):
    """(rh, bh, s00, s10, s11, det, valid), each [L]; only lower-triangle entries of P are read"""
    X, P = np.asarray(X, dtype), np.asarray(P, dtype)
    L = (len(X) - 3) // 2
    out = [np.zeros(L, dtype) for _ in range(6)]
    valid = np.zeros(L, bool)
    Pl = np.tril(P) + np.tril(P, -1).T
    with np.errstate(all="ignore"):
        for k in range(L):
            a0, a1 = 3 + 2 * k, 4 + 2 * k
            dx, dy = X[a0] - X[0], X[a1] - X[1]
            q = dx * dx + dy * dy
            rh = np.sqrt(q)
            bh = np.arctan2(dy, dx) - X[2]
            H = np.array([[-dx / rh, -dy / rh, dtype(0), dx / rh, dy / rh], [dy / q, -dx / q, dtype(-1), -dy / q, dx / q]], dtype)
            idx = [0, 1, 2, a0, a1]
            S = H @ Pl[np.ix_(idx, idx)] @ H.T
            s00, s11, s10 = S[0, 0] + dtype(r_range), S[1, 1] + dtype(r_bearing), S[1, 0]
            det = s00 * s11 - s10 * s10
            for o, v in zip(out, (rh, bh, s00, s10, s11, det)):
                o[k] = v
            valid[k] = bool(q > 0) and bool(s00 > 0) and bool(det > 0)
    return (*out, valid)


def dense_S(X, P, k, dtype=np.float64):
    """H (2 x n) P H^T of landmark k, and the sum of |h| |p| |h| the rounding of either form is bounded by"""
    X, P = np.asarray(X, dtype), np.asarray(P, dtype)
    n = len(X)
    a0, a1 = 3 + 2 * k, 4 + 2 * k
    dx, dy = X[a0] - X[0], X[a1] - X[1]
    q = dx * dx + dy * dy
    rh = np.sqrt(q)
    H = np.zeros((2, n), dtype)
    H[0, [0, 1, a0, a1]] = [-dx / rh, -dy / rh, dx / rh, dy / rh]
    H[1, [0, 1, 2, a0, a1]] = [dy / q, -dx / q, -1, -dy / q, dx / q]
    return H @ P @ H.T, np.abs(H) @ np.abs(P) @ np.abs(H).T


def gate_matrix(X, P, obs, r_range=R_DEFAULT, r_bearing=R_DEFAULT, dtype=np.float64):
    """m [n_obs, L] in `dtype`; +inf where the landmark is invalid or m is NaN"""
    rh, bh, s00, s10, s11, det, valid = landmark_part(X, P, r_range, r_bearing, dtype)
    obs = np.asarray(obs, np.float32).reshape(-1, 2)
    r, beta = obs[:, 0].astype(dtype)[:, None], obs[:, 1].astype(dtype)[:, None]
    two_pi = dtype(2.0 * np.pi)
    with np.errstate(all="ignore"):
        v0 = r - rh[None, :]
        v1 = ieee_remainder(beta - bh[None, :], two_pi)
        m = (s11 * v0 * v0 - dtype(2) * s10 * v0 * v1 + s00 * v1 * v1) / det
    return np.where(valid[None, :] & ~np.isnan(m), m, dtype(np.inf))


def gate_ref(X, P, obs, r_range=R_DEFAULT, r_bearing=R_DEFAULT, gate=GATE, dtype=np.float64):
    """(assoc [n_obs] int32, mdist [n_obs] dtype): the landmark of smallest m if m < gate, else -1 (ties to the smaller index); the smallest m"""
    M = gate_matrix(X, P, obs, r_range, r_bearing, dtype)
    n_obs = M.shape[0]
    if M.shape[1] == 0:
        return np.full(n_obs, -1, np.int32), np.full(n_obs, np.inf, dtype)
    k = np.argmin(M, axis=1)  # (argmin: the first of equal minima)
    mdist = M[np.arange(n_obs), k]
    return np.where(mdist < dtype(gate), k, -1).astype(np.int32), mdist


def margins(X, P, obs, r_range=R_DEFAULT, r_bearing=R_DEFAULT, gate=GATE):
    """(gate margin, second-best margin) over the observations, from the long-double reference: min |best - gate| / gate over the finite best m,
    and min (second - best) / max(best, 1) -- the measure mdist is compared in -- over the observations with a finite second-best; +inf where
    there is none"""
    M = gate_matrix(X, P, obs, r_range, r_bearing, np.longdouble)
    g, s = np.inf, np.inf
    for row in M:
        srt = np.sort(row)
        if len(srt) >= 1 and np.isfinite(srt[0]) and np.isfinite(gate):
            g = min(g, float(abs(srt[0] - gate) / gate))
        if len(srt) >= 2 and np.isfinite(srt[1]):
            s = min(s, float((srt[1] - srt[0]) / max(srt[0], 1)))
    return g, s


def observations(X, n_obs, seed):
    """[n_obs, 2] float32 from default_rng(seed): three of four a landmark's predicted reading plus 0.3 normal in each component and a whole
    number of turns, the fourth anywhere"""
    rng = np.random.default_rng(seed)
    L = (len(X) - 3) // 2
    out = np.zeros((n_obs, 2), np.float32)
    for j in range(n_obs):
        if j % 4 != 3 and L > 0:
            k = int(rng.integers(L))
            dx, dy = X[3 + 2 * k] - X[0], X[4 + 2 * k] - X[1]
            r = np.hypot(dx, dy) + 0.3 * rng.normal()
            b = np.arctan2(dy, dx) - X[2] + 0.3 * rng.normal() + 2 * np.pi * rng.integers(-1, 2)
        else:
            r, b = rng.uniform(0.5, 30), rng.uniform(-3.1, 3.1)
        out[j] = (r, b)
    return out


def err_of(m_dev, m_ld):
    """max |m_dev - m_ld| / max(m_ld, 1) over the finite entries; where the reference is +inf the other side must be +inf too (else inf)"""
    m_dev, m_ld = np.asarray(m_dev, np.longdouble), np.asarray(m_ld, np.longdouble)
    fin = np.isfinite(m_ld)
    if not np.array_equal(np.isposinf(m_dev), ~fin):
        return np.inf
    if not fin.any():
        return 0.0
    return float((np.abs(m_dev[fin] - m_ld[fin]) / np.maximum(m_ld[fin], 1)).max())


def err_and_bar(m_dev, X, P, obs, r_range=R_DEFAULT, r_bearing=R_DEFAULT):
    """(err, spread, bar): the device against long double; spread = binary64 against long double of gate_ref on this very input in the same
    measure; bar = max(32 spread, 64 * 2^-52): a 25-product congruence in another order and a sqrt / atan2 that may differ by a few ulp"""
    _, m_ld = gate_ref(X, P, obs, r_range, r_bearing, np.inf, np.longdouble)
    _, m_64 = gate_ref(X, P, obs, r_range, r_bearing, np.inf, np.float64)
    spread = err_of(m_64, m_ld)
    return err_of(m_dev, m_ld), spread, max(32 * spread, 64 * EPS)


def predicted(X, k):
    """the exact predicted reading (range, bearing) of landmark k, binary64"""
    dx, dy = X[3 + 2 * k] - X[0], X[4 + 2 * k] - X[1]
    return np.hypot(dx, dy), np.arctan2(dy, dx) - X[2]


def crafted():
    """name -> dict(X, P, obs, gate, assoc): states and observations with the outputs they must give (assoc; mdist is +inf exactly where
    `inf` says so), r_range = r_bearing = the defaults"""
    def state(points, var=0.01):
        n = 3 + 2 * len(points)
        X = np.concatenate([[0.5, -0.25, 0.1], np.asarray(points, np.float64).reshape(-1)])
        return X, var * np.eye(n)

    def near(X, k, dr=0.01, db=0.005, turns=0):
        r, b = predicted(X, k)
        return [r + dr, b + db + 2 * np.pi * turns]

    out = {}
    # two landmarks with identical coordinates and identical covariance blocks: m is the same bit for bit, the smaller index wins
    X, P = state([[3.0, 1.0], [-2.0, 4.0], [3.0, 1.0]])
    P[0, 3] = P[3, 0] = P[0, 7] = P[7, 0] = 0.002
    out["twins"] = dict(X=X, P=P, obs=[near(X, 0), near(X, 2, -0.02), near(X, 1)], gate=GATE, assoc=[0, 0, 1], inf=[0, 0, 0])
    # a landmark exactly at the pose (q = 0) is skipped, whatever the gate
    X, P = state([[0.5, -0.25], [3.0, 1.0]])
    out["at-pose"] = dict(X=X, P=P, obs=[[0.001, 0.3], near(X, 1)], gate=np.inf, assoc=[1, 1], inf=[0, 0])
    # a negative variance that makes s00 = 0.01 - 1 + 0.2 <= 0: skipped
    X, P = state([[3.0, 1.0], [-2.0, 4.0]])
    P[3, 3] = P[4, 4] = -1.0
    out["negative-variance"] = dict(X=X, P=P, obs=[near(X, 0), near(X, 1)], gate=np.inf, assoc=[1, 1], inf=[0, 0])
    # the same with that landmark the only one: no valid landmark at all
    X, P = state([[3.0, 1.0]])
    P[3, 3] = P[4, 4] = -1.0
    out["nothing-valid"] = dict(X=X, P=P, obs=[near(X, 0)], gate=np.inf, assoc=[-1], inf=[1])
    # NaN or inf in range or bearing: -1 and +inf, even with an infinite gate
    X, P = state([[3.0, 1.0], [-2.0, 4.0]])
    nan, inf = np.nan, np.inf
    out["non-finite"] = dict(X=X, P=P, obs=[[nan, 0.1], [1.0, nan], [inf, 0.1], [1.0, inf], [-inf, -inf], near(X, 1)], gate=np.inf,
                             assoc=[-1, -1, -1, -1, -1, 1], inf=[1, 1, 1, 1, 1, 0])
    # a bearing offset by a whole turn either way: the same landmark
    X, P = state([[3.0, 1.0], [-2.0, 4.0], [-3.0, -2.0]])
    out["turns"] = dict(X=X, P=P, obs=[near(X, k, turns=t) for k in range(3) for t in (0, 1, -1)], gate=GATE,
                        assoc=[0, 0, 0, 1, 1, 1, 2, 2, 2], inf=[0] * 9)
    # far from everything: -1 at 9.21, the nearest in the metric with an infinite gate
    far = [[40.0, 0.0], [25.0, 2.0]]
    out["far-gated"] = dict(X=X, P=P, obs=far, gate=GATE, assoc=[-1, -1], inf=[0, 0])
    out["far-gate-inf"] = dict(X=X, P=P, obs=far, gate=np.inf, assoc=None, inf=[0, 0])  # (assoc: every entry >= 0, = the reference's)
    X, P = state([])
    out["no-landmark"] = dict(X=X, P=P, obs=[[1.0, 0.1], [2.0, -0.1]], gate=np.inf, assoc=[-1, -1], inf=[1, 1])
    return out
