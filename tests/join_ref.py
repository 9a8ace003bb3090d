"""NumPy reference of aslam_join_maps (include/aslam_snapshot.h).

  join             the header's formulas, literally, in binary64 or np.longdouble: reads the LOWER triangle of the source's P and mirrors
  spread_and_bar   the bar the device is held to, from the two evaluations alone (the precedent: merge_ref.spread_and_bar)
  synthetic        the inputs of the tests: SPD covariances with off-diagonal structure, a pose well away from every joined landmark
  fusion_case      filter A with 6 landmarks, record B with the same 6 and 2 others (host test 3, GPU test 7)
  wrap, predict    the binary64 wrap of the kernels' normalizeAngle; the reading a pose predicts for a point

A frame is (tx, ty, phi, cov3x3), as awesomeslam_amd.mapjoin.frame returns it; sel is None (every landmark) or one entry per landmark."""
import numpy as np

EPS = 2.0 ** -52
GENERAL = (3.0, -2.0, 0.7)  # the tests' general frame: (tx, ty, phi)


def identity():
    return 0.0, 0.0, 0.0, np.zeros((3, 3))


def general_frame(seed=7):
    """GENERAL with a full SPD covariance: centimetres in t, a fraction of a degree in phi, all correlated"""
    F = np.random.default_rng(seed).standard_normal((3, 3)) * np.array([[0.02], [0.02], [0.005]])
    cov = F @ F.T + np.diag([1e-5, 1e-5, 1e-6])
    return GENERAL + (np.tril(cov) + np.tril(cov, -1).T,)


def wrap(theta):
    """fmod by 2 pi, then one step into [-pi, pi]: device_common.h's normalizeAngle in the dtype of theta"""
    dt = np.asarray(theta).dtype.type
    pi = dt(np.pi) if dt is np.float64 else np.longdouble(3.14159265358979323846)  # (the device's constant: binary64 pi)
    r = np.fmod(theta, 2 * pi)
    r = np.where(r > pi, r - 2 * pi, r)
    return np.where(r < -pi, r + 2 * pi, r)


def predict(pose, x, y):
    """(range, bearing) of the point (x, y) from pose (px, py, heading)"""
    dx, dy = x - pose[0], y - pose[1]
    return np.sqrt(dx * dx + dy * dy), wrap(np.arctan2(dy, dx) - pose[2])


def selected(sel, LB):
    if sel is None:
        return list(range(LB))
    return [k for k in range(LB) if k < len(sel) and sel[k]]


def transform(frame, l, dtype=np.float64):
    """(l', R, G) of the point l under the frame: l' = t + R l, G = d l' / d (tx, ty, phi)"""
    tx, ty, phi = (dtype(v) for v in frame[:3])
    c, s = dtype(np.cos(np.float64(phi))), dtype(np.sin(np.float64(phi)))  # taken once, in binary64, as the call takes them on the host
    lx, ly = dtype(l[0]), dtype(l[1])
    lp = np.array([tx + c * lx - s * ly, ty + s * lx + c * ly], dtype)
    R = np.array([[c, -s], [s, c]], dtype)
    G = np.array([[1, 0, -s * lx - c * ly], [0, 1, c * lx - s * ly]], dtype)
    return lp, R, G


def join(XA, ZA, PA, XB, PB, sel, frame, dtype=np.float64):
    XA, ZA, PA, XB, PB = (np.asarray(a, dtype) for a in (XA, ZA, PA, XB, PB))
    cov = np.asarray(frame[3], dtype).reshape(3, 3)
    nA, ks = len(XA), selected(sel, (len(XB) - 3) // 2)
    m = len(ks)
    n = nA + 2 * m
    X, Z, P = np.zeros(n, dtype), np.zeros(n, dtype), np.zeros((n, n), dtype)
    X[:nA], Z[:nA], P[:nA, :nA] = XA, ZA, PA
    Gs = []
    for p, k in enumerate(ks):
        lp, R, G = transform(frame, XB[3 + 2 * k:5 + 2 * k], dtype)
        Gs.append(G)
        X[nA + 2 * p:nA + 2 * p + 2] = lp
        Z[nA + 2 * p], Z[nA + 2 * p + 1] = predict(XA[:3], lp[0], lp[1])
    for p, kp in enumerate(ks):
        for q, kq in enumerate(ks[:p + 1]):
            B = PB[3 + 2 * kp:5 + 2 * kp, 3 + 2 * kq:5 + 2 * kq].copy()
            if p == q:
                B[0, 1] = B[1, 0]  # the lower triangle only
            blk = R @ B @ R.T + Gs[p] @ cov @ Gs[q].T
            if p == q:
                blk[0, 1] = blk[1, 0]
            P[nA + 2 * p:nA + 2 * p + 2, nA + 2 * q:nA + 2 * q + 2] = blk
            P[nA + 2 * q:nA + 2 * q + 2, nA + 2 * p:nA + 2 * p + 2] = blk.T
    return X, Z, P


def spread_and_bar(XA, ZA, PA, XB, PB, sel, frame):
    """(spread, bar, (X, Z, P)): spread = the error of the binary64 evaluation against the same function in np.longdouble on this very input
    (util.rel_err on X and Z, util.cov_err on P); bar = max(32 spread, 64 * 2^-52).  32 is merge_ref's factor: an entry is a 3-term congruence
    after a 2-term one, in an order the device may choose, plus a device sqrt / atan2 that may differ from NumPy's by a few ulp."""
    from util import cov_err, rel_err

    X, Z, P = join(XA, ZA, PA, XB, PB, sel, frame)
    Xl, Zl, Pl = (np.asarray(a, np.float64) for a in join(XA, ZA, PA, XB, PB, sel, frame, np.longdouble))
    spread = max(rel_err(X, Xl), rel_err(Z, Zl), cov_err(P, Pl))
    return spread, max(32 * spread, 64 * EPS), (X, Z, P)


def spd(n, rng, ridge=0.01):
    F = rng.standard_normal((n, n))
    P = F @ F.T / n * 0.02 + ridge * np.eye(n)
    return np.tril(P) + np.tril(P, -1).T


def measurements(X):
    """the Z a filter at X would hold with every landmark just sighted: its pose, then (range, bearing) per landmark"""
    Z = np.array(X, np.float64)
    Z[3::2], Z[4::2] = predict(X[:3], X[3::2], X[4::2])
    return Z


def clear_of(pose, pts, frames):
    """every point, under every frame, at least 1 m from the pose and its bearing 0.1 rad away from the branch of atan2 and of the wrap"""
    for fr in frames:
        for l in pts:
            lp = transform(fr, l)[0]
            dx, dy = lp[0] - pose[0], lp[1] - pose[1]
            b = np.arctan2(dy, dx)
            if np.hypot(dx, dy) < 1.0 or abs(b) > np.pi - 0.1 or abs(abs(np.fmod(b - pose[2], 2 * np.pi)) - np.pi) < 0.1:
                return False
    return True


def synthetic(nA, LB, seed, junk_upper=True):
    """(XA, ZA, PA, XB, PB): P = F F^T / n * 0.02 + 0.01 I, landmark coordinates in +-20, A's pose at least 1 m from every landmark of B under
    the identity and under GENERAL (and its bearing away from the branches).  junk_upper: the strict upper triangle of PB holds other
    numbers than the lower one -- the join must not read it."""
    rng = np.random.default_rng(seed)
    frames = (identity(), GENERAL + (np.zeros((3, 3)),))
    XA = rng.uniform(-20, 20, nA)
    XA[:3] = rng.uniform(-0.5, 0.5, 3)
    XB = rng.uniform(-20, 20, 3 + 2 * LB)
    for k in range(LB):
        while not clear_of(XA[:3], [XB[3 + 2 * k:5 + 2 * k]], frames):
            XB[3 + 2 * k:5 + 2 * k] = rng.uniform(-20, 20, 2)
    PA, PB = spd(nA, rng), spd(3 + 2 * LB, rng)
    if junk_upper:
        PB = np.tril(PB) + np.triu(rng.standard_normal(PB.shape), 1)
    return XA, measurements(XA), PA, XB, PB


def fusion_case(displace=0.0, seed=11):
    """(XA, ZA, PA, XB, PB): A has a pose and 6 landmarks on a circle of 8 m, B the same 6 (each moved by `displace` metres in a direction of
    its own) and 2 others; every two distinct points are more than 4 m apart.  Both covariances are spd()."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(8) / 8 + 0.2
    pts = np.stack([8 * np.cos(ang), 8 * np.sin(ang)], 1)
    XA = np.concatenate([[0.3, -0.2, 0.1], pts[:6].reshape(-1)])
    d = rng.uniform(0, 2 * np.pi, 6)
    moved = pts[:6] + displace * np.stack([np.cos(d), np.sin(d)], 1)
    XB = np.concatenate([[1.0, 2.0, -0.4], moved.reshape(-1), pts[6:].reshape(-1)])
    return XA, measurements(XA), spd(15, rng), XB, spd(19, rng)


FUSION_PAIRS = [(i, 6 + i) for i in range(6)]  # A's landmark i and its twin among the joined ones
