"""NumPy reference of aslam_joint_compat (include/aslam_core.h): the sequential joint-compatibility test of a hypothesis of pairings.

  terms          per observation: the usable candidate, its 2 x 5 Jacobian, the five state indices and the innovation
  sequential     the rule in the bordering form the header gives: assoc, incr, D2, logdet, accepted, refused, and every attempt's figures
  dense          D2 = nu^T (H P H^T + R)^-1 nu and log det of the same hypothesis with the dense 2m x n Jacobian and a linear solve, the
                 increments as differences of D2 -- what the bordering form is a shortcut of
  margins        how far the decisions are from flipping, from the long-double bordering form
  err_and_bar    the device's numbers against long double, and the bar from the references' own spread
  crafted        the edge cases, shared by the host and the GPU test

Every function takes `dtype` (np.float64 or np.longdouble) and does all arithmetic in it; 2 pi is the binary64 constant in both.  np.linalg
does not take long double, so `dense` solves by Gaussian elimination with partial pivoting (solve_logdet) there and by np.linalg in binary64."""
from types import SimpleNamespace

import numpy as np

import assoc_ref as ar

EPS = ar.EPS


def lower(P, dtype):
    """the symmetric matrix the lower triangle of P stands for"""
    P = np.asarray(P, dtype)
    return np.tril(P) + np.tril(P, -1).T


def terms(X, obs, cand, dtype=np.float64):
    """one entry per observation: None where the candidate is not usable (outside [0, L) or q not > 0), else (k, H [2, 5], idx [5], nu [2])"""
    X = np.asarray(X, dtype)
    obs = np.asarray(obs, np.float32).reshape(-1, 2)
    L = (len(X) - 3) // 2
    two_pi = dtype(2.0 * np.pi)
    out = []
    with np.errstate(all="ignore"):
        for (r, beta), k in zip(obs, np.asarray(cand, np.int64)):
            if not 0 <= k < L:
                out.append(None)
                continue
            a0, a1 = 3 + 2 * int(k), 4 + 2 * int(k)
            dx, dy = X[a0] - X[0], X[a1] - X[1]
            q = dx * dx + dy * dy
            if not q > 0:
                out.append(None)
                continue
            rh = np.sqrt(q)
            bh = np.arctan2(dy, dx) - X[2]
            H = np.array([[-dx / rh, -dy / rh, dtype(0), dx / rh, dy / rh], [dy / q, -dx / q, dtype(-1), -dy / q, dx / q]], dtype)
            nu = np.array([dtype(r) - rh, ar.ieee_remainder(dtype(beta) - bh, two_pi)], dtype)
            out.append((int(k), H, [0, 1, 2, a0, a1], nu))
    return out


def sequential(X, P, obs, cand, r_range=ar.R_DEFAULT, r_bearing=ar.R_DEFAULT, gate_tab=None, dtype=np.float64, follow=None):
    """The rule, by bordering.  gate_tab [>= n_obs + 1] or None (evaluate mode: every usable candidate is accepted).  `follow`: a list of
    verdicts to take instead of deciding ("accept" / "refuse" / "unusable" per observation; the numbers of one hypothesis in another precision).
    Returns a namespace: assoc [n_obs] int32, incr [n_obs] (+inf where unusable), D2, logdet, accepted, refused, verdicts, prefix (per
    observation the accepted observations before it), attempts (per usable candidate that reached the test: dict(j, m, total, bound, T00, d,
    C00, C11))."""
    Pl = lower(P, dtype)
    R = np.diag(np.array([r_range, r_bearing], dtype))
    T = terms(X, obs, cand, dtype)
    n_obs = len(T)
    assoc, incr = np.full(n_obs, -1, np.int32), np.full(n_obs, np.inf, dtype)
    acc, verdicts, prefix, attempts = [], [], [], []
    LA = np.zeros((2 * n_obs, 2 * n_obs), dtype)
    z = np.zeros(2 * n_obs, dtype)
    D2, logdet, refused = dtype(0), dtype(0), 0
    with np.errstate(all="ignore"):
        for j, t in enumerate(T):
            prefix.append(list(acc))
            if t is None:
                verdicts.append("unusable")
                continue
            k, H, idx, nu = t
            m = len(acc)
            Cjj = H @ Pl[np.ix_(idx, idx)] @ H.T + R
            Y = np.zeros((2, 2 * m), dtype)
            for col, i in enumerate(acc):
                _, Hi, idi, _ = T[i]
                Y[:, 2 * col:2 * col + 2] = H @ Pl[np.ix_(idx, idi)] @ Hi.T  # c, solved in place below
            for p in range(2 * m):  # Y = c L_A^-T, forward substitution
                Y[:, p] = (Y[:, p] - Y[:, :p] @ LA[p, :p]) / LA[p, p]
            Tm = Cjj - Y @ Y.T
            T00 = Tm[0, 0]
            t00 = np.sqrt(T00)
            t10 = Tm[1, 0] / t00
            d = Tm[1, 1] - t10 * t10
            t11 = np.sqrt(d)
            w = nu - Y @ z[:2 * m]
            z0 = w[0] / t00
            z1 = (w[1] - t10 * z0) / t11
            dd = z0 * z0 + z1 * z1
            usable = bool(T00 > 0) and bool(d > 0) and bool(np.isfinite(dd))
            if follow is not None:
                verdict = follow[j]
            elif not usable:
                verdict = "unusable"
            else:
                verdict = "accept" if gate_tab is None or bool(D2 + dd < dtype(gate_tab[m + 1])) else "refuse"
            verdicts.append(verdict)
            if verdict == "unusable":
                if follow is None:
                    attempts.append(dict(j=j, m=m, total=None, bound=None, T00=T00, d=d, C00=Cjj[0, 0], C11=Cjj[1, 1]))
                continue
            attempts.append(dict(j=j, m=m, total=D2 + dd, bound=None if gate_tab is None else dtype(gate_tab[m + 1]), T00=T00, d=d, C00=Cjj[0, 0],
                                 C11=Cjj[1, 1]))
            incr[j] = dd
            if verdict == "refuse":
                refused += 1
                continue
            LA[2 * m, :2 * m], LA[2 * m + 1, :2 * m] = Y[0], Y[1]
            LA[2 * m, 2 * m], LA[2 * m + 1, 2 * m], LA[2 * m + 1, 2 * m + 1] = t00, t10, t11
            z[2 * m], z[2 * m + 1] = z0, z1
            D2 = D2 + dd
            logdet = logdet + dtype(2) * np.log(t00 * t11)
            acc.append(j)
            assoc[j] = k
    return SimpleNamespace(assoc=assoc, incr=incr, D2=D2, logdet=logdet, accepted=len(acc), refused=refused, verdicts=verdicts, prefix=prefix,
                           attempts=attempts, acc=acc)


def solve_logdet(C, v):
    """(C^-1 v, log det C) of a symmetric positive definite C in C's own dtype: np.linalg in binary64, elimination with partial pivoting else"""
    if len(v) == 0:
        return v.copy(), C.dtype.type(0)
    if C.dtype == np.float64:
        sign, ld = np.linalg.slogdet(C)
        assert sign > 0
        return np.linalg.solve(C, v), ld
    A, x = C.copy(), v.copy()
    n = len(x)
    ld = A.dtype.type(0)
    for p in range(n):
        q = p + int(np.argmax(np.abs(A[p:, p])))
        if q != p:
            A[[p, q]], x[[p, q]] = A[[q, p]], x[[q, p]]
        assert A[p, p] != 0
        ld = ld + np.log(np.abs(A[p, p]))
        f = A[p + 1:, p] / A[p, p]
        A[p + 1:, p:] -= np.outer(f, A[p, p:])
        x[p + 1:] -= f * x[p]
    for p in range(n - 1, -1, -1):
        x[p] = (x[p] - A[p, p + 1:] @ x[p + 1:]) / A[p, p]
    return x, ld


def dense(X, P, obs, cand, hyp, r_range=ar.R_DEFAULT, r_bearing=ar.R_DEFAULT, dtype=np.float64):
    """(D2, logdet, incr [n_obs]) of the hypothesis `hyp` (a result of sequential: its verdicts and prefixes) the dense way: the 2 x n Jacobian
    of every usable candidate, G = H_all P H_all^T + R once, and for a list A of observations D2(A) = nu_A^T G_AA^-1 nu_A by a linear solve;
    incr[j] = D2(prefix_j + [j]) - D2(prefix_j)"""
    Pl = lower(P, dtype)
    T = terms(X, obs, cand, dtype)
    n, n_obs = Pl.shape[0], len(T)
    H = np.zeros((2 * n_obs, n), dtype)
    nu = np.zeros(2 * n_obs, dtype)
    for j, t in enumerate(T):
        if t is not None:
            H[2 * j:2 * j + 2, t[2]] = t[1]
            nu[2 * j:2 * j + 2] = t[3]
    G = H @ Pl @ H.T + np.kron(np.eye(n_obs, dtype=dtype), np.diag(np.array([r_range, r_bearing], dtype)))

    def D2_of(A):
        rows = [2 * j + r for j in A for r in range(2)]
        x, ld = solve_logdet(G[np.ix_(rows, rows)], nu[rows])
        return nu[rows] @ x, ld

    incr = np.full(n_obs, np.inf, dtype)
    with np.errstate(all="ignore"):
        before = {}
        for j in range(n_obs):
            if hyp.verdicts[j] == "unusable":
                continue
            key = tuple(hyp.prefix[j])
            if key not in before:
                before[key] = D2_of(list(key))[0]
            incr[j] = D2_of(list(key) + [j])[0] - before[key]
        D2, ld = D2_of(hyp.acc)
    return D2, ld, incr


def margins(X, P, obs, cand, r_range=ar.R_DEFAULT, r_bearing=ar.R_DEFAULT, gate_tab=None):
    """(decision margin, pivot margin) from the long-double bordering form: min |D2 + dd - bound| / bound over the attempts with a finite bound,
    and min(|T00| / |C00|, |d| / |C11|) over every candidate that reached the factorisation; +inf where there is none"""
    ld = sequential(X, P, obs, cand, r_range, r_bearing, gate_tab, np.longdouble)
    g, t = np.inf, np.inf
    for a in ld.attempts:
        if a["bound"] is not None and np.isfinite(a["bound"]) and a["total"] is not None:
            g = min(g, float(abs(a["total"] - a["bound"]) / a["bound"]))
        t = min(t, float(abs(a["T00"]) / abs(a["C00"])))
        if np.isfinite(a["d"]):
            t = min(t, float(abs(a["d"]) / abs(a["C11"])))
    return g, t


def err_of(dev, ld, signed=False):
    """max |dev - ld| / max(ld, 1) (|ld| where `signed`) over the finite entries; where the reference is +inf the other side must be too"""
    dev, ld = np.atleast_1d(np.asarray(dev, np.longdouble)), np.atleast_1d(np.asarray(ld, np.longdouble))
    fin = np.isfinite(ld)
    if not np.array_equal(np.isposinf(dev), ~fin):
        return np.inf
    if not fin.any():
        return 0.0
    scale = np.maximum(np.abs(ld[fin]) if signed else ld[fin], 1)
    return float((np.abs(dev[fin] - ld[fin]) / scale).max())


def err_and_bar(dev, X, P, obs, cand, r_range=ar.R_DEFAULT, r_bearing=ar.R_DEFAULT, gate_tab=None):
    """dev: (D2, logdet, incr [n_obs]) of the device.  Returns (ld, {name: (err, spread, bar)}) for D2, incr and logdet: err against the
    long-double bordering form; spread = the larger of two binary64-versus-long-double differences of the reference on this very input, the
    bordering form's and the dense form's (both following the long-double decisions: one hypothesis, two binary64 evaluation orders -- the
    device's is a third); bar = max(32 spread, 64 * 2^-52)"""
    ld = sequential(X, P, obs, cand, r_range, r_bearing, gate_tab, np.longdouble)
    b64 = sequential(X, P, obs, cand, r_range, r_bearing, gate_tab, np.float64, follow=ld.verdicts)
    d64 = dense(X, P, obs, cand, ld, r_range, r_bearing, np.float64)
    dld = dense(X, P, obs, cand, ld, r_range, r_bearing, np.longdouble)
    out = {}
    for name, i, signed in (("D2", 0, False), ("logdet", 1, True), ("incr", 2, False)):
        want = (ld.D2, ld.logdet, ld.incr)[i]
        spread = max(err_of((b64.D2, b64.logdet, b64.incr)[i], want, signed), err_of(d64[i], dld[i], signed))
        out[name] = (err_of(dev[i], want, signed), spread, max(32 * spread, 64 * EPS))
    return ld, out


def shift_reading(X, point, shift):
    """the exact reading (range, bearing) of `point` moved by `shift`, from the pose in X"""
    dx, dy = point[0] + shift[0] - X[0], point[1] + shift[1] - X[1]
    return [np.hypot(dx, dy), np.arctan2(dy, dx) - X[2]]


def crafted():
    """name -> dict(X, P, r (= r_range = r_bearing), obs, cand, prob (None: evaluate mode), assoc (None: whatever the reference says), inf
    (where incr is +inf), accepted, refused)"""
    out = {}
    pts = np.array([[3.0, 1.0], [-2.0, 4.0], [-3.0, -2.0], [4.0, -3.0], [1.0, 5.0]])
    shifts = [(0.6, -0.4), (-0.6, 0.4), (0.6, -0.4), (0.62, -0.37), (0.1, 0.9)]
    X = np.concatenate([[0.5, -0.25, 0.1], pts.reshape(-1)])
    P = 1e-4 * np.eye(13)
    for a in range(5):
        for c in range(5):
            P[3 + 2 * a, 3 + 2 * c] += 0.25
            P[4 + 2 * a, 4 + 2 * c] += 0.25
    obs = [shift_reading(X, p, s) for p, s in zip(pts, shifts)]
    # a common translation of three landmarks is jointly consistent, the two that moved otherwise are not -- though each passes alone
    out["common-shift"] = dict(X=X, P=P, r=1e-3, obs=obs, cand=[0, 1, 2, 3, 4], prob=0.99, assoc=[0, -1, 2, 3, -1], inf=[0] * 5, accepted=3, refused=2)
    out["common-shift-evaluate"] = dict(X=X, P=P, r=1e-3, obs=obs, cand=[0, 1, 2, 3, 4], prob=None, assoc=[0, 1, 2, 3, 4], inf=[0] * 5, accepted=5,
                                        refused=0)
    # the same message with observation 1 at the front: the rule depends on the order
    order = [1, 0, 2, 3, 4]
    out["common-shift-reordered"] = dict(X=X, P=P, r=1e-3, obs=[obs[i] for i in order], cand=order, prob=0.99, assoc=None, inf=[0] * 5, accepted=None,
                                         refused=None)
    out["one-observation"] = dict(X=X, P=P, r=1e-3, obs=obs[:1], cand=[0], prob=0.99, assoc=[0], inf=[0], accepted=1, refused=0)
    c = ar.crafted()
    X2, P2 = c["turns"]["X"], c["turns"]["P"]
    near = [[ar.predicted(X2, 0)[0] + 0.01, ar.predicted(X2, 0)[1] + 0.005], [ar.predicted(X2, 0)[0] - 0.02, ar.predicted(X2, 0)[1] + 0.002]]
    out["same-candidate"] = dict(X=X2, P=P2, r=ar.R_DEFAULT, obs=near, cand=[0, 0], prob=0.99, assoc=[0, 0], inf=[0, 0], accepted=2, refused=0)
    out["bad-candidates"] = dict(X=X2, P=P2, r=ar.R_DEFAULT, obs=[near[0]] * 4, cand=[3, -7, 10 ** 6, 0], prob=0.99, assoc=[-1, -1, -1, 0],
                                 inf=[1, 1, 1, 0], accepted=1, refused=0)
    out["non-finite"] = dict(X=X2, P=P2, r=ar.R_DEFAULT, obs=[[np.nan, 0.1], near[0], [np.inf, 0.1], [1.0, np.nan]], cand=[0, 0, 1, 2], prob=0.99,
                             assoc=[-1, 0, -1, -1], inf=[1, 0, 1, 1], accepted=1, refused=0)
    for name, bad in (("at-pose", 0), ("negative-variance", 0)):
        s = c[name]
        out[name] = dict(X=s["X"], P=s["P"], r=ar.R_DEFAULT, obs=s["obs"], cand=[bad, 1], prob=0.99, assoc=[-1, 1], inf=[1, 0], accepted=1, refused=0)
    s = c["no-landmark"]
    out["no-landmark"] = dict(X=s["X"], P=s["P"], r=ar.R_DEFAULT, obs=s["obs"], cand=[0, -1], prob=0.99, assoc=[-1, -1], inf=[1, 1], accepted=0, refused=0)
    out["no-observation"] = dict(X=X2, P=P2, r=ar.R_DEFAULT, obs=[], cand=[], prob=0.99, assoc=[], inf=[], accepted=0, refused=0)
    return out


def cap64():
    """(X, P, obs [64, 2] float32, cand [64]): N = 133 (65 landmarks), the predicted readings of 64 distinct landmarks plus 0.05 normal noise"""
    import merge_ref as mr

    X, P = mr.synthetic(133, [])
    rng = np.random.default_rng(6464)
    cand = rng.permutation(65)[:64].astype(np.int32)
    obs = np.array([ar.predicted(X, int(k)) for k in cand]) + 0.05 * rng.standard_normal((64, 2))
    return X, P, obs.astype(np.float32), cand
