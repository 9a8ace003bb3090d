"""-m "not gpu": the reference of aslam_join_maps (join_ref) against first principles, and awesomeslam_amd.mapjoin.align.  No GPU, no library."""
import numpy as np
import pytest

import join_ref as jr
import merge_ref as mr
from awesomeslam_amd import mapjoin
from util import cov_err, rel_err

EPS = 2.0 ** -52


# ---- 1. Jacobians --------------------------------------------------------------------------------------------------------------------
def test_jacobians_against_finite_differences():
    """G_p and R against central differences of (t, phi, l) -> l' with h = 1e-6: truncation ~ h^2 |l|, rounding ~ eps / h, both near 1e-10"""
    h = 1e-6
    rng = np.random.default_rng(1)
    for _ in range(8):
        l = rng.uniform(-20, 20, 2)
        t = rng.uniform(-5, 5, 2)
        phi = rng.uniform(-3, 3)
        f = lambda v: jr.transform((v[0], v[1], v[2], None), v[3:5])[0]  # noqa: E731
        v0 = np.array([t[0], t[1], phi, l[0], l[1]])
        J = np.zeros((2, 5))
        for k in range(5):
            e = np.zeros(5)
            e[k] = h
            J[:, k] = (f(v0 + e) - f(v0 - e)) / (2 * h)
        _, R, G = jr.transform((t[0], t[1], phi, None), l)
        assert np.abs(J[:, :3] - G).max() < 1e-7 and np.abs(J[:, 3:] - R).max() < 1e-7


# ---- 2. structure --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nA,LB,sel", [(3, 1, None), (13, 6, [1, 0, 1, 0, 1, 0]), (29, 9, None)])
def test_structure(nA, LB, sel):
    XA, ZA, PA, XB, PB = jr.synthetic(nA, LB, seed=nA)
    ks = jr.selected(sel, LB)
    rows = [r for k in ks for r in (3 + 2 * k, 4 + 2 * k)]
    low = np.tril(PB) + np.tril(PB, -1).T
    X, Z, P = jr.join(XA, ZA, PA, XB, PB, sel, jr.identity())
    n = nA + 2 * len(ks)
    assert X.shape == Z.shape == (n,) and P.shape == (n, n)
    assert np.array_equal(X[nA:], XB[rows]) and np.array_equal(P[nA:, nA:], low[np.ix_(rows, rows)])  # bit for bit, the upper triangle unread
    assert np.array_equal(X[:nA], XA) and np.array_equal(Z[:nA], ZA) and np.array_equal(P[:nA, :nA], PA)
    assert not P[:nA, nA:].any() and not P[nA:, :nA].any() and not np.signbit(P[:nA, nA:]).any()
    assert np.array_equal(P, P.T)
    r, b = jr.predict(XA[:3], X[nA::2], X[nA + 1::2])
    assert np.array_equal(Z[nA::2], r) and np.array_equal(Z[nA + 1::2], b) and r.min() >= 1.0
    # a general frame with an SPD covariance keeps the matrix positive semi-definite to rounding
    Xg, Zg, Pg = jr.join(XA, ZA, PA, XB, PB, sel, jr.general_frame())
    assert np.array_equal(Pg, Pg.T) and np.array_equal(Pg[:nA, :nA], PA) and not Pg[:nA, nA:].any()
    assert np.linalg.eigvalsh(Pg).min() >= -64 * EPS * np.linalg.norm(Pg, 2)
    spread, bar, _ = jr.spread_and_bar(XA, ZA, PA, XB, PB, sel, jr.general_frame())
    print(f"join_ref nA={nA} m={len(ks)}: spread {spread:.2e} bar {bar:.2e}")
    assert spread < 1e-13


# ---- 3. join then merge is Bayesian fusion ----------------------------------------------------------------------------------------------
def inv_ld(M):
    """Gauss-Jordan with partial pivoting in np.longdouble (np.linalg has no extended precision)"""
    M = np.array(M, np.longdouble)
    n = len(M)
    A = np.concatenate([M, np.eye(n, dtype=np.longdouble)], 1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]] = A[[p, k]]
        A[k] = A[k] / A[k, k]
        for r in range(n):
            if r != k:
                A[r] = A[r] - A[r, k] * A[k]
    return A[:, n:]


def test_join_then_merge_is_bayesian_fusion():
    """A's Gaussian updated with the observation x_B[shared] of covariance P_B[shared, shared], the unshared landmarks appended with their
    conditional cross terms: in information form over y = (a, b_unshared), Lambda = blkdiag(Lambda_A, 0) + M^T Lambda_B M and
    eta = (Lambda_A x_A, 0) + M^T Lambda_B x_B, M mapping y to B's landmark vector (the shared ones are A's own landmarks)."""
    XA, ZA, PA, XB, PB = jr.fusion_case()
    X, _, P = jr.join(XA, ZA, PA, XB, PB, None, jr.identity())
    assert len(X) == 31
    Xm, Pm = mr.merge_joint(X, P, jr.FUSION_PAIRS, 0.0)
    assert len(Xm) == 19
    ld = np.longdouble
    LA, LB = inv_ld(PA), inv_ld(PB[3:, 3:])
    M = np.zeros((16, 19), ld)
    M[:12, 3:15] = np.eye(12)
    M[12:, 15:] = np.eye(4)
    Lam = M.T @ LB @ M
    Lam[:15, :15] += LA
    eta = M.T @ (LB @ XB[3:].astype(ld))
    eta[:15] += LA @ XA.astype(ld)
    Pe = inv_ld(Lam)
    Xe = Pe @ eta
    _, bar, _ = mr.spread_and_bar(X, P, jr.FUSION_PAIRS, 0.0)
    ex, ep = rel_err(Xm, np.asarray(Xe, np.float64)), cov_err(Pm, np.asarray(Pe, np.float64))
    print(f"join + merge against the information form: X {ex:.2e} P {ep:.2e} bar {bar:.2e}")
    assert max(ex, ep) <= bar


# ---- 4. mapjoin.align ---------------------------------------------------------------------------------------------------------------------
def test_align_recovers_a_noiseless_transform():
    rng = np.random.default_rng(4)
    xb = rng.uniform(-20, 20, (8, 2))
    tx, ty, phi = jr.GENERAL
    xa = np.stack([jr.transform((tx, ty, phi, None), l)[0] for l in xb])
    perm = rng.permutation(8)
    got = mapjoin.align(xa[perm], xb, [(int(np.flatnonzero(perm == k)[0]), k) for k in range(8)])
    assert np.abs(np.array(got[:3]) - np.array([tx, ty, phi])).max() <= 64 * EPS * 25
    assert got[3].shape == (3, 3) and np.array_equal(got[3], got[3].T)


def test_align_covariance_of_centred_points():
    rng = np.random.default_rng(5)
    K, sa, sb = 7, 0.03, 0.05
    xb = rng.uniform(-20, 20, (K, 2))
    xb -= xb.mean(axis=0)
    xa = np.stack([jr.transform(jr.GENERAL + (None,), l)[0] for l in xb])
    cov = mapjoin.align(xa, xb, [(k, k) for k in range(K)], cov_a=sa ** 2 * np.eye(2), cov_b=sb ** 2 * np.eye(2))[3]
    want = (sa ** 2 + sb ** 2) / K
    assert np.abs(cov[:2, :2] - want * np.eye(2)).max() <= 1e-12 * want
    assert np.abs(cov[:2, 2]).max() <= 1e-12 * np.sqrt(want * cov[2, 2])
    assert abs(cov[2, 2] - (sa ** 2 + sb ** 2) / (xb ** 2).sum()) <= 1e-12 * cov[2, 2]


def test_align_needs_two_pairs():
    with pytest.raises(ValueError):
        mapjoin.align([[0.0, 0.0]], [[1.0, 1.0]], [(0, 0)])
    with pytest.raises(ValueError):
        mapjoin.align([[0.0, 0.0]], [[1.0, 1.0]], [])


def test_frame_defaults():
    assert mapjoin.frame()[:3] == (0.0, 0.0, 0.0) and not mapjoin.frame()[3].any()
