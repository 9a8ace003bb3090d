"""Consistency statistics of a filter run, from what Core.replay_stats() streams out (NumPy only).

    nis      y^T S^-1 y of every callback's slam() (chi-square with `dims` degrees of freedom for a consistent filter)
    logdet   ln |det S|
    pose_cov the lower triangle of the pose block of P after the update: P(0,0) P(1,0) P(1,1) P(2,0) P(2,1) P(2,2)

Callbacks in which slam() did not run carry NaN; the functions below pass it through.
"""
import numpy as np

LN_2PI = float(np.log(2.0 * np.pi))


def log_likelihood(nis, logdet, dims):
    """Gaussian log-likelihood of the innovation, -1/2 (NIS + ln det S + n ln 2 pi), element-wise."""
    nis, logdet, dims = np.asarray(nis, np.float64), np.asarray(logdet, np.float64), np.asarray(dims, np.float64)
    return -0.5 * (nis + logdet + dims * LN_2PI)


def wrap_angle(a):
    """a wrapped into [-pi, pi)."""
    return (np.asarray(a, np.float64) + np.pi) % (2.0 * np.pi) - np.pi


def pose_cov_matrix(pose_cov):
    """[..., 6] lower triangles -> [..., 3, 3] symmetric matrices."""
    c = np.asarray(pose_cov, np.float64)
    P = np.empty(c.shape[:-1] + (3, 3))
    for k, (i, j) in enumerate(((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))):
        P[..., i, j] = c[..., k]
        P[..., j, i] = c[..., k]
    return P


def pose_nees(poses, pose_cov, truth):
    """Normalised estimation error squared of the pose, e^T P^-1 e with e = pose - truth and the heading error wrapped.
    poses, truth: [..., 3] (x, y, heading); pose_cov: [..., 6].  Chi-square with 3 degrees of freedom for a consistent filter.
    NaN where the covariance is NaN or singular."""
    e = np.asarray(poses, np.float64) - np.asarray(truth, np.float64)
    e[..., 2] = wrap_angle(e[..., 2])
    P = pose_cov_matrix(pose_cov)
    out = np.full(e.shape[:-1], np.nan)
    ok = np.isfinite(P).all(axis=(-1, -2)) & np.isfinite(e).all(axis=-1)
    with np.errstate(all="ignore"):
        ok &= np.abs(np.linalg.det(np.where(ok[..., None, None], P, np.eye(3)))) > 0.0
    if ok.any():
        x = np.linalg.solve(P[ok], e[ok][..., None])[..., 0]
        out[ok] = np.einsum("...i,...i->...", e[ok], x)
    return out
