"""Map joining around Core.join_maps (aslam_join_maps, include/aslam_snapshot.h): host NumPy only, nothing here touches the GPU by itself.

    frame(tx, ty, phi, cov)              the (tx, ty, phi, cov3x3) tuple Core.join_maps takes: p' = t + R(phi) p, source frame -> destination
    align(xa, xb, pairs, cov_a, cov_b)   that transform, with its first-order covariance, from matched landmark pairs
    fuse(core, blob, ...)                join_maps followed by Core.merge_duplicates: stack two independent maps, then apply "these are the
                                         same point" to every gated pair -- textbook map joining

The join treats the two maps as INDEPENDENT.  Two filters that shared observations, or a fork joined back into its origin, are not: their
common information is then counted twice and the fused covariance is too small (covariance intersection is not implemented).
"""
import numpy as np


def frame(tx=0.0, ty=0.0, phi=0.0, cov=None):
    """(tx, ty, phi, cov): cov is the 3 x 3 covariance of (tx, ty, phi), zero when None; it must be exactly symmetric."""
    cov = np.zeros((3, 3)) if cov is None else np.array(cov, np.float64).reshape(3, 3)
    return float(tx), float(ty), float(phi), cov


def _blocks(cov, K):
    """[K, 2, 2] from None (zero), one 2 x 2, or one 2 x 2 per pair"""
    if cov is None:
        return np.zeros((K, 2, 2))
    return np.broadcast_to(np.asarray(cov, np.float64), (K, 2, 2))


def align(xa, xb, pairs, cov_a=None, cov_b=None):
    """The rigid 2-D transform that takes B's landmarks onto A's, from matched pairs: xa [La, 2] and xb [Lb, 2] are landmark coordinates,
    pairs is a list of (index into xa, index into xb).  Returns frame(tx, ty, phi, cov).

    Rotation and translation are the closed-form least-squares fit (no scale, equal weights): phi from the cross-covariance of the centred
    points, t = mean(a) - R mean(b).  cov is the first-order covariance (sum_k J_k^T W_k J_k)^-1 with J_k = [[1, 0, -s bx - c by],
    [0, 1, c bx - s by]] and W_k = (P_a,kk + R P_b,kk R^T)^-1; cov_a / cov_b are the landmarks' own 2 x 2 covariance blocks, one per pair in
    the order of `pairs` or one 2 x 2 for all; without either, W_k is the identity (cov is then the geometry alone, in units of one).

    Cross-landmark correlations and the correlation of the landmarks with their filters' poses are IGNORED here: cov is optimistic where
    they are strong.  And the pairs used for align carry information that a later merge of the same pairs uses AGAIN: align on a subset
    and merge the others, or inflate cov (or the merge's noise_var) accordingly."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    K = len(pairs)
    if K < 2:
        raise ValueError("align needs at least 2 pairs")
    a = np.asarray(xa, np.float64).reshape(-1, 2)[pairs[:, 0]]
    b = np.asarray(xb, np.float64).reshape(-1, 2)[pairs[:, 1]]
    ma, mb = a.mean(axis=0), b.mean(axis=0)
    ac, bc = a - ma, b - mb
    phi = float(np.arctan2(np.sum(bc[:, 0] * ac[:, 1] - bc[:, 1] * ac[:, 0]), np.sum(bc[:, 0] * ac[:, 0] + bc[:, 1] * ac[:, 1])))
    c, s = np.cos(phi), np.sin(phi)
    R = np.array([[c, -s], [s, c]])
    t = ma - R @ mb
    Pa, Pb = _blocks(cov_a, K), _blocks(cov_b, K)
    weighted = cov_a is not None or cov_b is not None
    info = np.zeros((3, 3))
    for k in range(K):
        J = np.array([[1.0, 0.0, -s * b[k, 0] - c * b[k, 1]], [0.0, 1.0, c * b[k, 0] - s * b[k, 1]]])
        W = np.linalg.inv(Pa[k] + R @ Pb[k] @ R.T) if weighted else np.eye(2)
        info += J.T @ W @ J
    cov = np.linalg.inv(info)
    return frame(t[0], t[1], phi, (cov + cov.T) / 2)


def fuse(core, blob, records, trajs, frames, gate, max_dist, noise_var=0.0):
    """Core.join_maps(blob, records, trajs, frames) followed by Core.merge_duplicates(gate, max_dist, noise_var) on the whole context.
    Returns (joined [count], merged [batch]).  A selected pair is (i, j) with i < j and the joined landmarks come last, so the
    destination's landmark keeps its index and the foreign one is removed.  Two shards of one run in the shared odometry frame take
    frames=None (identity frames, zero covariance)."""
    joined = core.join_maps(blob, records, trajs, frames)
    merged = core.merge_duplicates(gate, max_dist, noise_var)
    return joined, merged
