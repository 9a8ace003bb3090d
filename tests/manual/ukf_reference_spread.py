"""How far two binary64 evaluations of one UKF step lie apart: oracle.c_oracle.CFilter("ukf") (plain C++, k-ascending sums, LU inverse)
against oracle.np_oracle.NpFilter("ukf") (BLAS / LAPACK) on the states and input ranges of tests/test_gpu_ukf_large_shapes.py.  CPU only.
UKF_STEP_TOL of that file is 10 x the worst figure of this table, rounded up to one digit (its docstring holds the table).

With --replay SEED: the same spread over the 13 delayed trajectories of that file's replay test (L = 80, T = 70), per trajectory, with the
first callback at which the two pose streams part by more than 1e-10.  The reference rounds every heading / bearing difference to binary32
inside normalizeAngle; a last-bit difference of a binary64 sum that lands on the other side of such a rounding boundary moves that entry by
6e-8 of its value, and the negative central weight amplifies it.  A trajectory on which the two ORACLES part by more than the replay bar
cannot be held against a device at that bar: the test's seed is one for which they do not (its docstring holds the figures).

    python tests/manual/ukf_reference_spread.py [--replay SEED]          (from the repository root; one to two minutes)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle.c_oracle import CFilter  # noqa: E402
from oracle.np_oracle import NpFilter  # noqa: E402
from test_gpu_batch_shapes import step_inputs  # noqa: E402
from test_gpu_ukf_large import synth  # noqa: E402
from util import block_rel_err, cov_err, rel_err  # noqa: E402

CASES = ((31, 2), (145, 2), (255, 2), (317, 2), (515, 1), (771, 1), (1085, 1))


def spread(n, steps, seed):
    """(worst rel_err(X) over the steps, cov_err(P) after the last, the blocks of that P, the smallest den)"""
    st = {n: synth(n, n)}
    inp = step_inputs("ukf", [n], st, seed, steps=steps)
    X, Z, P = st[n]
    c, f = CFilter("ukf", n + 1), NpFilter("ukf", n + 1)
    f.set_state(n, X, Z, P)
    ex, den = 0.0, 1.0
    for vx, az, dt, _, _, Zs in inp:
        # CFilter takes Z through set_state only: hand its own state back with this step's readings (binary64 both ways: nothing is rounded)
        c.set_state(n, X, Zs[0, :n], P)
        f.Z = Zs[0, :n].copy()
        c.slam(vx[0], az[0], dt[0])
        f.slam(vx[0], az[0], dt[0])
        X, _, P = c.state()
        ex, den = max(ex, rel_err(f.X, X)), min(den, f.sm_den)
    return ex, cov_err(f.P, P), block_rel_err(f.P, P), den


def replay_spread(seed, L=80, T=70, B=13):
    from awesomeslam_amd import trace as tg
    from test_gpu_batch_shapes import delayed_trace

    tr, ks = delayed_trace(L, T, B, seed, 0)
    print("| filter | first message | N | pose stream | X | P | poses part at callback |")
    print("|---|---|---|---|---|---|---|")
    worst = 0.0
    for b in range(B):
        c, f = CFilter("ukf", tg.dim_cap(L)), NpFilter("ukf", tg.dim_cap(L))
        pc, dc = c.replay(tr[b])
        pf, df = f.replay(tr[b])
        assert np.array_equal(dc, df)
        X, _, P = c.state()
        pd = bool(np.isfinite(P).all() and (c.N == 3 or np.linalg.eigvalsh((P + P.T) / 2).min() > 0))
        e = rel_err(pf, pc), rel_err(f.X, X), cov_err(f.P, P)
        apart = np.abs(pf - pc).max(axis=1) > 1e-10 * max(np.abs(pc).max(), 1e-300)
        worst = max(worst, *e)
        print(f"| {b} | {ks[b]} | {c.N} | {e[0]:.1e} | {e[1]:.1e} | {e[2]:.1e} | {int(np.argmax(apart)) if apart.any() else '-'} |"
              + ("" if pd else "   NOT POSITIVE DEFINITE"), flush=True)
    print(f"seed {seed}: worst spread {worst:.2e}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--replay":
        replay_spread(int(sys.argv[2]))
        sys.exit(0)
    worst = 0.0
    print("| n | steps | X | P | P blocks pose / cross / landmark | min den |")
    print("|---|---|---|---|---|---|")
    for n, steps in CASES:
        t0 = time.time()
        ex, ep, blocks, den = spread(n, steps, seed=1000 + n)
        worst = max(worst, ex, ep)
        print(f"| {n} | {steps} | {ex:.1e} | {ep:.1e} | {blocks[0]:.1e} / {blocks[1]:.1e} / {blocks[2]:.1e} | {den:.3f} |   ({time.time() - t0:.0f} s)", flush=True)
    print(f"worst spread {worst:.2e}; 10 x = {10 * worst:.2e}")
