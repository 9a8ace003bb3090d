"""-m gpu: `bench.py --dump-outputs` writes what the timed launches computed -- the last step's pose stream and the final filter
states -- and two runs with the same arguments write the same arrays.  Checked against the CPU oracle on a small EKF workload."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from util import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(out, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "ASLAM_CHOL_RESIDENT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "ekf8", "--batch", "4", "--chunk", "50", "--steps", "2",
           "--warmup", "1", "--dump-outputs", str(out)] + list(extra)
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def test_dump_outputs_are_the_timed_path_and_reproducible(tmp_path, built):
    from awesomeslam_amd import trace as tg
    from oracle.c_oracle import CFilter

    line = run_bench(tmp_path / "a")
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and "parity_check" not in line and "cpu_baseline" not in line
    run_bench(tmp_path / "b")
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["P.npy", "X.npy", "Z.npy", "poses.npy"] and sorted(os.listdir(tmp_path / "b")) == names
    d = {k[:-4]: np.load(tmp_path / "a" / k) for k in names}
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    assert all(a.dtype == np.float64 for a in d.values())
    for k in names:
        assert np.array_equal(np.load(tmp_path / "b" / k), d[k[:-4]], equal_nan=True), k
    L, C, B = 8, 50, 4
    n = tg.full_dim(L)
    assert d["poses"].shape == (B, C, 3) and d["X"].shape == (B, n) and d["P"].shape == (B, n, n)
    tr = tg.make_traces(L, 64 + 3 * C, B=B, seed=1)  # bench.py: 64-callback prologue, 1 warm-up + 2 timed steps of C callbacks
    for b in range(B):
        o = CFilter("ekf", tg.dim_cap(L))
        po, _ = o.replay(tr[b])
        Xo, Zo, Po = o.state()
        assert rel_err(d["poses"][b], po[-C:]) < 1e-6, b
        assert np.array_equal(d["Z"][b], Zo) and rel_err(d["X"][b], Xo) < 1e-6 and rel_err(d["P"][b], Po) < 1e-6, b
