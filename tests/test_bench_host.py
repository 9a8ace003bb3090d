"""bench.py's host logic without a GPU: flop models, rank spawning, and that it refuses to run without a device."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flop_models():
    import bench

    n = 1027
    alg, exe = bench.algorithmic_flops("ekf", n), bench.executed_flops("ekf512", n)
    assert abs(alg - (7.0 / 3.0) * n ** 3) < 1.0
    # padded to 17 blocks of 64, panel product instead of a triangular solve: between 1.1x and 1.5x the algorithmic figure
    assert 1.1 * alg < exe < 1.5 * alg
    assert bench.executed_flops("ekf64", 131) == 144 ** 3
    assert bench.algorithmic_flops("ukf", 131) == 10.7 * 131 ** 3


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the refusal on a box without a GPU")
def test_bench_without_gpu_fails_loudly_also_through_the_spawner():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    for extra in ([], ["--gpus", "2"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "ekf8", "--steps", "1", "--warmup", "0"] + extra,
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode != 0
        assert b"needs a GPU" in r.stderr
        assert b'"metric"' not in r.stdout


def test_traffic_is_reported_only_for_the_kernel_it_was_measured_on():
    """roofline.traffic comes from a stored PMC measurement (profiles/pmc_traffic.json): it must be null, with a note, when the entry's
    "kernel" is not the chain this run launched (round-3 verdict: a changed chain must not report stale bytes silently)."""
    import json

    import bench

    ent = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))["ekf64"]
    r = bench.roofline("ekf64", 256, 500, 0.035, ent["kernel"])
    assert r["traffic"] == ent["hbm_bytes_per_launch"] and r["traffic_note"] is None and r["hbm"] is not None
    r = bench.roofline("ekf64", 128, 250, 0.035, ent["kernel"])
    assert r["traffic"] == ent["hbm_bytes_per_launch"] / 4  # scaled to the launch
    r = bench.roofline("ekf64", 256, 500, 0.035, "some_other_kernel<9,0>")
    assert r["traffic"] is None and r["hbm"] is None and "some_other_kernel" in r["traffic_note"]


def test_more_ranks_than_gpus_is_refused(monkeypatch):
    """`--gpus N` beyond torch.cuda.device_count() stops with a clear message before any rank is spawned (the first RCCL run is the
    driver's: two ranks on one device would hang in the communicator set-up); ASLAM_DIST_BACKEND=gloo is the rehearsal that shares devices."""
    import bench

    monkeypatch.delenv("ASLAM_DIST_BACKEND", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    monkeypatch.setattr(bench, "spawn_ranks", lambda n: pytest.fail("ranks were spawned"))
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "this node has 1 GPU(s)" in str(e.value)


@pytest.mark.parametrize("full", [False, True])
def test_plain_run_does_only_what_the_headline_needs(full, monkeypatch, capsys):
    """A plain run times the K steps and prints the headline line; the parity check, the batch-1 / PCIe legs, the sub-records and
    the CPU baselines run only under --full.  The GPU work itself (measure) is replaced by a stand-in."""
    import json

    import bench
    from awesomeslam_amd import dist as adist

    called = []

    def fake_measure(wl, B, C, K, W, *a, full=False, dump=None):
        called.append(("measure", K, W, full, dump))
        info = {"name": "k", "grid": 256, "block": 768, "lds_bytes": 0, "launch": None, "parity_check": {"ok": True} if full else None}
        return 0.5, 0.04, info, 0.0

    for name in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(adist, "finalize", lambda: None)
    monkeypatch.setattr(bench, "measure", fake_measure)
    for fn in ("sub_records", "single_trajectory_latency", "pcie_step_batch", "cpu_baseline", "cpu_baseline_all_cores"):
        monkeypatch.setattr(bench, fn, lambda *a, _fn=fn, **k: called.append(_fn) or {"from": _fn})
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "5", "--warmup", "2"] + (["--full"] if full else []))
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert called[0] == ("sub_records" if full else ("measure", 5, 2, False, None))
    assert ("measure", 5, 2, full, None) in called
    extras = {"sub_records", "single_trajectory_latency", "pcie_step_batch", "cpu_baseline", "cpu_baseline_all_cores"}
    assert set(c for c in called if isinstance(c, str)) == (extras if full else set())
    assert line["steps"] == 5 and line["warmup"] == 2 and abs(line["ms_per_step"] - 100.0) < 1e-9
    assert line["value"] == 256 * 20 * 5 / 0.5 and line["unit"] == "filter-steps/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["metric"] == "EKF/UKF filter-steps/s @ N_landmarks" and "roofline" in line
    for key in ("parity_check", "sub", "single_trajectory", "pcie_step_batch", "cpu_baseline", "cpu_baseline_all_cores"):
        assert (key in line) == full, key


def test_dump_sample_is_fixed_and_within_64_mb():
    """--dump-outputs: an array over its budget is cut to a seeded sample of filters, the same one every run; the budgets add up to 64 MB."""
    import bench

    assert sum(bench.DUMP_BUDGET.values()) <= 64 << 20
    n = 1027
    ids = bench.dump_filters("P", 256, 8 * n * n)
    assert len(ids) == 3 and list(ids) == sorted(set(ids)) and all(0 <= i < 256 for i in ids)
    assert list(ids) == list(bench.dump_filters("P", 256, 8 * n * n))
    assert list(bench.dump_filters("X", 256, 8 * n)) == list(range(256))
    assert len(bench.dump_filters("poses", 4096, 500 * 3 * 8)) * 500 * 3 * 8 <= bench.DUMP_BUDGET["poses"]
