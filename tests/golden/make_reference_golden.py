"""Record tests/golden/reference/*.npz from the reference's own nodes.

Needs oracle/_ref (`make -C oracle ref`, or __graft_entry__.build(), with a checkout of the reference).  Unlike the
self-generated fixtures of make_golden.py these are the outputs of the reference's unmodified source text, compiled over
oracle/ref_shim: the oracles, and through them the kernels, are held against them wherever the reference itself is absent
(tests/test_reference_parity.py, tests/test_gpu_reference.py).  A fixture is data only: the input and the recorded outputs,
in the field layout of the other fixtures.

    python tests/golden/make_reference_golden.py      (re-run only when the cases in tests/reference_cases.py change)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import reference_cases as rc  # noqa: E402
from oracle import ref_oracle  # noqa: E402

OUT = os.path.join(HERE, "reference")


def record_filter(name):
    """-> the script plus the reference's outputs.  Every UKF case must keep the reference's own P finite and positive
    definite at every callback: what llt() does on an indefinite matrix is Eigen's business and is not pinned here."""
    sc = rc.FILTER_CASES[name]()
    f = ref_oracle.RefFilter(sc["kind"], 30, now_init=sc.get("now_init", 0.0))

    def pd(t, f):
        P = f.P
        assert np.isfinite(P).all() and np.linalg.eigvalsh((P + P.T) / 2).min() > 0, (name, t)

    out = rc.run_script(f, sc, on_step=pd if sc["kind"] == "ukf" else None)
    assert f.dt_mismatches() == 0, name        # the clock handed to the node gave back the trace's delta_time bit for bit
    assert np.isfinite(out["P"]).all() and np.isfinite(out["X"]).all(), name
    if sc["kind"] == "ekf":
        out["A"] = np.array(f.A())
    out["last_time"] = f.last_time()
    return {**sc, **out}


def record_scans():
    ranges, where, names = rc.scan_cases()
    assert ref_oracle.scan_left_to_right(), "the scan node must pair beam theta with table entry theta (oracle/Makefile)"
    st, n, rg, bg = ref_oracle.scan(ranges, max_out=32)
    return dict(ranges=ranges, status=st, n=n, range=rg, bearing=bg, constructed_names=np.array(names),
                **{"group_" + k: np.array([v.start, v.stop]) for k, v in where.items()})


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    for name in rc.FILTER_CASES:
        out = record_filter(name)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(name, "T =", len(out["dt"]), "N =", out["X"].shape[0], "bytes", os.path.getsize(path))
    out = record_scans()
    path = os.path.join(OUT, "scan.npz")
    np.savez_compressed(path, **out)
    print("scan:", len(out["ranges"]), "scans,", int(out["n"].sum()), "landmarks,", int((out["status"] == 1).sum()),
          "asserts, bytes", os.path.getsize(path))
