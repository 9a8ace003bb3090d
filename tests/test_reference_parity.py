"""The oracles against the reference's own source text.

oracle/_ref holds the reference's three nodes compiled unmodified over oracle/ref_shim (`make -C oracle ref`; needs a checkout
of the reference).  tests/golden/reference/ holds what those libraries gave on the cases of tests/reference_cases.py
(tests/golden/make_reference_golden.py).

* fixture comparisons run everywhere: CFilter, NpFilter and scan_oracle against the recorded outputs;
* live comparisons skip where oracle/_ref is absent: the libraries must still give the recorded outputs, the oracles are
  compared with what the libraries give now, and the as-coded claims that tests/test_oracle_cross.py and tests/test_scan.py
  make about the reference are asserted on the reference itself.

Bars.  Integers and binary32 bookkeeping (dimension per callback, Z, wait list, scan status and counts) are exact.  Poses and
X within 1e-10, P within 1e-9 relative: the bars this suite already sets between independent binary64 evaluations of the same
algebra (tests/test_oracle_cross.py, tests/test_oracle_eigen.py); the shim's products, inverse() and llt() are plain-loop
forms of Eigen's algorithms, the oracles' are their own.  Scan range within 1e-5 relative, bearing within 1e-5 rad
(tests/test_scan.py).  The worst figure of every case is printed."""
import os

import numpy as np
import pytest

import reference_cases as rc
from awesomeslam_amd import trace as tg
from oracle import ref_oracle
from oracle import scan_oracle as so
from oracle.c_oracle import CFilter
from oracle.np_oracle import NpFilter
from util import cov_err, rel_err

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")
POSE_X_TOL, P_TOL = 1e-10, 1e-9
SCAN_R_TOL, SCAN_B_TOL = 1e-5, 1e-5
# recorded outputs against a rebuild of the same text with the same flags: only the host libm's last bit can differ
REBUILD_TOL = 1e-12

need_filters = pytest.mark.skipif(not (ref_oracle.available("ekf") and ref_oracle.available("ukf")),
                                  reason="oracle/_ref is absent (no checkout of the reference to build it from)")
need_scan = pytest.mark.skipif(not ref_oracle.available("scan"), reason="oracle/_ref/libaslam_ref_scan.so is absent")


def load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return {k: z[k] for k in z.files}


def assert_same_inputs(sc, fx, name):
    for k, v in sc.items():
        v = np.asarray(v)
        assert np.array_equal(v, fx[k], equal_nan=v.dtype.kind == "f"), f"{name}: fixture input `{k}` is not what reference_cases builds"


def assert_outputs(name, who, got, ref, tol_px=POSE_X_TOL, tol_p=P_TOL):
    """bookkeeping exact, poses / X / P within the bars; returns the figures"""
    assert np.array_equal(got["dims"], ref["dims"]), f"{name} {who}: dimension per callback"
    assert np.array_equal(got["Z"], ref["Z"]), f"{name} {who}: Z"
    for k in ("wait_range", "wait_bearing", "wait_count"):
        assert np.array_equal(got[k], ref[k], equal_nan=True), f"{name} {who}: {k}"
    ran = np.any(ref["poses"] != 0, axis=1)
    assert np.array_equal(np.any(got["poses"] != 0, axis=1), ran), f"{name} {who}: which callbacks ran"
    e = rel_err(got["poses"], ref["poses"]), rel_err(got["X"], ref["X"]), cov_err(got["P"], ref["P"])
    print(f"{name}: {who} vs reference  poses {e[0]:.2e}  X {e[1]:.2e}  P {e[2]:.2e}")
    assert e[0] < tol_px and e[1] < tol_px and e[2] < tol_p, (name, who, e)
    return e


def oracle_outputs(cls, sc):
    return rc.run_script(cls(str(sc["kind"]), 30), sc)


# ------------------------------------------------------------------------------------------------ fixtures: always
@pytest.mark.parametrize("name", list(rc.FILTER_CASES))
def test_oracles_against_recorded_reference(name, built):
    fx = load(name)
    sc = rc.FILTER_CASES[name]()
    assert_same_inputs(sc, fx, name)
    assert int(fx["cap"]) == 30 and len(fx["dt"]) <= 300
    c = CFilter(str(sc["kind"]), 30)
    out = rc.run_script(c, sc)
    assert_outputs(name, "C++ oracle", out, fx)
    if sc["kind"] == "ekf":
        assert np.array_equal(np.array(c.A()), fx["A"]), name     # host libm on both sides
    assert_outputs(name, "NumPy oracle", oracle_outputs(NpFilter, sc), fx)


CLOCKS = ("ekf_clock_0", "ekf_clock_100", "ekf_clock_epoch")


def test_recorded_clock_cases_depend_on_delta_time():
    """delta_time is a local of the reference's cbOdom: it shows in the outputs only, through the twist.  The three clock
    scripts are the same messages at three clock offsets; the robot drives in the last 28 callbacks, so the recordings must
    differ from each other (they were identical, and blind to delta_time, while the scripts stood still)."""
    fx = {n: load(n) for n in CLOCKS}
    for n in CLOCKS:
        o = fx[n]["odom"]
        assert np.count_nonzero((o[:, 6] != 0) & (o[:, 7] != 0)) >= 20 and o[-1, 6] != 0 and o[-1, 7] != 0
        assert fx[n]["last_time"] == np.float32(fx[n]["nows"][-1]) and fx[n]["last_time"].dtype == np.float32   # ekf.h:98
    assert float(fx["ekf_clock_epoch"]["last_time"]) == 1.7e9 != fx["ekf_clock_epoch"]["nows"][-1]   # binary32 spacing 128 s
    # clocks 0 and 100 differ only in how last_time rounds to binary32 (spacings up to 3.8e-6 s and 7.6e-6 s): visible, and small
    for k in ("poses", "X", "P"):
        assert not np.array_equal(fx["ekf_clock_0"][k], fx["ekf_clock_100"][k]), k
        assert rel_err(fx["ekf_clock_0"][k], fx["ekf_clock_100"][k]) < 1e-3, k
        # at epoch stamps every delta_time is 1 where the other two have 0.37 s steps
        assert rel_err(fx["ekf_clock_0"][k], fx["ekf_clock_epoch"][k]) > 1e-3, k
        assert rel_err(fx["ekf_clock_100"][k], fx["ekf_clock_epoch"][k]) > 1e-3, k


# another reading of ekf.cpp:80-81 -> the clock cases on which it gives another delta_time than min(now - float last_time, 1.0)
# and how far off the recording it must land at the least (the bars of the true reading are 1e-10 / 1e-9).  At stamps near 100 s
# a binary64 last_time moves delta_time by the binary32 rounding of the stamp only (<= 3.8e-6 s in 0.37 s)
OTHER_READINGS = [("double", "ekf_clock_epoch", 1e-4), ("double", "ekf_clock_100", 1e-8), ("unclamped", "ekf_clock_0", 1e-4),
                  ("unclamped", "ekf_clock_100", 1e-4), ("stored_first", "ekf_clock_0", 1e-4), ("stored_first", "ekf_clock_100", 1e-4)]


@pytest.mark.parametrize("reading,name,floor", OTHER_READINGS)
def test_other_readings_of_delta_time_do_not_reproduce_the_reference(reading, name, floor, built):
    """The fixture comparison above feeds the oracles the delta_time of OUR reading and meets the recording within 1e-10.  Fed
    the delta_time of another reading -- a binary64 last_time (0.37 s steps at epoch stamps where the reference clamps every
    step to 1), no clamp, last_time stored before the subtraction -- the same oracle misses the recording by far more than any
    bar here: the recording pins the reading."""
    fx = load(name)
    sc = rc.FILTER_CASES[name]()
    sc["dt"] = rc.clock_dt(sc, reading)
    assert not np.array_equal(sc["dt"], fx["dt"])
    c = CFilter("ekf", 30)
    out = rc.run_script(c, sc)
    errs = rel_err(out["poses"], fx["poses"]), rel_err(out["X"], fx["X"]), cov_err(out["P"], fx["P"])
    print(f"{name} read as `{reading}`: poses {errs[0]:.2e}  X {errs[1]:.2e}  P {errs[2]:.2e} away from the reference")
    assert min(errs) > floor, errs


def compare_scans(who, scan_fn, fx, idx=None):
    worst_r = worst_b = 0.0
    tot = 0
    for i in (range(len(fx["ranges"])) if idx is None else idx):
        st, r, b = scan_fn(fx["ranges"][i])
        n = int(fx["n"][i])
        assert st == fx["status"][i] and len(r) == n, (who, i, st, fx["status"][i], len(r), n)
        rr, rb = fx["range"][i, :n], fx["bearing"][i, :n]
        fin = np.isfinite(rr)
        # a cluster joined with first_cluster holds a non-finite point: a landmark is published, its values are not pinned
        assert np.array_equal(np.isfinite(r), fin) and np.array_equal(np.isfinite(b), np.isfinite(rb)), (who, i)
        if fin.any():
            assert np.all(rr[fin] > 0.1), (who, i)       # no centre at the robot itself, where a bearing means nothing
            er, eb = float(np.max(np.abs(r[fin] - rr[fin]) / rr[fin])), float(np.max(np.abs(b[fin] - rb[fin])))
            assert np.isfinite(er) and np.isfinite(eb), (who, i)
            worst_r, worst_b = max(worst_r, er), max(worst_b, eb)
        tot += n
    print(f"scan: {who} vs reference, {tot} landmarks: worst range {worst_r:.2e} relative, worst bearing {worst_b:.2e} rad")
    assert worst_r < SCAN_R_TOL and worst_b < SCAN_B_TOL
    return tot


def test_scan_oracle_against_recorded_reference():
    fx = load("scan")
    ranges, where, names = rc.scan_cases()
    assert np.array_equal(ranges, fx["ranges"], equal_nan=True) and list(fx["constructed_names"]) == names
    assert compare_scans("scan_oracle", so.scan, fx) > 1000


def constructed(fx, name):
    i = int(fx["group_constructed"][0]) + list(fx["constructed_names"]).index(name)
    n = int(fx["n"][i])
    return int(fx["status"][i]), fx["range"][i, :n], fx["bearing"][i, :n]


def test_recorded_scan_quirks():
    """What tests/test_scan.py::test_oracle_as_coded_quirks claims, read off the reference's own outputs."""
    fx = load("scan")
    for name in ("cluster_up_to_359", "small_cluster", "wall", "empty", "all_nan"):
        st, r, _ = constructed(fx, name)
        assert st == so.ST_OK and len(r) == 0, name
    # assert(theta < 359) fails only when the walk from beam 0 meets no beam without a return before beam 358 ...
    assert constructed(fx, "ring_all_finite")[0] == so.ST_REF_ABORT
    assert constructed(fx, "ring_open_at_358")[0] == so.ST_REF_ABORT
    assert constructed(fx, "ring_open_at_357")[0] == so.ST_OK and constructed(fx, "ring_open_at_356")[0] == so.ST_OK
    # ... an obstacle dead ahead with free space beside it does not abort: the walk ends at the first beam without a return,
    # the beams before it are in no cluster, and the other cylinders are found
    st, r, _ = constructed(fx, "dead_ahead")
    assert st == so.ST_OK and len(r) == 0
    st, r, b = constructed(fx, "dead_ahead_with_others")
    assert st == so.ST_OK and len(r) == 3 and np.allclose(r, 2.5, atol=0.03)
    # a cluster broken by beam 359 itself is joined with first_cluster, whose last point is not finite
    st, r, b = constructed(fx, "dead_ahead_joined")
    assert st == so.ST_OK and len(r) == 4 and np.isfinite(r[:3]).all() and not np.isfinite(r[3])
    # the scan of tests/test_gpu_reference.py's run-loop test
    i = int(fx["group_many_runs"][0])
    assert fx["status"][i] == 0 and fx["n"][i] == 5


# ------------------------------------------------------------------------------------------------ live: need oracle/_ref
@need_filters
@pytest.mark.parametrize("name", list(rc.FILTER_CASES))
def test_live_reference_filters(name, built):
    fx = load(name)
    sc = rc.FILTER_CASES[name]()
    f = ref_oracle.RefFilter(str(sc["kind"]), 30, now_init=float(sc.get("now_init", 0.0)))
    live = rc.run_script(f, sc)
    assert f.dt_mismatches() == 0
    assert_outputs(name, "rebuilt reference", live, fx, REBUILD_TOL, REBUILD_TOL)
    assert f.last_time() == fx["last_time"]
    assert_outputs(name, "C++ oracle (live)", oracle_outputs(CFilter, sc), live)
    assert_outputs(name, "NumPy oracle (live)", oracle_outputs(NpFilter, sc), live)


@need_filters
def test_reference_refuses_growth_at_cap():
    """tests/test_oracle_cross.py::test_growth_refused_at_cap on the reference: `N >= MAX_LANDMARK_COUNT` (ekf.cpp:263) compares
    the DIMENSION with 30, and a refused batch is dropped whole."""
    for kind in ("ekf", "ukf"):
        f = ref_oracle.RefFilter(kind)
        _, dims = f.replay(tg.make_traces(14, 120, B=1, seed=9, stages=1)[0])
        assert dims[-1] == 3, kind                # 3 + 28 = 31 >= 30
        f = ref_oracle.RefFilter(kind)
        _, dims = f.replay(tg.make_traces(13, 120, B=1, seed=9, stages=1)[0])
        assert dims[-1] == 29, kind


@need_filters
def test_reference_drops_callbacks_before_the_first_sensor_message():
    tr = tg.make_traces(5, 30, B=1, seed=10)[0]
    for kind in ("ekf", "ukf"):
        f = ref_oracle.RefFilter(kind)
        assert f.odom_msg(*tr.odom[0], 1.0) == 0 and f.N == 3 and np.all(f.X == 0)
        f.sensor_msg([], [])
        assert f.odom_msg(*tr.odom[0], 1.0) == 1 and f.N == 3


@need_filters
def test_reference_growth_uses_the_ukf_constants_in_the_ekf():
    """ekf.cpp:277-278: a grown EKF gets UKF_KP_LANDMARK_POSE = 1.0 on the new diagonal of P, not EKF_KP_LANDMARK_POSE = 1e4.
    One landmark at 5 m is promoted and updated once in the same callback (R = 0.2 on range and bearing).  From a prior of 1.0
    the landmark block's trace comes out near 1/1.2 * (0.2 + 25 * 0.04) = 1.0; from 1e4 it would be near 0.2 * (1 + 25) = 5.2."""
    f = ref_oracle.RefFilter("ekf")
    f.set_state(3, np.zeros(3), np.zeros(3), np.eye(3) * 1e-3)
    odom = [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    for _ in range(10):
        f.sensor_msg([5.0], [0.25])
        f.odom_msg(*odom, 0.5)
    assert f.N == 5
    c = CFilter("ekf", 30)
    c.set_state(3, np.zeros(3), np.zeros(3), np.eye(3) * 1e-3)
    for _ in range(10):
        c.sensor_msg([5.0], [0.25])
        c.odom_msg(*odom, 0.5)
    assert c.N == 5 and np.array_equal(c.Z, f.Z) and rel_err(c.P, f.P) < P_TOL
    assert 0.5 < f.P[3, 3] + f.P[4, 4] < 1.5, f.P[3:5, 3:5]


@need_scan
def test_live_reference_scan():
    assert ref_oracle.scan_left_to_right(), "built with a compiler that pairs beam theta with table entry theta + 1 (oracle/Makefile)"
    fx = load("scan")
    st, n, rg, bg = ref_oracle.scan(fx["ranges"], max_out=32)
    assert np.array_equal(st, fx["status"]) and np.array_equal(n, fx["n"])
    fin = np.isfinite(fx["range"])
    assert np.array_equal(np.isfinite(rg), fin)
    assert np.allclose(rg[fin], fx["range"][fin], rtol=1e-6, atol=0) and np.allclose(bg[fin], fx["bearing"][fin], rtol=0, atol=1e-6)
    live = dict(fx, status=st, n=n, range=rg, bearing=bg)
    compare_scans("scan_oracle (live)", so.scan, live)
