"""The run-time parameters without a GPU: the C structure and its defaults, validation, the Python round trip, the reference helper at the
defaults, and the ROS wrappers with their new parameter reads."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from awesomeslam_amd import trace as tg
from oracle.np_oracle import NpFilter
from params_ref import DEFAULTS, FIELDS, SETS, ParamFilter, full

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "awesomeslam_amd", "csrc")
STUB = os.path.join(ROOT, "tests", "ros_stub")
f32 = np.float32


def bits(x):
    return struct.pack("<d", float(x))


def test_struct_is_80_bytes_and_defaults_are_the_widened_constants(built):
    from awesomeslam_amd import core

    assert ctypes.sizeof(core.Params) == 80
    assert tuple(k for k, _ in core.Params._fields_) == FIELDS
    p = core.default_params()
    want = dict(r_xy=f32(0.2), r_yaw=f32(0.2), r_range=f32(0.2), r_bearing=f32(0.2), q_xy=f32(0.001), q_yaw=f32(0.001), p0_pose=f32(0.001),
                p0_landmark=1.0, var_a=f32(f32(0.2) * f32(0.2)))
    for k, v in want.items():
        assert bits(getattr(p, k)) == bits(v), k  # to the bit: the value the reference's binary32 constant widens to
        assert bits(DEFAULTS[k]) == bits(v), k
    assert p.assoc_dist == 0.5 and p.promote_count == 10
    assert p.as_dict() == DEFAULTS


@pytest.mark.parametrize("field,value,ok", [(k, v, False) for k in FIELDS[:9] + ("assoc_dist",) for v in (float("nan"), float("inf"), -1.0)] +
                         [(k, 0.0, False) for k in ("r_xy", "r_yaw", "r_range", "r_bearing", "p0_pose", "p0_landmark", "var_a", "assoc_dist")] +
                         [("q_xy", 0.0, True), ("q_yaw", 0.0, True), ("promote_count", 0, False), ("promote_count", 1, True)])
def test_validation_names_the_field(field, value, ok, built):
    """a refused record is reported before the context is looked at, so this needs no device: a good record then fails on the null context"""
    from awesomeslam_amd import core

    lib = core.core_lib()
    p = core.Params.make({field: value})
    rc = lib.aslam_set_params(None, 0, ctypes.byref(p))
    msg = lib.aslam_last_error().decode()
    assert rc == -1  # ASLAM_ERR_ARG
    assert (field not in msg and "null context" in msg) if ok else (f"aslam_params.{field} " in msg), msg


def test_dict_round_trip(built):
    from awesomeslam_amd import core

    for name, s in SETS.items():
        p = core.Params.make(s)
        assert p.as_dict() == full(s), name
        q = core.Params.make(p)
        assert q is not p and q.as_dict() == p.as_dict()
    with pytest.raises(KeyError):
        core.Params.make(dict(r_xz=1.0))
    assert core.Params.make(None).as_dict() == DEFAULTS


@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_param_filter_with_defaults_is_the_oracle(kind):
    tr = tg.make_traces(5, 120, B=1, seed=41)[0]
    a, b = NpFilter(kind, tg.dim_cap(5)), ParamFilter(kind, tg.dim_cap(5))
    pa, da = a.replay(tr)
    pb, db = b.replay(tr)
    assert np.array_equal(pa, pb) and np.array_equal(da, db)
    assert np.array_equal(a.X, b.X) and np.array_equal(a.Z, b.Z) and np.array_equal(a.P, b.P) and a.wait == b.wait
    assert a.N == tg.full_dim(5)


def test_param_filter_restores_the_oracle_constants():
    from oracle import np_oracle

    keep = np_oracle.MIN_DIST_THRESH, np_oracle.MIN_LANDMARK_OCC, np_oracle.UKF_STD_A
    tr = tg.make_traces(5, 40, B=1, seed=41)[0]
    o = ParamFilter("ukf", tg.dim_cap(5), SETS["A"])
    o.replay(tr)
    assert (np_oracle.MIN_DIST_THRESH, np_oracle.MIN_LANDMARK_OCC, np_oracle.UKF_STD_A) == keep
    assert float(f32(o._std_a * o._std_a)) == SETS["A"]["var_a"] and o._std_a == f32(0.3)


@pytest.mark.parametrize("node", ["ekf", "ukf"])
def test_wrapper_with_parameter_reads_compiles_and_links(node, built, tmp_path):
    """tests/test_ros_wrappers.py's mechanism; besides: the wrapper reads every parameter by its name and hands the record to the mirror"""
    src = os.path.join(CSRC, "ros", f"{node}_node.cpp")
    obj, exe = str(tmp_path / f"{node}_node.o"), str(tmp_path / f"{node}_node")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{STUB}", f"-I{os.path.join(ROOT, 'include')}", "-c", src, "-o", obj],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    r = subprocess.run(["g++", "-o", exe, obj, f"-L{CSRC}", "-laslam_node", "-laslam_core", f"-Wl,-rpath,{CSRC}", "-Wl,--allow-shlib-undefined"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    syms = subprocess.run(["nm", "-u", "-C", exe], stdout=subprocess.PIPE, text=True).stdout
    assert "aslam::FilterNode::setParams(aslam_params const&)" in syms, syms
    text = open(os.path.join(CSRC, "ros", "node_main.h")).read()
    for k in FIELDS:
        assert f'ros::param::param("~{k}"' in text, k
