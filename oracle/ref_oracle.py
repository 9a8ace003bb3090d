"""ctypes binding of oracle/_ref/libaslam_ref_{ekf,ukf,scan}.so: the reference's own nodes, compiled unmodified over
oracle/ref_shim by `make -C oracle ref` (which needs a checkout of the reference).  TEST INFRASTRUCTURE ONLY.

The filter libraries export the orc_* interface of aslam_oracle.h, so RefFilter is CFilter over another library: the same
replay(), state(), wait_list(), set_state() and slam().  A reference filter exists for the shipped MAX_LANDMARK_COUNT = 30 only."""
import ctypes
import os

import numpy as np

from . import c_oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
_libs = {}


def path(which):
    return os.path.join(REF_DIR, f"libaslam_ref_{which}.so")


def available(which):
    return os.path.exists(path(which))


def lib(which):
    if which not in _libs:
        if which == "scan":
            L = ctypes.CDLL(path(which))
            c_fp, c_ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
            L.ref_scan.restype = None
            L.ref_scan.argtypes = [ctypes.c_int64, c_fp, ctypes.c_int, c_ip, c_ip, c_fp, c_fp]
            L.ref_scan_left_to_right.restype = ctypes.c_int
        else:
            L = c_oracle.bind(path(which))
            L.ref_create_at.restype = ctypes.c_void_p
            L.ref_create_at.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double]
            L.ref_odom_at.restype = ctypes.c_int
            L.ref_odom_at.argtypes = [ctypes.c_void_p] + [ctypes.c_double] * 9
            L.ref_dt_mismatches.restype = ctypes.c_int64
            L.ref_dt_mismatches.argtypes = [ctypes.c_void_p]
            L.ref_last_time.restype = ctypes.c_float
            L.ref_last_time.argtypes = [ctypes.c_void_p]
        _libs[which] = L
    return _libs[which]


class RefFilter(c_oracle.CFilter):
    """aslam::EKFSlam / aslam::UKFSlam themselves.  now_init: the clock value at which the node is constructed."""

    def __init__(self, kind, max_landmark_count=30, now_init=0.0):
        self.kind = kind
        self._L = lib(kind)
        self._h = self._L.ref_create_at(c_oracle._KIND[kind], int(max_landmark_count), float(now_init))
        if not self._h:
            raise ValueError(f"the reference has no {kind} filter with max_landmark_count={max_landmark_count} in this library")

    def odom_msg_now(self, odom, now):
        """an odom message delivered at the absolute clock value `now`: the node derives delta_time itself"""
        return self._L.ref_odom_at(self._h, *[float(v) for v in odom], float(now))

    def dt_mismatches(self):
        """callbacks of replay()/odom_msg() at which the node's own delta_time was not, bit for bit, the dt handed in"""
        return int(self._L.ref_dt_mismatches(self._h))

    def last_time(self):
        return np.float32(self._L.ref_last_time(self._h))


def scan_left_to_right():
    """True when the scan library pairs beam theta with table entry theta (see oracle/Makefile)."""
    return bool(lib("scan").ref_scan_left_to_right())


def scan(ranges, max_out=64):
    """ranges [count, 360] -> status [count], n [count], range [count, max_out], bearing [count, max_out] (binary32)"""
    r = np.ascontiguousarray(ranges, np.float32).reshape(-1, 360)
    count = r.shape[0]
    st, n = np.zeros(count, np.int32), np.zeros(count, np.int32)
    rg, bg = np.zeros((count, max_out), np.float32), np.zeros((count, max_out), np.float32)
    c_fp, c_ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    lib("scan").ref_scan(count, r.ctypes.data_as(c_fp), max_out, st.ctypes.data_as(c_ip), n.ctypes.data_as(c_ip),
                         rg.ctypes.data_as(c_fp), bg.ctypes.data_as(c_fp))
    assert n.max(initial=0) <= max_out, "max_out too small for this scan"
    return st, n, rg, bg
