"""How a build of the reference's scan node with another compiler differs from the recording ("Argument order").

    cp -r oracle /tmp/oracle_gxx && make -B -C /tmp/oracle_gxx ref REF_SCAN_CXX=g++
    python tests/manual/scan_argument_order.py /tmp/oracle_gxx/_ref/libaslam_ref_scan.so

`bearing2pose(theta, msg->ranges[theta++])` (sensor_landmark.cpp:75,84,94): g++ hands the first argument theta + 1.  Prints
which order the library got, how many of the 200 random scans of tests/golden/reference/scan.npz (recorded left to right) keep
their landmark count, and on those the bearing shift and the worst relative range difference.  CPU only."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
fx = np.load(os.path.join(HERE, "..", "golden", "reference", "scan.npz"))
L = ctypes.CDLL(sys.argv[1])
c_fp, c_ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
L.ref_scan.restype = None
L.ref_scan.argtypes = [ctypes.c_int64, c_fp, ctypes.c_int, c_ip, c_ip, c_fp, c_fp]
print("left to right:", bool(L.ref_scan_left_to_right()))
lo, hi = fx["group_random"]
r = np.ascontiguousarray(fx["ranges"][lo:hi])
cnt, mo = len(r), fx["range"].shape[1]
st, n = np.zeros(cnt, np.int32), np.zeros(cnt, np.int32)
rg, bg = np.zeros((cnt, mo), np.float32), np.zeros((cnt, mo), np.float32)
L.ref_scan(cnt, r.ctypes.data_as(c_fp), mo, st.ctypes.data_as(c_ip), n.ctypes.data_as(c_ip), rg.ctypes.data_as(c_fp), bg.ctypes.data_as(c_fp))
same = n == fx["n"][lo:hi]
print(f"{int(same.sum())} of {cnt} scans with the recorded landmark count; status {np.bincount(st).tolist()}")
db, dr = [], []
for i in np.nonzero(same & (n > 0))[0]:
    k = n[i]
    f = np.isfinite(fx["range"][lo + i, :k]) & np.isfinite(rg[i, :k])
    db += list((bg[i, :k] - fx["bearing"][lo + i, :k])[f])
    dr += list((np.abs(rg[i, :k] - fx["range"][lo + i, :k]) / fx["range"][lo + i, :k])[f])
db = np.degrees((np.array(db) + np.pi) % (2 * np.pi) - np.pi)
print(f"bearing shift: median {np.median(db):.4f} deg, {db.min():.4f} .. {db.max():.4f}; range: worst {max(dr):.2e} relative")
