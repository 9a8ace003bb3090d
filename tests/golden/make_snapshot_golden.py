"""Writes tests/golden/snapshot_v1_ekf.bin: a two-record EKF snapshot (n = 3 and n = 7) that pins version 1 of the format of
include/aslam_snapshot.h.  The records are made up (no filter ever held them) and exactly representable, so the file does not depend on
the platform; tests/test_snapshot_host.py rebuilds them through golden_records() and compares.

    python tests/golden/make_snapshot_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from awesomeslam_amd import snapshot  # noqa: E402

PATH = os.path.join(HERE, "snapshot_v1_ekf.bin")


def golden_records():
    # a filter before its first callback: both init flags, A = identity's first column, nothing stored
    r0 = dict(n=3, flags=snapshot.INIT_X | snapshot.INIT_Z, status=0, A=np.array([1.0, 0.0]), X=np.zeros(3), Z=np.zeros(3),
              P=np.eye(3) * 0.5, sens=np.zeros((0, 2), np.float32), wait_rb=np.zeros((0, 2), np.float32), wait_cnt=np.zeros(0, np.uint32))
    # two landmarks, an UNSYMMETRIC P (the record is lossless for it), a stored message of three, a wait-list of two, two status bits
    n = 7
    P = (np.arange(n * n, dtype=np.float64).reshape(n, n) - 24.0) / 64.0
    r1 = dict(n=n, flags=0, status=1 | 8, A=np.array([0.75, -0.125]), X=np.arange(n) * 0.25 - 1.0, Z=np.arange(n) * -0.5 + 2.0, P=P,
              sens=np.array([[1.5, 0.25], [2.25, -0.5], [3.0, 0.125]], np.float32),
              wait_rb=np.array([[4.5, 1.0], [5.25, -1.25]], np.float32), wait_cnt=np.array([3, 9], np.uint32))
    return [r0, r1]


if __name__ == "__main__":
    blob = snapshot.pack(golden_records(), "ekf")
    blob.tofile(PATH)
    print(f"{PATH}: {blob.size} bytes")
