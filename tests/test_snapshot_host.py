"""The snapshot format (include/aslam_snapshot.h, version 1) without a GPU: the exported symbols, the size formula, the NumPy reader and
writer against each other and against the golden file, and aslam_snapshot_check's refusals."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from awesomeslam_amd import core, snapshot
from test_abi import declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "snapshot_v1_ekf.bin")


def golden_records():
    spec = importlib.util.spec_from_file_location("make_snapshot_golden", os.path.join(ROOT, "tests", "golden", "make_snapshot_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.golden_records()


def check(blob, nbytes=None):
    """(return code, filter, count) of aslam_snapshot_check on a host array"""
    blob = np.ascontiguousarray(blob, np.uint8)
    f, c = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = core.core_lib().aslam_snapshot_check(blob.ctypes.data, blob.size if nbytes is None else nbytes, ctypes.byref(f), ctypes.byref(c))
    return rc, f.value, c.value


def test_snapshot_api_is_exported(built):
    names = declared(os.path.join(ROOT, "include", "aslam_snapshot.h"))
    assert sorted(names) == sorted(core.SNAPSHOT_SYMBOLS)
    lib = ctypes.CDLL(os.path.join(ROOT, "awesomeslam_amd", "csrc", "libaslam_core.so"))
    for n in names:
        assert hasattr(lib, n), n
    assert lib.aslam_abi_version() == 1  # the new header does not move the ABI version of aslam_core.h


@pytest.mark.parametrize("n", [3, 7, 143, 1085])
def test_record_bytes_matches_the_library(n, built):
    lib = core.core_lib()
    for sens_n, wait_n in ((0, 0), (1, 0), (0, 1), (5, 3), (16, 27), (128, 512), (1024, 2048)):
        want = 64 + 8 * (2 * (n + 1) + n * (n + 1)) + 8 * sens_n + 8 * wait_n + 4 * wait_n  # the sections of the header comment, one by one
        assert snapshot.record_bytes(n, sens_n, wait_n) == want
        assert lib.aslam_snapshot_record_bytes(n, sens_n, wait_n) == want
    assert lib.aslam_snapshot_record_bytes(n + 1, 0, 0) == -1 and lib.aslam_snapshot_record_bytes(n, -1, 0) == -1
    with pytest.raises(ValueError):
        snapshot.record_bytes(n + 1, 0, 0)


def random_records(rng, dims):
    out = []
    for n in dims:
        sn, wn = int(rng.integers(0, 9)), int(rng.integers(0, 12))
        X, Z, P = rng.normal(size=n), rng.normal(size=n), rng.normal(size=(n, n))  # P unsymmetric on purpose
        X[0], P[n - 1, n - 1], P[0, 1] = np.nan, -0.0, np.inf                       # bit for bit means these too
        out.append(dict(n=n, flags=int(rng.integers(0, 4)), status=int(rng.integers(0, 32)), A=rng.normal(size=2), X=X, Z=Z, P=P,
                        sens=rng.normal(size=(sn, 2)).astype(np.float32), wait_rb=rng.normal(size=(wn, 2)).astype(np.float32),
                        wait_cnt=rng.integers(0, 10, wn).astype(np.uint32)))
    return out


@pytest.mark.parametrize("filt", ["ekf", "ukf"])
def test_parse_inverts_pack(filt, built):
    recs = random_records(np.random.default_rng(11), [3, 7, 9, 143, 57, 3])
    blob = snapshot.pack(recs, filt)
    assert blob.dtype == np.uint8 and blob.size % 64 == 0
    back = snapshot.parse(blob)
    assert len(back) == len(recs)
    for a, b in zip(back, recs):
        assert snapshot.records_equal(a, b)
        assert a["P"].shape == (a["n"], a["n"]) and a["sens"].shape[1] == 2
    assert snapshot.pack(back, filt).tobytes() == blob.tobytes()
    assert snapshot.blob_info(blob) == (core.FILTERS[filt], len(recs), blob.size)
    # the library reads what the NumPy writer wrote, and every offset is 64-byte aligned
    assert check(blob) == (0, core.FILTERS[filt], len(recs))
    offs = blob[64:64 + 8 * len(recs)].view("<u8")
    assert not (offs % 64).any()
    sizes = [snapshot.record_bytes(r["n"], len(r["sens"]), len(r["wait_cnt"])) for r in recs]
    assert list(np.diff(offs)) == [(s + 63) // 64 * 64 for s in sizes[:-1]]


def test_golden_file_pins_version_1(built):
    blob = np.fromfile(GOLDEN, np.uint8)
    assert blob.size < 4096
    assert blob[:8].tobytes() == b"ASLSNP01" and blob[8:12].view("<u4")[0] == 1
    recs, want = snapshot.parse(blob), golden_records()
    assert [r["n"] for r in recs] == [3, 7]
    for a, b in zip(recs, want):
        assert snapshot.records_equal(a, b)
    r = recs[1]
    assert r["status"] == 9 and r["flags"] == 0 and r["A"].tolist() == [0.75, -0.125] and r["wait_cnt"].tolist() == [3, 9]
    assert r["P"][2, 5] == (2 * 7 + 5 - 24) / 64 and r["P"][5, 2] == (5 * 7 + 2 - 24) / 64  # the full matrix, not a triangle
    assert r["sens"].tolist() == [[1.5, 0.25], [2.25, -0.5], [3.0, 0.125]]
    assert snapshot.pack(want, "ekf").tobytes() == blob.tobytes()  # today's writer still writes version 1 byte for byte
    assert check(blob) == (0, core.EKF, 2)


def mutate(what):
    blob = np.fromfile(GOLDEN, np.uint8)
    off1 = int(blob[64:80].view("<u8")[1])
    nbytes = blob.size
    if what == "magic":
        blob[7] = ord("2")
    elif what == "version":
        blob[8:12].view("<u4")[0] = 2
    elif what == "offset-unaligned":
        blob[64:80].view("<u8")[1] = off1 + 8
    elif what == "offset-beyond":
        blob[64:80].view("<u8")[1] = (nbytes + 63) // 64 * 64
    elif what == "even-n":
        blob[off1:off1 + 4].view("<i4")[0] = 6
        blob[off1 + 20:off1 + 24].view("<i4")[0] = 7
    elif what == "status-bit":
        blob[off1 + 8:off1 + 12].view("<u4")[0] |= 1 << 9
    elif what == "truncated":
        nbytes -= 64
    return blob, nbytes


@pytest.mark.parametrize("what", ["magic", "version", "offset-unaligned", "offset-beyond", "even-n", "status-bit", "truncated"])
def test_check_refuses(what, built):
    blob, nbytes = mutate(what)
    rc, _, _ = check(blob, nbytes)
    assert rc == -1 and core.core_lib().aslam_last_error()  # ASLAM_ERR_ARG with a message
    assert check(np.fromfile(GOLDEN, np.uint8))[0] == 0     # ... and the file itself passes
