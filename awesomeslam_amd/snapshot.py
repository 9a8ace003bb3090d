"""The snapshot format of include/aslam_snapshot.h (version 1) in pure NumPy: no GPU and no shared library needed.

    record_bytes(n, sens_n, wait_n)   exact bytes of one record (header + body)
    parse(blob)                       -> list of dicts, one per record
    pack(records, filter)             -> blob (uint8 array); parse(pack(x)) == x bit for bit
    blob_info(blob)                   -> (filter, count, total_bytes) of the blob header

A record dict: n, flags (INIT_X | INIT_Z), status (core.ST_* bits), A (float64[2]: A(0,0), A(1,0)), X, Z (float64[n]), P (float64[n, n], the
full matrix), sens (float32[sens_n, 2]: range, bearing of the stored sensor message), wait_rb (float32[wait_n, 2]), wait_cnt (uint32[wait_n]).
"""
import numpy as np

MAGIC = b"ASLSNP01"
VERSION = 1
INIT_X, INIT_Z = 1, 2
KNOWN_FLAGS = INIT_X | INIT_Z
KNOWN_STATUS = 31
FIELDS = ("n", "flags", "status", "A", "X", "Z", "P", "sens", "wait_rb", "wait_cnt")


def _pad64(x):
    return (int(x) + 63) & ~63


def record_bytes(n, sens_n, wait_n):
    n, sens_n, wait_n = int(n), int(sens_n), int(wait_n)
    if n < 3 or n % 2 == 0 or sens_n < 0 or wait_n < 0:
        raise ValueError("n must be 3 + 2k, counts must not be negative")
    return 64 + 8 * (n + 1) * (n + 2) + 8 * sens_n + 12 * wait_n


def blob_info(blob):
    b = np.ascontiguousarray(blob, np.uint8).reshape(-1)
    if b.size < 64 or b[:8].tobytes() != MAGIC:
        raise ValueError("not a snapshot (magic)")
    version, filt, count, _ = (int(v) for v in b[8:24].view("<u4"))
    total = int(b[24:32].view("<u8")[0])
    if version != VERSION:
        raise ValueError(f"snapshot version {version}, this reader knows {VERSION}")
    if total > b.size or total < 64 + _pad64(8 * count):
        raise ValueError("snapshot truncated")
    return filt, count, total


def parse(blob):
    b = np.ascontiguousarray(blob, np.uint8).reshape(-1)
    _, count, total = blob_info(b)
    offs = b[64:64 + 8 * count].view("<u8")
    out = []
    for off in (int(o) for o in offs):
        if off % 64 or off + 64 > total:
            raise ValueError("record offset unaligned or outside the blob")
        n, flags, status, sens_n, wait_n, ld = (int(v) for v in b[off:off + 24].view("<i4"))
        status &= 0xFFFFFFFF
        if n < 3 or n % 2 == 0 or ld != n + 1 or sens_n < 0 or wait_n < 0 or off + record_bytes(n, sens_n, wait_n) > total:
            raise ValueError("malformed record header")
        p = off + 64
        take = lambda cnt, dt: (b[p:p + cnt * np.dtype(dt).itemsize].view(dt).copy(), p + cnt * np.dtype(dt).itemsize)  # noqa: E731
        A = b[off + 32:off + 48].view("<f8").copy()
        X, p = take(ld, "<f8")
        Z, p = take(ld, "<f8")
        P, p = take(n * ld, "<f8")
        sens, p = take(2 * sens_n, "<f4")
        wrb, p = take(2 * wait_n, "<f4")
        wcnt, p = take(wait_n, "<u4")
        out.append(dict(n=n, flags=flags, status=status, A=A, X=X[:n], Z=Z[:n], P=P.reshape(n, ld)[:, :n].copy(),
                        sens=sens.reshape(sens_n, 2), wait_rb=wrb.reshape(wait_n, 2), wait_cnt=wcnt))
    return out


def pack(records, filter):
    """`filter`: core.EKF / core.UKF (0 / 1) or "ekf" / "ukf"."""
    filt = {"ekf": 0, "ukf": 1}.get(filter, filter)
    count = len(records)
    offs, off = [], 64 + _pad64(8 * count)
    for r in records:
        offs.append(off)
        off += _pad64(record_bytes(r["n"], len(r["sens"]), len(r["wait_cnt"])))
    b = np.zeros(off, np.uint8)
    b[:8] = np.frombuffer(MAGIC, np.uint8)
    b[8:24].view("<u4")[:] = (VERSION, filt, count, 0)
    b[24:32].view("<u8")[0] = off
    b[64:64 + 8 * count].view("<u8")[:] = offs
    for r, o in zip(records, offs):
        n = int(r["n"])
        ld = n + 1
        sens = np.asarray(r["sens"], "<f4").reshape(-1, 2)
        wrb = np.asarray(r["wait_rb"], "<f4").reshape(-1, 2)
        wcnt = np.asarray(r["wait_cnt"], "<u4").reshape(-1)
        if len(wrb) != len(wcnt):
            raise ValueError("wait_rb and wait_cnt differ in length")
        b[o:o + 24].view("<i4")[:] = (n, int(r["flags"]), np.uint32(r["status"]).view(np.int32), len(sens), len(wcnt), ld)
        b[o + 32:o + 48].view("<f8")[:] = np.asarray(r["A"], "<f8").reshape(2)
        p = o + 64
        for v in (r["X"], r["Z"]):
            b[p:p + 8 * n].view("<f8")[:] = np.asarray(v, "<f8").reshape(n)
            p += 8 * ld
        Pm = np.zeros((n, ld), "<f8")
        Pm[:, :n] = np.asarray(r["P"], "<f8").reshape(n, n)
        for a in (Pm, sens, wrb, wcnt):
            raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
            b[p:p + raw.size] = raw
            p += raw.size
    return b


def records_equal(a, b):
    """bit for bit (NaNs compare by their bits)"""
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() and np.asarray(a[k]).shape == np.asarray(b[k]).shape for k in FIELDS)
