"""ctypes binding of libaslam_core.so / libaslam_node.so (include/aslam_core.h, csrc/host/aslam_node.h).

This is plumbing: every number comes out of the HIP kernels.  There is no CPU fallback -- if the shared
library is missing, or no HIP device is present, the calls raise (AslamError / OSError).
"""
import ctypes
import os
import subprocess

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
_CORE = os.path.join(_CSRC, "libaslam_core.so")
_NODE = os.path.join(_CSRC, "libaslam_node.so")

EKF, UKF = 0, 1
F64, F32 = 0, 1
FILTERS = {"ekf": EKF, "ukf": UKF}

ST_GROWTH_REFUSED, ST_WAIT_OVERFLOW, ST_NOT_PD, ST_OBS_OVERFLOW, ST_INTERNAL = 1, 2, 4, 8, 16
CFG_UKF_LARGE = 1  # aslam_config.flags: a UKF context beyond the single-CU kernels (state dimension 144 .. 1085), fp64 launch chain

# every symbol include/aslam_core.h declares (tests check the library exports them all)
CORE_SYMBOLS = (
    "aslam_create", "aslam_destroy", "aslam_reset", "aslam_last_error", "aslam_abi_version", "aslam_set_state",
    "aslam_grow", "aslam_ekf_step", "aslam_ukf_step", "aslam_ekf_step_batch", "aslam_ukf_step_batch", "aslam_set_trace", "aslam_replay", "aslam_get_dim",
    "aslam_get_state", "aslam_get_A", "aslam_get_landmarks", "aslam_get_wait", "aslam_get_status",
    "aslam_get_layout", "aslam_kernel_info", "aslam_get_launch_info", "aslam_get_syrk_tail",
    "aslam_replay_stats", "aslam_innovation_enable", "aslam_get_innovation",
    "aslam_params_default", "aslam_set_params", "aslam_get_params",
    "aslam_remove_landmarks", "aslam_select_beyond",
    "aslam_get_sightings", "aslam_select_stale",
    "aslam_sighted_update_enable", "aslam_get_sighted", "aslam_ekf_step_sighted", "aslam_ekf_step_batch_sighted",
    "aslam_merge_landmarks", "aslam_select_duplicates",
    "aslam_gate_observations", "aslam_joint_compat", "aslam_chi2_point",
    "aslam_set_replay_gate", "aslam_get_replay_gate", "aslam_get_assoc_rejected",
)
NODE_SYMBOLS = (
    "aslam_node_create", "aslam_node_create_at", "aslam_node_destroy", "aslam_node_error", "aslam_node_sensor", "aslam_node_odom",
    "aslam_node_odom_now", "aslam_node_dim", "aslam_node_get", "aslam_node_wait", "aslam_node_core",
    "aslam_host_narrow_odom", "aslam_node_enable_innovation", "aslam_node_innovation",
    "aslam_node_set_params", "aslam_node_get_params", "aslam_node_remove_landmarks",
    "aslam_node_get_sightings", "aslam_node_remove_stale", "aslam_node_set_sighted_only",
    "aslam_node_merge_landmarks", "aslam_node_merge_duplicates",
    "aslam_node_set_assoc_gate", "aslam_node_assoc_rejected", "aslam_node_set_joint_prob", "aslam_node_joint_rejected",
    "aslam_node_join_map",
)
TRACE_FILE_SYMBOLS = (
    "aslam_trace_file_open", "aslam_trace_file_close", "aslam_trace_file_error", "aslam_trace_file_dims",
    "aslam_trace_file_view", "aslam_trace_file_raw", "aslam_trace_file_write",
)


class AslamError(RuntimeError):
    pass


class Config(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in
                ("filter", "dtype", "max_landmark_count", "batch", "max_obs", "max_wait", "device", "flags")]


class TraceView(ctypes.Structure):
    _fields_ = [("T", ctypes.c_int64), ("max_obs", ctypes.c_int32), ("is_device", ctypes.c_int32),
                ("pose", ctypes.c_void_p), ("yaw", ctypes.c_void_p), ("twist", ctypes.c_void_p),
                ("dt", ctypes.c_void_p), ("obs_new", ctypes.c_void_p), ("n_obs", ctypes.c_void_p),
                ("obs", ctypes.c_void_p)]


class Params(ctypes.Structure):
    """aslam_params (include/aslam_core.h): the noise and association parameters of one filter.  80 bytes."""
    _fields_ = [(k, ctypes.c_double) for k in
                ("r_xy", "r_yaw", "r_range", "r_bearing", "q_xy", "q_yaw", "p0_pose", "p0_landmark", "var_a")] + \
               [("assoc_dist", ctypes.c_float), ("promote_count", ctypes.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

    @classmethod
    def make(cls, params=None):
        """A Params from a Params (copied), a dict of overrides of the defaults, or None (the defaults)."""
        if isinstance(params, cls):
            return cls.from_buffer_copy(params)
        p = default_params()
        names = {k for k, _ in cls._fields_}
        for k, v in (params or {}).items():
            if k not in names:
                raise KeyError(f"aslam_params has no field {k!r}")
            setattr(p, k, v)
        return p


class Frame(ctypes.Structure):
    """aslam_frame (include/aslam_snapshot.h): p' = t + R(phi) p with the covariance of (tx, ty, phi), row-major.  96 bytes."""
    _fields_ = [("tx", ctypes.c_double), ("ty", ctypes.c_double), ("phi", ctypes.c_double), ("cov", ctypes.c_double * 9)]

    @classmethod
    def make(cls, frame=None):
        """A Frame from a Frame, a (tx, ty, phi, cov3x3 or None) tuple, or None (the identity with zero covariance)."""
        if isinstance(frame, cls):
            return cls.from_buffer_copy(frame)
        tx, ty, phi, cov = (0.0, 0.0, 0.0, None) if frame is None else frame
        cov = np.zeros(9) if cov is None else np.asarray(cov, np.float64).reshape(9)
        return cls(float(tx), float(ty), float(phi), (ctypes.c_double * 9)(*cov))


def default_params():
    """The reference's constants (include/awesome_slam/config.h) as the library holds them: aslam_params_default."""
    p = Params()
    _chk(core_lib().aslam_params_default(ctypes.byref(p)))
    return p


_BUILT_HERE = False  # set by build() when THIS process's make run (re)compiled libaslam_core.so


def _sha256(path):
    import hashlib

    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()


def build(force=False, ukf=True):
    """Compile csrc/ for gfx950 (hipcc cross-compiles without a GPU): `make all`, which decides itself what is stale.  The Makefile scans
    the device assembly of the very compilation that produces libaslam_core.so (tools/check_spill_exec.py, check_agpr_strip.py,
    check_vmcnt_protocol.py), moves the library into place only when all guards are clean -- a library that failed one is never left where
    core_lib() would load it; GUARDS=0 installs under another name -- and THEN writes csrc/build_info.json (sha256 of the library, hash of
    the sources, guards, compiler, time) from the same rule, so the record always describes the file under the loader's name."""
    global _BUILT_HERE
    have_ukf = ukf and os.path.exists(os.path.join(_CSRC, "ukf_small.h"))
    before = _sha256(_CORE) if os.path.exists(_CORE) else None
    cmd = ["make", "-s", "-C", _CSRC, f"UKF={1 if have_ukf else 0}", "GUARDS=1"] + (["-B"] if force else []) + ["all"]
    subprocess.check_call(cmd)
    _BUILT_HERE = _BUILT_HERE or before != _sha256(_CORE)
    return _CORE, _NODE


def build_info():
    """The record the Makefile wrote for csrc/libaslam_core.so, CHECKED against the file that is there now: "matches_library" is True only
    when the sha256 in the record is the sha256 of the library core_lib() loads (False: the record describes some other binary -- the library
    was replaced behind the Makefile's back; None: no record).  "reused_here": this process did not compile it (it came with the snapshot)."""
    import json

    p = os.path.join(_CSRC, "build_info.json")
    try:
        info = json.load(open(p))
    except (OSError, ValueError):
        info = {"built": "unknown (no build_info.json: the library was not installed by csrc/Makefile)"}
    info.pop("sources", None)
    if "sha256" in info and os.path.exists(_CORE):
        info["matches_library"] = info["sha256"] == _sha256(_CORE)
        if not info["matches_library"]:
            info["built"] = "unknown (build_info.json does not describe the libaslam_core.so that is loaded)"
    else:
        info["matches_library"] = None
    info["reused_here"] = not _BUILT_HERE
    return info


_core = None
_node = None


def core_lib():
    global _core
    if _core is None:
        if not os.path.exists(_CORE):
            raise OSError(f"{_CORE} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback for the filter core)")
        # PyTorch-ROCm bundles its own HIP runtime (same SONAME as /opt/rocm's libamdhip64.so.7): it has to be in
        # the process first so that libaslam_core.so binds to that one copy instead of loading a second runtime
        import torch  # noqa: F401

        L = ctypes.CDLL(_CORE)
        vp, ci, cf, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
        pd, pf, pi, pu = (ctypes.POINTER(t) for t in (ctypes.c_double, ctypes.c_float, ctypes.c_int, ctypes.c_uint32))
        L.aslam_last_error.restype = ctypes.c_char_p
        L.aslam_create.argtypes = [ctypes.POINTER(Config), ctypes.POINTER(vp)]
        L.aslam_destroy.argtypes = [vp]
        L.aslam_reset.argtypes = [vp]
        L.aslam_set_state.argtypes = [vp, ci, ci, pd, pd, pd]
        L.aslam_grow.argtypes = [vp, ci, ci, pd, pd]
        L.aslam_ekf_step.argtypes = [vp, ci, cf, cf, cf, pd, cd, cd, pd, vp]
        L.aslam_ukf_step.argtypes = [vp, ci, cf, cf, cf, pd, pd, vp]
        L.aslam_ekf_step_batch.argtypes = [vp, pf, pf, pf, pd, ci, pd, pd, pd, ci, vp]
        L.aslam_ukf_step_batch.argtypes = [vp, pf, pf, pf, pd, ci, pd, ci, vp]
        L.aslam_set_trace.argtypes = [vp, ctypes.POINTER(TraceView)]
        L.aslam_replay.argtypes = [vp, ctypes.c_int64, ctypes.c_int64, vp, vp, vp]
        L.aslam_replay_stats.argtypes = [vp, ctypes.c_int64, ctypes.c_int64, vp, vp, vp, vp, vp, vp]
        L.aslam_innovation_enable.argtypes = [vp, ci]
        L.aslam_get_innovation.argtypes = [vp, ci, pd, pd]
        L.aslam_params_default.argtypes = [ctypes.POINTER(Params)]
        L.aslam_set_params.argtypes = [vp, ci, ctypes.POINTER(Params)]
        L.aslam_get_params.argtypes = [vp, ci, ctypes.POINTER(Params)]
        L.aslam_get_dim.argtypes = [vp, ci, pi]
        L.aslam_get_state.argtypes = [vp, ci, pd, pd, pd]
        L.aslam_get_A.argtypes = [vp, ci, pd, pd]
        L.aslam_get_landmarks.argtypes = [vp, ci, pd, pd, pi]
        L.aslam_get_wait.argtypes = [vp, ci, pf, pf, pu, ci, pi]
        L.aslam_get_status.argtypes = [vp, ci, pu]
        L.aslam_get_layout.argtypes = [vp, pi, ctypes.POINTER(ctypes.c_int64)]
        L.aslam_kernel_info.argtypes = [vp, ctypes.c_char_p, ci, pi, pi, pi]
        L.aslam_get_launch_info.argtypes = [vp, pi, pi, pi]
        L.aslam_get_syrk_tail.argtypes = [vp, pi]
        L.aslam_remove_landmarks.argtypes = [vp, vp, ci, ci, vp]
        L.aslam_select_beyond.argtypes = [vp, pd, vp, ci, vp]
        L.aslam_get_sightings.argtypes = [vp, ci, pu, pu, ci, pi, pu]
        L.aslam_select_stale.argtypes = [vp, pu, vp, ci, vp]
        L.aslam_merge_landmarks.argtypes = [vp, vp, ci, ci, cd, vp, vp]
        L.aslam_select_duplicates.argtypes = [vp, pd, pd, vp, ci, vp]
        L.aslam_gate_observations.argtypes = [vp, vp, ci, ci, ctypes.POINTER(ctypes.c_int32), pd, vp, vp, vp]
        L.aslam_joint_compat.argtypes = [vp, vp, ci, ci, ctypes.POINTER(ctypes.c_int32), vp, pd, vp, vp, vp, vp, vp]
        L.aslam_chi2_point.argtypes = [cd, ci, pd]
        L.aslam_set_replay_gate.argtypes = [vp, ci, cd]
        L.aslam_get_replay_gate.argtypes = [vp, ci, pd]
        L.aslam_get_assoc_rejected.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_uint64)]
        pb = ctypes.POINTER(ctypes.c_uint8)
        L.aslam_sighted_update_enable.argtypes = [vp, ci]
        L.aslam_get_sighted.argtypes = [vp, ci, pb, ci, pi]
        L.aslam_ekf_step_sighted.argtypes = [vp, ci, cf, cf, cf, pd, pb, cd, cd, pd, vp]
        L.aslam_ekf_step_batch_sighted.argtypes = [vp, pf, pf, pf, pd, ci, pb, ci, pd, pd, pd, ci, vp]
        # include/aslam_snapshot.h
        p32, p64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
        L.aslam_snapshot_record_bytes.restype = ctypes.c_int64
        L.aslam_snapshot_record_bytes.argtypes = [ci, ci, ci]
        L.aslam_snapshot_check.argtypes = [vp, ctypes.c_int64, p32, p32]
        L.aslam_snapshot.argtypes = [vp, p32, ci, vp, ctypes.c_int64, ci, p64, vp]
        L.aslam_restore.argtypes = [vp, p32, p32, ci, vp, ctypes.c_int64, ci, vp]
        L.aslam_join_maps.argtypes = [vp, p32, p32, ci, vp, ctypes.c_int64, ci, ctypes.POINTER(Frame), vp, ci, p32, vp]
        _core = L
    return _core


def node_lib():
    global _node
    if _node is None:
        if not os.path.exists(_NODE):
            raise OSError(f"{_NODE} is missing: run __graft_entry__.build()")
        core_lib()
        L = ctypes.CDLL(_NODE)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        pd, pf, pu = (ctypes.POINTER(t) for t in (ctypes.c_double, ctypes.c_float, ctypes.c_uint32))
        L.aslam_node_create.restype = vp
        L.aslam_node_create.argtypes = [ci, ci, ci]
        L.aslam_node_create_at.restype = vp
        L.aslam_node_create_at.argtypes = [ci, ci, ci, ctypes.c_double]
        L.aslam_node_destroy.argtypes = [vp]
        L.aslam_node_error.restype = ctypes.c_char_p
        L.aslam_node_sensor.argtypes = [vp, ci, pd, pd]
        L.aslam_node_odom.argtypes = [vp, pd, ctypes.c_float]
        L.aslam_node_odom_now.argtypes = [vp, pd, ctypes.c_double]
        L.aslam_node_dim.argtypes = [vp]
        L.aslam_node_get.argtypes = [vp, pd, pd, pd, pd]
        L.aslam_node_wait.argtypes = [vp, pf, pf, pu, ci]
        L.aslam_node_core.restype = vp
        L.aslam_node_core.argtypes = [vp]
        L.aslam_host_narrow_odom.argtypes = [ctypes.c_int64, pd, pd, pf, pd]
        L.aslam_node_enable_innovation.argtypes = [vp, ci]
        L.aslam_node_innovation.argtypes = [vp, pd, pd]
        L.aslam_node_set_params.argtypes = [vp, ctypes.POINTER(Params)]
        L.aslam_node_get_params.argtypes = [vp, ctypes.POINTER(Params)]
        L.aslam_node_remove_landmarks.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ci]
        L.aslam_node_get_sightings.argtypes = [vp, pu, pu, ci, pu]
        L.aslam_node_remove_stale.argtypes = [vp, ctypes.c_uint32]
        L.aslam_node_set_sighted_only.argtypes = [vp, ci]
        L.aslam_node_merge_landmarks.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ci, ctypes.c_double]
        L.aslam_node_merge_duplicates.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_double]
        L.aslam_node_join_map.argtypes = [vp, vp, ctypes.c_int64, ci, pd, ctypes.POINTER(ctypes.c_uint8), ci]
        L.aslam_node_set_assoc_gate.argtypes = [vp, ctypes.c_double]
        L.aslam_node_assoc_rejected.argtypes = [vp]
        L.aslam_node_assoc_rejected.restype = ctypes.c_uint64
        L.aslam_node_set_joint_prob.argtypes = [vp, ctypes.c_double]
        L.aslam_node_joint_rejected.argtypes = [vp]
        L.aslam_node_joint_rejected.restype = ctypes.c_uint64
        # include/aslam_trace_file.h
        L.aslam_trace_file_error.restype = ctypes.c_char_p
        L.aslam_trace_file_open.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp)]
        L.aslam_trace_file_close.argtypes = [vp]
        L.aslam_trace_file_close.restype = None
        L.aslam_trace_file_dims.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                            ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
        L.aslam_trace_file_view.argtypes = [vp, ctypes.POINTER(TraceView)]
        L.aslam_trace_file_raw.argtypes = [vp] + [ctypes.POINTER(vp)] * 5
        L.aslam_trace_file_write.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                             vp, vp, vp, vp, vp, ctypes.c_int32, vp, vp]
        _node = L
    return _node


def _ptr(a, ct):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ct))


def _chk(rc):
    if rc != 0:
        raise AslamError(f"aslam_core error {rc}: {core_lib().aslam_last_error().decode()}")


def chi2_point(prob, dof):
    """The `prob` quantile of chi-square with `dof` degrees of freedom (aslam_chi2_point; host arithmetic, no device needed)."""
    out = ctypes.c_double()
    _chk(core_lib().aslam_chi2_point(float(prob), int(dof), ctypes.byref(out)))
    return out.value


def joint_gates(prob, m_max):
    """The table aslam_joint_compat takes: [0, chi2(prob, 2), chi2(prob, 4), ..., chi2(prob, 2 m_max)] -- entry m bounds D2 of m pairings."""
    return np.array([0.0] + [chi2_point(prob, 2 * m) for m in range(1, int(m_max) + 1)], np.float64)


SCAN_SYMBOLS = ("aslam_scan_landmarks",)
# every symbol include/aslam_snapshot.h declares
SNAPSHOT_SYMBOLS = ("aslam_snapshot_record_bytes", "aslam_snapshot_check", "aslam_snapshot", "aslam_restore", "aslam_join_maps")
SCAN_BEAMS = 360
SCAN_REF_ABORT, SCAN_OVERFLOW = 1, 2


def scan_landmarks(ranges, max_out=64, device=0, stream=None):
    """include/aslam_scan.h on host arrays: ranges [count, 360] f32 -> (n [count] i32, range [count, max_out] f32,
    bearing [count, max_out] f32, status [count] u32).  Runs on the GPU (on `stream`, which it synchronises); there is no CPU fallback."""
    r = np.ascontiguousarray(ranges, np.float32)
    if r.ndim != 2 or r.shape[1] != SCAN_BEAMS:
        raise ValueError("ranges must be [count, 360]")
    cnt = r.shape[0]
    rg = np.zeros((cnt, max_out), np.float32)
    bg = np.zeros((cnt, max_out), np.float32)
    n = np.zeros(cnt, np.int32)
    st = np.zeros(cnt, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lib = core_lib()
    lib.aslam_scan_landmarks.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    _chk(lib.aslam_scan_landmarks(vp(r), cnt, 0, int(max_out), vp(rg), vp(bg), vp(n), vp(st), int(device), stream))
    return n, rg, bg, st


def scan_landmarks_device(ranges_ptr, count, max_out, range_ptr, bearing_ptr, n_ptr, status_ptr, device=0, stream=None):
    """include/aslam_scan.h on device pointers (ints), asynchronous on `stream`."""
    lib = core_lib()
    lib.aslam_scan_landmarks.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    _chk(lib.aslam_scan_landmarks(ranges_ptr, int(count), 1, int(max_out), range_ptr, bearing_ptr, n_ptr, status_ptr, int(device), stream))


class TraceFile:
    """A trace file opened by the C++ host library (include/aslam_trace_file.h)."""

    def __init__(self, path):
        h = ctypes.c_void_p()
        if node_lib().aslam_trace_file_open(os.fsencode(path), ctypes.byref(h)) != 0:
            raise AslamError(node_lib().aslam_trace_file_error().decode())
        self._h = h
        B, T, mo, L = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        node_lib().aslam_trace_file_dims(h, ctypes.byref(B), ctypes.byref(T), ctypes.byref(mo), ctypes.byref(L))
        self.B, self.T, self.max_obs, self.L = B.value, T.value, mo.value, L.value

    def view(self):
        """The narrowed aslam_trace view (host pointers owned by this object)."""
        v = TraceView()
        if node_lib().aslam_trace_file_view(self._h, ctypes.byref(v)) != 0:
            raise AslamError(node_lib().aslam_trace_file_error().decode())
        return v

    def arrays(self):
        """NumPy copies of the narrowed view: pose, yaw, twist, dt, obs_new, n_obs, obs."""
        v = self.view()
        B, T, mo = self.B, self.T, self.max_obs

        def arr(ptr, ct, shape):
            n = int(np.prod(shape))
            if n == 0:
                return np.zeros(shape, ct)
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ct)), (n,)).reshape(shape).copy()

        return (arr(v.pose, ctypes.c_double, (B, T, 2)), arr(v.yaw, ctypes.c_float, (B, T)),
                arr(v.twist, ctypes.c_double, (B, T, 2)), arr(v.dt, ctypes.c_float, (B, T)),
                arr(v.obs_new, ctypes.c_uint8, (B, T)), arr(v.n_obs, ctypes.c_int32, (B, T)),
                arr(v.obs, ctypes.c_float, (B, T, mo, 2)))

    def close(self):
        if getattr(self, "_h", None):
            try:
                node_lib().aslam_trace_file_close(self._h)
            except TypeError:
                pass
            self._h = None

    __del__ = close

    @staticmethod
    def write(path, tr, with_truth=True):
        """Write a trace.Trace through the C++ writer."""
        p = lambda a, dt: np.ascontiguousarray(a, dt)  # noqa: E731
        odom, dt, new, nobs, obs = p(tr.odom, np.float64), p(tr.dt, np.float32), p(tr.obs_new, np.uint8), \
            p(tr.n_obs, np.int32), p(tr.obs, np.float32)
        has = bool(with_truth and tr.truth is not None and tr.L > 0)
        lm = p(tr.landmarks, np.float64) if has else None
        truth = p(tr.truth, np.float64) if has else None
        vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        rc = node_lib().aslam_trace_file_write(os.fsencode(path), tr.B, tr.T, tr.max_obs, int(tr.warmup), vp(odom), vp(dt),
                                               vp(new), vp(nobs), vp(obs), tr.L if has else 0, vp(lm), vp(truth))
        if rc != 0:
            raise AslamError(node_lib().aslam_trace_file_error().decode())


def narrow_odom(odom):
    """Message-level odometry [..., 8] -> (pose [..., 2] f64, yaw [...] f32, twist [..., 2] f64), done by the
    C++ host mirror so that quat2euler is the host libm's atan2f (tools.h:62-66)."""
    odom = np.ascontiguousarray(odom, np.float64)
    lead = odom.shape[:-1]
    cnt = int(np.prod(lead))
    pose = np.empty(lead + (2,), np.float64)
    yaw = np.empty(lead, np.float32)
    twist = np.empty(lead + (2,), np.float64)
    node_lib().aslam_host_narrow_odom(cnt, _ptr(odom, ctypes.c_double), _ptr(pose, ctypes.c_double),
                                      _ptr(yaw, ctypes.c_float), _ptr(twist, ctypes.c_double))
    return pose, yaw, twist


class Core:
    """One libaslam_core context: `batch` independent filters resident on one GPU."""

    def __init__(self, filter="ekf", max_landmark_count=30, batch=1, max_obs=16, max_wait=128, device=0, dtype=F64, flags=0):
        self.filter = filter
        self.batch = int(batch)
        self.max_obs = int(max_obs)
        self.max_landmark_count = int(max_landmark_count)
        cfg = Config(FILTERS[filter], dtype, int(max_landmark_count), int(batch), int(max_obs), int(max_wait),
                     int(device), int(flags))
        h = ctypes.c_void_p()
        _chk(core_lib().aslam_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        self._trace_keep = None
        self.T = 0

    def close(self):
        if getattr(self, "_h", None):
            try:
                core_lib().aslam_destroy(self._h)
            except TypeError:  # interpreter shutdown: module globals are already gone
                pass
            self._h = None

    __del__ = close

    def reset(self):
        _chk(core_lib().aslam_reset(self._h))

    # ---- noise and association parameters (aslam_set_params / aslam_get_params)
    def set_params(self, params, traj=None):
        """Set the parameters of filter `traj` (None: every filter).  `params`: a Params, or a dict of overrides of the DEFAULTS (not of the
        filter's current record).  Synchronises.  R, Q, var_a and assoc_dist apply from the next callback, p0_landmark to later growths, p0_pose
        at the next reset(); promote_count is meant to be set before the first callback.  AslamError names a refused field."""
        p = Params.make(params)
        _chk(core_lib().aslam_set_params(self._h, -1 if traj is None else int(traj), ctypes.byref(p)))

    def params(self, traj=0):
        """The record of filter `traj` as the kernels read it (synchronises)."""
        p = Params()
        _chk(core_lib().aslam_get_params(self._h, int(traj), ctypes.byref(p)))
        return p

    # ---- per-callback seam
    def set_state(self, traj, n, X=None, Z=None, P=None):
        X, Z, P = (None if a is None else np.ascontiguousarray(a, np.float64) for a in (X, Z, P))
        _chk(core_lib().aslam_set_state(self._h, traj, int(n), _ptr(X, ctypes.c_double), _ptr(Z, ctypes.c_double),
                                        _ptr(P, ctypes.c_double)))

    def grow(self, traj, n_new, x_seed, z_seed):
        x_seed = np.ascontiguousarray(x_seed, np.float64)
        z_seed = np.ascontiguousarray(z_seed, np.float64)
        _chk(core_lib().aslam_grow(self._h, traj, int(n_new), _ptr(x_seed, ctypes.c_double), _ptr(z_seed, ctypes.c_double)))

    def ekf_step(self, traj, vx, az, dt, Z, a00, a10, stream=None, sighted=None):
        """`sighted` ([n_landmarks] bool / uint8, optional): the mask of this callback (aslam_ekf_step_sighted)."""
        Z = np.ascontiguousarray(Z, np.float64)
        X = np.empty(len(Z))
        if sighted is not None:
            m = np.zeros(max((len(Z) - 3) // 2, 1), np.uint8)
            m[: (len(Z) - 3) // 2] = np.asarray(sighted)[: (len(Z) - 3) // 2] != 0
            _chk(core_lib().aslam_ekf_step_sighted(self._h, traj, float(np.float32(vx)), float(np.float32(az)), float(np.float32(dt)),
                                                   _ptr(Z, ctypes.c_double), _ptr(m, ctypes.c_uint8), float(a00), float(a10),
                                                   _ptr(X, ctypes.c_double), stream))
            return X
        _chk(core_lib().aslam_ekf_step(self._h, traj, float(np.float32(vx)), float(np.float32(az)), float(np.float32(dt)),
                                       _ptr(Z, ctypes.c_double), float(a00), float(a10), _ptr(X, ctypes.c_double), stream))
        return X

    def ukf_step(self, traj, vx, az, dt, Z, stream=None):
        Z = np.ascontiguousarray(Z, np.float64)
        X = np.empty(len(Z))
        _chk(core_lib().aslam_ukf_step(self._h, traj, float(np.float32(vx)), float(np.float32(az)), float(np.float32(dt)),
                                       _ptr(Z, ctypes.c_double), _ptr(X, ctypes.c_double), stream))
        return X

    def step_batch(self, vx, az, dt, Z, a00=None, a10=None, X_out=None, stream=None, sighted=None):
        """slam() for all filters of the context in one launch chain.  vx, az, dt: [batch] float32; Z: [batch, ldz] float64;
        a00, a10: [batch] float64 (EKF).  Asynchronous: the arrays are used until `stream` is synchronised; X_out ([batch, ldx]
        float64, optional) is valid only after that.  Arrays are taken as they are (no copies): pass C-contiguous ones.
        `sighted` ([batch, ld] uint8, EKF, optional): the masks of this callback (aslam_ekf_step_batch_sighted)."""
        for a, t in ((vx, np.float32), (az, np.float32), (dt, np.float32), (Z, np.float64)):
            assert a.dtype == t and a.flags.c_contiguous and a.shape[0] == self.batch
        ldx = 0 if X_out is None else X_out.shape[1]
        if self.filter == "ekf":
            assert a00.dtype == np.float64 and a10.dtype == np.float64
            if sighted is not None:
                assert sighted.dtype == np.uint8 and sighted.flags.c_contiguous and sighted.shape[0] == self.batch
                _chk(core_lib().aslam_ekf_step_batch_sighted(self._h, _ptr(vx, ctypes.c_float), _ptr(az, ctypes.c_float), _ptr(dt, ctypes.c_float),
                                                             _ptr(Z, ctypes.c_double), Z.shape[1], _ptr(sighted, ctypes.c_uint8), sighted.shape[1],
                                                             _ptr(a00, ctypes.c_double), _ptr(a10, ctypes.c_double), _ptr(X_out, ctypes.c_double), ldx, stream))
                return
            _chk(core_lib().aslam_ekf_step_batch(self._h, _ptr(vx, ctypes.c_float), _ptr(az, ctypes.c_float), _ptr(dt, ctypes.c_float),
                                                 _ptr(Z, ctypes.c_double), Z.shape[1], _ptr(a00, ctypes.c_double), _ptr(a10, ctypes.c_double),
                                                 _ptr(X_out, ctypes.c_double), ldx, stream))
        else:
            _chk(core_lib().aslam_ukf_step_batch(self._h, _ptr(vx, ctypes.c_float), _ptr(az, ctypes.c_float), _ptr(dt, ctypes.c_float),
                                                 _ptr(Z, ctypes.c_double), Z.shape[1], _ptr(X_out, ctypes.c_double), ldx, stream))

    def sync(self, stream=None):
        import torch
        torch.cuda.synchronize() if stream is None else torch.cuda.ExternalStream(stream).synchronize()

    # ---- replay seam
    def set_trace(self, trace):
        """Bind a message-level awesomeslam_amd.trace.Trace (B == batch): narrowed on the host, copied to HBM."""
        if trace.B != self.batch or trace.max_obs != self.max_obs:
            raise ValueError(f"trace is B={trace.B}, max_obs={trace.max_obs}; context is B={self.batch}, max_obs={self.max_obs}")
        pose, yaw, twist = narrow_odom(trace.odom)
        arrs = dict(pose=pose, yaw=yaw, twist=twist, dt=np.ascontiguousarray(trace.dt, np.float32),
                    obs_new=np.ascontiguousarray(trace.obs_new, np.uint8),
                    n_obs=np.ascontiguousarray(trace.n_obs, np.int32), obs=np.ascontiguousarray(trace.obs, np.float32))
        tv = TraceView(trace.T, trace.max_obs, 0, *(arrs[k].ctypes.data for k in ("pose", "yaw", "twist", "dt", "obs_new", "n_obs", "obs")))
        _chk(core_lib().aslam_set_trace(self._h, ctypes.byref(tv)))
        self.T = trace.T

    def set_trace_file(self, tf):
        """Bind a TraceFile: the C++ host library narrows the messages, aslam_set_trace copies the view to HBM."""
        if tf.B != self.batch or tf.max_obs != self.max_obs:
            raise ValueError(f"trace file is B={tf.B}, max_obs={tf.max_obs}; context is B={self.batch}, max_obs={self.max_obs}")
        v = tf.view()
        _chk(core_lib().aslam_set_trace(self._h, ctypes.byref(v)))
        self.T = tf.T

    def set_trace_device(self, T, pose, yaw, twist, dt, obs_new, n_obs, obs):
        """Bind device-resident arrays (raw device pointers as ints, e.g. torch.Tensor.data_ptr())."""
        tv = TraceView(int(T), self.max_obs, 1, pose, yaw, twist, dt, obs_new, n_obs, obs)
        _chk(core_lib().aslam_set_trace(self._h, ctypes.byref(tv)))
        self.T = int(T)

    def replay(self, t0, nsteps, poses_ptr=None, dims_ptr=None, stream=None):
        """Asynchronous.  poses_ptr / dims_ptr: raw device pointers ([batch][nsteps][3] f64, [batch][nsteps] i32)."""
        _chk(core_lib().aslam_replay(self._h, int(t0), int(nsteps), poses_ptr, dims_ptr, stream))

    def replay_stats(self, t0, nsteps, poses_ptr=None, dims_ptr=None, nis_ptr=None, logdet_ptr=None, pose_cov_ptr=None, stream=None):
        """replay() with the innovation statistics of every callback (aslam_replay_stats).  Raw device pointers, all optional:
        nis_ptr, logdet_ptr [batch][nsteps] f64 (y^T S^-1 y, ln|det S|), pose_cov_ptr [batch][nsteps][6] f64 (the lower triangle of the
        pose block of P after the update).  NaN where slam() did not run."""
        _chk(core_lib().aslam_replay_stats(self._h, int(t0), int(nsteps), poses_ptr, dims_ptr, nis_ptr, logdet_ptr, pose_cov_ptr, stream))

    def enable_innovation(self, on=True):
        """Keep (nis, logdet) of every filter's last callback for innovation() (aslam_innovation_enable); off by default."""
        _chk(core_lib().aslam_innovation_enable(self._h, 1 if on else 0))

    def innovation(self, traj=0):
        """(nis, logdet) of filter `traj`'s last callback; synchronises.  AslamError (ASLAM_ERR_STATE) unless enable_innovation() was called."""
        a, b = ctypes.c_double(), ctypes.c_double()
        _chk(core_lib().aslam_get_innovation(self._h, traj, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # ---- sighted-only update (aslam_sighted_update_enable / aslam_get_sighted)
    def sighted_only(self, on=True):
        """Update with the rows of the landmarks sighted in each callback alone (EKF contexts; off by default; kept by reset())."""
        _chk(core_lib().aslam_sighted_update_enable(self._h, 1 if on else 0))

    def sighted(self, traj=0):
        """The mask [L] uint8 the last callback of filter `traj` used (written with the mode off as well); synchronises."""
        cap = max(self.landmark_capacity(), 1)
        m = np.zeros(cap, np.uint8)
        k = ctypes.c_int()
        _chk(core_lib().aslam_get_sighted(self._h, int(traj), _ptr(m, ctypes.c_uint8), cap, ctypes.byref(k)))
        return m[: min(k.value, cap)]

    # ---- read-back
    def dim(self, traj=0):
        n = ctypes.c_int()
        _chk(core_lib().aslam_get_dim(self._h, traj, ctypes.byref(n)))
        return n.value

    def state(self, traj=0, with_P=True):
        n = self.dim(traj)
        X, Z = np.empty(n), np.empty(n)
        P = np.empty((n, n)) if with_P else None
        _chk(core_lib().aslam_get_state(self._h, traj, _ptr(X, ctypes.c_double), _ptr(Z, ctypes.c_double), _ptr(P, ctypes.c_double)))
        return X, Z, P

    def A(self, traj=0):
        a, b = ctypes.c_double(), ctypes.c_double()
        _chk(core_lib().aslam_get_A(self._h, traj, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def landmarks(self, traj=0):
        n = self.dim(traj)
        L = (n - 3) // 2
        x, y = np.empty(L), np.empty(L)
        k = ctypes.c_int()
        _chk(core_lib().aslam_get_landmarks(self._h, traj, _ptr(x, ctypes.c_double), _ptr(y, ctypes.c_double), ctypes.byref(k)))
        return x[: k.value], y[: k.value]

    def wait_list(self, traj=0, cap=512):
        r, b, c = np.empty(cap, np.float32), np.empty(cap, np.float32), np.empty(cap, np.uint32)
        k = ctypes.c_int()
        _chk(core_lib().aslam_get_wait(self._h, traj, _ptr(r, ctypes.c_float), _ptr(b, ctypes.c_float), _ptr(c, ctypes.c_uint32), cap, ctypes.byref(k)))
        k = min(k.value, cap)
        return r[:k], b[:k], c[:k]

    def status(self, traj=0):
        s = ctypes.c_uint32()
        _chk(core_lib().aslam_get_status(self._h, traj, ctypes.byref(s)))
        return s.value

    # ---- snapshot / restore (include/aslam_snapshot.h)
    def snapshot_bytes(self, trajs=None):
        """Exact size of snapshot(trajs) in bytes (synchronises)."""
        t = None if trajs is None else np.ascontiguousarray(trajs, np.int32)
        need = ctypes.c_int64()
        _chk(core_lib().aslam_snapshot(self._h, _ptr(t, ctypes.c_int32), 0 if t is None else len(t), None, 0, 0, ctypes.byref(need), None))
        return need.value

    def snapshot(self, trajs=None, out=None, stream=None):
        """Everything filters `trajs` (default: the whole batch) are, as one blob.  Without `out`: a host uint8 array, complete on return.
        With `out`, a uint8 torch tensor on the context's device that is large enough (snapshot_bytes): one pack launch on `stream`, the
        tensor is complete when the stream is; returns `out[:size]`."""
        t = None if trajs is None else np.ascontiguousarray(trajs, np.int32)
        cnt = 0 if t is None else len(t)
        need = ctypes.c_int64()
        if out is not None:
            _chk(core_lib().aslam_snapshot(self._h, _ptr(t, ctypes.c_int32), cnt, out.data_ptr(), out.numel(), 1, ctypes.byref(need), stream))
            return out[: need.value]
        blob = np.empty(self.snapshot_bytes(trajs), np.uint8)
        _chk(core_lib().aslam_snapshot(self._h, _ptr(t, ctypes.c_int32), cnt, blob.ctypes.data, blob.size, 0, ctypes.byref(need), stream))
        return blob

    def restore(self, blob, records=None, trajs=None, stream=None):
        """Record records[i] of `blob` (default i) into slot trajs[i] (default i).  `blob`: a host uint8 array (bytes-like) or a uint8 torch
        tensor on the device.  Without both lists every record of the blob is restored, record i into slot i.  A refused call (AslamError)
        leaves the context unchanged.  Asynchronous on `stream` for a device blob, which must stay alive until the stream has passed."""
        r = None if records is None else np.ascontiguousarray(records, np.int32)
        t = None if trajs is None else np.ascontiguousarray(trajs, np.int32)
        dev = hasattr(blob, "data_ptr")
        if not dev:
            blob = np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else np.ascontiguousarray(blob, np.uint8)
        ptr, size = (blob.data_ptr(), blob.numel()) if dev else (blob.ctypes.data, blob.size)
        if r is not None or t is not None:
            cnt = len(r if r is not None else t)
        elif dev:
            raise ValueError("name the records or the slots of a device blob (its count is on the device)")
        else:
            from . import snapshot as snapfmt

            cnt = snapfmt.blob_info(blob)[1]
        _chk(core_lib().aslam_restore(self._h, _ptr(r, ctypes.c_int32), _ptr(t, ctypes.c_int32), cnt, ptr, size, 1 if dev else 0, stream))

    # ---- joining maps (aslam_join_maps)
    def join_maps(self, blob, records=None, trajs=None, frames=None, select=None, stream=None):
        """Append the landmarks of record records[i] of `blob` (default i), with their covariance block, behind the state of the running filter
        trajs[i] (default i): the two maps are taken as INDEPENDENT (zero cross-covariance), which is the caller's to ensure.  `blob`: bytes, a
        host uint8 array, a uint8 torch tensor on the device, or a (device pointer, bytes) pair; the record may come from either filter kind.
        `frames`: None (identity, zero covariance) or one (tx, ty, phi, cov3x3) per entry -- source frame -> this filter's frame, see
        mapjoin.frame / mapjoin.align.  `select`: None (every landmark of the record) or a [count, L] bool / uint8 array, entry (i, k) != 0
        takes landmark k of entry i's record.  Returns the landmarks appended per entry, int32 [count].  A refused call (AslamError) leaves the
        context unchanged.  Asynchronous on `stream` for a device blob, which must stay alive until the stream has passed."""
        r = None if records is None else np.ascontiguousarray(records, np.int32)
        t = None if trajs is None else np.ascontiguousarray(trajs, np.int32)
        if isinstance(blob, tuple):
            ptr, size, dev = int(blob[0]), int(blob[1]), True
        elif hasattr(blob, "data_ptr"):
            ptr, size, dev = blob.data_ptr(), blob.numel(), True
        else:
            blob = np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else np.ascontiguousarray(blob, np.uint8)
            ptr, size, dev = blob.ctypes.data, blob.size, False
        if r is not None or t is not None:
            cnt = len(r if r is not None else t)
        elif dev:
            raise ValueError("name the records or the slots of a device blob (its count is on the device)")
        else:
            from . import snapshot as snapfmt

            cnt = snapfmt.blob_info(blob)[1]
        if frames is not None and len(frames) != cnt:
            raise ValueError("one frame per entry")
        m = None
        if select is not None:
            m = np.ascontiguousarray(np.asarray(select) != 0, np.uint8)
            if m.ndim != 2 or m.shape[0] != cnt:
                raise ValueError("`select` is [count, L]")
        return self.join_maps_ptr(r, t, cnt, ptr, size, dev, frames, None if m is None else m.ctypes.data, 0 if m is None else m.shape[1], stream)

    def join_maps_ptr(self, records, trajs, count, blob_ptr, nbytes, is_device, frames=None, select_ptr=None, ld=0, stream=None):
        """aslam_join_maps as it is: raw pointers (ints) to the blob and to a host [count][ld] u8 selection (or None); `records` / `trajs`:
        int32 arrays or None; `frames`: None, one Frame / (tx, ty, phi, cov) per entry, or a ready (Frame * count) array.  Returns joined_out
        [count]."""
        fr = frames if frames is None or isinstance(frames, ctypes.Array) else (Frame * int(count))(*(Frame.make(f) for f in frames))
        out = np.zeros(int(count), np.int32)
        _chk(core_lib().aslam_join_maps(self._h, _ptr(records, ctypes.c_int32), _ptr(trajs, ctypes.c_int32), int(count), blob_ptr, int(nbytes),
                                        1 if is_device else 0, fr, select_ptr, int(ld), _ptr(out, ctypes.c_int32), stream))
        return out

    def save(self, path, trajs=None):
        """snapshot() to a file: the file IS the blob."""
        self.snapshot(trajs).tofile(path)

    def load(self, path, records=None, trajs=None):
        """restore() from a file written by save()."""
        self.restore(np.fromfile(path, np.uint8), records, trajs)

    # ---- removing landmarks (aslam_remove_landmarks / aslam_select_beyond)
    def landmark_capacity(self):
        """Landmarks a filter of this context can hold: the least row length of a mask."""
        return max(0, (self.max_landmark_count - 2) // 2)

    def remove_landmarks(self, mask_or_indices, traj=None, stream=None):
        """Remove landmarks from running filters; survivors keep their order and their values bit for bit, everything else a filter is stays.
        `mask_or_indices`: a [batch, L] bool / uint8 array (entry (b, i) != 0 removes landmark i of filter b; L at least landmark_capacity()),
        a uint8 torch tensor of that shape on the device, or, with `traj`, a list of landmark indices of that one filter.  Returns the new
        dimensions [batch].  A refused call (AslamError) leaves the context unchanged."""
        if traj is not None:
            idx = np.asarray(mask_or_indices, np.int64).reshape(-1)
            L = max(self.landmark_capacity(), 1)
            if not 0 <= int(traj) < self.batch:
                raise ValueError("traj out of range")
            if idx.size and (idx.min() < 0 or idx.max() >= L):
                raise ValueError(f"landmark index out of range (capacity {L})")
            mask = np.zeros((self.batch, L), np.uint8)
            mask[int(traj), idx] = 1
            mask_or_indices = mask
        if hasattr(mask_or_indices, "data_ptr"):
            m = mask_or_indices
            if m.dim() != 2 or m.shape[0] != self.batch or m.element_size() != 1 or not m.is_contiguous():
                raise ValueError("a device mask is a contiguous [batch, L] uint8 / bool tensor")
            self.remove_landmarks_ptr(m.data_ptr(), m.shape[1], True, stream)
        else:
            m = np.ascontiguousarray(np.asarray(mask_or_indices) != 0, np.uint8)
            if m.ndim != 2 or m.shape[0] != self.batch:
                raise ValueError("a mask is [batch, L]")
            self.remove_landmarks_ptr(m.ctypes.data, m.shape[1], False, stream)
        return np.array([self.dim(b) for b in range(self.batch)])

    def remove_landmarks_ptr(self, mask_ptr, ld, is_device, stream=None):
        """aslam_remove_landmarks as it is: a raw pointer (int or None) to a [batch][ld] u8 mask."""
        _chk(core_lib().aslam_remove_landmarks(self._h, mask_ptr, int(ld), 1 if is_device else 0, stream))

    def select_beyond(self, max_range, mask_ptr, ld, stream=None):
        """Device mask [batch][ld] u8 at `mask_ptr` <- 1 where a landmark lies farther than max_range (a scalar, or one value per filter) from
        its filter's own pose, 0 elsewhere (aslam_select_beyond).  Asynchronous on `stream`."""
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(max_range, np.float64), (self.batch,)))
        _chk(core_lib().aslam_select_beyond(self._h, _ptr(r, ctypes.c_double), mask_ptr, int(ld), stream))

    def prune_beyond(self, max_range, stream=None):
        """select_beyond + remove_landmarks with a device mask that never leaves the GPU.  Returns the landmarks removed per filter [batch]."""
        import torch

        before = np.array([self.dim(b) for b in range(self.batch)])
        ld = (max(self.landmark_capacity(), 1) + 15) // 16 * 16
        mask = torch.empty((self.batch, ld), dtype=torch.uint8, device="cuda")
        self.select_beyond(max_range, mask.data_ptr(), ld, stream)
        after = self.remove_landmarks(mask, stream=stream)  # (synchronises: `mask` may go)
        return (before - after) // 2

    # ---- sighting records and the forgetting policy (aslam_get_sightings / aslam_select_stale)
    def sightings(self, traj=0, padded=False):
        """(last_seen [L] u32, hits [L] u32, clock) of filter `traj` (padded: landmark_capacity() entries, zero from L on): the clock counts the callbacks in which the association ran, last_seen[i]
        is the clock of the last one that associated an observation with landmark i (of its promotion before the first), hits[i] counts them.
        The age of a landmark is clock - last_seen[i] in unsigned 32-bit arithmetic.  Synchronises."""
        cap = max(self.landmark_capacity(), 1)
        seen, hits = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        k, clk = ctypes.c_int(), ctypes.c_uint32()
        _chk(core_lib().aslam_get_sightings(self._h, int(traj), _ptr(seen, ctypes.c_uint32), _ptr(hits, ctypes.c_uint32), cap, ctypes.byref(k),
                                            ctypes.byref(clk)))
        k = cap if padded else min(k.value, cap)
        return seen[:k], hits[:k], clk.value

    def select_stale(self, max_age, mask_ptr, ld, stream=None):
        """Device mask [batch][ld] u8 at `mask_ptr` <- 1 where a landmark was last sighted more than max_age callbacks ago (a scalar, or one value
        per filter; 0xFFFFFFFF = never), 0 elsewhere (aslam_select_stale).  Asynchronous on `stream`."""
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(max_age, np.uint32), (self.batch,)))
        _chk(core_lib().aslam_select_stale(self._h, _ptr(a, ctypes.c_uint32), mask_ptr, int(ld), stream))

    def _device_mask(self):
        import torch

        ld = (max(self.landmark_capacity(), 1) + 15) // 16 * 16
        return torch.empty((self.batch, ld), dtype=torch.uint8, device="cuda"), ld

    def prune_stale(self, max_age, stream=None):
        """select_stale + remove_landmarks with a device mask that never leaves the GPU.  Returns the landmarks removed per filter [batch]."""
        before = np.array([self.dim(b) for b in range(self.batch)])
        mask, ld = self._device_mask()
        self.select_stale(max_age, mask.data_ptr(), ld, stream)
        after = self.remove_landmarks(mask, stream=stream)  # (synchronises: `mask` may go)
        return (before - after) // 2

    def replay_forget(self, t0, nsteps, period, max_age, poses_ptr=None, dims_ptr=None, stream=None):
        """replay() with a forgetting policy: after every `period` callbacks (the last chunk may be shorter, and is pruned too) the landmarks
        last sighted more than `max_age` callbacks ago are removed -- a host loop over replay, select_stale and remove_landmarks, nothing more.
        Returns the dimensions after each prune, [n_chunks][batch].  Synchronises once per chunk.
        The output buffers are CHUNK-MAJOR: chunk c's [batch][len_c][3] poses (and [batch][len_c] dimensions) follow those of chunk c - 1; the
        stride of a kernel's outputs is its launch's nsteps, and the kernels take no separate stride."""
        t0, nsteps, period = int(t0), int(nsteps), int(period)
        if period < 1:
            raise ValueError("period must be at least 1")
        mask, ld = self._device_mask()
        dims, done = [], 0
        while done < nsteps:
            k = min(period, nsteps - done)
            self.replay(t0 + done, k, None if poses_ptr is None else poses_ptr + 8 * 3 * self.batch * done,
                        None if dims_ptr is None else dims_ptr + 4 * self.batch * done, stream)
            self.select_stale(max_age, mask.data_ptr(), ld, stream)
            dims.append(self.remove_landmarks(mask, stream=stream))
            done += k
        return np.array(dims, np.int64).reshape(len(dims), self.batch)

    # ---- merging duplicate landmarks (aslam_merge_landmarks / aslam_select_duplicates)
    def merge_landmarks(self, into_or_pairs, traj=None, noise_var=0.0, stream=None):
        """Fuse duplicate landmarks: entry (b, j) = i of a [batch, L] int32 array (or int32 device tensor) merges landmark j of filter b into
        landmark i < j, -1 keeps j; with `traj`, a list of (i, j) pairs of that one filter.  The constraint "both are the same point" (with
        `noise_var` on its diagonal) is applied to X and P, then j is removed as remove_landmarks removes it.  Returns the pairs fused and
        removed per filter [batch].  A refused call (AslamError: i >= j, a chain, an index out of range) leaves the context unchanged."""
        if traj is not None:
            L = max(self.landmark_capacity(), 1)
            if not 0 <= int(traj) < self.batch:
                raise ValueError("traj out of range")
            into = np.full((self.batch, L), -1, np.int32)
            for i, j in np.asarray(into_or_pairs, np.int64).reshape(-1, 2):
                if not 0 <= j < L:
                    raise ValueError(f"landmark index out of range (capacity {L})")
                into[int(traj), j] = i
            into_or_pairs = into
        if hasattr(into_or_pairs, "data_ptr"):
            m = into_or_pairs
            if m.dim() != 2 or m.shape[0] != self.batch or m.element_size() != 4 or m.is_floating_point() or not m.is_contiguous():
                raise ValueError("a device array is a contiguous [batch, L] int32 tensor")
            return self.merge_landmarks_ptr(m.data_ptr(), m.shape[1], True, noise_var, stream)
        m = np.ascontiguousarray(into_or_pairs, np.int32)
        if m.ndim != 2 or m.shape[0] != self.batch:
            raise ValueError("`into` is [batch, L]")
        return self.merge_landmarks_ptr(m.ctypes.data, m.shape[1], False, noise_var, stream)

    def merge_landmarks_ptr(self, into_ptr, ld, is_device, noise_var=0.0, stream=None):
        """aslam_merge_landmarks as it is: a raw pointer (int) to a [batch][ld] i32 array.  Returns merged_out [batch]."""
        out = np.zeros(self.batch, np.int32)
        _chk(core_lib().aslam_merge_landmarks(self._h, into_ptr, int(ld), 1 if is_device else 0, float(noise_var), out.ctypes.data, stream))
        return out

    def select_duplicates(self, gate, max_dist, into_ptr, ld, stream=None):
        """Device array [batch][ld] i32 at `into_ptr` <- for every landmark j the i < j to merge it into (the candidate of smallest Mahalanobis
        distance below `gate` within `max_dist`; scalars, or one value per filter), -1 elsewhere (aslam_select_duplicates).  Asynchronous."""
        g = np.ascontiguousarray(np.broadcast_to(np.asarray(gate, np.float64), (self.batch,)))
        d = np.ascontiguousarray(np.broadcast_to(np.asarray(max_dist, np.float64), (self.batch,)))
        _chk(core_lib().aslam_select_duplicates(self._h, _ptr(g, ctypes.c_double), _ptr(d, ctypes.c_double), into_ptr, int(ld), stream))

    def merge_duplicates(self, gate, max_dist, noise_var=0.0, max_passes=4, stream=None):
        """select_duplicates + merge_landmarks with a device array that never leaves the GPU, until a pass merges nothing or `max_passes` ran
        (the selector leaves a landmark whose partner is itself merged for the next pass).  Returns the landmarks merged per filter [batch]."""
        import torch

        ld = (max(self.landmark_capacity(), 1) + 15) // 16 * 16
        into = torch.empty((self.batch, ld), dtype=torch.int32, device="cuda")
        total = np.zeros(self.batch, np.int64)
        for _ in range(int(max_passes)):
            self.select_duplicates(gate, max_dist, into.data_ptr(), ld, stream)
            k = self.merge_landmarks(into, noise_var=noise_var, stream=stream)  # (synchronises)
            total += k
            if not k.any():
                break
        return total

    # ---- Mahalanobis-gated data association (aslam_gate_observations)
    def gate_observations(self, obs, n_obs, gate, stream=None):
        """For every observation the landmark of smallest Mahalanobis distance m = v^T (H_k P H_k^T + R)^-1 v if m < gate, else -1
        (aslam_gate_observations; binary64 on the device, P never leaves it).  `obs`: [batch, ldo, 2] float32 (range, bearing), a NumPy array
        or a contiguous float32 device tensor; `n_obs`: [batch] observations per filter; `gate`: a scalar or one value per filter (9.21: the
        99 % point of chi-square with 2 degrees of freedom).  Returns (assoc [batch, ldo] int32, mdist [batch, ldo] float64) as NumPy arrays:
        -1 and +inf from n_obs[b] on.  Reads the filters, changes nothing."""
        import torch

        if hasattr(obs, "data_ptr"):
            if obs.dim() != 3 or obs.shape[0] != self.batch or obs.shape[2] != 2 or obs.dtype != torch.float32 or not obs.is_contiguous():
                raise ValueError("a device obs is a contiguous [batch, ldo, 2] float32 tensor")
            ptr, ldo, dev = obs.data_ptr(), obs.shape[1], True
        else:
            obs = np.ascontiguousarray(obs, np.float32)
            if obs.ndim != 3 or obs.shape[0] != self.batch or obs.shape[2] != 2:
                raise ValueError("`obs` is [batch, ldo, 2]")
            ptr, ldo, dev = obs.ctypes.data, obs.shape[1], False
        assoc = torch.empty((self.batch, max(ldo, 1)), dtype=torch.int32, device="cuda")
        mdist = torch.empty((self.batch, max(ldo, 1)), dtype=torch.float64, device="cuda")
        self.gate_observations_ptr(ptr, ldo, dev, n_obs, gate, assoc.data_ptr(), mdist.data_ptr(), stream)
        self.sync(stream)
        return assoc.cpu().numpy(), mdist.cpu().numpy()

    def gate_observations_ptr(self, obs_ptr, ldo, is_device, n_obs, gate, assoc_ptr, mdist_ptr=None, stream=None):
        """aslam_gate_observations as it is: raw pointers (ints) to obs [batch][ldo][2] f32 and to the device outputs assoc [batch][ldo] i32 and
        mdist [batch][ldo] f64 (or None); n_obs [batch] and gate (a scalar, or [batch]) are host values.  Asynchronous on `stream`."""
        k = None if n_obs is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n_obs, np.int32), (self.batch,)))
        g = None if gate is None else np.ascontiguousarray(np.broadcast_to(np.asarray(gate, np.float64), (self.batch,)))
        _chk(core_lib().aslam_gate_observations(self._h, obs_ptr, int(ldo), 1 if is_device else 0, _ptr(k, ctypes.c_int32), _ptr(g, ctypes.c_double),
                                                assoc_ptr, mdist_ptr, stream))

    # ---- joint compatibility of the gated pairings (aslam_joint_compat)
    def joint_compat(self, obs, n_obs, cand=None, prob=0.99, ic_gate=9.21, stream=None):
        """The sequential joint-compatibility test of aslam_joint_compat on the candidates `cand` ([batch, ldo] int32, a NumPy array or a device
        tensor; None: aslam_gate_observations at `ic_gate` runs first and the joint test takes its output in place, on the device).  `obs`,
        `n_obs`: as for gate_observations, ldo <= 64.  `prob`: the chi-square probability of the bounds (joint_gates), None = evaluate mode
        (every usable candidate is accepted, the call reports the numbers of the given hypothesis).  Returns (assoc [batch, ldo] int32,
        incr [batch, ldo] float64, D2 [batch], logdet [batch], accepted [batch], refused [batch]).  The decisions depend on the message order.
        Reads the filters, changes nothing."""
        import torch

        if hasattr(obs, "data_ptr"):
            if obs.dim() != 3 or obs.shape[0] != self.batch or obs.shape[2] != 2 or obs.dtype != torch.float32 or not obs.is_contiguous():
                raise ValueError("a device obs is a contiguous [batch, ldo, 2] float32 tensor")
            ptr, ldo, dev = obs.data_ptr(), obs.shape[1], True
        else:
            obs = np.ascontiguousarray(obs, np.float32)
            if obs.ndim != 3 or obs.shape[0] != self.batch or obs.shape[2] != 2:
                raise ValueError("`obs` is [batch, ldo, 2]")
            ptr, ldo, dev = obs.ctypes.data, obs.shape[1], False
        shape = (self.batch, max(ldo, 1))
        if cand is None:
            assoc = torch.empty(shape, dtype=torch.int32, device="cuda")
            self.gate_observations_ptr(ptr, ldo, dev, n_obs, ic_gate, assoc.data_ptr(), None, stream)
        elif hasattr(cand, "data_ptr"):
            if tuple(cand.shape) != shape or cand.dtype != torch.int32 or not cand.is_contiguous():
                raise ValueError("a device cand is a contiguous [batch, ldo] int32 tensor")
            assoc = cand.clone()
        else:
            cand = np.ascontiguousarray(cand, np.int32)
            if cand.shape != shape:
                raise ValueError("`cand` is [batch, ldo]")
            assoc = torch.from_numpy(cand).cuda()
        incr = torch.empty(shape, dtype=torch.float64, device="cuda")
        joint = torch.empty((self.batch, 2), dtype=torch.float64, device="cuda")
        count = torch.empty((self.batch, 2), dtype=torch.int32, device="cuda")
        tab = None if prob is None else joint_gates(prob, ldo)
        self.joint_compat_ptr(ptr, ldo, dev, n_obs, assoc.data_ptr(), tab, assoc.data_ptr(), incr.data_ptr(), joint.data_ptr(), count.data_ptr(), stream)
        self.sync(stream)
        joint, count = joint.cpu().numpy(), count.cpu().numpy()
        return assoc.cpu().numpy(), incr.cpu().numpy(), joint[:, 0].copy(), joint[:, 1].copy(), count[:, 0].copy(), count[:, 1].copy()

    def joint_compat_ptr(self, obs_ptr, ldo, is_device, n_obs, cand_ptr, gate_tab, assoc_ptr, incr_ptr, joint_ptr, count_ptr, stream=None):
        """aslam_joint_compat as it is: raw pointers (ints) to obs [batch][ldo][2] f32, to the device candidates and outputs; n_obs [batch] and
        gate_tab ([ldo + 1] float64, or None for evaluate mode) are host values.  Asynchronous on `stream`."""
        k = None if n_obs is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n_obs, np.int32), (self.batch,)))
        g = None if gate_tab is None else np.ascontiguousarray(gate_tab, np.float64)
        if g is not None and g.shape != (int(ldo) + 1,) and int(ldo) >= 1:
            raise ValueError("`gate_tab` is [ldo + 1]")
        _chk(core_lib().aslam_joint_compat(self._h, obs_ptr, int(ldo), 1 if is_device else 0, _ptr(k, ctypes.c_int32), cand_ptr, _ptr(g, ctypes.c_double),
                                           assoc_ptr, incr_ptr, joint_ptr, count_ptr, stream))

    # ---- the same gate inside the replay seam (aslam_set_replay_gate)
    def set_replay_gate(self, gate, traj=None):
        """Associate by the Mahalanobis gate inside replay() / replay_stats() for filter `traj` (None: every filter): 0 = the Euclidean rule (the
        default), > 0 (inf allowed) = accept the landmark of smallest m if m < gate, drop what only the Euclidean rule would have matched (counted:
        assoc_rejected), hand the rest to the wait-list.  Kept by reset(), not carried by snapshots.  Synchronises.  AslamError on a NaN or
        negative gate or a bad `traj`."""
        _chk(core_lib().aslam_set_replay_gate(self._h, -1 if traj is None else int(traj), float(gate)))

    def replay_gate(self, traj=0):
        """The gate of filter `traj` as the kernels read it (synchronises)."""
        g = ctypes.c_double()
        _chk(core_lib().aslam_get_replay_gate(self._h, int(traj), ctypes.byref(g)))
        return g.value

    def assoc_rejected(self, traj=0):
        """Observations of filter `traj` the gate has dropped since the last reset() / restore of the slot (synchronises)."""
        k = ctypes.c_uint64()
        _chk(core_lib().aslam_get_assoc_rejected(self._h, int(traj), ctypes.byref(k)))
        return int(k.value)

    def layout(self):
        npad, nbytes = ctypes.c_int(), ctypes.c_int64()
        _chk(core_lib().aslam_get_layout(self._h, ctypes.byref(npad), ctypes.byref(nbytes)))
        return npad.value, nbytes.value

    def kernel_info(self):
        name = ctypes.create_string_buffer(320)
        g, b, l = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _chk(core_lib().aslam_kernel_info(self._h, name, 320, ctypes.byref(g), ctypes.byref(b), ctypes.byref(l)))
        return {"name": name.value.decode(), "grid": g.value, "block": b.value, "lds_bytes": l.value}

    def launch_info(self):
        """What the last replay / step of this context really launched (aslam_get_launch_info)."""
        g, r, l = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _chk(core_lib().aslam_get_launch_info(self._h, ctypes.byref(g), ctypes.byref(r), ctypes.byref(l)))
        return {"stream_groups": g.value, "chol_resident": bool(r.value), "launches_per_callback": l.value}

    def syrk_tail(self):
        """Whether the last replay / step handed the syrk its tail rule (aslam_get_syrk_tail)."""
        on = ctypes.c_int()
        _chk(core_lib().aslam_get_syrk_tail(self._h, ctypes.byref(on)))
        return bool(on.value)


class Node:
    """aslam::EKFSlam / aslam::UKFSlam host mirror (C++), driving the per-callback seam of the core."""

    def __init__(self, filter="ekf", max_landmark_count=30, device=0, now_init=0.0):
        """`now_init`: the clock reading (seconds) at construction -- initialize()'s last_time = ros::Time::now().toSec() (ekf.cpp:54)"""
        h = node_lib().aslam_node_create_at(FILTERS[filter], int(max_landmark_count), int(device), float(now_init))
        if not h:
            raise AslamError(node_lib().aslam_node_error().decode())
        self._h = ctypes.c_void_p(h)

    def close(self):
        if getattr(self, "_h", None):
            node_lib().aslam_node_destroy(self._h)
            self._h = None

    __del__ = close

    def sensor_msg(self, xs, ys):
        xs = np.ascontiguousarray(xs, np.float64)
        ys = np.ascontiguousarray(ys, np.float64)
        node_lib().aslam_node_sensor(self._h, len(xs), _ptr(xs, ctypes.c_double), _ptr(ys, ctypes.c_double))

    def odom_msg(self, msg8, dt):
        m = np.ascontiguousarray(msg8, np.float64)
        rc = node_lib().aslam_node_odom(self._h, _ptr(m, ctypes.c_double), float(np.float32(dt)))
        if rc < 0:
            raise AslamError(node_lib().aslam_node_error().decode())
        return rc

    def odom_msg_now(self, msg8, now):
        m = np.ascontiguousarray(msg8, np.float64)
        rc = node_lib().aslam_node_odom_now(self._h, _ptr(m, ctypes.c_double), float(now))
        if rc < 0:
            raise AslamError(node_lib().aslam_node_error().decode())
        return rc

    @property
    def N(self):
        return node_lib().aslam_node_dim(self._h)

    def state(self):
        n = self.N
        X, Z = np.empty(n), np.empty(n)
        a, b = ctypes.c_double(), ctypes.c_double()
        node_lib().aslam_node_get(self._h, _ptr(X, ctypes.c_double), _ptr(Z, ctypes.c_double), ctypes.byref(a), ctypes.byref(b))
        return X, Z, a.value, b.value

    def P(self):
        n = self.N
        P = np.empty((n, n))
        core = ctypes.c_void_p(node_lib().aslam_node_core(self._h))
        _chk(core_lib().aslam_get_state(core, 0, None, None, _ptr(P, ctypes.c_double)))
        return P

    def enable_innovation(self, on=True):
        """Keep (nis, logdet) of the last callback (aslam_node_enable_innovation); off by default."""
        if node_lib().aslam_node_enable_innovation(self._h, 1 if on else 0) != 0:
            raise AslamError(node_lib().aslam_node_error().decode())

    def innovation(self):
        """(nis, logdet) of the last odometry callback: NaN when slam() did not run in it."""
        a, b = ctypes.c_double(), ctypes.c_double()
        if node_lib().aslam_node_innovation(self._h, ctypes.byref(a), ctypes.byref(b)) != 0:
            raise AslamError(node_lib().aslam_node_error().decode())
        return a.value, b.value

    def set_sighted_only(self, on=True):
        """FilterNode::setSightedOnly: update with the rows of the landmarks each callback's own association sighted (EKF nodes)."""
        if node_lib().aslam_node_set_sighted_only(self._h, 1 if on else 0) != 0:
            raise AslamError(node_lib().aslam_node_error().decode())

    def set_params(self, params):
        """FilterNode::setParams: a Params or a dict of overrides of the defaults.  Before the first callback (p0_pose applies then)."""
        p = Params.make(params)
        if node_lib().aslam_node_set_params(self._h, ctypes.byref(p)) != 0:
            raise AslamError(node_lib().aslam_node_error().decode())

    def params(self):
        p = Params()
        node_lib().aslam_node_get_params(self._h, ctypes.byref(p))
        return p

    def remove_landmarks(self, indices):
        """FilterNode::removeLandmarks: forget these landmarks (0-based indices) between two callbacks.  Returns the new dimension."""
        idx = np.ascontiguousarray(indices, np.int32).reshape(-1)
        if node_lib().aslam_node_remove_landmarks(self._h, _ptr(idx, ctypes.c_int32), len(idx)) != 0:
            raise AslamError(node_lib().aslam_node_error().decode())
        return self.N

    def sightings(self):
        """(last_seen, hits, clock) as Core.sightings, from the mirror's own association (FilterNode::lastSeen / hits / clock)."""
        L = (self.N - 3) // 2
        seen, hits = np.zeros(max(L, 1), np.uint32), np.zeros(max(L, 1), np.uint32)
        clk = ctypes.c_uint32()
        node_lib().aslam_node_get_sightings(self._h, _ptr(seen, ctypes.c_uint32), _ptr(hits, ctypes.c_uint32), L, ctypes.byref(clk))
        return seen[:L], hits[:L], clk.value

    def remove_stale(self, max_age):
        """FilterNode::removeStale: forget the landmarks last sighted more than max_age callbacks ago.  Returns how many went."""
        k = node_lib().aslam_node_remove_stale(self._h, int(max_age))
        if k < 0:
            raise AslamError(node_lib().aslam_node_error().decode())
        return k

    def merge_landmarks(self, pairs, noise_var=0.0):
        """FilterNode::mergeLandmarks: fuse each (i, j), i < j, and drop j; the mirror's own records fuse by the core's rule.  Returns how many."""
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        k = node_lib().aslam_node_merge_landmarks(self._h, _ptr(pr, ctypes.c_int32), len(pr), float(noise_var))
        if k < 0:
            raise AslamError(node_lib().aslam_node_error().decode())
        return k

    def merge_duplicates(self, gate, max_dist, noise_var=0.0):
        """FilterNode::mergeDuplicates: aslam_select_duplicates + mergeLandmarks, passes until one merges nothing (4 at the most)."""
        k = node_lib().aslam_node_merge_duplicates(self._h, float(gate), float(max_dist), float(noise_var))
        if k < 0:
            raise AslamError(node_lib().aslam_node_error().decode())
        return k

    def join_map(self, blob, record=0, frame=None, select=None):
        """FilterNode::joinMap: the landmarks of record `record` of a host snapshot `blob` (bytes or a uint8 array), with their covariance
        block, behind this filter's state as an independent map (Core.join_maps).  `frame`: None or (tx, ty, phi, cov3x3); `select`: None or one
        bool per landmark of the record.  Returns how many were joined."""
        b = np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else np.ascontiguousarray(blob, np.uint8)
        f12 = None
        if frame is not None:
            fr = Frame.make(frame)
            f12 = np.array([fr.tx, fr.ty, fr.phi] + list(fr.cov), np.float64)
        m = None if select is None else np.ascontiguousarray(np.asarray(select).reshape(-1) != 0, np.uint8)
        k = node_lib().aslam_node_join_map(self._h, b.ctypes.data, b.size, int(record), _ptr(f12, ctypes.c_double), _ptr(m, ctypes.c_uint8),
                                           0 if m is None else len(m))
        if k < 0:
            raise AslamError(node_lib().aslam_node_error().decode())
        return k

    def set_assoc_gate(self, gate):
        """FilterNode::setAssocGate: associate by the Mahalanobis gate of aslam_gate_observations (9.21: 99 % of chi-square with 2 degrees of
        freedom); 0, the default, keeps the reference's Euclidean rule.  A negative or NaN value is refused."""
        if node_lib().aslam_node_set_assoc_gate(self._h, float(gate)) != 0:
            raise AslamError(node_lib().aslam_node_error().decode())

    def set_joint_prob(self, prob):
        """FilterNode::setJointProb: behind the Mahalanobis gate (set_assoc_gate > 0), test the gated pairings of every message jointly
        (aslam_joint_compat) at the chi-square probability `prob` in (0, 1); 0 = off, the default.  A pairing the joint test refuses is dropped and
        counted in joint_rejected().  AslamError on any other value."""
        if node_lib().aslam_node_set_joint_prob(self._h, float(prob)) != 0:
            raise AslamError(node_lib().aslam_node_error().decode())

    def joint_rejected(self):
        """FilterNode::jointRejected: pairings the individual gate accepted and the joint test refused."""
        return int(node_lib().aslam_node_joint_rejected(self._h))

    def assoc_rejected(self):
        """FilterNode::assocRejected: observations dropped because the gate refused them while the Euclidean rule would have associated them."""
        return int(node_lib().aslam_node_assoc_rejected(self._h))

    def wait_list(self, cap=4096):
        r, b, c = np.empty(cap, np.float32), np.empty(cap, np.float32), np.empty(cap, np.uint32)
        k = node_lib().aslam_node_wait(self._h, _ptr(r, ctypes.c_float), _ptr(b, ctypes.c_float), _ptr(c, ctypes.c_uint32), cap)
        k = min(k, cap)
        return r[:k], b[:k], c[:k]

    def replay(self, traj, T=None):
        """Drive one message-level trajectory through the callbacks; returns poses[T,3], dims[T]."""
        T = traj.T if T is None else T
        poses = np.zeros((T, 3))
        dims = np.zeros(T, np.int32)
        for t in range(T):
            if traj.obs_new[t]:
                k = int(traj.n_obs[t])
                self.sensor_msg(traj.obs[t, :k, 0], traj.obs[t, :k, 1])
            if self.odom_msg(traj.odom[t], traj.dt[t]):
                poses[t] = self.state()[0][:3]
            dims[t] = self.N
        return poses, dims
