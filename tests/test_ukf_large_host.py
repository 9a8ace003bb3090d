"""The opt-in flag of the large-state UKF (ASLAM_CFG_UKF_LARGE) at the C ABI: declared in the header, mirrored by the ctypes binding, and
decided by aslam_create before it touches a device -- so the return codes below hold with and without a GPU."""
import ctypes
import os
import re

from awesomeslam_amd import core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, ARG, HIP = -3, -1, -2


def test_header_and_binding_agree(built):
    txt = open(os.path.join(ROOT, "include", "aslam_core.h")).read()
    assert re.search(r"\bASLAM_CFG_UKF_LARGE\s*=\s*1\b", txt)
    assert re.search(r"#define\s+ASLAM_ABI_VERSION\s+1\b", txt)
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*aslam_config;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"int32_t\s+(\w+)\s*;", body)
    assert fields == ["filter", "dtype", "max_landmark_count", "batch", "max_obs", "max_wait", "device", "flags"]
    assert [f[0] for f in core.Config._fields_] == fields
    assert all(f[1] is ctypes.c_int32 for f in core.Config._fields_) and ctypes.sizeof(core.Config) == 32
    assert core.CFG_UKF_LARGE == 1
    assert core.core_lib().aslam_abi_version() == 1


def create(filter, dtype, cap, flags):
    lib = core.core_lib()
    h = ctypes.c_void_p()
    cfg = core.Config(filter, dtype, cap, 1, 8, 8, 0, flags)
    rc = lib.aslam_create(ctypes.byref(cfg), ctypes.byref(h))
    if rc == 0:
        lib.aslam_destroy(h)
    return rc


def test_create_return_codes(built):
    import torch

    F = core.CFG_UKF_LARGE
    assert create(core.UKF, core.F64, 400, 0) == UNSUPPORTED     # without the flag: as before
    assert create(core.UKF, core.F32, 400, F) == UNSUPPORTED     # no fp32 UKF
    assert create(core.UKF, core.F32, 30, F) == UNSUPPORTED
    assert create(core.UKF, core.F64, 1088, F) == UNSUPPORTED    # n + 2 rows no longer fit 17 blocks of 64
    assert create(core.UKF, core.F64, 400, 2) == ARG             # unknown bit
    assert create(core.UKF, core.F64, 400, F | 4) == ARG
    assert create(core.EKF, core.F64, 30, 2) == ARG
    # the feature: the support check precedes hipSetDevice, so without a device the call gets as far as the runtime
    want = 0 if torch.cuda.is_available() else HIP
    assert create(core.UKF, core.F64, 400, F) == want
    assert create(core.UKF, core.F64, 1087, F) == want           # the largest cap: n = 1085, 541 landmarks
    # the flag changes nothing where the single-CU kernels hold the state, and the EKF ignores it
    assert create(core.UKF, core.F64, 30, F) == create(core.UKF, core.F64, 30, 0) == want
    assert create(core.EKF, core.F64, 400, F) == want


def test_python_keyword(built):
    import inspect

    params = list(inspect.signature(core.Core.__init__).parameters)
    assert params[-1] == "flags" and inspect.signature(core.Core.__init__).parameters["flags"].default == 0
