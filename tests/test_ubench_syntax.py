"""The stand-alone harnesses under tools/ubench/ that include the library's kernel headers are compiled by nothing else: a kernel whose
signature changes would break them silently.  Every such harness must pass hipcc's front end for gfx950 (-fsyntax-only: no code
generation, no GPU)."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "awesomeslam_amd", "csrc")
UBENCH = os.path.join(ROOT, "tools", "ubench")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def includes_library_header(path):
    with open(path) as f:
        names = re.findall(r'^\s*#include\s+"([^"]+)"', f.read(), re.M)
    return any(os.path.exists(os.path.join(CSRC, n)) for n in names)


HARNESSES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(UBENCH, "*.hip")) if includes_library_header(p))


def test_the_harnesses_of_the_large_state_kernels_are_covered():
    assert {"syrk_bench.hip", "trsm_bench.hip", "fd_bench.hip", "lookahead_isolated.hip"} <= set(HARNESSES)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
@pytest.mark.parametrize("name", HARNESSES)
def test_ubench_harness_compiles(name):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-inline-asm", "-I", "awesomeslam_amd/csrc", "-I", "tools/ubench",
           "-fsyntax-only", os.path.join("tools", "ubench", name)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
