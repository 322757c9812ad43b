"""CPU-side checks of the superblock pass's per-thread load skip (k_super_hv,
LGS_OPT_HV_INZERO): the option and the two debug buffers are declared in the
header and bound with the same ids; the footprint -> precompute-tile range that
the device and the host share (csrc/hv_zero.hpp) runs against a brute-force
restatement of the kernel's loads under the sanitizers, in a stand-alone
program (tests/cpp_hv/hv_zero_check.cpp)."""
import os
import re
import subprocess

from lgs_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CHECK = os.path.join(ROOT, "tests", "cpp_hv", "build", "hv_zero_check")


def test_option_and_debug_buffers_are_declared_and_bound():
    hip_h = open(os.path.join(ROOT, "include", "lgs_hip.h")).read()
    m = re.search(r"#define\s+LGS_OPT_HV_INZERO\s+(\d+)", hip_h)
    assert m and int(m.group(1)) == abi.LGS_OPT_HV_INZERO
    ids = [int(x) for x in re.findall(r"#define\s+LGS_OPT_\w+\s+(\d+)", hip_h)]
    assert ids.count(abi.LGS_OPT_HV_INZERO) == 1, "the option id is taken twice"
    assert abi.Context.DEBUG_BUFFERS["hv_inmask"][0] == 10 and abi.Context.DEBUG_BUFFERS["hv_outmask"][0] == 11
    assert "10 the" in hip_h and "11 its out-masks" in hip_h   # the header's list of `which`


def test_tile_range_under_the_sanitizers():
    """every live thread of both kernel variants, map sizes 100-1010, LowRes 5 and 3, both
    precompute tilings: its loads stay inside the returned tile range or in the margins
    (make cpptest)"""
    assert os.path.exists(HOST_CHECK), "build first: make -C <repo> all"
    r = subprocess.run([HOST_CHECK], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "HV ZERO CHECKS PASSED" in r.stdout
    assert "FAIL" not in r.stdout
