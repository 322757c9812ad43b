"""CPU-side checks of the paired coarse lanes (k_coarse_list_p,
LGS_OPT_LIST_PAIRS) and the ordered work list (LGS_OPT_LIST_ORDER): the two
options and the four debug buffers are declared in the header and bound with
the same ids; the "pair read stays inside the allocation" condition that picks
the kernel (csrc/coarse_pair.hpp) runs against a brute-force restatement of
the kernel's reads under the sanitizers, in a stand-alone program
(tests/cpp_coarse_pair/coarse_pair_check.cpp)."""
import os
import re
import subprocess

from lgs_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CHECK = os.path.join(ROOT, "tests", "cpp_coarse_pair", "build", "coarse_pair_check")


def test_options_and_debug_buffers_are_declared_and_bound():
    hip_h = open(os.path.join(ROOT, "include", "lgs_hip.h")).read()
    ids = [int(x) for x in re.findall(r"#define\s+LGS_OPT_\w+\s+(\d+)", hip_h)]
    for name in ("LGS_OPT_LIST_ORDER", "LGS_OPT_LIST_PAIRS"):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, hip_h)
        assert m and int(m.group(1)) == getattr(abi, name), name
        assert ids.count(getattr(abi, name)) == 1, "the option id is taken twice"
    assert [abi.Context.DEBUG_BUFFERS[k][0] for k in ("cflag", "wl_sbl", "wl_cnt", "wl_al")] == [16, 17, 18, 19]
    assert "16 cflag" in hip_h and "17 the item's entries" in hip_h   # the header's list of `which`


def test_pair_reads_under_the_sanitizers():
    """map sizes 100-1010, LowRes 3 and 5, odd and even lattices, whole and shortened
    allocations: the condition equals the brute-force answer (make cpptest)"""
    assert os.path.exists(HOST_CHECK), "build first: make -C <repo> all"
    r = subprocess.run([HOST_CHECK], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "COARSE PAIR CHECKS PASSED" in r.stdout
    assert "FAIL" not in r.stdout
