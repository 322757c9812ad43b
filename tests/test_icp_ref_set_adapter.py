"""The adapter classes of the ICP reference set and the ICP loop refinement
(IcpReferenceSetHip, LoopRefinerIcpHip in my-lidar-graph-slam_amd/host/)
through their C++ test driver (tests/cpp_icp_ref_set/icp_ref_set_adapter_test.cpp,
built by `make cpptest`) on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp_icp_ref_set", "build", "icp_ref_set_adapter_test")


@pytest.mark.gpu
def test_icp_ref_set_adapter_on_gpu():
    assert os.path.exists(BIN), "build first: make -C <repo> all"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ICP REF SET ADAPTER TESTS PASSED" in r.stdout and "FAIL]" not in r.stdout
