"""The point-to-line ICP adapter class (ScanMatcherIcpPointToLineHip in
my-lidar-graph-slam_amd/host/) through its C++ test driver
(tests/cpp_icp/icp_adapter_test.cpp, built by `make cpptest`)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp_icp", "build", "icp_adapter_test")


def run():
    assert os.path.exists(BIN), "build first: make -C <repo> all"
    return subprocess.run([BIN], capture_output=True, text=True, timeout=300)


def test_icp_adapter_links_and_reports_missing_device():
    """CPU: the adapter and the C-ABI library load; without a GPU the driver
    exits with the skip status after Device() threw (with one, it runs the GPU
    checks and must pass them)."""
    r = run()
    if r.returncode == 0 and "ICP ADAPTER TESTS PASSED" in r.stdout:
        pytest.skip("a GPU is present: covered by the gpu test")
    assert r.returncode == 77, r.stdout + r.stderr
    assert "no GPU" in r.stdout


@pytest.mark.gpu
def test_icp_adapter_on_gpu():
    r = run()
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ICP ADAPTER TESTS PASSED" in r.stdout
