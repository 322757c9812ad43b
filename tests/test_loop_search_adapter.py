"""The loop searcher's adapter classes (LoopSearcherNearestHip, LoopGraphHip,
GetLoopDetectionQueries in my-lidar-graph-slam_amd/host/) through their C++
test driver (tests/cpp_loop_search/loop_search_adapter_test.cpp, built by
`make cpptest`)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp_loop_search", "build", "loop_search_adapter_test")


def run():
    assert os.path.exists(BIN), "build first: make -C <repo> all"
    return subprocess.run([BIN], capture_output=True, text=True, timeout=300)


def test_loop_search_adapter_links_and_reports_missing_device():
    """CPU: the adapter and the C-ABI library load; without a GPU the driver
    exits with the skip status after Device() threw (with one, it runs the GPU
    checks and must pass them)."""
    r = run()
    if r.returncode == 0 and "LOOP SEARCH ADAPTER TESTS PASSED" in r.stdout:
        pytest.skip("a GPU is present: covered by the gpu test")
    assert r.returncode == 77, r.stdout + r.stderr
    assert "no GPU" in r.stdout


@pytest.mark.gpu
def test_loop_search_adapter_on_gpu():
    """Search, SearchBatch and SearchAllMaps against brute force, and end to end through
    GetLoopDetectionQueries and the grid-search loop detector"""
    r = run()
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "LOOP SEARCH ADAPTER TESTS PASSED" in r.stdout
