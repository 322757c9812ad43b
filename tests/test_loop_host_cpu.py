"""The loop detectors' batch contract on the host alone (csrc/loop_host.hpp:
check_loop_batch and fill_loop_result, with the error and pose headers they
include): a stand-alone program (tests/cpp_loop/loop_host_check.cpp) runs them
under the address and undefined-behaviour sanitizers against an independent
statement of the rules and a hand-built result record."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CHECK = os.path.join(ROOT, "tests", "cpp_loop", "build", "loop_host_check")


def test_loop_batch_contract_under_the_sanitizers():
    """0 to 3 queries of 0 to 3 candidates, every first_candidate and num_candidates off by one
    either way, the declared total off by one either way, null maps and scans, thresholds at and
    around the ends of (0, 1] and NaN: accept or reject, and query_of, as the brute-force rule;
    the result record byte for byte, found and unfound, at three poses (make cpptest).
    About 310 000 batches, 1.8 s: each rejected one costs a throw under the sanitizers."""
    assert os.path.exists(HOST_CHECK), "build first: make -C <repo> all"
    r = subprocess.run([HOST_CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "LOOP HOST CHECKS PASSED" in r.stdout
    assert "FAIL" not in r.stdout
