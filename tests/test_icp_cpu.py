"""CPU-side checks of the point-to-line ICP matcher (lgs_icp_*): the symbols are
declared, exported and bound and the struct sizes are the library's; bad
arguments answer without a device; the restatement the GPU tests compare the
device with (tests/icp_oracle.py) is pinned by a committed vector
(tests/golden/icp_kat.json) and its tree sums agree with math.fsum within the
tree's bound; the host-only code runs under the sanitizers in a stand-alone
program (tests/cpp_icp/icp_host_check.cpp)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import icp_oracle as orc
from lgs_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CHECK = os.path.join(ROOT, "tests", "cpp_icp", "build", "icp_host_check")
KAT = os.path.join(ROOT, "tests", "golden", "icp_kat.json")
LGS_ERR_INVALID_ARG = 1
NAMES = ("lgs_icp_optimize_pose", "lgs_icp_optimize_pose_batch", "lgs_icp_pairs", "lgs_icp_params_size",
         "lgs_icp_summary_size")


def test_declared_exported_and_bound():
    hip_h = open(os.path.join(ROOT, "include", "lgs_hip.h")).read()
    lib = C.CDLL(abi.LIB_PATH)
    for name in NAMES:
        assert name + "(" in hip_h, name
        assert hasattr(lib, name), name
        assert name in abi.SYMBOLS, name
    for name in ("icp", "icp_batch", "icp_pairs"):
        assert hasattr(abi.Context, name), name


def test_struct_sizes_are_the_librarys():
    lib = abi.load()
    assert lib.lgs_icp_params_size() == C.sizeof(abi.IcpParams) == 64
    assert lib.lgs_icp_summary_size() == C.sizeof(abi.IcpSummary)
    assert abi.IcpSummary.hessian.offset + 9 * 8 == abi.IcpSummary.rhs.offset


def test_abi_version_unchanged():
    """entry points were added, none changed: the version stays, as with every earlier addition"""
    assert abi.load().lgs_abi_version() == 2


def test_bad_arguments_answer_without_a_device():
    lib = abi.load()
    P = abi.Pose2D
    out = abi.IcpSummary()
    prm = abi.IcpParams(5, 0.0, 0.01, 20.0, 1e-3, 1e-3, 1.0, 0.5)
    assert lib.lgs_icp_optimize_pose(None, None, P(0, 0, 0), None, P(0, 0, 0), C.byref(prm), C.byref(out), None) == \
        LGS_ERR_INVALID_ARG
    assert lib.lgs_icp_optimize_pose_batch(None, None, None, None, None, 0, C.byref(prm), None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_icp_pairs(None, None, P(0, 0, 0), None, P(0, 0, 0), C.byref(prm), None, None) == LGS_ERR_INVALID_ARG


def _f(h):
    return float.fromhex(h)


def _kat():
    d = json.load(open(KAT))
    prm = orc.Params(d["params"]["num_iterations_max"], *[_f(x) for x in d["params"]["doubles"]])
    arr = lambda v: np.array([_f(x) for x in v])
    ref = orc.ScanIn(arr(d["ref"]["ranges"]), arr(d["ref"]["angles"]), tuple(arr(d["ref"]["rel"])))
    cur = orc.ScanIn(arr(d["scan"]["ranges"]), arr(d["scan"]["angles"]), tuple(arr(d["scan"]["rel"])))
    return d, prm, ref, tuple(arr(d["ref"]["pose"])), cur, tuple(arr(d["scan"]["initial_pose"]))


def test_restatement_is_pinned_by_the_committed_vector():
    """a 64-beam refine of 8 steps: every pose, cost and pair count of the
    trajectory and the summary, bit for bit"""
    d, prm, ref, ref_pose, cur, init = _kat()
    r = orc.refine(prm, ref, ref_pose, cur, init)
    w = d["result"]
    assert len(ref.ranges) == len(cur.ranges) == 64
    assert (r.pose_found, r.iterations, r.num_pairs, r.initial_pairs) == \
        (w["pose_found"], w["iterations"], w["num_pairs"], w["initial_pairs"]) and r.iterations == 8
    hx = lambda v: [float(x).hex() for x in v]
    assert [float(r.cost).hex(), float(r.pair_cost).hex(), float(r.initial_cost).hex()] == \
        [w["cost"], w["pair_cost"], w["initial_cost"]]
    assert hx(r.best_sensor_pose) == w["best_sensor_pose"]
    assert hx(r.estimated_pose) == w["estimated_pose"]
    assert hx(r.hessian) == w["hessian"]
    assert hx(r.covariance) == w["covariance"]
    assert [hx(t) for t in r.trajectory] == w["trajectory"]
    assert r.cost < r.initial_cost


@pytest.mark.parametrize("n", [64, 1500, 2100])
def test_tree_sums_agree_with_fsum(n):
    """the kernel's tree on the terms of a real pass (64 beams, the vector's) and on
    random terms of mixed sign with beams skipped: within k 2^-53 sum |term|"""
    if n == 64:
        _, prm, ref, ref_pose, cur, init = _kat()
        table = orc.ref_table(prm, ref, orc.compound(ref_pose, ref.rel))
        b = orc.pass_beams(prm, table, cur, orc.compound(init, cur.rel))
        assert (b.state >= 0).sum() >= 3
    else:
        rng = np.random.default_rng(n)
        terms = rng.standard_normal((orc.SUMS, n)) * 10.0 ** rng.integers(-6, 6, (orc.SUMS, n))
        contrib = rng.random((orc.SUMS, n)) < 0.8
        b = orc.Beams(np.zeros(n, dtype=np.int64), np.zeros(n), terms, contrib)
    s, _ = orc.pass_sums(b)
    exact, absum = orc.pass_fsums(b)
    k = orc.tree_depth(n)
    assert k == (n + 1023) // 1024 - 1 + 6 + 15
    for q in range(orc.SUMS):
        assert abs(s[q] - exact[q]) <= k * 2.0 ** -53 * absum[q], q


def test_tree_sum_of_nothing_is_plus_zero():
    assert orc.tree_sum(np.zeros(0), np.zeros(0, dtype=bool)) == 0.0
    assert np.float64(orc.tree_sum(np.array([-0.0]), np.array([False]))).tobytes() == np.float64(0.0).tobytes()


def test_a_nan_pose_pairs_nothing():
    """the loop's rule for a NaN pose: every usable beam is rejected, so the pass has no pairs"""
    _, prm, ref, ref_pose, cur, _ = _kat()
    table = orc.ref_table(prm, ref, orc.compound(ref_pose, ref.rel))
    lo, hi = orc.usable_range(prm, cur)
    usable = int(orc.usable_mask(cur.ranges, lo, hi).sum())
    for pose in ((float("nan"), 0.0, 0.0), (0.0, 0.0, float("nan"))):
        b = orc.pass_beams(prm, table, cur, pose)
        s, pairs = orc.pass_sums(b)
        assert pairs == 0 and (b.state == -1).sum() == usable
        assert s[1] == 0.0 and s[0] > 0.0


def test_host_code_under_the_sanitizers():
    """argument checks, the usable count behind the table cap and the covariance, compiled with
    -fsanitize=address,undefined into a program of their own (make cpptest)"""
    assert os.path.exists(HOST_CHECK), "build first: make -C <repo> all"
    r = subprocess.run([HOST_CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ICP HOST CHECKS PASSED" in r.stdout
