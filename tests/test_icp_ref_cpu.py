"""CPU-side checks of the multi-scan reference of the point-to-line ICP
(lgs_icp_ref_*): the symbols are declared, exported and bound and the struct
sizes are unchanged; bad arguments answer without a device; the restatement
the GPU tests compare the device with (tests/icp_ref_oracle.py) is pinned by a
committed vector (tests/golden/icp_ref_kat.json); the grid's host-only code
runs against brute force under the sanitizers in a stand-alone program
(tests/cpp_icp_ref/icp_ref_host_check.cpp); the adapter's driver links."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import icp_oracle as orc
import icp_ref_oracle as rorc
from lgs_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CHECK = os.path.join(ROOT, "tests", "cpp_icp_ref", "build", "icp_ref_host_check")
ADAPTER = os.path.join(ROOT, "tests", "cpp_icp_ref", "build", "icp_ref_adapter_test")
KAT = os.path.join(ROOT, "tests", "golden", "icp_ref_kat.json")
LGS_ERR_INVALID_ARG = 1
NAMES = ("lgs_icp_ref_create", "lgs_icp_ref_destroy", "lgs_icp_ref_info", "lgs_icp_ref_optimize_pose",
         "lgs_icp_ref_optimize_pose_batch", "lgs_icp_ref_pairs")


def test_declared_exported_and_bound():
    hip_h = open(os.path.join(ROOT, "include", "lgs_hip.h")).read()
    lib = C.CDLL(abi.LIB_PATH)
    for name in NAMES:
        assert name + "(" in hip_h, name
        assert hasattr(lib, name), name
        assert name in abi.SYMBOLS, name
    assert "#define LGS_ICP_REF_MAX_ENTRIES 262144" in hip_h
    assert hasattr(abi.Context, "icp_ref")
    for name in ("info", "refine", "refine_batch", "pairs", "close"):
        assert hasattr(abi.IcpRef, name), name


def test_struct_sizes_and_abi_version_unchanged():
    lib = abi.load()
    assert lib.lgs_icp_params_size() == C.sizeof(abi.IcpParams) == 64
    assert lib.lgs_icp_summary_size() == C.sizeof(abi.IcpSummary)
    assert lib.lgs_abi_version() == 2


def test_bad_arguments_answer_without_a_device():
    lib = abi.load()
    P = abi.Pose2D
    out = abi.IcpSummary()
    prm = abi.IcpParams(5, 0.0, 0.01, 20.0, 1e-3, 1e-3, 1.0, 0.5)
    h = C.c_void_p()
    assert lib.lgs_icp_ref_create(None, None, None, 1, C.byref(prm), C.byref(h)) == LGS_ERR_INVALID_ARG
    assert lib.lgs_icp_ref_create(None, None, None, 0, None, None) == LGS_ERR_INVALID_ARG
    assert h.value is None
    assert lib.lgs_icp_ref_info(None, None, None, None, None, None, None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_icp_ref_optimize_pose(None, None, None, P(0, 0, 0), C.byref(prm), C.byref(out), None) == \
        LGS_ERR_INVALID_ARG
    assert lib.lgs_icp_ref_optimize_pose_batch(None, None, None, None, 0, C.byref(prm), None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_icp_ref_pairs(None, None, None, P(0, 0, 0), C.byref(prm), None, None, None) == LGS_ERR_INVALID_ARG
    lib.lgs_icp_ref_destroy(None)


def _f(h):
    return float.fromhex(h)


def _kat():
    d = json.load(open(KAT))
    prm = orc.Params(d["params"]["num_iterations_max"], *[_f(x) for x in d["params"]["doubles"]])
    arr = lambda v: np.array([_f(x) for x in v])
    refs = [orc.ScanIn(arr(r["ranges"]), arr(r["angles"]), tuple(arr(r["rel"]))) for r in d["refs"]]
    poses = [tuple(arr(r["pose"])) for r in d["refs"]]
    cur = orc.ScanIn(arr(d["scan"]["ranges"]), arr(d["scan"]["angles"]), tuple(arr(d["scan"]["rel"])))
    return d, prm, refs, poses, cur, tuple(arr(d["scan"]["initial_pose"]))


def test_restatement_is_pinned_by_the_committed_vector():
    """3 reference scans of 16 beams, 2 steps: the concatenated table with the (k, j) of every entry, the
    pairs at the initial pose, the trajectory and the summary, bit for bit"""
    d, prm, refs, poses, cur, init = _kat()
    hx = lambda v: [float(x).hex() for x in v]
    assert len(refs) == 3 and all(len(r.ranges) == 16 for r in refs) and len(cur.ranges) == 16
    rt = rorc.concat_tables(prm, refs, poses)
    t = d["table"]
    assert (rt.k.tolist(), rt.j.tolist()) == (t["k"], t["j"])
    assert rt.table.idx.tolist() == list(range(len(t["k"])))
    assert (hx(rt.table.qx), hx(rt.table.qy), hx(rt.table.nx), hx(rt.table.ny)) == (t["qx"], t["qy"], t["nx"], t["ny"])
    # scan order, then beam order; every scan contributes
    assert rt.k.tolist() == sorted(rt.k.tolist()) and set(rt.k.tolist()) == {0, 1, 2}
    assert all(a < b for a, b, ka, kb in zip(rt.j[:-1], rt.j[1:], rt.k[:-1], rt.k[1:]) if ka == kb)
    k, j, e, _ = rorc.pairs(prm, rt, cur, orc.compound(init, cur.rel))
    w = d["pairs_at_initial_pose"]
    assert (k.tolist(), j.tolist(), hx(e)) == (w["k"], w["j"], w["e"])
    assert (k >= 0).sum() >= 3
    r = rorc.refine(prm, refs, poses, cur, init, rt)
    w = d["result"]
    assert (r.pose_found, r.iterations, r.num_pairs, r.initial_pairs) == \
        (w["pose_found"], w["iterations"], w["num_pairs"], w["initial_pairs"]) and r.iterations == 2
    assert [float(r.cost).hex(), float(r.pair_cost).hex(), float(r.initial_cost).hex()] == \
        [w["cost"], w["pair_cost"], w["initial_cost"]]
    assert hx(r.best_sensor_pose) == w["best_sensor_pose"]
    assert hx(r.estimated_pose) == w["estimated_pose"]
    assert hx(r.hessian) == w["hessian"]
    assert hx(r.covariance) == w["covariance"]
    assert [hx(s) for s in r.trajectory] == w["trajectory"]
    assert r.cost < r.initial_cost


def test_lines_never_cross_scans():
    """the last beam of one scan and the first of the next are neighbours in the concatenation only"""
    a = np.array([0.0, 0.01, 0.02, 0.03])
    whole = orc.ScanIn(np.full(4, 2.0), a)
    halves = [orc.ScanIn(np.full(1, 2.0), a[:1]), orc.ScanIn(np.full(3, 2.0), a[1:])]
    prm = orc.Params(1, 0.0, 0.01, 20.0, 0.0, 0.0, 0.5, 0.5)
    O = (0.0, 0.0, 0.0)
    one = rorc.concat_tables(prm, [whole], [O])
    two = rorc.concat_tables(prm, halves, [O, O])
    assert not np.isnan(one.table.nx).any()
    assert np.isnan(two.table.nx).tolist() == [True, False, False, False]
    assert (two.k.tolist(), two.j.tolist()) == ([0, 1, 1, 1], [0, 0, 1, 2])
    assert two.table.qx.tobytes() == one.table.qx.tobytes()


def test_host_code_under_the_sanitizers():
    """grid geometry, the cell function and its clamping against brute force over every entry, compiled with
    -fsanitize=address,undefined into a program of its own (make cpptest)"""
    assert os.path.exists(HOST_CHECK), "build first: make -C <repo> all"
    r = subprocess.run([HOST_CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ICP REF HOST CHECKS PASSED" in r.stdout
    for case in ("coordinates near 1e5, D = 0.01", "D = 1e-3 over 24 m", "D = 100 over 10 m", "all points equal",
                 "points on one axis", "visit no cell"):
        assert case in r.stdout, case


def test_adapter_driver_links_and_reports_missing_device():
    """CPU: the adapter and the C-ABI library load; without a GPU the driver exits with the skip status
    after Device() threw (with one, tests/test_gpu_icp_ref.py runs it on a case file)"""
    assert os.path.exists(ADAPTER), "build first: make -C <repo> all"
    r = subprocess.run([ADAPTER], capture_output=True, text=True, timeout=120)
    if r.returncode == 2 and "usage" in r.stdout:
        pytest.skip("a GPU is present: covered by the gpu test")
    assert r.returncode == 77, r.stdout + r.stderr
    assert "no GPU" in r.stdout
