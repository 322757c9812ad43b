"""CPU-side checks of the pose-graph conjugate-gradient entry points
(lgs_pg_cg_solve, lgs_pose_graph_optimize_lm_device, io.optimize_lm(ctx=...)):
declared, exported, bound, and bad arguments are refused with the
invalid-argument status before the context is touched, so they answer without a
GPU.  The solver's host code (argument checks, block pattern) runs under the
sanitizers in a stand-alone program (tests/cpp_pgcg/pgcg_host_check.cpp)."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np

from lgs_amd import abi, io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LGS_ERR_INVALID_ARG = 1
HOST_CHECK = os.path.join(ROOT, "tests", "cpp_pgcg", "build", "pgcg_host_check")


def test_declared_exported_and_bound():
    hip_h = open(os.path.join(ROOT, "include", "lgs_hip.h")).read()
    io_h = open(os.path.join(ROOT, "include", "lgs_io.h")).read()
    assert "lgs_pg_cg_solve(" in hip_h and "lgs_pg_cg_stats(" in hip_h
    assert "lgs_pose_graph_optimize_lm_device(" in io_h
    lib = C.CDLL(abi.LIB_PATH)
    for name in ("lgs_pg_cg_solve", "lgs_pg_cg_stats"):
        assert hasattr(lib, name), name
        assert name in abi.SYMBOLS, name
    abi.load()
    host = C.CDLL(io.LIB_PATH)
    assert hasattr(host, "lgs_pose_graph_optimize_lm_device")
    assert "lgs_pose_graph_optimize_lm_device" in io.SYMBOLS
    assert "ctx" in inspect.signature(io.optimize_lm).parameters
    assert hasattr(abi.Context, "pg_cg_solve")


def test_abi_version_unchanged():
    assert abi.load().lgs_abi_version() == 2


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_null_and_malformed_arguments_are_rejected_without_a_device():
    lib = abi.load()
    diag = np.tile(np.eye(3).reshape(9), 2)
    pairs = np.array([[0, 1]], dtype=np.int32)
    off = np.zeros(9)
    rhs, x = np.ones(6), np.zeros(6)
    it, res = C.c_int(), C.c_double()
    ip = pairs.ctypes.data_as(C.POINTER(C.c_int))
    # every argument present but the context
    assert lib.lgs_pg_cg_solve(None, 2, _d(diag), 1, ip, _d(off), _d(rhs), 0.0, 0, _d(x), C.byref(it),
                               C.byref(res)) == LGS_ERR_INVALID_ARG
    assert lib.lgs_pg_cg_solve(None, 0, None, 0, None, None, None, 0.0, 0, None, None, None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_pg_cg_solve(None, 2, _d(diag), 1, ip, _d(off), _d(rhs), -1.0, -3, _d(x), C.byref(it),
                               C.byref(res)) == LGS_ERR_INVALID_ARG
    assert lib.lgs_pg_cg_stats(None, None, None, None, None) == LGS_ERR_INVALID_ARG
    L = io.load()
    prm = io.LMParams(io.LM_CONJUGATE_GRADIENT, 10, 1e-6, 1e-3, 0, 1.0)
    p = (abi.Pose2D * 1)(abi.Pose2D(0, 0, 0))
    assert L.lgs_pose_graph_optimize_lm_device(None, C.byref(prm), p, 1, None, 0, None, None) == LGS_ERR_INVALID_ARG
    assert L.lgs_pose_graph_optimize_lm_device(None, None, None, 0, None, 0, None, None) == LGS_ERR_INVALID_ARG


def test_host_code_under_the_sanitizers():
    """the argument checks and the block-pattern builder, compiled with
    -fsanitize=address,undefined into a program of their own (make cpptest)"""
    assert os.path.exists(HOST_CHECK), "build first: make -C <repo> all"
    r = subprocess.run([HOST_CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PGCG HOST CHECKS PASSED" in r.stdout
