"""CPU-side checks of the device-resident pose-graph optimizer's entry points
(lgs_pg_lm_optimize, lgs_pg_lm_linearize, lgs_pg_lm_stats,
lgs_pose_graph_optimize_lm_resident, lgs_pose_graph_linearize): declared,
exported and bound; bad arguments are refused with the invalid-argument status
before the context is touched, so they answer without a GPU; the host
linearisation, which the device's is compared with byte for byte
(tests/test_gpu_pglm.py), against a dense numpy restatement; and
lgs_pose_graph_optimize_lm, whose OptimizeStep now calls that linearisation,
against the bytes it gave before.  The incidence-list builder runs under the
sanitizers in a stand-alone program (tests/cpp_pglm/pglm_host_check.cpp)."""
import ctypes as C
import inspect
import json
import os
import subprocess

import numpy as np
import pytest

import pglm_graphs as pg
from lgs_amd import abi, io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LGS_ERR_INVALID_ARG = 1
HOST_CHECK = os.path.join(ROOT, "tests", "cpp_pglm", "build", "pglm_host_check")
GOLDEN = os.path.join(ROOT, "tests", "golden", "pglm_host_lm.json")


def test_declared_exported_and_bound():
    hip_h = open(os.path.join(ROOT, "include", "lgs_hip.h")).read()
    io_h = open(os.path.join(ROOT, "include", "lgs_io.h")).read()
    lib = C.CDLL(abi.LIB_PATH)
    for name in ("lgs_pg_lm_optimize", "lgs_pg_lm_linearize", "lgs_pg_lm_stats"):
        assert name + "(" in hip_h, name
        assert hasattr(lib, name), name
        assert name in abi.SYMBOLS, name
    abi.load()
    host = C.CDLL(io.LIB_PATH)
    for name in ("lgs_pose_graph_optimize_lm_resident", "lgs_pose_graph_linearize"):
        assert name + "(" in io_h, name
        assert hasattr(host, name), name
        assert name in io.SYMBOLS, name
    assert "resident" in inspect.signature(io.optimize_lm).parameters
    for name in ("pg_lm_optimize", "pg_lm_linearize", "pg_lm_stats"):
        assert hasattr(abi.Context, name), name
    assert callable(io.linearize)
    assert C.sizeof(abi.PgEdge) == C.sizeof(io.PoseGraphEdge) == 104


def test_abi_version_unchanged():
    assert abi.load().lgs_abi_version() == 2


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _optimize_args(n=2, m=1, start=0, end=1, kind=0, lam=1e-3, tol=1e-6, scale=1.0):
    prm = abi.PgLmParams(10, tol, kind, scale)
    poses = (abi.Pose2D * 2)(abi.Pose2D(0, 0, 0), abi.Pose2D(1, 0, 0))
    edges = abi.pg_edges([(start, end, (1.0, 0.0, 0.0), np.eye(3))])
    keep = [prm, poses, edges, C.c_double(lam), C.c_int(), C.c_double(), C.c_longlong()]
    return keep, [C.byref(prm), C.byref(keep[3]), poses, n, C.cast(edges, C.c_void_p), m, C.byref(keep[4]),
                  C.byref(keep[5]), C.byref(keep[6])]


INVALID = dict(n_zero=dict(n=0), n_negative=dict(n=-1), n_beyond=dict(n=2 ** 27 + 1), m_negative=dict(m=-1),
               m_beyond=dict(m=2 ** 27 + 1), start_negative=dict(start=-1), end_beyond=dict(end=2), kind_negative=dict(kind=-1),
               kind_seven=dict(kind=7), lambda_nan=dict(lam=float("nan")), lambda_inf=dict(lam=float("inf")),
               tolerance_nan=dict(tol=float("nan")), scale_inf=dict(scale=float("-inf")))


@pytest.mark.parametrize("case", list(INVALID))
def test_invalid_arguments_answer_without_a_device(case):
    """each with every pointer present but the context: status 1"""
    lib = abi.load()
    keep, args = _optimize_args(**INVALID[case])
    assert lib.lgs_pg_lm_optimize(None, *args) == LGS_ERR_INVALID_ARG


def test_null_arguments_answer_without_a_device():
    lib = abi.load()
    keep, args = _optimize_args()
    assert lib.lgs_pg_lm_optimize(None, *args) == LGS_ERR_INVALID_ARG
    assert lib.lgs_pg_lm_optimize(None, None, None, None, 1, None, 0, None, None, None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_pg_lm_linearize(None, 0, 1.0, 1e-4, None, 1, None, 0, None, None, None, None, None) == \
        LGS_ERR_INVALID_ARG
    assert lib.lgs_pg_lm_stats(None, None, None, None, None, None) == LGS_ERR_INVALID_ARG
    L = io.load()
    prm = io.LMParams(io.LM_CONJUGATE_GRADIENT, 10, 1e-6, 1e-3, 0, 1.0)
    p = (abi.Pose2D * 1)(abi.Pose2D(0, 0, 0))
    assert L.lgs_pose_graph_optimize_lm_resident(None, C.byref(prm), p, 1, None, 0, None, None) == LGS_ERR_INVALID_ARG
    assert L.lgs_pose_graph_linearize(None, p, 1, None, 0, None, None, None, None, None) == LGS_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        io.optimize_lm([[0.0, 0.0, 0.0]], [], resident=True)


@pytest.mark.parametrize("name", pg.LINEARISE_GRAPHS)
def test_host_linearize_matches_dense(name):
    init, edges = pg.graph(name)
    _check_host_linearize(init, edges, 0, 1.0)


@pytest.mark.parametrize("kind,scale", pg.LOSSES)
def test_host_linearize_every_loss(kind, scale):
    """the 80-node graph with outliers and the self-loop edge, so that the losses' weights differ from 1"""
    init, edges = pg.graph("selfloop")
    _check_host_linearize(init, edges, kind, scale)


def _check_host_linearize(init, edges, kind, scale):
    lam = 1e-4
    diag, pairs, off, rhs = io.linearize(init, edges, lam=lam, loss=kind, scale=scale)
    rdiag, rpairs, roff, rrhs = pg.dense_blocks(init, edges, lam, kind, scale)
    assert pairs.tolist() == rpairs.tolist()      # first-appearance order
    # H's largest entry is the 1e9 anchor: the bound is taken without node 0's block, which is compared at its own scale
    scale_h = max(np.abs(rdiag[1:]).max(initial=0.0), np.abs(roff).max(initial=0.0), lam)
    assert np.abs(diag[1:] - rdiag[1:]).max(initial=0.0) <= 1e-12 * scale_h
    assert np.abs(off - roff).max(initial=0.0) <= 1e-12 * scale_h
    assert np.abs(diag[0] - rdiag[0]).max() <= 1e-12 * np.abs(rdiag[0]).max()
    assert np.abs(rhs - rrhs).max() <= 1e-12 * max(np.abs(rrhs).max(), 1e-300)


def test_optimize_lm_keeps_its_bytes():
    """OptimizeStep calls the factored-out linearisation: the poses, the step
    count, the total error and the damping factor of three runs are the bytes
    recorded before the change"""
    runs = json.load(open(GOLDEN))["runs"]
    assert [(r["graph"], r["solver"], r["loss"], r["scale"]) for r in runs] == pg.GOLDEN_RUNS
    for r in runs:
        init, edges = pg.graph(r["graph"])
        P, it, tot, lam = io.optimize_lm(init, edges, solver=r["solver"], loss=r["loss"], scale=r["scale"],
                                         **pg.GOLDEN_KW)
        assert it == r["iterations"], r["graph"]
        assert P.tobytes().hex() == r["poses"], r["graph"]
        assert np.float64(tot).tobytes().hex() == r["total_error"], r["graph"]
        assert np.float64(lam).tobytes().hex() == r["lambda_"], r["graph"]


def test_host_code_under_the_sanitizers():
    """the argument checks and the incidence-list builder, compiled with
    -fsanitize=address,undefined into a program of their own (make cpptest)"""
    assert os.path.exists(HOST_CHECK), "build first: make -C <repo> all"
    r = subprocess.run([HOST_CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PGLM HOST CHECKS PASSED" in r.stdout
