"""CPU-side checks of the ICP reference set and the ICP loop refinement
(lgs_icp_ref_set_*, lgs_loop_refine_icp): the symbols are declared, exported
and bound and the ABI version and struct sizes are unchanged; bad arguments
answer without a device; the host-only code (csrc/icp_ref_set_host.hpp) runs
under the sanitizers in a stand-alone program
(tests/cpp_icp_ref_set/icp_ref_set_host_check.cpp); the adapter's driver links."""
import ctypes as C
import os
import subprocess

from lgs_amd import abi, loopbatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CHECK = os.path.join(ROOT, "tests", "cpp_icp_ref_set", "build", "icp_ref_set_host_check")
ADAPTER = os.path.join(ROOT, "tests", "cpp_icp_ref_set", "build", "icp_ref_set_adapter_test")
LGS_ERR_INVALID_ARG = 1
NAMES = ("lgs_icp_ref_set_create", "lgs_icp_ref_set_destroy", "lgs_icp_ref_set_size", "lgs_icp_ref_set_ref",
         "lgs_icp_ref_set_stats", "lgs_loop_refine_icp")


def test_declared_exported_and_bound():
    hip_h = open(os.path.join(ROOT, "include", "lgs_hip.h")).read()
    lib = C.CDLL(abi.LIB_PATH)
    for name in NAMES:
        assert name + "(" in hip_h, name
        assert hasattr(lib, name), name
        assert name in abi.SYMBOLS, name
    assert "#define LGS_ICP_REF_SET_MAX_ENTRIES 4194304" in hip_h
    assert "#define LGS_ICP_REF_SET_MAX_CELLS   16777216" in hip_h
    assert "} lgs_loop_refine_gate;" in hip_h
    for name in ("icp_ref_set", "icp_ref_set_stats", "loop_refine_icp"):
        assert hasattr(abi.Context, name), name
    for name in ("__len__", "__getitem__", "close"):
        assert hasattr(abi.IcpRefSet, name), name
    assert hasattr(loopbatch, "refine_icp")


def test_abi_version_and_struct_sizes():
    lib = abi.load()
    assert lib.lgs_abi_version() == 2
    assert C.sizeof(abi.LoopRefineGate) == 32 and C.sizeof(abi.LoopResult) == 176
    assert lib.lgs_icp_params_size() == C.sizeof(abi.IcpParams) == 64
    assert lib.lgs_icp_summary_size() == C.sizeof(abi.IcpSummary)


def test_a_borrowed_view_is_not_destroyed_by_close():
    class Lib:
        calls = []

        def lgs_icp_ref_destroy(self, h):
            self.calls.append(h)

    class Ctx:
        lib = Lib()

    view = abi.IcpRef(Ctx(), C.c_void_p(0x1000), borrowed=True)
    view.close()
    assert view.h and Ctx.lib.calls == []
    own = abi.IcpRef(Ctx(), C.c_void_p(0x2000))
    own.close()
    assert own.h is None and len(Ctx.lib.calls) == 1


def test_bad_arguments_answer_without_a_device():
    lib = abi.load()
    prm = abi.IcpParams(5, 0.0, 0.01, 20.0, 1e-3, 1e-3, 1.0, 0.5)
    gate = abi.LoopRefineGate(3, 1.0, 1.0, 1.0)
    h = C.c_void_p()
    lo, hi = (C.c_int * 1)(0), (C.c_int * 1)(0)
    assert lib.lgs_icp_ref_set_create(None, None, None, 1, lo, hi, 1, C.byref(prm), C.byref(h)) == LGS_ERR_INVALID_ARG
    assert lib.lgs_icp_ref_set_create(None, None, None, 0, None, None, 0, None, None) == LGS_ERR_INVALID_ARG
    assert h.value is None
    assert lib.lgs_icp_ref_set_size(None) == 0
    assert lib.lgs_icp_ref_set_ref(None, 0) is None
    lib.lgs_icp_ref_set_destroy(None)
    v = C.c_longlong(7)
    assert lib.lgs_icp_ref_set_stats(None, C.byref(v), None, None, None, None, None, None) == LGS_ERR_INVALID_ARG
    assert v.value == 7
    recs = (abi.LoopResult * 1)()
    refined = (C.c_int * 1)(77)
    assert lib.lgs_loop_refine_icp(None, None, None, 0, None, 0, C.byref(prm), C.byref(gate), recs, refined, None) == \
        LGS_ERR_INVALID_ARG
    assert refined[0] == 77 and bytes(recs) == bytes(176)


def test_host_code_under_the_sanitizers():
    """the range checks, the offsets, the block list, the box reduction, the caps, the gate at both sides of
    every threshold and the record update, compiled with -fsanitize=address,undefined into a program of its
    own (make cpptest)"""
    assert os.path.exists(HOST_CHECK), "build first: make -C <repo> all"
    r = subprocess.run([HOST_CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ICP REF SET HOST CHECKS PASSED" in r.stdout and "FAIL" not in r.stdout
    for case in ("block list: no straddling, no empty block, all entries covered once",
                 "block list: 130 + 195 + 65 + 65 entries are four blocks, not two",
                 "offsets: 256-byte aligned, disjoint, in reference order", "caps: 17 legal references",
                 "cells: 17 x 1024 x 1024 is LGS_ERR_OOM", "gate: translation at both sides of d2 == T * T",
                 "gate: a NaN in the cost, the estimate or the record rejects even at +inf",
                 "update: all 176 bytes equal the restatement", "queries: a gap"):
        assert case in r.stdout, case


def test_adapter_driver_links():
    """IcpReferenceSetHip and LoopRefinerIcpHip against the C-ABI: without a GPU the driver loads both
    libraries and exits with the skip status after Device() threw; with one it runs its checks"""
    assert os.path.exists(ADAPTER), "build first: make -C <repo> all"
    r = subprocess.run([ADAPTER], capture_output=True, text=True, timeout=300)
    if r.returncode == 77:
        assert "no GPU" in r.stdout
    else:
        assert r.returncode == 0 and "ICP REF SET ADAPTER TESTS PASSED" in r.stdout, r.stdout + r.stderr
