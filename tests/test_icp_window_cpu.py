"""CPU-side checks of the ICP loop detector's window search (lgs_icp_window,
lgs_icp_ref_window_scores, lgs_loop_detect_icp, lgs_icp_window_stats; DESIGN.md
4.5e): the symbols are declared, exported and bound and the ABI version and
struct sizes hold; bad arguments answer without a device and leave the outputs
untouched; the committed vector (tests/golden/icp_window_kat.json) pins the
restatement (tests/icp_window_oracle.py); the host-only code
(csrc/icp_window_host.hpp) runs under the sanitizers in a stand-alone program
(tests/cpp_icp_window/icp_window_host_check.cpp); the adapter's driver links."""
import ctypes as C
import importlib.util
import json
import math
import os
import subprocess


import icp_window_oracle as worc
from lgs_amd import abi, loopbatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CHECK = os.path.join(ROOT, "tests", "cpp_icp_window", "build", "icp_window_host_check")
ADAPTER = os.path.join(ROOT, "tests", "cpp_icp_window", "build", "icp_window_adapter_test")
KAT = os.path.join(ROOT, "tests", "golden", "icp_window_kat.json")
LGS_ERR_INVALID_ARG = 1
INF, NAN = float("inf"), float("nan")
NAMES = ("lgs_icp_window_size", "lgs_icp_ref_window_scores", "lgs_loop_detect_icp", "lgs_icp_window_stats")


def test_declared_exported_and_bound():
    hip_h = open(os.path.join(ROOT, "include", "lgs_hip.h")).read()
    lib = C.CDLL(abi.LIB_PATH)
    for name in NAMES:
        assert name + "(" in hip_h, name
        assert hasattr(lib, name), name
        assert name in abi.SYMBOLS, name
    assert "#define LGS_ICP_WINDOW_MAX_POSES 1048576" in hip_h
    assert "#define LGS_ICP_WINDOW_MAX_BEAMS 4096" in hip_h
    assert "} lgs_icp_window;" in hip_h
    for name in ("icp_window_scores", "loop_detect_icp", "icp_window_stats"):
        assert hasattr(abi.Context, name), name
    assert hasattr(abi, "IcpWindow") and hasattr(loopbatch, "hip_detect_fn_icp")


def test_abi_version_and_struct_sizes():
    lib = abi.load()
    assert lib.lgs_abi_version() == 2
    assert lib.lgs_icp_window_size() == C.sizeof(abi.IcpWindow) == 32
    assert C.sizeof(abi.LoopResult) == 176 and C.sizeof(abi.LoopRefineGate) == 32
    assert lib.lgs_icp_params_size() == C.sizeof(abi.IcpParams) == 64
    assert lib.lgs_icp_summary_size() == C.sizeof(abi.IcpSummary)


def test_the_binding_states_the_lattice():
    w = abi.IcpWindow(5, 5, 3, 0.1, 0.05)
    o = worc.Window(5, 5, 3, 0.1, 0.05)
    assert w.shape == (7, 11, 11) and worc.dims(o) == (11, 11, 7) and worc.num_poses(o) == 847
    centre = (-0.5, 0.65, -0.2)
    for p in (0, 1, 11, 121, 423, 745, 846):
        assert w.pose(centre, p) == worc.lattice_pose(o, centre, p)
        assert worc.index(o, *worc.decode(o, p)) == p
    assert worc.decode(o, 745) == (8, 1, 6) and worc.lattice_pose(o, centre, 423) == centre
    # the centre index gives the centre itself, the sign of a zero included
    assert math.copysign(1.0, worc.lattice_pose(o, (-0.0, 0.0, -0.0), 423)[0]) == -1.0
    assert math.copysign(1.0, w.pose((-0.0, 0.0, -0.0), 423)[2]) == -1.0


def test_the_selection_rule():
    assert worc.select([]) == -1 and worc.select([INF, NAN, INF]) == -1
    assert worc.select([3.0, 1.0, 2.0, 1.0]) == 1 and worc.select([NAN, 5.0, INF, 5.0]) == 1
    assert worc.select([0.0, -0.0]) == 0 and worc.select([1.7e308, INF]) == 0


# ------------------------------------------------------------------ bad arguments, no device
class Poisoned:
    """the outputs of the two entry points, filled with a pattern"""

    def __init__(self, P=27, n=2):
        self.cost = (C.c_double * P)(*[7.5] * P)
        self.pairs = (C.c_int * P)(*[77] * P)
        self.recs = (abi.LoopResult * n)()
        self.best = (C.c_int * n)(*[77] * n)
        self.sums = (abi.IcpSummary * n)()
        C.memset(self.recs, 0xAB, C.sizeof(self.recs))
        C.memset(self.sums, 0xAB, C.sizeof(self.sums))
        self.before = self.snapshot()

    def snapshot(self):
        return bytes(self.cost), bytes(self.pairs), bytes(self.recs), bytes(self.best), bytes(self.sums)

    def untouched(self):
        return self.snapshot() == self.before


BAD_WINDOWS = [(-1, 0, 0, 0.1, 0.1), (0, 513, 0, 0.1, 0.1), (0, 0, -2, 0.1, 0.1), (0, 0, 2 ** 31 - 1, 0.1, 0.1),
               (1, 1, 1, 0.0, 0.1), (1, 1, 1, 0.1, -0.1), (1, 1, 1, NAN, 0.1), (1, 1, 1, 0.1, INF), (1, 1, 1, -INF, 0.1),
               (512, 512, 0, 0.1, 0.1), (51, 50, 50, 0.1, 0.1)]
BAD_PARAMS = [(5, 0.0, 0.01, 20.0, 1e-3, 1e-3, 0.0, 0.5), (5, NAN, 0.01, 20.0, 1e-3, 1e-3, 1.0, 0.5),
              (5, 0.0, 0.01, 20.0, -1e-3, 1e-3, 1.0, 0.5), (5, 0.0, 0.01, INF, 1e-3, 1e-3, 1.0, 0.5)]
BAD_GATES = [(2, 1.0, 1.0, 1.0), (3, NAN, 1.0, 1.0), (3, 1.0, -1.0, 1.0), (3, 1.0, 1.0, -INF)]


def test_bad_arguments_answer_without_a_device():
    """Every rule that the entry points check before they look at the context: with no device there is no
    context, so a block of zero bytes stands in for it (and for the reference and the scan) wherever the
    argument under test is another one -- none of these calls may read it, and each must leave every output
    as it found it."""
    lib = abi.load()
    prm = abi.IcpParams(5, 0.0, 0.01, 20.0, 1e-3, 1e-3, 1.0, 0.5)
    win = abi.IcpWindow(1, 1, 1, 0.1, 0.05)
    gate = abi.LoopRefineGate(3, 1.0, 1.0, 1.0)
    blank = C.create_string_buffer(1 << 16)
    fake = C.cast(blank, C.c_void_p)
    refs = (C.c_void_p * 1)(fake)
    qs = (abi.LoopQuery * 1)(abi.LoopQuery(None, None, abi.Pose2D(0, 0, 0), 0, 0, 2))
    cs = (abi.LoopCandidate * 2)(abi.LoopCandidate(fake, abi.Pose2D(0, 0, 0), 1, 0),
                                 abi.LoopCandidate(fake, abi.Pose2D(0, 0, 0), 2, 0))
    o = Poisoned()

    def scores(ctx=fake, ref=fake, scan=fake, w=win, p=prm, cost=o.cost, pairs=o.pairs):
        return lib.lgs_icp_ref_window_scores(ctx, ref, scan, abi.Pose2D(0.0, 0.0, 0.0), C.byref(w) if w else None,
                                             C.byref(p) if p else None, cost, pairs)

    def detect(ctx=fake, r=refs, q=qs, c=cs, p=prm, w=win, g=gate, recs=o.recs):
        return lib.lgs_loop_detect_icp(ctx, r, q, 1, c, 2, C.byref(p) if p else None, C.byref(w) if w else None,
                                       C.byref(g) if g else None, recs, o.best, o.sums)

    # a NULL argument, the optional outputs apart
    for kw in ({"ctx": None}, {"ref": None}, {"scan": None}, {"w": None}, {"p": None}, {"cost": None}, {"pairs": None}):
        assert scores(**kw) == LGS_ERR_INVALID_ARG and o.untouched(), kw
    for kw in ({"ctx": None}, {"r": None}, {"q": None}, {"c": None}, {"p": None}, {"w": None}, {"g": None},
               {"recs": None}):
        assert detect(**kw) == LGS_ERR_INVALID_ARG and o.untouched(), kw
    # the window: a half outside 0 .. 512, a step that is not finite or <= 0, more than 1048576 poses
    for w in BAD_WINDOWS:
        assert scores(w=abi.IcpWindow(*w)) == LGS_ERR_INVALID_ARG and o.untouched(), w
        assert detect(w=abi.IcpWindow(*w)) == LGS_ERR_INVALID_ARG and o.untouched(), w
    # the parameter rules of lgs_icp_*, the gate rules of lgs_loop_refine_icp
    for p in BAD_PARAMS:
        assert scores(p=abi.IcpParams(*p)) == LGS_ERR_INVALID_ARG and o.untouched(), p
        assert detect(p=abi.IcpParams(*p)) == LGS_ERR_INVALID_ARG and o.untouched(), p
    for g in BAD_GATES:
        assert detect(g=abi.LoopRefineGate(*g)) == LGS_ERR_INVALID_ARG and o.untouched(), g
    v = C.c_longlong(7)
    assert lib.lgs_icp_window_stats(None, C.byref(v), None, None, None) == LGS_ERR_INVALID_ARG and v.value == 7
    assert bytes(blank) == bytes(1 << 16)


# ------------------------------------------------------------------ the vector
def _make_kat():
    spec = importlib.util.spec_from_file_location("make_icp_window_kat",
                                                  os.path.join(ROOT, "tests", "golden", "make_icp_window_kat.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_vector_pins_the_restatement():
    doc = json.load(open(KAT))
    want = doc.pop("result")
    _, got = _make_kat().compute(doc)
    assert got["poses"] == want["poses"]
    assert got["cost"] == want["cost"] and got["pairs"] == want["pairs"] and got["best"] == want["best"]
    assert got["refine"] == want["refine"]
    assert got["gate_terms"] == want["gate_terms"] and got["accepted"] == want["accepted"]
    for name in ("record", "record_rejected", "record_none"):
        assert got[name] == want[name], name
    # what the vector shows: a unique minimum away from the centre, an accepted and a rejected record that
    # differ only in found and the loop edge, and a record without a refine that holds the indices and the node
    cost = [float.fromhex(c) for c in want["cost"]]
    assert want["best"] not in (-1, 13) and sorted(cost)[0] < sorted(cost)[1] and want["accepted"] is True
    a, r, z = (abi.LoopResult.from_buffer_copy(bytes.fromhex(want[n])) for n in ("record", "record_rejected", "record_none"))
    assert (a.found, r.found, z.found) == (1, 0, 0)
    assert bytes(a.estimated_pose) == bytes(r.estimated_pose) and a.score == r.score == want["refine"]["num_pairs"] / 16
    assert bytes(r.relative_pose) == bytes(24) != bytes(a.relative_pose)
    assert (z.start_node_index, z.end_node_index) == (a.start_node_index, a.end_node_index) == (7, 31)
    assert bytes(z)[16:40] == bytes(24) and bytes(z)[64:] == bytes(176 - 64) and bytes(z)[40:64] == bytes(a)[40:64]


# ------------------------------------------------------------------ the stand-alone programs
def test_host_code_under_the_sanitizers():
    """the window's rules, index <-> (ix, iy, it) at every cap, the lattice pose, the slice plan, the combine of
    the partials against brute force and the record, compiled with -fsanitize=address,undefined into a program
    of its own (make cpptest)"""
    assert os.path.exists(HOST_CHECK), "build first: make -C <repo> all"
    r = subprocess.run([HOST_CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ICP WINDOW HOST CHECKS PASSED" in r.stdout and "FAIL" not in r.stdout
    for case in ("window: 1025 x 1023 and 101^3 poses pass, 1025 x 1025, 103 x 101 x 101 and 1025^3 do not",
                 "index: decode(index(ix, iy, it)) is the identity over whole windows, every cap included",
                 "slices: every translation in exactly one slice, none empty, none above the plan's length",
                 "pose: the centre index gives the centre, -0.0 included",
                 "combine: the lexicographic minimum of brute force over 400 random partitions",
                 "combine: nothing wins from no partial; NaN and +inf never win; a tie goes to the lower index",
                 "record: all 176 bytes equal the restatement: no refine, rejected, accepted"):
        assert case in r.stdout, case


def test_adapter_driver_links():
    """LoopDetectorIcpHip against the C-ABI: without a GPU the driver loads both libraries and exits with the
    skip status after Device() threw; with one it runs its checks"""
    assert os.path.exists(ADAPTER), "build first: make -C <repo> all"
    r = subprocess.run([ADAPTER], capture_output=True, text=True, timeout=300)
    if r.returncode == 77:
        assert "no GPU" in r.stdout
    else:
        assert r.returncode == 0 and "ICP WINDOW ADAPTER TESTS PASSED" in r.stdout, r.stdout + r.stderr
