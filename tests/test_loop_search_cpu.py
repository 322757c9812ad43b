"""CPU-side checks of the nearest-node loop searcher (lgs_loop_*, DESIGN.md
4.6g): the symbols are declared, exported and bound; the restatement
(tests/loop_search_oracle.py) is pinned by a committed vector; the host
function lgs_loop_search_nearest_host and lgs_pg_accum_travel_dist equal the
restatement byte for byte on every case the GPU tests use; every invalid
argument answers LGS_ERR_INVALID_ARG and writes nothing; a record is the
lowest-map strict minimum of its per-map row; candidates_from_search against
a hand-built list; the host-only code runs against brute force under the
sanitizers in a stand-alone program."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import loop_search_cases as lc
import loop_search_oracle as orc
from lgs_amd import abi, loopbatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CHECK = os.path.join(ROOT, "tests", "cpp_loop_search", "build", "loop_search_host_check")
KAT = os.path.join(ROOT, "tests", "golden", "loop_search_kat.json")
LGS_ERR_INVALID_ARG = 1
NAMES = ("lgs_loop_graph_create", "lgs_loop_graph_destroy", "lgs_loop_graph_info", "lgs_loop_graph_travel",
         "lgs_loop_search_nearest", "lgs_loop_search_nearest_host", "lgs_pg_accum_travel_dist", "lgs_loop_search_stats")
CASES = lc.cases()


def params_of(prm):
    return abi.LoopSearchParams(prm.travel_dist_threshold, prm.node_dist_threshold, prm.num_candidate_nodes, 0)


def test_declared_exported_and_bound():
    hip_h = open(os.path.join(ROOT, "include", "lgs_hip.h")).read()
    lib = C.CDLL(abi.LIB_PATH)
    for name in NAMES:
        assert name + "(" in hip_h, name
        assert hasattr(lib, name), name
        assert name in abi.SYMBOLS, name
    assert "#define LGS_OPT_LOOP_SEARCH_MIN_PAIRS 39" in hip_h and abi.LGS_OPT_LOOP_SEARCH_MIN_PAIRS == 39
    assert "#define LGS_OPT_LOOP_SEARCH_GROUP     40" in hip_h and abi.LGS_OPT_LOOP_SEARCH_GROUP == 40
    assert hasattr(abi.Context, "loop_graph") and hasattr(abi, "loop_search_host") and hasattr(abi, "accum_travel_dist")
    for name in ("info", "travel", "search", "close"):
        assert hasattr(abi.LoopGraph, name), name
    assert abi.load().lgs_abi_version() == 2


def test_struct_layouts():
    assert C.sizeof(abi.LoopSearchHint) == abi.LOOP_HINT_DTYPE.itemsize == 24
    assert C.sizeof(abi.LoopSearchParams) == 24
    assert C.sizeof(abi.LoopSearchResult) == abi.LOOP_RESULT_DTYPE.itemsize == orc.RESULT_DTYPE.itemsize == 32
    assert C.sizeof(abi.LoopSearchMapBest) == abi.LOOP_MAP_BEST_DTYPE.itemsize == orc.MAP_BEST_DTYPE.itemsize == 16
    for st, dt in ((abi.LoopSearchHint, abi.LOOP_HINT_DTYPE), (abi.LoopSearchResult, abi.LOOP_RESULT_DTYPE),
                   (abi.LoopSearchMapBest, abi.LOOP_MAP_BEST_DTYPE)):
        assert [(n, getattr(st, n).offset) for n, _ in st._fields_] == [(n, dt.fields[n][1]) for n in dt.names]
    assert abi.LOOP_RESULT_DTYPE == orc.RESULT_DTYPE and abi.LOOP_MAP_BEST_DTYPE == orc.MAP_BEST_DTYPE


def _f(h):
    return float.fromhex(h)


def test_restatement_is_pinned_by_the_committed_vector():
    """40 lattice nodes (every hypot exact), 5 maps, 10 hints: the travel chain, the records and the per-map
    rows, bit for bit, with each hint's own chain and with the snapshot's"""
    d = json.load(open(KAT))
    poses = [[_f(v) for v in p] for p in d["poses"]]
    lo, hi = d["idx_min"], d["idx_max"]
    prm = orc.Params(_f(d["params"]["travel_dist_threshold"]), _f(d["params"]["node_dist_threshold"]),
                     d["params"]["num_candidate_nodes"])
    hints = [orc.Hint(h[0], h[1], h[2], _f(h[3])) for h in d["hints"]]
    assert len(poses) == 40 and len(lo) == 5 and len(hints) == 10
    travel = orc.travel_chain(poses, lo, hi)
    assert [t.hex() for t in travel] == d["travel"] and len(travel) == 30
    assert all(t == round(t * 8) / 8 for t in travel)      # multiples of 5/8: the chain is exact
    assert orc.accum_travel_dist(poses).hex() == d["accum_travel_dist"]
    for own in (True, False):
        res, tab = orc.search_all(poses, lo, hi, prm, hints, own_chain=own)
        assert [[int(v) for v in list(r)[:6]] + [float(r["dist_sq"]).hex()] for r in res] == d["records"]
        assert [[[int(e["node_idx"]), float(e["dist_sq"]).hex()] for e in row] for row in tab] == d["per_map"]
    found = [r[0] for r in d["records"]]
    assert 0 in found and 1 in found
    assert d["records"][8][:6] == [0, -1, -1, -1, -1, 0]       # accum 0: cut at position 0


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_function_equals_the_restatement(case):
    """records and per-map rows, byte for byte; the restatement forms every hint's own chain, as the reference
    does (at most every third hint of the large cases, to keep the pure-Python loop short)"""
    hints = case.hints if len(case.hints) <= 120 else case.hints[::3]
    rows = lc.hint_rows(hints, abi.LOOP_HINT_DTYPE)
    res, tab = abi.loop_search_host(case.poses, case.idx_min, case.idx_max, params_of(case.prm), rows, per_map=True)
    only = abi.loop_search_host(case.poses, case.idx_min, case.idx_max, params_of(case.prm), rows)
    ores, otab = orc.search_all(case.poses, case.idx_min, case.idx_max, case.prm, hints, own_chain=True)
    assert res.tobytes() == ores.tobytes()
    assert tab.tobytes() == otab.tobytes()
    assert only.tobytes() == res.tobytes()
    assert tab.shape == (len(hints), len(case.idx_min))


def test_cases_hit_their_edges():
    """what each case is there for does happen, in the answers of lgs_loop_search_nearest_host"""
    by = {c.name: c for c in CASES}

    def run(name):
        c = by[name]
        rows = lc.hint_rows(c.hints, abi.LOOP_HINT_DTYPE)
        return c, abi.loop_search_host(c.poses, c.idx_min, c.idx_max, params_of(c.prm), rows, per_map=True)

    c, (res, tab) = run("figure eight")
    assert 40 < res["found"].sum() < len(res) and len(set(res["local_map_idx"])) > 5
    assert (res["walked"] > 0).any() and (res["walked"] == 0).any()
    c, (res, tab) = run("overlapping ranges")
    both = [(r, row) for r, row in zip(res, tab) if r["found"] and 15 <= r["local_map_node_idx"] <= 20]
    assert both and all(r["local_map_idx"] == 0 for r, _ in both)        # the node is in maps 0 and 1: map 0 wins
    assert any(row[1]["node_idx"] == r["local_map_node_idx"] for r, row in both)   # map 1's row names it too
    c, (res, tab) = run("duplicate poses")
    dup = res[res["local_map_node_idx"] == 10]
    assert len(dup) > 0 and not np.isin(res["local_map_node_idx"], [11, 12, 13, 40, 41, 42]).any()
    c, (res, tab) = run("d2 equals the squared threshold")
    assert res["found"].tolist() == [0] and res["walked"].tolist() == [3] and res["dist_sq"].tolist() == [25.0]
    c, (res, tab) = run("d2 just below the squared threshold")
    assert res["found"].tolist() == [1] and res["local_map_node_idx"].tolist() == [0] and res["dist_sq"][0] < 25.0
    c, (res, tab) = run("travel threshold edges")
    walked = res["walked"].tolist()
    for k, p in enumerate((0, 5, 11, 12, 30, 40)):
        # accum - travel == threshold continues past p; one ulp below stops at p; above continues too
        assert walked[3 * k + 1] == p and walked[3 * k] > p and walked[3 * k + 2] > p, (p, walked[3 * k: 3 * k + 3])
    assert walked[-3:] == [0, 0, 41] and res["found"][-3:].tolist() == [0, 0, 1]
    c, (res, tab) = run("fewer maps than the snapshot")
    assert res["found"][:3].tolist() == [0, 0, 0] and res["walked"][:3].tolist() == [0, 0, 0]
    for h, row in zip(c.hints, tab):
        assert (row["node_idx"][h.num_maps - 1:] == -1).all()
    assert (tab["node_idx"][:, :3] >= 0).any()
    c, (res, tab) = run("one map")
    assert res["found"].tolist() == [0] and tab.shape == (1, 1)
    c, (res, tab) = run("no node within range")
    assert not res["found"].any() and (res["walked"] > 0).all() and (res["dist_sq"] == orc.min_sq(c.prm)).all()
    c, (res, tab) = run("widest node range")
    f = res[res["found"] == 1]
    assert len(f) and all(r["node_idx_min"] == c.idx_min[h.latest_local_map_idx] and
                          r["node_idx_max"] == c.idx_max[h.latest_local_map_idx]
                          for r, h in zip(res, c.hints) if r["found"])
    c, (res, tab) = run("poses near 1e5")
    assert res["found"].sum() > 40


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_record_is_the_lowest_map_strict_minimum_of_its_row(case):
    rows = lc.hint_rows(case.hints, abi.LOOP_HINT_DTYPE)
    res, tab = abi.loop_search_host(case.poses, case.idx_min, case.idx_max, params_of(case.prm), rows, per_map=True)
    none = orc.min_sq(case.prm)
    for r, row, h in zip(res, tab, case.hints):
        best, bi = none, -1
        for i, e in enumerate(row):
            assert e["pad_"] == 0
            assert (e["node_idx"] == -1) == (e["dist_sq"] == none) and e["dist_sq"] <= none
            if e["dist_sq"] < best:
                best, bi = e["dist_sq"], i
        if bi < 0:
            assert (r["found"], r["local_map_idx"], r["local_map_node_idx"], r["dist_sq"]) == (0, -1, -1, none)
        else:
            assert (r["found"], r["local_map_idx"], r["local_map_node_idx"], r["dist_sq"]) == \
                (1, bi, row[bi]["node_idx"], best)
            assert case.idx_min[bi] <= row[bi]["node_idx"] <= case.idx_max[bi] and bi < h.num_maps - 1


def test_accum_travel_dist_equals_the_restatement():
    for c in CASES:
        assert abi.accum_travel_dist(c.poses).hex() == orc.accum_travel_dist(c.poses).hex()
    assert abi.accum_travel_dist([[3.0, 4.0]]) == 0.0
    assert abi.accum_travel_dist([[0.0, 0.0, 9.0], [3.0, 4.0, math.nan]]) == 5.0     # theta is not read
    for bad in ([[0.0, math.inf]], [[math.nan, 0.0], [1.0, 1.0]]):
        with pytest.raises(abi.LgsError) as e:
            abi.accum_travel_dist(bad)
        assert e.value.status == LGS_ERR_INVALID_ARG
    out = C.c_double(7.0)
    assert abi.load().lgs_pg_accum_travel_dist(None, 1, C.byref(out)) == LGS_ERR_INVALID_ARG
    p = (abi.Pose2D * 1)(abi.Pose2D(0, 0, 0))
    assert abi.load().lgs_pg_accum_travel_dist(p, 0, C.byref(out)) == LGS_ERR_INVALID_ARG
    assert abi.load().lgs_pg_accum_travel_dist(p, 1, None) == LGS_ERR_INVALID_ARG and out.value == 7.0


def _raw_host(poses, lo, hi, prm, hints, n=None, m=None, q=None, null=()):
    """lgs_loop_search_nearest_host through the raw symbol: (status, results untouched?)"""
    lib = abi.load()
    p = np.ascontiguousarray(poses, dtype=np.float64)
    p = np.ascontiguousarray(np.hstack([p, np.zeros((len(p), 1))]))
    lo, hi = np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32)
    h = lc.hint_rows(hints, abi.LOOP_HINT_DTYPE)
    res = np.full(max(1, len(h)) * 32, 0x55, dtype=np.uint8)
    tab = np.full(max(1, len(h)) * len(lo) * 16, 0x55, dtype=np.uint8)
    args = dict(poses=p.ctypes.data_as(C.POINTER(abi.Pose2D)), lo=lo.ctypes.data_as(C.POINTER(C.c_int)),
                hi=hi.ctypes.data_as(C.POINTER(C.c_int)), prm=C.byref(prm), hints=h.ctypes.data, res=res.ctypes.data)
    for k in null:
        args[k] = None
    rc = lib.lgs_loop_search_nearest_host(args["poses"], len(p) if n is None else n, args["lo"], args["hi"],
                                          len(lo) if m is None else m, args["prm"], args["hints"],
                                          len(h) if q is None else q, args["res"], tab.ctypes.data)
    return rc, bool((res == 0x55).all() and (tab == 0x55).all())


def test_invalid_arguments_answer_without_writing():
    poses = [[float(k), 0.5 * k] for k in range(10)]
    lo, hi = [0, 4, 7], [3, 6, 9]
    P = abi.LoopSearchParams
    good, H = P(1.0, 2.0, 3, 0), orc.Hint
    ok_hint = [H(8, 2, 3, 5.0)]
    rc, untouched = _raw_host(poses, lo, hi, good, ok_hint)
    assert rc == 0 and not untouched
    inf, nan = math.inf, math.nan
    bad = {
        "null poses": dict(null=("poses",)), "null idx_min": dict(null=("lo",)), "null idx_max": dict(null=("hi",)),
        "null params": dict(null=("prm",)), "null hints": dict(null=("hints",)), "null results": dict(null=("res",)),
        "n < 1": dict(n=0), "m < 1": dict(m=0), "q < 0": dict(q=-1),
        "n above 2^27": dict(n=2 ** 27 + 1), "m above 2^27": dict(m=2 ** 27 + 1), "q above 2^27": dict(q=2 ** 27 + 1),
    }
    for name, kw in bad.items():
        assert _raw_host(poses, lo, hi, good, ok_hint, **kw) == (LGS_ERR_INVALID_ARG, True), name
    for name, (a, b) in {"range below 0": ([-1, 4, 7], hi), "range at n": (lo, [3, 6, 10]),
                         "idx_min > idx_max": ([0, 7, 7], hi)}.items():
        assert _raw_host(poses, a, b, good, ok_hint) == (LGS_ERR_INVALID_ARG, True), name
    for v in (inf, -inf, nan):
        for col in (0, 1):
            p = [list(r) for r in poses]
            p[9 if col else 2][col] = v
            assert _raw_host(p, lo, hi, good, ok_hint) == (LGS_ERR_INVALID_ARG, True), ("pose", v, col)
        assert _raw_host(poses, lo, hi, P(v, 2.0, 3, 0), ok_hint) == (LGS_ERR_INVALID_ARG, True), ("travel thr", v)
        assert _raw_host(poses, lo, hi, P(1.0, v, 3, 0), ok_hint) == (LGS_ERR_INVALID_ARG, True), ("node thr", v)
        assert _raw_host(poses, lo, hi, good, [ok_hint[0], H(8, 2, 3, v)]) == (LGS_ERR_INVALID_ARG, True), ("accum", v)
    assert _raw_host(poses, lo, hi, P(1.0, 2.0, -1, 0), ok_hint) == (LGS_ERR_INVALID_ARG, True)
    hints = {"num_maps 0": H(8, 2, 0, 5.0), "num_maps above m": H(8, 2, 4, 5.0),
             "latest map at num_maps": H(5, 2, 2, 5.0), "latest map below 0": H(8, -1, 3, 5.0),
             "node below 0": H(-1, 0, 3, 5.0), "node at n": H(10, 2, 3, 5.0),
             "node before its latest map": H(6, 2, 3, 5.0), "node after its latest map": H(4, 0, 3, 5.0)}
    for name, h in hints.items():
        assert _raw_host(poses, lo, hi, good, [ok_hint[0], h]) == (LGS_ERR_INVALID_ARG, True), name
    # the handle's entry points answer a null handle without a device
    lib = abi.load()
    g = C.c_void_p()
    assert lib.lgs_loop_graph_create(None, None, 1, None, None, 1, C.byref(g)) == LGS_ERR_INVALID_ARG and g.value is None
    assert lib.lgs_loop_graph_info(None, None, None, None, None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_loop_graph_travel(None, None, 0) == LGS_ERR_INVALID_ARG
    assert lib.lgs_loop_search_nearest(None, C.byref(good), None, 0, None, None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_loop_search_stats(None, None) == LGS_ERR_INVALID_ARG
    lib.lgs_loop_graph_destroy(None)
    with pytest.raises(abi.LgsError) as e:
        abi.loop_search_host(poses, lo, hi, good, lc.hint_rows([H(8, 2, 4, 5.0)], abi.LOOP_HINT_DTYPE))
    assert e.value.status == LGS_ERR_INVALID_ARG


def test_candidates_from_search_against_a_hand_built_list():
    """two found records and one not found: queries in record order, candidates query-major in node order"""
    res = np.zeros(3, dtype=abi.LOOP_RESULT_DTYPE)
    res[0] = (1, 1, 5, 8, 10, 7, 0.25)
    res[1] = (0, -1, -1, -1, -1, 0, 4.0)
    res[2] = (1, 0, 2, 9, 9, 7, 0.5)
    scans = [(np.full(4, float(k)), np.arange(4.0)) for k in range(11)]
    poses = [(0.1 * k, -0.2 * k, 0.01 * k) for k in range(11)]
    cells = [np.zeros((3, 3)), np.ones((2, 2))]
    local = [loopbatch.LocalMap(cells[0], -1.0, -2.0, 0.05, (9.0, 9.0, 9.0), -7),
             loopbatch.LocalMap(cells[1], 3.0, 4.0, 0.05, (9.0, 9.0, 9.0), -7)]
    maps, cands = loopbatch.candidates_from_search(res, scans, poses, local)
    assert [(m.cells is c, m.min_x, m.min_y, m.res, m.node_pose, m.node_index) for m, c in zip(maps, (cells[1], cells[0]))] == \
        [(True, 3.0, 4.0, 0.05, poses[5], 5), (True, -1.0, -2.0, 0.05, poses[2], 2)]
    assert [(c.query, c.node_index, c.pose) for c in cands] == \
        [(0, 8, poses[8]), (0, 9, poses[9]), (0, 10, poses[10]), (1, 9, poses[9])]
    assert all(c.ranges is scans[c.node_index][0] and c.angles is scans[c.node_index][1] for c in cands)
    assert loopbatch.sub_queries(cands, 0, 4) == [(0, 0, 3), (1, 3, 1)]
    assert loopbatch.candidates_from_search(res[1:2], scans, poses, local) == ([], [])


def test_host_code_under_the_sanitizers():
    """validation, the walk builder, the group partition and the loop against brute force, compiled with
    -fsanitize=address,undefined into a program of its own (make cpptest)"""
    assert os.path.exists(HOST_CHECK), "build first: make -C <repo> all"
    r = subprocess.run([HOST_CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "LOOP SEARCH HOST CHECKS PASSED" in r.stdout
    for case in ("walk builder == brute force", "every position in exactly one group", "snapshot validation",
                 "hint validation", "writes nothing"):
        assert case in r.stdout, case
