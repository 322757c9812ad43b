"""Restatement of LoopSearcherNearest::Search (the reference's
C/mapping/loop_searcher_nearest.cpp:13-108) in pure Python, line for line,
over the flat arrays of DESIGN.md 4.6g: what lgs_loop_search_nearest(_host)
must equal byte for byte.  hypot and pow are the machine's libm's, called
through ctypes (math.hypot and ** are Python's own and need not agree with
them in the last bit); everything else is IEEE double arithmetic, which
Python's float is.  Pinned by tests/golden/loop_search_kat.json."""
import ctypes as C
import ctypes.util
from collections import namedtuple

import numpy as np

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.hypot.argtypes = [C.c_double, C.c_double]
_libm.hypot.restype = C.c_double
_libm.pow.argtypes = [C.c_double, C.c_double]
_libm.pow.restype = C.c_double

Params = namedtuple("Params", "travel_dist_threshold node_dist_threshold num_candidate_nodes")
Hint = namedtuple("Hint", "latest_node_idx latest_local_map_idx num_maps accum_travel_dist")
Record = namedtuple("Record", "found local_map_idx local_map_node_idx node_idx_min node_idx_max walked dist_sq")

RESULT_DTYPE = np.dtype([("found", "<i4"), ("local_map_idx", "<i4"), ("local_map_node_idx", "<i4"),
                         ("node_idx_min", "<i4"), ("node_idx_max", "<i4"), ("walked", "<i4"), ("dist_sq", "<f8")])
MAP_BEST_DTYPE = np.dtype([("node_idx", "<i4"), ("pad_", "<i4"), ("dist_sq", "<f8")])


def hypot(a: float, b: float) -> float:
    return _libm.hypot(float(a), float(b))


def min_sq(prm: Params) -> float:
    """nodeDistMinSq's initial value (:33)"""
    return _libm.pow(float(prm.node_dist_threshold), 2.0)


def travel_chain(poses, idx_min, idx_max):
    """nodeTravelDist after every position of the walk over the maps 0 .. m - 2 (:40-41, :59-60)"""
    out = []
    t = 0.0
    px, py = float(poses[0][0]), float(poses[0][1])
    for i in range(len(idx_min) - 1):
        for k in range(idx_min[i], idx_max[i] + 1):
            x, y = float(poses[k][0]), float(poses[k][1])
            t += hypot(px - x, py - y)
            px, py = x, y
            out.append(t)
    return out


def accum_travel_dist(poses) -> float:
    """GridMapBuilder::UpdateAccumTravelDist (C/mapping/grid_map_builder.cpp:210-224)"""
    t = 0.0
    for i in range(1, len(poses)):
        t += hypot(float(poses[i - 1][0]) - float(poses[i][0]), float(poses[i - 1][1]) - float(poses[i][1]))
    return t


def search(poses, idx_min, idx_max, prm: Params, hint: Hint, travel=None):
    """One hint: (Record, rows) with rows[i] = (node index or -1, dist_sq) per
    map.  travel: None (the loop forms its own chain, as the reference does)
    or travel_chain(...) of the same snapshot, whose entries are that chain's
    values."""
    m = len(idx_min)
    num_of_maps = hint.num_maps
    latest = hint.latest_node_idx
    rx, ry = float(poses[latest][0]), float(poses[latest][1])
    min0 = min_sq(prm)
    node_dist_min_sq = min0
    cand_map, cand_node = -1, -1
    accum = float(hint.accum_travel_dist)
    thr = float(prm.travel_dist_threshold)
    node_travel = 0.0
    px, py = float(poses[0][0]), float(poses[0][1])
    rows = [(-1, min0)] * m
    walked = 0
    done = False
    for map_idx in range(num_of_maps - 1):
        map_min = min0
        for node_idx in range(idx_min[map_idx], idx_max[map_idx] + 1):
            x, y = float(poses[node_idx][0]), float(poses[node_idx][1])
            if travel is None:
                node_travel += hypot(px - x, py - y)
                px, py = x, y
            else:
                node_travel = travel[walked]
            if accum - node_travel < thr:
                done = True
                break
            walked += 1
            d2 = (x - rx) * (x - rx) + (y - ry) * (y - ry)
            if d2 < node_dist_min_sq:
                node_dist_min_sq = d2
                cand_map, cand_node = map_idx, node_idx
            if d2 < map_min:
                map_min = d2
                rows[map_idx] = (node_idx, d2)
        if done:
            break
    if cand_map < 0:
        return Record(0, -1, -1, -1, -1, walked, min0), rows
    lm = hint.latest_local_map_idx
    lo = max(idx_min[lm], latest - prm.num_candidate_nodes)
    hi = min(idx_max[lm], latest + prm.num_candidate_nodes)
    return Record(1, cand_map, cand_node, lo, hi, walked, node_dist_min_sq), rows


def search_all(poses, idx_min, idx_max, prm: Params, hints, own_chain: bool = False):
    """Every hint: (records as RESULT_DTYPE rows, the q x m table as
    MAP_BEST_DTYPE rows), laid out as the library lays them out.  own_chain:
    every hint forms its own travel chain, as the reference does; else the
    snapshot's chain is formed once."""
    poses = [(float(p[0]), float(p[1])) for p in poses]
    idx_min, idx_max = [int(v) for v in idx_min], [int(v) for v in idx_max]
    travel = None if own_chain else travel_chain(poses, idx_min, idx_max)
    res = np.zeros(len(hints), dtype=RESULT_DTYPE)
    tab = np.zeros((len(hints), len(idx_min)), dtype=MAP_BEST_DTYPE)
    for j, h in enumerate(hints):
        rec, rows = search(poses, idx_min, idx_max, prm, h, travel)
        res[j] = tuple(rec)
        for i, (node, d2) in enumerate(rows):
            tab[j, i] = (node, 0, d2)
    return res, tab
