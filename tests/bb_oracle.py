"""Oracle-side helpers of the branch-and-bound matcher's tests.

oracle_bb        the oracle's ScanMatcherBranchBound::OptimizePose
                 (orc_bb_optimize_pose / _query) with the scan's relative pose
                 and range limits exposed
assert_bb_same   the parity bar of the BB tests (bit-exact search, 1e-5 cost)
exact_search     the reference's LIFO search (:81-140) in Python over
                 orc_pixel_accurate_score: visited count, best node, and the
                 set of nodes it expands
superset_model   what csrc/k_bb.hip's header says the device scores: level by
                 level, every node scored above thr_exp (or on a valid first
                 descent) expanded into its four children

TEST INFRASTRUCTURE ONLY (like oracle_bind.py).
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np

import oracle_bind as ob
from conftest import launcher_cost

DBL_MIN = 2.2250738585072014e-308
TOL = 1e-5


def oracle_bb(cells, mx, my, res, prm, ranges, angles, init, thr=None, rel=(0, 0, 0), smin=0.0, smax=30.0):
    g = ob.OGrid(cells, mx, my, res)
    sc = ob.OScan(ranges, angles, rel, smin, smax)
    P = ob.BBParams(*prm)
    out = ob.Summary()
    cost = launcher_cost(oracle=True)
    if thr is None:
        ob.lib().orc_bb_optimize_pose_query(C.byref(g.g), C.byref(P), C.byref(cost), C.byref(sc.s), ob.Pose(*init),
                                            C.byref(out))
    else:
        keep = [ob.OGrid(m, mx, my, res) for m in ob.precompute_pyramid(cells, prm[0])]
        maps = (ob.Grid * len(keep))(*[k.g for k in keep])
        ob.lib().orc_bb_optimize_pose(C.byref(g.g), maps, C.byref(P), C.byref(cost), C.byref(sc.s), ob.Pose(*init),
                                      thr, C.byref(out))
    return out


def assert_bb_same(gpu, ora, tag=""):
    assert gpu.pose_found == ora.pose_found, tag
    assert list(gpu.win) == list(ora.win), tag
    assert list(gpu.steps) == list(ora.steps), tag
    assert list(gpu.best_win) == list(ora.best_win), (tag, list(gpu.best_win), list(ora.best_win))
    assert gpu.score_max == ora.score_max, (tag, gpu.score_max, ora.score_max)
    assert gpu.score_threshold == ora.score_threshold, tag
    assert gpu.fine_blocks == ora.coarse_evals, (tag, gpu.fine_blocks, ora.coarse_evals)   # nodes visited
    assert gpu.coarse_blocks >= gpu.fine_blocks
    assert gpu.estimated_pose.tuple() == (ora.estimated_pose.x, ora.estimated_pose.y, ora.estimated_pose.theta)
    assert abs(gpu.normalized_cost - ora.normalized_cost) <= TOL, tag
    assert np.allclose(list(gpu.covariance), list(ora.covariance), rtol=0, atol=TOL), tag


class _Plan:
    """One match's geometry (:54-88) and its node scores, memoised.
    score_maps: the pyramid levels the scores are read from (default: the
    map's own PrecomputeGridMaps pyramid)."""

    def __init__(self, cells, mx, my, res, prm, ranges, angles, init, thr, rel, smin, smax, score_maps):
        L = ob.lib()
        self.L = L
        self.P = ob.BBParams(*prm)
        self.sc = ob.OScan(ranges, angles, rel, smin, smax)
        self.hm = int(prm[0])
        maps = score_maps if score_maps is not None else ob.precompute_pyramid(cells, self.hm)
        assert len(maps) == self.hm + 1
        self.grids = [ob.OGrid(m, mx, my, res) for m in maps]
        self.sp = L.orc_compound(ob.Pose(*init), ob.Pose(*rel))
        sx, sy, st = C.c_double(), C.c_double(), C.c_double()
        L.orc_rtcsm_search_step(res, C.byref(self.sc.s), prm[4], C.byref(sx), C.byref(sy), C.byref(st))
        self.steps = (sx.value, sy.value, st.value)
        self.win = tuple(int(math.ceil(0.5 * r / s)) for r, s in zip(prm[1:4], self.steps))
        self.thr0 = (DBL_MIN if thr is None else thr) * len(self.sc.r)
        ws = 1 << self.hm
        self.top_x = list(range(-self.win[0], self.win[0] + 1, ws))
        self.top_y = list(range(-self.win[1], self.win[1] + 1, ws))
        self.T = 2 * self.win[2] + 1
        self.memo = {}

    def top_nodes(self):
        """the reference's push order (:81-88): x outer, y, theta inner"""
        return [(x, y, t, self.hm) for x in self.top_x for y in self.top_y
                for t in range(-self.win[2], self.win[2] + 1)]

    def score(self, node):
        s = self.memo.get(node)
        if s is None:
            x, y, t, h = node
            pose = ob.Pose(self.sp.x + x * self.steps[0], self.sp.y + y * self.steps[1],
                           self.sp.theta + t * self.steps[2])
            s = self.L.orc_pixel_accurate_score(C.byref(self.grids[h].g), C.byref(self.P), C.byref(self.sc.s), pose)
            self.memo[node] = s
        return s


def children(node):
    """:123-135, in push order"""
    x, y, t, h = node
    ws = 1 << (h - 1)
    return [(x, y, t, h - 1), (x + ws, y, t, h - 1), (x, y + ws, t, h - 1), (x + ws, y + ws, t, h - 1)]


def exact_search(cells, mx, my, res, prm, ranges, angles, init, thr=None, rel=(0, 0, 0), smin=0.0, smax=30.0,
                 score_maps=None):
    """The reference's LIFO loop (:92-140).  Returns visited (nodes scored),
    best (x, y, t), score_max, found, and expanded, the set of (x, y, t, h)
    nodes whose children the search pushed."""
    pl = _Plan(cells, mx, my, res, prm, ranges, angles, init, thr, rel, smin, smax, score_maps)
    stack = pl.top_nodes()
    smax_, best, visited, expanded = pl.thr0, (0, 0, 0), 0, set()
    while stack:
        node = stack.pop()
        s = pl.score(node)
        visited += 1
        if s <= smax_:
            continue
        if node[3] == 0:
            smax_, best = s, node[:3]
            continue
        expanded.add(node)
        stack += children(node)
    return SimpleNamespace(visited=visited, best=best, score_max=smax_, found=int(smax_ > pl.thr0),
                           expanded=expanded, win=pl.win, T=pl.T, n_top=len(pl.top_x) * len(pl.top_y) * pl.T)


def _levels(pl, rule):
    """Level by level from the top nodes: the nodes `rule` expands and the
    number of nodes scored (top nodes + 4 per expansion)."""
    cur = pl.top_nodes()
    count, expanded = len(cur), set()
    for h in range(pl.hm, 0, -1):
        nxt = []
        for node in cur:
            if rule(node):
                expanded.add(node)
                nxt += children(node)
        count += len(nxt)
        cur = nxt
    return count, expanded


def superset_model(cells, mx, my, res, prm, ranges, angles, init, thr=None, rel=(0, 0, 0), smin=0.0, smax=30.0,
                   score_maps=None):
    """The device's scored set (k_bb.hip's header).  The first descent is the
    last-pushed top node and then always the last-pushed child; when its whole
    path scores above thr0, thr_exp = max(thr0, s(L1)) and the path nodes are
    expanded whatever they score, else thr_exp = thr0.  Returns count (nodes
    scored under that rule), count_thr0 (under the plain thr0 rule: the
    rerun's superset), path_ok, thr_exp, expanded, expanded_thr0, T, n_top."""
    pl = _Plan(cells, mx, my, res, prm, ranges, angles, init, thr, rel, smin, smax, score_maps)
    hm = pl.hm
    px, py, pt = pl.top_x[-1], pl.top_y[-1], pl.win[2]
    path = [(px + (1 << hm) - (1 << h), py + (1 << hm) - (1 << h), pt, h) for h in range(hm, -1, -1)]
    path_ok = all(pl.score(nd) > pl.thr0 for nd in path)
    thr_exp = max(pl.thr0, pl.score(path[-1])) if path_ok else pl.thr0
    on_path = set(path) if path_ok else set()
    count, expanded = _levels(pl, lambda nd: pl.score(nd) > thr_exp or nd in on_path)
    count_thr0, expanded_thr0 = _levels(pl, lambda nd: pl.score(nd) > pl.thr0)
    return SimpleNamespace(count=count, count_thr0=count_thr0, path_ok=path_ok, thr_exp=thr_exp, thr0=pl.thr0,
                           expanded=expanded, expanded_thr0=expanded_thr0, path=path, top=pl.top_nodes(), win=pl.win,
                           T=pl.T,
                           n_top=len(pl.top_x) * len(pl.top_y) * pl.T)
