"""Loop-closure candidate batch sharded over GPUs.

LoopDetectorRealTimeCorrelative::Detect (C/mapping/loop_detector_real_time_correlative.cpp:26-92)
matches every candidate node of every query against the query's local map;
candidates are independent (:38, :66), so with one process per GPU:

  * rank r takes the contiguous block [start_r, start_r + count_r) of the
    candidate list (query-major, node order inside a query: the reference's
    iteration order);
  * it uploads only the local maps its block references and computes their
    coarse maps once (:52-60), then runs lgs_loop_detect_rtcsm on its block
    -- no collective on the data path;
  * one all_gather of fixed 176-byte result records (uint8 rows, padded to the
    largest block) restores the full, ordered list on every rank; results with
    found == 0 are dropped WITHOUT reordering, because the order of loop edges
    feeds the pose-graph optimizer (C/mapping/lidar_graph_slam.cpp:252-282).

`detect_fn(sub_queries, cand_lo, cand_hi) -> np.uint8 [count, 176]` does the
per-rank matching; `hip_detect_fn` is the product implementation (C-ABI);
tests inject an oracle-based one to exercise the sharding on CPU (gloo).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import abi

RECORD_BYTES = C.sizeof(abi.LoopResult)   # 176


@dataclass
class LocalMap:
    """LoopDetectionQuery::mLocalMapInfo (dense cells) + mLocalMapNode."""
    cells: np.ndarray          # (H, W) fp64, 0.0 = unknown
    min_x: float
    min_y: float
    res: float
    node_pose: Tuple[float, float, float]
    node_index: int


@dataclass
class Candidate:
    """One poseGraphNode of a query: scan + pose (initial guess) + index."""
    query: int
    ranges: np.ndarray
    angles: np.ndarray
    pose: Tuple[float, float, float]
    node_index: int


def candidates_from_search(records, scans, poses, local_maps: Sequence[LocalMap]
                           ) -> Tuple[List[LocalMap], List[Candidate]]:
    """LidarGraphSlam::GetLoopDetectionQueries (C/mapping/lidar_graph_slam.cpp:155-188)
    over the loop searcher's records (abi.LOOP_RESULT_DTYPE rows, from
    LoopGraph.search or abi.loop_search_host): every found record becomes one
    query, in record order -- the local map records[j].local_map_idx with the
    node local_map_node_idx as its node -- and its nodes node_idx_min ..
    node_idx_max become that query's candidates, in node order.
    scans[k] = (ranges, angles) and poses[k] = (x, y, theta) of node k;
    local_maps[i] = map i (its node fields are not read; the cells are shared,
    not copied).  Returns (maps, candidates): candidates[*].query indexes maps,
    query-major, as hip_detect_fn* and run_sharded take them."""
    maps: List[LocalMap] = []
    cands: List[Candidate] = []
    for r in records:
        if not r["found"]:
            continue
        lm, node = local_maps[int(r["local_map_idx"])], int(r["local_map_node_idx"])
        maps.append(LocalMap(lm.cells, lm.min_x, lm.min_y, lm.res, tuple(float(v) for v in poses[node]), node))
        for k in range(int(r["node_idx_min"]), int(r["node_idx_max"]) + 1):
            cands.append(Candidate(len(maps) - 1, scans[k][0], scans[k][1], tuple(float(v) for v in poses[k]), k))
    return maps, cands


def shard_bounds(n: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous block of rank r: sizes differ by at most one."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def sub_queries(cands: Sequence[Candidate], lo: int, hi: int) -> List[Tuple[int, int, int]]:
    """[(query index, first local candidate, count)] covering [lo, hi) in order.
    Candidates must be query-major (all of query q before q+1)."""
    out: List[Tuple[int, int, int]] = []
    for i in range(lo, hi):
        q = cands[i].query
        if out and out[-1][0] == q:
            out[-1] = (q, out[-1][1], out[-1][2] + 1)
        else:
            out.append((q, i - lo, 1))
    return out


def hip_detect_fn(ctx: "abi.Context", maps: Sequence[LocalMap], cands: Sequence[Candidate],
                  params: "abi.RtcsmParams", cost, threshold: float
                  ) -> Callable[[List[Tuple[int, int, int]], int, int], np.ndarray]:
    """Per-rank matcher on the GPU: uploads the maps its block needs once.
    cost: the detector's matcher's cost function, a CostGEParams, a CostSQParams
    (the records' normalized_cost and covariance are then CostSquareError's) or a
    CostSpec such as abi.cost_spec(ge, exact=True) (the greedy-endpoint values
    bit for bit); the same holds for hip_detect_fn_bb and hip_detect_fn_gs."""
    grids = {}
    scans = {}

    def fn(subq, lo, hi):
        queries, cl = [], []
        for q, first, count in subq:
            if q not in grids:
                m = maps[q]
                g = ctx.grid_from_array(m.cells, m.min_x, m.min_y, m.res)
                grids[q] = (g, ctx.precompute_max(g, params.low_resolution))
            g, coarse = grids[q]
            queries.append((g, coarse, maps[q].node_pose, maps[q].node_index, first, count))
        for i in range(lo, hi):
            c = cands[i]
            if i not in scans:
                scans[i] = ctx.scan(c.ranges, c.angles)
            cl.append((scans[i], c.pose, c.node_index))
        out = ctx.loop_detect(params, cost, threshold, queries, cl)
        return np.frombuffer(bytes(out), dtype=np.uint8)[: (hi - lo) * RECORD_BYTES].reshape(hi - lo, RECORD_BYTES)

    return fn


def hip_detect_fn_bb(ctx: "abi.Context", maps: Sequence[LocalMap], cands: Sequence[Candidate],
                     params: "abi.BBParams", cost, threshold: float
                     ) -> Callable[[List[Tuple[int, int, int]], int, int], np.ndarray]:
    """As hip_detect_fn with LoopDetectorBranchBound (C/mapping/loop_detector_branch_bound.cpp:26-117):
    lgs_loop_detect_bb builds each query's map pyramid itself."""
    grids = {}
    scans = {}

    def fn(subq, lo, hi):
        queries, cl = [], []
        for q, first, count in subq:
            if q not in grids:
                m = maps[q]
                grids[q] = ctx.grid_from_array(m.cells, m.min_x, m.min_y, m.res)
            queries.append((grids[q], None, maps[q].node_pose, maps[q].node_index, first, count))
        for i in range(lo, hi):
            c = cands[i]
            if i not in scans:
                scans[i] = ctx.scan(c.ranges, c.angles)
            cl.append((scans[i], c.pose, c.node_index))
        out = ctx.loop_detect_bb(params, cost, threshold, queries, cl)
        return np.frombuffer(bytes(out), dtype=np.uint8)[: (hi - lo) * RECORD_BYTES].reshape(hi - lo, RECORD_BYTES)

    return fn


def hip_detect_fn_gs(ctx: "abi.Context", maps: Sequence[LocalMap], cands: Sequence[Candidate],
                     params: "abi.GSParams", cost, threshold: float
                     ) -> Callable[[List[Tuple[int, int, int]], int, int], np.ndarray]:
    """As hip_detect_fn with LoopDetectorGridSearch (C/mapping/loop_detector_grid_search.cpp:26-106):
    lgs_loop_detect_gs needs nothing precomputed per map."""
    grids = {}
    scans = {}

    def fn(subq, lo, hi):
        queries, cl = [], []
        for q, first, count in subq:
            if q not in grids:
                m = maps[q]
                grids[q] = ctx.grid_from_array(m.cells, m.min_x, m.min_y, m.res)
            queries.append((grids[q], None, maps[q].node_pose, maps[q].node_index, first, count))
        for i in range(lo, hi):
            c = cands[i]
            if i not in scans:
                scans[i] = ctx.scan(c.ranges, c.angles)
            cl.append((scans[i], c.pose, c.node_index))
        out = ctx.loop_detect_gs(params, cost, threshold, queries, cl)
        return np.frombuffer(bytes(out), dtype=np.uint8)[: (hi - lo) * RECORD_BYTES].reshape(hi - lo, RECORD_BYTES)

    return fn


def hip_detect_fn_icp(ctx: "abi.Context", ref_set, maps: Sequence[LocalMap], cands: Sequence[Candidate],
                      prm: "abi.IcpParams", window: "abi.IcpWindow", gate: "abi.LoopRefineGate",
                      ref_of_query: Optional[Sequence[int]] = None
                      ) -> Callable[[List[Tuple[int, int, int]], int, int], np.ndarray]:
    """As hip_detect_fn with the ICP loop detector (lgs_loop_detect_icp, DESIGN.md
    4.5e): no grid at all.  ref_set[i] is an abi.IcpRef (an abi.IcpRefSet, or a
    list); query q uses ref_set[ref_of_query[q]], by default ref_set[q].  Of maps
    only node_pose and node_index are read.  fn.best and fn.summaries keep the
    last call's best lattice indices and IcpSummary list."""
    ref_of_query = list(range(len(maps))) if ref_of_query is None else list(ref_of_query)
    scans = {}

    def fn(subq, lo, hi):
        queries = [(None, None, maps[q].node_pose, maps[q].node_index, first, count) for q, first, count in subq]
        refs = [ref_set[ref_of_query[q]] for q, _, _ in subq]
        cl = []
        for i in range(lo, hi):
            c = cands[i]
            if i not in scans:
                scans[i] = ctx.scan(c.ranges, c.angles)
            cl.append((scans[i], c.pose, c.node_index))
        out, fn.best, fn.summaries = ctx.loop_detect_icp(refs, queries, cl, prm, window, gate)
        return np.frombuffer(bytes(out), dtype=np.uint8)[: (hi - lo) * RECORD_BYTES].reshape(hi - lo, RECORD_BYTES)

    fn.best, fn.summaries = [], []
    return fn


def run_sharded(cands: Sequence[Candidate], detect_fn, rank: int = 0, world: int = 1, dist=None,
                device=None) -> np.ndarray:
    """All candidates' records (uint8 [n, 176]) in candidate order, on every rank."""
    n = len(cands)
    lo, hi = shard_bounds(n, world, rank)
    local = detect_fn(sub_queries(cands, lo, hi), lo, hi) if hi > lo else np.zeros((0, RECORD_BYTES), np.uint8)
    assert local.shape == (hi - lo, RECORD_BYTES)
    if world == 1:
        return local
    import torch
    rows = shard_bounds(n, world, 0)[1]        # largest block
    buf = torch.zeros((rows, RECORD_BYTES), dtype=torch.uint8)
    buf[: hi - lo] = torch.from_numpy(local.copy())
    if device is not None and str(device).startswith("cuda"):
        # RCCL: one all-gather into one device tensor, one copy back
        out = torch.empty((world * rows, RECORD_BYTES), dtype=torch.uint8, device=device)
        dist.all_gather_into_tensor(out, buf.to(device))
        allrows = out.cpu().numpy().reshape(world, rows, RECORD_BYTES)
    else:
        if device is not None:
            buf = buf.to(device)
        gathered = [torch.empty_like(buf) for _ in range(world)]
        dist.all_gather(gathered, buf)
        allrows = np.stack([g.cpu().numpy() for g in gathered])
    parts = []
    for r in range(world):
        a, b = shard_bounds(n, world, r)
        parts.append(allrows[r, : b - a])
    return np.concatenate(parts, axis=0)


class RcclGather:
    """The all-gather of the records through the library's C-ABI
    (lgs_loop_records_allgather: one ncclAllGather of fixed-size rows on the
    context's stream, RCCL over xGMI) instead of torch: one communicator per
    rank, its unique id made on rank 0 and broadcast over `dist` once."""

    def __init__(self, ctx: "abi.Context", rank: int, world: int, dist=None):
        self.ctx, self.rank, self.world = ctx, rank, world
        uid = None
        if rank == 0:
            buf = (C.c_ubyte * 128)()
            ctx.check(ctx.lib.lgs_rccl_unique_id(buf), "rccl_unique_id")
            uid = bytes(buf)
        if world > 1:
            box = [uid]
            dist.broadcast_object_list(box, src=0)
            uid = box[0]
        self.comm = ctx.rccl_comm(world, rank, uid)

    def __call__(self, n: int, lo: int, hi: int, local: np.ndarray) -> np.ndarray:
        loc = (abi.LoopResult * max(1, hi - lo)).from_buffer_copy(
            local.tobytes() if hi > lo else bytes(RECORD_BYTES))
        out = (abi.LoopResult * max(1, n))()
        self.ctx.check(self.ctx.lib.lgs_loop_records_allgather(self.ctx.h, self.comm, self.rank, self.world, n,
                                                               loc, out), "loop_records_allgather")
        return np.frombuffer(bytes(out), dtype=np.uint8)[: n * RECORD_BYTES].reshape(n, RECORD_BYTES)

    def close(self):
        if self.comm:
            self.ctx.rccl_comm_destroy(self.comm)
            self.comm = None


def run_sharded_rccl(cands: Sequence[Candidate], detect_fn, gather: RcclGather) -> np.ndarray:
    """run_sharded with the records gathered by the C-ABI collective."""
    n = len(cands)
    lo, hi = shard_bounds(n, gather.world, gather.rank)
    local = detect_fn(sub_queries(cands, lo, hi), lo, hi) if hi > lo else np.zeros((0, RECORD_BYTES), np.uint8)
    assert local.shape == (hi - lo, RECORD_BYTES)
    return gather(n, lo, hi, local)


def refine_icp(ctx: "abi.Context", ref_set, maps: Sequence[LocalMap], cands: Sequence[Candidate],
               records: np.ndarray, prm: "abi.IcpParams", gate: "abi.LoopRefineGate",
               ref_of_query: Optional[Sequence[int]] = None):
    """lgs_loop_refine_icp over the record array run_sharded returns (uint8
    [n, 176], candidate order): every found record is refined by ICP from its
    estimate against its query's reference and, where the gate accepts it,
    gets the ICP's estimate, loop edge, covariance and cost.
    ref_set[i] is an abi.IcpRef (an abi.IcpRefSet, or a list); query q uses
    ref_set[ref_of_query[q]], by default ref_set[q].  Of maps only node_pose
    and node_index are read.  Returns (records, refined, summaries): a new
    uint8 [n, 176] array, an int array [n] and the candidates' IcpSummary list."""
    n = len(cands)
    assert records.shape == (n, RECORD_BYTES)
    ref_of_query = list(range(len(maps))) if ref_of_query is None else list(ref_of_query)
    scans = [ctx.scan(c.ranges, c.angles) for c in cands]
    queries = [(None, None, maps[q].node_pose, maps[q].node_index, first, count)
               for q, first, count in sub_queries(cands, 0, n)]
    refs = [ref_set[ref_of_query[q]] for q, _, _ in sub_queries(cands, 0, n)]
    cl = [(scans[i], c.pose, c.node_index) for i, c in enumerate(cands)]
    out = (abi.LoopResult * max(1, n)).from_buffer_copy(records.tobytes() if n else bytes(RECORD_BYTES))
    refined, sums = ctx.loop_refine_icp(refs, queries, cl, prm, gate, out)
    for s in scans:
        s.close()
    new = np.frombuffer(bytes(out), dtype=np.uint8)[: n * RECORD_BYTES].reshape(n, RECORD_BYTES).copy()
    return new, np.array(refined, dtype=np.int32), sums


def decode(records: np.ndarray) -> List[abi.LoopResult]:
    raw = records.tobytes()
    return [abi.LoopResult.from_buffer_copy(raw[i * RECORD_BYTES:(i + 1) * RECORD_BYTES])
            for i in range(records.shape[0])]


def loop_results(records: np.ndarray) -> List[abi.LoopResult]:
    """LoopDetectionResultVector: found records, order preserved (:77-88)."""
    return [r for r in decode(records) if r.found]
