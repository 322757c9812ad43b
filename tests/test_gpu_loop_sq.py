"""GPU tests of the loop detectors whose matcher was constructed with
CostSquareError (lgs_loop_detect_rtcsm_cost, _multi_cost, _bb_cost, _gs_cost):
the 176-byte records against the oracle's (cost_spec_oracle.oracle_sq_detect_fn:
the oracle matcher's record with CostSquareError's cost and covariance at its
best sensor pose).  Bar: equality of bytes; there is no tolerance.  A
square-error record differs from the greedy-endpoint detector's in the
normalized_cost and covariance bytes only.
"""
import numpy as np
import pytest

import cost_spec_oracle as cso
import test_loopbatch_cpu as small
from hc_sq_oracle import SQ_RANGE
from lgs_amd import abi, loopbatch, scene
from test_gpu_rtcsm import build_map

pytestmark = pytest.mark.gpu
BB = (4, 1.0, 1.0, 0.6, 20.0, 0.01, 20.0)
GS = (0.6, 0.4, 0.1, 0.05, 0.05, 0.01, 0.01, 20.0)
# detector -> (matcher parameters, parameter type, score threshold, Context method, sharded-path factory)
DETECTORS = {
    "rtcsm": (small.PARAMS, abi.RtcsmParams, small.THR, "loop_detect", loopbatch.hip_detect_fn),
    "bb": (BB, abi.BBParams, 0.6, "loop_detect_bb", loopbatch.hip_detect_fn_bb),
    "gs": (GS, abi.GSParams, 0.5, "loop_detect_gs", loopbatch.hip_detect_fn_gs),
}


def sq():
    return abi.CostSQParams(*SQ_RANGE)


def ge():
    return abi.CostGEParams(*small.COST)


@pytest.fixture(scope="module")
def problem(ctx):
    maps, cands = small.make_problem()
    grids = [ctx.grid_from_array(m.cells, m.min_x, m.min_y, m.res) for m in maps]
    scans = [ctx.scan(c.ranges, c.angles) for c in cands]
    queries, first = [], 0
    for qi, m in enumerate(maps):
        n = sum(1 for c in cands if c.query == qi)
        queries.append((grids[qi], None, m.node_pose, m.node_index, first, n))
        first += n
    cl = [(s, c.pose, c.node_index) for s, c in zip(scans, cands)]
    return maps, cands, queries, cl


def records(out, n):
    return np.frombuffer(bytes(out), dtype=np.uint8)[: n * loopbatch.RECORD_BYTES].reshape(n, loopbatch.RECORD_BYTES)


@pytest.mark.parametrize("kind", ["rtcsm", "bb", "gs"])
def test_detector_records_equal_the_oracles(ctx, problem, kind):
    maps, cands, queries, cl = problem
    prm, ptype, thr, method, factory = DETECTORS[kind]
    n = len(cands)
    detect = getattr(ctx, method)
    dev = records(detect(ptype(*prm), sq(), thr, queries, cl), n)
    ora = loopbatch.run_sharded(cands, cso.oracle_sq_detect_fn(kind, maps, cands, prm, thr))
    assert dev.tobytes() == ora.tobytes(), sorted(cso.differing_bytes(dev, ora))
    # against the greedy-endpoint detector: the cost bytes differ, nothing else
    dev_ge = records(detect(ptype(*prm), ge(), thr, queries, cl), n)
    diff = cso.differing_bytes(dev, dev_ge)
    assert diff and diff <= cso.COST_BYTES, sorted(diff - cso.COST_BYTES)
    dec, dec_ge = loopbatch.decode(dev), loopbatch.decode(dev_ge)
    found = [r.found for r in dec]
    assert 0 < sum(found) < n, found
    assert found == [r.found for r in dec_ge]
    # candidates that are not found carry the square-error cost and covariance too
    for a, b in zip(dec, dec_ge):
        assert a.normalized_cost != b.normalized_cost and list(a.covariance) != list(b.covariance)
        assert 0.0 < a.normalized_cost <= 1.0
    # the sharded Python path passes the cost through, and the records survive the all-gather
    fn = factory(ctx, maps, cands, ptype(*prm), sq(), thr)
    sharded = loopbatch.run_sharded(cands, fn, rank=0, world=1)
    assert sharded.tobytes() == dev.tobytes()
    if kind == "rtcsm":
        gather = loopbatch.RcclGather(ctx, 0, 1)
        try:
            assert loopbatch.run_sharded_rccl(cands, fn, gather).tobytes() == dev.tobytes()
        finally:
            gather.close()


@pytest.mark.parametrize("kind", ["bb", "gs"])
def test_two_queries_over_maps_of_different_size(ctx, world, kind):
    prm, ptype, thr, method, _ = DETECTORS[kind]
    shapes = ((300, 4), (400, 6))
    built = [build_map(world, n, 0.05, 100, scene.arc_poses(k), n_beams=541) for n, k in shapes]
    ang = scene.beam_angles(181)
    rng = np.random.default_rng(21)
    maps, cands, queries, cl = [], [], [], []
    for q, (c, mx, my) in enumerate(built):
        node_pose = (0.1 * q, -0.05, 0.02 * q)
        maps.append(loopbatch.LocalMap(c, mx, my, 0.05, node_pose, q))
        queries.append((ctx.grid_from_array(c, mx, my, 0.05), None, node_pose, q, len(cl), 2))
        for k in range(2):
            true = (rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), rng.uniform(-3, 3))
            r = scene.ray_cast(world, true, ang)
            far = k == 1   # the second node of a query starts outside the window's reach
            init = (true[0] + (0.9 if far else rng.uniform(-0.15, 0.15)),
                    true[1] + (-0.9 if far else rng.uniform(-0.15, 0.15)), true[2] + (0.4 if far else 0.03))
            cands.append(loopbatch.Candidate(q, r, ang, init, 100 * q + k))
            cl.append((ctx.scan(r, ang), init, 100 * q + k))
    dev = records(getattr(ctx, method)(ptype(*prm), sq(), thr, queries, cl), len(cl))
    ora = loopbatch.run_sharded(cands, cso.oracle_sq_detect_fn(kind, maps, cands, prm, thr))
    assert dev.tobytes() == ora.tobytes(), sorted(cso.differing_bytes(dev, ora))
    assert len({r.normalized_cost for r in loopbatch.decode(dev)}) == len(cl)


@pytest.mark.parametrize("n_shards", [2, 3])
def test_multi_context_records_identical(ctx, problem, n_shards):
    """lgs_loop_detect_rtcsm_multi_cost passes the cost to every shard: the records
    of 2 and 3 contexts equal the one-context call's over both copy paths"""
    maps, cands, queries, cl = problem
    p = abi.RtcsmParams(*small.PARAMS)
    n = len(cands)
    one = records(ctx.loop_detect(p, sq(), small.THR, queries, cl), n).tobytes()
    others = [abi.Context(0) for _ in range(n_shards - 1)]
    try:
        multi = records(ctx.loop_detect(p, sq(), small.THR, queries, cl, shards=others), n).tobytes()
        for o in others:
            o.set_option(abi.LGS_OPT_PEER_COPY, 1)
        staged = records(ctx.loop_detect(p, sq(), small.THR, queries, cl, shards=others), n).tobytes()
        counters = [o.copy_counters() for o in others]
    finally:
        for o in others:
            o.close()
    assert multi == one and staged == one
    assert all(c["direct"] > 0 and c["staged"] > 0 for c in counters), counters
