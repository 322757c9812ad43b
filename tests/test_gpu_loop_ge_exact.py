"""GPU tests of the loop detectors with LGS_COST_GREEDY_ENDPOINT_EXACT
(lgs_loop_detect_rtcsm_cost, _multi_cost, _bb_cost, _gs_cost): the 176-byte
records against the oracle's as they stand (loop_oracle.oracle_detect_fn; for
bb and gs the oracle matcher's summary as the same record).  Bar: equality of
all 176 bytes; there is no tolerance.  A kind-2 record differs from the kind-0
detector's in the normalized_cost and covariance bytes only.
"""
import numpy as np
import pytest

import cost_spec_oracle as cso
import ge_exact_oracle as gx
import test_loopbatch_cpu as small
from loop_oracle import oracle_detect_fn
from lgs_amd import abi, loopbatch

pytestmark = pytest.mark.gpu
BB = (4, 1.0, 1.0, 0.6, 20.0, 0.01, 20.0)
GS = (0.6, 0.4, 0.1, 0.05, 0.05, 0.01, 0.01, 20.0)
# detector -> (matcher parameters, parameter type, score threshold, Context method, sharded-path factory)
DETECTORS = {
    "rtcsm": (small.PARAMS, abi.RtcsmParams, small.THR, "loop_detect", loopbatch.hip_detect_fn),
    "bb": (BB, abi.BBParams, 0.6, "loop_detect_bb", loopbatch.hip_detect_fn_bb),
    "gs": (GS, abi.GSParams, 0.5, "loop_detect_gs", loopbatch.hip_detect_fn_gs),
}


def exact():
    return gx.exact_spec(small.COST)


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


def oracle_records(kind, maps, cands, prm, thr):
    if kind == "rtcsm":
        return loopbatch.run_sharded(cands, oracle_detect_fn(maps, cands, prm, small.COST, thr))
    return loopbatch.run_sharded(cands, gx.oracle_ge_detect_fn(kind, maps, cands, prm, thr))


@pytest.mark.parametrize("kind", ["rtcsm", "bb", "gs"])
def test_detector_records_equal_the_oracles(ctx, problem, kind):
    maps, cands, queries, cl = problem
    prm, ptype, thr, method, factory = DETECTORS[kind]
    n = len(cands)
    detect = getattr(ctx, method)
    dev = records(detect(ptype(*prm), exact(), thr, queries, cl), n)
    ora = oracle_records(kind, maps, cands, prm, thr)
    assert dev.shape[1] == 176
    assert dev.tobytes() == ora.tobytes(), sorted(cso.differing_bytes(dev, ora))
    # against kind 0: nothing outside the cost bytes differs
    dev_ge = records(detect(ptype(*prm), ge(), thr, queries, cl), n)
    diff = cso.differing_bytes(dev, dev_ge)
    assert diff <= cso.COST_BYTES, sorted(diff - cso.COST_BYTES)
    dec = loopbatch.decode(dev)
    found = [r.found for r in dec]
    assert 0 < sum(found) < n, found
    assert found == [r.found for r in loopbatch.decode(dev_ge)]
    # candidates that are not found carry a cost and a covariance of their own too
    assert all(r.normalized_cost < 0.0 for r in dec)
    assert len({r.normalized_cost for r in dec}) > n // 2
    # the sharded Python path passes the spec through: world 1, 2 and 3
    fn = factory(ctx, maps, cands, ptype(*prm), exact(), thr)
    # (every rank's block computed here and joined in rank order: what the all-gather returns)
    for world in (1, 2, 3):
        parts = []
        for rank in range(world):
            lo, hi = loopbatch.shard_bounds(n, world, rank)
            parts.append(fn(loopbatch.sub_queries(cands, lo, hi), lo, hi))
        assert np.concatenate(parts, axis=0).tobytes() == dev.tobytes(), world


@pytest.mark.parametrize("n_shards", [2])
def test_multi_context_records_identical(ctx, problem, n_shards):
    """lgs_loop_detect_rtcsm_multi_cost passes the spec to every shard: the
    records over two contexts equal the one-context call's"""
    maps, cands, queries, cl = problem
    p = abi.RtcsmParams(*small.PARAMS)
    n = len(cands)
    one = records(ctx.loop_detect(p, exact(), small.THR, queries, cl), n).tobytes()
    others = [abi.Context(0) for _ in range(n_shards - 1)]
    try:
        multi = records(ctx.loop_detect(p, exact(), small.THR, queries, cl, shards=others), n).tobytes()
    finally:
        for o in others:
            o.close()
    assert multi == one
    assert one == oracle_records("rtcsm", maps, cands, small.PARAMS, small.THR).tobytes()
