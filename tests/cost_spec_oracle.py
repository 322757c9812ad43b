"""Oracle-side helpers for the `_cost` entry points (test infrastructure only).

What a search matcher constructed with CostSquareError returns, composed over
the oracle: the oracle matcher's own summary (orc_rtcsm_optimize_pose*, the
composed references of bb_oracle.py and test_gpu_gs.py) with the normalized
cost and the covariance replaced by orc_sq_cost / orc_sq_covariance at that
matcher's best sensor pose, found or not, as the reference evaluates them
(scan_matcher_real_time_correlative.cpp:128-138, scan_matcher_grid_search.cpp:97-107).
The same for the 176-byte loop records of tests/loop_oracle.py.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import oracle_bind as ob
from conftest import launcher_cost
from hc_sq_oracle import SQ_RANGE, sq_covariance, sq_cost
from lgs_amd import abi
from lgs_amd.loopbatch import RECORD_BYTES

DBL_MIN = 2.2250738585072014e-308
COST_OFF = abi.LoopResult.normalized_cost.offset
COV_OFF = abi.LoopResult.covariance.offset
COST_BYTES = set(range(COST_OFF, COST_OFF + 8)) | set(range(COV_OFF, COV_OFF + 72))


def sq_params():
    return abi.CostSQParams(*SQ_RANGE)


def sq_at(g, sc, pose, usable=SQ_RANGE):
    """(Cost / NumOfScans(), covariance) of CostSquareError(*usable) at `pose`"""
    return sq_cost(g, sc, pose, usable) / len(sc.r), sq_covariance(g, sc, pose, usable)


def pose3(p):
    return (p.x, p.y, p.theta)


def ref_rtcsm(map3, res, params, r, ang, init, thr=None, rel=(0.0, 0.0, 0.0), usable=SQ_RANGE):
    """the oracle's correlative summary plus .sq_cost / .sq_cov at its best sensor pose"""
    cells, mx, my = map3
    g, sc = ob.OGrid(cells, mx, my, res), ob.OScan(r, ang, rel, 0.0, 30.0)
    out = ob.Summary()
    cost = launcher_cost(oracle=True)
    if thr is None:
        ob.lib().orc_rtcsm_optimize_pose_query(C.byref(g.g), C.byref(ob.RtcsmParams(*params)), C.byref(cost),
                                               C.byref(sc.s), ob.Pose(*init), C.byref(out))
    else:
        cg = ob.OGrid(ob.precompute(cells, params[0]), mx, my, res)
        ob.lib().orc_rtcsm_optimize_pose(C.byref(g.g), C.byref(cg.g), C.byref(ob.RtcsmParams(*params)), C.byref(cost),
                                         C.byref(sc.s), ob.Pose(*init), thr, C.byref(out))
    c, cov = sq_at(g, sc, pose3(out.best_sensor_pose), usable)
    return SimpleNamespace(s=out, sq_cost=c, sq_cov=cov, best=pose3(out.best_sensor_pose))


def ref_bb(map3, res, prm, r, ang, init, thr=None, rel=(0.0, 0.0, 0.0)):
    from bb_oracle import oracle_bb
    cells, mx, my = map3
    out = oracle_bb(cells, mx, my, res, prm, r, ang, init, thr=thr, rel=rel)
    g, sc = ob.OGrid(cells, mx, my, res), ob.OScan(r, ang, rel, 0.0, 30.0)
    c, cov = sq_at(g, sc, pose3(out.best_sensor_pose))
    return SimpleNamespace(s=out, sq_cost=c, sq_cov=cov, best=pose3(out.best_sensor_pose))


def ref_gs(map3, res, prm, r, ang, init, nthr=DBL_MIN, rel=(0.0, 0.0, 0.0)):
    """compose_gs (tests/test_gpu_gs.py) and the best sensor pose it keeps (:71, :78-80)"""
    from test_gpu_gs import compose_gs, literal_steps
    cells, mx, my = map3
    ref = compose_gs(cells, mx, my, res, prm, r, ang, init, nthr=nthr, rel=rel)
    sp = ob.lib().orc_compound(ob.Pose(*init), ob.Pose(*rel))
    best = (sp.x, sp.y, sp.theta)
    if ref.pose_found:
        xs, ys, ts = literal_steps(prm[0], prm[3]), literal_steps(prm[1], prm[4]), literal_steps(prm[2], prm[5])
        ix, iy, it = ref.best_win
        best = (sp.x + xs[ix], sp.y + ys[iy], sp.theta + ts[it])
    g, sc = ob.OGrid(cells, mx, my, res), ob.OScan(r, ang, rel, 0.0, 30.0)
    c, cov = sq_at(g, sc, best)
    return SimpleNamespace(s=ref, sq_cost=c, sq_cov=cov, best=best)


def assert_sq(summary, ref, tag=""):
    """the summary's cost fields are the oracle's square-error values, bit for bit"""
    assert summary.best_sensor_pose.tuple() == ref.best, (tag, summary.best_sensor_pose.tuple(), ref.best)
    assert summary.normalized_cost == ref.sq_cost, (tag, summary.normalized_cost, ref.sq_cost)
    assert np.array(list(summary.covariance)).tobytes() == np.array(ref.sq_cov).tobytes(), \
        (tag, list(summary.covariance), ref.sq_cov)


def same_but_counters(a, b):
    """two RtcsmSummary equal in every byte except guard_hits and fixups"""
    x = abi.RtcsmSummary.from_buffer_copy(bytes(a))
    x.guard_hits, x.fixups = b.guard_hits, b.fixups
    return bytes(x) == bytes(b)


def _record(m, c, found, estimated, score, norm_cost, cov):
    r = abi.LoopResult()
    r.found = found
    r.start_node_index = m.node_index
    r.end_node_index = c.node_index
    r.start_node_pose = abi.Pose2D(*m.node_pose)
    r.estimated_pose = abi.Pose2D(*estimated)
    if found:
        rel = ob.lib().orc_inverse_compound(ob.Pose(*m.node_pose), ob.Pose(*estimated))
        r.relative_pose = abi.Pose2D(rel.x, rel.y, rel.theta)
    for k in range(9):
        r.covariance[k] = cov[k]
    r.score = score
    r.normalized_cost = norm_cost
    return np.frombuffer(bytes(r), dtype=np.uint8)


def oracle_sq_detect_fn(kind, maps, cands, params, thr):
    """As loop_oracle.oracle_detect_fn for the detector `kind` ("rtcsm", "bb",
    "gs") whose matcher was constructed with CostSquareError: the records'
    normalized_cost and covariance are the oracle's square-error values at the
    oracle matcher's best sensor pose, for found and not-found candidates alike."""

    def fn(subq, lo, hi):
        out = np.zeros((hi - lo, RECORD_BYTES), dtype=np.uint8)
        for q, first, count in subq:
            m = maps[q]
            map3 = (m.cells, m.min_x, m.min_y)
            for j in range(first, first + count):
                c = cands[lo + j]
                if kind == "rtcsm":
                    ref = ref_rtcsm(map3, m.res, params, c.ranges, c.angles, c.pose, thr=thr)
                    found, est, score = ref.s.pose_found, pose3(ref.s.estimated_pose), ref.s.score_max
                elif kind == "bb":
                    ref = ref_bb(map3, m.res, params, c.ranges, c.angles, c.pose, thr=thr)
                    found, est, score = ref.s.pose_found, pose3(ref.s.estimated_pose), ref.s.score_max
                else:
                    ref = ref_gs(map3, m.res, params, c.ranges, c.angles, c.pose, nthr=thr)
                    found, est, score = ref.s.pose_found, ref.s.estimated_pose, ref.s.score_max
                out[j] = _record(m, c, found, est, score, ref.sq_cost, ref.sq_cov)
        return out

    return fn


def differing_bytes(a, b):
    """the set of byte offsets (within a record) at which two record arrays differ"""
    a, b = np.asarray(a).reshape(-1, RECORD_BYTES), np.asarray(b).reshape(-1, RECORD_BYTES)
    return set(np.nonzero((a != b).any(axis=0))[0].tolist())
