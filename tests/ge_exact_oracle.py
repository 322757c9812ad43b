"""Oracle-side helpers for LGS_COST_GREEDY_ENDPOINT_EXACT (test infrastructure only).

The reference of every kind-2 comparison is the oracle as it stands: the
summaries of orc_rtcsm_optimize_pose*, bb_oracle.oracle_bb and
test_gpu_gs.compose_gs already carry orc_cost_ge_cost / NumOfScans() and
orc_cost_ge_covariance at the matcher's best sensor pose, found or not.  For
cost parameters other than the launcher's, ge_at evaluates the same two oracle
functions at that pose.  Every comparison is equality of bytes.
"""
import ctypes as C

import numpy as np

import oracle_bind as ob
from lgs_amd import abi

LAUNCHER = (0.01, 20.0, 0.075, 0.1, 1, 0.05, 1.0)   # conftest.launcher_cost
REL = (0.1, -0.05, 0.02)
RES = 0.05


def exact_spec(vals=LAUNCHER):
    return abi.cost_spec(abi.CostGEParams(*vals), exact=True)


def oracle_cost(g, sc, pose, vals=LAUNCHER):
    """CostGreedyEndpoint(*vals)::Cost at `pose`"""
    return ob.lib().orc_cost_ge_cost(C.byref(g.g), C.byref(ob.CostGE(*vals)), C.byref(sc.s), ob.Pose(*pose))


def oracle_covariance(g, sc, pose, vals=LAUNCHER):
    cov = (C.c_double * 9)()
    ob.lib().orc_cost_ge_covariance(C.byref(g.g), C.byref(ob.CostGE(*vals)), C.byref(sc.s), ob.Pose(*pose), cov)
    return list(cov)


def ge_at(map3, res, r, ang, rel, pose, vals=LAUNCHER):
    """(Cost / NumOfScans(), covariance) of CostGreedyEndpoint(*vals) at `pose`"""
    cells, mx, my = map3
    g, sc = ob.OGrid(cells, mx, my, res), ob.OScan(r, ang, rel, 0.0, 30.0)
    return oracle_cost(g, sc, pose, vals) / len(r), oracle_covariance(g, sc, pose, vals)


def seven_poses(pose, res):
    """the pose and the six poses of ComputeGradient around it (:119-136)"""
    x, y, th = pose
    dl, da = res, 1e-2
    return [(x, y, th), (x + dl, y + 0.0, th + 0.0), (x - dl, y - 0.0, th - 0.0), (x + 0.0, y + dl, th + 0.0),
            (x - 0.0, y - dl, th - 0.0), (x + 0.0, y + 0.0, th + da), (x - 0.0, y - 0.0, th - da)]


def beam_terms(map3, res, r, ang, rel, pose, vals=LAUNCHER):
    """The term of every beam at `pose`, from the oracle alone: with a scaling
    factor of 1 the cost of a one-beam scan is (0.0 - term) * 1.0, the negated
    term exactly."""
    cells, mx, my = map3
    g = ob.OGrid(cells, mx, my, res)
    unit = vals[:5] + (1.0,) + vals[6:]
    out = []
    for k in range(len(r)):
        sc = ob.OScan(r[k:k + 1].copy(), ang[k:k + 1].copy(), rel, 0.0, 30.0)
        out.append(-oracle_cost(g, sc, pose, unit))
    return out


def assert_gx(summary, best, cost, cov, tag=""):
    """the summary's cost fields are the oracle's greedy-endpoint values, bit for bit"""
    assert summary.best_sensor_pose.tuple() == tuple(best), (tag, summary.best_sensor_pose.tuple(), best)
    assert summary.normalized_cost == cost, (tag, summary.normalized_cost, cost)
    assert np.array(list(summary.covariance)).tobytes() == np.array(list(cov)).tobytes(), \
        (tag, list(summary.covariance), list(cov))


def assert_gx_ref(summary, ref, tag=""):
    """against a cost_spec_oracle reference (ref.s: the oracle matcher's own summary)"""
    cov = ref.s.covariance
    assert_gx(summary, ref.best, ref.s.normalized_cost, list(cov), tag)


def oracle_ge_detect_fn(kind, maps, cands, params, thr):
    """As loop_oracle.oracle_detect_fn (the "rtcsm" reference itself) for the
    detectors "bb" and "gs": the oracle matcher's own summary, whose
    normalized_cost and covariance are the greedy-endpoint values at its best
    sensor pose for found and not-found candidates alike, as a 176-byte record."""
    import cost_spec_oracle as cso
    from lgs_amd.loopbatch import RECORD_BYTES

    def fn(subq, lo, hi):
        out = np.zeros((hi - lo, RECORD_BYTES), dtype=np.uint8)
        for q, first, count in subq:
            m = maps[q]
            map3 = (m.cells, m.min_x, m.min_y)
            for j in range(first, first + count):
                c = cands[lo + j]
                if kind == "bb":
                    s = cso.ref_bb(map3, m.res, params, c.ranges, c.angles, c.pose, thr=thr).s
                    est = cso.pose3(s.estimated_pose)
                else:
                    s = cso.ref_gs(map3, m.res, params, c.ranges, c.angles, c.pose, nthr=thr).s
                    est = s.estimated_pose
                out[j] = cso._record(m, c, s.pose_found, est, s.score_max, s.normalized_cost, list(s.covariance))
        return out

    return fn
