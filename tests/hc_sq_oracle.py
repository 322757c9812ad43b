"""The reference's hill-climbing matcher with CostSquareError composed over the
CPU oracle: ScanMatcherHillClimbing::OptimizePose
(C/mapping/scan_matcher_hill_climbing.cpp:26-109), statement for statement,
over the oracle's pinned orc_sq_cost, orc_sq_covariance, orc_compound and
orc_move_backward.

TEST INFRASTRUCTURE ONLY (tests/test_gpu_hc_sq.py, tools/bench_hc.py's CPU baseline).
"""
import ctypes as C

import oracle_bind as ob
from hc_oracle import MOVE_THETA, MOVE_X, MOVE_Y, Ref

SQ_RANGE = (0.01, 20.0)   # CostSquareError in launcher_settings_default.json:12-15


def sq_cost(g, sc, pose, usable=SQ_RANGE):
    return ob.lib().orc_sq_cost(C.byref(g.g), usable[0], usable[1], C.byref(sc.s), ob.Pose(*pose))


def sq_covariance(g, sc, pose, usable=SQ_RANGE):
    cov = (C.c_double * 9)()
    ob.lib().orc_sq_covariance(C.byref(g.g), usable[0], usable[1], C.byref(sc.s), ob.Pose(*pose), cov)
    return list(cov)


def compose_hc_sq(g, sc, init, rel, lin_step, ang_step, max_iterations, max_refinements, usable=SQ_RANGE):
    """g: ob.OGrid, sc: ob.OScan (its rel_sensor_pose = rel)."""
    L = ob.lib()
    s = L.orc_compound(ob.Pose(*init), ob.Pose(*rel))
    sensor = (s.x, s.y, s.theta)
    min_cost = sq_cost(g, sc, sensor, usable)
    best = sensor
    num_iterations = num_refinements = 0
    lin, ang = lin_step, ang_step
    moves, costs = [], []
    evals = 1
    while True:   # do { ... } while (...)
        min_local, best_local, updated, move = min_cost, best, False, -1
        for i in range(6):
            local = (best[0] + MOVE_X[i] * lin, best[1] + MOVE_Y[i] * lin, best[2] + MOVE_THETA[i] * ang)
            c = sq_cost(g, sc, local, usable)
            evals += 1
            if c < min_local:
                min_local, best_local, updated, move = c, local, True, i
        if updated:
            min_cost, best = min_local, best_local
        else:
            num_refinements += 1
            lin *= 0.5
            ang *= 0.5
        moves.append(move)
        costs.append(min_cost)
        if not (updated or num_refinements < max_refinements):
            break
        num_iterations += 1
        if not num_iterations < max_iterations:
            break
    r = Ref()
    r.moves, r.costs = moves, costs
    r.passes = len(moves)
    r.num_iterations, r.num_refinements = num_iterations, num_refinements
    r.final_steps = (lin, ang)
    r.min_cost = min_cost
    r.best = best
    r.normalized_cost = min_cost / len(sc.r)
    e = L.orc_move_backward(ob.Pose(*best), ob.Pose(*rel))
    r.estimated_pose = (e.x, e.y, e.theta)
    r.covariance = sq_covariance(g, sc, best, usable)
    r.cost_evals = evals   # the analytic gradient calls Cost not once
    return r
