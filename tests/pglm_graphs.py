"""Graphs shared by the tests of the device-resident pose-graph optimizer
(tests/test_gpu_pglm.py, tests/test_pglm_cpu.py): the seeds of
tests/test_gpu_pgcg.py, for which the LM schedule of the host's and the
device's conjugate gradients is known to agree, plus a self-loop edge.  Test
infrastructure only."""
import functools

import numpy as np

import lm_oracle as lo
import pgcg_oracle as po

LOSSES = [(0, 1.0), (1, 0.5), (2, 2.0), (3, 1.0), (4, 3.0), (5, 2.0), (6, 1.0)]
# Weight is IEEE arithmetic only (+, -, *, /, sqrt): the device's H equals the host's byte for byte.
# DCS is among them: GCC folds its pow(x, 2.0) to x * x, which is what the device evaluates
WEIGHT_EXACT = (0, 1, 2, 3, 5, 6)
# Loss is IEEE-only as well: the total error is the host's, byte for byte
LOSS_EXACT = (0, 3, 5, 6)
LINEARISE_GRAPHS = ["n1", "n2", "dup", "hub", "selfloop", "n300"]


@functools.lru_cache(maxsize=None)
def graph(name):
    """(initial poses [n, 3], edges [(start, end, z, info)])"""
    if name == "n1":
        return np.array([[0.3, -0.2, 0.1]]), []
    if name == "hub":      # node 5 starts 327 loop edges: one block row of 329 neighbours
        return po.hub_graph(330, 5, np.random.default_rng(21))
    if name == "dup":      # a pair named in both directions and three times over
        init, edges = lo.random_graph(40, 3, np.random.default_rng(22))
        info = np.diag([50.0, 80.0, 200.0])
        z = tuple(lo.error(init[3], init[17], (0.0, 0.0, 0.0)))
        zi = tuple(lo.error(init[17], init[3], (0.0, 0.0, 0.0)))
        return init, edges + [(3, 17, z, info), (17, 3, zi, info), (3, 17, z, 2.0 * info)]
    if name == "selfloop":  # an edge from a node to itself: four terms on one diagonal block
        init, edges = lo.random_graph(80, 12, np.random.default_rng(110), outliers=2)
        return init, edges + [(9, 9, (0.01, -0.02, 0.005), np.array([[90.0, 3.0, 1.0], [3.0, 70.0, 2.0],
                                                                      [1.0, 2.0, 300.0]]))]
    if name == "n300":     # 339 edges: more than one 256-thread workgroup, no multiple of 64
        return lo.random_graph(300, 40, np.random.default_rng(7))
    if name.startswith("loss"):   # the loss cases of test_gpu_pgcg.test_optimize_device_matches_host_cg
        return lo.random_graph(80, 12, np.random.default_rng(110 + int(name[4:])), outliers=2)
    n = int(name[1:])
    return lo.random_graph(n, max(1, n // 25), np.random.default_rng(20 + n))


def dense_blocks(init, edges, lam, kind, scale):
    """(diag, pairs, off, rhs) of pgcg_oracle.linearise, with a self-loop's four terms on its diagonal block"""
    H, b = po.linearise(init, edges, lam=lam, loss_kind=kind, scale=scale)
    diag, pairs, off = po.blocks(H, edges)
    return diag, pairs, off, -b


# lgs_pose_graph_optimize_lm runs whose poses tests/golden/pglm_host_lm.json records: (graph, solver, loss, scale)
GOLDEN_RUNS = [("loss0", 1, 0, 1.0), ("n300", 0, 1, 0.5), ("selfloop", 1, 2, 2.0)]
GOLDEN_KW = dict(iters=10, tol=1e-6, lam=1e-3)
