"""Snapshots and hints shared by the loop searcher's CPU and GPU tests
(tests/test_loop_search_cpu.py, tests/test_gpu_loop_search.py): small walks
(about 300 positions) built so that every edge of DESIGN.md 4.6g is hit.
Each case is (name, poses n x 2, idx_min, idx_max, Params, [Hint])."""
import math
from collections import namedtuple

import numpy as np

import loop_search_oracle as orc

Case = namedtuple("Case", "name poses idx_min idx_max prm hints")


def ranges_of(sizes):
    """consecutive inclusive node ranges of the given sizes"""
    lo, hi, k = [], [], 0
    for s in sizes:
        lo.append(k)
        hi.append(k + s - 1)
        k += s
    return lo, hi


def accum_at(poses):
    """UpdateAccumTravelDist's chain after every node: accum[k] = the sum over nodes 1 .. k"""
    out, t = [0.0], 0.0
    for i in range(1, len(poses)):
        t += orc.hypot(poses[i - 1][0] - poses[i][0], poses[i - 1][1] - poses[i][1])
        out.append(t)
    return out


def hints_of_nodes(nodes, idx_min, idx_max, accum, num_maps=None):
    """the hint the reference forms when node k is the latest one: the first map that holds it is the
    latest, unfinished one, and the maps before it are walked"""
    out = []
    for k in nodes:
        lm = next(i for i in range(len(idx_min)) if idx_min[i] <= k <= idx_max[i])
        out.append(orc.Hint(int(k), lm, lm + 1 if num_maps is None else num_maps, accum[k]))
    return out


def figure_eight(n, offset=0.0, step=0.11):
    """a path that crosses itself again and again, so that loops exist at every scale"""
    k = np.arange(n)
    return np.stack([4.0 * np.sin(step * k) + offset, 3.0 * np.sin(2.0 * step * k + 0.3) + offset], axis=1)


def lattice_path(n, seed):
    """steps of (3, 4) or (4, 3) times a power of two and a sign: every hypot is exact, and so is every sum"""
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 2))
    for i in range(1, n):
        a, b = ((3.0, 4.0), (4.0, 3.0))[int(rng.integers(2))]
        s = 2.0 ** int(rng.integers(-3, 2))
        p[i] = p[i - 1] + (a * s * rng.choice([-1.0, 1.0]), b * s * rng.choice([-1.0, 1.0]))
    return p


SIZES = [17, 1, 1, 40, 100, 1, 23, 64, 9, 31, 1, 42]   # 330 nodes: one-node maps, one map above a 64-position group


def main_case(offset=0.0, name="figure eight"):
    poses = figure_eight(sum(SIZES), offset)
    lo, hi = ranges_of(SIZES)
    acc = accum_at(poses)
    return Case(name, poses, lo, hi, orc.Params(3.0, 0.8, 3), hints_of_nodes(range(len(poses)), lo, hi, acc))


def cases():
    out = [main_case()]
    out.append(main_case(1.0e5, "poses near 1e5"))

    # the same node in two maps: the first map wins
    poses = figure_eight(80, step=0.16)
    lo, hi = [0, 15, 35, 55], [20, 40, 60, 79]
    acc = accum_at(poses)
    hints = [orc.Hint(k, 3, 4, acc[k]) for k in range(55, 80)]
    out.append(Case("overlapping ranges", poses, lo, hi, orc.Params(1.0, 1.5, 2), hints))

    # duplicate poses: the lowest position wins
    poses = figure_eight(120, step=0.2)
    poses[10:14] = poses[10]
    poses[40:43] = poses[10]
    poses[100] = poses[10]
    lo, hi = ranges_of([30, 30, 30, 30])
    acc = accum_at(poses)
    out.append(Case("duplicate poses", poses, lo, hi, orc.Params(0.5, 1.0, 1),
                    hints_of_nodes(range(90, 120), lo, hi, acc)))

    # d2 == pow(threshold, 2): a strict <, so not found; one node just inside is
    poses = np.array([[0.0, 0.0], [0.0, 0.0], [8.0, 0.0], [3.0, 4.0]])
    out.append(Case("d2 equals the squared threshold", poses, [0, 2, 3], [1, 2, 3], orc.Params(0.0, 5.0, 0),
                    [orc.Hint(3, 2, 3, 100.0)]))
    poses = np.array([[0.0, 0.0], [0.0, 0.0], [8.0, 0.0], [3.0, 4.0 - 2.0 ** -40]])
    out.append(Case("d2 just below the squared threshold", poses, [0, 2, 3], [1, 2, 3], orc.Params(0.0, 5.0, 0),
                    [orc.Hint(3, 2, 3, 100.0)]))

    # accum - travel == threshold continues, one ulp below stops (a lattice: the chain is exact)
    poses = lattice_path(60, 5)
    lo, hi = ranges_of([12, 9, 20, 19])
    travel = orc.travel_chain(poses, lo, hi)
    thr, hints = 7.0, []
    for p in (0, 5, 11, 12, 30, 40):
        edge = travel[p] + thr
        assert edge - travel[p] == thr
        hints += [orc.Hint(59, 3, 4, edge), orc.Hint(59, 3, 4, math.nextafter(edge, -math.inf)),
                  orc.Hint(59, 3, 4, math.nextafter(edge, math.inf))]
    hints += [orc.Hint(59, 3, 4, 0.0), orc.Hint(59, 3, 4, -3.0), orc.Hint(59, 3, 4, 1.0e9)]   # cut at 0; never cut
    out.append(Case("travel threshold edges", poses, lo, hi, orc.Params(thr, 1.0e3, 4), hints))

    # num_maps = 1 (nothing walked), num_maps < m (unwalked rows none), one map only
    poses = figure_eight(100, step=0.21)
    lo, hi = ranges_of([25, 25, 25, 25])
    acc = accum_at(poses)
    hints = [orc.Hint(k, 0, 1, acc[k]) for k in (0, 7, 24)]
    hints += [orc.Hint(k, 1, 2, acc[k]) for k in range(25, 50, 3)]
    hints += [orc.Hint(k, 2, 3, acc[k]) for k in range(50, 75, 3)]
    hints += [orc.Hint(k, 3, 4, acc[k]) for k in range(75, 100, 3)]
    out.append(Case("fewer maps than the snapshot", poses, lo, hi, orc.Params(0.5, 2.0, 5), hints))
    out.append(Case("one map", poses, [0], [99], orc.Params(0.5, 2.0, 5), [orc.Hint(50, 0, 1, acc[50])]))

    # nothing within range; a negative travel threshold; K = 0 and K = INT_MAX
    base = main_case()
    some = base.hints[200:330:7]
    out.append(Case("no node within range", base.poses, base.idx_min, base.idx_max, orc.Params(3.0, 1.0e-6, 3), some))
    out.append(Case("negative travel threshold", base.poses, base.idx_min, base.idx_max, orc.Params(-2.0, 0.8, 0), some))
    out.append(Case("widest node range", base.poses, base.idx_min, base.idx_max, orc.Params(3.0, 0.8, 2 ** 31 - 1), some))
    return out


def hint_rows(hints, dtype):
    h = np.zeros(len(hints), dtype=dtype)
    for j, x in enumerate(hints):
        h[j] = (x.latest_node_idx, x.latest_local_map_idx, x.num_maps, 0, x.accum_travel_dist)
    return h
