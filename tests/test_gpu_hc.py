"""GPU parity tests of the hill-climbing matcher: lgs_cost_ge_exact,
lgs_hc_trace, lgs_hc_optimize_pose_query / _batch against the reference's
loop composed over the oracle's pinned pieces (hc_oracle.compose_hc):
ScanMatcherHillClimbing::OptimizePose (C/mapping/scan_matcher_hill_climbing.cpp:26-109)
over orc_cost_ge_cost, orc_cost_ge_covariance, orc_compound, orc_move_backward.

Bar: every comparison is bitwise (== / .tobytes()); there is no tolerance.

Inputs: the map of the grid-search tests (four scans) has no cell below the
occupancy threshold 0.1 -- a free cell sits at about 0.31 after four misses --
so the launcher cost is constant on it and a walk never moves.  The walks here
run on a map of 24 scans, and the composed reference is checked to be alive
(accepted moves, all six move kinds, walks cut short by max_iterations) before
anything is compared with it.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_bind as ob
from conftest import launcher_cost
from hc_oracle import compose_hc
from lgs_amd import abi, scene
from test_gpu_gs import draw
from test_gpu_rtcsm import build_map

pytestmark = pytest.mark.gpu
LGS_ERR_INVALID_ARG = 1
LGS_ERR_INTERNAL = 5
REL = (0.1, -0.05, 0.02)
RES = 0.05
DEFAULTS = (0.1, 0.1, 100, 5)   # launcher_settings_default.json:22-29
SEEDS = range(6)
# name -> (linear step, angular step, max iterations, max refinements)
VARIANTS = {"defaults": DEFAULTS, "it6": (0.1, 0.1, 6, 5), "it1": (0.1, 0.1, 1, 5), "it0": (0.1, 0.1, 0, 5),
            "ref0": (0.1, 0.1, 100, 0)}
COST_VALS = (0.01, 20.0, 0.075, 0.1)


def cost_pair(K=1, scale=0.05, stddev=1.0):
    vals = COST_VALS + (K, scale, stddev)
    return abi.CostGEParams(*vals), ob.CostGE(*vals)


def reference(map3, prm, r, ang, init, cost=None, rel=REL):
    cells, mx, my = map3
    return compose_hc(ob.OGrid(cells, mx, my, RES), cost or launcher_cost(oracle=True), ob.OScan(r, ang, rel), init,
                      rel, *prm)


def assert_summary(s, ref, init, tag=""):
    assert s.pose_found == 1, tag
    assert s.passes == ref.passes, (tag, s.passes, ref.passes)
    assert (s.num_iterations, s.num_refinements) == (ref.num_iterations, ref.num_refinements), tag
    assert (s.final_linear_step, s.final_angular_step) == ref.final_steps, tag
    assert s.min_cost == ref.min_cost, (tag, s.min_cost, ref.min_cost)
    assert s.best_sensor_pose.tuple() == ref.best, (tag, s.best_sensor_pose.tuple(), ref.best)
    assert s.normalized_cost == ref.normalized_cost, (tag, s.normalized_cost, ref.normalized_cost)
    assert s.initial_pose.tuple() == tuple(init), tag
    assert s.estimated_pose.tuple() == ref.estimated_pose, (tag, s.estimated_pose.tuple(), ref.estimated_pose)
    assert np.array(list(s.covariance)).tobytes() == np.array(ref.covariance).tobytes(), \
        (tag, list(s.covariance), ref.covariance)
    assert s.cost_evals == ref.cost_evals == 1 + 6 * ref.passes + 6, tag


@pytest.fixture(scope="module")
def dense_map(world):
    return build_map(world, 300, RES, 100, scene.arc_poses(24), n_beams=1081)


@pytest.fixture(scope="module")
def dense_grid(ctx, dense_map):
    cells, mx, my = dense_map
    return ctx.grid_from_array(cells, mx, my, RES)


@pytest.fixture(scope="module")
def sparse_map(world):
    """the grid-search tests' map: the launcher cost is constant on it"""
    return build_map(world, 300, RES, 100, scene.arc_poses(4), n_beams=361)


@pytest.fixture(scope="module")
def scans(world):
    return [draw(world, seed, 361) for seed in SEEDS]


@pytest.fixture(scope="module")
def refs(dense_map, scans):
    """the composed reference of every (variant, seed), computed once, and the
    properties that show the walks exercise the matcher"""
    out = {name: [reference(dense_map, prm, *scans[seed]) for seed in SEEDS] for name, prm in VARIANTS.items()}
    full = out["defaults"]
    assert all(sum(m >= 0 for m in r.moves) >= 4 for r in full), [r.moves for r in full]
    assert {m for r in full for m in r.moves} == {-1, 0, 1, 2, 3, 4, 5}
    assert all(r.num_refinements == 5 for r in full)
    cut = out["it6"]
    assert all(r.num_iterations == 6 and r.passes == 6 and r.num_refinements < 5 for r in cut), \
        [(r.num_iterations, r.num_refinements) for r in cut]
    assert any(r.moves[-1] >= 0 for r in cut)
    assert all(r.passes == 1 for r in out["it1"] + out["it0"])
    return out


# ---------------------------------------------------------------- the cost
def poses_around(init, seed, n=64):
    rng = np.random.default_rng(900 + seed)
    return [(init[0] + rng.uniform(-0.2, 0.2), init[1] + rng.uniform(-0.2, 0.2), init[2] + rng.uniform(-0.1, 0.1))
            for _ in range(n)]


def oracle_costs(map3, ocost, r, ang, poses, rel=(0.0, 0.0, 0.0)):
    cells, mx, my = map3
    g, sc = ob.OGrid(cells, mx, my, RES), ob.OScan(r, ang, rel)
    return np.array([ob.lib().orc_cost_ge_cost(C.byref(g.g), C.byref(ocost), C.byref(sc.s), ob.Pose(*p))
                     for p in poses])


@pytest.mark.parametrize("scale,stddev", [(0.05, 1.0), (1.0, 0.05)])
@pytest.mark.parametrize("K", [1, 2])
def test_cost_exact(ctx, dense_map, dense_grid, scans, K, scale, stddev):
    gcost, ocost = cost_pair(K, scale, stddev)
    for seed in (0, 3):
        r, ang, init = scans[seed]
        poses = poses_around(init, seed)
        ref = oracle_costs(dense_map, ocost, r, ang, poses)
        assert len(set(ref.tolist())) > 32   # a live cost, not the constant
        gpu = ctx.cost_ge_exact(dense_grid, gcost, ctx.scan(r, ang), poses)
        assert gpu.tobytes() == ref.tobytes(), (seed, int((gpu != ref).sum()), float(np.abs(gpu - ref).max()))


def test_cost_exact_filtered_beams(ctx, dense_map, dense_grid, scans):
    """filtered beams interleaved: range 0.0 <= minRange, 25.0 >= maxRange"""
    r, ang, init = scans[1]
    r = r.copy()
    r[::7] = 0.0
    r[::11] = 25.0
    gcost, ocost = cost_pair()
    poses = poses_around(init, 1)
    ref = oracle_costs(dense_map, ocost, r, ang, poses)
    assert len(set(ref.tolist())) > 32
    gpu = ctx.cost_ge_exact(dense_grid, gcost, ctx.scan(r, ang), poses)
    assert gpu.tobytes() == ref.tobytes()


def test_cost_exact_window_leaves_the_map(ctx, dense_map, scans):
    """the map cropped so that its low edges run through the room: hit points
    and kernel windows reach negative cell indices"""
    cells, mx, my = dense_map
    cx0, cy0 = int(round((-1.0 - mx) / RES)), int(round((-0.5 - my) / RES))
    crop = (np.ascontiguousarray(cells[cy0:, cx0:]), mx + cx0 * RES, my + cy0 * RES)
    grid = ctx.grid_from_array(*crop, RES)
    gcost, ocost = cost_pair()
    for seed in (0, 2):
        r, ang, init = scans[seed]
        poses = poses_around(init, 10 + seed)
        # a pose on the corner cell itself: the window straddles index -1 / 0 on both axes
        poses[0] = (crop[1] + 0.01, crop[2] + 0.01, init[2])
        hx = np.array([p[0] + r * np.cos(p[2] + ang) for p in poses])
        hy = np.array([p[1] + r * np.sin(p[2] + ang) for p in poses])
        assert (hx < crop[1] - RES).any() and (hy < crop[2] - RES).any() and (hx > crop[1] + RES).any()
        ref = oracle_costs(crop, ocost, r, ang, poses)
        assert len(set(ref.tolist())) > 32
        gpu = ctx.cost_ge_exact(grid, gcost, ctx.scan(r, ang), poses)
        assert gpu.tobytes() == ref.tobytes(), int((gpu != ref).sum())


def test_cost_exact_unknown_map(ctx, scans):
    """every cell unknown: every valid beam takes the start distance"""
    empty = (np.zeros((120, 130)), -3.0, -3.25)
    grid = ctx.grid_from_array(*empty, RES)
    gcost, ocost = cost_pair()
    r, ang, init = scans[4]
    poses = poses_around(init, 4, 8)
    ref = oracle_costs(empty, ocost, r, ang, poses)
    assert len(set(ref.tolist())) == 1 and ref[0] < 0.0
    gpu = ctx.cost_ge_exact(grid, gcost, ctx.scan(r, ang), poses)
    assert gpu.tobytes() == ref.tobytes()


def test_cost_exact_more_poses_than_one_workgroup_and_none(ctx, dense_map, dense_grid, scans):
    """7 poses span two workgroups of six; n = 0 writes nothing"""
    r, ang, init = scans[5]
    gcost, ocost = cost_pair()
    poses = poses_around(init, 5, 7)
    gpu = ctx.cost_ge_exact(dense_grid, gcost, ctx.scan(r, ang), poses)
    assert gpu.tobytes() == oracle_costs(dense_map, ocost, r, ang, poses).tobytes()
    assert len(ctx.cost_ge_exact(dense_grid, gcost, ctx.scan(r, ang), [])) == 0


# ---------------------------------------------------------------- the walk
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_walk(ctx, dense_grid, scans, refs, variant, seed):
    """trace and summary: launcher defaults, max_iterations 6 / 1 / 0, no refinements"""
    r, ang, init = scans[seed]
    ref = refs[variant][seed]
    prm = abi.HCParams(*VARIANTS[variant])
    sc = ctx.scan(r, ang, REL)
    moves, costs = ctx.hc_trace(dense_grid, prm, launcher_cost(), sc, init)
    assert len(moves) == ref.passes, (len(moves), ref.passes)
    assert moves.tolist() == ref.moves, (moves.tolist(), ref.moves)
    assert costs.tobytes() == np.array(ref.costs).tobytes(), (costs.tolist(), ref.costs)
    s = ctx.hc_optimize_pose_query(dense_grid, prm, launcher_cost(), sc, init)
    assert_summary(s, ref, init, f"{variant} seed{seed}")
    if variant in ("it1", "it0"):
        assert s.passes == 1


def test_walk_empty_map(ctx, scans):
    """nothing to climb: 5 passes, all refinements; the increment of
    numOfIterations is skipped when the left side of the loop condition is false"""
    empty = (np.zeros((300, 300)), -7.5, -7.5)
    grid = ctx.grid_from_array(*empty, RES)
    r, ang, init = scans[0]
    ref = reference(empty, DEFAULTS, r, ang, init)
    assert (ref.passes, ref.num_iterations, ref.num_refinements) == (5, 4, 5) and ref.moves == [-1] * 5
    prm = abi.HCParams(*DEFAULTS)
    sc = ctx.scan(r, ang, REL)
    s = ctx.hc_optimize_pose_query(grid, prm, launcher_cost(), sc, init)
    assert (s.passes, s.num_iterations, s.num_refinements) == (5, 4, 5)
    assert (s.final_linear_step, s.final_angular_step) == (0.1 / 32, 0.1 / 32)
    assert_summary(s, ref, init)
    moves, costs = ctx.hc_trace(grid, prm, launcher_cost(), sc, init)
    assert moves.tolist() == [-1] * 5 and costs.tobytes() == np.array(ref.costs).tobytes()


@pytest.mark.parametrize("n_beams", [1081, 2000, 8200])
def test_walk_term_rows(ctx, world, dense_map, dense_grid, n_beams):
    """where the term rows (6 N doubles) live: in LDS within the 64 KiB default
    (1081 beams, and the 361 of the walks above), in LDS beyond it (2000) and
    -- 6 x 8200 doubles cannot fit a CU's 160 KiB -- in the global rows"""
    r, ang, init = draw(world, 1, n_beams)
    ref = reference(dense_map, DEFAULTS, r, ang, init)
    assert sum(m >= 0 for m in ref.moves) >= 4
    prm = abi.HCParams(*DEFAULTS)
    sc = ctx.scan(r, ang, REL)
    moves, costs = ctx.hc_trace(dense_grid, prm, launcher_cost(), sc, init)
    assert moves.tolist() == ref.moves
    assert costs.tobytes() == np.array(ref.costs).tobytes()
    assert_summary(ctx.hc_optimize_pose_query(dense_grid, prm, launcher_cost(), sc, init), ref, init, str(n_beams))
    # the cost entry takes the same path
    gcost, ocost = cost_pair()
    poses = poses_around(init, 7, 7)
    gpu = ctx.cost_ge_exact(dense_grid, gcost, ctx.scan(r, ang), poses)
    assert gpu.tobytes() == oracle_costs(dense_map, ocost, r, ang, poses).tobytes()


def test_batch_equals_lone_calls(ctx, world, dense_map, dense_grid, sparse_map):
    """six matches of different beam counts, two maps among them, different
    walk lengths: byte-identical to six lone calls and to the reference, and
    again after an unrelated correlative match on the same context"""
    sparse_grid = ctx.grid_from_array(*sparse_map, RES)
    maps = [(dense_map, dense_grid), (sparse_map, sparse_grid)]
    items = []
    for k in range(6):
        r, ang, init = draw(world, 20 + k, 361 if k % 2 == 0 else 1081)
        m, g = maps[1 if k in (2, 5) else 0]
        items.append((m, g, r, ang, init, ctx.scan(r, ang, REL)))
    prm = abi.HCParams(*DEFAULTS)
    ref = [reference(m, DEFAULTS, r, ang, init) for m, g, r, ang, init, sc in items]
    assert len({x.passes for x in ref}) >= 3 and ref[2].passes == 5 and max(x.passes for x in ref) > 8

    def batch():
        return ctx.hc_optimize_pose_batch([it[1] for it in items], prm, launcher_cost(), [it[5] for it in items],
                                          [it[4] for it in items])

    first = batch()
    lone = [ctx.hc_optimize_pose_query(g, prm, launcher_cost(), sc, init) for m, g, r, ang, init, sc in items]
    for k in range(6):
        assert bytes(first[k]) == bytes(lone[k]), k
        assert_summary(first[k], ref[k], items[k][4], f"item{k}")
    # workspace history: an unrelated RTCSM match in between
    m, g, r, ang, init, sc = items[0]
    ctx.optimize_pose_query(g, abi.RtcsmParams(5, 0.6, 0.6, 0.4, 20.0), launcher_cost(), sc, init)
    again = batch()
    assert [bytes(x) for x in again] == [bytes(x) for x in first]


# ---------------------------------------------------------------- arguments
def test_argument_errors(ctx, dense_grid, scans):
    r, ang, init = scans[0]
    sc = ctx.scan(r, ang, REL)
    lib = ctx.lib

    def query(prm, cost, pose):
        out = abi.HCSummary()
        return lib.lgs_hc_optimize_pose_query(ctx.h, dense_grid.h, C.byref(abi.HCParams(*prm)), C.byref(cost), sc.h,
                                              abi.Pose2D(*pose), C.byref(out))

    assert query(DEFAULTS, launcher_cost(), init) == abi.LGS_OK
    assert query((0.0, 0.1, 100, 5), launcher_cost(), init) == LGS_ERR_INVALID_ARG
    assert query((0.1, 0.0, 100, 5), launcher_cost(), init) == LGS_ERR_INVALID_ARG
    assert query((float("nan"), 0.1, 100, 5), launcher_cost(), init) == LGS_ERR_INVALID_ARG
    assert query(DEFAULTS, launcher_cost(), (float("nan"), init[1], init[2])) == LGS_ERR_INVALID_ARG
    assert query(DEFAULTS, launcher_cost(), (init[0], init[1], float("inf"))) == LGS_ERR_INVALID_ARG
    assert query((0.1, 0.1, 65537, 5), launcher_cost(), init) == LGS_ERR_INVALID_ARG
    assert query(DEFAULTS, cost_pair(K=17)[0], init) == LGS_ERR_INVALID_ARG
    # n = 0: OK, nothing written
    out = (abi.HCSummary * 1)()
    C.memset(out, 0x5A, C.sizeof(out))
    rc = lib.lgs_hc_optimize_pose_batch(ctx.h, None, C.byref(abi.HCParams(*DEFAULTS)), C.byref(launcher_cost()), None,
                                        None, 0, out)
    assert rc == abi.LGS_OK and bytes(out) == b"\x5A" * C.sizeof(out)
    # the context still matches
    assert query(DEFAULTS, launcher_cost(), init) == abi.LGS_OK


def test_angle_outside_the_sincos_domain_is_an_error(ctx, dense_grid, scans):
    """|theta + angle| >= 105414350 is outside the restated glibc sincos: the
    device raises its error flag and the call fails, as the grid search does"""
    r, ang, init = scans[0]
    sc = ctx.scan(r, ang, REL)
    out = np.zeros(1)
    poses = (abi.Pose2D * 1)(abi.Pose2D(init[0], init[1], 2.0e8))
    rc = ctx.lib.lgs_cost_ge_exact(ctx.h, dense_grid.h, C.byref(launcher_cost()), sc.h, poses, 1, abi.dptr(out))
    assert rc == LGS_ERR_INTERNAL
    hs = abi.HCSummary()
    rc = ctx.lib.lgs_hc_optimize_pose_query(ctx.h, dense_grid.h, C.byref(abi.HCParams(*DEFAULTS)),
                                            C.byref(launcher_cost()), sc.h, abi.Pose2D(init[0], init[1], 2.0e8),
                                            C.byref(hs))
    assert rc == LGS_ERR_INTERNAL
