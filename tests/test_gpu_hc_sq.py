"""GPU parity tests of CostSquareError for every scan matcher:
lgs_cost_square_error_batch, lgs_hc_sq_trace, lgs_hc_sq_optimize_pose_query /
_batch and lgs_summaries_apply_cost_sq against the reference's code composed
over the oracle's pinned pieces (hc_sq_oracle): ScanMatcherHillClimbing::OptimizePose
(C/mapping/scan_matcher_hill_climbing.cpp:26-109) over orc_sq_cost,
orc_sq_covariance, orc_compound, orc_move_backward.

Bar: every comparison is bitwise (== / .tobytes()); there is no tolerance.

Inputs: the maps and scans of tests/test_gpu_hc.py.  The composed reference is
checked to be alive (accepted moves, all six move kinds, walks cut short by
max_iterations) before anything is compared with it.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_bind as ob
from conftest import launcher_cost
from hc_sq_oracle import SQ_RANGE, compose_hc_sq, sq_covariance, sq_cost
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


def sq():
    return abi.CostSQParams(*SQ_RANGE)


def reference(map3, prm, r, ang, init, rel=REL, res=RES):
    cells, mx, my = map3
    return compose_hc_sq(ob.OGrid(cells, mx, my, res), ob.OScan(r, ang, rel), init, rel, *prm)


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
    assert s.cost_evals == ref.cost_evals == 1 + 6 * ref.passes, tag


@pytest.fixture(scope="module")
def dense_map(world):
    return build_map(world, 300, RES, 100, scene.arc_poses(24), n_beams=1081)


@pytest.fixture(scope="module")
def dense_grid(ctx, dense_map):
    cells, mx, my = dense_map
    return ctx.grid_from_array(cells, mx, my, RES)


@pytest.fixture(scope="module")
def coarse_map(world):
    """the same room at 0.1 m per cell"""
    return build_map(world, 150, 0.1, 50, scene.arc_poses(24), n_beams=1081)


@pytest.fixture(scope="module")
def coarse_grid(ctx, coarse_map):
    cells, mx, my = coarse_map
    return ctx.grid_from_array(cells, mx, my, 0.1)


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


def oracle_costs(map3, r, ang, poses, res=RES, cov=False):
    cells, mx, my = map3
    g, sc = ob.OGrid(cells, mx, my, res), ob.OScan(r, ang)
    c = np.array([sq_cost(g, sc, p) for p in poses])
    if not cov:
        return c
    return c, np.array([sq_covariance(g, sc, p) for p in poses]).reshape(len(poses), 9)


def check_costs(ctx, map3, grid, r, ang, poses, res=RES, live=True):
    """with and without the covariance, against the oracle"""
    ref, rcov = oracle_costs(map3, r, ang, poses, res, cov=True)
    if live:
        assert len(set(ref.tolist())) > len(poses) // 2   # a live cost, not a constant
    sc = ctx.scan(r, ang)
    gpu = ctx.cost_square_error_batch(grid, sq(), sc, poses)
    assert gpu.tobytes() == ref.tobytes(), (int((gpu != ref).sum()), float(np.abs(gpu - ref).max()))
    gpu2, cov = ctx.cost_square_error_batch(grid, sq(), sc, poses, covariance=True)
    assert gpu2.tobytes() == ref.tobytes(), int((gpu2 != ref).sum())
    assert cov.tobytes() == rcov.tobytes(), (int((cov != rcov).sum()), float(np.abs(cov - rcov).max()))
    return ref, rcov


def test_cost_batch(ctx, dense_map, dense_grid, scans):
    """64 poses around two scans"""
    for seed in (0, 3):
        r, ang, init = scans[seed]
        _, rcov = check_costs(ctx, dense_map, dense_grid, r, ang, poses_around(init, seed))
        # a live gradient of either sign: the chains hold negative terms
        assert (rcov[:, 1] < 0).any() and (rcov[:, 1] > 0).any()


def test_cost_batch_filtered_beams(ctx, dense_map, dense_grid, scans):
    """filtered beams interleaved: range 0.0 <= minRange, 25.0 >= maxRange; and all of them"""
    r, ang, init = scans[1]
    r = r.copy()
    r[::7] = 0.0
    r[::11] = 25.0
    check_costs(ctx, dense_map, dense_grid, r, ang, poses_around(init, 1))
    ref, rcov = check_costs(ctx, dense_map, dense_grid, np.full_like(r, 25.0), ang, poses_around(init, 1, 5), live=False)
    assert (ref == 0.0).all() and rcov[0].tolist() == [0.01, 0, 0, 0, 0.01, 0, 0, 0, 0.01]


def test_cost_batch_footprint_leaves_the_map(ctx, dense_map, scans):
    """the map cropped so that its low edges run through the room: hit points
    and bicubic footprints reach negative and beyond-edge cell indices; poses
    far outside, up to where the reference's truncation gives INT_MIN"""
    cells, mx, my = dense_map
    cx0, cy0 = int(round((-1.0 - mx) / RES)), int(round((-0.5 - my) / RES))
    cx1, cy1 = int(round((5.9 - mx) / RES)), int(round((5.8 - my) / RES))   # just inside the room's far walls
    crop = (np.ascontiguousarray(cells[cy0:cy1, cx0:cx1]), mx + cx0 * RES, my + cy0 * RES)
    grid = ctx.grid_from_array(*crop, RES)
    for seed in (0, 2):
        r, ang, init = scans[seed]
        poses = poses_around(init, 10 + seed)
        poses[0] = (crop[1] + 0.01, crop[2] + 0.01, init[2])   # on the corner cell: the footprint straddles index 0
        poses[1] = (-1e4, 1e4, 2.0)
        poses[2] = (-2e8, 2e8, 0.3)                            # (x - min) / res beyond int: INT_MIN, clamped to 0
        poses[3] = (2e8, -2e8, -0.3)
        hx = np.array([p[0] + r * np.cos(p[2] + ang) for p in poses[4:]])
        hy = np.array([p[1] + r * np.sin(p[2] + ang) for p in poses[4:]])
        assert (hx < crop[1] - RES).any() and (hy < crop[2] - RES).any() and (hx > crop[1] + RES).any()
        assert (hx > 5.9 + RES).any() and (hy > 5.8 + RES).any()
        check_costs(ctx, crop, grid, r, ang, poses)


@pytest.mark.parametrize("shape", [(1, 1), (2, 3)])
def test_cost_batch_tiny_maps(ctx, scans, shape):
    """a 1 x 1 and a 3 x 2 map: every bicubic index clamps"""
    rng = np.random.default_rng(5)
    tiny = (rng.uniform(0.05, 0.95, shape), 0.4, 0.2)
    grid = ctx.grid_from_array(*tiny, RES)
    r, ang, init = scans[2]
    r = np.minimum(r, 0.2)
    poses = [(0.4 + rng.uniform(-0.1, 0.25), 0.2 + rng.uniform(-0.1, 0.25), rng.uniform(-3, 3)) for _ in range(9)]
    check_costs(ctx, tiny, grid, r, ang, poses, live=False)


def test_cost_batch_unknown_map(ctx, scans):
    """every cell unknown: S = 0, every valid beam's term is 1"""
    empty = (np.zeros((120, 130)), -3.0, -3.25)
    grid = ctx.grid_from_array(*empty, RES)
    r, ang, init = scans[4]
    ref, rcov = check_costs(ctx, empty, grid, r, ang, poses_around(init, 4, 8), live=False)
    assert len(set(ref.tolist())) == 1 and ref[0] == float(((r > 0.01) & (r < 20.0)).sum())


@pytest.mark.parametrize("n", [0, 1, 70])
def test_cost_batch_item_counts_and_lone_calls(ctx, dense_map, dense_grid, scans, n):
    """no item, one item, and a count that is no multiple of 64: the batch
    equals n lone lgs_cost_square_error calls byte for byte"""
    r, ang, init = scans[5]
    poses = poses_around(init, 5, n)
    sc = ctx.scan(r, ang)
    gpu, cov = ctx.cost_square_error_batch(dense_grid, sq(), sc, poses, covariance=True)
    assert len(gpu) == len(cov) == n
    lone = [ctx.cost_square_error(dense_grid, *SQ_RANGE, sc, p, covariance=True) for p in poses]
    assert gpu.tolist() == [c for c, _ in lone]
    assert cov.tobytes() == np.array([v for _, v in lone]).reshape(n, 9).tobytes()
    if n:
        ref, rcov = oracle_costs(dense_map, r, ang, poses, cov=True)
        assert gpu.tobytes() == ref.tobytes() and cov.tobytes() == rcov.tobytes()


def test_cost_batch_mixes_resolutions_and_scans(ctx, dense_map, dense_grid, coarse_map, coarse_grid, scans, world):
    """items of two maps (0.05 and 0.1 m per cell) and scans of two lengths in one call"""
    items = []
    for k in range(10):
        r, ang, init = scans[k % 6] if k % 3 else draw(world, 30 + k, 1081)
        m, g, res = (coarse_map, coarse_grid, 0.1) if k % 2 else (dense_map, dense_grid, RES)
        items.append((m, g, res, r, ang, poses_around(init, 20 + k, 1)[0]))
    gpu, cov = ctx.cost_square_error_batch([it[1] for it in items], sq(), [ctx.scan(it[3], it[4]) for it in items],
                                           [it[5] for it in items], covariance=True)
    for k, (m, g, res, r, ang, pose) in enumerate(items):
        ref, rcov = oracle_costs(m, r, ang, [pose], res, cov=True)
        assert gpu[k] == ref[0], (k, gpu[k], ref[0])
        assert cov[k].tobytes() == rcov[0].tobytes(), k
    assert len(set(gpu.tolist())) == 10


def test_cost_batch_more_than_one_launch(ctx, dense_map, dense_grid, scans):
    """4100 items: a second launch of four items behind the first chunk of 4096"""
    r, ang, init = scans[2]
    rng = np.random.default_rng(77)
    poses = [(init[0] + rng.uniform(-0.2, 0.2), init[1] + rng.uniform(-0.2, 0.2), init[2] + rng.uniform(-0.1, 0.1))
             for _ in range(4100)]
    gpu, cov = ctx.cost_square_error_batch(dense_grid, sq(), ctx.scan(r, ang), poses, covariance=True)
    ref = oracle_costs(dense_map, r, ang, poses)
    assert gpu.tobytes() == ref.tobytes(), int((gpu != ref).sum())
    pick = list(range(0, 4096, 128)) + list(range(4090, 4100))
    _, rcov = oracle_costs(dense_map, r, ang, [poses[k] for k in pick], cov=True)
    assert cov[pick].tobytes() == rcov.tobytes()
    only = ctx.cost_square_error_batch(dense_grid, sq(), ctx.scan(r, ang), poses)
    assert only.tobytes() == ref.tobytes()


# ---------------------------------------------------------------- the walk
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_walk(ctx, dense_grid, scans, refs, variant, seed):
    """trace and summary: launcher defaults, max_iterations 6 / 1 / 0, no refinements"""
    r, ang, init = scans[seed]
    ref = refs[variant][seed]
    prm = abi.HCParams(*VARIANTS[variant])
    sc = ctx.scan(r, ang, REL)
    moves, costs = ctx.hc_sq_trace(dense_grid, prm, sq(), sc, init)
    assert len(moves) == ref.passes, (len(moves), ref.passes)
    assert moves.tolist() == ref.moves, (moves.tolist(), ref.moves)
    assert costs.tobytes() == np.array(ref.costs).tobytes(), (costs.tolist(), ref.costs)
    s = ctx.hc_sq_optimize_pose_query(dense_grid, prm, sq(), sc, init)
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
    s = ctx.hc_sq_optimize_pose_query(grid, prm, sq(), sc, init)
    assert (s.passes, s.num_iterations, s.num_refinements) == (5, 4, 5)
    assert (s.final_linear_step, s.final_angular_step) == (0.1 / 32, 0.1 / 32)
    assert_summary(s, ref, init)
    moves, costs = ctx.hc_sq_trace(grid, prm, sq(), sc, init)
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
    moves, costs = ctx.hc_sq_trace(dense_grid, prm, sq(), sc, init)
    assert moves.tolist() == ref.moves
    assert costs.tobytes() == np.array(ref.costs).tobytes()
    assert_summary(ctx.hc_sq_optimize_pose_query(dense_grid, prm, sq(), sc, init), ref, init, str(n_beams))
    # the cost entry takes the same path (its rows: 4 N or N doubles)
    check_costs(ctx, dense_map, dense_grid, r, ang, poses_around(init, 7, 3), live=False)


def test_batch_equals_lone_calls(ctx, world, dense_map, dense_grid, coarse_map, coarse_grid):
    """six matches of different beam counts over two maps of different
    resolution, different walk lengths: byte-identical to six lone calls and to
    the reference, and again after an unrelated correlative match on the same
    context"""
    maps = [(dense_map, dense_grid, RES), (coarse_map, coarse_grid, 0.1)]
    items = []
    for k in range(6):
        r, ang, init = draw(world, 20 + k, 361 if k % 2 == 0 else 1081)
        m, g, res = maps[1 if k in (2, 5) else 0]
        items.append((m, g, res, r, ang, init, ctx.scan(r, ang, REL)))
    prm = abi.HCParams(*DEFAULTS)
    ref = [reference(m, DEFAULTS, r, ang, init, res=res) for m, g, res, r, ang, init, sc in items]
    assert len({x.passes for x in ref}) >= 3 and all(sum(m >= 0 for m in x.moves) >= 1 for x in ref)

    def batch():
        return ctx.hc_sq_optimize_pose_batch([it[1] for it in items], prm, sq(), [it[6] for it in items],
                                             [it[5] for it in items])

    first = batch()
    lone = [ctx.hc_sq_optimize_pose_query(g, prm, sq(), sc, init) for m, g, res, r, ang, init, sc in items]
    for k in range(6):
        assert bytes(first[k]) == bytes(lone[k]), k
        assert_summary(first[k], ref[k], items[k][5], f"item{k}")
    # workspace history: an unrelated RTCSM match in between
    m, g, res, r, ang, init, sc = items[0]
    ctx.optimize_pose_query(g, abi.RtcsmParams(5, 0.6, 0.6, 0.4, 20.0), launcher_cost(), sc, init)
    again = batch()
    assert [bytes(x) for x in again] == [bytes(x) for x in first]


def test_batch_more_than_one_launch_and_global_rows(ctx, world, dense_grid, scans):
    """4100 matches (a second launch behind the first chunk of 4096) and a batch
    whose matches keep their term rows in global memory side by side: both
    equal the lone calls byte for byte"""
    prm = abi.HCParams(*DEFAULTS)
    scs = [ctx.scan(r, ang, REL) for r, ang, _ in scans]
    lone = [ctx.hc_sq_optimize_pose_query(dense_grid, prm, sq(), scs[k], scans[k][2]) for k in range(6)]
    assert len({bytes(x) for x in lone}) == 6
    n = 4100
    out = ctx.hc_sq_optimize_pose_batch(dense_grid, prm, sq(), [scs[k % 6] for k in range(n)],
                                        [scans[k % 6][2] for k in range(n)])
    assert all(bytes(out[k]) == bytes(lone[k % 6]) for k in range(n))
    r, ang, init = draw(world, 1, 8200)
    r2, ang2, init2 = draw(world, 2, 8200)
    big = [(ctx.scan(r, ang, REL), init), (scs[0], scans[0][2]), (ctx.scan(r2, ang2, REL), init2)]
    lone = [ctx.hc_sq_optimize_pose_query(dense_grid, prm, sq(), sc, p) for sc, p in big]
    out = ctx.hc_sq_optimize_pose_batch(dense_grid, prm, sq(), [sc for sc, _ in big], [p for _, p in big])
    assert [bytes(x) for x in out] == [bytes(x) for x in lone]
    assert bytes(lone[0]) != bytes(lone[2]) and lone[0].passes > 5


# ---------------------------------------------------------------- arguments
def test_argument_errors(ctx, dense_grid, scans):
    r, ang, init = scans[0]
    sc = ctx.scan(r, ang, REL)
    lib = ctx.lib
    nan, inf = float("nan"), float("inf")

    def query(prm, cost, pose):
        out = abi.HCSummary()
        return lib.lgs_hc_sq_optimize_pose_query(ctx.h, dense_grid.h, C.byref(abi.HCParams(*prm)),
                                                 C.byref(abi.CostSQParams(*cost)), sc.h, abi.Pose2D(*pose),
                                                 C.byref(out))

    assert query(DEFAULTS, SQ_RANGE, init) == abi.LGS_OK
    assert query((0.0, 0.1, 100, 5), SQ_RANGE, init) == LGS_ERR_INVALID_ARG
    assert query((0.1, 0.0, 100, 5), SQ_RANGE, init) == LGS_ERR_INVALID_ARG
    assert query((nan, 0.1, 100, 5), SQ_RANGE, init) == LGS_ERR_INVALID_ARG
    assert query(DEFAULTS, SQ_RANGE, (nan, init[1], init[2])) == LGS_ERR_INVALID_ARG
    assert query(DEFAULTS, SQ_RANGE, (init[0], init[1], inf)) == LGS_ERR_INVALID_ARG
    assert query((0.1, 0.1, 65537, 5), SQ_RANGE, init) == LGS_ERR_INVALID_ARG
    assert query(DEFAULTS, (nan, 20.0), init) == LGS_ERR_INVALID_ARG
    assert query(DEFAULTS, (0.01, inf), init) == LGS_ERR_INVALID_ARG
    # the trace returns the negated status
    mv, cs = (C.c_int * 4)(), (C.c_double * 4)()
    assert lib.lgs_hc_sq_trace(ctx.h, dense_grid.h, C.byref(abi.HCParams(0.0, 0.1, 100, 5)), C.byref(sq()), sc.h,
                               abi.Pose2D(*init), mv, cs, 4) == -LGS_ERR_INVALID_ARG
    # the cost entries: non-finite ranges and poses
    one = np.zeros(1)
    garr, sarr = (abi._P * 1)(dense_grid.h), (abi._P * 1)(sc.h)
    for cost, pose in (((nan, 20.0), init), (SQ_RANGE, (init[0], nan, init[2]))):
        assert lib.lgs_cost_square_error_batch(ctx.h, garr, C.byref(abi.CostSQParams(*cost)), sarr,
                                               (abi.Pose2D * 1)(abi.Pose2D(*pose)), 1, abi.dptr(one), None) == \
            LGS_ERR_INVALID_ARG
    # n = 0: OK, nothing written
    out = (abi.HCSummary * 1)()
    C.memset(out, 0x5A, C.sizeof(out))
    rc = lib.lgs_hc_sq_optimize_pose_batch(ctx.h, None, C.byref(abi.HCParams(*DEFAULTS)), C.byref(sq()), None, None, 0,
                                           out)
    assert rc == abi.LGS_OK and bytes(out) == b"\x5A" * C.sizeof(out)
    # the context still matches
    assert query(DEFAULTS, SQ_RANGE, init) == abi.LGS_OK


def test_angle_outside_the_sincos_domain_is_an_error(ctx, dense_grid, scans):
    """|theta + angle| >= 105414350 is outside the restated glibc sincos: the
    device raises its error flag and the call fails, as the greedy-endpoint walk does"""
    r, ang, init = scans[0]
    sc = ctx.scan(r, ang, REL)
    out = np.zeros(1)
    garr, sarr = (abi._P * 1)(dense_grid.h), (abi._P * 1)(sc.h)
    poses = (abi.Pose2D * 1)(abi.Pose2D(init[0], init[1], 2.0e8))
    assert ctx.lib.lgs_cost_square_error_batch(ctx.h, garr, C.byref(sq()), sarr, poses, 1, abi.dptr(out), None) == \
        LGS_ERR_INTERNAL
    hs = abi.HCSummary()
    rc = ctx.lib.lgs_hc_sq_optimize_pose_query(ctx.h, dense_grid.h, C.byref(abi.HCParams(*DEFAULTS)), C.byref(sq()),
                                               sc.h, abi.Pose2D(init[0], init[1], 2.0e8), C.byref(hs))
    assert rc == LGS_ERR_INTERNAL


# ---------------------------------------------------------------- the search matchers
def check_applied(ctx, map3, grid, r, ang, before, tag):
    """normalized cost and covariance are CostSquareError's at best_sensor_pose;
    every other byte of the summary is as the search entry point left it"""
    cells, mx, my = map3
    g, sc = ob.OGrid(cells, mx, my, RES), ob.OScan(r, ang, REL)
    after = ctx.summaries_apply_cost_sq(grid, sq(), [ctx.scan(r, ang, REL)], [before])[0]
    bp = before.best_sensor_pose.tuple()
    assert after.normalized_cost == sq_cost(g, sc, bp) / len(r), tag
    assert list(after.covariance) == sq_covariance(g, sc, bp), tag
    assert after.normalized_cost != before.normalized_cost and list(after.covariance) != list(before.covariance), tag
    restored = abi.RtcsmSummary.from_buffer_copy(bytes(after))
    restored.normalized_cost = before.normalized_cost
    for k in range(9):
        restored.covariance[k] = before.covariance[k]
    assert bytes(restored) == bytes(before), tag
    return after


def test_search_matchers_with_the_square_error_cost(ctx, dense_map, dense_grid, scans):
    """one correlative, one branch-and-bound and one grid-search summary from the
    existing entry points, found and not found"""
    r, ang, init = scans[1]
    sc = ctx.scan(r, ang, REL)
    cells, mx, my = dense_map
    sp = ob.lib().orc_compound(ob.Pose(*init), ob.Pose(*REL))
    rt = abi.RtcsmParams(5, 0.6, 0.6, 0.4, 20.0)
    found = ctx.optimize_pose_query(dense_grid, rt, launcher_cost(), sc, init)
    assert found.pose_found == 1
    check_applied(ctx, dense_map, dense_grid, r, ang, found, "rtcsm found")
    # a threshold no score reaches: the reference keeps the window corner it started from
    coarse = ctx.precompute_max(dense_grid, 5)
    lost = ctx.optimize_pose(dense_grid, coarse, rt, launcher_cost(), sc, init, 2.0)
    assert lost.pose_found == 0 and lost.best_sensor_pose.tuple() != (sp.x, sp.y, sp.theta)
    check_applied(ctx, dense_map, dense_grid, r, ang, lost, "rtcsm not found")

    bb = ctx.bb_optimize_pose_query(dense_grid, abi.BBParams(3, 0.8, 0.8, 0.3, 20.0, 0.01, 20.0), launcher_cost(), sc,
                                    init)
    assert bb.pose_found == 1
    check_applied(ctx, dense_map, dense_grid, r, ang, bb, "bb found")

    gp = abi.GSParams(0.6, 0.4, 0.1, 0.05, 0.05, 0.01, 0.01, 20.0)
    gs = ctx.gs_optimize_pose_query(dense_grid, gp, launcher_cost(), sc, init)
    assert gs.pose_found == 1
    check_applied(ctx, dense_map, dense_grid, r, ang, gs, "gs found")
    gl = ctx.gs_optimize_pose_batch(dense_grid, gp, launcher_cost(), [sc], [init], 2.0)[0]
    assert gl.pose_found == 0 and gl.best_sensor_pose.tuple() == (sp.x, sp.y, sp.theta)
    check_applied(ctx, dense_map, dense_grid, r, ang, gl, "gs not found")
