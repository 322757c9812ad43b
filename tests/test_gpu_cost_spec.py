"""GPU tests of the `_cost` entry points of the search matchers
(lgs_rtcsm_*_cost, lgs_bb_*_cost, lgs_gs_*_cost): a matcher constructed with
CostSquareError, the cost evaluated by the correlative pipeline's own stage
(k_cost_sq) or by one k_sq_cost_batch launch (bb, gs).

Reference: the oracle matcher's own best sensor pose, and orc_sq_cost /
orc_sq_covariance there (cost_spec_oracle).  Bar: every comparison is equality
of bytes; there is no tolerance.  The second reference is the path the new
entry points replace: the greedy-endpoint entry point followed by
lgs_summaries_apply_cost_sq, equal in every byte but the diagnostic counters
guard_hits and fixups.
"""
import ctypes as C

import numpy as np
import pytest

import cost_spec_oracle as cso
import test_loopbatch_cpu as small
from conftest import launcher_cost
from hc_sq_oracle import SQ_RANGE
from lgs_amd import abi, scene
from test_gpu_gs import draw
from test_gpu_rtcsm import build_map

pytestmark = pytest.mark.gpu
LGS_ERR_INVALID_ARG = 1
LGS_ERR_INTERNAL = 5
REL = (0.1, -0.05, 0.02)
RES = 0.05
RT = (5, 0.6, 0.6, 0.4, 20.0)
RT_SMALL = (5, 0.19, 0.19, 0.4, 20.0)     # winX = winY = 2: 2 win < LowRes, one coarse block per angle
BB = (3, 0.8, 0.8, 0.3, 20.0, 0.01, 20.0)
GS = (0.6, 0.4, 0.1, 0.05, 0.05, 0.01, 0.01, 20.0)


def sq():
    return abi.CostSQParams(*SQ_RANGE)


@pytest.fixture(scope="module")
def dense_map(world):
    return build_map(world, 300, RES, 100, scene.arc_poses(24), n_beams=1081)


@pytest.fixture(scope="module")
def other_map(world):
    """a second 300 x 300 room map (fewer scans: other cell values, same geometry)"""
    return build_map(world, 300, RES, 100, scene.arc_poses(7), n_beams=541)


@pytest.fixture(scope="module")
def dense_grid(ctx, dense_map):
    return ctx.grid_from_array(*dense_map, RES)


@pytest.fixture(scope="module")
def other_grid(ctx, other_map):
    return ctx.grid_from_array(*other_map, RES)


@pytest.fixture(scope="module")
def scans(world):
    return [draw(world, seed, 361) for seed in range(3)]


def chained(ctx, grid, sc, summary):
    """what the greedy-endpoint entry point's summary becomes under lgs_summaries_apply_cost_sq"""
    return ctx.summaries_apply_cost_sq(grid, sq(), [sc], [summary])[0]


def check(new, ref, old, grid, ctx, sc, tag):
    """new: the `_cost` summary; ref: the oracle; old: the greedy-endpoint entry point's summary"""
    cso.assert_sq(new, ref, tag)
    assert new.pose_found == ref.s.pose_found and new.score_max == ref.s.score_max, tag
    assert cso.same_but_counters(new, chained(ctx, grid, sc, old)), tag
    # the comparison is not vacuous: the greedy-endpoint values are others
    assert new.normalized_cost != old.normalized_cost and list(new.covariance) != list(old.covariance), tag


# ---------------------------------------------------------------- 1. the three matchers
def test_correlative_matcher_found_and_not_found(ctx, dense_map, dense_grid, scans):
    r, ang, init = scans[1]
    sc = ctx.scan(r, ang, REL)
    rt = abi.RtcsmParams(*RT)
    new = ctx.optimize_pose_query(dense_grid, rt, sq(), sc, init)
    ref = cso.ref_rtcsm(dense_map, RES, RT, r, ang, init, rel=REL)
    assert new.pose_found == 1
    check(new, ref, ctx.optimize_pose_query(dense_grid, rt, launcher_cost(), sc, init), dense_grid, ctx, sc, "found")
    # a threshold no score reaches, through the coarse-map overload: the window corner
    coarse = ctx.precompute_max(dense_grid, 5)
    lost = ctx.optimize_pose(dense_grid, coarse, rt, sq(), sc, init, 2.0)
    ref = cso.ref_rtcsm(dense_map, RES, RT, r, ang, init, thr=2.0, rel=REL)
    assert lost.pose_found == 0
    check(lost, ref, ctx.optimize_pose(dense_grid, coarse, rt, launcher_cost(), sc, init, 2.0), dense_grid, ctx, sc,
          "not found")
    # the loop overload over several scans
    items = [(ctx.scan(r, ang, REL), r, ang, init) for r, ang, init in scans]
    outs = ctx.optimize_pose_batch(dense_grid, coarse, rt, sq(), [it[0] for it in items], [it[3] for it in items], 0.5)
    olds = ctx.optimize_pose_batch(dense_grid, coarse, rt, launcher_cost(), [it[0] for it in items],
                                   [it[3] for it in items], 0.5)
    for k, (s, r, ang, init) in enumerate(items):
        check(outs[k], cso.ref_rtcsm(dense_map, RES, RT, r, ang, init, thr=0.5, rel=REL), olds[k], dense_grid, ctx, s,
              f"loop overload {k}")


def test_branch_and_bound_matcher_found_and_not_found(ctx, dense_map, dense_grid, scans):
    r, ang, init = scans[1]
    sc = ctx.scan(r, ang, REL)
    P = abi.BBParams(*BB)
    new = ctx.bb_optimize_pose_query(dense_grid, P, sq(), sc, init)
    assert new.pose_found == 1
    check(new, cso.ref_bb(dense_map, RES, BB, r, ang, init, rel=REL),
          ctx.bb_optimize_pose_query(dense_grid, P, launcher_cost(), sc, init), dense_grid, ctx, sc, "bb found")
    pyr = ctx.precompute_pyramid(dense_grid, BB[0])
    lost = ctx.bb_optimize_pose_batch(dense_grid, pyr, P, sq(), [sc], [init], 2.0)[0]
    assert lost.pose_found == 0
    check(lost, cso.ref_bb(dense_map, RES, BB, r, ang, init, thr=2.0, rel=REL),
          ctx.bb_optimize_pose_batch(dense_grid, pyr, P, launcher_cost(), [sc], [init], 2.0)[0], dense_grid, ctx, sc,
          "bb not found")


def test_grid_search_matcher_found_and_not_found(ctx, dense_map, dense_grid, scans):
    r, ang, init = scans[1]
    sc = ctx.scan(r, ang, REL)
    P = abi.GSParams(*GS)
    new = ctx.gs_optimize_pose_query(dense_grid, P, sq(), sc, init)
    assert new.pose_found == 1
    check(new, cso.ref_gs(dense_map, RES, GS, r, ang, init, rel=REL),
          ctx.gs_optimize_pose_query(dense_grid, P, launcher_cost(), sc, init), dense_grid, ctx, sc, "gs found")
    lost = ctx.gs_optimize_pose_batch(dense_grid, P, sq(), [sc], [init], 2.0)[0]
    assert lost.pose_found == 0
    check(lost, cso.ref_gs(dense_map, RES, GS, r, ang, init, nthr=2.0, rel=REL),
          ctx.gs_optimize_pose_batch(dense_grid, P, launcher_cost(), [sc], [init], 2.0)[0], dense_grid, ctx, sc,
          "gs not found")


# ---------------------------------------------------------------- 2. kind == 0
def test_kind_zero_returns_the_existing_entry_points_bytes(ctx, dense_grid, scans):
    r, ang, init = scans[0]
    sc = ctx.scan(r, ang, REL)
    ge = launcher_cost()
    spec = abi.cost_spec(ge)
    assert spec.kind == abi.LGS_COST_GREEDY_ENDPOINT
    rt, bb, gs = abi.RtcsmParams(*RT), abi.BBParams(*BB), abi.GSParams(*GS)
    assert bytes(ctx.optimize_pose_query(dense_grid, rt, spec, sc, init)) == \
        bytes(ctx.optimize_pose_query(dense_grid, rt, ge, sc, init))
    assert bytes(ctx.optimize_pose_query_batch(dense_grid, rt, spec, [sc, sc], [init, init])[1]) == \
        bytes(ctx.optimize_pose_query_batch(dense_grid, rt, ge, [sc, sc], [init, init])[1])
    assert bytes(ctx.bb_optimize_pose_query(dense_grid, bb, spec, sc, init)) == \
        bytes(ctx.bb_optimize_pose_query(dense_grid, bb, ge, sc, init))
    assert bytes(ctx.gs_optimize_pose_query(dense_grid, gs, spec, sc, init)) == \
        bytes(ctx.gs_optimize_pose_query(dense_grid, gs, ge, sc, init))
    # the three detectors
    maps, cands = small.make_problem()
    grids = [ctx.grid_from_array(m.cells, m.min_x, m.min_y, m.res) for m in maps]
    queries = [(grids[q], None, maps[q].node_pose, maps[q].node_index, 4 * q, 4) for q in range(len(maps))]
    cl = [(ctx.scan(c.ranges, c.angles), c.pose, c.node_index) for c in cands]
    n = len(cl) * 176
    lp = abi.RtcsmParams(*small.PARAMS)
    assert bytes(ctx.loop_detect(lp, spec, small.THR, queries, cl))[:n] == \
        bytes(ctx.loop_detect(lp, ge, small.THR, queries, cl))[:n]
    bbl = abi.BBParams(4, 1.0, 1.0, 0.6, 20.0, 0.01, 20.0)
    assert bytes(ctx.loop_detect_bb(bbl, spec, 0.6, queries, cl))[:n] == \
        bytes(ctx.loop_detect_bb(bbl, ge, 0.6, queries, cl))[:n]
    assert bytes(ctx.loop_detect_gs(gs, spec, 0.5, queries, cl))[:n] == \
        bytes(ctx.loop_detect_gs(gs, ge, 0.5, queries, cl))[:n]


# ---------------------------------------------------------------- 3. the correlative paths
@pytest.fixture(scope="module")
def path_case(dense_map, scans):
    """one query and its oracle summaries for the two windows, computed once"""
    r, ang, init = scans[2]
    return (r, ang, init, cso.ref_rtcsm(dense_map, RES, RT, r, ang, init, rel=REL),
            cso.ref_rtcsm(dense_map, RES, RT_SMALL, r, ang, init, rel=REL))


def run_both(ctx, grid, params, sc, init):
    P = abi.RtcsmParams(*params)
    return ctx.optimize_pose_query(grid, P, sq(), sc, init), ctx.optimize_pose_query(grid, P, launcher_cost(), sc, init)


@pytest.mark.parametrize("option,value,params", [
    (None, 0, RT),                                  # the lone call
    (abi.LGS_OPT_SMALL_WINDOW, 1, RT_SMALL),        # k_match_small
    (abi.LGS_OPT_SMALL_WINDOW, 0, RT_SMALL),        # the same window on the general path
    (abi.LGS_OPT_FORCE_DENSE, 1, RT),
    (abi.LGS_OPT_POST_RECORDS, 0, RT),
    (abi.LGS_OPT_POISON_WS, 1, RT),
    (abi.LGS_OPT_POISON_WS, 1, RT_SMALL),
])
def test_correlative_paths(ctx, dense_grid, path_case, option, value, params):
    r, ang, init, ref_wide, ref_small = path_case
    ref = ref_wide if params == RT else ref_small
    sc = ctx.scan(r, ang, REL)
    defaults = {abi.LGS_OPT_SMALL_WINDOW: 1, abi.LGS_OPT_FORCE_DENSE: 0, abi.LGS_OPT_POST_RECORDS: 1,
                abi.LGS_OPT_POISON_WS: 0}
    try:
        ctx.set_option(abi.LGS_OPT_PROFILE, 1)
        ctx.reset_stats()
        if option is not None:
            ctx.set_option(option, value)
        new = ctx.optimize_pose_query(dense_grid, abi.RtcsmParams(*params), sq(), sc, init)
        stats = ctx.kernel_stats()
        old = ctx.optimize_pose_query(dense_grid, abi.RtcsmParams(*params), launcher_cost(), sc, init)
    finally:
        ctx.set_option(abi.LGS_OPT_PROFILE, 0)
        if option is not None:
            ctx.set_option(option, defaults[option])
    check(new, ref, old, dense_grid, ctx, sc, f"option {option}={value}")
    small_path = params == RT_SMALL and not (option == abi.LGS_OPT_SMALL_WINDOW and value == 0)
    assert ("k_match_small" in stats) == small_path, stats.keys()
    assert "k_cost" not in stats and stats["k_cost_sq"]["launches"] == 1, stats.keys()


@pytest.mark.parametrize("params", [RT, RT_SMALL])
def test_correlative_guard_fixup_reruns(ctx, dense_grid, path_case, params):
    """LGS_OPT_INJECT_INDEX corrupts every guarded projection: the fix-up rerun's
    cost stage is the square-error one too"""
    r, ang, init, ref_wide, ref_small = path_case
    ref = ref_wide if params == RT else ref_small
    sc = ctx.scan(r, ang, REL)
    try:
        ctx.set_option(abi.LGS_OPT_GUARD_EPS, 0.02)
        ctx.set_option(abi.LGS_OPT_INJECT_INDEX, 1)
        ctx.set_option(abi.LGS_OPT_PROFILE, 1)
        ctx.reset_stats()
        new = ctx.optimize_pose_query(dense_grid, abi.RtcsmParams(*params), sq(), sc, init)
        stats = ctx.kernel_stats()
        old = ctx.optimize_pose_query(dense_grid, abi.RtcsmParams(*params), launcher_cost(), sc, init)
    finally:
        ctx.set_option(abi.LGS_OPT_PROFILE, 0)
        ctx.set_option(abi.LGS_OPT_GUARD_EPS, 1e-9)
        ctx.set_option(abi.LGS_OPT_INJECT_INDEX, 0)
    assert new.fixups > 0 and new.guard_hits > 0, (new.fixups, new.guard_hits)
    assert "k_cost" not in stats and stats["k_cost_sq"]["launches"] == 2, stats   # the first run and the rerun
    check(new, ref, old, dense_grid, ctx, sc, "inject")


def test_correlative_batch_of_two_chunks(ctx, world, dense_map, dense_grid, other_map, other_grid):
    """70 queries: two chunks (64 + 6) on the two buffer banks, scans of 361 and
    1081 beams mixed, two distinct maps; and what LGS_OPT_PROFILE counts: no
    k_cost launch, one k_cost_sq launch per chunk (kind 0: as today)"""
    base = []
    for k in range(5):
        r, ang, init = draw(world, 30 + k, 361 if k % 2 == 0 else 1081)
        m, g = (other_map, other_grid) if k in (1, 4) else (dense_map, dense_grid)
        base.append((m, g, r, ang, init, ctx.scan(r, ang, REL), cso.ref_rtcsm(m, RES, RT, r, ang, init, rel=REL)))
    items = [base[(3 * k) % 5] for k in range(70)]
    P = abi.RtcsmParams(*RT)
    grids, scs, inits = [it[1] for it in items], [it[5] for it in items], [it[4] for it in items]
    try:
        ctx.set_option(abi.LGS_OPT_PROFILE, 1)
        ctx.reset_stats()
        new = ctx.optimize_pose_query_batch(grids, P, sq(), scs, inits)
        stats = ctx.kernel_stats()
        ctx.reset_stats()
        old = ctx.optimize_pose_query_batch(grids, P, launcher_cost(), scs, inits)
        stats0 = ctx.kernel_stats()
    finally:
        ctx.set_option(abi.LGS_OPT_PROFILE, 0)
    assert "k_cost" not in stats and stats["k_cost_sq"]["launches"] == 2, stats.keys()
    assert "k_cost_sq" not in stats0 and stats0["k_cost"]["launches"] >= 2, stats0.keys()
    assert {k: v["launches"] for k, v in stats.items() if k != "k_cost_sq"} == \
        {k: v["launches"] for k, v in stats0.items() if k != "k_cost"}
    after = ctx.summaries_apply_cost_sq(grids, sq(), scs, old)
    for k, it in enumerate(items):
        cso.assert_sq(new[k], it[6], f"item {k}")
        assert cso.same_but_counters(new[k], after[k]), k
    assert len({bytes(s) for s in new}) == 5
    # a lone call gives the batch's result (the block counters depend on the batch's pruning)
    lone = ctx.optimize_pose_query(grids[1], P, sq(), scs[1], inits[1])
    cso.assert_sq(lone, items[1][6], "lone")
    assert (lone.pose_found, lone.score_max, list(lone.best_win)) == \
        (new[1].pose_found, new[1].score_max, list(new[1].best_win))


# ---------------------------------------------------------------- 4. edge shapes of the cost stage
def test_one_beam_scan(ctx, dense_map, dense_grid, scans):
    r, ang, init = scans[0]
    r1, a1 = r[180:181].copy(), ang[180:181].copy()
    sc = ctx.scan(r1, a1, REL)
    new = ctx.optimize_pose_query(dense_grid, abi.RtcsmParams(*RT_SMALL), sq(), sc, init)
    cso.assert_sq(new, cso.ref_rtcsm(dense_map, RES, RT_SMALL, r1, a1, init, rel=REL), "one beam")


def test_every_beam_outside_the_usable_range(ctx, dense_map, dense_grid, scans):
    """CostSquareError(0.01, 0.02) filters every beam: the chains stay +0.0"""
    r, ang, init = scans[0]
    assert (r > 0.02).all()
    sc = ctx.scan(r, ang, REL)
    new = ctx.optimize_pose_query(dense_grid, abi.RtcsmParams(*RT_SMALL), abi.CostSQParams(0.01, 0.02), sc, init)
    cso.assert_sq(new, cso.ref_rtcsm(dense_map, RES, RT_SMALL, r, ang, init, rel=REL, usable=(0.01, 0.02)), "filtered")
    assert new.normalized_cost == 0.0 and np.array(list(new.covariance)).tobytes() == \
        np.array([0.01, 0, 0, 0, 0.01, 0, 0, 0, 0.01], dtype=np.float64).tobytes()


def test_more_beams_than_the_lds_rows_hold(ctx, world, dense_map, dense_grid):
    """8200 beams: 4 x 8200 doubles exceed the stage's 144 KiB of LDS rows, the
    terms go through the item's global rows; 4000 beams: LDS beyond the 64 KiB default"""
    for n_beams in (8200, 4000):
        r, ang, init = draw(world, 1, n_beams)
        sc = ctx.scan(r, ang, REL)
        params = (5, 0.19, 0.19, 0.1, 20.0)
        new = ctx.optimize_pose_query(dense_grid, abi.RtcsmParams(*params), sq(), sc, init)
        cso.assert_sq(new, cso.ref_rtcsm(dense_map, RES, params, r, ang, init, rel=REL), str(n_beams))
        old = ctx.optimize_pose_query(dense_grid, abi.RtcsmParams(*params), launcher_cost(), sc, init)
        assert cso.same_but_counters(new, chained(ctx, dense_grid, sc, old))


def test_footprint_leaves_a_tiny_map(ctx):
    """a 3 x 2 map and a scan at its edge: every bicubic index clamps"""
    rng = np.random.default_rng(5)
    tiny = (rng.uniform(0.05, 0.95, (2, 3)), 0.0, 0.0)
    grid = ctx.grid_from_array(*tiny, RES)
    ang = scene.beam_angles(181)
    r = rng.uniform(0.05, 0.4, size=181)
    init = (0.05, 0.05, 0.1)
    params = (5, 0.2, 0.2, 0.3, 20.0)
    new = ctx.optimize_pose_query(grid, abi.RtcsmParams(*params), sq(), ctx.scan(r, ang), init)
    ref = cso.ref_rtcsm(tiny, RES, params, r, ang, init)
    cso.assert_sq(new, ref, "tiny map")
    assert 0.0 < new.normalized_cost < 1.0


def test_all_unknown_map(ctx, scans):
    """every cell unknown: S = 0, every valid beam's term is 1, the gradient 0"""
    empty = (np.zeros((120, 130)), -3.0, -3.25)
    grid = ctx.grid_from_array(*empty, RES)
    r, ang, init = scans[1]
    new = ctx.optimize_pose_query(grid, abi.RtcsmParams(*RT_SMALL), sq(), ctx.scan(r, ang, REL), init)
    cso.assert_sq(new, cso.ref_rtcsm(empty, RES, RT_SMALL, r, ang, init, rel=REL), "unknown map")
    assert new.pose_found == 0 and new.normalized_cost == float(((r > 0.01) & (r < 20.0)).sum()) / len(r)


# ---------------------------------------------------------------- 6. errors
def test_errors(ctx, dense_grid, scans):
    r, ang, init = scans[0]
    sc = ctx.scan(r, ang, REL)
    rt, bb, gs = abi.RtcsmParams(*RT_SMALL), abi.BBParams(*BB), abi.GSParams(*GS)
    bad_kind = abi.CostSpec(7, launcher_cost(), sq())
    nan_range = abi.CostSQParams(float("nan"), 20.0)
    for cost in (bad_kind, nan_range):
        for call in (lambda c: ctx.optimize_pose_query(dense_grid, rt, c, sc, init),
                     lambda c: ctx.bb_optimize_pose_query(dense_grid, bb, c, sc, init),
                     lambda c: ctx.gs_optimize_pose_query(dense_grid, gs, c, sc, init),
                     lambda c: ctx.loop_detect(rt, c, 0.5, [(dense_grid, None, (0, 0, 0), 0, 0, 1)], [(sc, init, 1)])):
            with pytest.raises(abi.LgsError) as e:
                call(cost)
            assert e.value.status == LGS_ERR_INVALID_ARG
    # an angle outside the restated sincos domain: LGS_ERR_INTERNAL, the caller's buffer untouched
    far = (init[0], init[1], 2.0e8)
    spec = abi.cost_spec(sq())
    for name, fn in (
            ("rtcsm", lambda out: ctx.lib.lgs_rtcsm_optimize_pose_query_cost(
                ctx.h, dense_grid.h, C.byref(rt), C.byref(spec), sc.h, abi.Pose2D(*far), C.byref(out))),
            ("bb", lambda out: ctx.lib.lgs_bb_optimize_pose_query_cost(
                ctx.h, dense_grid.h, C.byref(bb), C.byref(spec), sc.h, abi.Pose2D(*far), C.byref(out))),
            ("gs", lambda out: ctx.lib.lgs_gs_optimize_pose_query_cost(
                ctx.h, dense_grid.h, C.byref(gs), C.byref(spec), sc.h, abi.Pose2D(*far), C.byref(out)))):
        out = abi.RtcsmSummary()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        assert fn(out) == LGS_ERR_INTERNAL, name
        assert bytes(out) == b"\x5A" * C.sizeof(out), name
        with pytest.raises(abi.LgsError) as e:
            {"rtcsm": lambda: ctx.optimize_pose_query(dense_grid, rt, sq(), sc, far),
             "bb": lambda: ctx.bb_optimize_pose_query(dense_grid, bb, sq(), sc, far),
             "gs": lambda: ctx.gs_optimize_pose_query(dense_grid, gs, sq(), sc, far)}[name]()
        assert e.value.status == LGS_ERR_INTERNAL
        # the context works on the next call
        again = ctx.optimize_pose_query(dense_grid, rt, sq(), sc, init)
        assert again.normalized_cost > 0.0
