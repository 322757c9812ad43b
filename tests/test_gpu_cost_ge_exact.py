"""GPU tests of LGS_COST_GREEDY_ENDPOINT_EXACT through the `_cost` entry points of
the search matchers and of the batched evaluator behind them
(lgs_cost_ge_exact_batch, lgs_summaries_apply_cost_ge_exact): the correlative
pipeline's stage k_cost_gx, one k_ge_cost_batch launch for bb and gs.

Reference: the oracle matcher's own summary as it stands -- its normalized_cost
and covariance are orc_cost_ge_cost / NumOfScans() and orc_cost_ge_covariance
at its best sensor pose, found or not.  Bar: every comparison is equality of
bytes; there is no tolerance.  The second reference is kind 0: a kind-2 summary
equals the kind-0 summary in every byte but normalized_cost, covariance and the
diagnostic counters guard_hits and fixups.
"""
import ctypes as C

import numpy as np
import pytest

import cost_spec_oracle as cso
import ge_exact_oracle as gx
from conftest import launcher_cost
from ge_exact_oracle import REL, RES
from lgs_amd import abi, scene
from test_gpu_gs import draw
from test_gpu_rtcsm import build_map

pytestmark = pytest.mark.gpu
LGS_ERR_INVALID_ARG = 1
LGS_ERR_INTERNAL = 5
RT = (5, 0.6, 0.6, 0.4, 20.0)
RT_SMALL = (5, 0.19, 0.19, 0.4, 20.0)     # winX = winY = 2: 2 win < LowRes, one coarse block per angle
BB = (3, 0.8, 0.8, 0.3, 20.0, 0.01, 20.0)
GS = (0.6, 0.4, 0.1, 0.05, 0.05, 0.01, 0.01, 20.0)


def exact():
    return gx.exact_spec()


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


def chained(ctx, grid, sc, summary, cost=None):
    """what a kind-0 summary becomes under lgs_summaries_apply_cost_ge_exact"""
    return ctx.summaries_apply_cost_ge_exact(grid, cost or launcher_cost(), [sc], [summary])[0]


def check(new, ref, old, grid, ctx, sc, tag):
    """new: the kind-2 summary; ref: the oracle; old: the kind-0 summary"""
    gx.assert_gx_ref(new, ref, tag)
    assert new.pose_found == ref.s.pose_found and new.score_max == ref.s.score_max, tag
    assert cso.same_but_counters(new, chained(ctx, grid, sc, old)), tag
    # kind 0 holds the same two fields to 1e-5
    assert abs(new.normalized_cost - old.normalized_cost) <= 1e-5, tag
    assert np.allclose(list(new.covariance), list(old.covariance), rtol=0, atol=1e-5), tag


# ---------------------------------------------------------------- 1. the three matchers
def test_correlative_matcher_found_and_not_found(ctx, dense_map, dense_grid, scans):
    r, ang, init = scans[1]
    sc = ctx.scan(r, ang, REL)
    rt = abi.RtcsmParams(*RT)
    new = ctx.optimize_pose_query(dense_grid, rt, exact(), sc, init)
    ref = cso.ref_rtcsm(dense_map, RES, RT, r, ang, init, rel=REL)
    assert new.pose_found == 1
    check(new, ref, ctx.optimize_pose_query(dense_grid, rt, launcher_cost(), sc, init), dense_grid, ctx, sc, "found")
    # a threshold no score reaches, through the coarse-map overload: the window corner
    coarse = ctx.precompute_max(dense_grid, 5)
    lost = ctx.optimize_pose(dense_grid, coarse, rt, exact(), sc, init, 2.0)
    ref = cso.ref_rtcsm(dense_map, RES, RT, r, ang, init, thr=2.0, rel=REL)
    assert lost.pose_found == 0
    check(lost, ref, ctx.optimize_pose(dense_grid, coarse, rt, launcher_cost(), sc, init, 2.0), dense_grid, ctx, sc,
          "not found")
    # the loop overload over several scans
    items = [(ctx.scan(r, ang, REL), r, ang, init) for r, ang, init in scans]
    outs = ctx.optimize_pose_batch(dense_grid, coarse, rt, exact(), [it[0] for it in items], [it[3] for it in items],
                                   0.5)
    olds = ctx.optimize_pose_batch(dense_grid, coarse, rt, launcher_cost(), [it[0] for it in items],
                                   [it[3] for it in items], 0.5)
    for k, (s, r, ang, init) in enumerate(items):
        check(outs[k], cso.ref_rtcsm(dense_map, RES, RT, r, ang, init, thr=0.5, rel=REL), olds[k], dense_grid, ctx, s,
              f"loop overload {k}")


def test_branch_and_bound_matcher_found_and_not_found(ctx, dense_map, dense_grid, scans):
    r, ang, init = scans[1]
    sc = ctx.scan(r, ang, REL)
    P = abi.BBParams(*BB)
    new = ctx.bb_optimize_pose_query(dense_grid, P, exact(), sc, init)
    assert new.pose_found == 1
    check(new, cso.ref_bb(dense_map, RES, BB, r, ang, init, rel=REL),
          ctx.bb_optimize_pose_query(dense_grid, P, launcher_cost(), sc, init), dense_grid, ctx, sc, "bb found")
    pyr = ctx.precompute_pyramid(dense_grid, BB[0])
    lost = ctx.bb_optimize_pose_batch(dense_grid, pyr, P, exact(), [sc], [init], 2.0)[0]
    assert lost.pose_found == 0
    check(lost, cso.ref_bb(dense_map, RES, BB, r, ang, init, thr=2.0, rel=REL),
          ctx.bb_optimize_pose_batch(dense_grid, pyr, P, launcher_cost(), [sc], [init], 2.0)[0], dense_grid, ctx, sc,
          "bb not found")


def test_grid_search_matcher_found_and_not_found(ctx, dense_map, dense_grid, scans):
    r, ang, init = scans[1]
    sc = ctx.scan(r, ang, REL)
    P = abi.GSParams(*GS)
    new = ctx.gs_optimize_pose_query(dense_grid, P, exact(), sc, init)
    assert new.pose_found == 1
    check(new, cso.ref_gs(dense_map, RES, GS, r, ang, init, rel=REL),
          ctx.gs_optimize_pose_query(dense_grid, P, launcher_cost(), sc, init), dense_grid, ctx, sc, "gs found")
    lost = ctx.gs_optimize_pose_batch(dense_grid, P, exact(), [sc], [init], 2.0)[0]
    assert lost.pose_found == 0
    check(lost, cso.ref_gs(dense_map, RES, GS, r, ang, init, nthr=2.0, rel=REL),
          ctx.gs_optimize_pose_batch(dense_grid, P, launcher_cost(), [sc], [init], 2.0)[0], dense_grid, ctx, sc,
          "gs not found")


# ---------------------------------------------------------------- 2. kind == 0 is untouched
def test_kind_zero_still_returns_the_namesakes_bytes(ctx, dense_grid, scans):
    r, ang, init = scans[0]
    sc = ctx.scan(r, ang, REL)
    ge = launcher_cost()
    spec = abi.cost_spec(ge)
    assert spec.kind == abi.LGS_COST_GREEDY_ENDPOINT
    rt, bb, gs = abi.RtcsmParams(*RT), abi.BBParams(*BB), abi.GSParams(*GS)
    assert bytes(ctx.optimize_pose_query(dense_grid, rt, spec, sc, init)) == \
        bytes(ctx.optimize_pose_query(dense_grid, rt, ge, sc, init))
    assert bytes(ctx.bb_optimize_pose_query(dense_grid, bb, spec, sc, init)) == \
        bytes(ctx.bb_optimize_pose_query(dense_grid, bb, ge, sc, init))
    assert bytes(ctx.gs_optimize_pose_query(dense_grid, gs, spec, sc, init)) == \
        bytes(ctx.gs_optimize_pose_query(dense_grid, gs, ge, sc, init))


# ---------------------------------------------------------------- 3. the correlative paths
@pytest.fixture(scope="module")
def path_case(dense_map, scans):
    """one query and its oracle summaries for the two windows, computed once"""
    r, ang, init = scans[2]
    return (r, ang, init, cso.ref_rtcsm(dense_map, RES, RT, r, ang, init, rel=REL),
            cso.ref_rtcsm(dense_map, RES, RT_SMALL, r, ang, init, rel=REL))


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
        new = ctx.optimize_pose_query(dense_grid, abi.RtcsmParams(*params), exact(), sc, init)
        stats = ctx.kernel_stats()
        old = ctx.optimize_pose_query(dense_grid, abi.RtcsmParams(*params), launcher_cost(), sc, init)
    finally:
        ctx.set_option(abi.LGS_OPT_PROFILE, 0)
        if option is not None:
            ctx.set_option(option, defaults[option])
    check(new, ref, old, dense_grid, ctx, sc, f"option {option}={value}")
    small_path = params == RT_SMALL and not (option == abi.LGS_OPT_SMALL_WINDOW and value == 0)
    assert ("k_match_small" in stats) == small_path, stats.keys()
    assert "k_cost" not in stats and stats["k_cost_gx"]["launches"] == 1, stats.keys()


@pytest.mark.parametrize("params", [RT, RT_SMALL])
def test_correlative_guard_fixup_reruns(ctx, dense_grid, path_case, params):
    """LGS_OPT_INJECT_INDEX corrupts every guarded projection: the slow-path
    rerun's cost stage is the exact one too, and nothing is patched for it"""
    r, ang, init, ref_wide, ref_small = path_case
    ref = ref_wide if params == RT else ref_small
    sc = ctx.scan(r, ang, REL)
    try:
        ctx.set_option(abi.LGS_OPT_GUARD_EPS, 0.02)
        ctx.set_option(abi.LGS_OPT_INJECT_INDEX, 1)
        ctx.set_option(abi.LGS_OPT_PROFILE, 1)
        ctx.reset_stats()
        new = ctx.optimize_pose_query(dense_grid, abi.RtcsmParams(*params), exact(), sc, init)
        stats = ctx.kernel_stats()
    finally:
        ctx.set_option(abi.LGS_OPT_PROFILE, 0)
        ctx.set_option(abi.LGS_OPT_GUARD_EPS, 1e-9)
        ctx.set_option(abi.LGS_OPT_INJECT_INDEX, 0)
    assert new.fixups > 0 and new.guard_hits > 0, (new.fixups, new.guard_hits)
    assert "k_cost" not in stats and stats["k_cost_gx"]["launches"] == 2, stats   # the first run and the rerun
    gx.assert_gx_ref(new, ref, "inject")
    assert new.pose_found == ref.s.pose_found and new.score_max == ref.s.score_max


def test_correlative_batch_of_two_chunks(ctx, world, dense_map, dense_grid, other_map, other_grid):
    """70 queries: two chunks (64 + 6) on the two buffer banks, scans of 361 and
    1081 beams mixed, two distinct maps; one k_cost_gx launch per chunk in
    k_cost's place, every other launch count as kind 0's"""
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
        new = ctx.optimize_pose_query_batch(grids, P, exact(), scs, inits)
        stats = ctx.kernel_stats()
        ctx.reset_stats()
        old = ctx.optimize_pose_query_batch(grids, P, launcher_cost(), scs, inits)
        stats0 = ctx.kernel_stats()
    finally:
        ctx.set_option(abi.LGS_OPT_PROFILE, 0)
    assert "k_cost" not in stats and stats["k_cost_gx"]["launches"] == 2, stats.keys()
    assert "k_cost_gx" not in stats0 and stats0["k_cost"]["launches"] >= 2, stats0.keys()
    after = ctx.summaries_apply_cost_ge_exact(grids, launcher_cost(), scs, old)
    for k, it in enumerate(items):
        gx.assert_gx_ref(new[k], it[6], f"item {k}")
        assert cso.same_but_counters(new[k], after[k]), k
    assert len({bytes(s) for s in new}) == 5
    # a lone call gives the batch's result (the block counters depend on the batch's pruning)
    lone = ctx.optimize_pose_query(grids[1], P, exact(), scs[1], inits[1])
    gx.assert_gx_ref(lone, items[1][6], "lone")
    assert (lone.pose_found, lone.score_max, list(lone.best_win)) == \
        (new[1].pose_found, new[1].score_max, list(new[1].best_win))


# ---------------------------------------------------------------- 4. edge shapes of the cost stage
@pytest.mark.parametrize("first,count", [(180, 1), (100, 37)])
def test_short_scans(ctx, dense_map, dense_grid, scans, first, count):
    """one beam, and 37 beams: less than a wave, and an odd tail of the chain's groups of eight"""
    r, ang, init = scans[0]
    r1, a1 = r[first:first + count].copy(), ang[first:first + count].copy()
    sc = ctx.scan(r1, a1, REL)
    for params in ((RT_SMALL,) if count == 1 else (RT_SMALL, RT)):
        new = ctx.optimize_pose_query(dense_grid, abi.RtcsmParams(*params), exact(), sc, init)
        gx.assert_gx_ref(new, cso.ref_rtcsm(dense_map, RES, params, r1, a1, init, rel=REL), f"{count} beams")
    bb = ctx.bb_optimize_pose_query(dense_grid, abi.BBParams(*BB), exact(), sc, init)
    gx.assert_gx_ref(bb, cso.ref_bb(dense_map, RES, BB, r1, a1, init, rel=REL), f"bb {count} beams")


def test_every_beam_outside_the_usable_range(ctx, dense_map, dense_grid, scans):
    """CostGreedyEndpoint with usable ranges (0.01, 0.02) filters every beam: the chains stay 0"""
    r, ang, init = scans[0]
    assert (r > 0.02).all()
    vals = (0.01, 0.02) + gx.LAUNCHER[2:]
    sc = ctx.scan(r, ang, REL)
    for name, new, ref in (
            ("rtcsm", ctx.optimize_pose_query(dense_grid, abi.RtcsmParams(*RT_SMALL), gx.exact_spec(vals), sc, init),
             cso.ref_rtcsm(dense_map, RES, RT_SMALL, r, ang, init, rel=REL)),
            ("gs", ctx.gs_optimize_pose_query(dense_grid, abi.GSParams(*GS), gx.exact_spec(vals), sc, init),
             cso.ref_gs(dense_map, RES, GS, r, ang, init, rel=REL))):
        cost, cov = gx.ge_at(dense_map, RES, r, ang, REL, ref.best, vals)
        gx.assert_gx(new, ref.best, cost, cov, name)
        assert new.normalized_cost == 0.0 and np.array(list(new.covariance)).tobytes() == \
            np.array([0.01, 0, 0, 0, 0.01, 0, 0, 0, 0.01], dtype=np.float64).tobytes(), name


def test_more_beams_than_the_lds_rows_hold(ctx, world, dense_map, dense_grid):
    """8200 beams: more than the stage's 8192 LDS terms, they go through the
    item's global rows; 4000 beams: in LDS for k_cost_gx, but 6 x 4000 doubles
    exceed k_ge_cost_batch's 144 KiB of LDS rows"""
    params = (5, 0.19, 0.19, 0.1, 20.0)
    for n_beams in (8200, 4000):
        r, ang, init = draw(world, 1, n_beams)
        sc = ctx.scan(r, ang, REL)
        new = ctx.optimize_pose_query(dense_grid, abi.RtcsmParams(*params), exact(), sc, init)
        ref = cso.ref_rtcsm(dense_map, RES, params, r, ang, init, rel=REL)
        gx.assert_gx_ref(new, ref, str(n_beams))
        old = ctx.optimize_pose_query(dense_grid, abi.RtcsmParams(*params), launcher_cost(), sc, init)
        assert cso.same_but_counters(new, chained(ctx, dense_grid, sc, old))   # the batch evaluator's global rows


def test_footprint_leaves_a_tiny_map(ctx):
    """a 3 x 2 map and a scan at its edge: almost every window cell lies outside the map"""
    rng = np.random.default_rng(5)
    tiny = (rng.uniform(0.05, 0.95, (2, 3)), 0.0, 0.0)
    grid = ctx.grid_from_array(*tiny, RES)
    ang = scene.beam_angles(181)
    r = rng.uniform(0.05, 0.4, size=181)
    init = (0.05, 0.05, 0.1)
    params = (5, 0.2, 0.2, 0.3, 20.0)
    sc = ctx.scan(r, ang)
    new = ctx.optimize_pose_query(grid, abi.RtcsmParams(*params), exact(), sc, init)
    gx.assert_gx_ref(new, cso.ref_rtcsm(tiny, RES, params, r, ang, init), "tiny map")
    assert new.normalized_cost < 0.0
    gs = ctx.gs_optimize_pose_query(grid, abi.GSParams(*GS), exact(), sc, init)
    gx.assert_gx_ref(gs, cso.ref_gs(tiny, RES, GS, r, ang, init), "tiny map gs")


def test_all_unknown_map(ctx, scans):
    """every cell unknown: every valid beam keeps the start value of the table"""
    empty = (np.zeros((120, 130)), -3.0, -3.25)
    grid = ctx.grid_from_array(*empty, RES)
    r, ang, init = scans[1]
    new = ctx.optimize_pose_query(grid, abi.RtcsmParams(*RT_SMALL), exact(), ctx.scan(r, ang, REL), init)
    gx.assert_gx_ref(new, cso.ref_rtcsm(empty, RES, RT_SMALL, r, ang, init, rel=REL), "unknown map")
    assert new.pose_found == 0 and new.normalized_cost < 0.0
    assert np.array(list(new.covariance)).tobytes() == \
        np.array([0.01, 0, 0, 0, 0.01, 0, 0, 0, 0.01], dtype=np.float64).tobytes()


@pytest.mark.parametrize("kernel_size", [0, 1, 2])
def test_kernel_sizes(ctx, dense_map, dense_grid, scans, kernel_size):
    """kernel size 1 is the unrolled instantiation, 0 and 2 the generic one"""
    r, ang, init = scans[2]
    sc = ctx.scan(r, ang, REL)
    vals = gx.LAUNCHER[:4] + (kernel_size,) + gx.LAUNCHER[5:]
    spec = gx.exact_spec(vals)
    for name, new, ref in (
            ("rtcsm", ctx.optimize_pose_query(dense_grid, abi.RtcsmParams(*RT_SMALL), spec, sc, init),
             cso.ref_rtcsm(dense_map, RES, RT_SMALL, r, ang, init, rel=REL)),
            ("bb", ctx.bb_optimize_pose_query(dense_grid, abi.BBParams(*BB), spec, sc, init),
             cso.ref_bb(dense_map, RES, BB, r, ang, init, rel=REL))):
        cost, cov = gx.ge_at(dense_map, RES, r, ang, REL, ref.best, vals)
        gx.assert_gx(new, ref.best, cost, cov, f"{name} K={kernel_size}")
        assert cost < 0.0


# ---------------------------------------------------------------- 5. the batched evaluator
def test_batch_evaluator_over_grids_of_different_resolution(ctx, world, dense_map, dense_grid, scans):
    """items over a 0.05 m and a 0.1 m map in one call: one term table per
    resolution; equal to lone lgs_cost_ge_exact calls at the seven poses and to
    the oracle"""
    coarse_map = build_map(world, 150, 0.1, 50, scene.arc_poses(9), n_beams=541)
    coarse_grid = ctx.grid_from_array(*coarse_map, 0.1)
    ge = launcher_cost()
    maps, grids, scs, raw, poses = [], [], [], [], []
    for k, (r, ang, init) in enumerate(scans + scans[:2]):
        m, g, res = (coarse_map, coarse_grid, 0.1) if k % 2 else (dense_map, dense_grid, RES)
        maps.append((m, res))
        grids.append(g)
        scs.append(ctx.scan(r, ang, REL))
        raw.append((r, ang))
        poses.append((init[0] + 0.01 * k, init[1] - 0.02 * k, init[2] + 0.003 * k))
    costs, covs = ctx.cost_ge_exact_batch(grids, ge, scs, poses, covariance=True)
    only = ctx.cost_ge_exact_batch(grids, ge, scs, poses)
    assert only.tobytes() == costs.tobytes()
    for k in range(len(poses)):
        (m, res), (r, ang) = maps[k], raw[k]
        c7 = ctx.cost_ge_exact(grids[k], ge, scs[k], gx.seven_poses(poses[k], res))
        assert costs[k] == c7[0], k
        grad = [0.5 * (c7[1] - c7[2]) / res, 0.5 * (c7[3] - c7[4]) / res, 0.5 * (c7[5] - c7[6]) / 1e-2]
        cov = [grad[a] * grad[b] for a in range(3) for b in range(3)]
        for d in (0, 4, 8):
            cov[d] += 0.01
        assert covs[k].tobytes() == np.array(cov).tobytes(), k
        oc, ocov = gx.ge_at(m, res, r, ang, REL, poses[k])
        assert costs[k] / len(r) == oc and covs[k].tobytes() == np.array(ocov).tobytes(), k
    assert len(set(costs.tolist())) == len(poses)


# ---------------------------------------------------------------- 6. determinism
def test_same_bytes_on_a_second_run_and_a_second_context(ctx, dense_map, scans):
    r, ang, init = scans[1]
    rt, bb = abi.RtcsmParams(*RT), abi.BBParams(*BB)

    def run(c):
        grid = c.grid_from_array(*dense_map, RES)
        sc = c.scan(r, ang, REL)
        return (bytes(c.optimize_pose_query(grid, rt, exact(), sc, init)),
                bytes(c.bb_optimize_pose_query(grid, bb, exact(), sc, init)))

    first, second = run(ctx), run(ctx)
    other = abi.Context(0)
    try:
        third = run(other)
    finally:
        other.close()
    assert first == second == third


# ---------------------------------------------------------------- 7. errors
def test_errors(ctx, dense_grid, scans):
    r, ang, init = scans[0]
    sc = ctx.scan(r, ang, REL)
    rt, bb, gs = abi.RtcsmParams(*RT_SMALL), abi.BBParams(*BB), abi.GSParams(*GS)
    too_wide = gx.exact_spec(gx.LAUNCHER[:4] + (17,) + gx.LAUNCHER[5:])
    for call in (lambda c: ctx.optimize_pose_query(dense_grid, rt, c, sc, init),
                 lambda c: ctx.bb_optimize_pose_query(dense_grid, bb, c, sc, init),
                 lambda c: ctx.gs_optimize_pose_query(dense_grid, gs, c, sc, init),
                 lambda c: ctx.loop_detect(rt, c, 0.5, [(dense_grid, None, (0, 0, 0), 0, 0, 1)], [(sc, init, 1)])):
        with pytest.raises(abi.LgsError) as e:
            call(too_wide)
        assert e.value.status == LGS_ERR_INVALID_ARG
    # an angle outside the restated sincos domain: LGS_ERR_INTERNAL, the caller's buffer untouched
    far = (init[0], init[1], 2.0e8)
    spec = exact()
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
        # the context works on the next call
        again = ctx.optimize_pose_query(dense_grid, rt, exact(), sc, init)
        assert again.normalized_cost < 0.0
    costs = np.full(1, 7.0)
    rc = ctx.lib.lgs_cost_ge_exact_batch(ctx.h, (C.c_void_p * 1)(dense_grid.h), C.byref(launcher_cost()),
                                         (C.c_void_p * 1)(sc.h), (abi.Pose2D * 1)(abi.Pose2D(*far)), 1,
                                         abi.dptr(costs), None)
    assert rc == LGS_ERR_INTERNAL and costs[0] == 7.0
