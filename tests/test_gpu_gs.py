"""GPU parity tests for the exhaustive grid-search matcher and loop detector:
lgs_gs_dense_scores, lgs_gs_optimize_pose_query / _batch, lgs_loop_detect_gs,
against the reference's algorithm composed from the oracle's pinned pieces
(compose_gs): ScanMatcherGridSearch::OptimizePose
(C/mapping/scan_matcher_grid_search.cpp:44-114) over orc_pixel_accurate_score.

Bar: dense scores bit-exact; pose_found, best_win, win, score_max and
estimated_pose bit-exact; normalized cost and covariance within 1e-5 (k_cost's
tolerance: the device's exp differs from glibc's in the last ulp).
"""
import ctypes as C

import numpy as np
import pytest

import oracle_bind as ob
from conftest import launcher_cost
from lgs_amd import abi, loopbatch, scene
from test_gpu_rtcsm import build_map

pytestmark = pytest.mark.gpu
DBL_MIN = 2.2250738585072014e-308
TOL = 1e-5
REL = (0.1, -0.05, 0.02)
WINDOW = (0.6, 0.4, 0.1, 0.05, 0.05, 0.01)   # 13 x 9 x 10 poses
SCORE_RANGE = (0.01, 20.0)                   # ScorePixelAccurate usable range


def literal_steps(rng, step):
    """for (double d = -r; d <= r; d += s) (:72-74)"""
    r, out = rng / 2.0, []
    d = -r
    while d <= r:
        out.append(d)
        d += step
    return out


class Ref:
    pass


def compose_gs(cells, mx, my, res, prm, ranges, angles, init, nthr=DBL_MIN, rel=(0.0, 0.0, 0.0), smin=0.0,
               smax=30.0):
    """The reference's OptimizePose, statement for statement, over the oracle."""
    L = ob.lib()
    g = ob.OGrid(cells, mx, my, res)
    sc = ob.OScan(ranges, angles, rel, smin, smax)
    P = ob.BBParams(0, 0, 0, 0, 0, prm[6], prm[7])
    cost = launcher_cost(oracle=True)
    sp = L.orc_compound(ob.Pose(*init), ob.Pose(*rel))
    xs, ys, ts = literal_steps(prm[0], prm[3]), literal_steps(prm[1], prm[4]), literal_steps(prm[2], prm[5])
    thr = nthr * len(sc.r)
    score_max, best, bp = thr, (-1, -1, -1), sp
    dense = np.zeros((len(ys), len(xs), len(ts)))
    for iy, dy in enumerate(ys):
        for ix, dx in enumerate(xs):
            for it, dt in enumerate(ts):
                pose = ob.Pose(sp.x + dx, sp.y + dy, sp.theta + dt)
                s = L.orc_pixel_accurate_score(C.byref(g.g), C.byref(P), C.byref(sc.s), pose)
                dense[iy, ix, it] = s
                if s > score_max:
                    score_max, best, bp = s, (ix, iy, it), pose
    r = Ref()
    r.dense = dense
    r.win = (len(xs), len(ys), len(ts))
    r.pose_found = int(score_max > thr)
    r.best_win = best
    r.score_max = score_max
    r.score_threshold = thr
    r.normalized_cost = L.orc_cost_ge_cost(C.byref(g.g), C.byref(cost), C.byref(sc.s), bp) / len(sc.r)
    cov = (C.c_double * 9)()
    L.orc_cost_ge_covariance(C.byref(g.g), C.byref(cost), C.byref(sc.s), bp, cov)
    r.covariance = list(cov)
    e = L.orc_move_backward(bp, ob.Pose(*rel))
    r.estimated_pose = (e.x, e.y, e.theta)
    r.ties = int((dense == dense.max()).sum())
    return r


def assert_gs_same(gpu, ref, tag=""):
    assert gpu.pose_found == ref.pose_found, tag
    assert tuple(gpu.win) == ref.win, (tag, tuple(gpu.win), ref.win)
    assert tuple(gpu.best_win) == ref.best_win, (tag, tuple(gpu.best_win), ref.best_win)
    assert gpu.score_max == ref.score_max, (tag, gpu.score_max, ref.score_max)
    assert gpu.score_threshold == ref.score_threshold, tag
    assert gpu.estimated_pose.tuple() == ref.estimated_pose, (tag, gpu.estimated_pose.tuple(), ref.estimated_pose)
    assert gpu.coarse_blocks == ref.win[0] * ref.win[1] * ref.win[2] and gpu.fine_blocks == 0, tag
    assert abs(gpu.normalized_cost - ref.normalized_cost) <= TOL, (tag, gpu.normalized_cost, ref.normalized_cost)
    assert np.allclose(list(gpu.covariance), ref.covariance, rtol=0, atol=TOL), tag


def draw(world, seed, n_beams):
    """true pose as test_gpu_bb.test_bb_query_dbl_min draws it; the initial
    pose is off by up to 0.15 m and 0.04 rad"""
    rng = np.random.default_rng(40 + seed)
    ang = scene.beam_angles(n_beams)
    true = (rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), rng.uniform(-np.pi, np.pi))
    r = scene.ray_cast(world, true, ang)
    init = (true[0] + rng.uniform(-0.15, 0.15), true[1] + rng.uniform(-0.15, 0.15),
            true[2] + rng.uniform(-0.04, 0.04))
    return r, ang, init


def gs_params(window=WINDOW, score_range=SCORE_RANGE):
    return abi.GSParams(*window, *score_range)


@pytest.fixture(scope="module")
def small_map(world):
    return build_map(world, 300, 0.05, 100, scene.arc_poses(4), n_beams=361)


@pytest.fixture(scope="module")
def small_refs(world, small_map):
    """the composed reference of the four small-map cases, computed once"""
    cells, mx, my = small_map
    out = []
    for seed in range(4):
        r, ang, init = draw(world, seed, 361)
        out.append((r, ang, init, compose_gs(cells, mx, my, 0.05, WINDOW + SCORE_RANGE, r, ang, init, rel=REL)))
    return out


@pytest.fixture(scope="module")
def small_grid(ctx, small_map):
    cells, mx, my = small_map
    return ctx.grid_from_array(cells, mx, my, 0.05)


@pytest.mark.parametrize("seed", range(4))
def test_gs_dense_parity(ctx, small_grid, small_refs, seed):
    r, ang, init, ref = small_refs[seed]
    assert ref.win == (13, 9, 10)
    gpu = ctx.gs_dense_scores(small_grid, gs_params(), ctx.scan(r, ang, REL), init)
    assert gpu.shape == ref.dense.shape
    assert gpu.tobytes() == ref.dense.tobytes(), int((gpu != ref.dense).sum())


@pytest.mark.parametrize("seed", range(4))
def test_gs_query(ctx, small_grid, small_refs, seed):
    """OptimizePose(query): threshold DBL_MIN, the whole summary"""
    r, ang, init, ref = small_refs[seed]
    gpu = ctx.gs_optimize_pose_query(small_grid, gs_params(), launcher_cost(), ctx.scan(r, ang, REL), init)
    assert ref.pose_found == 1
    assert_gs_same(gpu, ref, f"seed{seed}")
    assert list(gpu.steps) == list(WINDOW[3:])
    assert gpu.initial_pose.tuple() == init


def test_gs_batch_threshold(ctx, world):
    """LoopDetectorGridSearch's use: a batch against one 600-cell map with a
    threshold that three candidates pass and one does not; the batch equals
    the lone calls."""
    cells, mx, my = build_map(world, 600, 0.05, 100, scene.arc_poses(10), n_beams=1081)
    g = ctx.grid_from_array(cells, mx, my, 0.05)
    cases = [draw(world, seed, 1081) for seed in range(4)]
    refs = [compose_gs(cells, mx, my, 0.05, WINDOW + SCORE_RANGE, r, ang, init, nthr=0.5, rel=REL)
            for r, ang, init in cases]
    print("best normalised scores:", [round(float(ref.dense.max()) / 1081, 3) for ref in refs])
    assert [ref.pose_found for ref in refs] == [1, 1, 0, 1]
    scans = [ctx.scan(r, ang, REL) for r, ang, _ in cases]
    inits = [init for _, _, init in cases]
    out = ctx.gs_optimize_pose_batch(g, gs_params(), launcher_cost(), scans, inits, 0.5)
    for j, (o, ref) in enumerate(zip(out, refs)):
        assert_gs_same(o, ref, f"cand{j}")
    assert tuple(out[2].best_win) == (-1, -1, -1) and out[2].score_max == out[2].score_threshold == 0.5 * 1081
    for j in range(4):
        lone = ctx.gs_optimize_pose_batch(g, gs_params(), launcher_cost(), [scans[j]], [inits[j]], 0.5)[0]
        assert bytes(lone) == bytes(out[j]), j


@pytest.mark.parametrize("n_beams", [17, 64, 65, 361])
def test_gs_beam_counts_and_strict_range_tests(ctx, world, small_map, small_grid, n_beams):
    """Beam counts around the kernel's beam step and a wave's 64, with ranges
    exactly at scan.max, at umax and at umin (all excluded: both range tests
    are strict) and one ulp inside them (included)."""
    cells, mx, my = small_map
    r, ang, init = draw(world, 1, n_beams)
    umin, umax, smin, smax = 0.1, 5.0, 0.05, 6.0
    r = np.array(r, dtype=np.float64)
    edge = [smax, umax, umin, np.nextafter(umax, 0.0), np.nextafter(umin, 1.0), smin, umax, umin]
    for k, v in enumerate(edge):
        r[(2 * k + 1) % n_beams] = v
    prm = WINDOW + (umin, umax)
    ref = compose_gs(cells, mx, my, 0.05, prm, r, ang, init, nthr=0.3, rel=REL, smin=smin, smax=smax)
    sc = ctx.scan(r, ang, REL, smin, smax)
    P = gs_params(score_range=(umin, umax))
    dense = ctx.gs_dense_scores(small_grid, P, sc, init)
    assert dense.tobytes() == ref.dense.tobytes(), int((dense != ref.dense).sum())
    gpu = ctx.gs_optimize_pose_batch(small_grid, P, launcher_cost(), [sc], [init], 0.3)[0]
    assert_gs_same(gpu, ref, f"beams{n_beams}")


def test_gs_low_map_edge(ctx, small_map, small_grid, small_refs):
    """Many hit points left of and below the map: quotients floor to negative
    cells (truncation would fold cell -1 onto cell 0), and the poses tied at
    the maximum (two, with this scan at the sensor's own frame) resolve to the
    first in (iy, ix, it) order."""
    cells, mx, my = small_map
    r, ang, _, _ = small_refs[2]
    init = (mx + 0.3, my + 0.2, 0.4)
    ref = compose_gs(cells, mx, my, 0.05, WINDOW + SCORE_RANGE, r, ang, init)
    print("poses tied at the maximum:", ref.ties)
    assert ref.ties >= 2
    sc = ctx.scan(r, ang)
    dense = ctx.gs_dense_scores(small_grid, gs_params(), sc, init)
    assert dense.tobytes() == ref.dense.tobytes(), int((dense != ref.dense).sum())
    gpu = ctx.gs_optimize_pose_query(small_grid, gs_params(), launcher_cost(), sc, init)
    assert_gs_same(gpu, ref, "edge")
    iy, ix, it = np.unravel_index(int(np.argmax(ref.dense)), ref.dense.shape)   # first maximum in loop order
    assert tuple(gpu.best_win) == (ix, iy, it)


def test_gs_plateau(ctx):
    """Every pose scores the same sum: the first pose wins; on an all-zero map
    nothing is found and the estimate comes from the initial sensor pose."""
    ang = scene.beam_angles(17)
    r = np.full(17, 1.0)
    window = (0.2, 0.1, 0.3, 0.05, 0.05, 0.05)
    init = (0.0, 0.0, 0.3)
    P = gs_params(window)
    sc = ctx.scan(r, ang, REL)
    for value in (0.7, 0.0):
        cells = np.full((200, 200), value)
        g = ctx.grid_from_array(cells, -5.0, -5.0, 0.05)
        ref = compose_gs(cells, -5.0, -5.0, 0.05, window + SCORE_RANGE, r, ang, init, rel=REL)
        gpu = ctx.gs_optimize_pose_query(g, P, launcher_cost(), sc, init)
        assert_gs_same(gpu, ref, f"plateau{value}")
        if value:
            assert np.all(ref.dense == ref.dense[0, 0, 0])
            assert gpu.pose_found == 1 and tuple(gpu.best_win) == (0, 0, 0)
        else:
            assert gpu.pose_found == 0 and tuple(gpu.best_win) == (-1, -1, -1)
            assert gpu.score_max == gpu.score_threshold == DBL_MIN * 17
            sp = ob.lib().orc_compound(ob.Pose(*init), ob.Pose(*REL))
            e = ob.lib().orc_move_backward(sp, ob.Pose(*REL))
            assert gpu.estimated_pose.tuple() == (e.x, e.y, e.theta)
            assert gpu.best_sensor_pose.tuple() == (sp.x, sp.y, sp.theta)


def test_gs_step_accumulation_end_to_end(ctx, small_map, small_grid, small_refs):
    """0.6 / 0.1 and 0.3 / 0.05 give 6 values each, not 7, and the accumulated
    offsets differ from a -r + k s lattice in the last bits: the estimate must
    be the reference's bit for bit."""
    cells, mx, my = small_map
    r, ang, init, _ = small_refs[2]
    window = (0.6, 0.3, 0.1, 0.1, 0.05, 0.01)
    ref = compose_gs(cells, mx, my, 0.05, window + SCORE_RANGE, r, ang, init, rel=REL)
    gpu = ctx.gs_optimize_pose_query(small_grid, gs_params(window), launcher_cost(), ctx.scan(r, ang, REL), init)
    assert tuple(gpu.win)[:2] == (6, 6)
    assert_gs_same(gpu, ref, "steps")


def test_loop_detect_gs(ctx, world):
    """LoopDetectorGridSearch::Detect over two local maps of different size
    (four loops detected, two not), record by record, and through the
    sharding at world 1."""
    L = ob.lib()
    maps = [build_map(world, n, 0.05, 100, scene.arc_poses(k), n_beams=1081) for n, k in ((600, 10), (400, 8))]
    ang = scene.beam_angles(1081)
    rng = np.random.default_rng(21)
    grids = [ctx.grid_from_array(c, mx, my, 0.05) for c, mx, my in maps]
    queries, cands, ref, lmaps, lcands = [], [], [], [], []
    for q, (c, mx, my) in enumerate(maps):
        first = len(cands)
        node_pose = (0.1 * q, -0.05, 0.02 * q)
        for k in range(3):
            true = (rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), rng.uniform(-3, 3))
            r = scene.ray_cast(world, true, ang)
            # each query's last node starts outside the window's reach: no loop
            far = k == 2
            init = (true[0] + (0.7 if far else rng.uniform(-0.15, 0.15)),
                    true[1] + (-0.6 if far else rng.uniform(-0.15, 0.15)), true[2] + (0.2 if far else 0.03))
            cands.append((ctx.scan(r, ang), init, 100 * q + k))
            lcands.append(loopbatch.Candidate(q, r, ang, init, 100 * q + k))
            ref.append((compose_gs(c, mx, my, 0.05, WINDOW + SCORE_RANGE, r, ang, init, nthr=0.5), node_pose, q))
        queries.append((grids[q], None, node_pose, q, first, 3))
        lmaps.append(loopbatch.LocalMap(c, mx, my, 0.05, node_pose, q))
    P = gs_params()
    res = ctx.loop_detect_gs(P, launcher_cost(), 0.5, queries, cands)
    print("found:", [o.pose_found for o, _, _ in ref])
    assert [o.pose_found for o, _, _ in ref] == [1, 1, 0, 1, 1, 0]
    for k, (rr, (o, node_pose, q)) in enumerate(zip(res, ref)):
        assert rr.found == o.pose_found, k
        assert (rr.start_node_index, rr.end_node_index) == (q, cands[k][2]), k
        assert rr.start_node_pose.tuple() == node_pose, k
        assert rr.score == o.score_max, k
        assert rr.estimated_pose.tuple() == o.estimated_pose, k
        rel = L.orc_inverse_compound(ob.Pose(*node_pose), ob.Pose(*o.estimated_pose))
        assert rr.relative_pose.tuple() == ((rel.x, rel.y, rel.theta) if o.pose_found else (0.0, 0.0, 0.0)), k
        assert abs(rr.normalized_cost - o.normalized_cost) <= TOL, k
        assert np.allclose(list(rr.covariance), o.covariance, rtol=0, atol=TOL), k
    n = len(cands)
    direct = np.frombuffer(bytes(res), dtype=np.uint8)[: n * loopbatch.RECORD_BYTES].reshape(n, -1)
    fn = loopbatch.hip_detect_fn_gs(ctx, lmaps, lcands, P, launcher_cost(), 0.5)
    sharded = loopbatch.run_sharded(lcands, fn, rank=0, world=1)
    assert sharded.tobytes() == direct.tobytes()


def test_gs_invalid_arguments_launch_nothing(ctx, small_grid, small_refs):
    r, ang, init, _ = small_refs[0]
    sc = ctx.scan(r, ang, REL)
    bad = [(0.6, 0.4, 0.1, 0.0, 0.05, 0.01), (0.6, 0.4, 0.1, 0.05, -0.05, 0.01),
           (0.6, 0.4, 0.1, 0.05, 0.05, float("nan")), (0.6, 0.4, 0.1, float("inf"), 0.05, 0.01),
           (-0.6, 0.4, 0.1, 0.05, 0.05, 0.01), (0.6, float("nan"), 0.1, 0.05, 0.05, 0.01),
           (0.6, 0.4, float("inf"), 0.05, 0.05, 0.01),
           (0.6, 0.4, 0.1, 1e-6, 0.05, 0.01),      # 600,000 x values: beyond the per-axis cap
           (20.0, 20.0, 3.0, 0.05, 0.05, 0.001)]   # 401 x 401 x 3001 poses: beyond the window cap
    try:
        ctx.set_option(abi.LGS_OPT_PROFILE, 1)
        ctx.reset_stats()
        for window in bad:
            P = gs_params(window)
            for call in (lambda: ctx.gs_optimize_pose_query(small_grid, P, launcher_cost(), sc, init),
                         lambda: ctx.gs_optimize_pose_batch(small_grid, P, launcher_cost(), [sc], [init], 0.5),
                         lambda: ctx.loop_detect_gs(P, launcher_cost(), 0.5,
                                                    [(small_grid, None, (0, 0, 0), 0, 0, 1)], [(sc, init, 1)])):
                with pytest.raises(abi.LgsError, match="status 1"):
                    call()
            buf = np.zeros(13 * 9 * 10)
            assert ctx.lib.lgs_gs_dense_scores(ctx.h, small_grid.h, C.byref(P), sc.h, abi.Pose2D(*init),
                                               abi.dptr(buf), buf.size) == 1
        assert ctx.kernel_stats().get("k_gs_score", {}).get("launches", 0) == 0
        # the counter does count: one valid call, one score launch
        ctx.gs_optimize_pose_query(small_grid, gs_params(), launcher_cost(), sc, init)
        assert ctx.kernel_stats()["k_gs_score"]["launches"] == 1
    finally:
        ctx.set_option(abi.LGS_OPT_PROFILE, 0)
