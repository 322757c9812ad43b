"""GPU tests of the branch-and-bound matcher at its edges and fallback paths
(csrc/k_bb.hip): non-square maps, scans leaving the map, the scan's relative
pose and strict range tests, valid-beam counts around the score loop's step,
node heights from 0 to the limit, ties and empty maps, the scored-node count
against a model of the device's superset, the guard machinery's three
branches (selective re-score, re-score of everything past the cap, the
careful rerun over the thr0 superset), the batch size limit and the loop
detector's query packing.

Bar (test_gpu_bb.py's): best node, score, found flag, window, steps,
estimated pose and visited count bit-exact against the oracle; cost and
covariance within 1e-5.  Where no guard was corrected (fixups == 0) the
number of nodes the device scored equals bb_oracle.superset_model's count,
which test_bb_model_cpu.py pins against the oracle's search.

Every builder below is host-only and asserts the conditions its test states
on the oracle or model side before anything runs on the device.
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest

import bb_oracle as bo
import oracle_bind as ob
from bb_oracle import DBL_MIN, TOL, assert_bb_same, oracle_bb
from conftest import launcher_cost
from lgs_amd import abi, scene

pytestmark = pytest.mark.gpu
LGS_ERR_INVALID_ARG = 1
RES = 0.05
REL = (0.1, -0.05, 0.02)
SCORE_RANGE = (0.01, 20.0)
GUARD_EPS_DEFAULT, GUARD_CAP_DEFAULT = 1e-9, 64


# ------------------------------------------------------------------ inputs
def crop(cells, mx, my, res, x0, y0, w, h):
    """the w x h cells whose low corner is (x0, y0), zero where the map has none"""
    c0, r0 = int(round((x0 - mx) / res)), int(round((y0 - my) / res))
    out = np.zeros((h, w))
    H, W = cells.shape
    for r in range(h):
        for c in range(w):
            if 0 <= r0 + r < H and 0 <= c0 + c < W:
                out[r, c] = cells[r0 + r, c0 + c]
    return out, mx + c0 * res, my + r0 * res


def mini_map(res=RES, w=130, h=90, x0=-3.25, y0=-2.25):
    """A 6 m x 6 m walled room with four boxes, mapped from six poses on a small
    arc, cut to w x h cells: the walls at y = +-3 m lie outside a 90-row cut."""
    world = scene.make_world(seed=8, n_boxes=4, room_half=3.0, clear=1.2)
    ang = scene.beam_angles(361)
    m = ob.OMap(res, 10, w, h, (0.0, 0.0))
    bp = ob.BuilderParams(0.01, 20.0, 0.6, 0.45)
    for p in scene.arc_poses(6, spacing=0.3, radius=0.6):
        m.integrate(p, ob.OScan(scene.ray_cast(world, p, ang), ang), bp)
    cells, mx, my = crop(m.cells(), m.m.min_x, m.m.min_y, res, x0, y0, w, h)
    return SimpleNamespace(world=world, cells=cells, mx=mx, my=my, res=res)


@pytest.fixture(scope="module")
def mini():
    return mini_map()


def draw(mini, rng, n_beams, off=(0.12, 0.12, 0.03), exact_off=None):
    """a scan from a pose near the room's centre and an initial pose off it"""
    ang = scene.beam_angles(n_beams)
    true = (rng.uniform(-0.6, 0.6), rng.uniform(-0.4, 0.4), rng.uniform(-np.pi, np.pi))
    r = scene.ray_cast(mini.world, true, ang)
    d = exact_off if exact_off is not None else [rng.uniform(-o, o) for o in off]
    return r, ang, (true[0] + d[0], true[1] + d[1], true[2] + d[2])


def case(mini, prm, r, ang, init, thr=None, rel=(0.0, 0.0, 0.0), smin=0.0, smax=30.0, cells=None):
    return dict(cells=mini.cells if cells is None else cells, mx=mini.mx, my=mini.my, res=mini.res, prm=prm, ranges=r,
                angles=ang, init=init, thr=thr, rel=rel, smin=smin, smax=smax)


def valid_mask(kw):
    """ScorePixelAccurate's beam filter (:27-41), both tests strict"""
    r = np.asarray(kw["ranges"])
    lo, hi = max(kw["prm"][5], kw["smin"]), min(kw["prm"][6], kw["smax"])
    return ~((r >= hi) | (r <= lo))


def hit_cells(kw, node=(0, 0, 0), ora=None):
    """(ix, iy) of the valid beams at a node's pose: WorldCoordinateToGridCellIndex in numpy"""
    ora = ora or oracle_bb(**kw)
    sp = ob.lib().orc_compound(ob.Pose(*kw["init"]), ob.Pose(*kw["rel"]))
    x, y, th = (sp.x + node[0] * ora.steps[0], sp.y + node[1] * ora.steps[1], sp.theta + node[2] * ora.steps[2])
    m = valid_mask(kw)
    r, a = np.asarray(kw["ranges"])[m], np.asarray(kw["angles"])[m]
    ix = np.floor((x + r * np.cos(th + a) - kw["mx"]) / kw["res"]).astype(np.int64)
    iy = np.floor((y + r * np.sin(th + a) - kw["my"]) / kw["res"]).astype(np.int64)
    return ix, iy


# ------------------------------------------------------------------ device side
def gpu_match(ctx, kw, grid=None):
    g = grid if grid is not None else ctx.grid_from_array(kw["cells"], kw["mx"], kw["my"], kw["res"])
    sc = ctx.scan(kw["ranges"], kw["angles"], kw["rel"], kw["smin"], kw["smax"])
    P = abi.BBParams(*kw["prm"])
    if kw["thr"] is None:
        return ctx.bb_optimize_pose_query(g, P, launcher_cost(), sc, kw["init"])
    pyr = ctx.precompute_pyramid(g, kw["prm"][0])
    return ctx.bb_optimize_pose_batch(g, pyr, P, launcher_cost(), [sc], [kw["init"]], kw["thr"])[0]


def gpu_batch(ctx, kws):
    """one batch call over cases that share map, parameters and threshold"""
    k0 = kws[0]
    g = ctx.grid_from_array(k0["cells"], k0["mx"], k0["my"], k0["res"])
    pyr = ctx.precompute_pyramid(g, k0["prm"][0])
    scans = [ctx.scan(kw["ranges"], kw["angles"], kw["rel"], kw["smin"], kw["smax"]) for kw in kws]
    return ctx.bb_optimize_pose_batch(g, pyr, abi.BBParams(*k0["prm"]), launcher_cost(), scans,
                                      [kw["init"] for kw in kws], k0["thr"])


def check(gpu, kw, tag, ora=None, model=None):
    """the parity bar, and the scored-node count where no guard was corrected"""
    ora = ora or oracle_bb(**kw)
    assert_bb_same(gpu, ora, tag)
    if gpu.fixups == 0:
        m = model or bo.superset_model(**kw)
        want = m.count if m.path_ok else m.count_thr0
        print(f"{tag}: scored {gpu.coarse_blocks} (model {want}), visited {gpu.fine_blocks}, path_ok {m.path_ok}")
        assert gpu.coarse_blocks == want, (tag, gpu.coarse_blocks, want, m.count_thr0)
    return ora


class guard_options:
    """LGS_OPT_GUARD_EPS / INJECT_INDEX / GUARD_CAP for a block, restored after it"""

    def __init__(self, ctx, eps, inject=1, cap=GUARD_CAP_DEFAULT):
        self.ctx, self.eps, self.inject, self.cap = ctx, eps, inject, cap

    def __enter__(self):
        self.ctx.set_option(abi.LGS_OPT_GUARD_EPS, self.eps)
        self.ctx.set_option(abi.LGS_OPT_GUARD_CAP, self.cap)
        self.ctx.set_option(abi.LGS_OPT_INJECT_INDEX, self.inject)

    def __exit__(self, *exc):
        self.ctx.set_option(abi.LGS_OPT_INJECT_INDEX, 0)
        self.ctx.set_option(abi.LGS_OPT_GUARD_CAP, GUARD_CAP_DEFAULT)
        self.ctx.set_option(abi.LGS_OPT_GUARD_EPS, GUARD_EPS_DEFAULT)
        return False


# ------------------------------------------------------------------ 1. non-square maps
def nonsquare_cases(mini):
    """The 90 x 130 map and its 130 x 90 transpose (same corner, same scans).
    Conditions: at the best pose several valid beams hit known cells beyond
    the shorter side (a W/H swap in a bounds test zeroes them without leaving
    the buffer), and the result on the transpose differs from the map's."""
    out = {}
    rng = np.random.default_rng(101)
    prm = (3, 0.5, 0.4, 0.08, 20.0) + SCORE_RANGE
    scans = [draw(mini, rng, 181) for _ in range(4)]
    for name, cells in (("wide", mini.cells), ("tall", np.ascontiguousarray(mini.cells.T))):
        H, W = cells.shape
        short = min(W, H)
        q = case(mini, prm, *scans[0], cells=cells)
        b = [case(mini, prm, *s, thr=0.05, cells=cells) for s in scans[1:]]
        refs = [oracle_bb(**kw) for kw in [q] + b]
        for kw, o in zip([q] + b, refs):
            assert o.pose_found == 1
            ix, iy = hit_cells(kw, tuple(o.best_win), o)
            far = (ix >= short) & (ix < W) & (iy >= 0) & (iy < H) if W > H else \
                  (iy >= short) & (iy < H) & (ix >= 0) & (ix < W)
            known = int((cells[iy[far], ix[far]] > 0).sum())
            assert known >= 5, (name, known)
        out[name] = SimpleNamespace(query=q, batch=b, refs=refs)
    for a, b in zip(out["wide"].refs, out["tall"].refs):
        assert (list(a.best_win), a.score_max) != (list(b.best_win), b.score_max)
    return out


@pytest.fixture(scope="module")
def nonsquare(mini):
    return nonsquare_cases(mini)


@pytest.mark.parametrize("name", ["wide", "tall"])
def test_bb_nonsquare_maps(ctx, nonsquare, name):
    c = nonsquare[name]
    check(gpu_match(ctx, c.query), c.query, f"{name}/query", c.refs[0])
    for j, (o, kw) in enumerate(zip(gpu_batch(ctx, c.batch), c.batch)):
        check(o, kw, f"{name}/batch{j}", c.refs[1 + j])
    with guard_options(ctx, 0.01):
        gpu = gpu_match(ctx, c.query)
    assert gpu.fixups == 1 and gpu.guard_hits > 0
    check(gpu, c.query, f"{name}/inject", c.refs[0])


# ------------------------------------------------------------------ 2. map edges
def edge_cases(mini):
    """A pose 0.4 m inside each border: at the window's centre pose at least
    10 % of the valid beams hit outside the map on that side; a corner pose
    with hits in cell -1 on both axes; a pose from which no beam reaches the map."""
    rng = np.random.default_rng(202)
    r, ang, _ = draw(mini, rng, 181)
    H, W = mini.cells.shape
    x1, y1 = mini.mx + W * RES, mini.my + H * RES
    prm = (3, 0.5, 0.5, 0.08, 20.0) + SCORE_RANGE
    out = {}
    for name, init, side in (("left", (mini.mx + 0.4, 0.1, 0.3), lambda ix, iy: ix < 0),
                             ("right", (x1 - 0.4, -0.2, 2.0), lambda ix, iy: ix >= W),
                             ("bottom", (0.3, mini.my + 0.4, -1.0), lambda ix, iy: iy < 0),
                             ("top", (-0.2, y1 - 0.4, 1.2), lambda ix, iy: iy >= H)):
        kw = case(mini, prm, r, ang, init)
        ora = oracle_bb(**kw)
        ix, iy = hit_cells(kw, ora=ora)
        assert side(ix, iy).sum() >= 0.1 * len(ix), (name, int(side(ix, iy).sum()), len(ix))
        assert ora.pose_found == 1
        out[name] = (kw, ora)
    kw = case(mini, prm, r, ang, (mini.mx + 0.3, mini.my + 0.2, 0.4))
    ix, iy = hit_cells(kw)
    assert (ix == -1).any() and (iy == -1).any() and ((ix < 0) & (iy < 0)).any()
    out["corner"] = (kw, oracle_bb(**kw))
    kw = case(mini, prm, r, ang, (mini.mx - 40.0, mini.my - 40.0, 0.0))
    ora = oracle_bb(**kw)
    m = bo.superset_model(**kw)
    assert ora.pose_found == 0 and ora.score_max == DBL_MIN * 181 and m.count == m.n_top == ora.coarse_evals
    out["outside"] = (kw, ora)
    return out


@pytest.fixture(scope="module")
def edges(mini):
    return edge_cases(mini)


@pytest.mark.parametrize("name", ["left", "right", "bottom", "top", "corner", "outside"])
def test_bb_map_edges(ctx, edges, name):
    kw, ora = edges[name]
    gpu = gpu_match(ctx, kw)
    check(gpu, kw, name, ora)
    if name == "outside":
        assert gpu.pose_found == 0 and gpu.score_max == gpu.score_threshold and list(gpu.best_win) == [0, 0, 0]


# ------------------------------------------------------------------ 3. scan geometry
UMIN, UMAX, SMIN, SMAX = 0.1, 5.0, 0.05, 6.0
NV = [0, 1, 15, 16, 17, 32, 33]


def geometry_case(mini, nv, scan_range_max=20.0):
    """nv valid beams and six excluded ones: ranges exactly at scan.max, umax,
    umin and scan.min (twice umax and umin: every test is strict); the first
    two valid beams one ulp inside umin and umax.  The scan's largest range is
    scan.max = 6.0, so ComputeSearchStep takes min(6.0, scan_range_max)."""
    rng = np.random.default_rng(300 + nv)
    n = nv + 6
    r, ang, init = draw(mini, rng, n, off=(0.08, 0.08, 0.02))
    r = np.clip(np.array(r, dtype=np.float64), 0.3, 4.5)
    pos = rng.permutation(n)
    for k, v in enumerate([SMAX, UMAX, UMIN, SMIN, UMAX, UMIN]):
        r[pos[k]] = v
    for k, v in enumerate([np.nextafter(UMIN, 1.0), np.nextafter(UMAX, 0.0)][:nv]):
        r[pos[6 + k]] = v
    prm = (2, 0.3, 0.3, 0.05, scan_range_max, UMIN, UMAX)
    kw = case(mini, prm, r, ang, init, thr=None if nv % 2 else 0.2, rel=REL, smin=SMIN, smax=SMAX)
    assert int(valid_mask(kw).sum()) == nv and r.max() == SMAX
    return kw


@pytest.mark.parametrize("nv", NV)
def test_bb_beam_counts_and_strict_range_tests(ctx, mini, nv):
    kw = geometry_case(mini, nv)
    ora = oracle_bb(**kw)
    th = RES / SMAX
    assert ora.steps[2] == math.acos(1.0 - 0.5 * th * th)
    if nv == 0:
        assert ora.pose_found == 0 and ora.coarse_evals == bo.superset_model(**kw).n_top
    gpu = gpu_match(ctx, kw)
    check(gpu, kw, f"nv{nv}", ora)
    sp = ob.lib().orc_compound(ob.Pose(*kw["init"]), ob.Pose(*REL))
    b = ora.best_win
    assert gpu.best_sensor_pose.tuple() == ((sp.x + b[0] * ora.steps[0], sp.y + b[1] * ora.steps[1],
                                             sp.theta + b[2] * ora.steps[2]) if ora.pose_found else
                                            (sp.x, sp.y, sp.theta))
    assert gpu.initial_pose.tuple() == kw["init"]


def test_bb_scan_range_max_sets_the_angular_step(ctx, mini):
    kw = geometry_case(mini, 33, scan_range_max=3.0)
    ora = oracle_bb(**kw)
    th = RES / 3.0
    assert ora.steps[2] == math.acos(1.0 - 0.5 * th * th)
    check(gpu_match(ctx, kw), kw, "srm3", ora)


# ------------------------------------------------------------------ 4. node heights
HEIGHT_WINDOW = (0.5, 0.5, 0.06)   # win 5 x 5: 11 cells a side


def height_case(mini, h):
    """One scan whose true pose lies about 8 and 7 cells beyond the initial
    pose: outside the 5-cell window, inside the leaves of a top node of
    2^h >= 16.  (Not whole cells and not the cost's 0.01 rad step: at the true
    pose the beams end on the walls, which lie on cell boundaries.)"""
    rng = np.random.default_rng(404)
    r, ang, init = draw(mini, rng, 181, exact_off=(-8 * RES + 0.012, -7 * RES - 0.009, 0.013))
    return case(mini, (h,) + HEIGHT_WINDOW + (20.0,) + SCORE_RANGE, r, ang, init)


@pytest.mark.parametrize("h", [0, 1, 2, 5, 8])
def test_bb_node_heights(ctx, mini, h):
    kw = height_case(mini, h)
    ora, m = oracle_bb(**kw), bo.superset_model(**kw)
    assert list(ora.win)[:2] == [5, 5] and ora.pose_found == 1
    H, W = mini.cells.shape
    if h in (1, 2):      # (a) the window is no multiple of 2^h: the last top node's leaves pass +win
        assert 11 % (1 << h) != 0 and ora.best_win[0] == 6
    if h >= 5:           # (b) one top node per angle; the best node lies beyond +win
        assert (1 << h) > 11 and m.n_top == m.T
        assert max(ora.best_win[0], ora.best_win[1]) > 5, list(ora.best_win)
    if h == 8:           # (c) 2^h at or above both map dimensions
        assert (1 << h) >= max(W, H)
    if h == 0:
        assert m.count == m.n_top == 11 * 11 * m.T == ora.coarse_evals
    check(gpu_match(ctx, kw), kw, f"h{h}", ora, m)


def tiny_noise_case(hm, n_beams=17, seed=5, window=(0.3, 0.3, 0.1)):
    rng = np.random.default_rng(seed)
    cells = np.where(rng.random((56, 40)) < 0.15, rng.choice([0.45, 0.6, 0.8, 0.999], size=(56, 40)), 0.0)
    ang = -np.pi + np.arange(n_beams) * (2 * np.pi / n_beams)
    r = rng.uniform(0.15, 0.9, size=n_beams)
    return dict(cells=cells, mx=-1.0, my=-1.4, res=RES, prm=(hm,) + window + (20.0,) + SCORE_RANGE, ranges=r,
                angles=ang, init=(0.05, 0.0, 0.3), thr=None, rel=(0.0, 0.0, 0.0), smin=0.0, smax=30.0)


def test_bb_node_height_limit(ctx):
    """node_height_max 12 (a 4096-cell top node) on a 40 x 56 map, 17 beams"""
    kw = tiny_noise_case(12)
    ora = oracle_bb(**kw)
    assert ora.pose_found == 1
    check(gpu_match(ctx, kw), kw, "h12", ora)


@pytest.mark.parametrize("h", [0, 3])
def test_bb_zero_ranges(ctx, h):
    """range_x = range_y = range_theta = 0: a 0 x 0 x 0 window; at height 0 one pose"""
    kw = tiny_noise_case(h, window=(0.0, 0.0, 0.0))
    ora = oracle_bb(**kw)
    assert list(ora.win) == [0, 0, 0]
    if h == 0:
        assert ora.coarse_evals == 1 and list(ora.best_win) == [0, 0, 0]
    check(gpu_match(ctx, kw), kw, f"zero/h{h}", ora)


@pytest.mark.parametrize("shape", [(8, 3), (37, 53), (64, 200)])
def test_bb_pyramid_parity_height_7(ctx, shape):
    """windows up to 128: past the array's size in every shape's short axis"""
    rng = np.random.default_rng(shape[0])
    cells = rng.choice([0.0, 0.0, 0.45, 0.6, 0.9], size=shape) * rng.uniform(0.5, 1.0, size=shape)
    g = ctx.grid_from_array(cells, -2.0, -3.0, RES)
    for h, (d, o) in enumerate(zip(ctx.precompute_pyramid(g, 7), ob.precompute_pyramid(cells, 7))):
        assert np.array_equal(d.download(), o), h


# ------------------------------------------------------------------ 5. ties, empties, thresholds
def plateau_case(mini, value):
    rng = np.random.default_rng(505)
    ang = scene.beam_angles(33)
    r = rng.uniform(0.3, 1.0, size=33)
    return case(mini, (3, 0.4, 0.4, 0.1, 20.0) + SCORE_RANGE, r, ang, (0.1, -0.1, 0.3), rel=REL,
                cells=np.full(mini.cells.shape, value))


def test_bb_uniform_map_first_leaf_wins(ctx, mini):
    """Every node scores 33 x 0.5: the first descent's leaf is accepted and
    every later node ties with it and is pruned (score <= scoreMax)."""
    kw = plateau_case(mini, 0.5)
    ora, m, es = oracle_bb(**kw), bo.superset_model(**kw), bo.exact_search(**kw)
    assert m.path_ok and ora.score_max == 16.5
    assert tuple(ora.best_win) == m.path[-1][:3] and es.expanded == set(m.path[:-1])
    assert ora.coarse_evals == m.n_top + 4 * 3 == m.count
    gpu = gpu_match(ctx, kw)
    check(gpu, kw, "uniform", ora, m)
    assert gpu.pose_found == 1 and tuple(gpu.best_win) == m.path[-1][:3]


def test_bb_empty_map(ctx, mini):
    kw = plateau_case(mini, 0.0)
    ora = oracle_bb(**kw)
    gpu = gpu_match(ctx, kw)
    check(gpu, kw, "empty", ora)
    assert gpu.pose_found == 0 and list(gpu.best_win) == [0, 0, 0]
    assert gpu.score_max == gpu.score_threshold == DBL_MIN * 33
    sp = ob.lib().orc_compound(ob.Pose(*kw["init"]), ob.Pose(*REL))
    e = ob.lib().orc_move_backward(sp, ob.Pose(*REL))
    assert gpu.estimated_pose.tuple() == (e.x, e.y, e.theta)
    assert gpu.best_sensor_pose.tuple() == (sp.x, sp.y, sp.theta)


BATCH_THR = 0.2


def threshold_batch(mini):
    """six candidates, the odd ones started far outside the window's reach"""
    rng = np.random.default_rng(606)
    prm = (3, 0.4, 0.4, 0.08, 20.0) + SCORE_RANGE
    kws = []
    for k in range(6):
        off = (0.9, -0.8, 0.5) if k % 2 else (0.1, -0.05, 0.02)
        kws.append(case(mini, prm, *draw(mini, rng, 91, exact_off=off), thr=BATCH_THR, rel=REL))
    refs = [oracle_bb(**kw) for kw in kws]
    assert [o.pose_found for o in refs] == [1, 0, 1, 0, 1, 0], [o.score_max / 91 for o in refs]
    return kws, refs


def test_bb_batch_threshold(ctx, mini):
    """a batch in which some candidates pass and some do not equals the lone calls byte for byte"""
    kws, refs = threshold_batch(mini)
    out = gpu_batch(ctx, kws)
    for j, (o, kw, ora) in enumerate(zip(out, kws, refs)):
        check(o, kw, f"cand{j}", ora)
        if not ora.pose_found:
            assert list(o.best_win) == [0, 0, 0] and o.score_max == o.score_threshold == BATCH_THR * 91
    for j, kw in enumerate(kws):
        assert bytes(gpu_batch(ctx, [kw])[0]) == bytes(out[j]), j


def nobody_passes_batch(mini):
    kws, _ = threshold_batch(mini)
    kws = [dict(kw, thr=0.97) for kw in kws]
    refs = [oracle_bb(**kw) for kw in kws]
    assert not any(o.pose_found for o in refs)
    return kws, refs


def test_bb_batch_nobody_passes(ctx, mini):
    kws, refs = nobody_passes_batch(mini)
    for j, (o, kw, ora) in enumerate(zip(gpu_batch(ctx, kws), kws, refs)):
        check(o, kw, f"none{j}", ora)
        assert o.pose_found == 0 and list(o.best_win) == [0, 0, 0] and o.score_max == o.score_threshold


PATH_MISS_SEED = 0


def path_miss_case(mini, seed=PATH_MISS_SEED):
    """the first descent (towards the +x, +y, +theta corner) misses thr0 while
    the true pose, in the opposite corner, passes it"""
    rng = np.random.default_rng(700 + seed)
    r, ang, init = draw(mini, rng, 91, exact_off=(0.15, 0.15, 0.03))
    return case(mini, (3, 0.4, 0.4, 0.08, 20.0) + SCORE_RANGE, r, ang, init, thr=BATCH_THR)


def test_bb_first_descent_misses_threshold(ctx, mini):
    kw = path_miss_case(mini)
    ora, m = oracle_bb(**kw), bo.superset_model(**kw)
    assert not m.path_ok and ora.pose_found == 1
    check(gpu_match(ctx, kw), kw, "path_miss", ora, m)


# ------------------------------------------------------------------ 7. guard machinery
GUARD_PRM = (2, 0.1, 0.1, 0.05, 20.0) + SCORE_RANGE   # win 1 x 1: at most 21 nodes an angle
SELECTIVE_EPS_ONE, SELECTIVE_EPS_BATCH = 6e-3, 5e-5


def predicted_guards(kw, eps, nodes):
    """score_node's guard test for the listed (x, y, t, h) nodes, in numpy:
    the records the device writes for them at guard_eps = eps (its ~1e-13-cell
    differences aside).  The top nodes are scored whatever the scores are, so
    their records bound the device's count from below also under injection."""
    ora = oracle_bb(**kw)
    sp = ob.lib().orc_compound(ob.Pose(*kw["init"]), ob.Pose(*kw["rel"]))
    m = valid_mask(kw)
    r, a = np.asarray(kw["ranges"])[m], np.asarray(kw["angles"])[m]
    n = 0
    for x, y, t, _ in nodes:
        th = sp.theta + t * ora.steps[2]
        qx = (sp.x + x * ora.steps[0] + r * np.cos(th + a) - kw["mx"]) / kw["res"]
        qy = (sp.y + y * ora.steps[1] + r * np.sin(th + a) - kw["my"]) / kw["res"]
        fx, fy = qx - np.floor(qx), qy - np.floor(qy)
        n += int(((fx < eps) | (fx > 1 - eps) | (fy < eps) | (fy > 1 - eps)).sum())
    return n


def top_guards(kws, eps):
    return sum(predicted_guards(kw, eps, bo.superset_model(**kw).top) for kw in kws)


def guard_inputs(mini):
    """One 9-beam match and a 64-match batch of 9..17-beam scans, threshold
    0.2.  The steps equal the resolution, so every node of one angle sees a
    beam at the same offset inside its cell: records come in groups of up to
    the angle's node count (21 here), and an eps is chosen per input so that
    at least one group and fewer than 64 records appear."""
    rng = np.random.default_rng(808)
    one = case(mini, GUARD_PRM, *draw(mini, rng, 9, off=(0.08, 0.08, 0.02)))
    batch = [case(mini, GUARD_PRM, *draw(mini, rng, int(rng.integers(9, 18)), off=(0.08, 0.08, 0.02)), thr=0.2)
             for _ in range(64)]
    assert 0 < top_guards([one], SELECTIVE_EPS_ONE) and 0 < top_guards(batch, SELECTIVE_EPS_BATCH)
    return one, batch


@pytest.fixture(scope="module")
def guard_cases(ctx, mini):
    one, batch = guard_inputs(mini)
    c = SimpleNamespace(one=one, batch=batch, ref_one=oracle_bb(**one), refs=[oracle_bb(**kw) for kw in batch])
    c.grid = ctx.grid_from_array(mini.cells, mini.mx, mini.my, mini.res)
    c.clean = bytes(gpu_match(ctx, one, c.grid))   # (d): the same bytes after every guard test
    return c


def assert_clean_again(ctx, c):
    assert bytes(gpu_match(ctx, c.one, c.grid)) == c.clean


def test_bb_guard_selective_path(ctx, guard_cases):
    """Under the record cap: the guard-node gather, the host cell check, the
    sort and dedupe of dirty nodes and their re-score slots, with a real
    mismatch in every record (LGS_OPT_INJECT_INDEX).  guard_hits also counts
    the cost kernel's guard records, so fewer than 64 in all, with at least
    one predicted among the top nodes (guard_inputs), puts the matcher's own
    count inside (0, 64): the selective branch."""
    c = guard_cases
    try:
        with guard_options(ctx, SELECTIVE_EPS_ONE):
            gpu = gpu_match(ctx, c.one, c.grid)
        print("selective, one match: guard records", gpu.guard_hits)
        assert 0 < gpu.guard_hits < GUARD_CAP_DEFAULT and gpu.fixups == 1
        check(gpu, c.one, "selective/one", c.ref_one)
        with guard_options(ctx, SELECTIVE_EPS_BATCH):
            out = gpu_batch(ctx, c.batch)
        hits = sum(o.guard_hits for o in out)
        print("selective, 64 matches: guard records", hits, "matches fixed", sum(o.fixups for o in out))
        assert 0 < hits < GUARD_CAP_DEFAULT and 1 <= sum(o.fixups for o in out) < 64
        for j, (o, kw, ora) in enumerate(zip(out, c.batch, c.refs)):
            check(o, kw, f"selective/cand{j}", ora)
    finally:
        assert_clean_again(ctx, c)


@pytest.mark.parametrize("eps,cap", [(SELECTIVE_EPS_ONE, 0), (SELECTIVE_EPS_BATCH, 0), (1e-2, GUARD_CAP_DEFAULT)])
def test_bb_guard_past_cap_path(ctx, guard_cases, eps, cap):
    """Past the cap on purpose (cap 0: any record is past it): every node of
    every level re-scored from host cells, so every match of the batch reports a fix."""
    c = guard_cases
    top_one, top_batch = top_guards([c.one], eps), top_guards(c.batch, eps)
    assert top_batch > cap
    try:
        with guard_options(ctx, eps, cap=cap):
            gpu = gpu_match(ctx, c.one, c.grid)
            out = gpu_batch(ctx, c.batch)
        print(f"past cap (eps {eps}, cap {cap}): top-node records predicted {top_one} / {top_batch},",
              "credited", gpu.guard_hits, "/", sum(o.guard_hits for o in out))
        if top_one > cap:
            assert gpu.fixups == 1
        assert sum(o.fixups for o in out) == 64
        check(gpu, c.one, "pastcap/one", c.ref_one)
        for j, (o, kw, ora) in enumerate(zip(out, c.batch, c.refs)):
            check(o, kw, f"pastcap/cand{j}", ora)
    finally:
        assert_clean_again(ctx, c)


RERUN_SEED = 1


def shifted(levels):
    """each pyramid level read one column to the right, the last column zero"""
    out = []
    for m in levels:
        s = np.zeros_like(m)
        s[:, :-1] = m[:, 1:]
        out.append(s)
    return out


def rerun_case(mini, seed=RERUN_SEED):
    """LGS_OPT_GUARD_EPS 0.5 with injection guards every cell: the device's
    first pass scores the map one column to the right.  The true pose lies one
    cell right of the first descent's leaf, so the shifted leaf scores the
    highest there is and the shifted superset expands next to nothing, while
    the exact search expands nodes outside it: the replay meets an unexpanded
    node and the match is rerun over the thr0 superset, level by level from
    corrected scores."""
    rng = np.random.default_rng(900 + seed)
    n = 33
    ang = scene.beam_angles(n)
    true = (rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), rng.uniform(-np.pi, np.pi))
    r = np.minimum(scene.ray_cast(mini.world, true, ang), 1.6)
    prm = (2, 0.3, 0.3, 0.03, 20.0) + SCORE_RANGE
    probe = oracle_bb(**case(mini, prm, r, ang, true))
    wx, wy, wt = probe.win
    lx = -wx + ((2 * wx) // 4) * 4 + 3          # the first descent's leaf: last top node + 2^h - 1
    ly = -wy + ((2 * wy) // 4) * 4 + 3
    init = (true[0] - (lx + 1) * RES, true[1] - ly * RES, true[2] - wt * probe.steps[2])
    kw = case(mini, prm, r, ang, init)
    ora = oracle_bb(**kw)
    H, W = mini.cells.shape
    margin = (1 << prm[0]) + 1
    for node in [(x, y, t) for x in (-wx, lx) for y in (-wy, ly) for t in (-wt, wt)]:
        ix, iy = hit_cells(kw, node, ora)
        assert ix.min() > margin and ix.max() < W - 1 - margin and iy.min() > margin and iy.max() < H - 1 - margin
    true_m = bo.superset_model(**kw)
    shift_m = bo.superset_model(**kw, score_maps=shifted(ob.precompute_pyramid(mini.cells, prm[0])))
    es = bo.exact_search(**kw)
    assert shift_m.path[-1][:2] == (lx, ly)
    return SimpleNamespace(kw=kw, ora=ora, true_m=true_m, shift_m=shift_m, es=es)


def test_bb_guard_rerun(ctx, mini, guard_cases):
    c = rerun_case(mini)
    missing = c.es.expanded - c.shift_m.expanded
    assert missing, "the exact search stays inside the shifted superset: no rerun"
    assert c.shift_m.path_ok and c.true_m.count_thr0 != c.shift_m.count
    try:
        with guard_options(ctx, 0.5):
            gpu = gpu_match(ctx, c.kw, guard_cases.grid)
        print("rerun: scored", gpu.coarse_blocks, "thr0 superset (true maps)", c.true_m.count_thr0,
              "shifted thr_exp superset", c.shift_m.count, "true thr_exp superset", c.true_m.count)
        assert_bb_same(gpu, c.ora, "rerun")
        assert gpu.fixups == 1
        assert gpu.coarse_blocks == c.true_m.count_thr0
        assert gpu.coarse_blocks != c.shift_m.count
    finally:
        assert_clean_again(ctx, guard_cases)


# ------------------------------------------------------------------ 8. batch limits and mixed waves
def small_scans(mini, rng, n, prm, thr, cells=None, geom=None, far_every=0):
    kws = []
    for k in range(n):
        off = (0.9, -0.7, 0.4) if far_every and k % far_every == far_every - 1 else None
        r, ang, init = draw(mini, rng, int(rng.integers(9, 18)), off=(0.08, 0.08, 0.02), exact_off=off)
        kw = case(mini, prm, r, ang, init, thr=thr, cells=cells)
        if geom:
            kw.update(mx=geom[0], my=geom[1], res=geom[2])
        kws.append(kw)
    return kws


def test_bb_batch_crosses_the_chunk_size(ctx, mini):
    """513 candidates: two chunks of the entry point's 512-match launches"""
    kws = small_scans(mini, np.random.default_rng(1001), 513, (2, 0.2, 0.2, 0.04, 20.0) + SCORE_RANGE, 0.2)
    out = gpu_batch(ctx, kws)
    assert len(out) == 513
    for j, (o, kw) in enumerate(zip(out, kws)):
        assert_bb_same(o, oracle_bb(**kw), f"cand{j}")
    for j in (0, 511, 512):
        check(out[j], kws[j], f"cand{j}")
        assert bytes(gpu_batch(ctx, [kws[j]])[0]) == bytes(out[j]), j


LOOP_THR = 0.25


def loop_problem(mini):
    """three local maps of different shape, the third at resolution 0.1;
    300 + 0 + 250 candidates, every fourth started out of the window's reach"""
    tall = np.ascontiguousarray(mini.cells.T)
    coarse = mini_map(res=0.1, w=70, h=60, x0=-3.5, y0=-3.0)
    maps = [(mini.cells, mini.mx, mini.my, RES), (tall, mini.mx, mini.my, RES),
            (coarse.cells, coarse.mx, coarse.my, 0.1)]
    prm = (2, 0.2, 0.2, 0.04, 20.0) + SCORE_RANGE
    rng = np.random.default_rng(1102)
    counts = (300, 0, 250)
    kws = []
    for q, cnt in enumerate(counts):
        c, mx, my, res = maps[q]
        kws += small_scans(mini, rng, cnt, prm, LOOP_THR, cells=c, geom=(mx, my, res), far_every=4)
    return maps, counts, prm, kws


def test_loop_detect_bb_query_packing(ctx, mini):
    L = ob.lib()
    maps, counts, prm, kws = loop_problem(mini)
    refs = [oracle_bb(**kw) for kw in kws]
    found = [o.pose_found for o in refs]
    assert 0 in found and 1 in found
    grids = [ctx.grid_from_array(c, mx, my, res) for c, mx, my, res in maps]
    node_poses = [(0.1 * q, -0.05, 0.02 * q) for q in range(3)]
    queries, first = [], 0
    for q, cnt in enumerate(counts):
        queries.append((grids[q], None, node_poses[q], 10 + q, first, cnt))
        first += cnt
    cands = [(ctx.scan(kw["ranges"], kw["angles"]), kw["init"], 1000 + k) for k, kw in enumerate(kws)]
    res = ctx.loop_detect_bb(abi.BBParams(*prm), launcher_cost(), LOOP_THR, queries, cands)
    for k, (kw, o) in enumerate(zip(kws, refs)):
        rr, q = res[k], 0 if k < 300 else 2
        assert rr.found == o.pose_found, k
        assert (rr.start_node_index, rr.end_node_index) == (10 + q, 1000 + k), k
        assert rr.start_node_pose.tuple() == node_poses[q], k
        assert rr.score == o.score_max, k
        assert rr.estimated_pose.tuple() == (o.estimated_pose.x, o.estimated_pose.y, o.estimated_pose.theta), k
        if o.pose_found:
            rel = L.orc_inverse_compound(ob.Pose(*node_poses[q]), o.estimated_pose)
            assert rr.relative_pose.tuple() == (rel.x, rel.y, rel.theta), k
        else:
            assert rr.relative_pose.tuple() == (0.0, 0.0, 0.0), k
            assert rr.score == LOOP_THR * len(kw["ranges"]), k
        assert abs(rr.normalized_cost - o.normalized_cost) <= TOL, k
        assert np.allclose(list(rr.covariance), list(o.covariance), rtol=0, atol=TOL), k


def test_bb_mixed_waves(ctx, mini):
    """Matches of at most 7 top nodes each (one per angle): every wave of the
    top level holds several matches, and the score kernel takes its
    per-lane path instead of the wave-uniform one."""
    prm = (4, 0.3, 0.3, 0.02, 20.0) + SCORE_RANGE
    kws = small_scans(mini, np.random.default_rng(1203), 40, prm, 0.2)
    refs = [oracle_bb(**kw) for kw in kws]
    for kw, o in zip(kws, refs):
        assert 2 * o.win[2] + 1 <= 7 and 2 * o.win[0] + 1 < 16
    assert len({len(kw["ranges"]) for kw in kws}) > 3
    for j, (o, kw, ora) in enumerate(zip(gpu_batch(ctx, kws), kws, refs)):
        check(o, kw, f"mixed{j}", ora)


# ------------------------------------------------------------------ argument checks
def test_bb_invalid_arguments_leave_outputs_untouched(ctx, mini):
    """LGS_ERR_INVALID_ARG before any device work; the output records keep their bytes"""
    lib = ctx.lib
    rng = np.random.default_rng(1)
    r, ang, init = draw(mini, rng, 17)
    g = ctx.grid_from_array(mini.cells, mini.mx, mini.my, RES)
    other = ctx.grid_from_array(mini.cells[:, :-1], mini.mx, mini.my, RES)
    sc = ctx.scan(r, ang)
    cost = launcher_cost()
    good = (2, 0.3, 0.3, 0.05, 20.0) + SCORE_RANGE
    pyr = ctx.precompute_pyramid(g, 2)
    parr = (C.c_void_p * 3)(*[p.h for p in pyr])
    bad_parr = (C.c_void_p * 3)(pyr[0].h, other.h, pyr[2].h)
    sarr = (C.c_void_p * 1)(sc.h)
    null_scan = (C.c_void_p * 1)(None)
    poses = (abi.Pose2D * 1)(abi.Pose2D(*init))
    pattern = bytes([0xAB]) * C.sizeof(abi.RtcsmSummary)

    def fresh(T=abi.RtcsmSummary, pat=pattern):
        return T.from_buffer_copy(pat)

    def query(prm):
        out = fresh()
        rc = lib.lgs_bb_optimize_pose_query(ctx.h, g.h, C.byref(abi.BBParams(*prm)), C.byref(cost), sc.h,
                                            abi.Pose2D(*init), C.byref(out))
        return rc, bytes(out) == pattern

    def batch(prm, pa=parr, sa=sarr):
        out = fresh()
        rc = lib.lgs_bb_optimize_pose_batch(ctx.h, g.h, pa, C.byref(abi.BBParams(*prm)), C.byref(cost), sa, poses, 1,
                                            0.3, C.byref(out))
        return rc, bytes(out) == pattern

    lpat = bytes([0xAB]) * C.sizeof(abi.LoopResult)

    def loop(prm, thr, first=0, count=1, scan=sc.h):
        out = fresh(abi.LoopResult, lpat)
        qs = (abi.LoopQuery * 1)(abi.LoopQuery(g.h, None, abi.Pose2D(0, 0, 0), 0, first, count))
        cs = (abi.LoopCandidate * 1)(abi.LoopCandidate(scan, abi.Pose2D(*init), 1, 0))
        rc = lib.lgs_loop_detect_bb(ctx.h, C.byref(abi.BBParams(*prm)), C.byref(cost), thr, qs, 1, cs, 1,
                                    C.byref(out))
        return rc, bytes(out) == lpat

    bad = (LGS_ERR_INVALID_ARG, True)
    for prm in ((-1,) + good[1:], (13,) + good[1:], (2, -0.3) + good[2:], (2, 0.3, -0.3) + good[3:],
                (2, 0.3, 0.3, -0.05) + good[4:]):
        assert query(prm) == bad, prm
        assert batch(prm) == bad, prm
        assert loop(prm, 0.5) == bad, prm
    assert batch(good, pa=bad_parr) == bad            # a pyramid grid of another size
    assert batch(good, sa=null_scan) == bad           # no scan
    assert loop(good, 0.5, scan=None) == bad
    assert loop(good, 0.0) == bad and loop(good, 1.0 + 1e-9) == bad and loop(good, -0.1) == bad
    assert loop(good, 0.5, count=0) == bad            # the queries cover no candidate of one
    assert loop(good, 0.5, first=1, count=0) == bad   # not from the first candidate on
    assert loop(good, 0.5, count=2) == bad            # past the candidates
    # an empty scan cannot be made: lgs_scan_create refuses it and leaves no handle
    one = np.zeros(1)
    hs = abi.ScanHost(abi.dptr(one), abi.dptr(one), 0, abi.Pose2D(0, 0, 0), 0.0, 30.0)
    h = C.c_void_p(0xAB)
    assert lib.lgs_scan_create(ctx.h, C.byref(hs), C.byref(h)) == LGS_ERR_INVALID_ARG and not h.value
    for n_bad in (-1, 13):
        arr = (C.c_void_p * 14)(*([pyr[0].h] * 14))
        assert lib.lgs_grid_precompute_pyramid(ctx.h, g.h, n_bad, arr) == LGS_ERR_INVALID_ARG
    assert lib.lgs_grid_precompute_pyramid(ctx.h, g.h, 2, bad_parr) == LGS_ERR_INVALID_ARG
    # the same calls with good arguments succeed, so the refusals above are the arguments'
    assert query(good)[0] == 0 and batch(good)[0] == 0 and loop(good, 0.5)[0] == 0
