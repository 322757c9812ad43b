"""The map builder (csrc/k_raycast.hip) off 5 cm cells, the origin and square
rooms, against the oracle bit for bit (same_map: geometry, hit/miss counts,
cell values, patch flags).  map_cases.py holds the inputs and the sequences;
test_map_cases_cpu.py checks on the oracle alone that each input reaches the
path it is here for.

Path -> test:
  k_emit's closed-form Bresenham over several 64-lane trips, lengths 64 k +- 1
    in every octant, |dx| == |dy|, dx == 0, dy == 0, a zero-length ray,
    through UpdateGridMap, the device and the host hit points and chunked
    passes                                         test_directed_rays
  cell-bit counts from 8 (2.5 m) to 24 (1 cm) handed to the key sort,
    every builder entry point                      test_matrix_*
  odd w (the constructor's + 0.5 centre offset)    test_matrix_fixed_odd_width
  patch size 1 (mark_patch / k_patch_remap with one flag per cell)
                                                   test_matrix_* [*-1]
  a patch larger than the whole box                test_matrix_* [0.5-300], [2.5-300]
  runs past kShortRun at 0.5 m and 2.5 m           test_matrix_global
  a latest map above kMaxTblCells, both crossings  test_latest_map_across_table_limit
  |coordinates| up to 1e6                          test_far_from_origin, test_all_negative_far_out
  w >> h and h >> w, render_gray on them           test_corridor
  a sensor offset with the scan's range limits binding, device hit points
                                                   test_sensor_offset_and_scan_limits
  more maps in a pass than k_apply's LDS table     test_more_maps_than_lds_table
  angles outside the device sincos domain hand over to the host
                                                   test_headings_*
  a hand-over on a box that starts at cell -k PatchSize (one Resize only)
                                                   test_handover_resizes_once
  a built map at 0.1 m / 0.025 m feeds the correlative matcher
                                                   test_map_grid_feeds_matcher_at_resolution
"""
import ctypes as C

import numpy as np
import pytest

import map_cases as mc
import oracle_bind as ob
from lgs_amd import abi, scene
from test_gpu_raycast import same_map

pytestmark = pytest.mark.gpu


def check(gm, om, tag, full):
    if full:
        same_map(gm, om, tag)
    else:
        assert gm.geometry() == om.geometry(), tag


ENTRIES = ("growth", "window", "append", "maps-dev", "maps-host", "global-dev", "global-host")


def run_entry(entry, case, ctx, ranges):
    """One of the five builder entry points (device hit points on and off
    where the entry has them) on `case`, every step against the oracle."""
    if entry == "growth":
        return mc.run_growth(case, ctx, check)
    if entry == "window":
        return mc.run_window(case, ctx, check)
    if entry == "append":
        return mc.run_append(case, ctx, check)
    if entry.startswith("maps"):
        return mc.run_maps(case, ctx, check, ranges, dev=int(entry == "maps-dev"))
    return mc.run_global(case, ctx, check, dev=int(entry == "global-dev"))


# ---------------------------------------------------------------------------
# 1. directed rays
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("res,ps,centre", mc.DIRECTED_CONFIGS)
@pytest.mark.parametrize("mode", ["update", "maps-dev", "maps-host", "update-chunked", "maps-chunked"])
def test_directed_rays(ctx, res, ps, centre, mode):
    """One scan of chosen beams from the centre of a cell into a new 0x0 map:
    beam i ends at the centre of the cell (dx_i, dy_i) away, the deltas of
    map_cases.directed_deltas (1056 and the zero-length ray).  Grown by
    UpdateGridMap the map has at most 3010 x 3010 cells; rebuilt by
    ConstructMapFromScans from the centres (812.4, -377.7) and (-5000, 5000)
    it reaches to 0 on the negative axis (the DBL_MIN top right): 66e6 and
    42e6 cells, 26 cell bits."""
    case = mc.directed_case(res, ps, centre)
    chunk = mc.DIRECTED_CHUNK if mode.endswith("chunked") else 0
    if mode.startswith("update"):
        mc.run_growth(case, ctx, check, chunk=chunk)
    else:
        mc.run_maps(case, ctx, check, [(0, 0)], dev=int(mode != "maps-host"), chunk=chunk, grown=False)


# ---------------------------------------------------------------------------
# 2. resolution x patch size, every builder entry point
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("res,ps", mc.MATRIX)
def test_matrix(ctx, world, res, ps, entry):
    case = mc.matrix_case(world, res, ps)
    om = run_entry(entry, case, ctx, mc.matrix_ranges(case))
    if entry.startswith("global") and res >= 0.5:
        # as test_long_runs: the wavefront-per-run apply, not the inline short runs
        assert om.hits().max() > mc.K_SHORT_RUN and om.misses().max() >= 10 * mc.K_SHORT_RUN


@pytest.mark.parametrize("res,ps", [c for c in mc.MATRIX if c[1] % 2 == 1])
def test_matrix_fixed_odd_width(ctx, world, res, ps):
    """A map constructed with an odd number of cells (min = centre - (w/2 + 0.5) res)."""
    case = mc.matrix_case(world, res, ps)
    n = mc.odd_cells(res, ps)
    assert n % 2 == 1
    mc.run_fixed(case, ctx, check, n, n)


# ---------------------------------------------------------------------------
# 3. the latest map across kMaxTblCells
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["append", "construct"])
def test_latest_map_across_table_limit(ctx, world, entry):
    """A window of 4 scans at 1 cm whose box starts below 4 Mi cells (ranges
    beyond 4 m skipped), rises above it with four full-range scans (steps
    6-12) and returns below: every step equals the oracle; no step is
    incremental while the latest map is above the limit (the untagged full
    rebuild), at least one is in each phase below it."""
    case = mc.latest_case(world)
    inc = []
    state = {"prev": 0}

    def step(gm, om, tag, full):
        if tag.startswith("local"):
            check(gm, om, tag, full)
            return
        same_map(gm, om, tag)
        k = len(inc)
        cells = om.geometry()["w"] * om.geometry()["h"]
        assert (cells > mc.K_MAX_TBL_CELLS) == mc.latest_above(k), (k, cells)
        rb = gm.rebuilds()
        inc.append(rb["incremental"] - state["prev"])
        state["prev"] = rb["incremental"]
        assert rb["incremental"] + rb["full"] == k + 1, (k, rb)

    if entry == "append":
        mc.run_append(case, ctx, step, win=mc.LATEST_WIN)
    else:
        mc.run_window(case, ctx, step, win=mc.LATEST_WIN)
    assert len(inc) == mc.LATEST_STEPS
    above = [mc.latest_above(k) for k in range(mc.LATEST_STEPS)]
    assert not any(i for i, a in zip(inc, above) if a), inc
    first = above.index(True)
    last = len(above) - 1 - above[::-1].index(True)
    assert sum(inc[:first]) >= 1 and sum(inc[last + 1:]) >= 1, inc


# ---------------------------------------------------------------------------
# 4. far from the origin, far from square
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("res,ps,offset,entry", mc.far_cases())
def test_far_from_origin(ctx, world, res, ps, offset, entry):
    """The room and the trajectory moved by up to 1e6 m: floor((x - min_x) / res)
    on the host and in k_raycells, min_x += (pminx ps) res."""
    case = mc.room_case(world, res, ps, seed=41, offset=offset)
    run_entry(entry, case, ctx, mc.MATRIX_RANGES)


@pytest.mark.parametrize("entry", ["window", "maps-dev", "maps-host", "global-dev"])
def test_all_negative_far_out(ctx, world, entry):
    """Every coordinate negative, 1.5 km out: the map reaches to x = y = 0
    (1.9e7 cells; the DBL_MIN top-right quirk)."""
    case = mc.room_case(world, 0.05, 64, n=4, seed=43, offset=mc.NEGATIVE_OFFSET)
    if entry == "window":
        om = mc.run_window(case, ctx, lambda gm, om, tag, full: check(gm, om, tag, tag == "window3"))
    elif entry.startswith("maps"):
        om = mc.run_maps(case, ctx, check, [(0, 3)], dev=int(entry == "maps-dev"), grown=False)[0]
    else:
        om = mc.run_global(case, ctx, check)
    g = om.geometry()
    assert g["min_x"] + g["w"] * 0.05 > 0.0 and g["min_y"] + g["h"] * 0.05 > 0.0


@pytest.mark.parametrize("along_y", [False, True])
def test_corridor(ctx, along_y):
    """A 60 m x 2 m corridor driven end to end: w >= 6 h along x, h >= 6 w
    along y (a swapped W / H or npx / npy cannot pass both), through the
    global map with device and host hit points, growth and the fused rebuild;
    render_gray of the global map against DrawMap's gray levels."""
    case = mc.corridor_case(along_y)
    keep = {}
    om = mc.run_global(case, ctx, lambda gm, om, tag, full: (check(gm, om, tag, full), keep.update(gm=gm)))
    g = om.geometry()
    assert (g["h"] >= 6 * g["w"]) if along_y else (g["w"] >= 6 * g["h"]), g
    img = keep["gm"].render_gray()
    assert img.shape == (g["h"], g["w"])
    assert np.array_equal(img, mc.gray(om.cells()))
    assert (img == 192).any() and (img < 192).any()
    mc.run_global(case, ctx, check, dev=0)
    mc.run_growth(case, ctx, check)
    mc.run_maps(case, ctx, check, [(0, 9), (8, 20), (21, 28)])


# ---------------------------------------------------------------------------
# 5. sensor offset and the scan's own range limits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_sensor_offset_and_scan_limits(ctx, world, entry):
    """Relative sensor pose (0.2, -0.1, 0.5); scan limits (1.5 m, 8 m) inside
    the builder's (0.01 m, 20 m), beams exactly at all four limits."""
    case = mc.limits_case(world)
    run_entry(entry, case, ctx, mc.MATRIX_RANGES)


# ---------------------------------------------------------------------------
# 6. more maps than k_apply stages in LDS
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [1, 0])
def test_more_maps_than_lds_table(ctx, world, dev):
    """70 maps of one or two nodes in one pass: k_apply finds a key's map in
    the table in global memory."""
    case, ranges = mc.many_maps_case(world)
    assert len(ranges) > mc.K_APPLY_MAPS_LDS
    mc.run_maps(case, ctx, check, ranges, dev=dev, grown=False)


# ---------------------------------------------------------------------------
# 7. angles outside the device sincos domain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("heading", mc.HEADINGS_IN)
def test_headings_inside_domain(ctx, world, heading, entry):
    """Headings of +-1000 rad: gl_sincos on the device, glibc's in the oracle."""
    case = mc.heading_case(world, heading)
    run_entry(entry, case, ctx, mc.MATRIX_RANGES)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("entry", ["maps-dev", "global-dev", "growth", "window", "append", "maps-host"])
def test_headings_outside_domain_hand_over(ctx, world, entry, mixed):
    """Heading 1.06e8: |theta + angle| >= 105414350, outside gl_sincos's domain.
    With device hit points k_hits flags the pass and the host path builds the
    map: the call succeeds and the map is the oracle's (libm's sincos); the
    entry points that take the host hit points at once give the same.  `mixed`
    has two such nodes among six ordinary ones."""
    case = mc.heading_case(world, mc.HEADING_OUT, mixed=mixed)
    run_entry(entry, case, ctx, mc.MATRIX_RANGES)


@pytest.mark.parametrize("entry", ["maps", "global"])
@pytest.mark.parametrize("why", ["no-rays", "chunked"])
def test_handover_resizes_once(ctx, entry, why):
    """A pass the device hit points hand over to the host path (no usable beam
    at all; more keys than the chunk budget) whose box starts on a cell index
    of -k PatchSize: the reference's Resize keeps the patch before that cell,
    a second Resize to the same box would drop it."""
    case = mc.handover_case(why == "chunked")
    chunk = 5 if why == "chunked" else 0
    if entry == "maps":
        mc.run_maps(case, ctx, check, [(0, 1)], dev=1, chunk=chunk, grown=False)
    else:
        mc.run_global(case, ctx, check, dev=1, chunk=chunk)


# ---------------------------------------------------------------------------
# 8. a built map feeds a matcher at another resolution
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("res,n", [(0.1, 200), (0.025, 800)])
def test_map_grid_feeds_matcher_at_resolution(ctx, world, res, n):
    """As test_map_grid_feeds_matcher, off 5 cm: the device map's grid view in
    the correlative matcher, best window and score equal to the oracle's."""
    from conftest import launcher_cost
    ang = scene.beam_angles(361)
    gm = ctx.map(res, 100, n, n)
    om = ob.OMap(res, 100, n, n)
    for p in scene.arc_poses(4):
        r = scene.ray_cast(world, p, ang)
        gm.update_scan(ctx.scan(r, ang), p, abi.BuilderParams(*mc.BP))
        om.integrate(p, ob.OScan(r, ang), ob.BuilderParams(*mc.BP))
    same_map(gm, om)
    r = scene.ray_cast(world, (0.3, 0.2, 0.1), ang)
    params = (5, 0.6, 0.6, 0.3, 20.0)
    gpu = ctx.optimize_pose_query(gm.grid(), abi.RtcsmParams(*params), launcher_cost(), ctx.scan(r, ang),
                                  (0.33, 0.18, 0.12))
    og = ob.OGrid(om.cells(), om.m.min_x, om.m.min_y, res)
    out = ob.Summary()
    ob.lib().orc_rtcsm_optimize_pose_query(C.byref(og.g), C.byref(ob.RtcsmParams(*params)),
                                           C.byref(launcher_cost(oracle=True)), C.byref(ob.OScan(r, ang).s),
                                           ob.Pose(0.33, 0.18, 0.12), C.byref(out))
    assert gpu.pose_found == out.pose_found
    assert list(gpu.best_win) == list(out.best_win) and gpu.score_max == out.score_max
