"""The inputs of test_gpu_map_shapes.py, built with the oracle alone: each
case must still reach the builder path it was written for (map_cases.py holds
the inputs and the sequences; no GPU here)."""
import numpy as np
import pytest

import map_cases as mc
import oracle_bind as ob


def _none(gm, om, tag, full):
    pass


def test_directed_delta_set():
    d = mc.directed_deltas()
    assert len(d) == len(set(d)) == 1057 and d[0] == (0, 0)      # 1056 deltas and the zero-length ray
    for M in mc.DIRECTED_MAJOR:
        for m in {0, 1, 2, M // 3, M // 2, M - 2, M - 1, M}:
            if 0 <= m <= M:
                for sa in (1, -1):
                    for sb in (1, -1):
                        assert (sa * M, sb * m) in d and (sa * m, sb * M) in d
    # every multiple of the 64-lane trip +- 1, the tie |dx| == |dy|, both axes
    assert {(63, 0), (64, 0), (65, 0), (0, -128), (129, 129), (-257, 257), (1000, 999), (-999, 1000)} <= set(d)


@pytest.mark.parametrize("res,ps,centre", mc.DIRECTED_CONFIGS)
@pytest.mark.parametrize("entry", ["update", "construct"])
def test_directed_deltas_realised(res, ps, centre, entry):
    """Every intended delta is realised: the oracle counts a hit in the cell
    (dx, dy) from the sensor's for every beam, and as many hits as beams; no
    beam is filtered; the sensor sits at the centre of its cell."""
    case = mc.directed_case(res, ps, centre)
    lo, hi = case.limits()
    assert case.usable(0).all() and lo == res / 4 and hi == 400.0
    if entry == "update":
        om = mc.run_growth(case, None, _none)
    else:
        om = mc.run_maps(case, None, _none, [(0, 0)], grown=False)[0]
    g = om.geometry()
    fx = (case.poses[0][0] - g["min_x"]) / res
    fy = (case.poses[0][1] - g["min_y"]) / res
    assert abs(fx - np.floor(fx) - 0.5) < 1e-9 and abs(fy - np.floor(fy) - 0.5) < 1e-9, (fx, fy)
    sx, sy = int(np.floor(fx)), int(np.floor(fy))
    hits = om.hits()
    d = np.array(mc.directed_deltas())
    assert (hits[sy + d[:, 1], sx + d[:, 0]] >= 1).all()
    assert int(hits.sum()) == len(d)
    # grown by Expand the map is square; ConstructMapFromScans' DBL_MIN top right makes it reach
    # to 0 from the two centres with a negative coordinate (42e6 and 66e6 cells)
    assert g["w"] * g["h"] <= (3010 * 3010 if entry == "update" else 70_000_000)
    # rays of 1000 cells: 16 trips through k_emit's 64-lane loop
    assert max(g["w"], g["h"]) > 2000


def test_directed_chunk_splits_the_scan():
    keys = sum(max(abs(dx), abs(dy)) + 1 for dx, dy in mc.directed_deltas())
    assert keys > 3 * mc.DIRECTED_CHUNK


def test_matrix_reaches_its_paths(world):
    """Over the resolution x patch size matrix: cell-bit counts from 8 to 24,
    rays of 1000 cells and more at 0.01, patch size 1, a patch larger than the
    whole box, odd widths, and at 0.5 / 2.5 runs past kShortRun."""
    assert len(mc.MATRIX) == 22
    bits = set()
    for res, ps in mc.MATRIX:
        case = mc.matrix_case(world, res, ps)
        assert 6 <= len(case.poses) <= 12 and 91 <= len(case.angles) <= 181
        ranges = mc.matrix_ranges(case)
        assert 3 <= len(ranges) <= 4 and all(0 <= a <= b < len(case.poses) for a, b in ranges)
        assert any(a2 <= b1 for (_, b1), (a2, _) in zip(ranges, ranges[1:]))   # overlapping
        om = mc.run_global(case, None, _none)
        g = om.geometry()
        bits.add(mc.cell_bits(om))
        assert g["w"] * g["h"] <= mc.MAX_CELLS
        if ps == 300 and res >= 0.1:
            # the patch (30 m and more) is larger than the box (the 24 m room)
            assert ps * res > 24.0 and g["npx"] <= 2 and g["npy"] <= 2
        if ps == 1:
            assert g["npx"] == g["w"] and g["npx"] * g["npy"] > 10000 * (res < 0.1)
        if res == 0.01:
            sx, sy, hx, hy = case.ray_cells(0, g)
            assert max(np.abs(hx - sx).max(), np.abs(hy - sy).max()) >= 1000
        if res >= 0.5:
            assert om.hits().max() > mc.K_SHORT_RUN and om.misses().max() >= 10 * mc.K_SHORT_RUN, \
                (res, ps, om.hits().max(), om.misses().max())
        if res in (0.01, 2.5) and ps == 7:
            gr = mc.run_growth(case, None, _none)
            bits.add(mc.cell_bits(gr))
        if ps % 2 == 1:
            n = mc.odd_cells(res, ps)
            fx = ob.OMap(res, ps, n, n)
            assert fx.geometry()["w"] == n and n % 2 == 1
    assert min(bits) <= 8 and max(bits) >= 24, sorted(bits)


def test_latest_map_crosses_the_table_limit(world):
    """Which steps of the latest-map sequence lie above kMaxTblCells: steps
    6-12 (the window holds a full-range scan), below before and after, and in
    each phase below the geometry holds over consecutive steps (the condition
    for an incremental step)."""
    case = mc.latest_case(world)
    assert len(case.poses) == mc.LATEST_STEPS
    cells, geoms = [], []

    def see(gm, om, tag, full):
        g = om.geometry()
        cells.append(g["w"] * g["h"])
        geoms.append(g)

    mc.run_window(case, None, see, win=mc.LATEST_WIN)
    above = [c > mc.K_MAX_TBL_CELLS for c in cells]
    assert above == [mc.latest_above(k) for k in range(mc.LATEST_STEPS)]
    assert above == [False] * 6 + [True] * 7 + [False] * 6
    assert max(cells) <= mc.MAX_CELLS
    for phase in (range(1, 6), range(14, 19)):
        assert any(geoms[k] == geoms[k - 1] for k in phase)
    # the same windows through AppendScan
    cells2 = []
    mc.run_append(case, None, lambda gm, om, tag, full: tag.startswith("latest") and cells2.append(
        om.geometry()["w"] * om.geometry()["h"]), win=mc.LATEST_WIN)
    assert [c > mc.K_MAX_TBL_CELLS for c in cells2] == above


def test_far_offsets_keep_the_room(world):
    """The moved room gives the scans of the room at the origin (to the
    rounding of the larger coordinates) and a map that far out; every offset
    of the issue runs through growth, and the window's map can be allocated."""
    cases = mc.far_cases()
    assert {(r, p, o) for r, p, o, e in cases if e == "growth"} == \
        {(r, p, o) for r, p in mc.FAR_CONFIGS for o in mc.FAR_OFFSETS}
    assert max(max(abs(o[0]), abs(o[1])) for _, _, o, e in cases if e == "window") >= 1.0e6
    for res, ps, offset, entry in cases:
        if entry not in ("growth", "window"):
            continue
        case = mc.room_case(world, res, ps, seed=41, offset=offset)
        near = mc.room_case(world, res, ps, seed=41)
        for a, b in zip(case.ranges, near.ranges):
            assert np.abs(a - b).max() < 1e-6
        if entry == "window":
            om = mc.run_window(case, None, _none)
            g = om.geometry()
            assert g["w"] * g["h"] <= mc.MAX_CELLS, (res, ps, offset, g)
            assert g["min_x"] <= offset[0] - 10 and g["min_y"] <= offset[1] - 10


def test_negative_case_reaches_the_origin(world):
    """All coordinates negative: the box's top right stays at DBL_MIN, so the
    oracle's map runs from the scans to x = y = 0, under 2e7 cells."""
    case = mc.room_case(world, 0.05, 64, seed=43, offset=mc.NEGATIVE_OFFSET)
    for k in range(len(case.poses)):
        sx, sy, st = case.sensor(k)
        u = case.usable(k)
        assert (sx + case.ranges[k][u] * np.cos(st + case.angles[u])).max() < 0
        assert (sy + case.ranges[k][u] * np.sin(st + case.angles[u])).max() < 0
    om = mc.run_window(case, None, _none)
    g = om.geometry()
    assert g["min_x"] + g["w"] * 0.05 > 0.0 and g["min_y"] + g["h"] * 0.05 > 0.0
    assert g["min_x"] < -1512.0 and g["min_y"] < -26.0
    assert 1.5e7 < g["w"] * g["h"] < mc.MAX_CELLS
    assert g["w"] > 40 * g["h"]


@pytest.mark.parametrize("along_y", [False, True])
def test_corridor_aspect(along_y):
    case = mc.corridor_case(along_y)
    om = mc.run_global(case, None, _none)
    g = om.geometry()
    if along_y:
        assert g["h"] >= 6 * g["w"], g
    else:
        assert g["w"] >= 6 * g["h"], g
    assert om.hits().sum() > 1000
    img = mc.gray(om.cells())
    assert (img == 192).any() and (img < 192).any()


def test_scan_limits_bind(world):
    """The scan's range limits are the binding ones: beams the builder's
    limits alone would accept lie on and outside the scan's on both sides, and
    the oracle counts exactly the beams strictly inside the scan's limits."""
    case = mc.limits_case(world)
    lo, hi = case.limits()
    assert (lo, hi) == (mc.SCAN_MIN, mc.SCAN_MAX) and mc.BP[0] < lo and hi < mc.BP[1]
    assert case.rel == mc.REL
    total = 0
    for k, r in enumerate(case.ranges):
        assert (r == lo).any() and (r == hi).any() and (r == mc.BP[0]).any() and (r == mc.BP[1]).any()
        assert ((r > mc.BP[0]) & (r < lo)).any() and ((r > hi) & (r < mc.BP[1])).any()
        u = case.usable(k)
        assert np.array_equal(u, (r > lo) & (r < hi)) and u.sum() > 20
        total += int(u.sum())
    om = mc.run_global(case, None, _none)
    assert int(om.hits().sum()) == total


def test_many_maps_exceed_the_lds_table(world):
    case, ranges = mc.many_maps_case(world)
    assert len(ranges) == mc.MANY_MAPS > mc.K_APPLY_MAPS_LDS
    assert {b - a + 1 for a, b in ranges} == {1, 2} and ranges[-1][1] == len(case.poses) - 1
    beams = {int(case.usable(k).sum()) for k in range(len(case.poses))}
    assert len(case.angles) == 61 and min(beams) >= 1 and max(beams) <= 61
    assert any(b <= 31 for b in beams) and any(b > 31 for b in beams)
    oms = mc.run_maps(case, None, _none, ranges, grown=False)
    assert all(om.hits().sum() > 0 for om in oms)


@pytest.mark.parametrize("heading", mc.HEADINGS_IN + (mc.HEADING_OUT,))
def test_headings_and_the_sincos_domain(world, heading):
    case = mc.heading_case(world, heading)
    th = np.array([[case.sensor(k)[2] + a for a in case.angles] for k in range(len(case.poses))])
    if heading == mc.HEADING_OUT:
        assert (np.abs(th) >= mc.SINCOS_DOMAIN).all()
        mixed = mc.heading_case(world, heading, mixed=True)
        out = [abs(p[2]) >= mc.SINCOS_DOMAIN for p in mixed.poses]
        assert sum(out) == 2 and not out[0]
    else:
        assert (np.abs(th) < mc.SINCOS_DOMAIN).all() and (np.abs(th) > 900).all()
    # the scans still see the room: the oracle's map has its walls
    om = mc.run_global(case, None, _none)
    assert om.hits().sum() > 500


@pytest.mark.parametrize("usable", [False, True])
def test_handover_case_sits_on_a_patch_multiple(usable):
    """The box starts on cells (-16, -32) of patches of 16: the oracle's one
    Resize keeps the patch before them (three by four patches up to the
    origin's), a second Resize to the same box would not."""
    case = mc.handover_case(usable)
    assert int(case.usable(0).sum()) == (8 if usable else 0)
    om = mc.run_maps(case, None, _none, [(0, 1)], grown=False)[0]
    g = om.geometry()
    assert (g["npx"], g["npy"]) == (3, 4) and g["min_x"] == -32 * 0.05 and g["min_y"] == -48 * 0.05
    sx, sy, _, _ = case.ray_cells(0, g)
    assert (sx, sy) == (16, 16)        # a whole patch lies before the sensor's on both axes
    assert int(om.hits().sum()) == (16 if usable else 0)
