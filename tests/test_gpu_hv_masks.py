"""GPU tests of the superblock pass's per-thread skips (k_super_hv, k_hv_inzero).

A thread of k_super_hv whose inputs the call's precompute found all +0 loads
nothing (its bit in the set's in-mask, LGS_OPT_HV_INZERO), and a thread whose
maxima are all 0 stores nothing when its previous build of the set left +0
there (its bit in the plane's out-mask, LGS_OPT_ZERO_TILES).  Neither may
change a byte: three contexts run the same calls -- the defaults, one with
LGS_OPT_ZERO_TILES 0 and one with LGS_OPT_HV_INZERO 0 -- and must leave the same
records and bit-identical phase planes and superblock units after every call.
The masks themselves are read back (lgs_debug_item_buffer 10 and 11) and
compared with a numpy restatement: the in-mask must equal the set derived from
the precompute's all-zero tiles exactly and lie inside the truly-zero threads,
the out-mask must equal the threads whose maxima are zero.
"""
import numpy as np
import pytest

from conftest import launcher_cost
from lgs_amd import abi, scene
from test_gpu_batch import _diff, _queries, _record

pytestmark = pytest.mark.gpu

LR = 5
RES = 0.05


# ---- the kernels' index arithmetic, restated -------------------------------------------------
def _win_start(i, n, w):
    return min(i, n - w) if n >= w else 0


class Geom:
    """k_rtcsm.hip super_geom / k_super_hv's thread slots for a W x H map with margin M."""

    def __init__(self, W, H, M, nq):
        self.W, self.H, self.M, self.nq = W, H, M, nq
        self.Wq, self.Hq = (W + LR - 1) // LR, (H + LR - 1) // LR
        self.Wqp, self.Hqp = (self.Wq + 2 * M + 3) & ~3, self.Hq + 2 * M
        self.X4lo = (M - 4) >> 2
        self.ncol = ((M + self.Wq - 1) >> 2) - self.X4lo + 1
        self.qlo = (M - 4) >> 4
        self.nqt = ((M + self.Hq - 1) >> 4) - self.qlo + 1
        self.hgx = (self.ncol * (self.nqt + nq - 1) + 255) // 256
        self.nwv = 4 * self.hgx
        self.NR = 16 * nq + 3

    def threads(self):
        """(slot, qt, X4) of every live thread"""
        for tq in range(256 * self.hgx):
            qi, c = divmod(tq, self.ncol)
            qt = self.qlo + qi - (self.nq - 1)
            if qi < self.nqt + self.nq - 1 and qt >= 0:
                yield tq, qt, self.X4lo + c

    def slot(self, qt, X4):
        return (qt - self.qlo + self.nq - 1) * self.ncol + (X4 - self.X4lo)


def _axis(a, b, M, n, ext, per, nt):
    """hv_zero.hpp hv_axis_range: inclusive tile range of padded cells [a, b], or None"""
    if b < M - 1 or a >= M + n:
        return None
    lo = max(a, M) - M
    hi = min(max(b, M), M + n - 1) - M
    f0, f1 = lo * LR, hi * LR + LR - 1
    if f0 >= ext:
        return None
    f1 = min(f1, ext - 1)
    return f0 // per, min(f1 // per, nt - 1)


def _tile_zero(cells, prows):
    """the precompute's words: tile (ty, tx) read an all-(+0) footprint (bit patterns)"""
    H, W = cells.shape
    pcols = (((257 - LR) // LR) & ~1) * LR
    pgx, pgy = (W + pcols - 1) // pcols, (H + prows - 1) // prows
    nzb = np.ascontiguousarray(cells, dtype=np.float64).view(np.uint64) != 0
    z = np.zeros((pgy, pgx), dtype=bool)
    for ty in range(pgy):
        sy0 = _win_start(ty * prows, H, LR)
        for tx in range(pgx):
            x0 = tx * pcols
            x1 = min(x0 + pcols, W)
            sx0 = _win_start(x0, W, LR)
            fw = _win_start(x1 - 1, W, LR) + LR - sx0
            z[ty, tx] = not nzb[sy0:min(sy0 + prows + LR - 1, H), sx0:min(sx0 + fw, W)].any()
    return z, pcols, pgx, pgy


def expected_inmask(g, cells, prows):
    z, pcols, pgx, pgy = _tile_zero(cells, prows)
    out = np.zeros(g.nwv, dtype=np.uint64)
    for tq, qt, X4 in g.threads():
        ry = _axis(16 * qt, 16 * qt + 16 * g.nq + 2, g.M, g.Hq, g.H, prows, pgy)
        rx = _axis(4 * X4, 4 * X4 + 6, g.M, g.Wq, g.W, pcols, pgx)
        if ry is None or rx is None or z[ry[0]:ry[1] + 1, rx[0]:rx[1] + 1].all():
            out[tq >> 6] |= np.uint64(1) << np.uint64(tq & 63)
    return out


def _strip_clamped_nonzero(g, planes):
    """per plane: which cells of the strip-clamped copy V are not +0 (k_super_hv's comment)"""
    M = g.M
    nz = planes[:LR * LR * g.Hqp * g.Wqp].reshape(LR * LR, g.Hqp, g.Wqp).view(np.uint64) != 0   # (the buffer is padded)
    out = []
    for p in range(LR * LR):
        ry, rx = divmod(p, LR)
        a = nz[p].copy()
        if ry > 0:
            a[M - 1, :] = nz[rx][M, :]
        if rx > 0:
            a[:, M - 1] = nz[ry * LR][:, M]
        if rx > 0 and ry > 0:
            a[M - 1, M - 1] = nz[0][M, M]
        out.append(a)
    return out


def expected_outmask_and_true_zero(g, planes):
    """out-mask: bit = the thread's maxima in that plane are all 0; true zero: in every plane"""
    V = _strip_clamped_nonzero(g, planes)
    out = np.zeros((LR * LR, g.nwv), dtype=np.uint64)
    tz = np.zeros(g.nwv, dtype=np.uint64)
    for tq, qt, X4 in g.threads():
        bit = np.uint64(1) << np.uint64(tq & 63)
        allz = True
        for p in range(LR * LR):
            z = not V[p][16 * qt:min(16 * qt + g.NR, g.Hqp), 4 * X4:4 * X4 + 7].any()
            if z:
                out[p, tq >> 6] |= bit
            allz = allz and z
        if allz:
            tz[tq >> 6] |= bit
    return out, tz


def _margin(planes_len, W, H):
    """the plan's margin M (a multiple of 4) from the size of the planes buffer"""
    Wq, Hq = (W + LR - 1) // LR, (H + LR - 1) // LR
    found = [M for M in range(4, 200, 4)
             if (8 * LR * LR * ((Wq + 2 * M + 3) & ~3) * (Hq + 2 * M) + 255) // 256 * 256 == 8 * planes_len]
    assert len(found) == 1, found
    return found[0]


def _popcount(words):
    return sum(bin(int(w)).count("1") for w in np.asarray(words).ravel())


# ---- three contexts on the same calls ------------------------------------------------------
@pytest.fixture(scope="module")
def others():
    nozt, noin = abi.Context(0), abi.Context(0)
    nozt.set_option(abi.LGS_OPT_ZERO_TILES, 0)
    noin.set_option(abi.LGS_OPT_HV_INZERO, 0)
    yield nozt, noin
    nozt.close()
    noin.close()


@pytest.fixture(scope="module")
def queries(world):
    rng = np.random.default_rng(77)
    return {nb: _queries(world, rng, 6, nb, jitter=(0.1, 0.1, 0.1)) for nb in (181, 361, 541)}


def run_calls(ctx, others, queries, maps, calls, n_beams=181, window=1.0, nq=1, check_masks=True):
    """Every call on the three contexts; bytes compared after each; the default context's masks
    compared with the restatement.  Returns, per call and item, (in-mask, out-mask, Geom)."""
    nozt, noin = others
    ang, qs = queries[n_beams]
    P, cost = abi.RtcsmParams(LR, 2.0 * window, 2.0 * window, 0.25, 20.0), launcher_cost()   # ranges are full widths
    inits = [i for _, i in qs]
    state = []
    for cx in (ctx, nozt, noin):
        grids = {k: cx.grid_from_array(v, -0.5 * v.shape[1] * RES, -0.5 * v.shape[0] * RES, RES) for k, v in maps.items()}
        state.append((cx, grids, [cx.scan(r, ang) for r, _ in qs]))
    seen = []
    for step, names in enumerate(calls):
        n = len(names)
        res = []
        for cx, grids, scans in state:
            if n == 1:
                out = [cx.optimize_pose_query(grids[names[0]], P, cost, scans[0], inits[0])]
            else:
                out = cx.optimize_pose_query_batch([grids[k] for k in names], P, cost, scans[:n], inits[:n])
            recs = [_record(o) for o in out]
            bufs = [{b: cx.debug_buffer(b, j) for b in ("planes", "super", "hv_inmask", "hv_outmask")} for j in range(n)]
            res.append((recs, bufs))
        (r0, b0), (r1, b1), (r2, b2) = res
        assert r0 == r1, (step, "zero tiles off", _diff(r0, r1))
        assert r0 == r2, (step, "in-masks off", _diff(r0, r2))
        per_item = []
        for j in range(n):
            for other in (b1, b2):
                for name in ("planes", "super"):
                    u, v = b0[j][name], other[j][name]
                    assert u.size > 0 and u.shape == v.shape and np.array_equal(u.view(np.uint8), v.view(np.uint8)), \
                        (step, j, names[j], name, int(np.argmax(u.view(np.uint8) != v.view(np.uint8))))
            assert b1[j]["hv_inmask"].size == 0 and b1[j]["hv_outmask"].size == 0    # no zero tiles: no masks
            assert b2[j]["hv_inmask"].size == 0 and b2[j]["hv_outmask"].size > 0     # no in-masks: out-masks only
            cells = maps[names[j]]
            H, W = cells.shape
            g = Geom(W, H, _margin(len(b0[j]["planes"]), W, H), nq)
            inm, outm = b0[j]["hv_inmask"], b0[j]["hv_outmask"].reshape(LR * LR, -1)
            assert outm.shape == (LR * LR, g.nwv), (step, j, outm.shape, g.nwv)
            assert np.array_equal(outm, b2[j]["hv_outmask"].reshape(LR * LR, -1)), (step, j, "out-masks differ")
            if W % LR or H % LR:
                assert inm.size == 0, (step, j, "a map the batched precompute does not write took an in-mask")
            elif n == 1:
                assert inm.size == 0, (step, "a lone call took an in-mask (its pre-pass costs more than it saves)")
            else:
                assert inm.shape == (g.nwv,), (step, j, inm.shape, g.nwv)
            if check_masks:
                want_out, true_zero = expected_outmask_and_true_zero(g, b0[j]["planes"])
                assert np.array_equal(outm, want_out), (step, j, names[j], "out-mask")
                if inm.size:
                    want_in = expected_inmask(g, cells, 8)   # a batch's 8-row precompute tiles
                    assert np.array_equal(inm, want_in), (step, j, names[j], "in-mask", [hex(int(x)) for x in inm],
                                                          [hex(int(x)) for x in want_in])
                    assert not np.any(inm & ~true_zero), (step, j, names[j], "in-mask bit of a thread with a nonzero input")
            per_item.append((inm, outm, g))
        seen.append(per_item)
    return seen


def _zeros(n=300):
    return np.zeros((n, n))


def _blob(n=300):
    m = _zeros(n)
    m[n - 40:n - 22, n - 36:n - 20] = 0.7
    return m


def test_all_zero_map_and_blob_only_map(ctx, others, queries):
    """Nothing to load on an empty map: every live thread's in-bit and out-bits are set.  With one
    blob in a corner more than half of the threads still load nothing."""
    maps = {"z": _zeros(), "blob": _blob()}
    seen = run_calls(ctx, others, queries, maps, [["z", "z", "z"], ["z", "blob", "z", "blob"], ["blob", "blob", "z"]])
    inm, outm, g = seen[0][0]
    live = sum(1 for _ in g.threads())
    assert live > 64                                  # more than one wave
    assert _popcount(inm) == live and _popcount(outm) == LR * LR * live
    for inm, outm, g in (seen[1][1], seen[2][0]):
        assert live // 2 < _popcount(inm) < live, (_popcount(inm), live)
        assert _popcount(outm) < LR * LR * live


def test_one_cell_at_the_extremes_of_a_footprint(ctx, others, queries):
    """One nonzero cell in the first / last padded row and column of one thread's footprint, and
    just outside each: the thread's out-bits are clear in every plane for the former and set for
    the latter, whatever the map of the set's previous build was."""
    n = 300
    probe = Geom(n, n, 12, 1)   # (the margin is checked against the planes buffer in run_calls)
    qt, X4 = 2, 8
    # padded rows 16 qt .. + 18, columns 4 X4 .. + 6 -> coarse cells -> the last fine cell of each window
    ylo, yhi = LR * (16 * qt - probe.M), LR * (16 * qt + 18 - probe.M)
    xlo, xhi = LR * (4 * X4 - probe.M), LR * (4 * X4 + 6 - probe.M)
    ymid, xmid = (ylo + yhi) // 2, (xlo + xhi) // 2
    inside = {"top": (ylo + LR - 1, xmid), "bottom": (yhi + LR - 1, xmid), "left": (ymid, xlo + LR - 1),
              "right": (ymid, xhi + LR - 1)}
    outside = {"above": (ylo - 1, xmid), "below": (yhi + 2 * LR - 1, xmid), "before": (ymid, xlo - 1),
               "after": (ymid, xhi + 2 * LR - 1)}
    maps = {}
    for k, (y, x) in {**inside, **outside}.items():
        maps[k] = _zeros(n)
        maps[k][y, x] = 0.6
    calls = [["top", "above", "bottom", "below"], ["left", "before", "right", "after"],
             ["above", "top", "below", "bottom"], ["before", "left", "after", "right"]]
    seen = run_calls(ctx, others, queries, maps, calls)
    for names, items in zip(calls, seen):
        for name, (inm, outm, g) in zip(names, items):
            assert g.M == probe.M
            tq = g.slot(qt, X4)
            bits = (outm[:, tq >> 6] >> np.uint64(tq & 63)) & np.uint64(1)
            assert np.all(bits == (0 if name in inside else 1)), (name, bits)
            assert not (int(inm[tq >> 6]) >> (tq & 63)) & 1 or name in outside


def test_map_edges_strips_and_flagged_cells(ctx, others, queries):
    """Cells at (0, 0) and in the last row and column (the strip clamp reads the map's first coarse
    row and column), a -0.0 cell (not +0: its tile and threads are built) and a cell above 1 (the
    set's flag is still raised: the records say so in all three contexts)."""
    n = 320
    first, last, both, negz, over = _zeros(n), _zeros(n), _zeros(n), _zeros(n), _zeros(n)
    first[0, 0] = 0.5
    last[n - 1, n - 1] = 0.5
    both[0, 0] = both[n - 1, n - 1] = both[0, n - 1] = both[n - 1, 0] = 0.4
    negz[100, 40] = -0.0
    negz[200:210, 200:210] = 0.5
    over[30, 290] = 1.5
    over[200:210, 200:210] = 0.5
    maps = {"first": first, "last": last, "both": both, "negz": negz, "over": over, "z": _zeros(n)}
    run_calls(ctx, others, queries, maps, [["first", "last", "both"], ["last", "both", "first"], ["z", "first", "z"]],
              n_beams=361)
    # the restated masks assume nonnegative cells; the bytes and records are compared all the same
    run_calls(ctx, others, queries, maps, [["negz", "over", "z"], ["z", "negz", "over"], ["over", "z", "negz"]],
              n_beams=361, check_masks=False)


def test_sets_that_switch_maps_grow_shrink_and_a_lone_query(ctx, others, queries, world):
    """A set's out-bit goes stale when its map changes (a zero thread must store once, then skip
    again); calls with more and fewer sets than the one before; a lone query between batches (its
    own precompute tiling, 4-row tiles: the tile words change layout, and it takes no in-mask); a
    map with a room in it."""
    from test_gpu_rtcsm import build_map
    built, _, _ = build_map(world, 300, RES, 100, scene.arc_poses(3), n_beams=181)
    room = _zeros()   # (the builder rounds its map up to whole patches: cut to the other maps' size)
    h, w = min(300, built.shape[0]), min(300, built.shape[1])
    room[:h, :w] = built[:h, :w]
    assert np.count_nonzero(room) > 1000
    other = _zeros()
    other[20:40, 30:200] = 0.8
    maps = {"z": _zeros(), "blob": _blob(), "room": room, "other": other}
    calls = [["blob", "z", "room"], ["z", "blob", "other"], ["blob", "z", "room"], ["room"], ["other", "room", "z", "blob", "z", "room"],
             ["blob"], ["z", "other", "blob"], ["room", "room", "room", "z"], ["blob", "z", "room"]]
    seen = run_calls(ctx, others, queries, maps, calls, n_beams=541)
    assert seen[3][0][0].size == 0 and seen[3][0][1].size > 0   # the lone query: out-masks, no in-mask
    assert _popcount(seen[4][2][0]) > 0                          # and the batch after it skips loads again


def test_units_stored_whole(ctx, others, queries):
    """LGS_OPT_HV_FULL 1: two quads per thread (35-row footprints), units stored whole."""
    nozt, noin = others
    maps = {"z": _zeros(), "blob": _blob()}
    edge = _zeros()
    edge[0, 0] = edge[299, 299] = 0.5
    maps["edge"] = edge
    try:
        for cx in (ctx, nozt, noin):
            cx.set_option(abi.LGS_OPT_HV_FULL, 1)
        seen = run_calls(ctx, others, queries, maps, [["blob", "z", "edge"], ["z", "edge", "blob"], ["edge"], ["blob", "z", "edge"]],
                         nq=2)
        inm, _, g = seen[0][0]
        assert _popcount(inm) > sum(1 for _ in g.threads()) // 2
    finally:
        for cx in (ctx, nozt, noin):
            cx.set_option(abi.LGS_OPT_HV_FULL, 0)


def test_wide_window_and_odd_map_size(ctx, others, queries):
    """A +-2.5 m window (12-row units: a quad's rows go to three units).  A map whose size is no
    multiple of LowRes is not written by the batched precompute: no in-mask, every thread loads."""
    maps = {"z": _zeros(320), "blob": _blob(320)}
    edge = _zeros(320)
    edge[0, 0] = edge[319, 319] = 0.5
    maps["edge"] = edge
    seen = run_calls(ctx, others, queries, maps, [["blob", "z", "edge"], ["edge", "blob", "z"], ["blob", "z", "edge"]],
                     n_beams=361, window=2.5)
    assert seen[0][0][2].M >= 24
    odd = {"z": _zeros(303), "blob": _blob(303)}
    seen = run_calls(ctx, others, queries, odd, [["blob", "z", "blob"], ["z", "blob", "z"]])
    assert all(inm.size == 0 for items in seen for inm, _, _ in items)
