"""Certified fast rows and packed gathers of the superblock pass (k_super_oct,
LGS_OPT_FAST_ROWS).

A lean batch's superblock pass forms its hit-point cells with a shorter fp64
chain wherever a whole wave's cells are certified equal to the exact chain's
and unguarded, and gathers the superblock units through packed row entries.
Nothing it writes may change: every case below runs the same batch three ways
-- fast rows on, fast rows off (the exact chain in the same kernel), lean off
(rows materialised by k_project) -- and compares the records and the
sbound / part_c / part_k / tedge buffers of every item bit for bit.

The valid-beam counts straddle a beam slot row (12 beams of a 5-column
window per wave instruction), a pipeline batch (8 x 12 = 96), the four waves'
deal (4 x 96 = 384) and a full scan (1081); both window classes run (5 x 5
superblocks: 8-row units; 6 x 6: 12-row units, the loop detector's window).
"""
import numpy as np
import pytest

from conftest import launcher_cost
from lgs_amd import abi
from test_gpu_batch import _diff, _record

pytestmark = pytest.mark.gpu

N = 240                                          # map cells per side, 5 cm
WIN5 = (5, 4.0, 4.0, 1.0471976, 20.0)            # 5 x 5 superblocks (bench.py config 2's window)
WIN9 = (5, 5.0, 5.0, 1.0, 20.0)                  # 6 x 6 superblocks (the loop detector's window)
BUFS = ("sbound", "part_c", "part_k", "tedge")


@pytest.fixture(scope="module")
def cells():
    """Occupancy with walls, blobs and empty space (values in [0, 1])."""
    rng = np.random.default_rng(42)
    c = np.where(rng.random((N, N)) < 0.08, rng.random((N, N)), 0.0)
    c[40:200, 60] = 0.9
    c[40, 60:180] = 0.8
    c[199, 60:180] = 0.95
    c[100:140, 150:153] = rng.random((40, 3))
    c[0:3, :] = 0.7                                # occupied cells on the low edges
    c[:, 0:3] = 0.6
    return c


def _scans(rng, nv, n=3, rmax=5.0):
    ang = np.linspace(-2.3, 2.3, nv) if nv > 1 else np.array([0.3])
    return ang, [rng.uniform(0.3, rmax, nv) for _ in range(n)]


def _run(ctx, g, P, ds, inits, lean, fast, inject=0, geps=1e-9):
    ctx.set_option(abi.LGS_OPT_LEAN_PROJECT, lean)
    ctx.set_option(abi.LGS_OPT_FAST_ROWS, fast)
    ctx.set_option(abi.LGS_OPT_POISON_WS, 1)
    ctx.set_option(abi.LGS_OPT_INJECT_INDEX, inject)
    ctx.set_option(abi.LGS_OPT_GUARD_EPS, geps)
    try:
        out = ctx.optimize_pose_query_batch(g, P, launcher_cost(), ds, inits)
        bufs = None
        if not inject:   # (a forced fix-up reruns its item: the buffers are then the rerun's)
            bufs = [{b: ctx.debug_buffer(b, j) for b in BUFS} for j in range(len(ds))]
            # the batch did run lean: no (angle, beam) row was written (a
            # host rerun of an item -- the exact dense path -- materialises rows)
            if lean and not any(o.slow_path or o.fixups for o in out):
                assert (ctx.debug_buffer("cbase", 0).view(np.uint8) == 0xFF).all()
        return out, bufs
    finally:
        ctx.set_option(abi.LGS_OPT_LEAN_PROJECT, 1)
        ctx.set_option(abi.LGS_OPT_FAST_ROWS, 1)
        ctx.set_option(abi.LGS_OPT_POISON_WS, 0)
        ctx.set_option(abi.LGS_OPT_INJECT_INDEX, 0)
        ctx.set_option(abi.LGS_OPT_GUARD_EPS, 1e-9)


def _three_ways(ctx, cells, origin, params, ang, ranges, inits, **kw):
    """fast rows on / off / lean off: identical records and buffers; returns the fast run"""
    g = ctx.grid_from_array(cells, origin[0], origin[1], 0.05)
    P = abi.RtcsmParams(*params)
    ds = [ctx.scan(r, ang) for r in ranges]
    runs = [_run(ctx, g, P, ds, inits, lean, fast, **kw) for lean, fast in ((1, 1), (1, 0), (0, 1))]
    recs = [[_record(o) for o in out] for out, _ in runs]
    for k, name in ((1, "fast rows off"), (2, "lean off")):
        assert recs[0] == recs[k], (name, _diff(recs[0], recs[k]))
        if runs[0][1] is None:
            continue
        for j, (a, b) in enumerate(zip(runs[0][1], runs[k][1])):
            for buf in BUFS:
                assert a[buf].shape == b[buf].shape and np.array_equal(a[buf].view(np.uint8), b[buf].view(np.uint8)), \
                    (name, j, buf)
    return runs[0]


def _inits(rng, origin, n=3):
    return [(origin[0] + rng.uniform(3.0, 9.0), origin[1] + rng.uniform(3.0, 9.0), rng.uniform(-np.pi, np.pi))
            for _ in range(n)]


@pytest.mark.parametrize("params", [WIN5, WIN9], ids=["win5", "win9"])
@pytest.mark.parametrize("nv", [1, 11, 12, 13, 95, 96, 97, 385])
def test_fast_rows_beam_counts(ctx, cells, params, nv):
    rng = np.random.default_rng(1000 + nv)
    origin = (-6.0, -6.0)
    ang, ranges = _scans(rng, nv)
    out, _ = _three_ways(ctx, cells, origin, params, ang, ranges, _inits(rng, origin))
    assert all(o.guard_hits == 0 for o in out)


def test_fast_rows_full_scan(ctx, cells):
    rng = np.random.default_rng(7)
    origin = (-6.0, -6.0)
    ang, ranges = _scans(rng, 1081)
    out, _ = _three_ways(ctx, cells, origin, WIN5, ang, ranges, _inits(rng, origin))
    assert all(o.guard_hits == 0 for o in out)


@pytest.mark.parametrize("params", [WIN5, WIN9], ids=["win5", "win9"])
def test_fast_rows_far_origin(ctx, cells, params):
    """A map origin at (8192, -4096): the error bound grows with |s| + |min|."""
    rng = np.random.default_rng(11)
    origin = (8192.0, -4096.0)
    ang, ranges = _scans(rng, 97)
    out, _ = _three_ways(ctx, cells, origin, params, ang, ranges, _inits(rng, origin))
    assert all(o.guard_hits == 0 for o in out)


def test_fast_rows_low_edges(ctx, cells):
    """Poses against the map's low edges: coarse lattices start left of /
    below the map, the angles' edge flags (tedge) get set."""
    rng = np.random.default_rng(13)
    origin = (-6.0, -6.0)
    ang, ranges = _scans(rng, 97, rmax=2.0)
    inits = [(-5.6, -5.7, 0.4), (-5.9, -2.0, -2.0), (-1.0, -5.8, 3.0)]
    _, bufs = _three_ways(ctx, cells, origin, WIN5, ang, ranges, inits)
    assert all(b["tedge"].any() for b in bufs)


def test_fast_rows_window_misses_map(ctx, cells):
    """Every beam's coarse window misses the map: base 0 (all-zero units) everywhere."""
    rng = np.random.default_rng(17)
    origin = (-6.0, -6.0)
    ang, ranges = _scans(rng, 97)
    inits = [(60.0, 70.0, 0.1), (-80.0, -6.0, 1.0), (0.0, 40.0, -1.0)]
    out, bufs = _three_ways(ctx, cells, origin, WIN5, ang, ranges, inits)
    assert all(o.pose_found == 0 for o in out)
    assert all((b["sbound"] == 0.0).all() for b in bufs)


def test_fast_rows_boundary_hits(ctx, cells):
    """Hit points exactly on cell boundaries (the sensor on a cell corner,
    axis-aligned beams of a whole number of cells at the central search
    angle): guarded by the exact chain, so never certain -- the same guard
    hits on every side."""
    origin = (-6.0, -6.0)
    ang = np.array([0.0, np.pi / 2, -np.pi / 2, np.pi] * 6 + [0.7, -1.1, 2.0])
    ranges = [np.array([0.05 * k for k in range(20, 44)] + [1.3, 2.2, 0.9]) for _ in range(3)]
    inits = [(-1.0, -2.0, 0.0), (-3.0, -1.5, 0.0), (-2.0, -2.5, 0.0)]
    out, _ = _three_ways(ctx, cells, origin, WIN5, ang, ranges, inits)
    assert all(o.guard_hits > 0 for o in out)


def test_fast_rows_nan_range(ctx, cells):
    """A NaN range passes the valid-beam filter (!(r >= rmax)): never certain."""
    rng = np.random.default_rng(19)
    origin = (-6.0, -6.0)
    ang, ranges = _scans(rng, 97)
    for r in ranges:
        r[40] = np.nan
    _three_ways(ctx, cells, origin, WIN5, ang, ranges, _inits(rng, origin))


@pytest.mark.parametrize("params", [WIN5, WIN9], ids=["win5", "win9"])
def test_fast_rows_forced_guards(ctx, cells, params):
    """geps = 1e-5 and the injected index: every guarded projection is shifted
    on the device and fixed up on the host, on every side alike."""
    rng = np.random.default_rng(23)
    origin = (-6.0, -6.0)
    # 2000 beams of up to 8 m: some 4e-5 x 2000 x (search angles) guarded
    # projections per query, over ten expected
    ang, ranges = _scans(rng, 2000, rmax=8.0)
    out, _ = _three_ways(ctx, cells, origin, params, ang, ranges, _inits(rng, origin), inject=1, geps=1e-5)
    assert sum(o.guard_hits for o in out) > 0
    assert all(o.fixups > 0 for o in out if o.guard_hits > 0)
