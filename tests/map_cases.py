"""Inputs and sequences of the map builder's shape tests.

test_gpu_map_shapes.py runs every sequence here on the device next to the
oracle; test_map_cases_cpu.py runs them on the oracle alone (ctx = None) and
asserts that each input still reaches the path it was written for.  A sequence
is written once: `run_*(case, ctx, check, ...)` drives the oracle's map and,
with a context, the device's map through the same calls and hands both to
`check(gm, om, tag, full)` after every step (gm is None without a context).
`full` says whether the step is one at which the whole map is compared: every
step of a small map, three steps of a map of millions of cells.

The constants restate csrc/k_raycast.hip (kShortRun, kMaxTblCells,
kApplyMapsLds) and csrc/glibc_math.hpp (the sincos domain)."""
from __future__ import annotations

import numpy as np

import oracle_bind as ob
from lgs_amd import scene

K_SHORT_RUN = 26                 # runs stored inline in the latest map's index
K_MAX_TBL_CELLS = 4 << 20        # largest latest map with an index table
K_APPLY_MAPS_LDS = 64            # maps of a pass that k_apply stages in LDS
SINCOS_DOMAIN = 105414350.0      # gl_sincos restates glibc below this |x|
BP = (0.01, 20.0, 0.6, 0.45)
BIG_CELLS = 2_000_000            # maps above this are compared in full at three steps only


class Case:
    """The scans of one sequence: poses, ranges per pose, the beam angles and
    everything a scan and the builder take besides."""

    def __init__(self, res, ps, poses, ranges, angles, bp=BP, rel=(0.0, 0.0, 0.0), min_range=0.0,
                 max_range=30.0):
        self.res, self.ps = float(res), int(ps)
        self.poses = [tuple(float(v) for v in p) for p in poses]
        self.ranges = [np.ascontiguousarray(r, dtype=np.float64) for r in ranges]
        self.angles = np.ascontiguousarray(angles, dtype=np.float64)
        self.bp, self.rel, self.min_range, self.max_range = tuple(bp), tuple(rel), min_range, max_range
        self.center = None            # of new local maps; None: the first pose of the map
        self._oscans = None
        self._dscans = None

    def origin(self, k):
        return self.poses[k][:2] if self.center is None else self.center

    def oscans(self):
        if self._oscans is None:
            self._oscans = [ob.OScan(r, self.angles, rel=self.rel, min_range=self.min_range,
                                     max_range=self.max_range) for r in self.ranges]
        return self._oscans

    def dscans(self, ctx):
        if self._dscans is None or self._dscans[0] is not ctx:
            self._dscans = (ctx, [ctx.scan(r, self.angles, self.rel, self.min_range, self.max_range)
                                  for r in self.ranges])
        return self._dscans[1]

    def obp(self):
        return ob.BuilderParams(*self.bp)

    def dbp(self):
        from lgs_amd import abi
        return abi.BuilderParams(*self.bp)

    def limits(self):
        """The open range interval a beam must lie in (std::max / std::min of both limits)."""
        return max(self.bp[0], self.min_range), min(self.bp[1], self.max_range)

    def usable(self, k):
        lo, hi = self.limits()
        return ~((self.ranges[k] >= hi) | (self.ranges[k] <= lo))

    def sensor(self, k):
        x, y, t = self.poses[k]
        rx, ry, rt = self.rel
        return x + np.cos(t) * rx - np.sin(t) * ry, y + np.sin(t) * rx + np.cos(t) * ry, t + rt

    def ray_cells(self, k, geom):
        """Sensor cell and hit cells of scan k in a map geometry, restated with
        numpy (for conditions such as the ray length, not for parity)."""
        sx, sy, st = self.sensor(k)
        u = self.usable(k)
        hx = sx + self.ranges[k][u] * np.cos(st + self.angles[u])
        hy = sy + self.ranges[k][u] * np.sin(st + self.angles[u])
        cell = lambda v, m: np.floor((v - m) / self.res).astype(np.int64)
        return (int(cell(sx, geom["min_x"])), int(cell(sy, geom["min_y"])),
                cell(hx, geom["min_x"]), cell(hy, geom["min_y"]))


def cell_bits(om):
    """The cell-bit count raycast hands to the key sort for this map alone."""
    g = om.geometry()
    bits = 1
    while bits < 32 and (1 << bits) < g["w"] * g["h"]:
        bits += 1
    return bits


def _full_steps(n):
    return {0, n // 2, n - 1}


def _is_full(om, k, n):
    g = om.geometry()
    return g["w"] * g["h"] <= BIG_CELLS or k in _full_steps(n)


def _map_pair(ctx, res, ps, ncx, ncy, center):
    om = ob.OMap(res, ps, ncx, ncy, center=center)
    gm = ctx.map(res, ps, ncx, ncy, center=center) if ctx is not None else None
    return gm, om


class _Options:
    """LGS_OPT_DEVICE_HITS / LGS_OPT_RAY_CHUNK_KEYS for one call, then the defaults again."""

    def __init__(self, ctx, dev=1, chunk=0):
        self.ctx, self.dev, self.chunk = ctx, dev, chunk

    def __enter__(self):
        if self.ctx is not None:
            from lgs_amd import abi
            self.ctx.set_option(abi.LGS_OPT_DEVICE_HITS, self.dev)
            if self.chunk:
                self.ctx.set_option(abi.LGS_OPT_RAY_CHUNK_KEYS, self.chunk)

    def __exit__(self, *exc):
        if self.ctx is not None:
            from lgs_amd import abi
            self.ctx.set_option(abi.LGS_OPT_RAY_CHUNK_KEYS, 1 << 28)
            self.ctx.set_option(abi.LGS_OPT_DEVICE_HITS, 1)
        return False


# ---------------------------------------------------------------------------
# the five builder entry points (and a fixed-size map), each against the oracle
# ---------------------------------------------------------------------------
def run_growth(case, ctx, check, chunk=0):
    """UpdateGridMap scan by scan into a 0x0 map centred on the first pose."""
    gm, om = _map_pair(ctx, case.res, case.ps, 0, 0, case.origin(0))
    n = len(case.poses)
    with _Options(ctx, 1, chunk):
        for k in range(n):
            om.integrate(case.poses[k], case.oscans()[k], case.obp())
            if gm is not None:
                gm.update_scan(case.dscans(ctx)[k], case.poses[k], case.dbp())
            check(gm, om, f"growth{k}", _is_full(om, k, n))
    return om


def run_fixed(case, ctx, check, ncx, ncy, center=(0.0, 0.0)):
    """UpdateGridMap into a map constructed with a size (odd w: the + 0.5 centre offset)."""
    gm, om = _map_pair(ctx, case.res, case.ps, ncx, ncy, center)
    check(gm, om, "fixed new", False)
    n = len(case.poses)
    for k in range(n):
        om.integrate(case.poses[k], case.oscans()[k], case.obp())
        if gm is not None:
            gm.update_scan(case.dscans(ctx)[k], case.poses[k], case.dbp())
        check(gm, om, f"fixed{k}", k == n - 1)
    return om


def run_window(case, ctx, check, win=4, center=(0.0, 0.0)):
    """ConstructMapFromScans over a sliding window on one map object."""
    gm, om = _map_pair(ctx, case.res, case.ps, 0, 0, center)
    n = len(case.poses)
    for k in range(n):
        lo = max(0, k - win + 1)
        om.construct(case.poses[lo:k + 1], case.oscans()[lo:k + 1], case.obp())
        if gm is not None:
            gm.construct(case.dscans(ctx)[lo:k + 1], case.poses[lo:k + 1], case.dbp())
        check(gm, om, f"window{k}", _is_full(om, k, n))
    return om


def run_append(case, ctx, check, win=4):
    """AppendScan: the newest scan into the local map, the latest map rebuilt
    from the window.  check sees the latest map at every step (tag "latest<k>")
    and the local map at the full steps (tag "local<k>")."""
    c = case.poses[0][:2]
    local, olocal = _map_pair(ctx, case.res, case.ps, 0, 0, c)
    latest, olatest = _map_pair(ctx, case.res, case.ps, 0, 0, c)
    n = len(case.poses)
    for k in range(n):
        lo = max(0, k - win + 1)
        olocal.integrate(case.poses[k], case.oscans()[k], case.obp())
        olatest.construct(case.poses[lo:k + 1], case.oscans()[lo:k + 1], case.obp())
        if ctx is not None:
            local.append_scan(latest, case.dscans(ctx)[lo:k + 1], case.poses[lo:k + 1], case.dbp())
        check(latest, olatest, f"latest{k}", _is_full(olatest, k, n))
        full = _is_full(olocal, k, n)
        check(local, olocal, f"local{k}", full)
    return olocal, olatest


def perturb(poses, seed=1):
    rng = np.random.default_rng(seed)
    return [(x + rng.uniform(-0.04, 0.04), y + rng.uniform(-0.04, 0.04), t + rng.uniform(-0.02, 0.02))
            for x, y, t in poses]


def run_maps(case, ctx, check, ranges, dev=1, chunk=0, grown=True, new_poses=None):
    """AfterLoopClosure's fused rebuild of one local map per node range.  With
    `grown` the maps are first grown scan by scan at the case's poses and
    rebuilt at `new_poses` (default: the poses perturbed), so that Resize is
    anchored to a previous geometry; without, they are new 0x0 maps."""
    new = case.poses if not grown else (perturb(case.poses) if new_poses is None else new_poses)
    gms, oms = [], []
    for lo, hi in ranges:
        gm, om = _map_pair(ctx, case.res, case.ps, 0, 0, case.origin(lo))
        if grown:
            for k in range(lo, hi + 1):
                om.integrate(case.poses[k], case.oscans()[k], case.obp())
                if gm is not None:
                    gm.update_scan(case.dscans(ctx)[k], case.poses[k], case.dbp())
        gms.append(gm)
        oms.append(om)
    if ctx is not None:
        with _Options(ctx, dev, chunk):
            ctx.construct_maps(gms, ranges, case.dscans(ctx), new, case.dbp())
    for i, ((lo, hi), gm, om) in enumerate(zip(ranges, gms, oms)):
        om.construct(new[lo:hi + 1], case.oscans()[lo:hi + 1], case.obp())
        check(gm, om, f"map{i}", True)
    return oms


def run_global(case, ctx, check, dev=1, chunk=0):
    """ConstructGlobalMap: a new 0x0 map at (0, 0), every node."""
    om = ob.OMap(case.res, case.ps, 0, 0)
    om.construct(case.poses, case.oscans(), case.obp())
    gm = None
    if ctx is not None:
        with _Options(ctx, dev, chunk):
            gm = ctx.construct_global_map(case.res, case.ps, case.dscans(ctx), case.poses, case.dbp())
    check(gm, om, "global", True)
    return om


# ---------------------------------------------------------------------------
# 1. directed rays
# ---------------------------------------------------------------------------
DIRECTED_MAJOR = (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 255, 256, 257, 640, 1000)
DIRECTED_CONFIGS = ((0.05, 64, (0.0, 0.0)), (0.01, 7, (0.0, 0.0)), (0.013, 100, (812.4, -377.7)),
                    (0.25, 3, (-5000.0, 5000.0)))
DIRECTED_CHUNK = 50000          # keys per pass: the scan's ~2.4e5 keys split into several passes


def directed_deltas():
    """Cell deltas (dx, dy): major length M, minor length in {0, 1, 2, M/3, M/2,
    M - 2, M - 1, M}, every sign pair, either axis the major one."""
    out, seen = [], set()
    for M in DIRECTED_MAJOR:
        for m in sorted({0, 1, 2, M // 3, M // 2, M - 2, M - 1, M}):
            if not 0 <= m <= M:
                continue
            for sa in (1, -1):
                for sb in (1, -1):
                    for d in ((sa * M, sb * m), (sa * m, sb * M)):
                        if d not in seen:
                            seen.add(d)
                            out.append(d)
    return out


def directed_case(res, ps, centre):
    """One scan from the centre of the cell whose corner is `centre` (the
    corner of a 0x0 map centred there); beam i ends at the centre of the cell
    (dx_i, dy_i) away.  The zero delta's beam has length 0.3 res (a beam of
    length 0 is not usable), so it ends inside the sensor's cell."""
    d = np.array(directed_deltas(), dtype=np.float64)
    r = res * np.hypot(d[:, 0], d[:, 1])
    a = np.arctan2(d[:, 1], d[:, 0])
    zero = (d[:, 0] == 0) & (d[:, 1] == 0)
    r[zero] = 0.3 * res
    a[zero] = np.pi / 4
    pose = (centre[0] + 0.5 * res, centre[1] + 0.5 * res, 0.0)
    case = Case(res, ps, [pose], [r], a, bp=(res / 4, 400.0, 0.6, 0.45), max_range=500.0)
    case.center = tuple(centre)
    return case


# ---------------------------------------------------------------------------
# 2. resolution x patch size
# ---------------------------------------------------------------------------
MATRIX_RES = (0.01, 0.013, 0.03125, 0.1, 0.5, 2.5)
MATRIX_PS = (1, 7, 64, 300)
MATRIX = [(res, ps) for res in MATRIX_RES for ps in MATRIX_PS if not (ps == 1 and res < 0.02)]
MATRIX_RANGES = [(0, 3), (2, 5), (5, 5), (4, 7)]


def trajectory(n, seed=0, offset=(0.0, 0.0)):
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 2.0 * np.pi, n, endpoint=False)
    return [(offset[0] + 1.2 * np.cos(a) + rng.uniform(-0.05, 0.05),
             offset[1] + 0.9 * np.sin(a) + rng.uniform(-0.05, 0.05),
             a + np.pi / 2 + rng.uniform(-0.05, 0.05)) for a in t]


def shifted(world, offset):
    return world + np.array([offset[0], offset[1], offset[0], offset[1]])


def room_case(world, res, ps, n=8, beams=91, seed=0, offset=(0.0, 0.0), **kw):
    """n poses on a loop in the room's clear centre (moved by `offset`, the room with it)."""
    poses = trajectory(n, seed, offset)
    ang = scene.beam_angles(beams)
    w = shifted(world, offset)
    return Case(res, ps, poses, [scene.ray_cast(w, p, ang) for p in poses], ang, **kw)


def matrix_case(world, res, ps):
    """91 beams and 8 poses below 0.5 m; 181 beams and 12 poses from 0.5 m on,
    where a cell collects enough hits of one pass for runs past kShortRun."""
    coarse = res >= 0.5
    seed = int(round(res * 1e5)) % 1000 + ps
    return room_case(world, res, ps, n=12 if coarse else 8, beams=181 if coarse else 91, seed=seed)


def matrix_ranges(case):
    n = len(case.poses)
    return MATRIX_RANGES if n == 8 else [(0, 4), (3, 7), (8, 8), (6, n - 1)]


def odd_cells(res, ps):
    """An odd number of patches of an odd size covering 26 m: an odd cell count."""
    assert ps % 2 == 1
    np_ = int(np.ceil(26.0 / res / ps))
    np_ += 1 - np_ % 2
    return np_ * ps


# ---------------------------------------------------------------------------
# 3. the latest map either side of kMaxTblCells (res 0.01)
# ---------------------------------------------------------------------------
LATEST_WIN = 4
LATEST_FULL_STEPS = range(6, 10)     # scans with their full range; the others stop at 4 m
LATEST_STEPS = 19


def latest_case(world):
    """A sensor that all but stands still (1 mm a step, so the window's box
    keeps its patches): scans 0-5 and 10-18 have every range beyond 4 m set
    to 25 m (>= the usable maximum: skipped), scans 6-9 are whole.  A window
    of 4 holds a whole scan at steps 6-12."""
    ang = scene.beam_angles(181)
    poses = [(0.1 + 0.001 * k, -0.2 + 0.0005 * k, 0.3 + 0.001 * k) for k in range(LATEST_STEPS)]
    rs = []
    for k, p in enumerate(poses):
        r = scene.ray_cast(world, p, ang)
        if k not in LATEST_FULL_STEPS:
            r = np.where(r > 4.0, 25.0, r)
        rs.append(r)
    return Case(0.01, 64, poses, rs, ang)


def latest_above(k):
    """Steps at which the window holds a full-range scan."""
    return any(j in LATEST_FULL_STEPS for j in range(max(0, k - LATEST_WIN + 1), k + 1))


# ---------------------------------------------------------------------------
# 4. far from the origin, far from square
# ---------------------------------------------------------------------------
FAR_OFFSETS = ((1000.3, -777.7), (-4096.0, 4096.0), (1.0e5, -1.0e5), (1.0e6 + 0.3, 1.0e6))
FAR_CONFIGS = ((0.05, 64), (0.013, 7))
# All-negative coordinates: ConstructMapFromScans' box starts its top right at
# DBL_MIN, so the map reaches from the scans to x = y = 0.  1.5 km out along
# x and just past the room's half width along y the oracle's map has 1.9e7
# cells at 5 cm; 2 km gives 2.3e7 (a diagonal offset would be capped near 200 m).
NEGATIVE_OFFSET = (-1500.3, -14.7)
MAX_CELLS = 20_000_000


def far_cases():
    """(res, ps, offset, entry).  Growth runs at every offset.
    ConstructMapFromScans starts its box's top right at DBL_MIN, so with a
    negative coordinate its map reaches to 0 on that axis: at (1000.3, -777.7)
    / 1.3 cm, (-4096, 4096) and (1e5, -1e5) the oracle's map would have 1e8 to
    1e10 cells, which nothing here can allocate.  The window and the fused
    rebuild run at the offsets whose map stays under 2e7 cells, and at the
    mirror image of the others in the positive quadrant."""
    out = []
    for res, ps in FAR_CONFIGS:
        for off in FAR_OFFSETS:
            out.append((res, ps, off, "growth"))
            cells = 1.0
            for v in off:           # the room is 24 m wide; patches round up
                cells *= ((abs(v) + 14.0) if v < 0 else 28.0) / res
            use = off if cells < MAX_CELLS else (abs(off[0]), abs(off[1]))
            for entry in ("window", "maps-dev", "maps-host"):
                out.append((res, ps, use, entry))
    return out


def corridor_world(along_y=False):
    """A 60 m x 2 m corridor with three pillars on its walls, along x or along y."""
    segs = [(-30.0, -1.0, 30.0, -1.0), (30.0, -1.0, 30.0, 1.0), (30.0, 1.0, -30.0, 1.0), (-30.0, 1.0, -30.0, -1.0)]
    for x0, y0 in ((-17.0, -1.0), (3.5, 0.6), (21.0, -1.0)):
        x1, y1 = x0 + 0.8, y0 + 0.4
        segs += [(x0, y0, x1, y0), (x1, y0, x1, y1), (x1, y1, x0, y1), (x0, y1, x0, y0)]
    s = np.array(segs, dtype=np.float64)
    return s[:, [1, 0, 3, 2]] if along_y else s


def corridor_case(along_y=False, res=0.05, ps=64):
    """Driven end to end, 29 poses 2 m apart, 181 beams; beams along the axis
    beyond the usable 20 m are skipped."""
    w = corridor_world(along_y)
    ang = scene.beam_angles(181)
    xs = np.linspace(-28.0, 28.0, 29)
    poses = [((0.1 * np.sin(x), x, np.pi / 2 + 0.02 * np.cos(x)) if along_y else
              (x, 0.1 * np.sin(x), 0.02 * np.cos(x))) for x in xs]
    return Case(res, ps, poses, [scene.ray_cast(w, p, ang) for p in poses], ang)


def gray(cells):
    """MapSaver::DrawMap's gray levels, rows flipped (as test_render_gray_matches_drawmap)."""
    want = np.where((cells <= 0.0) | (cells > 1.0), 192, ((1.0 - cells) * 255.0).astype(np.uint8)).astype(np.uint8)
    return want[::-1]


# ---------------------------------------------------------------------------
# 5. sensor offset, the scan's own range limits binding
# ---------------------------------------------------------------------------
REL = (0.2, -0.1, 0.5)
SCAN_MIN, SCAN_MAX = 1.5, 8.0


def limits_case(world, res=0.05, ps=32):
    """The scan's limits (1.5 m, 8 m) lie inside the builder's (0.01 m, 20 m).
    Beams are placed exactly at each of the four limits, and between the
    builder's and the scan's on either side (usable for the builder alone)."""
    case = room_case(world, res, ps, n=8, beams=181, seed=11, rel=REL, min_range=SCAN_MIN, max_range=SCAN_MAX)
    for k, r in enumerate(case.ranges):
        r[(3 + k) % 7::7] = SCAN_MAX
        r[(5 + k) % 11::11] = SCAN_MIN
        r[(1 + k) % 13::13] = 0.7            # between the two minima
        r[(2 + k) % 17::17] = BP[0]
        r[(4 + k) % 19::19] = BP[1]
    return case


# ---------------------------------------------------------------------------
# 6. more maps in a pass than k_apply's LDS table holds
# ---------------------------------------------------------------------------
MANY_MAPS = 70


def many_maps_case(world):
    """70 maps at res 0.1 / patch size 16: map i covers one node (i odd) or two
    nodes (i even); 31-61 beams would need scans of several lengths, so the
    scans have 61 beams and every other one keeps its first 31 usable."""
    n_nodes = sum(2 if i % 2 == 0 else 1 for i in range(MANY_MAPS))
    case = room_case(world, 0.1, 16, n=n_nodes, beams=61, seed=21)
    for k in range(1, n_nodes, 2):
        case.ranges[k][31:] = 25.0
    ranges, lo = [], 0
    for i in range(MANY_MAPS):
        c = 2 if i % 2 == 0 else 1
        ranges.append((lo, lo + c - 1))
        lo += c
    return case, ranges


# ---------------------------------------------------------------------------
# 7. headings outside the device sincos domain
# ---------------------------------------------------------------------------
HEADINGS_IN = (1.0e3, -1.0e3)
HEADING_OUT = 1.06e8


def heading_case(world, heading, res=0.05, ps=64, mixed=False):
    """8 poses whose headings are `heading` plus the loop's (ray-cast at that
    heading, so the scans see the room as ever); `mixed` keeps the heading of
    all but poses 2 and 5."""
    base = trajectory(8, seed=31)
    poses = [(x, y, t + (heading if (not mixed or k in (2, 5)) else 0.0)) for k, (x, y, t) in enumerate(base)]
    ang = scene.beam_angles(121)
    return Case(res, ps, poses, [scene.ray_cast(world, p, ang) for p in poses], ang)


# ---------------------------------------------------------------------------
# a hand-over from the device hit points must leave Resize to the host path
# ---------------------------------------------------------------------------
def handover_case(usable):
    """Two scans from the centre of cell (-16, -32) of a 0x0 map at the origin
    (5 cm, patches of 16): the box starts on a cell whose index is a negative
    multiple of the patch size, where Resize adds the patch before it and a
    second Resize to the same box would drop it again.  Without `usable`
    every range is beyond the usable maximum (a pass without rays), with it
    eight 0.6 m beams look into the first quadrant (a pass over a chunk
    budget of a few keys)."""
    res, ps = 0.05, 16
    ang = np.linspace(0.1, 1.4, 8)
    r = np.full(8, 0.6 if usable else 25.0)
    poses = [(-16 * res + 0.5 * res, -32 * res + 0.5 * res, 0.0)] * 2
    case = Case(res, ps, poses, [r, r.copy()], ang)
    case.center = (0.0, 0.0)
    return case
