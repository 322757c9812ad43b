"""Host restatement of what the correlative matcher's pruning bounds must
dominate, from the CPU oracle alone.

TEST INFRASTRUCTURE ONLY.  For one match (map, coarse map, scan, initial
pose, search parameters) `PruneOracle` holds

  cs[t, jx, jy], fs[t, fx, fy]   orc_rtcsm_dense_scores: every coarse / fine score
  c_B, fmax_B [t, jx, jy]        a block's coarse score, the max of its lr x lr fine scores
  cmax, fmax [t, s]              their maxima over the member blocks of superblock
                                 s = b * nsbx + a (a along x), clipped to ncx, ncy
  edge[t]                        some valid beam's coarse lattice starts left of /
                                 below the map (ix - winX < 0 or iy - winY < 0)
  U[t, s]                        the ideal bound: the sum over the valid beams, in beam
                                 order, of the max of the coarse map over the full 4 x 4
                                 lattice of a superblock's blocks, reads outside the map 0
  Ustrip[t, s]                   the same with the strip left of / below the map
                                 (x, y in [-(lr - 1), -1]) reading the map's first coarse
                                 column / row, as the superblock planes hold it (§4.1b
                                 "Low map edges"); equal to U wherever no beam's 4 x 4
                                 lattice touches the strip

and the keep rule of the pruned paths.  The sums run in beam order: fp64
addition is monotone, so U >= every member's reference-order coarse score
holds exactly, not only up to rounding.

`SCENE_BUILDERS` names the inputs the GPU invariant tests use; the CPU test checks
the restatement itself on every one of them.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import oracle_bind as ob
from lgs_amd import scene

SB = 4   # kSB: a superblock is SB x SB coarse blocks of one angle


def build_map(world, n_cells, res, patch, poses, n_beams, center=(0.0, 0.0)):
    ang = scene.beam_angles(n_beams)
    m = ob.OMap(res, patch, n_cells, n_cells, center)
    bp = ob.BuilderParams(0.01, 20.0, 0.6, 0.45)
    for p in poses:
        m.integrate(p, ob.OScan(scene.ray_cast(world, p, ang), ang), bp)
    return m.cells(), m.m.min_x, m.m.min_y


def forward_max(coarse, lr, strip):
    """G[y + lo, x + lo] = max over a', b' < 4 of V(x + lr a', y + lr b') for every
    base cell (x, y) that can see a nonzero value; V = the coarse map, 0 outside
    (strip: C(max(x, 0), max(y, 0)) for x, y >= -(lr - 1) inside the high edges)."""
    H, W = coarse.shape
    lo, hi = SB * lr, (SB - 1) * lr
    E = np.zeros((H + lo + hi, W + lo + hi))
    E[lo:lo + H, lo:lo + W] = coarse
    if strip and lr > 1:
        k = lr - 1
        E[lo - k:lo, lo:lo + W] = coarse[0:1, :]
        E[lo:lo + H, lo - k:lo] = coarse[:, 0:1]
        E[lo - k:lo, lo - k:lo] = coarse[0, 0]
    G = np.zeros((H + lo, W + lo))
    for b in range(SB):
        for a in range(SB):
            np.maximum(G, E[lr * b:lr * b + H + lo, lr * a:lr * a + W + lo], out=G)
    return G, lo


def plane_layout(W, H, lr, ncx, ncy):
    """set_plane_layout / super_bytes of k_rtcsm.hip: which superblock layout a
    search takes and the size of its superblock buffer (what the debug buffer
    "super" reports), so that a test can tell the layouts apart."""
    Wq, Hq = -(-W // lr), -(-H // lr)
    nsbx, nsby = -(-ncx // SB), -(-ncy // SB)
    M = max(SB * nsbx, SB * nsby)
    Wqp, Hqp = (Wq + 2 * M + 3) & ~3, Hq + 2 * M
    Wq4, Hq4 = (((Wqp + 3) // 4) + 7) & ~7, (Hqp + 3) // 4
    octet = nsbx <= 9 and nsby <= 9 and nsbx * nsby <= 64
    unit8 = 3 if (octet and nsby > 5) else 2
    Qo = (Hq4 + 3) // 4 + 1
    raw = 4 * unit8 * lr * lr * 16 * Qo * Wq4 if octet else 2 * lr * lr * 16 * Wq4 * Hq4
    return dict(oct=octet, unit8=unit8, nsbx=nsbx, nsby=nsby, super_bytes=(raw + 255) & ~255)


class PruneOracle:
    def __init__(self, cells, min_x, min_y, res, params, ranges, angles, init, coarse=None, rel=(0.0, 0.0, 0.0)):
        lr = int(params[0])
        cells = np.ascontiguousarray(cells, dtype=np.float64)
        self.coarse = ob.precompute(cells, lr) if coarse is None else np.ascontiguousarray(coarse, dtype=np.float64)
        g, cg = ob.OGrid(cells, min_x, min_y, res), ob.OGrid(self.coarse, min_x, min_y, res)
        sc = ob.OScan(ranges, angles, rel, 0.0, 30.0)
        prm = ob.RtcsmParams(*params)
        L = ob.lib()
        dims = (C.c_int * 7)()
        L.orc_rtcsm_dense_scores(C.byref(g.g), C.byref(cg.g), C.byref(prm), C.byref(sc.s), ob.Pose(*init), None,
                                 None, dims)
        self.win_x, self.win_y, self.win_t, self.ncx, self.ncy, nfx, nfy = list(dims)
        self.lr, self.T = lr, 2 * self.win_t + 1
        T, ncx, ncy = self.T, self.ncx, self.ncy
        cs, fs = np.zeros((T, ncx, ncy)), np.zeros((T, nfx, nfy))   # jy / fy fastest (lgs_oracle.c:521-561)
        L.orc_rtcsm_dense_scores(C.byref(g.g), C.byref(cg.g), C.byref(prm), C.byref(sc.s), ob.Pose(*init),
                                 ob.dp(cs), ob.dp(fs), dims)
        self.cs, self.fs = cs, fs
        self.c_B = cs
        self.fmax_B = fs.reshape(T, ncx, lr, ncy, lr).max(axis=(2, 4))
        self.nsbx, self.nsby = -(-ncx // SB), -(-ncy // SB)
        self.nsb2 = self.nsbx * self.nsby
        self.cmax, self.fmax = self._super_max(self.c_B), self._super_max(self.fmax_B)
        self.layout = plane_layout(cells.shape[1], cells.shape[0], lr, ncx, ncy)

        # the angles' scan indices on the coarse grid (ComputeScanIndices), as the dense scores take them
        sx, sy, st = C.c_double(), C.c_double(), C.c_double()
        L.orc_rtcsm_search_step(res, C.byref(sc.s), params[4], C.byref(sx), C.byref(sy), C.byref(st))
        sp = L.orc_compound(ob.Pose(*init), ob.Pose(*rel))
        buf = (C.c_int * (2 * len(sc.r)))()
        rows = []
        for t in range(-self.win_t, self.win_t + 1):
            n = L.orc_rtcsm_scan_indices(C.byref(cg.g), ob.Pose(sp.x, sp.y, sp.theta + st.value * t), C.byref(sc.s),
                                         params[4], buf)
            rows.append(np.array(buf[:2 * n], dtype=np.int64).reshape(n, 2))
        self.Nv = len(rows[0])
        assert all(len(r) == self.Nv for r in rows)   # a beam is valid by its range alone
        self.idx = np.stack(rows) if self.Nv else np.zeros((T, 0, 2), dtype=np.int64)
        bx, by = self.idx[:, :, 0] - self.win_x, self.idx[:, :, 1] - self.win_y   # [T, Nv] lattice starts
        self.edge = ((bx < 0) | (by < 0)).any(axis=1)
        self.U = self._ideal(bx, by, strip=False)
        self.Ustrip = self._ideal(bx, by, strip=True)

    def _super_max(self, blk):
        T = blk.shape[0]
        pad = np.full((T, SB * self.nsbx, SB * self.nsby), -np.inf)
        pad[:, :self.ncx, :self.ncy] = blk
        m = pad.reshape(T, self.nsbx, SB, self.nsby, SB).max(axis=(2, 4))   # [t, a, b]
        return np.ascontiguousarray(m.transpose(0, 2, 1)).reshape(T, self.nsb2)   # s = b * nsbx + a

    def _ideal(self, bx, by, strip):
        G, lo = forward_max(self.coarse, self.lr, strip)
        out = np.zeros((self.T, self.nsb2))
        for b in range(self.nsby):
            for a in range(self.nsbx):
                x, y = bx + SB * self.lr * a + lo, by + SB * self.lr * b + lo
                ok = (x >= 0) & (x < G.shape[1]) & (y >= 0) & (y < G.shape[0])
                v = np.where(ok, G[np.clip(y, 0, G.shape[0] - 1), np.clip(x, 0, G.shape[1] - 1)], 0.0)
                # beam order, one addition per beam (cumsum is sequential)
                out[:, b * self.nsbx + a] = np.cumsum(v, axis=1)[:, -1] if self.Nv else 0.0
        return out

    # ---- per-block views of per-superblock quantities
    def super_of_block(self):
        """s[jx, jy] of every coarse block"""
        jx, jy = np.meshgrid(np.arange(self.ncx), np.arange(self.ncy), indexing="ij")
        return (jy // SB) * self.nsbx + jx // SB

    def members(self):
        """member blocks of every superblock, clipped to ncx, ncy: [nsb2]"""
        a, b = np.arange(self.nsb2) % self.nsbx, np.arange(self.nsb2) // self.nsbx
        return np.minimum(SB, self.ncx - SB * a) * np.minimum(SB, self.ncy - SB * b)

    def unsafe_blocks(self):
        """blocks whose coarse score does not bound their fine scores: [T, ncx, ncy] bool"""
        return self.fmax_B > self.c_B

    # ---- the keep rule of every pruned path
    def kept(self, sbound, L, thr):
        """k_coarse_rows (k_rtcsm.hip, `kp = (bnd > pl.thr) && bnd >= L` in its
        selection ballot), k_keep and unsafe_angle (the same line) and k_select
        (`kp = (bnd > pl.thr) && bnd >= L` before it reads cscore): a superblock's
        blocks are scored iff its bound passes, whatever the angle's edge flag."""
        sb = np.asarray(sbound).reshape(self.T, self.nsb2)
        return (sb > thr) & (sb >= L)

    def kept_blocks(self, sbound, L, thr):
        return int((self.kept(sbound, L, thr) * self.members()[None, :]).sum())


# --------------------------------------------------------------------------
# The scenes of tests/test_gpu_prune_invariants.py.  Each is a dict:
#   cells, mx, my, res, params, ranges, angles, init  -- the match
#   low_edge -- declared: some block's fine max exceeds its coarse score
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _world():
    return scene.make_world()


@functools.lru_cache(maxsize=None)
def _room(n_cells, n_poses, n_beams):
    return build_map(_world(), n_cells, 0.05, 100, scene.arc_poses(n_poses), n_beams)


def _scan(true, n_beams, drop=0):
    ang = scene.beam_angles(n_beams)
    r = scene.ray_cast(_world(), true, ang)
    if drop:
        r[::drop] = 25.0   # >= ScanRangeMax: not a valid beam (Nv < n)
    return r, ang


def _room_scene(n, n_beams, true, dinit, params, drop=0, org=None, low_edge=False):
    """An n[1] x n[0]-cell crop (origin `org`, default: centred) of the room map."""
    cells, mx, my = _room(400, 4, 361)   # the room's 480 cells and a margin: 800 x 800
    h, w = (n, n) if isinstance(n, int) else n
    x0, y0 = org if org is not None else ((cells.shape[1] - w) // 2, (cells.shape[0] - h) // 2)
    cells, mx, my = cells[y0:y0 + h, x0:x0 + w].copy(), mx + x0 * 0.05, my + y0 * 0.05
    r, ang = _scan(true, n_beams, drop)
    init = (true[0] + dinit[0], true[1] + dinit[1], true[2] + dinit[2])
    return dict(cells=cells, mx=mx, my=my, res=0.05, params=params, ranges=r, angles=ang, init=init,
                low_edge=low_edge)


NOISE_VALUES = (1.0, 0.999, 254.5 / 255.0, 0.62, 0.3, 1.0 / 255.0, 2.0 ** -24, 2.0 ** -25, 1e-30)
NOISE_WEIGHTS = (0.35, 0.2, 0.15, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05)   # mostly near 1: window maxima stay near the sums


def _noise_scene():
    """Noise in [0, 1] holding exactly 1.0, +0, 2^-24, 2^-25 and 1e-30 -- the
    fp16 subnormal round-ups and the bytes 1 and 255 of the 8-bit units -- on
    the room's occupied cells (so that bounds differ between superblocks), a
    dense patch and a sparse background."""
    rng = np.random.default_rng(4242)
    s = _room_scene((230, 250), 203, (0.3, -0.8, 0.7), (0.1, 0.05, -0.02), (5, 1.0, 1.0, 0.15, 20.0), org=(290, 270))
    occ = s["cells"] > 0.5
    shape = occ.shape
    cells = np.where(occ | (rng.random(shape) < 0.002), rng.choice(NOISE_VALUES, size=shape, p=NOISE_WEIGHTS), 0.0)
    cells[100:106, 120:130] = rng.choice(NOISE_VALUES, size=(6, 10))
    s["cells"] = cells
    return s


def _half_plane_scene(params, value):
    """A half plane of one value: a superblock's rightmost members read it
    wherever any member does, so a full superblock's ideal bound EQUALS its best
    member's coarse score and the device's bound has no slack but its own
    round-ups and factors.  1.0: the fp16 round-up and the byte 255 are exact
    (only sb_mult separates the bound from the score); 0.62: neither is, and a
    round-up taken in the wrong direction falls below the score."""
    cells = np.zeros((240, 240))
    cells[:, 130:] = value
    rng = np.random.default_rng(7)
    ang = scene.beam_angles(181)
    return dict(cells=cells, mx=-6.0, my=-6.0, res=0.05, params=params, ranges=rng.uniform(0.5, 3.0, size=181),
                angles=ang, init=(0.1, -0.2, 3.1),   # facing left: the first and the last beam end in the plane
                low_edge=False)


SCENE_BUILDERS = {
    # 5 x 5 blocks, 2 x 2 partial superblocks, k_super_oct<5, 2>; the low walls sit 14 cells inside the map, so
    # that some angles have a beam whose lattice starts left of / below it and others none
    "room": lambda: _room_scene(400, 361, (0.4, 0.2, 0.3), (0.1, -0.05, 0.03), (5, 1.0, 1.0, 0.2, 20.0), org=(146, 146)),
    # Nv = 144 of 181 beams; 7 x 5 blocks
    "beams181": lambda: _room_scene(300, 181, (-0.3, 0.5, 2.0), (0.05, 0.1, -0.04), (5, 1.5, 1.0, 0.3, 20.0), drop=5),
    # a map 298 cells wide and 293 high (no multiple of LowRes): the plain precompute and the phase-plane copy
    "oddmap": lambda: _room_scene((293, 298), 250, (0.2, -0.4, -1.1), (-0.1, 0.05, 0.02), (5, 1.0, 1.0, 0.2, 20.0)),
    # occupied cells on x = 0 / y = 0 and a scan that leaves the map low: unsafe blocks in every angle
    "lowedge": lambda: _room_scene(320, 361, (-0.6, -0.7, 0.4), (0.1, -0.1, 0.05), (5, 1.0, 1.0, 0.2, 20.0),
                                   org=(352, 344), low_edge=True),
    # +-2.5 m: 21 x 21 blocks, 6 x 6 superblocks, k_super_oct<9, 3>
    "win6x6": lambda: _room_scene(300, 181, (0.5, 0.3, 0.9), (0.2, -0.3, 0.02), (5, 5.0, 5.0, 0.1, 20.0)),
    # 9.0 x 1.0 m: 37 x 5 blocks, 10 x 2 superblocks: the fp16 planes and k_super (the wide window reaches
    # past the map's left edge: a few unsafe blocks here too)
    "aniso": lambda: _room_scene(300, 181, (0.4, -0.1, 0.9), (0.1, -0.1, 0.03), (5, 9.0, 1.0, 0.1, 20.0),
                                 low_edge=True),
    "lr2": lambda: _room_scene(300, 181, (0.1, 0.6, -0.5), (0.05, -0.05, 0.02), (2, 1.0, 1.0, 0.1, 20.0)),
    "lr4": lambda: _room_scene(300, 181, (0.1, 0.6, -0.5), (0.1, -0.05, 0.02), (4, 1.0, 1.0, 0.1, 20.0)),
    "lr8": lambda: _room_scene(400, 181, (0.1, 0.6, -0.5), (0.1, -0.1, 0.02), (8, 1.6, 1.6, 0.1, 20.0)),
    "noise": _noise_scene,
    "ones": lambda: _half_plane_scene((5, 1.0, 1.0, 0.15, 20.0), 1.0),          # 8-bit octet units
    "ones_wide": lambda: _half_plane_scene((5, 9.0, 1.0, 0.1, 20.0), 1.0),      # fp16 planes
    "half062": lambda: _half_plane_scene((5, 1.0, 1.0, 0.15, 20.0), 0.62),
    "half062_wide": lambda: _half_plane_scene((5, 9.0, 1.0, 0.1, 20.0), 0.62),
    "half062_6x6": lambda: _half_plane_scene((5, 5.0, 5.0, 0.1, 20.0), 0.62),   # 12-row units
}


@functools.lru_cache(maxsize=None)
def scene_inputs(name):
    return SCENE_BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def scene_oracle(name):
    """The scene's PruneOracle, computed once and shared (never modified)."""
    s = scene_inputs(name)
    return PruneOracle(s["cells"], s["mx"], s["my"], s["res"], s["params"], s["ranges"], s["angles"], s["init"])
