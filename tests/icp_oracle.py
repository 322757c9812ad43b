"""Test-side restatement of the point-to-line ICP matcher (DESIGN.md 4.5b,
csrc/k_icp.hip), operation for operation: IEEE fp64 through numpy's
element-wise ufuncs (one rounding per operation, nothing fused), glibc's
sincos() for every sin/cos pair (what GCC makes of ScanData::HitPoint and what
glm::gl_sincos restates on the device; separate sin()/cos() calls differ from
it in about one input in a thousand, so they are not used), the oracle
library's orc_solve3_colpiv_qr for the solve and its pose algebra, and the
summation tree of the kernel reproduced addition for addition.  A second,
order-free evaluation of the same eleven sums uses math.fsum.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import ctypes as C
import ctypes.util
import math
from collections import namedtuple

import numpy as np

import oracle_bind as ob

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sincos.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
_libm.sincos.restype = None

Params = namedtuple("Params", "num_iterations_max convergence_threshold usable_range_min usable_range_max "
                              "translation_regularizer rotation_regularizer max_correspondence_dist "
                              "max_segment_length")
ScanIn = namedtuple("ScanIn", "ranges angles rel min_range max_range", defaults=((0.0, 0.0, 0.0), 0.0, 30.0))

THREADS, WAVES, SUMS = 1024, 16, 11
DBL_MAX = 1.7976931348623157e308


def sincos(x: float):
    s, c = C.c_double(), C.c_double()
    _libm.sincos(float(x), C.byref(s), C.byref(c))
    return s.value, c.value


def sincos_array(x: np.ndarray):
    s, c = np.empty(len(x)), np.empty(len(x))
    for i, v in enumerate(x):
        s[i], c[i] = sincos(v)
    return s, c


def compound(p, rel):
    r = ob.lib().orc_compound(ob.Pose(*p), ob.Pose(*rel))
    return (r.x, r.y, r.theta)


def move_backward(p, rel):
    r = ob.lib().orc_move_backward(ob.Pose(*p), ob.Pose(*rel))
    return (r.x, r.y, r.theta)


def usable_range(prm: Params, scan: ScanIn):
    return max(prm.usable_range_min, scan.min_range), min(prm.usable_range_max, scan.max_range)


def usable_mask(ranges, lo, hi):
    """the linear solver's comparisons: !(r >= hi || r <= lo)"""
    r = np.asarray(ranges, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return ~((r >= hi) | (r <= lo))


def hit_points(ranges, angles, pose):
    """ScanData::HitPoint per beam; also r cos, r sin"""
    s, c = sincos_array(np.float64(pose[2]) + np.asarray(angles, dtype=np.float64))
    r = np.asarray(ranges, dtype=np.float64)
    rc, rs = r * c, r * s
    return np.float64(pose[0]) + rc, np.float64(pose[1]) + rs, rc, rs


Table = namedtuple("Table", "idx qx qy nx ny")


def ref_table(prm: Params, ref: ScanIn, ref_sensor_pose) -> Table:
    """the usable reference beams in index order: point and unit normal (NaN: no line)"""
    lo, hi = usable_range(prm, ref)
    us = usable_mask(ref.ranges, lo, hi)
    with np.errstate(all="ignore"):
        hx, hy, _, _ = hit_points(ref.ranges, ref.angles, ref_sensor_pose)
    S2 = np.float64(prm.max_segment_length) * np.float64(prm.max_segment_length)
    n = len(us)
    idx, qx, qy, nx, ny = [], [], [], [], []
    with np.errstate(all="ignore"):
        for j in range(n):
            if not us[j]:
                continue
            best = None
            for k in (j - 1, j + 1):
                if k < 0 or k >= n or not us[k]:
                    continue
                ux, uy = hx[k] - hx[j], hy[k] - hy[j]
                l2 = ux * ux + uy * uy
                if l2 > 0.0 and l2 <= S2 and (best is None or l2 < best[2]):
                    best = (ux, uy, l2)
            idx.append(j)
            qx.append(hx[j])
            qy.append(hy[j])
            if best is None:
                nx.append(np.nan)
                ny.append(np.nan)
            else:
                l = np.sqrt(best[2])
                nx.append((-best[1]) / l)
                ny.append(best[0] / l)
    f = lambda a: np.array(a, dtype=np.float64)
    return Table(np.array(idx, dtype=np.int64), f(qx), f(qy), f(nx), f(ny))


Beams = namedtuple("Beams", "state e terms contrib")


def pass_beams(prm: Params, table: Table, scan: ScanIn, pose) -> Beams:
    """One pass, per beam: state (-2 unusable, -1 rejected, else the table entry),
    e, the eleven terms and which of them the beam contributes."""
    lo, hi = usable_range(prm, scan)
    us = usable_mask(scan.ranges, lo, hi)
    n = len(us)
    D2 = np.float64(prm.max_correspondence_dist) * np.float64(prm.max_correspondence_dist)
    with np.errstate(all="ignore"):
        hx, hy, rc, rs = hit_points(scan.ranges, scan.angles, pose)
        state = np.full(n, -2, dtype=np.int64)
        e = np.zeros(n)
        terms = np.zeros((SUMS, n))
        contrib = np.zeros((SUMS, n), dtype=bool)
        m = len(table.idx)
        for i0 in range(0, n, 256):
            sl = slice(i0, min(n, i0 + 256))
            k = sl.stop - sl.start
            if m:
                dx = hx[sl, None] - table.qx[None, :]
                dy = hy[sl, None] - table.qy[None, :]
                d2 = dx * dx + dy * dy
                d2 = np.where(d2 < np.inf, d2, np.inf)     # NaN and +inf never win a strict minimum from +inf
                jb = np.argmin(d2, axis=1)                 # the first minimum
                best = d2[np.arange(k), jb]
                has = best < np.inf
            else:
                jb = np.zeros(k, dtype=np.int64)
                best = np.full(k, np.inf)
                has = np.zeros(k, dtype=bool)
            for a in range(k):
                i = i0 + a
                if not us[i]:
                    continue
                j = int(jb[a])
                if not (has[a] and best[a] <= D2 and not np.isnan(table.nx[j])):
                    state[i] = -1
                    terms[0, i] = D2
                    contrib[0, i] = True
                    continue
                nx, ny = table.nx[j], table.ny[j]
                ddx, ddy = hx[i] - table.qx[j], hy[i] - table.qy[j]
                ee = nx * ddx + ny * ddy
                g = (nx, ny, nx * (-rs[i]) + ny * rc[i])
                state[i] = j
                e[i] = ee
                me = -ee
                terms[:, i] = (ee * ee, ee * ee, g[0] * g[0], g[0] * g[1], g[0] * g[2], g[1] * g[1], g[1] * g[2],
                               g[2] * g[2], me * g[0], me * g[1], me * g[2])
                contrib[:, i] = True
    return Beams(state, e, terms, contrib)


def tree_sum(term: np.ndarray, contrib: np.ndarray) -> float:
    """The kernel's tree: thread t of 1024 adds its beams t, t + 1024, ... in
    ascending order from +0.0 (beams that contribute nothing are skipped), six
    xor-butterfly steps per wave (masks 32 .. 1, v = v + partner), the sixteen
    wave sums added in wave order starting from wave 0."""
    n = len(term)
    acc = np.zeros(THREADS)
    with np.errstate(all="ignore"):
        for r0 in range(0, n, THREADS):
            k = min(THREADS, n - r0)
            t = np.zeros(THREADS)
            c = np.zeros(THREADS, dtype=bool)
            t[:k] = term[r0:r0 + k]
            c[:k] = contrib[r0:r0 + k]
            acc = np.where(c, acc + t, acc)
        v = acc.reshape(WAVES, 64)
        lanes = np.arange(64)
        for mask in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lanes ^ mask]
        s = v[0, 0]
        for w in range(1, WAVES):
            s = s + v[w, 0]
    return float(s)


def tree_depth(n: int) -> int:
    """additions on the longest path of the tree: rounds - 1 + 6 + 15"""
    rounds = max(1, (n + THREADS - 1) // THREADS)
    return rounds - 1 + 6 + 15


def pass_sums(b: Beams):
    """(the eleven tree sums, pairs)"""
    return [tree_sum(b.terms[k], b.contrib[k]) for k in range(SUMS)], int(np.count_nonzero(b.state >= 0))


def pass_fsums(b: Beams):
    """order-free: (the eleven exact sums rounded once, the eleven sums of |term|)"""
    ex = [math.fsum(b.terms[k][b.contrib[k]]) for k in range(SUMS)]
    ab = [math.fsum(np.abs(b.terms[k][b.contrib[k]])) for k in range(SUMS)]
    return ex, ab


def hessian(s):
    return [s[2], s[3], s[4], s[3], s[5], s[6], s[4], s[6], s[7]]


def solve_step(prm: Params, s, pose):
    """regularizers on H's diagonal, delta = solve3_colpiv_qr(H, b), pose + delta"""
    H = hessian(s)
    H[0] = H[0] + prm.translation_regularizer
    H[4] = H[4] + prm.translation_regularizer
    H[8] = H[8] + prm.rotation_regularizer
    Ha = (C.c_double * 9)(*H)
    ba = (C.c_double * 3)(s[8], s[9], s[10])
    x = (C.c_double * 3)()
    ob.lib().orc_solve3_colpiv_qr(Ha, ba, x)
    with np.errstate(all="ignore"):
        return tuple(float(np.float64(pose[k]) + np.float64(x[k])) for k in range(3))


def covariance(prm: Params, H, pair_cost, pairs, found):
    """lgs_icp_summary::covariance: the header comment, product by product"""
    if not found:
        return [0.0] * 9
    f = np.float64
    with np.errstate(all="ignore"):
        a0, a1, a2 = f(H[0]) + f(prm.translation_regularizer), f(H[1]), f(H[2])
        a3, a4, a5 = f(H[3]), f(H[4]) + f(prm.translation_regularizer), f(H[5])
        a6, a7, a8 = f(H[6]), f(H[7]), f(H[8]) + f(prm.rotation_regularizer)
        c = [a4 * a8 - a5 * a7, a2 * a7 - a1 * a8, a1 * a5 - a2 * a4,
             a5 * a6 - a3 * a8, a0 * a8 - a2 * a6, a2 * a3 - a0 * a5,
             a3 * a7 - a4 * a6, a1 * a6 - a0 * a7, a0 * a4 - a1 * a3]
        det = (a0 * c[0] + a1 * c[3]) + a2 * c[6]
        if det == 0.0 or not np.isfinite(det):
            return [0.0] * 9
        scale = f(pair_cost) / f(max(1, pairs - 3))
        return [float((ck / det) * scale) for ck in c]


Result = namedtuple("Result", "pose_found iterations num_pairs initial_pairs normalized_cost estimated_pose covariance "
                              "sensor_pose best_sensor_pose cost pair_cost initial_cost hessian trajectory")


def refine(prm: Params, ref: ScanIn, ref_pose, scan: ScanIn, initial_pose, table: Table = None) -> Result:
    """the whole loop (OptimizePose's shape) and the summary"""
    if table is None:
        table = ref_table(prm, ref, compound(ref_pose, ref.rel))
    sensor = compound(initial_pose, scan.rel)
    pose = sensor
    s, pairs = pass_sums(pass_beams(prm, table, scan, pose))
    initial_cost, initial_pairs = s[0], pairs
    prev, iterations, found, traj = DBL_MAX, 0, 1, []
    if pairs < 3:
        found = 0
    else:
        while True:
            pose = solve_step(prm, s, pose)
            s, pairs = pass_sums(pass_beams(prm, table, scan, pose))
            iterations += 1
            traj.append((pose[0], pose[1], pose[2], s[0], float(pairs)))
            if pairs < 3:
                found = 0
                break
            if iterations >= prm.num_iterations_max or abs(prev - s[0]) < prm.convergence_threshold:
                break
            prev = s[0]
    H = hessian(s)
    return Result(found, iterations, pairs, initial_pairs, s[0] / len(scan.ranges), move_backward(pose, scan.rel),
                  covariance(prm, H, s[1], pairs, found), sensor, pose, s[0], s[1], initial_cost, H, traj)
