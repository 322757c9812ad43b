"""Test-side restatement of the ICP loop detector's window search (DESIGN.md
4.5e, csrc/k_icp_window.hip, csrc/icp_window_host.hpp): the lattice pose, the
scores composed from icp_oracle.pass_beams and its summation tree, the
selection, the gate of lgs_loop_refine_icp and the 176-byte record.  Pinned by
tests/golden/icp_window_kat.json (tests/golden/make_icp_window_kat.py).

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple

import numpy as np

import icp_oracle as orc
import oracle_bind as ob
from lgs_amd import abi

Window = namedtuple("Window", "half_x half_y half_theta step_xy step_theta")
Gate = namedtuple("Gate", "min_pairs max_normalized_cost max_translation max_rotation")


def dims(w: Window):
    """(nx, ny, nt)"""
    return 2 * w.half_x + 1, 2 * w.half_y + 1, 2 * w.half_theta + 1


def num_poses(w: Window) -> int:
    nx, ny, nt = dims(w)
    return nx * ny * nt


def index(w: Window, ix: int, iy: int, it: int) -> int:
    nx, ny, _ = dims(w)
    return (it * ny + iy) * nx + ix


def decode(w: Window, p: int):
    """(ix, iy, it): theta outermost, x innermost"""
    nx, ny, _ = dims(w)
    return p % nx, (p // nx) % ny, p // (nx * ny)


def coord(c: float, i: int, half: int, step: float) -> float:
    """the product and the sum rounded once each; the centre index gives c itself"""
    if i == half:
        return float(c)
    with np.errstate(all="ignore"):
        return float(np.float64(c) + np.float64(i - half) * np.float64(step))


def lattice_pose(w: Window, centre, p: int):
    ix, iy, it = decode(w, p)
    return (coord(centre[0], ix, w.half_x, w.step_xy), coord(centre[1], iy, w.half_y, w.step_xy),
            coord(centre[2], it, w.half_theta, w.step_theta))


def score(prm: orc.Params, table: orc.Table, scan: orc.ScanIn, robot_pose):
    """(cost, pairs) of the first pass at Compound(robot_pose, relPose): initial_cost and initial_pairs"""
    b = orc.pass_beams(prm, table, scan, orc.compound(robot_pose, scan.rel))
    return orc.tree_sum(b.terms[0], b.contrib[0]), int(np.count_nonzero(b.state >= 0))


def scores(prm: orc.Params, table: orc.Table, scan: orc.ScanIn, centre, w: Window):
    """(cost float64 [P], pairs int32 [P]) in lattice order"""
    P = num_poses(w)
    cost, pairs = np.zeros(P), np.zeros(P, dtype=np.int32)
    for p in range(P):
        cost[p], pairs[p] = score(prm, table, scan, lattice_pose(w, centre, p))
    return cost, pairs


def select(cost) -> int:
    """the lexicographic minimum of (cost, p) from (+inf, -1): ties to the lowest index, NaN and +inf never win"""
    best, bp = math.inf, -1
    for p, c in enumerate(cost):
        c = float(c)
        if c < best or (c == best and p < bp):
            best, bp = c, p
    return bp


def normalize_angle(t: float) -> float:
    """NormalizeAngle (H/util.hpp:125-135)"""
    t = math.fmod(t, 2.0 * math.pi)
    if t > math.pi:
        t -= 2.0 * math.pi
    elif t < -math.pi:
        t += 2.0 * math.pi
    return t


def _pose(p):
    return (p.x, p.y, p.theta) if hasattr(p, "theta") else tuple(p)


def gate_terms(s, start_pose):
    """what the gate compares, in its arithmetic; s: an abi.IcpSummary or an icp_oracle.Result"""
    ex, ey, et = _pose(s.estimated_pose)
    dx, dy = ex - start_pose[0], ey - start_pose[1]
    return s.num_pairs, s.normalized_cost, dx * dx + dy * dy, abs(normalize_angle(et - start_pose[2]))


def gate_accepts(gate, s, start_pose) -> bool:
    pairs, cost, d2, rot = gate_terms(s, start_pose)
    return bool(s.pose_found != 0 and pairs >= gate[0] and cost <= gate[1] and d2 <= gate[2] * gate[2]
                and rot <= gate[3])


def clear_of_thresholds(gate, s, start_pose, rel=1e-6) -> bool:
    """every floating-point comparison of the gate lies more than `rel` relative from its threshold"""
    _, cost, d2, rot = gate_terms(s, start_pose)
    far = lambda v, t: math.isinf(t) or abs(v - t) > rel * max(abs(v), abs(t))
    return far(cost, gate[1]) and far(d2, gate[2] * gate[2]) and far(rot, gate[3])


def record(node_pose, node_index: int, end_index: int, s, accepted: bool, scan_n: int) -> bytes:
    """the record of one candidate: 176 zero bytes, then the indices and the start node's pose; s (an
    abi.IcpSummary or an icp_oracle.Result, None: no refine ran) gives the estimate, the cost, the covariance
    and score = num_pairs / NumOfScans(); found and the loop edge only where the gate accepted"""
    r = abi.LoopResult()
    C.memset(C.byref(r), 0, C.sizeof(r))
    r.start_node_index, r.end_node_index = node_index, end_index
    r.start_node_pose = abi.Pose2D(*node_pose)
    if s is not None:
        est = _pose(s.estimated_pose)
        r.found = 1 if accepted else 0
        r.estimated_pose = abi.Pose2D(*est)
        r.score = float(np.float64(s.num_pairs) / np.float64(scan_n))
        r.normalized_cost = s.normalized_cost
        if accepted:
            rel = ob.lib().orc_inverse_compound(ob.Pose(*node_pose), ob.Pose(*est))
            r.relative_pose = abi.Pose2D(rel.x, rel.y, rel.theta)
        for k in range(9):
            r.covariance[k] = s.covariance[k]
    return bytes(r)
