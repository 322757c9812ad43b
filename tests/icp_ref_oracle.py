"""Test-side restatement of the multi-scan reference of the point-to-line ICP
(csrc/k_icp_ref.hip): the table is the concatenation of the
per-scan tables of tests/icp_oracle.py, in scan order then beam order, and the
pass, the loop and the summary are icp_oracle's over that table -- brute force
over every entry, which is what the device's grid search has to reproduce.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import icp_oracle as orc

RefTable = namedtuple("RefTable", "table k j")


def concat_tables(prm: orc.Params, refs, poses) -> RefTable:
    """refs: ScanIn per reference scan, poses: their robot poses.  Returns the
    concatenated table (its idx is the concatenated index) and, per entry, the
    reference scan k and its beam j."""
    parts = [orc.ref_table(prm, r, orc.compound(p, r.rel)) for r, p in zip(refs, poses)]
    cat = lambda name: np.concatenate([getattr(t, name) for t in parts]) if parts else np.zeros(0)
    k = np.concatenate([np.full(len(t.idx), i, dtype=np.int64) for i, t in enumerate(parts)])
    j = np.concatenate([t.idx for t in parts]).astype(np.int64)
    table = orc.Table(np.arange(len(j), dtype=np.int64), cat("qx"), cat("qy"), cat("nx"), cat("ny"))
    return RefTable(table, k, j)


def pairs(prm: orc.Params, rt: RefTable, scan: orc.ScanIn, sensor_pose):
    """(k, j, e) per beam of `scan`: -1 / -1 rejected, -2 / -2 unusable; also the pass's beams"""
    b = orc.pass_beams(prm, rt.table, scan, sensor_pose)
    hit = b.state >= 0
    at = np.maximum(b.state, 0)
    if len(rt.k):
        k = np.where(hit, rt.k[at], b.state)
        j = np.where(hit, rt.j[at], b.state)
    else:
        k, j = b.state.copy(), b.state.copy()
    return k, j, np.where(hit, b.e, 0.0), b


def nearest_d2(rt: RefTable, scan: orc.ScanIn, sensor_pose, i: int) -> float:
    """the smallest computed d2 of beam i over the whole table"""
    hx, hy, _, _ = orc.hit_points(scan.ranges, scan.angles, sensor_pose)
    dx, dy = hx[i] - rt.table.qx, hy[i] - rt.table.qy
    return float(np.min(dx * dx + dy * dy))


def refine(prm: orc.Params, refs, poses, scan: orc.ScanIn, initial_pose, rt: RefTable = None) -> orc.Result:
    rt = rt or concat_tables(prm, refs, poses)
    return orc.refine(prm, None, None, scan, initial_pose, table=rt.table)
