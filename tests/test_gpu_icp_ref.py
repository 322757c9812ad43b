"""The multi-scan reference of the point-to-line ICP (lgs_icp_ref_*,
csrc/k_icp_ref.hip) on the GPU.  Tolerance: none -- every
comparison is bit-exact: with one reference scan against the existing entry
points (lgs_icp_*), otherwise against the test-side restatement
(tests/icp_ref_oracle.py: brute force over the concatenated per-scan tables of
tests/icp_oracle.py), which the device's grid search has to reproduce.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import icp_oracle as orc
import icp_ref_oracle as rorc
from lgs_amd import abi, scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAPTER = os.path.join(ROOT, "tests", "cpp_icp_ref", "build", "icp_ref_adapter_test")
LGS_ERR_INVALID_ARG, LGS_ERR_INTERNAL = 1, 5
# tests/test_gpu_icp.py's scene and relative sensor poses
REF_POSE = (0.3, -0.2, 0.1)
TRUE_POSE = (0.5, 0.0, 0.15)
REL_REF, REL_CUR = (0.1, -0.05, 0.02), (-0.03, 0.08, -0.015)
O = (0.0, 0.0, 0.0)


def prm_for(n, cap=50, conv=0.0, D=1.0, reg=(1e-3, 1e-3)):
    return orc.Params(cap, conv, 0.01, 20.0, reg[0], reg[1], D, 3.0 if n < 100 else 0.5)


def dev_scan(ctx, s: orc.ScanIn):
    return ctx.scan(np.ascontiguousarray(s.ranges, dtype=np.float64), np.ascontiguousarray(s.angles, dtype=np.float64),
                    s.rel, s.min_range, s.max_range)


def dev_ref(ctx, prm, refs, poses):
    return ctx.icp_ref([dev_scan(ctx, r) for r in refs], poses, abi.IcpParams(*prm))


def bits(x):
    return np.float64(x).tobytes()


def same(a, b):
    return bits(a) == bits(b)


def pose_t(p):
    return (p.x, p.y, p.theta)


def assert_summary(dev, ref: orc.Result, init):
    assert dev.pose_found == ref.pose_found
    assert dev.iterations == ref.iterations
    assert dev.num_pairs == ref.num_pairs and dev.initial_pairs == ref.initial_pairs
    for name in ("cost", "pair_cost", "initial_cost", "normalized_cost"):
        assert same(getattr(dev, name), getattr(ref, name)), name
    for name, want in (("initial_pose", init), ("sensor_pose", ref.sensor_pose),
                       ("best_sensor_pose", ref.best_sensor_pose), ("estimated_pose", ref.estimated_pose)):
        got = pose_t(getattr(dev, name))
        assert all(same(g, w) for g, w in zip(got, want)), (name, got, want)
    assert all(same(g, w) for g, w in zip(dev.hessian, ref.hessian)), "hessian"
    assert all(same(g, w) for g, w in zip(dev.covariance, ref.covariance)), "covariance"


_SCENES = {}


def scene_pair(world, n):
    """tests/test_gpu_icp.py's (ref, cur): n beams taken at REF_POSE / TRUE_POSE (sensor poses)"""
    if n not in _SCENES:
        ang = scene.beam_angles(n)
        _SCENES[n] = (orc.ScanIn(scene.ray_cast(world, REF_POSE, ang), ang, REL_REF),
                      orc.ScanIn(scene.ray_cast(world, TRUE_POSE, ang), ang, REL_CUR))
    return _SCENES[n]


_SETS = {}
CUR_ROBOT = (0.65, 0.3, 0.21)


def scene_set(world, n, K):
    """the issue's loop scene, computed once: K reference scans of n beams at robot poses
    (0.1 k - 0.4, 0.05 k - 0.2, 0.02 k), the current scan at robot pose CUR_ROBOT; every scan is
    cast from its sensor pose Compound(robot pose, rel)"""
    if (n, K) not in _SETS:
        ang = scene.beam_angles(n)
        poses = [(0.1 * k - 0.4, 0.05 * k - 0.2, 0.02 * k) for k in range(K)]
        refs = [orc.ScanIn(scene.ray_cast(world, orc.compound(p, REL_REF), ang), ang, REL_REF) for p in poses]
        cur = orc.ScanIn(scene.ray_cast(world, orc.compound(CUR_ROBOT, REL_CUR), ang), ang, REL_CUR)
        _SETS[(n, K)] = (refs, poses, cur)
    return _SETS[(n, K)]


# ------------------------------------------------------------------ 1. K = 1 equals the existing path
@pytest.mark.parametrize("n", [65, 1081])
def test_one_reference_scan_equals_the_existing_entry_points(ctx, world, n):
    ref, cur = scene_pair(world, n)
    prm = abi.IcpParams(*prm_for(n, 50))
    ref_robot = orc.move_backward(REF_POSE, REL_REF)
    init = orc.move_backward((TRUE_POSE[0] + 0.2, TRUE_POSE[1] - 0.15, TRUE_POSE[2] + 0.05), REL_CUR)
    R, S = dev_scan(ctx, ref), dev_scan(ctx, cur)
    want, want_traj = ctx.icp(R, ref_robot, S, init, prm, trajectory=True)
    handle = ctx.icp_ref([R], [ref_robot], prm)
    got, got_traj = handle.refine(S, init, prm, trajectory=True)
    assert bytes(got) == bytes(want)
    assert np.array(got_traj).tobytes() == np.array(want_traj).tobytes() and len(got_traj) == want.iterations == 50
    assert got.pose_found == 1
    info = handle.info()
    usable = int(orc.usable_mask(ref.ranges, *orc.usable_range(prm_for(n), ref)).sum())
    assert (info.n_refs, info.entries) == (1, usable) and 0 < info.lines <= usable
    # the search alone, at a pose off the truth
    sensor = (TRUE_POSE[0] + 0.1, TRUE_POSE[1] - 0.1, TRUE_POSE[2] + 0.03)
    prm4 = abi.IcpParams(*prm_for(n, D=0.4))
    idx, res = ctx.icp_pairs(R, ref_robot, S, sensor, prm4)
    k, j, e = ctx.icp_ref([R], [ref_robot], prm4).pairs(S, sensor, prm4)
    assert j.tolist() == idx.tolist() and k.tolist() == np.where(idx >= 0, 0, idx).tolist()
    assert e.tobytes() == res.tobytes()
    assert (idx >= 0).sum() >= 3 and (idx == -1).sum() >= 1


# ------------------------------------------------------------------ 2. pairs against the restatement
def pairs_case(ctx, prm, refs, poses, cur, sensor_pose, handle=None):
    rt = rorc.concat_tables(prm, refs, poses)
    wk, wj, we, _ = rorc.pairs(prm, rt, cur, sensor_pose)
    handle = handle or dev_ref(ctx, prm, refs, poses)
    k, j, e = handle.pairs(dev_scan(ctx, cur), sensor_pose, abi.IcpParams(*prm))
    assert k.tolist() == wk.tolist()
    assert j.tolist() == wj.tolist()
    assert e.tobytes() == we.tobytes()
    assert handle.info().entries == len(rt.k)
    assert handle.info().lines == int(np.count_nonzero(~np.isnan(rt.table.nx)))
    return k, j, e


# test_gpu_icp.py::test_pairs_edge_cases' hand-made reference and current scan
EDGE_REF_A = [0.0, 0.001, 0.5, 0.5, 0.501, 1.0, 1.2, 1.201, 1.5, 1.8, 1.801, 1.802, -0.5, -0.499]
EDGE_REF_R = [1.0, 1.0, 2.0, 2.0, 2.0, 3.0, 25.0, 3.0, 3.0, 4.0, 25.0, 4.0, 5.0, 6.0]
EDGE_CUR_A = [0.0, 0.0, 0.5, 1.0, 1.201, 1.8, -0.5, 0.0, 0.0005, 0.0]
EDGE_CUR_R = [1.5, math.nextafter(1.5, 2.0), 2.1, 3.0, 3.05, 4.0, 5.1, 25.0, 1.2, 0.005]


@pytest.mark.parametrize("cuts", [(14,), (7, 14), (3, 14), (5, 10, 14), (1, 13, 14)])
def test_pairs_edge_cases_split_over_scans(ctx, cuts):
    """the hand-made reference as one scan and cut into two and three: gaps, duplicates and lines at scan
    ends (a line never crosses from one scan into the next)"""
    a, r = np.array(EDGE_REF_A), np.array(EDGE_REF_R)
    refs, lo = [], 0
    for hi in cuts:
        refs.append(orc.ScanIn(r[lo:hi].copy(), a[lo:hi].copy()))
        lo = hi
    cur = orc.ScanIn(np.array(EDGE_CUR_R), np.array(EDGE_CUR_A))
    prm = orc.Params(1, 0.0, 0.01, 20.0, 0.0, 0.0, 0.5, 0.5)
    k, j, _ = pairs_case(ctx, prm, refs, [O] * len(refs), cur, O)
    assert j[1] == -1 and k[1] == -1, "one ulp beyond D^2 is rejected"
    assert (k[7], j[7], k[9], j[9]) == (-2, -2, -2, -2), "unusable beams of the current scan"
    if cuts == (14,):
        assert (k[0], j[0]) == (0, 0), "a beam exactly at D^2 (d2 == 0.25) is accepted"
    if cuts == (1, 13, 14):
        assert (k[0], j[0]) == (-1, -1), "beam 0's line to beam 1 would cross a scan end: no line, rejected"
    prm2 = prm._replace(max_segment_length=3.0)
    k2, j2, _ = pairs_case(ctx, prm2, refs, [O] * len(refs), cur, O)
    if cuts == (14,):
        assert (k2[2], j2[2]) == (0, 2), "duplicate reference points: the lowest index wins"
    if cuts == (3, 14):
        # the duplicates 2 and 3 now sit in different scans: 2 is scan 0's last beam, 3 scan 1's first
        assert (k2[2], j2[2]) == (0, 2)


def test_the_same_scan_twice_ties_go_to_copy_zero(ctx, world):
    ref, cur = scene_pair(world, 65)
    prm = prm_for(65, D=0.4)
    p = orc.move_backward(REF_POSE, REL_REF)
    sensor = (TRUE_POSE[0] + 0.1, TRUE_POSE[1] - 0.1, TRUE_POSE[2] + 0.03)
    k, j, _ = pairs_case(ctx, prm, [ref, ref], [p, p], cur, sensor)
    assert (k >= 0).sum() >= 3 and set(k[k >= 0].tolist()) == {0}


def test_the_d2_boundary(ctx, world):
    """D = sqrt(nearest d2) of a beam and its two neighbours: whatever the products D * D give, the
    restatement's answer"""
    refs, poses, cur = scene_set(world, 65, 3)
    sensor = orc.compound((0.6, 0.25, 0.2), REL_CUR)
    base = prm_for(65, D=1.0)
    rt = rorc.concat_tables(base, refs, poses)
    us = np.flatnonzero(orc.usable_mask(cur.ranges, *orc.usable_range(base, cur)))
    seen = set()
    for i in us[[3, len(us) // 2, -4]]:
        d = math.sqrt(rorc.nearest_d2(rt, cur, sensor, int(i)))
        assert 0.0 < d < 1.0
        for D in (math.nextafter(d, 0.0), d, math.nextafter(d, 1.0)):
            prm = base._replace(max_correspondence_dist=D)
            k, _, _ = pairs_case(ctx, prm, refs, poses, cur, sensor)
            seen.add(int(k[i]) >= 0)
    assert seen == {True, False}, "the boundary was crossed"


def test_beams_outside_the_tables_bounding_box(ctx, world):
    """single beams whose hit point lies beyond the table's extreme points by less and by more than D"""
    refs, poses, _ = scene_set(world, 65, 3)
    prm = prm_for(65, D=0.3)
    handle = dev_ref(ctx, prm, refs, poses)
    rt = rorc.concat_tables(prm, refs, poses)
    t = rt.table
    right, low = int(np.argmax(t.qx)), int(np.argmin(t.qy))
    within = 0
    for delta in (0.5, 0.999, 1.0, 1.001, 1.5, 3.0, 40.0):
        d = delta * 0.3
        # angle 0, range 1: the hit point is the sensor's + (1, 0); angle -pi/2: + (~0, -1)
        beam_x = orc.ScanIn(np.array([1.0]), np.array([0.0]))
        k, _, _ = pairs_case(ctx, prm, refs, poses, beam_x, (t.qx[right] + d - 1.0, t.qy[right], 0.0), handle)
        within += int(rorc.nearest_d2(rt, beam_x, (t.qx[right] + d - 1.0, t.qy[right], 0.0), 0) <= 0.09)
        beam_y = orc.ScanIn(np.array([1.0]), np.array([-math.pi / 2]))
        pairs_case(ctx, prm, refs, poses, beam_y, (t.qx[low], t.qy[low] - d + 1.0, 0.0), handle)
        if delta > 1.001:
            assert k[0] == -1
    assert within >= 2


def test_poses_near_1e5(ctx, world):
    refs, poses, cur = scene_set(world, 65, 3)
    far = lambda p: (p[0] + 1e5, p[1] - 1e5, p[2])
    prm = prm_for(65, D=0.4)
    sensor = far(orc.compound((0.6, 0.25, 0.2), REL_CUR))
    k, _, _ = pairs_case(ctx, prm, refs, [far(p) for p in poses], cur, sensor)
    assert (k >= 0).sum() >= 3
    prm = prm_for(65, D=0.01)
    pairs_case(ctx, prm, refs, [far(p) for p in poses], cur, far(orc.compound(CUR_ROBOT, REL_CUR)))


@pytest.mark.parametrize("D", [1e-3, 100.0])
def test_very_small_and_very_large_distances(ctx, world, D):
    refs, poses, cur = scene_set(world, 361, 10)
    prm = prm_for(361, D=D)
    handle = dev_ref(ctx, prm, refs, poses)
    k, _, _ = pairs_case(ctx, prm, refs, poses, cur, orc.compound(CUR_ROBOT, REL_CUR), handle)
    info = handle.info()
    if D == 100.0:
        assert (info.cells_x, info.cells_y) == (1, 1) and (k >= 0).sum() > 100
    else:
        assert max(info.cells_x, info.cells_y) == 1024 and info.cell_size > 2 * D


def test_a_sensor_pose_at_1e300_rejects_every_beam(ctx, world):
    refs, poses, cur = scene_set(world, 65, 3)
    prm = prm_for(65)
    k, j, _ = pairs_case(ctx, prm, refs, poses, cur, (1e300, 0.0, 0.0))
    us = orc.usable_mask(cur.ranges, *orc.usable_range(prm, cur))
    assert k.tolist() == np.where(us, -1, -2).tolist() and us.sum() > 3


def test_a_one_entry_table_and_an_all_unusable_reference(ctx, world):
    ref = orc.ScanIn(np.array([25.0, 2.0, 25.0]), np.array([-0.1, 0.0, 0.1]))
    none = orc.ScanIn(np.array([25.0, 25.0]), np.array([0.0, 0.1]))
    cur = orc.ScanIn(np.array([2.0, 2.1, 30.0]), np.array([0.0, 0.01, 0.02]))
    prm = prm_for(3)
    k, _, _ = pairs_case(ctx, prm, [none, ref, none], [O, O, O], cur, O)
    assert k.tolist() == [-1, -1, -2]
    handle = dev_ref(ctx, prm, [none, none], [O, (1.0, 2.0, 0.5)])
    info = handle.info()
    assert (info.n_refs, info.entries, info.lines, info.cells_x, info.cells_y) == (2, 0, 0, 1, 1)
    k, j, e = handle.pairs(dev_scan(ctx, cur), O, abi.IcpParams(*prm))
    assert k.tolist() == j.tolist() == [-1, -1, -2] and not e.any()
    _, cur65 = scene_pair(world, 65)
    out = handle.refine(dev_scan(ctx, cur65), TRUE_POSE, abi.IcpParams(*prm))
    assert out.pose_found == 0 and out.iterations == 0 and out.initial_pairs == 0 and out.num_pairs == 0
    assert_summary(out, rorc.refine(prm, [none, none], [O, (1.0, 2.0, 0.5)], cur65, TRUE_POSE), TRUE_POSE)


# ------------------------------------------------------------------ 3. beyond the one-scan cap
def test_one_reference_scan_of_4200_usable_beams(ctx):
    n = 4200
    ang = np.linspace(-2.0, 2.0, n + 3)
    rng = 4.0 + 0.5 * np.sin(7.0 * ang)
    ranges = rng.copy()
    ranges[[10, 2000, 4000]] = 25.0     # n + 3 beams, 3 unusable: n usable
    ref = orc.ScanIn(ranges, ang)
    cur = orc.ScanIn(rng[::50].copy(), ang[::50].copy())
    prm = orc.Params(2, 0.0, 0.01, 20.0, 1e-3, 1e-3, 0.5, 0.5)
    handle = dev_ref(ctx, prm, [ref], [O])
    assert handle.info().entries == 4200
    k, _, _ = pairs_case(ctx, prm, [ref], [O], cur, (0.02, -0.01, 0.003), handle)
    assert (k == 0).sum() > 50
    with pytest.raises(abi.LgsError):   # the one-scan entry point still refuses it
        ctx.icp_pairs(dev_scan(ctx, ref), O, dev_scan(ctx, cur), O, abi.IcpParams(*prm))


# ------------------------------------------------------------------ 4. the whole loop against the restatement
STARTS = [(0.4, 0.1, 0.15), (0.8, 0.45, 0.27)]


@pytest.mark.parametrize("start", range(2))
@pytest.mark.parametrize("n,K,steps", [(65, 3, 5), (361, 10, 5), (1081, 10, 3)])
def test_every_step_and_the_whole_loop(ctx, world, n, K, steps, start):
    refs, poses, cur = scene_set(world, n, K)
    prm = prm_for(n, steps)
    init = STARTS[start]
    key = ("table", n, K)
    if key not in _SETS:
        _SETS[key] = rorc.concat_tables(prm, refs, poses)
    rt = _SETS[key]
    handle = dev_ref(ctx, prm, refs, poses)
    out, traj = handle.refine(dev_scan(ctx, cur), init, abi.IcpParams(*prm), trajectory=True)
    want = rorc.refine(prm, refs, poses, cur, init, rt)
    assert len(traj) == out.iterations == want.iterations == steps
    for s, (g, w) in enumerate(zip(traj, want.trajectory)):
        assert all(same(a, b) for a, b in zip(g, w)), f"step {s}: pose, cost, pairs {g} != {w}"
    assert_summary(out, want, init)
    assert out.pose_found == 1
    e = out.estimated_pose
    d0, a0 = math.hypot(init[0] - CUR_ROBOT[0], init[1] - CUR_ROBOT[1]), abs(init[2] - CUR_ROBOT[2])
    d1, a1 = math.hypot(e.x - CUR_ROBOT[0], e.y - CUR_ROBOT[1]), abs(e.theta - CUR_ROBOT[2])
    print(f"n {n}, K {K}, start {start}: {d0:.4f} m / {a0:.4f} rad -> {d1:.3e} m / {a1:.3e} rad, {out.num_pairs} pairs")
    assert d1 < d0 and a1 < a0


# ------------------------------------------------------------------ 5. stability of the bytes
def batch_setup(ctx, world):
    refs3, poses3, cur65 = scene_set(world, 65, 3)
    refs10, poses10, cur361 = scene_set(world, 361, 10)
    prm = orc.Params(5, 0.0, 0.01, 20.0, 1e-3, 1e-3, 1.0, 3.0)
    p = abi.IcpParams(*prm)
    H3 = dev_ref(ctx, prm, refs3, poses3)
    H10 = dev_ref(ctx, prm, refs10, poses10)
    H1 = dev_ref(ctx, prm, refs10[4:5], poses10[4:5])
    C65, C361 = dev_scan(ctx, cur65), dev_scan(ctx, cur361)
    far = (CUR_ROBOT[0] + 60.0, CUR_ROBOT[1] + 60.0, CUR_ROBOT[2] + 1.0)   # outside the room: not found
    items = [(H10, C361, STARTS[0]), (H3, C65, STARTS[1]), (H10, C65, far), (H1, C361, STARTS[0]),
             (H3, C361, STARTS[0]), (H10, C361, STARTS[0])]
    return items, p


def test_batch_equals_lone_calls(ctx, world):
    """six items: K = 1, 3 and 10 mixed, references and scans repeated, found and not found"""
    items, p = batch_setup(ctx, world)
    got = items[0][0].refine_batch([i[1] for i in items], [i[2] for i in items], p, refs=[i[0] for i in items])
    lone = [h.refine(s, ip, p) for h, s, ip in items]
    assert [bytes(g) for g in got] == [bytes(l) for l in lone]
    assert sorted({l.pose_found for l in lone}) == [0, 1]
    assert bytes(got[0]) == bytes(got[5])
    assert items[0][0].refine_batch([], [], p) == []
    same_ref = items[0][0].refine_batch([items[0][1]] * 3, [STARTS[0], STARTS[1], STARTS[0]], p)
    assert bytes(same_ref[0]) == bytes(same_ref[2]) == bytes(lone[0]) != bytes(same_ref[1])


def test_two_runs_two_contexts_and_destroyed_scans(ctx, world):
    refs, poses, cur = scene_set(world, 361, 10)
    prm = orc.Params(5, 0.0, 0.01, 20.0, 1e-3, 1e-3, 1.0, 3.0)
    p = abi.IcpParams(*prm)
    scans = [dev_scan(ctx, r) for r in refs]
    handle = ctx.icp_ref(scans, poses, p)
    S = dev_scan(ctx, cur)
    a = handle.refine(S, STARTS[0], p)
    for s in scans:   # the reference copied what it needs
        s.close()
    b = handle.refine(S, STARTS[0], p)
    again = dev_ref(ctx, prm, refs, poses)
    c = again.refine(S, STARTS[0], p)
    other = abi.Context(0)
    try:
        theirs = dev_ref(other, prm, refs, poses)
        d = theirs.refine(dev_scan(other, cur), STARTS[0], p)
        assert theirs.info() == handle.info()
    finally:
        other.close()
    theirs.close()   # after its context, as an lgs_grid may be
    assert bytes(a) == bytes(b) == bytes(c) == bytes(d)
    assert a.pose_found == 1 and a.iterations == 5


# ------------------------------------------------------------------ 6. validation
NAN, INF = float("nan"), float("inf")
GOOD = orc.Params(5, 0.0, 0.01, 20.0, 1e-3, 1e-3, 1.0, 0.5)
BAD_PARAMS = {
    "conv_nan": GOOD._replace(convergence_threshold=NAN), "range_min_inf": GOOD._replace(usable_range_min=-INF),
    "range_max_inf": GOOD._replace(usable_range_max=INF), "reg_t_nan": GOOD._replace(translation_regularizer=NAN),
    "reg_r_inf": GOOD._replace(rotation_regularizer=INF), "dist_nan": GOOD._replace(max_correspondence_dist=NAN),
    "seg_inf": GOOD._replace(max_segment_length=INF), "dist_zero": GOOD._replace(max_correspondence_dist=0.0),
    "dist_negative": GOOD._replace(max_correspondence_dist=-1.0), "seg_zero": GOOD._replace(max_segment_length=0.0),
    "reg_t_negative": GOOD._replace(translation_regularizer=-1e-9),
    "reg_r_negative": GOOD._replace(rotation_regularizer=-1.0),
}
BAD_POSES = {"x_nan": (NAN, 0.0, 0.0), "y_inf": (0.0, INF, 0.0), "theta_nan": (0.0, 0.0, NAN), "theta_inf": (0.0, 0.0, -INF)}
IP = C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def small(ctx, world):
    ref, cur = scene_pair(world, 65)
    R, S = dev_scan(ctx, ref), dev_scan(ctx, cur)
    return R, S, ctx.icp_ref([R, R], [REF_POSE, (0.35, -0.2, 0.1)], abi.IcpParams(*GOOD))


def raw_create(ctx, scans, poses, n, prm, null=None):
    """lgs_icp_ref_create on a poisoned out pointer; (status, untouched)"""
    P = abi.Pose2D
    p = abi.IcpParams(*prm)
    arr = (C.c_void_p * max(1, len(scans)))(*[s.h if s is not None else None for s in scans])
    ps = (P * max(1, len(poses)))(*[P(*q) for q in poses])
    out = C.c_void_p(0xABABABAB)
    a = dict(ctx=ctx.h, scans=arr, poses=ps, prm=C.byref(p), out=C.byref(out))
    if null:
        a[null] = None
    st = ctx.lib.lgs_icp_ref_create(a["ctx"], a["scans"], a["poses"], n, a["prm"], a["out"])
    untouched = out.value == 0xABABABAB
    if st == 0:
        ctx.lib.lgs_icp_ref_destroy(out)
    return st, untouched


def raw_calls(ctx, handle, S, init, prm, null=None):
    """the three refine-time entry points on poisoned outputs; [(status, untouched)]"""
    lib, P = ctx.lib, abi.Pose2D
    p = abi.IcpParams(*prm)
    res = []
    out = abi.IcpSummary()
    C.memset(C.byref(out), 0xAB, C.sizeof(out))
    before = bytes(out)
    traj = np.full(5 * 8, 7.0)
    a = dict(ctx=ctx.h, ref=handle.h, scan=S.h, prm=C.byref(p), out=C.byref(out))
    if null:
        a[null] = None
    st = lib.lgs_icp_ref_optimize_pose(a["ctx"], a["ref"], a["scan"], P(*init), a["prm"], a["out"], abi.dptr(traj))
    res.append((st, bytes(out) == before and (traj == 7.0).all()))
    outs = (abi.IcpSummary * 2)()
    C.memset(outs, 0xAB, C.sizeof(outs))
    before = bytes(outs)
    rarr, sarr = (C.c_void_p * 2)(handle.h, a["ref"]), (C.c_void_p * 2)(S.h, a["scan"])
    ip = (P * 2)(P(*TRUE_POSE), P(*init))
    st = lib.lgs_icp_ref_optimize_pose_batch(a["ctx"], rarr, sarr, ip, 2, a["prm"], outs if a["out"] else None)
    res.append((st, bytes(outs) == before))
    k, j = np.full(len(S.ranges), 77, dtype=np.int32), np.full(len(S.ranges), 77, dtype=np.int32)
    e = np.full(len(S.ranges), 7.0)
    st = lib.lgs_icp_ref_pairs(a["ctx"], a["ref"], a["scan"], P(*init), a["prm"],
                               k.ctypes.data_as(IP) if a["out"] else None, j.ctypes.data_as(IP), abi.dptr(e))
    res.append((st, (k == 77).all() and (j == 77).all() and (e == 7.0).all()))
    return res


def test_valid_arguments_pass_the_raw_calls(ctx, small):
    R, S, handle = small
    assert raw_create(ctx, [R, R], [REF_POSE, TRUE_POSE], 2, GOOD) == (0, False)
    assert [st for st, _ in raw_calls(ctx, handle, S, TRUE_POSE, GOOD)] == [0, 0, 0]
    # the parameters the table does not depend on are free at refine time
    free = GOOD._replace(num_iterations_max=2, convergence_threshold=1e-3, translation_regularizer=0.0,
                         rotation_regularizer=0.5)
    assert [st for st, _ in raw_calls(ctx, handle, S, TRUE_POSE, free)] == [0, 0, 0]


@pytest.mark.parametrize("case", list(BAD_PARAMS))
def test_invalid_parameters(ctx, small, case):
    R, S, handle = small
    assert raw_create(ctx, [R], [REF_POSE], 1, BAD_PARAMS[case]) == (LGS_ERR_INVALID_ARG, True)
    assert raw_calls(ctx, handle, S, TRUE_POSE, BAD_PARAMS[case]) == [(LGS_ERR_INVALID_ARG, True)] * 3


@pytest.mark.parametrize("case", list(BAD_POSES))
def test_poses_that_are_not_finite(ctx, small, case):
    R, S, handle = small
    assert raw_create(ctx, [R, R], [REF_POSE, BAD_POSES[case]], 2, GOOD) == (LGS_ERR_INVALID_ARG, True)
    assert raw_calls(ctx, handle, S, BAD_POSES[case], GOOD) == [(LGS_ERR_INVALID_ARG, True)] * 3


@pytest.mark.parametrize("null", ["ctx", "ref", "scan", "prm", "out"])
def test_null_arguments_at_refine_time(ctx, small, null):
    R, S, handle = small
    assert raw_calls(ctx, handle, S, TRUE_POSE, GOOD, null=null) == [(LGS_ERR_INVALID_ARG, True)] * 3


def test_null_arguments_counts_and_arrays(ctx, small):
    R, S, handle = small
    lib, P = ctx.lib, abi.Pose2D
    for null in ("ctx", "scans", "poses", "prm", "out"):
        st, untouched = raw_create(ctx, [R], [REF_POSE], 1, GOOD, null=null)
        assert st == LGS_ERR_INVALID_ARG and (untouched or null == "out"), null
    assert raw_create(ctx, [R, None], [REF_POSE, REF_POSE], 2, GOOD) == (LGS_ERR_INVALID_ARG, True)
    with pytest.raises(abi.LgsError):   # an empty scan cannot reach the matcher: lgs_scan_create refuses to make one
        ctx.scan(np.zeros(0), np.zeros(0))
    assert raw_create(ctx, [R], [REF_POSE], 0, GOOD) == (LGS_ERR_INVALID_ARG, True)
    assert raw_create(ctx, [R], [REF_POSE], -1, GOOD) == (LGS_ERR_INVALID_ARG, True)
    assert raw_create(ctx, [R] * 4097, [REF_POSE] * 4097, 4097, GOOD) == (LGS_ERR_INVALID_ARG, True)
    p = abi.IcpParams(*GOOD)
    out = abi.IcpSummary()
    C.memset(C.byref(out), 0xAB, C.sizeof(out))
    before = bytes(out)
    rarr, sarr, ip = (C.c_void_p * 1)(handle.h), (C.c_void_p * 1)(S.h), (P * 1)(P(*TRUE_POSE))
    f = lib.lgs_icp_ref_optimize_pose_batch
    assert f(ctx.h, rarr, sarr, ip, -1, C.byref(p), C.byref(out)) == LGS_ERR_INVALID_ARG
    assert f(ctx.h, None, sarr, ip, 1, C.byref(p), C.byref(out)) == LGS_ERR_INVALID_ARG
    assert f(ctx.h, rarr, None, ip, 1, C.byref(p), C.byref(out)) == LGS_ERR_INVALID_ARG
    assert f(ctx.h, rarr, sarr, None, 1, C.byref(p), C.byref(out)) == LGS_ERR_INVALID_ARG
    assert f(ctx.h, rarr, sarr, ip, 0, C.byref(p), C.byref(out)) == 0
    assert bytes(out) == before
    k = np.zeros(len(S.ranges), dtype=np.int32)
    assert lib.lgs_icp_ref_pairs(ctx.h, handle.h, S.h, P(*TRUE_POSE), C.byref(p), k.ctypes.data_as(IP), None,
                                 abi.dptr(np.zeros(len(S.ranges)))) == LGS_ERR_INVALID_ARG
    assert lib.lgs_icp_ref_pairs(ctx.h, handle.h, S.h, P(*TRUE_POSE), C.byref(p), k.ctypes.data_as(IP),
                                 k.ctypes.data_as(IP), None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_icp_ref_info(None, None, None, None, None, None, None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_icp_ref_info(handle.h, None, None, None, None, None, None) == 0
    assert lib.lgs_icp_ref_optimize_pose(ctx.h, handle.h, S.h, P(*TRUE_POSE), C.byref(p), C.byref(out), None) == 0
    assert bytes(out) != before and out.pose_found == 1
    lib.lgs_icp_ref_destroy(None)


@pytest.mark.parametrize("field", ["usable_range_min", "usable_range_max", "max_segment_length",
                                   "max_correspondence_dist"])
def test_refine_time_parameters_must_be_the_references(ctx, small, field):
    R, S, handle = small
    other = GOOD._replace(**{field: math.nextafter(getattr(GOOD, field), 1e9)})
    assert raw_calls(ctx, handle, S, TRUE_POSE, other) == [(LGS_ERR_INVALID_ARG, True)] * 3


def test_a_reference_of_another_context(ctx, small):
    R, S, handle = small
    other = abi.Context(0)
    try:
        theirs = other.icp_ref([R], [REF_POSE], abi.IcpParams(*GOOD))   # the scan may be anyone's, as for lgs_icp_*
        assert raw_calls(ctx, theirs, S, TRUE_POSE, GOOD) == [(LGS_ERR_INVALID_ARG, True)] * 3
        assert [st for st, _ in raw_calls(other, theirs, S, TRUE_POSE, GOOD)] == [0, 0, 0]
        theirs.close()
    finally:
        other.close()


def test_the_entry_cap(ctx):
    """64 scans of 4096 usable beams are a reference; 65 are refused before any device work"""
    ang = np.linspace(-2.0, 2.0, 4096)
    rng = 4.0 + 0.5 * np.sin(7.0 * ang)
    scans = [ctx.scan(rng + 1e-3 * k, ang) for k in range(65)]
    poses = [(0.01 * k, 0.0, 0.0) for k in range(65)]
    st, untouched = raw_create(ctx, scans, poses, 65, GOOD)
    assert (st, untouched) == (LGS_ERR_INVALID_ARG, True)
    assert all(s.h for s in scans)
    handle = ctx.icp_ref(scans[:64], poses[:64], abi.IcpParams(*GOOD))
    assert handle.info().entries == 262144 and handle.info().n_refs == 64
    cur = orc.ScanIn(rng[::64].copy(), ang[::64].copy())
    k, j, _ = handle.pairs(dev_scan(ctx, cur), (0.005, 0.002, 0.001), abi.IcpParams(*GOOD))
    assert (k >= 0).sum() > 32


def test_angle_outside_the_sincos_domain(ctx, small):
    """|theta + angle| >= 105414350: LGS_ERR_INTERNAL, at create for the reference scans' angles and at
    refine for the scan's; the outputs as they were"""
    R, S, handle = small
    far = (0.0, 0.0, 2.0e8)
    assert raw_create(ctx, [R, R], [REF_POSE, far], 2, GOOD) == (LGS_ERR_INTERNAL, True)
    assert raw_calls(ctx, handle, S, far, GOOD) == [(LGS_ERR_INTERNAL, True)] * 3
    assert [st for st, _ in raw_calls(ctx, handle, S, TRUE_POSE, GOOD)] == [0, 0, 0]


# ------------------------------------------------------------------ 7. the adapter
def test_adapter_multi_scan_reference(ctx, world, tmp_path):
    """ScanMatcherIcpPointToLineHip::SetReference(scans, poses) through its C++ driver, against the
    bindings' result on the same inputs (which test 4 holds to the restatement)"""
    assert os.path.exists(ADAPTER), "build first: make -C <repo> all"
    refs, poses, cur = scene_set(world, 361, 10)
    cur = cur._replace(rel=REL_REF)   # the driver gives every scan one relative sensor pose
    prm = orc.Params(5, 0.0, 0.01, 20.0, 1e-3, 1e-3, 1.0, 0.5)
    init = STARTS[0]
    out = dev_ref(ctx, prm, refs, poses).refine(dev_scan(ctx, cur), init, abi.IcpParams(*prm))
    assert out.pose_found == 1
    hx = lambda v: " ".join(float(x).hex() for x in v)
    lines = [f"{len(refs)} {len(cur.ranges)} {prm.num_iterations_max}", hx(prm[1:]), hx(REL_REF), hx(cur.angles)]
    for r, p in zip(refs, poses):
        lines += [hx(p), hx(r.ranges)]
    lines += [hx(cur.ranges), hx(init), f"{out.pose_found}", hx([out.normalized_cost]), hx(pose_t(out.estimated_pose)),
              hx(out.covariance)]
    case = tmp_path / "case.txt"
    case.write_text("\n".join(lines) + "\n")
    r = subprocess.run([ADAPTER, str(case)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ICP REF ADAPTER TESTS PASSED" in r.stdout
