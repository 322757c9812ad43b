"""The point-to-line ICP matcher (lgs_icp_*, csrc/k_icp.hip) on the GPU against
the test-side restatement of its contract (tests/icp_oracle.py, DESIGN.md
4.5b).  Tolerance: none -- every comparison is bit-exact -- except the one
test that compares a pass's eleven sums with math.fsum, whose bound is the
tree's: k * 2^-53 * sum |term|, k = rounds - 1 + 6 + 15 additions on the
longest path.

A note on one case of the issue: it lists "a pose that is not finite" among
the invalid arguments and also a fewer-than-3-pairs case "with a NaN initial
pose".  The entry points refuse a NaN initial pose (the first rule), so the
second cannot be reached through them; the rule that a NaN pose pairs nothing
is covered by the restatement (tests/test_icp_cpu.py).
"""
import ctypes as C
import math

import numpy as np
import pytest

import icp_oracle as orc
from lgs_amd import abi, scene

pytestmark = pytest.mark.gpu

LGS_ERR_INVALID_ARG, LGS_ERR_INTERNAL = 1, 5
REF_POSE = (0.3, -0.2, 0.1)
TRUE_POSE = (0.5, 0.0, 0.15)
REL_REF, REL_CUR = (0.1, -0.05, 0.02), (-0.03, 0.08, -0.015)


def prm_for(n, cap=50, conv=0.0, D=1.0, reg=(1e-3, 1e-3)):
    return orc.Params(cap, conv, 0.01, 20.0, reg[0], reg[1], D, 3.0 if n < 100 else 0.5)


def dev_scan(ctx, s: orc.ScanIn):
    return ctx.scan(np.ascontiguousarray(s.ranges, dtype=np.float64), np.ascontiguousarray(s.angles, dtype=np.float64),
                    s.rel, s.min_range, s.max_range)


def sensor_to_robot(sensor, rel):
    """the robot pose whose Compound with rel is (close to) `sensor`; only used to place scenes"""
    return orc.move_backward(sensor, rel)


_SCENES = {}


def scene_pair(world, n, rel=True):
    """(ref, cur) scans of n beams taken at REF_POSE / TRUE_POSE (sensor poses), computed once"""
    key = (n, rel)
    if key not in _SCENES:
        ang = scene.beam_angles(n)
        ref = orc.ScanIn(scene.ray_cast(world, REF_POSE, ang), ang, REL_REF if rel else (0.0, 0.0, 0.0))
        cur = orc.ScanIn(scene.ray_cast(world, TRUE_POSE, ang), ang, REL_CUR if rel else (0.0, 0.0, 0.0))
        _SCENES[key] = (ref, cur)
    return _SCENES[key]


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


# ------------------------------------------------------------------ the search alone
def pairs_case(ctx, prm, ref, ref_pose, cur, sensor_pose):
    table = orc.ref_table(prm, ref, orc.compound(ref_pose, ref.rel))
    b = orc.pass_beams(prm, table, cur, sensor_pose)
    want_idx = np.where(b.state >= 0, table.idx[np.maximum(b.state, 0)] if len(table.idx) else -1, b.state)
    idx, res = ctx.icp_pairs(dev_scan(ctx, ref), ref_pose, dev_scan(ctx, cur), sensor_pose, abi.IcpParams(*prm))
    assert idx.tolist() == want_idx.tolist()
    assert res.tobytes() == np.where(b.state >= 0, b.e, 0.0).tobytes()
    return idx, res


def test_pairs_edge_cases(ctx):
    """duplicates, the D^2 boundary, a beam without a line, an over-long
    segment, unusable beams and gaps -- each also asserted outright"""
    O = (0.0, 0.0, 0.0)
    # reference beams (angle, range); 25.0 is beyond the usable range
    ref_a = [0.0, 0.001, 0.5, 0.5, 0.501, 1.0, 1.2, 1.201, 1.5, 1.8, 1.801, 1.802, -0.5, -0.499]
    ref_r = [1.0, 1.0, 2.0, 2.0, 2.0, 3.0, 25.0, 3.0, 3.0, 4.0, 25.0, 4.0, 5.0, 6.0]
    #  0,1   a line 1 mm long; 0 sits exactly at (1, 0)
    #  2,3   duplicate points (l2 == 0 between them: 2 has no line, 3 takes 4)
    #  5     neighbours 4 (far: > max_segment_length) and 6 (unusable): no line
    #  7,8   7's neighbours are 6 (unusable) and 8, 0.9 m away: with max_segment_length 0.5 no line either
    #  9,11  separated by the unusable 10: a gap inside the reference, no lines
    #  12,13 1 m apart along the beam: a segment longer than max_segment_length
    ref = orc.ScanIn(np.array(ref_r), np.array(ref_a))
    prm = orc.Params(1, 0.0, 0.01, 20.0, 0.0, 0.0, 0.5, 0.5)
    up = math.nextafter(1.5, 2.0)
    cur_a = [0.0, 0.0, 0.5, 1.0, 1.201, 1.8, -0.5, 0.0, 0.0005, 0.0]
    cur_r = [1.5, up, 2.1, 3.0, 3.05, 4.0, 5.1, 25.0, 1.2, 0.005]
    cur = orc.ScanIn(np.array(cur_r), np.array(cur_a))
    idx, res = pairs_case(ctx, prm, ref, O, cur, O)
    assert idx[0] == 0, "a beam exactly at D^2 (d2 == 0.25) is accepted"
    assert idx[1] == -1, "one ulp beyond D^2 is rejected"
    assert idx[3] == -1, "nearest reference beam has no line: rejected"
    assert idx[4] == -1, "its only usable neighbour is farther than max_segment_length"
    assert idx[5] == -1, "a gap inside the reference breaks the line"
    assert idx[6] == -1, "a segment longer than max_segment_length"
    assert idx[7] == -2 and idx[9] == -2, "unusable beams of the current scan"
    assert idx[8] in (0, 1), "an ordinary pair"
    # duplicates: the lowest index wins the tie.  Beam 2 of cur is nearest to the
    # duplicate points 2 and 3 alike; 2 wins and has no line (l2 == 0 to 3, 1 is far)
    assert idx[2] == -1
    # with a longer segment allowed, 2 takes its line to 1 and still wins the tie
    prm2 = prm._replace(max_segment_length=3.0)
    idx2, _ = pairs_case(ctx, prm2, ref, O, cur, O)
    assert idx2[2] == 2, "duplicate reference points: the lowest index wins"
    assert idx2[6] == 12


def test_pairs_single_usable_reference_beam(ctx):
    """M = 1: one entry, no line, every usable beam rejected"""
    ref = orc.ScanIn(np.array([25.0, 2.0, 25.0]), np.array([-0.1, 0.0, 0.1]))
    cur = orc.ScanIn(np.array([2.0, 2.1, 30.0]), np.array([0.0, 0.01, 0.02]))
    idx, _ = pairs_case(ctx, prm_for(3), ref, (0.0, 0.0, 0.0), cur, (0.0, 0.0, 0.0))
    assert idx.tolist() == [-1, -1, -2]


def test_pairs_empty_table(ctx):
    ref = orc.ScanIn(np.array([25.0, 25.0]), np.array([0.0, 0.1]))
    cur = orc.ScanIn(np.array([2.0, 25.0]), np.array([0.0, 0.01]))
    idx, _ = pairs_case(ctx, prm_for(3), ref, (0.0, 0.0, 0.0), cur, (0.0, 0.0, 0.0))
    assert idx.tolist() == [-1, -2]


@pytest.mark.parametrize("n", [65, 1081])
def test_pairs_scene_with_relative_sensor_poses(ctx, world, n):
    """a non-zero relative sensor pose on both scans; unusable beams in both (ranges past 20 m,
    and a block of the reference cut out: gaps inside it)"""
    ref, cur = scene_pair(world, n)
    r = ref.ranges.copy()
    r[n // 3: n // 3 + 5] = 25.0
    r[n // 2] = 0.001
    ref = ref._replace(ranges=r)
    prm = prm_for(n, D=0.4)
    sensor = (TRUE_POSE[0] + 0.1, TRUE_POSE[1] - 0.1, TRUE_POSE[2] + 0.03)
    idx, _ = pairs_case(ctx, prm, ref, sensor_to_robot(REF_POSE, REL_REF), cur, sensor)
    assert (idx >= 0).sum() >= 3 and (idx == -1).sum() >= 1


# ------------------------------------------------------------------ the loop, step by step
CASES = [(n, 3) for n in (3, 63, 64, 65, 1023, 1024, 1025)] + [(65, 1), (65, 50), (1025, 1), (1025, 50), (1081, 50)]


@pytest.mark.parametrize("n,cap", CASES)
def test_every_step_and_the_whole_loop(ctx, world, n, cap):
    ref, cur = scene_pair(world, n)
    prm = prm_for(n, cap)
    ref_robot = sensor_to_robot(REF_POSE, REL_REF)
    init = sensor_to_robot((TRUE_POSE[0] + 0.2, TRUE_POSE[1] - 0.15, TRUE_POSE[2] + 0.05), REL_CUR)
    out, traj = ctx.icp(dev_scan(ctx, ref), ref_robot, dev_scan(ctx, cur), init, abi.IcpParams(*prm), trajectory=True)
    table = orc.ref_table(prm, ref, orc.compound(ref_robot, ref.rel))
    # pass 0 at the initial sensor pose, then: the device's pose k + 1 is the
    # restatement's step from the device's pose k, and the cost and pairs the
    # device reports at a pose are the restatement's there
    pose = orc.compound(init, cur.rel)
    assert all(same(a, b) for a, b in zip(pose_t(out.sensor_pose), pose))
    s, pairs = orc.pass_sums(orc.pass_beams(prm, table, cur, pose))
    assert same(out.initial_cost, s[0]) and out.initial_pairs == pairs
    for k, (x, y, th, cost, np_) in enumerate(traj):
        nxt = orc.solve_step(prm, s, pose)
        assert all(same(a, b) for a, b in zip((x, y, th), nxt)), f"step {k}"
        pose = (x, y, th)
        s, pairs = orc.pass_sums(orc.pass_beams(prm, table, cur, pose))
        assert same(cost, s[0]) and int(np_) == pairs, f"pass {k + 1}"
    # the whole loop, the stopping rule and the summary
    want = orc.refine(prm, ref, ref_robot, cur, init, table)
    assert len(traj) == out.iterations == want.iterations
    assert np.array(traj).tobytes() == np.array(want.trajectory).tobytes()
    assert_summary(out, want, init)
    if n >= 63:
        assert out.pose_found == 1 and out.iterations == max(1, cap)


def test_iteration_cap_below_one_runs_one_step(ctx, world):
    ref, cur = scene_pair(world, 65)
    prm = prm_for(65, 0)
    out = ctx.icp(dev_scan(ctx, ref), REF_POSE, dev_scan(ctx, cur), TRUE_POSE, abi.IcpParams(*prm))
    assert out.iterations == 1
    assert_summary(out, orc.refine(prm, ref, REF_POSE, cur, TRUE_POSE), TRUE_POSE)


def test_convergence_threshold_stops_early(ctx, world):
    n = 361
    ref, cur = scene_pair(world, n)
    prm = prm_for(n, 50, conv=1e-3)
    init = (TRUE_POSE[0] + 0.1, TRUE_POSE[1] - 0.1, TRUE_POSE[2] + 0.02)
    out, traj = ctx.icp(dev_scan(ctx, ref), REF_POSE, dev_scan(ctx, cur), init, abi.IcpParams(*prm), trajectory=True)
    want = orc.refine(prm, ref, REF_POSE, cur, init)
    assert 1 < out.iterations < 50
    assert abs(traj[-2][3] - traj[-1][3]) < 1e-3 and all(
        abs(traj[k - 1][3] - traj[k][3]) >= 1e-3 for k in range(1, len(traj) - 1))
    assert np.array(traj).tobytes() == np.array(want.trajectory).tobytes()
    assert_summary(out, want, init)


@pytest.mark.parametrize("n", [65, 1025, 2100])
def test_sums_of_one_pass_against_fsum(ctx, world, n):
    """the eleven sums of the pass after one step, within k 2^-53 sum |term| of the exact sums"""
    ref, cur = scene_pair(world, n)
    prm = prm_for(n, 1)
    init = (TRUE_POSE[0] + 0.05, TRUE_POSE[1] - 0.05, TRUE_POSE[2] + 0.01)
    out = ctx.icp(dev_scan(ctx, ref), REF_POSE, dev_scan(ctx, cur), init, abi.IcpParams(*prm))
    assert out.iterations == 1 and out.num_pairs > n // 2
    table = orc.ref_table(prm, ref, orc.compound(REF_POSE, ref.rel))
    b = orc.pass_beams(prm, table, cur, pose_t(out.best_sensor_pose))
    exact, absum = orc.pass_fsums(b)
    H = list(out.hessian)
    dev = [out.cost, out.pair_cost, H[0], H[1], H[2], H[4], H[5], H[8], out.rhs[0], out.rhs[1], out.rhs[2]]
    k = orc.tree_depth(n)
    assert k == (n + 1023) // 1024 - 1 + 6 + 15
    for q in range(11):
        err, bound = abs(dev[q] - exact[q]), k * 2.0 ** -53 * absum[q]
        print(f"sum {q}: |device - fsum| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, q
    assert (H[3], H[6], H[7]) == (H[1], H[2], H[5]), "H is mirrored"


# ------------------------------------------------------------------ fewer than three pairs
def test_fewer_than_three_pairs_at_pass_zero(ctx, world):
    ref, cur = scene_pair(world, 361)
    prm = prm_for(361, 50, D=1e-4)
    init = (TRUE_POSE[0] + 0.3, TRUE_POSE[1] - 0.3, TRUE_POSE[2] + 0.05)
    out, traj = ctx.icp(dev_scan(ctx, ref), REF_POSE, dev_scan(ctx, cur), init, abi.IcpParams(*prm), trajectory=True)
    assert out.pose_found == 0 and out.iterations == 0 and traj == [] and out.initial_pairs < 3
    assert list(out.covariance) == [0.0] * 9
    assert all(same(a, b) for a, b in zip(pose_t(out.best_sensor_pose), pose_t(out.sensor_pose)))
    assert_summary(out, orc.refine(prm, ref, REF_POSE, cur, init), init)


@pytest.mark.parametrize("seed,steps", [(6, 1), (38, 1)])
def test_fewer_than_three_pairs_after_a_step(ctx, world, seed, steps):
    """64-beam starts (found with the restatement) that pair at least three beams at first and lose them"""
    ref, _ = scene_pair(world, 64, rel=False)
    rng = np.random.default_rng(seed)
    true = (REF_POSE[0] + rng.uniform(-0.3, 0.3), REF_POSE[1] + rng.uniform(-0.3, 0.3), REF_POSE[2] + rng.uniform(-0.1, 0.1))
    cur = orc.ScanIn(scene.ray_cast(world, true, ref.angles), ref.angles)
    init = (true[0] + rng.uniform(-0.2, 0.2), true[1] + rng.uniform(-0.2, 0.2), true[2] + rng.uniform(-0.05, 0.05))
    prm = orc.Params(10, 0.0, 0.01, 20.0, 0.0, 0.0, 0.08, 3.0)
    out, traj = ctx.icp(dev_scan(ctx, ref), REF_POSE, dev_scan(ctx, cur), init, abi.IcpParams(*prm), trajectory=True)
    want = orc.refine(prm, ref, REF_POSE, cur, init)
    assert want.initial_pairs >= 3 and want.pose_found == 0 and want.iterations == steps
    assert out.pose_found == 0 and out.iterations == steps and out.num_pairs < 3 and len(traj) == steps
    assert list(out.covariance) == [0.0] * 9
    assert np.array(traj).tobytes() == np.array(want.trajectory).tobytes()
    assert_summary(out, want, init)


def test_all_reference_beams_unusable(ctx, world):
    ref, cur = scene_pair(world, 65)
    ref = ref._replace(max_range=0.005)
    prm = prm_for(65)
    out = ctx.icp(dev_scan(ctx, ref), REF_POSE, dev_scan(ctx, cur), TRUE_POSE, abi.IcpParams(*prm))
    assert out.pose_found == 0 and out.iterations == 0 and out.initial_pairs == 0 and out.num_pairs == 0
    usable = int(orc.usable_mask(cur.ranges, *orc.usable_range(prm, cur)).sum())
    assert usable > 3
    # every usable beam is rejected: D^2 each, added along the tree
    assert_summary(out, orc.refine(prm, ref, REF_POSE, cur, TRUE_POSE), TRUE_POSE)


# ------------------------------------------------------------------ batches, determinism
def batch_items(ctx, world):
    ref64, cur64 = scene_pair(world, 64)
    ref1081, cur1081 = scene_pair(world, 1081)
    R64, C64, R1081, C1081 = (dev_scan(ctx, s) for s in (ref64, cur64, ref1081, cur1081))
    rr = sensor_to_robot(REF_POSE, REL_REF)
    near = sensor_to_robot((TRUE_POSE[0] + 0.1, TRUE_POSE[1] - 0.1, TRUE_POSE[2] + 0.02), REL_CUR)
    far = (TRUE_POSE[0] + 60.0, TRUE_POSE[1] + 60.0, TRUE_POSE[2] + 1.0)   # outside the room: nothing within 1 m, not found
    #        ref    ref pose  scan   initial pose
    return [(R1081, rr, C1081, near), (R64, rr, C64, near), (R1081, rr, C64, far), (R64, rr, C1081, near),
            (R1081, rr, C1081, near)]


def test_batch_equals_lone_calls(ctx, world):
    """five items: sizes 64 and 1081 mixed, pointers repeated, found and not found"""
    items = batch_items(ctx, world)
    prm = abi.IcpParams(*orc.Params(5, 0.0, 0.01, 20.0, 1e-3, 1e-3, 1.0, 3.0))
    got = ctx.icp_batch([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [i[3] for i in items], prm)
    lone = [ctx.icp(r, rp, s, ip, prm) for r, rp, s, ip in items]
    assert [bytes(g) for g in got] == [bytes(l) for l in lone]
    assert sorted({l.pose_found for l in lone}) == [0, 1]
    assert bytes(got[0]) == bytes(got[4])
    assert ctx.icp_batch([], [], [], [], prm) == []


def test_two_runs_and_two_contexts_give_identical_bytes(ctx, world):
    items = batch_items(ctx, world)
    prm = abi.IcpParams(*orc.Params(5, 0.0, 0.01, 20.0, 1e-3, 1e-3, 1.0, 3.0))
    a = ctx.icp(*items[0], prm)
    b = ctx.icp(*items[0], prm)
    other = abi.Context(0)
    try:
        ref, cur = scene_pair(world, 1081)
        c = other.icp(dev_scan(other, ref), items[0][1], dev_scan(other, cur), items[0][3], prm)
    finally:
        other.close()
    assert bytes(a) == bytes(b) == bytes(c)
    assert a.pose_found == 1 and a.iterations == 5


# ------------------------------------------------------------------ arguments
def test_the_table_cap(ctx):
    """4096 usable reference beams run (the table fills 128 KiB of LDS); 4097 are refused.  Unusable beams do not count."""
    n = 4097
    ang = np.linspace(-2.0, 2.0, n + 3)
    rng = 4.0 + 0.5 * np.sin(7.0 * ang)
    ranges = rng.copy()
    ranges[[10, 2000, 4000]] = 25.0     # n + 3 beams, 3 unusable: n usable
    ref_big = orc.ScanIn(ranges, ang)
    ranges = ranges.copy()
    ranges[3000] = 25.0                 # 4096 usable
    ref_ok = orc.ScanIn(ranges, ang)
    cur = orc.ScanIn(rng[::50].copy(), ang[::50].copy())
    prm = orc.Params(2, 0.0, 0.01, 20.0, 1e-3, 1e-3, 0.5, 0.5)
    O, init = (0.0, 0.0, 0.0), (0.02, -0.01, 0.003)
    out = ctx.icp(dev_scan(ctx, ref_ok), O, dev_scan(ctx, cur), init, abi.IcpParams(*prm))
    assert out.pose_found == 1 and out.num_pairs >= 3
    assert_summary(out, orc.refine(prm, ref_ok, O, cur, init), init)
    pairs_case(ctx, prm, ref_ok, O, cur, init)
    with pytest.raises(abi.LgsError) as e:
        ctx.icp(dev_scan(ctx, ref_big), O, dev_scan(ctx, cur), init, abi.IcpParams(*prm))
    assert e.value.status == LGS_ERR_INVALID_ARG
    with pytest.raises(abi.LgsError) as e:
        ctx.icp_pairs(dev_scan(ctx, ref_big), O, dev_scan(ctx, cur), init, abi.IcpParams(*prm))
    assert e.value.status == LGS_ERR_INVALID_ARG


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


def raw_calls(ctx, R, S, ref_pose, init, prm, null=None):
    """every entry point with these arguments, on poisoned outputs; returns [(status, untouched)]"""
    lib, P = ctx.lib, abi.Pose2D
    p = abi.IcpParams(*prm)
    res = []
    out = abi.IcpSummary()
    C.memset(C.byref(out), 0xAB, C.sizeof(out))
    before = bytes(out)
    traj = np.full(5 * 8, 7.0)
    a = dict(ctx=ctx.h, ref=R.h, scan=S.h, prm=C.byref(p), out=C.byref(out))
    if null:
        a[null] = None
    st = lib.lgs_icp_optimize_pose(a["ctx"], a["ref"], P(*ref_pose), a["scan"], P(*init), a["prm"], a["out"], abi.dptr(traj))
    res.append((st, bytes(out) == before and (traj == 7.0).all()))
    outs = (abi.IcpSummary * 2)()
    C.memset(outs, 0xAB, C.sizeof(outs))
    before = bytes(outs)
    rarr, sarr = (C.c_void_p * 2)(R.h, a["ref"]), (C.c_void_p * 2)(S.h, a["scan"])
    rp, ip = (P * 2)(P(*REF_POSE), P(*ref_pose)), (P * 2)(P(*TRUE_POSE), P(*init))
    st = lib.lgs_icp_optimize_pose_batch(a["ctx"], rarr, rp, sarr, ip, 2, a["prm"], outs if a["out"] else None)
    res.append((st, bytes(outs) == before))
    idx, e = np.full(len(S.ranges), 77, dtype=np.int32), np.full(len(S.ranges), 7.0)
    st = lib.lgs_icp_pairs(a["ctx"], a["ref"], P(*ref_pose), a["scan"], P(*init), a["prm"],
                           idx.ctypes.data_as(C.POINTER(C.c_int)) if a["out"] else None, abi.dptr(e))
    res.append((st, (idx == 77).all() and (e == 7.0).all()))
    return res


@pytest.fixture(scope="module")
def small_scans(ctx, world):
    ref, cur = scene_pair(world, 65)
    return dev_scan(ctx, ref), dev_scan(ctx, cur)


def test_valid_arguments_pass_the_raw_calls(ctx, small_scans):
    assert [st for st, _ in raw_calls(ctx, *small_scans, REF_POSE, TRUE_POSE, GOOD)] == [0, 0, 0]


@pytest.mark.parametrize("case", list(BAD_PARAMS))
def test_invalid_parameters(ctx, small_scans, case):
    assert raw_calls(ctx, *small_scans, REF_POSE, TRUE_POSE, BAD_PARAMS[case]) == [(LGS_ERR_INVALID_ARG, True)] * 3


@pytest.mark.parametrize("case", list(BAD_POSES))
def test_poses_that_are_not_finite(ctx, small_scans, case):
    bad = BAD_POSES[case]
    assert raw_calls(ctx, *small_scans, bad, TRUE_POSE, GOOD) == [(LGS_ERR_INVALID_ARG, True)] * 3
    assert raw_calls(ctx, *small_scans, REF_POSE, bad, GOOD) == [(LGS_ERR_INVALID_ARG, True)] * 3


@pytest.mark.parametrize("null", ["ctx", "ref", "scan", "prm", "out"])
def test_null_arguments(ctx, small_scans, null):
    assert raw_calls(ctx, *small_scans, REF_POSE, TRUE_POSE, GOOD, null=null) == [(LGS_ERR_INVALID_ARG, True)] * 3


def test_negative_count_and_null_arrays(ctx, small_scans):
    lib, P = ctx.lib, abi.Pose2D
    R, S = small_scans
    p = abi.IcpParams(*GOOD)
    out = abi.IcpSummary()
    C.memset(C.byref(out), 0xAB, C.sizeof(out))
    before = bytes(out)
    rarr, sarr, rp, ip = (C.c_void_p * 1)(R.h), (C.c_void_p * 1)(S.h), (P * 1)(P(*REF_POSE)), (P * 1)(P(*TRUE_POSE))
    assert lib.lgs_icp_optimize_pose_batch(ctx.h, rarr, rp, sarr, ip, -1, C.byref(p), C.byref(out)) == LGS_ERR_INVALID_ARG
    assert lib.lgs_icp_optimize_pose_batch(ctx.h, None, rp, sarr, ip, 1, C.byref(p), C.byref(out)) == LGS_ERR_INVALID_ARG
    assert lib.lgs_icp_optimize_pose_batch(ctx.h, rarr, None, sarr, ip, 1, C.byref(p), C.byref(out)) == LGS_ERR_INVALID_ARG
    assert lib.lgs_icp_optimize_pose_batch(ctx.h, rarr, rp, None, ip, 1, C.byref(p), C.byref(out)) == LGS_ERR_INVALID_ARG
    assert lib.lgs_icp_optimize_pose_batch(ctx.h, rarr, rp, sarr, None, 1, C.byref(p), C.byref(out)) == LGS_ERR_INVALID_ARG
    assert lib.lgs_icp_optimize_pose_batch(ctx.h, rarr, rp, sarr, ip, 0, C.byref(p), C.byref(out)) == 0
    assert bytes(out) == before
    assert lib.lgs_icp_optimize_pose(ctx.h, R.h, P(*REF_POSE), S.h, P(*TRUE_POSE), C.byref(p), C.byref(out), None) == 0
    assert bytes(out) != before and out.pose_found == 1


def test_empty_scan_cannot_reach_the_matcher(ctx):
    """an empty scan is LGS_ERR_INVALID_ARG: lgs_scan_create refuses to make one"""
    with pytest.raises(abi.LgsError):
        ctx.scan(np.zeros(0), np.zeros(0))


def test_angle_outside_the_sincos_domain(ctx, small_scans):
    """|theta + angle| >= 105414350: LGS_ERR_INTERNAL, the outputs as they were"""
    far = (0.0, 0.0, 2.0e8)
    assert raw_calls(ctx, *small_scans, far, TRUE_POSE, GOOD) == [(LGS_ERR_INTERNAL, True)] * 3
    assert raw_calls(ctx, *small_scans, REF_POSE, far, GOOD) == [(LGS_ERR_INTERNAL, True)] * 3


# ------------------------------------------------------------------ it converges
STARTS = [(0.36 / math.sqrt(2), -0.36 / math.sqrt(2), 0.08), (-0.2, 0.15, -0.05), (0.1, 0.25, 0.06)]


@pytest.mark.parametrize("k", range(3))
def test_final_pose_is_closer_than_the_initial_one(ctx, world, k):
    """three 1081-beam starts of the scene: strictly closer to the true pose in distance and in angle"""
    ref, cur = scene_pair(world, 1081, rel=False)
    dx, dy, dth = STARTS[k]
    init = (TRUE_POSE[0] + dx, TRUE_POSE[1] + dy, TRUE_POSE[2] + dth)
    out = ctx.icp(dev_scan(ctx, ref), REF_POSE, dev_scan(ctx, cur), init, abi.IcpParams(*prm_for(1081, 50)))
    e = out.estimated_pose
    d0, a0 = math.hypot(dx, dy), abs(dth)
    d1, a1 = math.hypot(e.x - TRUE_POSE[0], e.y - TRUE_POSE[1]), abs(e.theta - TRUE_POSE[2])
    print(f"start {k}: {d0:.4f} m / {a0:.4f} rad -> {d1:.3e} m / {a1:.3e} rad, {out.num_pairs} pairs")
    assert out.pose_found == 1 and out.iterations == 50
    assert d1 < d0 and a1 < a0
