"""Loop records refined by ICP against their local maps' references
(lgs_loop_refine_icp, csrc/k_icp_ref.hip) on the GPU.
Tolerance: none.  The expected records are composed from
lgs_icp_ref_optimize_pose_batch's summaries (which must equal the test-side
restatement, tests/icp_ref_oracle.py), a Python restatement of the gate and the
oracle's InverseCompound; all 176 bytes of every record and the refined flags
must be equal.  Records from the correlative detector must end strictly closer
to the scene's true pose, in distance and in angle.
"""
import ctypes as C
import math

import numpy as np
import pytest

import icp_oracle as orc
import icp_ref_oracle as rorc
import oracle_bind as ob
from lgs_amd import abi, loopbatch, scene

pytestmark = pytest.mark.gpu

LGS_ERR_INVALID_ARG = 1
INF, NAN = float("inf"), float("nan")
REL_REF, REL_CUR = (0.1, -0.05, 0.02), (-0.03, 0.08, -0.015)
PRM = orc.Params(8, 0.0, 0.01, 20.0, 1e-3, 1e-3, 1.0, 3.0)
RANGES = [(0, 2), (3, 6)]               # two local maps of three and four scans
QUERY_OF = [0, 0, 1, 1, 1]              # five candidates
# the candidates' true robot poses and how far off their records start
TRUE = [(0.3, 0.1, 0.12), (-0.2, 0.25, -0.05), (0.55, -0.15, 0.2), (0.1, 0.4, 0.3), (0.7, 0.2, 0.1)]
OFF = [(0.05, 0.0, 0.02), (-0.12, 0.1, -0.04), (0.2, -0.2, 0.06), (0.1, 0.1, 0.03), (5.0, 0.5, 0.05)]
NOT_FOUND, FAR = 3, 4                   # candidate 3's record has found = 0, candidate 4 starts 5 m off
# the gate of the composition test: every comparison of the restated gate lies more than 1e-6 relative from
# its threshold (asserted below; by the restatement on the scene above the three near candidates pair 57 .. 61
# beams at costs of 0.07 .. 0.14 and move 0.02 .. 0.33 m and 0.016 .. 0.06 rad; the far one pairs 17 at 0.78)
GATE = (20, 0.5, 0.6, 0.2)


def dev_scan(ctx, s: orc.ScanIn):
    return ctx.scan(np.ascontiguousarray(s.ranges, dtype=np.float64), np.ascontiguousarray(s.angles, dtype=np.float64),
                    s.rel, s.min_range, s.max_range)


def normalize_angle(t):
    """NormalizeAngle (H/util.hpp:125-135)"""
    t = math.fmod(t, 2.0 * math.pi)
    if t > math.pi:
        t -= 2.0 * math.pi
    elif t < -math.pi:
        t += 2.0 * math.pi
    return t


def gate_terms(s, rec_pose):
    """what the gate compares, in its arithmetic"""
    dx, dy = s.estimated_pose.x - rec_pose[0], s.estimated_pose.y - rec_pose[1]
    return s.num_pairs, s.normalized_cost, dx * dx + dy * dy, abs(normalize_angle(s.estimated_pose.theta - rec_pose[2]))


def gate_accepts(gate, s, rec_pose):
    pairs, cost, d2, rot = gate_terms(s, rec_pose)
    return bool(s.pose_found != 0 and pairs >= gate[0] and cost <= gate[1] and d2 <= gate[2] * gate[2] and rot <= gate[3])


def clear_of_thresholds(gate, s, rec_pose, rel=1e-6):
    pairs, cost, d2, rot = gate_terms(s, rec_pose)
    far = lambda v, t: math.isinf(t) or abs(v - t) > rel * max(abs(v), abs(t))
    return far(cost, gate[1]) and far(d2, gate[2] * gate[2]) and far(rot, gate[3])


_PROBLEM = {}


def problem(world):
    """reference scans, their poses, the candidates' scans and hand-made records (ctypes LoopResult)"""
    if not _PROBLEM:
        ang = scene.beam_angles(65)
        poses = [(0.1 * k - 0.4, 0.05 * k - 0.2, 0.02 * k) for k in range(7)]
        refs = [orc.ScanIn(scene.ray_cast(world, orc.compound(p, REL_REF), ang), ang, REL_REF) for p in poses]
        cands = [orc.ScanIn(scene.ray_cast(world, orc.compound(t, REL_CUR), ang), ang, REL_CUR) for t in TRUE]
        _PROBLEM.update(refs=refs, poses=poses, cands=cands)
    return _PROBLEM["refs"], _PROBLEM["poses"], _PROBLEM["cands"]


def node_pose(poses, q):
    return poses[RANGES[q][0]]


def hand_records(poses, estimates=None):
    recs = (abi.LoopResult * 5)()
    for c in range(5):
        q = QUERY_OF[c]
        est = estimates[c] if estimates else tuple(t + o for t, o in zip(TRUE[c], OFF[c]))
        r = recs[c]
        r.found = 0 if c == NOT_FOUND else 1
        r.start_node_index, r.end_node_index, r.pad = RANGES[q][0], 100 + c, 0
        r.start_node_pose = abi.Pose2D(*node_pose(poses, q))
        r.estimated_pose = abi.Pose2D(*est)
        if r.found and all(math.isfinite(v) for v in est):
            rel = ob.lib().orc_inverse_compound(ob.Pose(*node_pose(poses, q)), ob.Pose(*est))
            r.relative_pose = abi.Pose2D(rel.x, rel.y, rel.theta)
        for k in range(9):
            r.covariance[k] = 0.001 * (k + 1) + c
        r.score, r.normalized_cost = 0.7 + 0.01 * c, 0.3 + 0.01 * c
    return recs


def copy_records(recs):
    return (abi.LoopResult * len(recs)).from_buffer_copy(bytes(recs))


class Setup:
    def __init__(self, ctx, world):
        self.refs, self.poses, self.cands = problem(world)
        self.p = abi.IcpParams(*PRM)
        scans = [dev_scan(ctx, r) for r in self.refs]
        self.rset = ctx.icp_ref_set(scans, self.poses, [a for a, _ in RANGES], [b for _, b in RANGES], self.p)
        self.S = [dev_scan(ctx, c) for c in self.cands]
        self.queries = [(None, None, node_pose(self.poses, 0), RANGES[0][0], 0, 2),
                        (None, None, node_pose(self.poses, 1), RANGES[1][0], 2, 3)]
        self.cl = [(self.S[c], TRUE[c], 100 + c) for c in range(5)]
        self.qrefs = [self.rset[0], self.rset[1]]

    def refine(self, ctx, gate, recs):
        return ctx.loop_refine_icp(self.qrefs, self.queries, self.cl, self.p, abi.LoopRefineGate(*gate), recs)

    def expected(self, gate, recs):
        """the composition: the batch's summaries, the restated gate, the oracle's InverseCompound"""
        run = [c for c in range(5) if recs[c].found and all(math.isfinite(v) for v in pose_t(recs[c].estimated_pose))]
        sums = self.rset[0].refine_batch([self.S[c] for c in run], [pose_t(recs[c].estimated_pose) for c in run], self.p,
                                         refs=[self.rset[QUERY_OF[c]] for c in run])
        want, flags = copy_records(recs), [0] * 5
        for c, s in zip(run, sums):
            if not gate_accepts(gate, s, pose_t(recs[c].estimated_pose)):
                continue
            r, node = want[c], node_pose(self.poses, QUERY_OF[c])
            rel = ob.lib().orc_inverse_compound(ob.Pose(*node), ob.Pose(*pose_t(s.estimated_pose)))
            r.estimated_pose = s.estimated_pose
            r.relative_pose = abi.Pose2D(rel.x, rel.y, rel.theta)
            for k in range(9):
                r.covariance[k] = s.covariance[k]
            r.normalized_cost = s.normalized_cost
            flags[c] = 1
        return want, flags, dict(zip(run, sums))


def pose_t(p):
    return (p.x, p.y, p.theta)


@pytest.fixture(scope="module")
def setup(ctx, world):
    return Setup(ctx, world)


def assert_summary(dev, ref: orc.Result):
    bits = lambda v: np.float64(v).tobytes()
    assert (dev.pose_found, dev.iterations, dev.num_pairs, dev.initial_pairs) == \
        (ref.pose_found, ref.iterations, ref.num_pairs, ref.initial_pairs)
    for name in ("cost", "pair_cost", "initial_cost", "normalized_cost"):
        assert bits(getattr(dev, name)) == bits(getattr(ref, name)), name
    assert bits(pose_t(dev.estimated_pose)) == bits(ref.estimated_pose)
    assert bits(list(dev.hessian)) == bits(ref.hessian) and bits(list(dev.covariance)) == bits(ref.covariance)


# ------------------------------------------------------------------ 5. records against the composition
def test_records_equal_the_composition(ctx, setup):
    recs = hand_records(setup.poses)
    before = copy_records(recs)
    want, flags, sums = setup.expected(GATE, recs)
    refined, got_sums = setup.refine(ctx, GATE, recs)
    assert refined == flags
    for c in range(5):
        assert bytes(recs[c]) == bytes(want[c]), c
    # the three near candidates are accepted, the others keep every byte
    assert flags == [1, 1, 1, 0, 0]
    for c in (NOT_FOUND, FAR):
        assert bytes(recs[c]) == bytes(before[c])
    for c in (0, 1, 2):
        assert bytes(recs[c]) != bytes(before[c])
        r, b = recs[c], before[c]
        assert (r.found, r.start_node_index, r.end_node_index, r.pad, r.score) == \
            (b.found, b.start_node_index, b.end_node_index, b.pad, b.score)
        assert bytes(r.start_node_pose) == bytes(b.start_node_pose)
    # the far one: fewer than min_pairs pairs, or no pose at all
    assert sums[FAR].pose_found == 0 or sums[FAR].num_pairs < GATE[0]
    # the summaries: the batch's, the restatement's; zero bytes where nothing ran
    assert NOT_FOUND not in sums and bytes(got_sums[NOT_FOUND]) == bytes(C.sizeof(abi.IcpSummary))
    for c, s in sums.items():
        assert bytes(got_sums[c]) == bytes(s)
        q = QUERY_OF[c]
        a, b = RANGES[q]
        assert_summary(s, rorc.refine(PRM, setup.refs[a:b + 1], setup.poses[a:b + 1], setup.cands[c],
                                      pose_t(before[c].estimated_pose)))
        assert clear_of_thresholds(GATE, s, pose_t(before[c].estimated_pose)), (c, gate_terms(s, pose_t(before[c].estimated_pose)))
    # accepted estimates moved towards the truth
    for c in (0, 1, 2):
        d0 = math.hypot(before[c].estimated_pose.x - TRUE[c][0], before[c].estimated_pose.y - TRUE[c][1])
        d1 = math.hypot(recs[c].estimated_pose.x - TRUE[c][0], recs[c].estimated_pose.y - TRUE[c][1])
        assert d1 < d0


@pytest.mark.parametrize("term", ["min_pairs", "max_normalized_cost", "max_translation", "max_rotation"])
def test_every_gate_term_rejects_on_its_own(ctx, setup, term):
    """candidate 1 passes every term of an open gate; with one term set 1 % below what candidate 1 shows (pairs:
    one more than it has) it is rejected and keeps its bytes, while candidate 0, which pairs more beams at a
    lower cost and moves less, still passes"""
    recs = hand_records(setup.poses)
    before = copy_records(recs)
    _, _, sums = setup.expected(GATE, recs)
    pairs, cost, d2, rot = gate_terms(sums[1], pose_t(before[1].estimated_pose))
    assert cost > 0.0 and d2 > 0.0 and rot > 0.0
    gate = {"min_pairs": (pairs + 1, INF, INF, INF), "max_normalized_cost": (3, 0.99 * cost, INF, INF),
            "max_translation": (3, INF, 0.99 * math.sqrt(d2), INF), "max_rotation": (3, INF, INF, 0.99 * rot)}[term]
    open_gate = (3, INF, INF, INF)
    assert gate_accepts(open_gate, sums[1], pose_t(before[1].estimated_pose))
    assert not gate_accepts(gate, sums[1], pose_t(before[1].estimated_pose))
    want, flags, _ = setup.expected(gate, recs)
    refined, _ = setup.refine(ctx, gate, recs)
    assert refined == flags and refined[1] == 0 and bytes(recs[1]) == bytes(before[1])
    assert [bytes(r) for r in recs] == [bytes(w) for w in want]
    assert refined[0] == 1, "the term rejects candidate 1, not everything"


# ------------------------------------------------------------------ 6. +inf gates, NaN, nothing found
def test_infinite_gates_accept_every_pose_found(ctx, setup):
    recs = hand_records(setup.poses)
    gate = (3, INF, INF, INF)
    want, flags, sums = setup.expected(gate, recs)
    refined, _ = setup.refine(ctx, gate, recs)
    assert refined == flags == [int(c in sums and sums[c].pose_found != 0) for c in range(5)]
    assert refined[:3] == [1, 1, 1] and refined[NOT_FOUND] == 0
    assert [bytes(r) for r in recs] == [bytes(w) for w in want]


@pytest.mark.parametrize("field", range(3))
def test_a_nan_estimate_rejects(ctx, setup, field):
    est = [tuple(t + o for t, o in zip(TRUE[c], OFF[c])) for c in range(5)]
    bad = list(est[1])
    bad[field] = NAN
    est[1] = tuple(bad)
    recs = hand_records(setup.poses, est)
    before = copy_records(recs)
    gate = (3, INF, INF, INF)
    want, flags, sums = setup.expected(gate, recs)
    launches = ctx.icp_ref_set_stats().refine_launches
    refined, got_sums = setup.refine(ctx, gate, recs)
    assert ctx.icp_ref_set_stats().refine_launches == launches + 1
    assert refined == flags and refined[1] == 0 and refined[0] == refined[2] == 1
    assert bytes(recs[1]) == bytes(before[1]) and bytes(got_sums[1]) == bytes(C.sizeof(abi.IcpSummary))
    assert [bytes(r) for r in recs] == [bytes(w) for w in want]


def test_records_that_were_not_found_are_never_launched(ctx, setup):
    recs = hand_records(setup.poses)
    for r in recs:
        r.found = 0
    before = copy_records(recs)
    stats = ctx.icp_ref_set_stats()
    refined, sums = setup.refine(ctx, (3, INF, INF, INF), recs)
    assert ctx.icp_ref_set_stats() == stats, "no launch at all"
    assert refined == [0] * 5 and bytes(recs) == bytes(before)
    assert all(bytes(s) == bytes(C.sizeof(abi.IcpSummary)) for s in sums)
    # no candidates at all
    assert ctx.loop_refine_icp([setup.rset[0]], [(None, None, (0.0, 0.0, 0.0), 0, 0, 0)], [], setup.p,
                               abi.LoopRefineGate(3, INF, INF, INF), (abi.LoopResult * 1)()) == ([], [])
    assert ctx.icp_ref_set_stats() == stats


# ------------------------------------------------------------------ argument checks
def raw_refine(ctx, setup, gate=(3, INF, INF, INF), prm=PRM, queries=None, null=None, refs=None, n_cand=5, recs=None):
    """lgs_loop_refine_icp on poisoned outputs; (status, everything untouched)"""
    queries = setup.queries if queries is None else queries
    qs = (abi.LoopQuery * max(1, len(queries)))()
    for i, (_, _, pose, idx, first, cnt) in enumerate(queries):
        qs[i] = abi.LoopQuery(None, None, abi.Pose2D(*pose), idx, first, cnt)
    cs = (abi.LoopCandidate * 5)(*[abi.LoopCandidate(s.h, abi.Pose2D(*pose), idx, 0) for s, pose, idx in setup.cl])
    refs = setup.qrefs if refs is None else refs
    rarr = (C.c_void_p * max(1, len(refs)))(*[r.h if r is not None else None for r in refs])
    recs = hand_records(setup.poses) if recs is None else recs
    before = bytes(recs)
    refined = (C.c_int * 5)(*[77] * 5)
    sums = (abi.IcpSummary * 5)()
    C.memset(sums, 0xAB, C.sizeof(sums))
    sums_before = bytes(sums)
    p, g = abi.IcpParams(*prm), abi.LoopRefineGate(*gate)
    a = dict(ctx=ctx.h, refs=rarr, queries=qs, cands=cs, prm=C.byref(p), gate=C.byref(g), results=recs, refined=refined,
             sums=sums)
    if null:
        a[null] = None
    st = ctx.lib.lgs_loop_refine_icp(a["ctx"], a["refs"], a["queries"], len(queries), a["cands"], n_cand, a["prm"],
                                     a["gate"], a["results"], a["refined"], a["sums"])
    return st, bytes(recs) == before and list(refined) == [77] * 5 and bytes(sums) == sums_before


def test_invalid_arguments_leave_the_results_untouched(ctx, setup, world):
    BAD = (LGS_ERR_INVALID_ARG, True)
    assert raw_refine(ctx, setup) == (0, False)
    st, _ = raw_refine(ctx, setup, null="sums")
    assert st == 0
    for null in ("ctx", "refs", "queries", "cands", "prm", "gate", "results", "refined"):
        assert raw_refine(ctx, setup, null=null) == BAD, null
    assert raw_refine(ctx, setup, refs=[setup.rset[0], None]) == BAD
    # the query / candidate range rules of the detectors
    q0, q1 = setup.queries
    for queries in ([q0], [q0, q1[:4] + (3, 2)], [q0, q1[:4] + (2, 4)], [q0, q1[:4] + (2, -1)], [q1, q0]):
        assert raw_refine(ctx, setup, queries=queries, refs=[setup.rset[0]] * len(queries)) == BAD, queries
    assert raw_refine(ctx, setup, n_cand=-1) == BAD
    # the gate
    for gate in ((2, 1.0, 1.0, 1.0), (0, INF, INF, INF), (3, NAN, 1.0, 1.0), (3, 1.0, NAN, 1.0), (3, 1.0, 1.0, NAN),
                 (3, -1e-300, 1.0, 1.0), (3, 1.0, -1.0, 1.0), (3, 1.0, 1.0, -INF)):
        assert raw_refine(ctx, setup, gate=gate) == BAD, gate
    assert raw_refine(ctx, setup, gate=(3, 0.0, 0.0, 0.0))[0] == 0
    # the refine-time rules of lgs_icp_ref_*: parameters, the reference's context, its bound parameters
    assert raw_refine(ctx, setup, prm=PRM._replace(max_correspondence_dist=0.0)) == BAD
    assert raw_refine(ctx, setup, prm=PRM._replace(convergence_threshold=NAN)) == BAD
    assert raw_refine(ctx, setup, prm=PRM._replace(max_segment_length=math.nextafter(PRM.max_segment_length, 9.0))) == BAD
    assert raw_refine(ctx, setup, prm=PRM._replace(num_iterations_max=2, rotation_regularizer=0.5))[0] == 0
    other = abi.Context(0)
    try:
        theirs = other.icp_ref([dev_scan(other, setup.refs[0])], [setup.poses[0]], setup.p)
        assert raw_refine(ctx, setup, refs=[setup.rset[0], theirs]) == BAD
        # ... unless no item runs against it
        recs = hand_records(setup.poses)
        for c in (2, 3, 4):
            recs[c].found = 0
        assert raw_refine(ctx, setup, refs=[setup.rset[0], theirs], recs=recs)[0] == 0
        theirs.close()
    finally:
        other.close()


# ------------------------------------------------------------------ 7. from the detector
LOOP_PARAMS = (5, 1.0, 1.0, 0.5, 20.0)               # tests/test_gpu_loop.py's small batch
LOOP_COST = (0.01, 20.0, 0.075, 0.1, 1, 0.05, 1.0)
LOOP_THR = 0.6
LOOP_ICP = orc.Params(20, 0.0, 0.01, 20.0, 1e-3, 1e-3, 0.5, 0.5)
LOOP_GATE = (30, INF, 0.5, 0.2)


def detector_problem(world, n_maps=3, nodes_per_map=4, n_beams=121, arc_scans=6, map_beams=1081, seed=9):
    """scene.loop_problem's batch at tests/test_gpu_loop.py's small sizes, made here so that the candidates'
    true poses and the maps' scans are known: (maps, candidates, truths, per map its scans and poses)"""
    rng = np.random.default_rng(seed)
    ang, mang = scene.beam_angles(n_beams), scene.beam_angles(map_beams)
    maps, cands, truths, map_scans = [], [], [], []
    node = 0
    for q in range(n_maps):
        c = (rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5))
        poses = scene.arc_poses(arc_scans, center=c)
        m = ob.OMap(0.05, 100, 500, 500)
        scans = []
        for p in poses:
            r = scene.ray_cast(world, p, mang)
            scans.append(r)
            m.integrate(p, ob.OScan(r, mang), ob.BuilderParams(0.01, 20.0, 0.6, 0.45))
        maps.append(loopbatch.LocalMap(m.cells(), m.m.min_x, m.m.min_y, 0.05, tuple(poses[0]), node))
        map_scans.append((scans, [tuple(p) for p in poses], mang))
        node += arc_scans
        for _ in range(nodes_per_map):
            true = (c[0] + rng.uniform(-1.0, 1.0), c[1] + rng.uniform(-1.0, 1.0), rng.uniform(-np.pi, np.pi))
            init = (true[0] + rng.uniform(-0.3, 0.3), true[1] + rng.uniform(-0.3, 0.3), true[2] + rng.uniform(-0.15, 0.15))
            cands.append(loopbatch.Candidate(q, scene.ray_cast(world, true, ang), ang, init, node))
            truths.append(true)
            node += 1
    return maps, cands, truths, map_scans


def test_records_of_the_correlative_detector_end_closer_to_the_truth(ctx, world):
    maps, cands, truths, map_scans = detector_problem(world)
    p, c = abi.RtcsmParams(*LOOP_PARAMS), abi.CostGEParams(*LOOP_COST)
    records = loopbatch.run_sharded(cands, loopbatch.hip_detect_fn(ctx, maps, cands, p, c, LOOP_THR))
    # one reference per local map from the maps' own scans, all in one pass
    scans, poses, lo, hi = [], [], [], []
    for rs, ps, mang in map_scans:
        lo.append(len(scans))
        scans += [ctx.scan(r, mang) for r in rs]
        poses += ps
        hi.append(len(scans) - 1)
    prm = abi.IcpParams(*LOOP_ICP)
    rset = ctx.icp_ref_set(scans, poses, lo, hi, prm)
    new, refined, sums = loopbatch.refine_icp(ctx, rset, maps, cands, records, prm, abi.LoopRefineGate(*LOOP_GATE))
    old_r, new_r = loopbatch.decode(records), loopbatch.decode(new)
    found = [i for i, r in enumerate(old_r) if r.found]
    assert 0 < len(found) and refined.sum() >= 1 and all(old_r[i].found for i in np.flatnonzero(refined))
    for i, (a, b, t) in enumerate(zip(old_r, new_r, truths)):
        if not refined[i]:
            assert bytes(a) == bytes(b)
            continue
        d0, d1 = (math.hypot(r.estimated_pose.x - t[0], r.estimated_pose.y - t[1]) for r in (a, b))
        a0, a1 = (abs(normalize_angle(r.estimated_pose.theta - t[2])) for r in (a, b))
        print(f"candidate {i}: {d0:.4f} m / {a0:.4f} rad -> {d1:.3e} m / {a1:.3e} rad, {sums[i].num_pairs} pairs")
        assert d1 < d0 and a1 < a0, i
        rel = ob.lib().orc_inverse_compound(ob.Pose(*maps[cands[i].query].node_pose), ob.Pose(*pose_t(b.estimated_pose)))
        assert pose_t(b.relative_pose) == (rel.x, rel.y, rel.theta)
        assert (b.found, b.start_node_index, b.end_node_index, b.score) == (a.found, a.start_node_index, a.end_node_index, a.score)
    rset.close()
