"""The ICP loop detector's window search (lgs_icp_ref_window_scores,
lgs_loop_detect_icp; csrc/k_icp_window.hip) on the GPU.
Tolerance: none.  A score must equal, in all bytes, the initial_cost and
initial_pairs that lgs_icp_ref_optimize_pose_batch reports from the same
lattice pose, and the test-side restatement (tests/icp_window_oracle.py); a
detector's records, best indices and summaries must equal the composition
dense argmin -> refine_batch from that pose -> restated gate -> record, in all
176 bytes.  The problem is that of tests/test_gpu_loop_refine_icp.py: 65
beams, seven reference scans, ranges (0, 2) and (3, 6).
"""
import ctypes as C
import math

import numpy as np
import pytest

import icp_oracle as orc
import icp_ref_oracle as rorc
import icp_window_oracle as worc
import test_gpu_loop_refine_icp as lr
from lgs_amd import abi, loopbatch, scene

pytestmark = pytest.mark.gpu

LGS_ERR_INVALID_ARG, LGS_ERR_INTERNAL = 1, 5
INF, NAN = float("inf"), float("nan")
PRM, RANGES, QUERY_OF, TRUE, OFF = lr.PRM, lr.RANGES, lr.QUERY_OF, lr.TRUE, lr.OFF
BEAMS = [65, 33, 65, 97, 65]              # the candidates' scans differ in size
NODE = [tuple(t + o for t, o in zip(TRUE[c], OFF[c])) for c in range(5)]   # drifted node poses; the last is 5 m off
WIN = worc.Window(2, 2, 1, 0.05, 0.02)    # 5 x 5 x 3
# The gate of the composition tests.  By the restatement on this scene the refines from the windows' best
# poses pair 61, 29, 57, 85 and 17 beams at normalized costs 0.072, 0.125, 0.140, 0.133 and 0.780 and move
# 0.027, 0.041, 0.223, 0.109 and 0.225 m and 0.002 .. 0.039 rad: candidates 0, 1 and 3 pass, 2 moves too far,
# 4 (whose window cannot reach its truth) pairs too few at too high a cost.  Every comparison lies more than
# 1e-6 relative from its threshold (asserted below).
GATE = (20, 0.5, 0.15, 0.2)
ACCEPTED = [1, 1, 0, 1, 0]


def bits(v):
    return np.asarray(v, dtype=np.float64).tobytes()


def awin(w):
    return abi.IcpWindow(*w)


def cand_scan(world, true, n):
    ang = scene.beam_angles(n)
    return orc.ScanIn(scene.ray_cast(world, orc.compound(true, lr.REL_CUR), ang), ang, lr.REL_CUR)


class Setup:
    def __init__(self, ctx, world):
        self.refs, self.poses, _ = lr.problem(world)
        self.p = abi.IcpParams(*PRM)
        self.ref_scans = [lr.dev_scan(ctx, r) for r in self.refs]
        self.rset = ctx.icp_ref_set(self.ref_scans, self.poses, [a for a, _ in RANGES], [b for _, b in RANGES], self.p)
        self.cands = [cand_scan(world, TRUE[c], BEAMS[c]) for c in range(5)]
        self.S = [lr.dev_scan(ctx, c) for c in self.cands]
        self.queries = [(None, None, lr.node_pose(self.poses, 0), RANGES[0][0], 0, 2),
                        (None, None, lr.node_pose(self.poses, 1), RANGES[1][0], 2, 3)]
        self.cl = [(self.S[c], NODE[c], 100 + c) for c in range(5)]
        self.qrefs = [self.rset[0], self.rset[1]]
        self.tables = [rorc.concat_tables(PRM, self.refs[a:b + 1], self.poses[a:b + 1]) for a, b in RANGES]

    def detect(self, ctx, window, gate, cands=range(5)):
        """lgs_loop_detect_icp over the candidates `cands` (a sorted subset), their queries rebuilt"""
        cands = list(cands)
        queries, refs = [], []
        for q in (0, 1):
            mine = [c for c in cands if QUERY_OF[c] == q]
            if mine:
                queries.append((None, None, lr.node_pose(self.poses, q), RANGES[q][0], cands.index(mine[0]), len(mine)))
                refs.append(self.rset[q])
        out, best, sums = ctx.loop_detect_icp(refs, queries, [self.cl[c] for c in cands], self.p, awin(window),
                                              abi.LoopRefineGate(*gate))
        return [bytes(out[i]) for i in range(len(cands))], best, [bytes(s) for s in sums]

    def composition(self, ctx, window, gate, cands=range(5)):
        """dense argmin -> refine_batch from that pose -> restated gate -> record"""
        cands = list(cands)
        best, starts = [], []
        for c in cands:
            cost, _ = ctx.icp_window_scores(self.rset[QUERY_OF[c]], self.S[c], NODE[c], awin(window), self.p)
            best.append(worc.select(cost.ravel()))
            starts.append(worc.lattice_pose(window, NODE[c], best[-1]) if best[-1] >= 0 else None)
        run = [i for i, p in enumerate(best) if p >= 0]
        sums = self.rset[0].refine_batch([self.S[cands[i]] for i in run], [starts[i] for i in run], self.p,
                                         refs=[self.rset[QUERY_OF[cands[i]]] for i in run])
        by = dict(zip(run, sums))
        recs, out_sums, accepted = [], [], []
        for i, c in enumerate(cands):
            s = by.get(i)
            ok = s is not None and worc.gate_accepts(gate, s, starts[i])
            q = QUERY_OF[c]
            recs.append(worc.record(lr.node_pose(self.poses, q), RANGES[q][0], 100 + c, s, ok, BEAMS[c]))
            out_sums.append(bytes(s) if s is not None else bytes(C.sizeof(abi.IcpSummary)))
            accepted.append(int(ok))
        return recs, best, out_sums, accepted, by, starts


@pytest.fixture(scope="module")
def setup(ctx, world):
    return Setup(ctx, world)


def assert_scores_equal_refine_batch(ctx, ref, scan, centre, window, p, cost, pairs):
    P = worc.num_poses(window)
    sums = ref.refine_batch([scan] * P, [worc.lattice_pose(window, centre, k) for k in range(P)], p)
    assert bits(cost.ravel()) == bits([s.initial_cost for s in sums])
    assert pairs.ravel().tolist() == [s.initial_pairs for s in sums]
    return sums


# ------------------------------------------------------------------ 1. the dense scores
def test_dense_scores_equal_the_restatement_and_the_refines(ctx, setup):
    cost, pairs = ctx.icp_window_scores(setup.rset[0], setup.S[0], NODE[0], awin(WIN), setup.p)
    assert cost.shape == pairs.shape == (3, 5, 5)
    want_cost, want_pairs = worc.scores(PRM, setup.tables[0].table, setup.cands[0], NODE[0], WIN)
    assert bits(cost.ravel()) == bits(want_cost) and pairs.ravel().tolist() == want_pairs.tolist()
    sums = assert_scores_equal_refine_batch(ctx, setup.rset[0], setup.S[0], NODE[0], WIN, setup.p, cost, pairs)
    # the lattice pose the device scored is the one the restatement names, the centre the node pose itself
    for k, s in enumerate(sums):
        assert bits(lr.pose_t(s.initial_pose)) == bits(worc.lattice_pose(WIN, NODE[0], k))
    assert bits(lr.pose_t(sums[37].initial_pose)) == bits(NODE[0]) and worc.decode(WIN, 37) == (2, 2, 1)
    assert len(set(cost.ravel().tolist())) == 75 and pairs.min() >= 3


@pytest.mark.parametrize("n", [3, 64, 65, 1024, 1025, 1081, 4096])
def test_the_one_wave_tree_at_its_edges(ctx, setup, world, n):
    """beam counts at the lane, wave and round edges of the tree that one wave walks alone (64 lanes, sixteen
    rounds of 64, 1024 beams per trip), and the cap, where the hit points fill 64 KiB of LDS"""
    scan = lr.dev_scan(ctx, cand_scan(world, TRUE[0], n))
    w = worc.Window(1, 0, 0, 0.05, 0.02)
    cost, pairs = ctx.icp_window_scores(setup.rset[0], scan, NODE[0], awin(w), setup.p)
    assert_scores_equal_refine_batch(ctx, setup.rset[0], scan, NODE[0], w, setup.p, cost, pairs)
    assert np.isfinite(cost).all() and (pairs <= n).all()
    scan.close()


def test_1081_beams_against_ten_reference_scans(ctx, world):
    ang = scene.beam_angles(1081)
    poses = [(0.1 * k - 0.4, 0.05 * k - 0.2, 0.02 * k) for k in range(10)]
    refs = [orc.ScanIn(scene.ray_cast(world, orc.compound(p, lr.REL_REF), ang), ang, lr.REL_REF) for p in poses]
    p = abi.IcpParams(*PRM)
    dev = [lr.dev_scan(ctx, r) for r in refs]
    ref = ctx.icp_ref(dev, poses, p)
    cur = cand_scan(world, TRUE[0], 1081)
    scan = lr.dev_scan(ctx, cur)
    w = worc.Window(1, 1, 0, 0.05, 0.02)
    cost, pairs = ctx.icp_window_scores(ref, scan, NODE[0], awin(w), p)
    assert_scores_equal_refine_batch(ctx, ref, scan, NODE[0], w, p, cost, pairs)
    want_cost, want_pairs = worc.scores(PRM, rorc.concat_tables(PRM, refs, poses).table, cur, NODE[0], w)
    assert bits(cost.ravel()) == bits(want_cost) and pairs.ravel().tolist() == want_pairs.tolist()
    assert pairs.min() > 500
    ref.close()
    for s in dev + [scan]:
        s.close()


@pytest.mark.parametrize("shift", [(0.0, 0.0), (1e5, -1e5)])
def test_the_centre_pose_scores_as_the_node_pose(ctx, setup, shift):
    """... also where a pose's x and y are near 1e5 and the lattice step falls into the last 30 bits"""
    poses = [(x + shift[0], y + shift[1], t) for x, y, t in setup.poses[:3]]
    centre = (NODE[0][0] + shift[0], NODE[0][1] + shift[1], NODE[0][2])
    ref = ctx.icp_ref(setup.ref_scans[:3], poses, setup.p)
    w = worc.Window(1, 1, 1, 0.05, 0.02)
    cost, pairs = ctx.icp_window_scores(ref, setup.S[0], centre, awin(w), setup.p)
    lone = ref.refine(setup.S[0], centre, setup.p)
    assert bits(cost[1, 1, 1]) == bits(lone.initial_cost) and pairs[1, 1, 1] == lone.initial_pairs
    assert bits(lr.pose_t(lone.initial_pose)) == bits(centre) and lone.initial_pairs > 50
    assert_scores_equal_refine_batch(ctx, ref, setup.S[0], centre, w, setup.p, cost, pairs)
    ref.close()


# ------------------------------------------------------------------ 2. selection and ties
def test_an_empty_reference_selects_index_0_and_finds_nothing(ctx, setup):
    """A reference whose beams are all unusable: every usable beam of the scan is rejected at every pose, so
    all 75 costs are the same n_usable * D^2 and the tie goes to index 0; the refine from there pairs nothing,
    so found = 0 and the summary reports no pose, no step, no pair, a zero Hessian and a zero covariance."""
    dead = ctx.scan(np.zeros(65), scene.beam_angles(65), lr.REL_REF)
    ref = ctx.icp_ref([dead], [(0.0, 0.0, 0.0)], setup.p)
    assert ref.info().entries == 0
    cost, pairs = ctx.icp_window_scores(ref, setup.S[0], NODE[0], awin(WIN), setup.p)
    usable = int(np.count_nonzero(orc.usable_mask(setup.cands[0].ranges, *orc.usable_range(PRM, setup.cands[0]))))
    assert bits(cost.ravel()) == bits([usable * PRM.max_correspondence_dist ** 2] * 75) and not pairs.any()
    out, best, sums = ctx.loop_detect_icp([ref], [(None, None, (0.0, 0.0, 0.0), 0, 0, 1)], [setup.cl[0]], setup.p,
                                          awin(WIN), abi.LoopRefineGate(3, INF, INF, INF))
    assert best == [0] and out[0].found == 0
    s = sums[0]
    assert (s.pose_found, s.iterations, s.num_pairs, s.initial_pairs, s.pair_cost) == (0, 0, 0, 0, 0.0)
    assert bytes(s.covariance) == bytes(72) and bytes(s.hessian) == bytes(72) and bytes(s.rhs) == bytes(24)
    want = ref.refine(setup.S[0], worc.lattice_pose(WIN, NODE[0], 0), setup.p)
    assert bytes(s) == bytes(want)
    assert bytes(out[0]) == worc.record((0.0, 0.0, 0.0), 0, 100, want, False, 65)
    # a scan without a usable beam scores +0.0 everywhere: again index 0
    blind = ctx.scan(np.zeros(65), scene.beam_angles(65), lr.REL_CUR)
    cost, pairs = ctx.icp_window_scores(setup.rset[0], blind, NODE[0], awin(WIN), setup.p)
    assert bits(cost.ravel()) == bits([0.0] * 75) and not pairs.any()
    _, best, _ = ctx.loop_detect_icp([setup.rset[0]], [(None, None, (0.0, 0.0, 0.0), 0, 0, 1)], [(blind, NODE[0], 1)],
                                     setup.p, awin(WIN), abi.LoopRefineGate(3, INF, INF, INF))
    assert best == [0]
    for h in (ref, dead, blind):
        h.close()


TIE_TRUE = (0.5, 0.125, 0.125)   # x, y and theta are powers of two: the spacing of doubles halves just below them


@pytest.mark.parametrize("window,tied,want", [
    # theta steps far below the spacing of doubles at 0.125: the three lattice thetas are one double, so poses
    # 1, 4 and 7 (the centre's x) are one pose in three workgroups -- the host's combine must pick 1
    (worc.Window(1, 0, 1, 0.1, 2.0 ** -60), (1, 4, 7), 1),
    # the same along x and y: all nine poses are one pose, spread over the four waves of one workgroup
    (worc.Window(1, 1, 0, 2.0 ** -60, 0.01), tuple(range(9)), 0),
    # a theta step of 0.75 spacings below 0.125, 0.375 above: theta - step is the next double down, theta +
    # step is theta again, so exactly the poses of theta indices 1 and 2 are made one pose: 4 and 7 at the
    # centre's x.  (The restatement says whether index 1, the double below, scores the same bytes as well.)
    (worc.Window(1, 0, 1, 0.1, 0.75 * 2.0 ** -56), (4, 7), None),
])
def test_tied_poses_select_the_lower_index(ctx, setup, world, window, tied, want):
    cur = cand_scan(world, TIE_TRUE, 65)
    scan = lr.dev_scan(ctx, cur)
    poses = [worc.lattice_pose(window, TIE_TRUE, p) for p in tied]
    assert all(bits(p) == bits(poses[0]) for p in poses), "the construction: one pose under several indices"
    cost, pairs = ctx.icp_window_scores(setup.rset[1], scan, TIE_TRUE, awin(window), setup.p)
    cost = cost.ravel()
    assert all(bits(cost[p]) == bits(cost[tied[0]]) for p in tied)
    want_cost, _ = worc.scores(PRM, setup.tables[1].table, cur, TIE_TRUE, window)
    assert bits(cost) == bits(want_cost)
    sel = worc.select(cost)
    assert sel == (want if want is not None else sel)
    assert sel <= tied[0] and bits(cost[sel]) == bits(cost[tied[0]]), "the tied poses hold the minimum"
    _, best, _ = ctx.loop_detect_icp([setup.rset[1]], [(None, None, (0.0, 0.0, 0.0), 0, 0, 1)], [(scan, TIE_TRUE, 1)],
                                     setup.p, awin(window), abi.LoopRefineGate(3, INF, INF, INF))
    assert best == [sel]
    scan.close()


# ------------------------------------------------------------------ 3. the detector against the composition
def test_records_equal_the_composition(ctx, setup):
    recs, best, sums, accepted, by, starts = setup.composition(ctx, WIN, GATE)
    got_recs, got_best, got_sums = setup.detect(ctx, WIN, GATE)
    assert got_best == best and all(p >= 0 for p in best)
    assert got_sums == sums
    for c in range(5):
        assert got_recs[c] == recs[c], c
    assert accepted == ACCEPTED
    for c in range(5):
        r = abi.LoopResult.from_buffer_copy(got_recs[c])
        s = by[c]
        print(f"candidate {c}: best {best[c]} {worc.decode(WIN, best[c])}, gate terms {worc.gate_terms(s, starts[c])}")
        assert worc.clear_of_thresholds(GATE, s, starts[c]), (c, worc.gate_terms(s, starts[c]))
        assert s.num_pairs != GATE[0]
        assert (r.found, r.start_node_index, r.end_node_index, r.pad) == (ACCEPTED[c], RANGES[QUERY_OF[c]][0], 100 + c, 0)
        assert r.score == s.num_pairs / BEAMS[c] and bits(lr.pose_t(r.estimated_pose)) == bits(lr.pose_t(s.estimated_pose))
        assert (bytes(r.relative_pose) != bytes(24)) == bool(ACCEPTED[c])
        # the summaries are the restatement's (the oracle library's QR)
        a, b = RANGES[QUERY_OF[c]]
        lr.assert_summary(s, rorc.refine(PRM, setup.refs[a:b + 1], setup.poses[a:b + 1], setup.cands[c], starts[c],
                                         setup.tables[QUERY_OF[c]]))
    # the window moved every reachable candidate's start towards its truth
    for c in range(4):
        d0 = math.hypot(NODE[c][0] - TRUE[c][0], NODE[c][1] - TRUE[c][1])
        d1 = math.hypot(starts[c][0] - TRUE[c][0], starts[c][1] - TRUE[c][1])
        assert d1 < d0, c


def test_zero_halves_refine_from_the_node_poses(ctx, setup):
    zero = worc.Window(0, 0, 0, 0.05, 0.02)
    got_recs, got_best, got_sums = setup.detect(ctx, zero, GATE)
    sums = setup.rset[0].refine_batch(setup.S, NODE, setup.p, refs=[setup.rset[q] for q in QUERY_OF])
    assert got_best == [0] * 5
    for c, s in enumerate(sums):
        assert got_sums[c] == bytes(s), c
        q = QUERY_OF[c]
        want = worc.record(lr.node_pose(setup.poses, q), RANGES[q][0], 100 + c, s, worc.gate_accepts(GATE, s, NODE[c]),
                           BEAMS[c])
        assert got_recs[c] == want, c
    recs, best, csums, _, _, _ = setup.composition(ctx, zero, GATE)
    assert (recs, best, csums) == (got_recs, got_best, got_sums)


def test_batch_equals_lone_calls_runs_and_contexts(ctx, setup, world):
    batch = setup.detect(ctx, WIN, GATE)
    assert setup.detect(ctx, WIN, GATE) == batch, "run == run"
    for c in range(5):
        recs, best, sums = setup.detect(ctx, WIN, GATE, [c])
        assert (recs[0], best[0], sums[0]) == (batch[0][c], batch[1][c], batch[2][c]), c
    other = abi.Context(0)
    try:
        theirs = Setup(other, world)
        assert theirs.detect(other, WIN, GATE) == batch, "context == context"
        cost_a, pairs_a = ctx.icp_window_scores(setup.rset[1], setup.S[3], NODE[3], awin(WIN), setup.p)
        cost_b, pairs_b = other.icp_window_scores(theirs.rset[1], theirs.S[3], NODE[3], awin(WIN), theirs.p)
        assert bits(cost_a) == bits(cost_b) and pairs_a.tolist() == pairs_b.tolist()
        theirs.rset.close()
    finally:
        other.close()


def test_the_sharded_detect_function_equals_its_halves(ctx, setup):
    maps = [loopbatch.LocalMap(None, 0.0, 0.0, 0.05, lr.node_pose(setup.poses, q), RANGES[q][0]) for q in (0, 1)]
    cands = [loopbatch.Candidate(QUERY_OF[c], setup.cands[c].ranges, setup.cands[c].angles, NODE[c], 100 + c)
             for c in range(5)]
    fn = loopbatch.hip_detect_fn_icp(ctx, setup.rset, maps, cands, setup.p, awin(WIN), abi.LoopRefineGate(*GATE))
    whole = loopbatch.run_sharded(cands, fn)
    best = list(fn.best)
    assert whole.shape == (5, 176) and len(best) == 5 and len(fn.summaries) == 5
    lo = fn(loopbatch.sub_queries(cands, 0, 2), 0, 2)
    best_lo = list(fn.best)
    hi = fn(loopbatch.sub_queries(cands, 2, 5), 2, 5)
    assert np.array_equal(np.concatenate([lo, hi]), whole) and best_lo + list(fn.best) == best
    # ... and the two ranks of a sharded run (three and two candidates)
    parts = [fn(loopbatch.sub_queries(cands, *loopbatch.shard_bounds(5, 2, r)), *loopbatch.shard_bounds(5, 2, r))
             for r in (0, 1)]
    assert np.array_equal(np.concatenate(parts), whole)
    rows = loopbatch.decode(whole)
    assert [r.end_node_index for r in rows] == [100 + c for c in range(5)] and sum(r.found for r in rows) >= 1


@pytest.mark.parametrize("n", [2, 20])
def test_two_waits_and_one_score_launch_per_call(ctx, setup, n):
    cl = [setup.cl[c % 5] for c in sorted(range(n), key=lambda k: QUERY_OF[k % 5])]
    first = sum(1 for k in range(n) if QUERY_OF[k % 5] == 0)
    queries = [(None, None, lr.node_pose(setup.poses, 0), 0, 0, first), (None, None, lr.node_pose(setup.poses, 1), 3, first, n - first)]
    before = ctx.icp_window_stats()
    refines = ctx.icp_ref_set_stats().refine_launches
    _, best, _ = ctx.loop_detect_icp(setup.qrefs, queries, cl, setup.p, awin(WIN), abi.LoopRefineGate(*GATE))
    after = ctx.icp_window_stats()
    assert all(p >= 0 for p in best)
    assert (after.calls - before.calls, after.score_launches - before.score_launches, after.syncs - before.syncs,
            after.refine_launches - before.refine_launches) == (1, 1, 2, 1)
    assert ctx.icp_ref_set_stats().refine_launches == refines + 1
    # the dense entry point: one launch, one wait, no refine
    ctx.icp_window_scores(setup.rset[0], setup.S[0], NODE[0], awin(WIN), setup.p)
    dense = ctx.icp_window_stats()
    assert (dense.calls - after.calls, dense.score_launches - after.score_launches, dense.syncs - after.syncs,
            dense.refine_launches - after.refine_launches) == (1, 1, 1, 0)
    # no candidate: no device work
    ctx.loop_detect_icp([setup.rset[0]], [(None, None, (0.0, 0.0, 0.0), 0, 0, 0)], [], setup.p, awin(WIN),
                        abi.LoopRefineGate(*GATE))
    assert ctx.icp_window_stats() == dense


# ------------------------------------------------------------------ 4. what it achieves
ACH_PRM = orc.Params(8, 0.0, 0.01, 20.0, 1e-3, 1e-3, 0.25, 3.0)
ACH_TRUE, ACH_NODE = (-0.2, 0.25, -0.05), (-0.5, 0.65, -0.2)
ACH_WIN = worc.Window(5, 5, 3, 0.1, 0.05)   # 11 x 11 x 7; the truth lies on the lattice pose (8, 1, 6)


def test_the_window_ends_closer_to_the_truth_than_the_node_pose(ctx, setup, world):
    """A candidate whose node pose is 0.5 m and 0.15 rad off, with a correspondence distance of 0.25 m: the
    refine from the node pose falls into a wrong minimum, the window's best pose is the lattice pose on the
    truth and the refine from there ends strictly closer, in distance and in angle.  (By the restatement: 14
    pairs, 0.42 m and 0.13 rad off, against 57 pairs, 7 mm and 0.4 mrad.)"""
    p = abi.IcpParams(*ACH_PRM)
    ref = ctx.icp_ref(setup.ref_scans[:4], setup.poses[:4], p)
    cur = cand_scan(world, ACH_TRUE, 65)
    scan = lr.dev_scan(ctx, cur)
    out, best, sums = ctx.loop_detect_icp([ref], [(None, None, setup.poses[0], 0, 0, 1)], [(scan, ACH_NODE, 9)], p,
                                          awin(ACH_WIN), abi.LoopRefineGate(3, INF, INF, INF))
    plain = ref.refine(scan, ACH_NODE, p)
    err = lambda e: (math.hypot(e.x - ACH_TRUE[0], e.y - ACH_TRUE[1]), abs(worc.normalize_angle(e.theta - ACH_TRUE[2])))
    (d0, a0), (d1, a1) = err(plain.estimated_pose), err(out[0].estimated_pose)
    print(f"from the node pose: {plain.num_pairs} pairs, {d0:.4f} m, {a0:.4f} rad; from lattice pose {best[0]} "
          f"{worc.decode(ACH_WIN, best[0])}: {sums[0].num_pairs} pairs, {d1:.3e} m, {a1:.3e} rad")
    assert d1 < d0 and a1 < a0
    # the lattice pose nearest the truth
    start = worc.lattice_pose(ACH_WIN, ACH_NODE, best[0])
    dist = lambda q: (q[0] - ACH_TRUE[0]) ** 2 + (q[1] - ACH_TRUE[1]) ** 2 + (q[2] - ACH_TRUE[2]) ** 2
    nearest = min(range(worc.num_poses(ACH_WIN)), key=lambda k: dist(worc.lattice_pose(ACH_WIN, ACH_NODE, k)))
    assert best[0] == nearest and worc.decode(ACH_WIN, best[0]) == (8, 1, 6)
    assert out[0].found == 1 and bits(lr.pose_t(sums[0].initial_pose)) == bits(start)
    # the restatement with the oracle library's QR agrees on both refines
    rt = rorc.concat_tables(ACH_PRM, setup.refs[:4], setup.poses[:4])
    lr.assert_summary(sums[0], rorc.refine(ACH_PRM, None, None, cur, start, rt))
    lr.assert_summary(plain, rorc.refine(ACH_PRM, None, None, cur, ACH_NODE, rt))
    ref.close()
    scan.close()


# ------------------------------------------------------------------ 5. argument checks on the device's side
def raw_detect(ctx, setup, window=WIN, gate=GATE, prm=PRM, queries=None, refs=None, cands=None, n_cand=5, null=None):
    """lgs_loop_detect_icp on poisoned outputs; (status, everything untouched)"""
    queries = setup.queries if queries is None else queries
    qs = (abi.LoopQuery * max(1, len(queries)))()
    for i, (_, _, pose, idx, first, cnt) in enumerate(queries):
        qs[i] = abi.LoopQuery(None, None, abi.Pose2D(*pose), idx, first, cnt)
    cands = setup.cl if cands is None else cands
    cs = (abi.LoopCandidate * 5)(*[abi.LoopCandidate(s.h if s is not None else None, abi.Pose2D(*pose), idx, 0)
                                   for s, pose, idx in cands])
    refs = setup.qrefs if refs is None else refs
    rarr = (C.c_void_p * max(1, len(refs)))(*[r.h if r is not None else None for r in refs])
    recs = (abi.LoopResult * 5)()
    best = (C.c_int * 5)(*[77] * 5)
    sums = (abi.IcpSummary * 5)()
    C.memset(recs, 0xAB, C.sizeof(recs))
    C.memset(sums, 0xAB, C.sizeof(sums))
    before = bytes(recs), bytes(best), bytes(sums)
    p, w, g = abi.IcpParams(*prm), awin(window), abi.LoopRefineGate(*gate)
    a = dict(best=best, sums=sums)
    if null:
        a[null] = None
    st = ctx.lib.lgs_loop_detect_icp(ctx.h, rarr, qs, len(queries), cs, n_cand, C.byref(p), C.byref(w), C.byref(g), recs,
                                     a["best"], a["sums"])
    return st, (bytes(recs), bytes(best), bytes(sums)) == before


def test_invalid_arguments_leave_the_outputs_untouched(ctx, setup, world):
    BAD = (LGS_ERR_INVALID_ARG, True)
    assert raw_detect(ctx, setup) == (0, False)
    for null in ("best", "sums"):   # the optional outputs
        assert raw_detect(ctx, setup, null=null)[0] == 0
    assert raw_detect(ctx, setup, refs=[setup.rset[0], None]) == BAD
    assert raw_detect(ctx, setup, cands=setup.cl[:4] + [(None, NODE[4], 104)]) == BAD
    # the query-cover rule
    q0, q1 = setup.queries
    for queries in ([q0], [q0, q1[:4] + (3, 2)], [q0, q1[:4] + (2, 4)], [q0, q1[:4] + (2, -1)], [q1, q0]):
        assert raw_detect(ctx, setup, queries=queries, refs=[setup.rset[0]] * len(queries)) == BAD, queries
    assert raw_detect(ctx, setup, n_cand=-1) == BAD
    # a centre that is not finite; an outermost lattice pose that is not
    for bad in ((NAN, 0.0, 0.0), (0.0, INF, 0.0), (0.0, 0.0, -INF)):
        assert raw_detect(ctx, setup, cands=setup.cl[:4] + [(setup.S[4], bad, 104)]) == BAD, bad
    assert raw_detect(ctx, setup, window=(2, 2, 1, 1e307, 0.02), cands=setup.cl[:4] + [(setup.S[4], (1.7e308, 0.0, 0.0), 104)]) == BAD
    # the window, the gate and the parameters, with a live context this time
    for w in ((513, 0, 0, 0.05, 0.02), (2, 2, -1, 0.05, 0.02), (2, 2, 1, 0.0, 0.02), (2, 2, 1, 0.05, NAN), (512, 512, 0, 0.05, 0.02)):
        assert raw_detect(ctx, setup, window=w) == BAD, w
    for g in ((2, 1.0, 1.0, 1.0), (3, NAN, 1.0, 1.0), (3, 1.0, -1.0, 1.0)):
        assert raw_detect(ctx, setup, gate=g) == BAD, g
    # the refine-time rules of lgs_icp_ref_*: the bound parameters, the reference's context
    assert raw_detect(ctx, setup, prm=PRM._replace(max_correspondence_dist=0.5)) == BAD
    assert raw_detect(ctx, setup, prm=PRM._replace(usable_range_max=math.nextafter(PRM.usable_range_max, 0.0))) == BAD
    assert raw_detect(ctx, setup, prm=PRM._replace(num_iterations_max=2, rotation_regularizer=0.5))[0] == 0
    # a scan of more than 4096 beams
    long_scan = lr.dev_scan(ctx, cand_scan(world, TRUE[4], 4097))
    assert raw_detect(ctx, setup, cands=setup.cl[:4] + [(long_scan, NODE[4], 104)]) == BAD
    cost, pairs = np.full(75, 7.5), np.full(75, 77, dtype=np.int32)
    p, w = abi.IcpParams(*PRM), awin(WIN)

    def raw_scores(ref, scan, centre):
        st = ctx.lib.lgs_icp_ref_window_scores(ctx.h, ref.h, scan.h, abi.Pose2D(*centre), C.byref(w), C.byref(p),
                                               abi.dptr(cost), pairs.ctypes.data_as(C.POINTER(C.c_int)))
        return st, bool((cost == 7.5).all() and (pairs == 77).all())

    assert raw_scores(setup.rset[0], long_scan, NODE[0]) == BAD
    assert raw_scores(setup.rset[0], setup.S[0], (NAN, 0.0, 0.0)) == BAD
    # a lattice theta outside the restated sincos domain: LGS_ERR_INTERNAL, nothing written
    assert raw_scores(setup.rset[0], setup.S[0], (0.0, 0.0, 2e8)) == (LGS_ERR_INTERNAL, True)
    assert raw_detect(ctx, setup, cands=setup.cl[:4] + [(setup.S[4], (0.0, 0.0, 2e8), 104)]) == (LGS_ERR_INTERNAL, True)
    other = abi.Context(0)
    try:
        theirs = other.icp_ref([lr.dev_scan(other, setup.refs[0])], [setup.poses[0]], setup.p)
        assert raw_detect(ctx, setup, refs=[setup.rset[0], theirs]) == BAD
        assert raw_scores(theirs, setup.S[0], NODE[0]) == BAD
        theirs.close()
    finally:
        other.close()
    assert raw_scores(setup.rset[0], setup.S[0], NODE[0]) == (0, False)
    long_scan.close()
