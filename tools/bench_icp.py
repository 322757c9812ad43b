#!/usr/bin/env python3
"""Point-to-line ICP matcher (lgs_icp_*) on config 3's shape:
1081-beam scans, 50 steps, convergence threshold 0, a scan matched against the
scan taken a short way off.  K4's linear solver (lgs_linsolve_*, the matcher
config 3 measures) runs in the same process on the same scans for scale.

Prints one JSON line per measurement:
  lone    lgs_icp_optimize_pose: p50 / p90 of the call (the host clock around
          a call that ends in a synchronisation), steps and pairs
  batch   lgs_icp_optimize_pose_batch of 256 refines: refines/s, time per refine
  ref_lone, ref_batch   the same refines through lgs_icp_ref_* against a
          reference of --ref-scans K scans: lgs_icp_ref_create's
          time, the lone refine, the batch of 256 (K = 1: the bytes of `lone`)
  k4      lgs_linsolve_optimize_pose (lone p50 / p90) and _batch of 256
With --ref-set M [M ...] instead, one line per M:
  ref_set lgs_icp_ref_set_create of M references x 10 scans and
          its two halves (table pass, grids), M lgs_icp_ref_create calls over
          the same ranges in the same run, lgs_loop_refine_icp per candidate
With --window HX HY HT instead, one line:
  window  the window search of start poses over (2 HX + 1) x
          (2 HY + 1) x (2 HT + 1) lattice poses, three ways in alternating
          rounds: (A) lgs_icp_ref_optimize_pose_batch over all lattice poses
          with num_iterations_max = 1, reading initial_cost -- the only way to
          score a window without the window kernel; (B)
          lgs_icp_ref_window_scores over the same lattice (compared with A byte
          for byte before anything is timed); (C) lgs_loop_detect_icp for 64
          candidates against 10-scan references

The GPU measurements run in one child process under a time limit; a child that
fails or times out ends the run.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "my-lidar-graph-slam_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

ICP = (50, 0.0, 0.01, 20.0, 1e-3, 1e-3, 1.0, 0.5)
LINSOLVE = (50, 0.0, 0.01, 20.0, 1e-3, 1e-3, 0.01, 20.0)
BATCH = 256


def pct(t, q):
    return round(float(np.percentile(1e6 * np.array(t), q)), 1)


def gpu_step(args):
    import oracle_bind as ob
    from lgs_amd import abi, scene
    world = scene.make_world()
    ang = scene.beam_angles(args.beams)
    rng = np.random.default_rng(11)
    items = []
    for _ in range(BATCH):
        ref = (rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), rng.uniform(-np.pi, np.pi))
        true = (ref[0] + rng.uniform(-0.2, 0.2), ref[1] + rng.uniform(-0.2, 0.2), ref[2] + rng.uniform(-0.05, 0.05))
        init = (true[0] + rng.uniform(-0.05, 0.05), true[1] + rng.uniform(-0.05, 0.05), true[2] + rng.uniform(-0.03, 0.03))
        items.append((ref, true, init))
    ctx = abi.Context(0)
    refs = [ctx.scan(scene.ray_cast(world, r, ang), ang) for r, _, _ in items]
    scans = [ctx.scan(scene.ray_cast(world, t, ang), ang) for _, t, _ in items]
    ref_poses, inits = [r for r, _, _ in items], [i for _, _, i in items]
    P = abi.IcpParams(*ICP)
    for k in range(args.warmup):
        ctx.icp(refs[k], ref_poses[k], scans[k], inits[k], P)
    lone, outs = [], []
    for k in range(args.lone):
        t0 = time.perf_counter()
        o = ctx.icp(refs[k], ref_poses[k], scans[k], inits[k], P)
        lone.append(time.perf_counter() - t0)
        outs.append(o)
    err = [float(np.hypot(o.estimated_pose.x - items[k][1][0], o.estimated_pose.y - items[k][1][1]))
           for k, o in enumerate(outs)]
    print(json.dumps(dict(line="lone", matcher="icp", calls=len(lone), beams=len(ang), settings=list(ICP),
                          p50_us=pct(lone, 50), p90_us=pct(lone, 90),
                          steps_mean=round(float(np.mean([o.iterations for o in outs])), 2),
                          pairs_mean=round(float(np.mean([o.num_pairs for o in outs])), 1),
                          found=int(sum(o.pose_found for o in outs)),
                          p50_us_per_pass=round(pct(lone, 50) / (ICP[0] + 1), 2),
                          median_error_m=float(np.median(err)))), flush=True)
    call = lambda: ctx.icp_batch(refs, ref_poses, scans, inits, P)
    for _ in range(args.warmup):
        call()
    t = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        out = call()
        t.append(time.perf_counter() - t0)
    wall = float(np.median(t))
    print(json.dumps(dict(line="batch", matcher="icp", refines=BATCH, beams=len(ang), call_ms=round(1e3 * wall, 3),
                          refines_per_s=round(BATCH / wall, 1), us_per_refine=round(1e6 * wall / BATCH, 2),
                          found=int(sum(o.pose_found for o in out)))), flush=True)
    # the same refines against a reference of K scans behind a grid (lgs_icp_ref_*):
    # item k's reference scan plus K - 1 scans taken a few centimetres further on; with K = 1 the
    # bytes are lgs_icp_optimize_pose's above
    K, nref = args.ref_scans, min(args.lone, BATCH)
    sets = []
    for k in range(nref):
        rp = [(ref_poses[k][0] + 0.04 * i, ref_poses[k][1] - 0.03 * i, ref_poses[k][2] + 0.01 * i) for i in range(K)]
        sets.append(([refs[k]] + [ctx.scan(scene.ray_cast(world, p, ang), ang) for p in rp[1:]], rp))
    create = []
    handles = []
    for k in range(-args.warmup, nref):
        t0 = time.perf_counter()
        h = ctx.icp_ref(*sets[max(k, 0)], P)
        if k >= 0:
            create.append(time.perf_counter() - t0)
            handles.append(h)
    info = handles[0].info()
    for k in range(args.warmup):
        handles[k % nref].refine(scans[k % nref], inits[k % nref], P)
    lone_r, outs_r = [], []
    for k in range(nref):
        t0 = time.perf_counter()
        o = handles[k].refine(scans[k], inits[k], P)
        lone_r.append(time.perf_counter() - t0)
        outs_r.append(o)
    err = [float(np.hypot(o.estimated_pose.x - items[k][1][0], o.estimated_pose.y - items[k][1][1]))
           for k, o in enumerate(outs_r)]
    # the items differ in how many entries a beam looks at; the spread of one item's repeated calls
    again = []
    for _ in range(8):
        t0 = time.perf_counter()
        handles[0].refine(scans[0], inits[0], P)
        again.append(time.perf_counter() - t0)
    print(json.dumps(dict(line="ref_lone", matcher="icp_ref", ref_scans=K, calls=len(lone_r), beams=len(ang),
                          entries=info.entries, cells=[info.cells_x, info.cells_y], cell_size=info.cell_size,
                          create_p50_us=pct(create, 50), create_p90_us=pct(create, 90),
                          p50_us=pct(lone_r, 50), p90_us=pct(lone_r, 90), p10_us=pct(lone_r, 10),
                          item0_repeated_us=[pct(again, 0), pct(again, 50), pct(again, 100)],
                          steps_mean=round(float(np.mean([o.iterations for o in outs_r])), 2),
                          pairs_mean=round(float(np.mean([o.num_pairs for o in outs_r])), 1),
                          found=int(sum(o.pose_found for o in outs_r)),
                          p50_us_per_pass=round(pct(lone_r, 50) / (ICP[0] + 1), 2),
                          median_error_m=float(np.median(err)),
                          equals_icp_bytes=(all(bytes(a) == bytes(b) for a, b in zip(outs_r, outs)) if K == 1 else None))),
          flush=True)
    # the batch of 256 cycles through the nref references made above
    b_refs = [handles[j % nref] for j in range(BATCH)]
    b_scans, b_inits = [scans[j % nref] for j in range(BATCH)], [inits[j % nref] for j in range(BATCH)]
    call = lambda: handles[0].refine_batch(b_scans, b_inits, P, refs=b_refs)
    for _ in range(args.warmup):
        call()
    t = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        out = call()
        t.append(time.perf_counter() - t0)
    wall = float(np.median(t))
    print(json.dumps(dict(line="ref_batch", matcher="icp_ref", ref_scans=K, refines=BATCH, distinct_refs=nref,
                          beams=len(ang), call_ms=round(1e3 * wall, 3), call_ms_min=round(1e3 * min(t), 3),
                          call_ms_max=round(1e3 * max(t), 3), refines_per_s=round(BATCH / wall, 1),
                          us_per_refine=round(1e6 * wall / BATCH, 2), found=int(sum(o.pose_found for o in out)))),
          flush=True)
    for h in handles:
        h.close()
    # K4 on a map of the same scene, the same current scans and starts
    m = ob.OMap(0.05, 100, 300, 300)
    bp = ob.BuilderParams(0.01, 20.0, 0.6, 0.45)
    mang = scene.beam_angles(361)
    for p in scene.arc_poses(10):
        m.integrate(p, ob.OScan(scene.ray_cast(world, p, mang), mang), bp)
    g = ctx.grid_from_array(m.cells(), m.m.min_x, m.m.min_y, 0.05)
    L = abi.LinsolveParams(*LINSOLVE)
    for k in range(args.warmup):
        ctx.linsolve(g, L, scans[k], inits[k])
    lone = []
    for k in range(args.lone):
        t0 = time.perf_counter()
        ctx.linsolve(g, L, scans[k], inits[k])
        lone.append(time.perf_counter() - t0)
    call = lambda: ctx.linsolve_batch(g, L, scans, inits)
    for _ in range(args.warmup):
        call()
    t = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    wall = float(np.median(t))
    print(json.dumps(dict(line="k4", matcher="linsolve", calls=len(lone), beams=len(ang), settings=list(LINSOLVE),
                          p50_us=pct(lone, 50), p90_us=pct(lone, 90), batch_refines=BATCH,
                          batch_call_ms=round(1e3 * wall, 3), batch_us_per_refine=round(1e6 * wall / BATCH, 2))),
          flush=True)
    ctx.close()


REF_SET_SCANS = 10   # scans per local map of --ref-set


def ref_set_step(args):
    """--ref-set: per M, lgs_icp_ref_set_create of M references x 10 scans against M lgs_icp_ref_create calls
    over the same ranges, alternating in one process, and lgs_loop_refine_icp with one candidate per map.
    Every timed call ends in a host wait on the stream; the host clock is around the whole call."""
    from lgs_amd import abi, scene
    world = scene.make_world()
    ang = scene.beam_angles(args.beams)
    rng = np.random.default_rng(17)
    ctx = abi.Context(0)
    P = abi.IcpParams(*ICP)
    m_max = max(args.ref_set)
    poses, scans, truths, cands = [], [], [], []
    for i in range(m_max):
        c = (rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5))
        for p in scene.arc_poses(REF_SET_SCANS, center=c):
            poses.append(tuple(p))
            scans.append(ctx.scan(scene.ray_cast(world, p, ang), ang))
        true = (c[0] + rng.uniform(-0.5, 0.5), c[1] + rng.uniform(-0.5, 0.5), rng.uniform(-np.pi, np.pi))
        truths.append(true)
        cands.append(ctx.scan(scene.ray_cast(world, true, ang), ang))
    for M in args.ref_set:
        lo = [REF_SET_SCANS * i for i in range(M)]
        hi = [a + REF_SET_SCANS - 1 for a in lo]
        n = REF_SET_SCANS * M

        def lone_creates():
            return [ctx.icp_ref(scans[a:b + 1], poses[a:b + 1], P) for a, b in zip(lo, hi)]

        t_set, t_lone, split = [], [], []
        for k in range(-args.warmup, args.steps):   # the two paths alternate
            t0 = time.perf_counter()
            rset = ctx.icp_ref_set(scans[:n], poses[:n], lo, hi, P)
            t1 = time.perf_counter()
            handles = lone_creates()
            t2 = time.perf_counter()
            if k >= 0:
                t_set.append(t1 - t0)
                t_lone.append(t2 - t1)
                split.append(ctx.icp_ref_set_last_build_ms())
            same = all(rset[i].info() == handles[i].info() for i in range(M))
            for h in handles:
                h.close()
            if k < args.steps - 1:
                rset.close()
        entries = sum(rset[i].info().entries for i in range(M))
        cells = sum(rset[i].info().cells_x * rset[i].info().cells_y for i in range(M))
        # one candidate per map, its record 5 cm and 0.02 rad off the truth
        queries = [(None, None, poses[lo[i]], lo[i], i, 1) for i in range(M)]
        cl = [(cands[i], truths[i], n + i) for i in range(M)]
        gate = abi.LoopRefineGate(3, float("inf"), float("inf"), float("inf"))

        def records():
            recs = (abi.LoopResult * M)()
            for i, t in enumerate(truths[:M]):
                recs[i].found = 1
                recs[i].estimated_pose = abi.Pose2D(t[0] + 0.05, t[1] - 0.03, t[2] + 0.02)
            return recs

        refs = [rset[i] for i in range(M)]
        t_ref = []
        for k in range(-args.warmup, args.steps):
            recs = records()
            t0 = time.perf_counter()
            refined, sums = ctx.loop_refine_icp(refs, queries, cl, P, gate, recs)
            if k >= 0:
                t_ref.append(time.perf_counter() - t0)
        err = [float(np.hypot(recs[i].estimated_pose.x - truths[i][0], recs[i].estimated_pose.y - truths[i][1]))
               for i in range(M) if refined[i]]
        rset.close()
        med = lambda t: float(np.median(t))
        print(json.dumps(dict(line="ref_set", refs=M, scans_per_ref=REF_SET_SCANS, beams=len(ang), entries=entries,
                              cells=cells, timed_calls=args.steps,
                              set_create_ms=round(1e3 * med(t_set), 3), set_create_ms_min_max=[round(1e3 * min(t_set), 3), round(1e3 * max(t_set), 3)],
                              set_table_pass_ms=round(float(np.median([s[0] for s in split])), 3),
                              set_grids_ms=round(float(np.median([s[1] for s in split])), 3),
                              lone_creates_ms=round(1e3 * med(t_lone), 3), lone_creates_ms_min_max=[round(1e3 * min(t_lone), 3), round(1e3 * max(t_lone), 3)],
                              lone_create_us_each=round(1e6 * med(t_lone) / M, 1),
                              set_over_lone=round(med(t_set) / med(t_lone), 4), same_info=bool(same),
                              refine_call_ms=round(1e3 * med(t_ref), 3), refine_us_per_candidate=round(1e6 * med(t_ref) / M, 2),
                              refined=int(sum(refined)), steps=ICP[0], median_error_m=float(np.median(err)) if err else None)),
              flush=True)
    ctx.close()


WINDOW_STEPS = (0.05, 0.01)   # m, rad
WINDOW_MAPS, WINDOW_CANDS = 8, 64


def window_step(args):
    """--window: A, B and C of the module's comment.  Every timed call ends in a host wait on the stream; the
    host clock is around the C call alone (its arrays are made before)."""
    import ctypes as C
    from lgs_amd import abi, scene
    world = scene.make_world()
    ang = scene.beam_angles(args.beams)
    rng = np.random.default_rng(23)
    ctx = abi.Context(0)
    P = abi.IcpParams(*ICP)
    P1 = abi.IcpParams(1, *ICP[1:])
    hx, hy, ht = args.window
    win = abi.IcpWindow(hx, hy, ht, *WINDOW_STEPS)
    nt, ny, nx = win.shape
    n_poses = nt * ny * nx
    poses, scans, lo = [], [], []
    for i in range(WINDOW_MAPS):
        c = (rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5))
        lo.append(len(scans))
        for p in scene.arc_poses(REF_SET_SCANS, center=c):
            poses.append(tuple(p))
            scans.append(ctx.scan(scene.ray_cast(world, p, ang), ang))
    hi = [a + REF_SET_SCANS - 1 for a in lo]
    rset = ctx.icp_ref_set(scans, poses, lo, hi, P)
    truths, nodes, cands, query_of = [], [], [], []
    for k in range(WINDOW_CANDS):
        q = k * WINDOW_MAPS // WINDOW_CANDS
        c = poses[lo[q]]
        true = (c[0] + rng.uniform(-0.5, 0.5), c[1] + rng.uniform(-0.5, 0.5), rng.uniform(-np.pi, np.pi))
        # the drift stays inside the window
        node = tuple(t + rng.uniform(-0.8, 0.8) * h * st for t, h, st in
                     zip(true, (hx, hy, ht), (WINDOW_STEPS[0], WINDOW_STEPS[0], WINDOW_STEPS[1])))
        truths.append(true)
        nodes.append(node)
        cands.append(ctx.scan(scene.ray_cast(world, true, ang), ang))
        query_of.append(q)
    # A and B score candidate 0's window
    ref0 = rset[query_of[0]]
    a_refs = (C.c_void_p * n_poses)(*[ref0.h] * n_poses)
    a_scans = (C.c_void_p * n_poses)(*[cands[0].h] * n_poses)
    a_init = (abi.Pose2D * n_poses)(*[abi.Pose2D(*win.pose(nodes[0], p)) for p in range(n_poses)])
    a_out = (abi.IcpSummary * n_poses)()
    b_cost, b_pairs = np.zeros(n_poses), np.zeros(n_poses, dtype=np.int32)

    def run_a():
        ctx.check(ctx.lib.lgs_icp_ref_optimize_pose_batch(ctx.h, a_refs, a_scans, a_init, n_poses, C.byref(P1), a_out),
                  "icp_ref_optimize_pose_batch")

    def run_b():
        ctx.check(ctx.lib.lgs_icp_ref_window_scores(ctx.h, ref0.h, cands[0].h, abi.Pose2D(*nodes[0]), C.byref(win),
                                                    C.byref(P), abi.dptr(b_cost),
                                                    b_pairs.ctypes.data_as(C.POINTER(C.c_int))), "icp_ref_window_scores")

    # C: all candidates, queries in map order
    qs = (abi.LoopQuery * WINDOW_MAPS)()
    per = WINDOW_CANDS // WINDOW_MAPS
    for q in range(WINDOW_MAPS):
        qs[q] = abi.LoopQuery(None, None, abi.Pose2D(*poses[lo[q]]), lo[q], q * per, per)
    cs = (abi.LoopCandidate * WINDOW_CANDS)(*[abi.LoopCandidate(cands[k].h, abi.Pose2D(*nodes[k]), 1000 + k, 0)
                                              for k in range(WINDOW_CANDS)])
    c_refs = (C.c_void_p * WINDOW_MAPS)(*[rset[q].h for q in range(WINDOW_MAPS)])
    gate = abi.LoopRefineGate(args.beams // 4, float("inf"), 0.5, 0.2)
    c_out = (abi.LoopResult * WINDOW_CANDS)()
    c_best = (C.c_int * WINDOW_CANDS)()

    def run_c():
        ctx.check(ctx.lib.lgs_loop_detect_icp(ctx.h, c_refs, qs, WINDOW_MAPS, cs, WINDOW_CANDS, C.byref(P), C.byref(win),
                                              C.byref(gate), c_out, c_best, None), "loop_detect_icp")

    run_a()
    run_b()
    same = bool(np.array_equal(np.array([o.initial_cost for o in a_out]).view(np.uint64), b_cost.view(np.uint64)) and
                [o.initial_pairs for o in a_out] == b_pairs.tolist())
    if not same:
        print(json.dumps(dict(line="window", error="A and B differ")), flush=True)
        sys.exit(1)
    t = {"a": [], "b": [], "c": []}
    for k in range(-args.warmup, args.steps):   # the three alternate
        for name, fn in (("a", run_a), ("b", run_b), ("c", run_c)):
            t0 = time.perf_counter()
            fn()
            if k >= 0:
                t[name].append(time.perf_counter() - t0)
    med = lambda v: float(np.median(v))
    ms = lambda v: [round(1e3 * med(v), 3), round(1e3 * min(v), 3), round(1e3 * max(v), 3)]
    found = [k for k in range(WINDOW_CANDS) if c_out[k].found]
    err = [float(np.hypot(c_out[k].estimated_pose.x - truths[k][0], c_out[k].estimated_pose.y - truths[k][1])) for k in found]
    drift = [float(np.hypot(nodes[k][0] - truths[k][0], nodes[k][1] - truths[k][1])) for k in range(WINDOW_CANDS)]
    stats = ctx.icp_window_stats()
    print(json.dumps(dict(line="window", halves=[hx, hy, ht], steps=list(WINDOW_STEPS), poses=n_poses, beams=len(ang),
                          scans_per_ref=REF_SET_SCANS, timed_rounds=args.steps, same_bytes=same,
                          a_refine_batch_ms_med_min_max=ms(t["a"]), b_window_scores_ms_med_min_max=ms(t["b"]),
                          a_spread=round((max(t["a"]) - min(t["a"])) / med(t["a"]), 4),
                          a_over_b=round(med(t["a"]) / med(t["b"]), 3),
                          b_ns_per_pose_beam=round(1e9 * med(t["b"]) / (n_poses * len(ang)), 3),
                          c_candidates=WINDOW_CANDS, c_detect_ms_med_min_max=ms(t["c"]),
                          c_ms_per_candidate=round(1e3 * med(t["c"]) / WINDOW_CANDS, 3),
                          c_ns_per_pose_beam=round(1e9 * med(t["c"]) / (WINDOW_CANDS * n_poses * len(ang)), 3),
                          c_found=len(found), c_median_drift_m=round(float(np.median(drift)), 4),
                          c_median_error_m=float(np.median(err)) if err else None,
                          window_stats=list(stats))), flush=True)
    rset.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--beams", type=int, default=1081)
    ap.add_argument("--lone", type=int, default=32, help="lone calls timed")
    ap.add_argument("--steps", type=int, default=5, help="timed batch calls")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ref-scans", type=int, default=1, help="reference scans per lgs_icp_ref (the ref path)")
    ap.add_argument("--timeout", type=float, default=240.0, help="time limit of the GPU step (s)")
    ap.add_argument("--ref-set", type=int, nargs="+", metavar="M",
                    help="instead of the lines above: per M, one lgs_icp_ref_set_create of M references x 10 scans "
                         "against M lgs_icp_ref_create calls, and lgs_loop_refine_icp per candidate (DESIGN.md 4.5d)")
    ap.add_argument("--window", type=int, nargs=3, metavar=("HX", "HY", "HT"),
                    help="instead of the lines above: the window search of (2 HX + 1) x (2 HY + 1) x (2 HT + 1) start "
                         "poses, scored by the refine batch, by lgs_icp_ref_window_scores, and lgs_loop_detect_icp "
                         "for 64 candidates (DESIGN.md 4.5e)")
    ap.add_argument("--step", choices=["gpu"], help=argparse.SUPPRESS)   # child mode
    args = ap.parse_args()
    if args.window and (min(args.window) < 0 or max(args.window) > 512 or
                        np.prod([2 * h + 1 for h in args.window]) > 1048576):
        ap.error("--window: halves in 0 .. 512, at most 1048576 poses")
    if args.ref_set and min(args.ref_set) < 1:
        ap.error("--ref-set: at least one reference")
    if args.step:
        if args.window:
            window_step(args)
        elif args.ref_set:
            ref_set_step(args)
        else:
            gpu_step(args)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "gpu", "--beams", str(args.beams), "--lone",
           str(args.lone), "--steps", str(args.steps), "--warmup", str(args.warmup), "--ref-scans", str(args.ref_scans)]
    if args.ref_set:
        cmd += ["--ref-set"] + [str(m) for m in args.ref_set]
    if args.window:
        cmd += ["--window"] + [str(h) for h in args.window]
    try:
        rc = subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps(dict(line="gpu", error="timeout")), flush=True)
        return 124
    if rc != 0:
        print(json.dumps(dict(line="gpu", error=f"exit status {rc}")), flush=True)
        return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
