#!/usr/bin/env python3
"""What a search matcher constructed with CostSquareError costs per match, before
and after the cost became a stage of the matchers' own entry points.

  A  the chained path: the greedy-endpoint entry point (k_cost, 7 workgroups per
     match, one synchronisation), then lgs_summaries_apply_cost_sq (the best
     poses uploaded again, k_sq_cost_batch, a second synchronisation)
  B  the `_cost` entry point with LGS_COST_SQUARE_ERROR (correlative matcher:
     k_cost_sq inside the pipeline, one synchronisation)

timed in the same process on the same context, interleaved A/B/A/B, --rounds
rounds each after --warmup untimed rounds, lgs_ctx_synchronize around every
timed region, no profiler attached:

  config4_frontend   lone calls, the launcher JSON frontend window (LowRes 5,
                     0.2 m / 0.2 m / 0.5 rad: the small-window path), 1081 beams
  config2_batch128   one 128-query batch, the config-2 window (+-2 m, +-30 deg)
  config5_loop64_*   a 64-candidate loop batch (4 local maps of 600 x 600 cells,
                     16 nodes each, 1081 beams) through the three detectors:
                     here A is the greedy-endpoint detector and B the
                     square-error one (rtcsm: the JSON loop window; bb: the JSON
                     branch-and-bound window; gs: a 1 m / 1 m / 0.2 rad window
                     at 0.05 m / 0.05 m / 0.01 rad, 9261 poses)

One JSON line per case: per round the wall clock of the whole region in ms,
their median and spread (max - min) for A and B, saving_us_per_match =
(median A - median B) / matches, and b_not_slower = median B <= median A +
spread A (the run-to-run spread this tool itself measures between the A rounds).
For the config5_loop64_* cases A is another cost function, not the path B
replaces: their lines report what the square-error detector costs, they are no bar.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "my-lidar-graph-slam_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

from lgs_amd import abi, loopbatch, scene   # noqa: E402

COST = (0.01, 20.0, 0.075, 0.1, 1, 0.05, 1.0)    # the launcher-built CostGreedyEndpoint
SQ = (0.01, 20.0)                                # CostSquareError in launcher_settings_default.json
FRONTEND = (5, 0.2, 0.2, 0.5, 20.0)
CONFIG2 = (5, 4.0, 4.0, 1.0471976, 20.0)
LOOP = (5, 5.0, 5.0, 1.0, 20.0)
LOOP_BB = (6, 2.0, 2.0, 1.0, 20.0, 0.01, 20.0)
LOOP_GS = (1.0, 1.0, 0.2, 0.05, 0.05, 0.01, 0.01, 20.0)
BUILDER = (0.01, 20.0, 0.6, 0.45)


def interleaved(ctx, run_a, run_b, rounds, warmup):
    """ms of every timed round of A and of B, A/B/A/B"""
    ta, tb = [], []
    for k in range(warmup + rounds):
        for run, sink in ((run_a, ta), (run_b, tb)):
            ctx.synchronize()
            t0 = time.perf_counter()
            run()
            ctx.synchronize()
            if k >= warmup:
                sink.append(1e3 * (time.perf_counter() - t0))
    return ta, tb


def line(case, matches, ta, tb, **extra):
    ma, mb = statistics.median(ta), statistics.median(tb)
    sa, sb = max(ta) - min(ta), max(tb) - min(tb)
    out = dict(case=case, matches_per_round=matches, rounds=len(ta),
               a_ms=round(ma, 4), a_spread_ms=round(sa, 4), b_ms=round(mb, 4), b_spread_ms=round(sb, 4),
               a_us_per_match=round(1e3 * ma / matches, 3), b_us_per_match=round(1e3 * mb / matches, 3),
               saving_us_per_match=round(1e3 * (ma - mb) / matches, 3), b_not_slower=bool(mb <= ma + sa),
               a_rounds_ms=[round(t, 4) for t in ta], b_rounds_ms=[round(t, 4) for t in tb], **extra)
    print(json.dumps(out), flush=True)
    return out


def frontend(ctx, world, grid, args):
    ang = scene.beam_angles(1081)
    rng = np.random.default_rng(4)
    n = args.frontend_calls
    items = []
    for _ in range(n):
        true = (rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(-np.pi, np.pi))
        init = (true[0] + rng.uniform(-0.05, 0.05), true[1] + rng.uniform(-0.05, 0.05), true[2] + rng.uniform(-0.1, 0.1))
        items.append((ctx.scan(scene.ray_cast(world, true, ang), ang), abi.Pose2D(*init)))
    lib, h = ctx.lib, ctx.h
    prm, ge, sq = abi.RtcsmParams(*FRONTEND), abi.CostGEParams(*COST), abi.CostSQParams(*SQ)
    spec = abi.cost_spec(sq)
    out = abi.RtcsmSummary()
    garr = (abi._P * 1)(grid.h)
    sarrs = [(abi._P * 1)(s.h) for s, _ in items]
    sums = (abi.RtcsmSummary * 1)()

    def run_a():
        for (s, p), sarr in zip(items, sarrs):
            rc = lib.lgs_rtcsm_optimize_pose_query(h, grid.h, C.byref(prm), C.byref(ge), s.h, p, C.byref(sums[0]))
            rc |= lib.lgs_summaries_apply_cost_sq(h, garr, C.byref(sq), sarr, sums, 1)
            assert rc == 0

    def run_b():
        for s, p in items:
            assert lib.lgs_rtcsm_optimize_pose_query_cost(h, grid.h, C.byref(prm), C.byref(spec), s.h, p,
                                                          C.byref(out)) == 0

    ta, tb = interleaved(ctx, run_a, run_b, args.rounds, args.warmup)
    same = sums[0].normalized_cost == out.normalized_cost and list(sums[0].covariance) == list(out.covariance)
    return line("config4_frontend", n, ta, tb, same_cost_last_match=bool(same))


def batch128(ctx, world, grid, args):
    ang = scene.beam_angles(1081)
    rng = np.random.default_rng(2)
    scans, inits = [], []
    for _ in range(128):
        true = (rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(-np.pi, np.pi))
        scans.append(ctx.scan(scene.ray_cast(world, true, ang), ang))
        inits.append((true[0] + rng.uniform(-0.3, 0.3), true[1] + rng.uniform(-0.3, 0.3), true[2] + rng.uniform(-0.2, 0.2)))
    prm, ge, sq = abi.RtcsmParams(*CONFIG2), abi.CostGEParams(*COST), abi.CostSQParams(*SQ)
    keep = {}

    def run_a():
        keep["a"] = ctx.summaries_apply_cost_sq(grid, sq, scans, ctx.optimize_pose_query_batch(grid, prm, ge, scans, inits))

    def run_b():
        keep["b"] = ctx.optimize_pose_query_batch(grid, prm, sq, scans, inits)

    ta, tb = interleaved(ctx, run_a, run_b, args.rounds, args.warmup)
    same = all(a.normalized_cost == b.normalized_cost and list(a.covariance) == list(b.covariance)
               for a, b in zip(keep["a"], keep["b"]))
    return line("config2_batch128", 128, ta, tb, same_costs=bool(same))


def loops(ctx, world, args):
    bp = abi.BuilderParams(*BUILDER)

    def build(poses, ang):
        m = ctx.map(0.05, 100, 600, 600)
        m.construct([ctx.scan(scene.ray_cast(world, p, ang), ang) for p in poses], poses, bp)
        cells, _, _ = m.download()
        g = m.geometry()
        return cells, g["min_x"], g["min_y"], 0.05

    out = []
    ge, sq = abi.CostGEParams(*COST), abi.CostSQParams(*SQ)
    for name, factory, prm, perturb in (("rtcsm", loopbatch.hip_detect_fn, abi.RtcsmParams(*LOOP), (2.0, 0.4)),
                                        ("bb", loopbatch.hip_detect_fn_bb, abi.BBParams(*LOOP_BB), (0.8, 0.3)),
                                        ("gs", loopbatch.hip_detect_fn_gs, abi.GSParams(*LOOP_GS), (0.4, 0.08))):
        maps, cands = scene.loop_problem(world, build, n_maps=4, nodes_per_map=16, n_beams=1081, seed=5,
                                         perturb=perturb, arc_scans=10)
        fa, fb = factory(ctx, maps, cands, prm, ge, 0.6), factory(ctx, maps, cands, prm, sq, 0.6)
        keep = {}

        def run_a():
            keep["a"] = loopbatch.run_sharded(cands, fa)

        def run_b():
            keep["b"] = loopbatch.run_sharded(cands, fb)

        ta, tb = interleaved(ctx, run_a, run_b, args.rounds, args.warmup)
        found_a = len(loopbatch.loop_results(keep["a"]))
        found_b = len(loopbatch.loop_results(keep["b"]))
        out.append(line(f"config5_loop64_{name}", len(cands), ta, tb, a="greedy-endpoint detector",
                        b="square-error detector", found=[found_a, found_b]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7, help="timed rounds of A and of B (at least 5)")
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds first")
    ap.add_argument("--frontend-calls", type=int, default=200, help="lone calls per round of config4_frontend")
    ap.add_argument("--cases", default="frontend,batch,loop")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("--rounds must be at least 5")
    ctx = abi.Context(0)
    world = scene.make_world()
    lines = []
    cases = args.cases.split(",")
    if "frontend" in cases or "batch" in cases:
        ang = scene.beam_angles(1081)
        w, h, mx, my = scene.map_geometry(1000, 100, 0.05)
        cells = scene.approx_occupancy_map(world, scene.arc_poses(10), ang, w, h, mx, my, 0.05)
        grid = ctx.grid_from_array(cells, mx, my, 0.05)
        if "frontend" in cases:
            lines.append(frontend(ctx, world, grid, args))
        if "batch" in cases:
            lines.append(batch128(ctx, world, grid, args))
    if "loop" in cases:
        lines += loops(ctx, world, args)
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
