#!/usr/bin/env python3
"""Hill-climbing matcher on the launcher's settings (ScanMatcherHillClimbing of
launcher_settings_default.json: steps 0.1 / 0.1, 100 iterations, 5
refinements; the launcher's greedy-endpoint cost) with 1081-beam scans on a
300 x 300 map of 24 scans (a map of fewer scans has no cell below the
occupancy threshold, and the walk never moves on it).  With --cost
square_error the same walks run over CostSquareError (usable range 0.01 / 20.0,
launcher_settings_default.json:12-15): lgs_hc_sq_optimize_pose_query / _batch
and, on the CPU, tests/hc_sq_oracle.py.  There a match pays the initial cost
and the gradient sums at the best pose (five smoothed values per beam), which
are counted as two more passes as well.

Prints one JSON line per measurement:
  lone    lgs_hc_optimize_pose_query: p50 / p90 of the call, passes per match
  batch   lgs_hc_optimize_pose_batch of 64 and of 256 matches: matches/s,
          time per match and per (match, pass) -- a pass is six cost
          evaluations; a match also pays the initial cost and the six of the
          gradient, counted as two more passes
  cpu     the same walks composed over the oracle on the CPU (the reference's
          loop, tests/hc_oracle.py): walks/s, the baseline of the ratios

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

HC = (0.1, 0.1, 100, 5)
COST = (0.01, 20.0, 0.075, 0.1, 1, 0.05, 1.0)
COST_SQ = (0.01, 20.0)
REL = (0.1, -0.05, 0.02)
BATCHES = (64, 256)


def scene_inputs(n, n_beams=1081, cells=300):
    import oracle_bind as ob
    from lgs_amd import scene
    world = scene.make_world()
    ang = scene.beam_angles(n_beams)
    m = ob.OMap(0.05, 100, cells, cells)
    bp = ob.BuilderParams(0.01, 20.0, 0.6, 0.45)
    for p in scene.arc_poses(24):
        m.integrate(p, ob.OScan(scene.ray_cast(world, p, ang), ang), bp)
    rng = np.random.default_rng(11)
    matches = []
    for _ in range(n):
        true = (rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), rng.uniform(-np.pi, np.pi))
        init = (true[0] + rng.uniform(-0.15, 0.15), true[1] + rng.uniform(-0.15, 0.15),
                true[2] + rng.uniform(-0.04, 0.04))
        matches.append((scene.ray_cast(world, true, ang), init))
    return m.cells(), m.m.min_x, m.m.min_y, ang, matches


def gpu_step(args):
    from lgs_amd import abi
    cells, mx, my, ang, matches = scene_inputs(max(BATCHES))
    ctx = abi.Context(0)
    g = ctx.grid_from_array(cells, mx, my, 0.05)
    P = abi.HCParams(*HC)
    if args.cost == "square_error":
        cost, query, batch = abi.CostSQParams(*COST_SQ), ctx.hc_sq_optimize_pose_query, ctx.hc_sq_optimize_pose_batch
    else:
        cost, query, batch = abi.CostGEParams(*COST), ctx.hc_optimize_pose_query, ctx.hc_optimize_pose_batch
    scans = [ctx.scan(r, ang, REL) for r, _ in matches]
    inits = [init for _, init in matches]
    # lone calls: every match once per step, the call's wall clock
    for k in range(args.warmup):
        query(g, P, cost, scans[k % len(scans)], inits[k % len(scans)])
    lone, passes = [], []
    for k in range(args.lone):
        t0 = time.perf_counter()
        s = query(g, P, cost, scans[k], inits[k])
        lone.append(time.perf_counter() - t0)
        passes.append(s.passes)
    lone_us = 1e6 * np.array(lone)
    print(json.dumps(dict(line="lone", cost=args.cost, calls=len(lone), beams=len(ang), settings=list(HC),
                          p50_us=round(float(np.percentile(lone_us, 50)), 1),
                          p90_us=round(float(np.percentile(lone_us, 90)), 1),
                          passes_mean=round(float(np.mean(passes)), 2), passes_min=int(min(passes)),
                          passes_max=int(max(passes)),
                          p50_us_per_pass=round(float(np.percentile(lone_us / (np.array(passes) + 2), 50)), 2))),
          flush=True)
    for n in BATCHES:
        call = lambda: batch(g, P, cost, scans[:n], inits[:n])
        for _ in range(args.warmup):
            out = call()
        t = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            out = call()
            t.append(time.perf_counter() - t0)
        wall = float(np.median(t))
        tot = sum(o.passes + 2 for o in out)
        print(json.dumps(dict(line="batch", cost=args.cost, matches=n, beams=len(ang), call_ms=round(1e3 * wall, 3),
                              matches_per_s=round(n / wall, 1), us_per_match=round(1e6 * wall / n, 2),
                              passes_mean=round(float(np.mean([o.passes for o in out])), 2),
                              passes_max=int(max(o.passes for o in out)),
                              us_per_match_pass=round(1e6 * wall / tot, 3),
                              longest_walk_us_per_pass=round(1e6 * wall / (max(o.passes for o in out) + 2), 2))),
              flush=True)
    ctx.close()


def cpu_line(args):
    """the reference's loop over the oracle's pinned cost, on this CPU"""
    import oracle_bind as ob
    from hc_oracle import compose_hc
    from hc_sq_oracle import compose_hc_sq
    cells, mx, my, ang, matches = scene_inputs(args.cpu_walks)
    g = ob.OGrid(cells, mx, my, 0.05)
    cost = ob.CostGE(*COST)
    t, passes = [], []
    for r, init in matches:
        sc = ob.OScan(r, ang, REL)
        t0 = time.perf_counter()
        if args.cost == "square_error":
            ref = compose_hc_sq(g, sc, init, REL, *HC, usable=COST_SQ)
        else:
            ref = compose_hc(g, cost, sc, init, REL, *HC)
        t.append(time.perf_counter() - t0)
        passes.append(ref.passes)
    ms = 1e3 * np.array(t)
    print(json.dumps(dict(line="cpu", cost=args.cost, walks=len(t), beams=len(ang), p50_ms=round(float(np.percentile(ms, 50)), 3),
                          walks_per_s=round(len(t) / float(np.sum(t)), 1),
                          passes_mean=round(float(np.mean(passes)), 2),
                          us_per_pass=round(1e3 * float(np.sum(ms)) / float(np.sum(np.array(passes) + 2)), 1))),
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lone", type=int, default=64, help="lone calls timed")
    ap.add_argument("--steps", type=int, default=5, help="timed calls per batch size")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-walks", type=int, default=64)
    ap.add_argument("--timeout", type=float, default=240.0, help="time limit of the GPU step (s)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cost", choices=["greedy_endpoint", "square_error"], default="greedy_endpoint",
                    help="the matcher's cost function")
    ap.add_argument("--step", choices=["gpu"], help=argparse.SUPPRESS)   # child mode
    args = ap.parse_args()
    if args.step:
        gpu_step(args)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "gpu", "--lone", str(args.lone), "--steps",
           str(args.steps), "--warmup", str(args.warmup), "--cost", args.cost]
    try:
        rc = subprocess.run(cmd, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps(dict(line="gpu", error="timeout")), flush=True)
        return 124
    if rc != 0:
        print(json.dumps(dict(line="gpu", error=f"exit status {rc}")), flush=True)
        return rc if rc > 0 else 1
    if not args.no_cpu:
        cpu_line(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
