#!/usr/bin/env python3
"""What the bit-exact greedy-endpoint cost (LGS_COST_GREEDY_ENDPOINT_EXACT) costs
per match against the default cost stage, through the correlative matcher's
entry points.

  A  kind 0: the namesake entry point (k_cost: device cos / sin / exp, tree sum,
     guard records and the host's fix-up of near-boundary cells)
  B  kind 2: the `_cost` entry point with the exact kind (k_cost_gx: restated
     sincos, table terms, seven beam-order chains)
  P  (with --parent-lib) kind 0 through another build of the library, the
     parent commit's: its kind-0 kernels are the same source, so P against A
     shows what the build itself moved

timed in the same process, interleaved P/A/B/P/A/B, --rounds rounds each after
--warmup untimed rounds, lgs_ctx_synchronize around every timed region, no
profiler attached:

  config4_frontend   lone calls, the launcher JSON frontend window (LowRes 5,
                     0.2 m / 0.2 m / 0.5 rad: the small-window path), 1081 beams
  config2_batch128   one 128-query batch, the config-2 window (+-2 m, +-30 deg)
  config5_loop64     a 64-candidate loop batch (4 local maps of 600 x 600 cells,
                     16 nodes each, 1081 beams) through the correlative detector,
                     the JSON loop window

One JSON line per case: per arm the wall clock of every round in ms, the
median and the spread (max - min), b_minus_a_us_per_match = (median B - median
A) / matches, and b_within_a_spread = |median B - median A| <= spread A (the
run-to-run spread this tool itself measures between the A rounds); with P the
same two figures for A against P.
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
FRONTEND = (5, 0.2, 0.2, 0.5, 20.0)
CONFIG2 = (5, 4.0, 4.0, 1.0471976, 20.0)
LOOP = (5, 5.0, 5.0, 1.0, 20.0)
BUILDER = (0.01, 20.0, 0.6, 0.45)


def context_over(path):
    """an abi.Context over another build of the library (symbols it lacks stay unbound)"""
    lib = C.CDLL(path)
    for name, res, args in abi._PROTOS:
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    ctx = abi.Context.__new__(abi.Context)
    ctx.lib = lib
    h = abi._P()
    assert lib.lgs_ctx_create(0, C.byref(h)) == 0
    ctx.h = h
    return ctx


def interleaved(arms, rounds, warmup):
    """arms: [(ctx, run)]; ms of every timed round of every arm, interleaved"""
    times = [[] for _ in arms]
    for k in range(warmup + rounds):
        for (ctx, run), sink in zip(arms, times):
            ctx.synchronize()
            t0 = time.perf_counter()
            run()
            ctx.synchronize()
            if k >= warmup:
                sink.append(1e3 * (time.perf_counter() - t0))
    return times


def line(case, matches, names, times, **extra):
    out = dict(case=case, matches_per_round=matches, rounds=len(times[0]))
    med = {}
    for name, t in zip(names, times):
        med[name] = statistics.median(t)
        out[f"{name}_ms"] = round(med[name], 4)
        out[f"{name}_spread_ms"] = round(max(t) - min(t), 4)
        out[f"{name}_us_per_match"] = round(1e3 * med[name] / matches, 3)
        out[f"{name}_rounds_ms"] = [round(v, 4) for v in t]
    spread_a = out["a_spread_ms"]
    out["b_minus_a_us_per_match"] = round(1e3 * (med["b"] - med["a"]) / matches, 3)
    out["b_over_a"] = round(med["b"] / med["a"], 4)
    out["b_within_a_spread"] = bool(abs(med["b"] - med["a"]) <= spread_a)
    if "p" in med:
        out["a_minus_p_us_per_match"] = round(1e3 * (med["a"] - med["p"]) / matches, 3)
        out["a_within_p_spread"] = bool(abs(med["a"] - med["p"]) <= out["p_spread_ms"])
    out.update(extra)
    print(json.dumps(out), flush=True)
    return out


_MAP = {}


def make_grid(ctx, world):
    """the 1000 x 1000 frontend map (built once) as a grid of `ctx`"""
    if not _MAP:
        ang = scene.beam_angles(1081)
        w, h, mx, my = scene.map_geometry(1000, 100, 0.05)
        _MAP["m"] = (scene.approx_occupancy_map(world, scene.arc_poses(10), ang, w, h, mx, my, 0.05), mx, my)
    return ctx.grid_from_array(*_MAP["m"], 0.05)


def frontend(ctxs, world, args):
    """ctxs: [(name, ctx, cost)]"""
    ang = scene.beam_angles(1081)
    rng = np.random.default_rng(4)
    n = args.frontend_calls
    raw = []
    for _ in range(n):
        true = (rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(-np.pi, np.pi))
        init = (true[0] + rng.uniform(-0.05, 0.05), true[1] + rng.uniform(-0.05, 0.05), true[2] + rng.uniform(-0.1, 0.1))
        raw.append((scene.ray_cast(world, true, ang), init))
    prm = abi.RtcsmParams(*FRONTEND)
    arms, last = [], {}
    for name, ctx, cost in ctxs:
        grid = make_grid(ctx, world)
        items = [(ctx.scan(r, ang), init) for r, init in raw]

        def run(ctx=ctx, grid=grid, items=items, cost=cost, name=name):
            for s, init in items:
                last[name] = ctx.optimize_pose_query(grid, prm, cost, s, init)

        arms.append((ctx, run))
    times = interleaved(arms, args.rounds, args.warmup)
    a, b = last["a"], last["b"]
    close = abs(a.normalized_cost - b.normalized_cost) <= 1e-5 and \
        np.allclose(list(a.covariance), list(b.covariance), rtol=0, atol=1e-5)
    return line("config4_frontend", n, [c[0] for c in ctxs], times, last_match_within_1e5=bool(close),
                last_match_same_pose=bool(a.best_sensor_pose.tuple() == b.best_sensor_pose.tuple()))


def batch128(ctxs, world, args):
    ang = scene.beam_angles(1081)
    rng = np.random.default_rng(2)
    raw, inits = [], []
    for _ in range(128):
        true = (rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(-np.pi, np.pi))
        raw.append(scene.ray_cast(world, true, ang))
        inits.append((true[0] + rng.uniform(-0.3, 0.3), true[1] + rng.uniform(-0.3, 0.3), true[2] + rng.uniform(-0.2, 0.2)))
    prm = abi.RtcsmParams(*CONFIG2)
    arms, keep = [], {}
    for name, ctx, cost in ctxs:
        grid = make_grid(ctx, world)
        scans = [ctx.scan(r, ang) for r in raw]

        def run(ctx=ctx, grid=grid, scans=scans, cost=cost, name=name):
            keep[name] = ctx.optimize_pose_query_batch(grid, prm, cost, scans, inits)

        arms.append((ctx, run))
    times = interleaved(arms, args.rounds, args.warmup)
    worst = max(abs(a.normalized_cost - b.normalized_cost) for a, b in zip(keep["a"], keep["b"]))
    return line("config2_batch128", 128, [c[0] for c in ctxs], times, max_cost_difference=worst)


def loop64(ctxs, world, args):
    bp = abi.BuilderParams(*BUILDER)
    ctx0 = ctxs[0][1]

    def build(poses, ang):
        m = ctx0.map(0.05, 100, 600, 600)
        m.construct([ctx0.scan(scene.ray_cast(world, p, ang), ang) for p in poses], poses, bp)
        cells, _, _ = m.download()
        g = m.geometry()
        return cells, g["min_x"], g["min_y"], 0.05

    maps, cands = scene.loop_problem(world, build, n_maps=4, nodes_per_map=16, n_beams=1081, seed=5,
                                     perturb=(2.0, 0.4), arc_scans=10)
    prm = abi.RtcsmParams(*LOOP)
    arms, keep = [], {}
    for name, ctx, cost in ctxs:
        fn = loopbatch.hip_detect_fn(ctx, maps, cands, prm, cost, 0.6)

        def run(fn=fn, name=name):
            keep[name] = loopbatch.run_sharded(cands, fn)

        arms.append((ctx, run))
    times = interleaved(arms, args.rounds, args.warmup)
    found = [len(loopbatch.loop_results(keep[c[0]])) for c in ctxs]
    return line("config5_loop64", len(cands), [c[0] for c in ctxs], times, found=found)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7, help="timed rounds of every arm (at least 5)")
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds first")
    ap.add_argument("--frontend-calls", type=int, default=200, help="lone calls per round of config4_frontend")
    ap.add_argument("--cases", default="frontend,batch,loop")
    ap.add_argument("--parent-lib", default=None, help="another build of liblgs_hip.so: adds arm P (its kind 0)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("--rounds must be at least 5")
    ctx = abi.Context(0)
    ge = abi.CostGEParams(*COST)
    ctxs = [("a", ctx, ge), ("b", ctx, abi.cost_spec(ge, exact=True))]
    parent = None
    if args.parent_lib:
        parent = context_over(args.parent_lib)
        ctxs.insert(0, ("p", parent, ge))
    world = scene.make_world()
    lines = []
    cases = args.cases.split(",")
    if "frontend" in cases:
        lines.append(frontend(ctxs, world, args))
    if "batch" in cases:
        lines.append(batch128(ctxs, world, args))
    if "loop" in cases:
        lines.append(loop64(ctxs, world, args))
    if parent is not None:
        parent.close()
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
