#!/usr/bin/env python3
"""Nearest-node loop searcher (lgs_loop_*): the host loop
against the device path of lgs_loop_search_nearest, both through the same
handle in the same run (LGS_OPT_LOOP_SEARCH_MIN_PAIRS set to 2^62 and to 0), on
snapshots of n nodes in local maps of 25 nodes along a path that keeps
crossing itself.

Prints one JSON line per measurement:
  search     n in {1000, 20000} x q in {1, 64, n} hints (the last q nodes as
             the latest one) x {records only, records + per-map table}: the
             median call time of the host loop and of the device path, pairs =
             q x walk positions, whether the bytes agree
  sweep      per n, q = 1, 2, 4, ... (records only): the two curves the
             crossover is read from
  crossover  the pairs count at which the two curves of a sweep cross (linear
             interpolation between the last point where the host loop is the
             faster one and the next), the smaller of the sweeps' crossings,
             and that count rounded down to a power of two (the default of
             LGS_OPT_LOOP_SEARCH_MIN_PAIRS)

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
for p in (os.path.join(ROOT, "my-lidar-graph-slam_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

PARAMS = (2.0, 0.5, 5)      # travel distance threshold, node distance threshold, candidate nodes
PER_MAP = 25
NEVER, ALWAYS = float(2 ** 62), 0.0


def snapshot(n):
    from lgs_amd import abi
    k = np.arange(n)
    poses = np.stack([4.0 * np.sin(0.0173 * k), 3.0 * np.sin(0.0346 * k + 0.3), np.zeros(n)], axis=1)
    m = (n + PER_MAP - 1) // PER_MAP
    lo = np.arange(m) * PER_MAP
    hi = np.minimum(lo + PER_MAP - 1, n - 1)
    step = np.hypot(np.diff(poses[:, 0]), np.diff(poses[:, 1]))
    accum = np.concatenate([[0.0], np.cumsum(step)])     # close to the library's chain; only the cut's place depends on it
    return poses, lo, hi, accum, abi


def hints_of(abi, nodes, accum):
    nodes = np.asarray(nodes)
    return abi.loop_hints(nodes, nodes // PER_MAP, nodes // PER_MAP + 1, accum[nodes])


def timed(call, reps, warmup):
    for _ in range(warmup):
        out = call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), out


def both(ctx, abi, g, prm, rows, table, reps, warmup):
    """(host seconds, device seconds, same bytes) of one call shape"""
    call = lambda: g.search(prm, rows, per_map=table)
    ctx.set_option(abi.LGS_OPT_LOOP_SEARCH_MIN_PAIRS, NEVER)
    th, a = timed(call, reps, warmup)
    ctx.set_option(abi.LGS_OPT_LOOP_SEARCH_MIN_PAIRS, ALWAYS)
    td, b = timed(call, reps, warmup)
    same = (a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()) if table else a.tobytes() == b.tobytes()
    return th, td, bool(same)


def gpu_step(args):
    curves = {}
    ctx = None
    for n in args.nodes:
        poses, lo, hi, accum, abi = snapshot(n)
        ctx = ctx or abi.Context(0)
        prm = abi.LoopSearchParams(*PARAMS, 0)
        t0 = time.perf_counter()
        g = ctx.loop_graph(poses, lo, hi)
        create = time.perf_counter() - t0
        positions = g.info().positions
        print(json.dumps(dict(line="graph", nodes=n, maps=len(lo), positions=positions,
                              create_ms=round(1e3 * create, 3))), flush=True)
        for q in (1, 64, n):
            rows = hints_of(abi, np.arange(n - q, n), accum)
            for table in (False, True):
                big = q * positions > 10 ** 7
                th, td, same = both(ctx, abi, g, prm, rows, table, 3 if big else args.reps, 1 if big else args.warmup)
                print(json.dumps(dict(line="search", nodes=n, hints=q, per_map_table=table, pairs=q * positions,
                                      host_us=round(1e6 * th, 1), device_us=round(1e6 * td, 1),
                                      host_ns_per_pair=round(1e9 * th / (q * positions), 3),
                                      device_ns_per_pair=round(1e9 * td / (q * positions), 3), same_bytes=same)),
                      flush=True)
        curve = []
        q = 1
        while q <= min(n, 4096):
            rows = hints_of(abi, np.arange(n - q, n), accum)
            th, td, same = both(ctx, abi, g, prm, rows, False, args.reps, args.warmup)
            curve.append((q * positions, th, td))
            print(json.dumps(dict(line="sweep", nodes=n, hints=q, pairs=q * positions, host_us=round(1e6 * th, 1),
                                  device_us=round(1e6 * td, 1), same_bytes=same)), flush=True)
            q *= 2
        curves[n] = curve
        g.close()
    # where the two curves cross: between the last point at which the host loop is the faster one and
    # the next, by linear interpolation of (device - host); the smaller of the sweeps' crossings
    crossings = {}
    for n, curve in curves.items():
        k = max([i for i, (p, th, td) in enumerate(curve) if td > th], default=-1)
        if k < 0:
            crossings[n] = curve[0][0]
        elif k + 1 == len(curve):
            crossings[n] = 2 * curve[k][0]      # never crossed inside the sweep
        else:
            (p0, h0, d0), (p1, h1, d1) = curve[k], curve[k + 1]
            crossings[n] = int(p0 + (p1 - p0) * (d0 - h0) / ((d0 - h0) + (h1 - d1)))
    cross = min(crossings.values())
    print(json.dumps(dict(line="crossover", pairs=cross, default_min_pairs=1 << (max(cross, 1).bit_length() - 1),
                          per_nodes_pairs=crossings,
                          per_nodes={n: [[p, round(1e6 * th, 1), round(1e6 * td, 1)] for p, th, td in c]
                                     for n, c in curves.items()})), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, nargs="+", default=[1000, 20000])
    ap.add_argument("--reps", type=int, default=21, help="timed calls per measurement (3 above 10^7 pairs)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=240.0, help="time limit of the GPU step (s)")
    ap.add_argument("--step", choices=["gpu"], help=argparse.SUPPRESS)   # child mode
    args = ap.parse_args()
    if args.step:
        gpu_step(args)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "gpu", "--nodes", *[str(n) for n in args.nodes],
           "--reps", str(args.reps), "--warmup", str(args.warmup)]
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
