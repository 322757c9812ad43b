#!/usr/bin/env python3
"""Grid-search loop detector on the launcher's settings (LoopDetectorGridSearch
of launcher_settings_default.json: a 2.0 x 2.0 m x 0.5 rad window at
0.05 / 0.05 / 0.005 steps = 40 x 40 x 100 poses, threshold 0.5) on a 600 x 600
local map with 1081-beam candidates.

Prints one JSON line per measurement:
  gs      lgs_loop_detect_gs: candidates/s, k_gs_score's time per launch, its
          algorithmic bytes (8 B x poses x valid beams) and their rate as a
          fraction of the 8 TB/s HBM basis and of the measured L2-gather range
          (16.8-18.8 TB/s)
  bb      lgs_loop_detect_bb on the same candidates and window (what a user of
          this library had before)
  cpu     one candidate, one Python loop over the oracle's
          orc_pixel_accurate_score (the reference's own triple loop)

Every GPU measurement runs in a child process of its own under a time limit;
a child that fails or times out ends the run.
"""
import argparse
import ctypes as C
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

WINDOW = (2.0, 2.0, 0.5, 0.05, 0.05, 0.005)
SCORE_RANGE = (0.01, 20.0)
COST = (0.01, 20.0, 0.075, 0.1, 1, 0.05, 1.0)
THRESHOLD = 0.5
HBM_TBS = 8.0
L2_GATHER_TBS = (16.8, 18.8)


def scene_inputs(n_cand, n_beams=1081, cells=600):
    import oracle_bind as ob
    from lgs_amd import scene
    world = scene.make_world()
    ang = scene.beam_angles(n_beams)
    m = ob.OMap(0.05, 100, cells, cells)
    bp = ob.BuilderParams(0.01, 20.0, 0.6, 0.45)
    for p in scene.arc_poses(10):
        m.integrate(p, ob.OScan(scene.ray_cast(world, p, ang), ang), bp)
    rng = np.random.default_rng(5)
    cands = []
    for _ in range(n_cand):
        true = (rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-3, 3))
        init = (true[0] + rng.uniform(-0.5, 0.5), true[1] + rng.uniform(-0.5, 0.5), true[2] + rng.uniform(-0.1, 0.1))
        cands.append((scene.ray_cast(world, true, ang), init))
    return m.cells(), m.m.min_x, m.m.min_y, ang, cands


def valid_beams(r):
    return int(np.sum((np.asarray(r) < min(SCORE_RANGE[1], 30.0)) & (np.asarray(r) > max(SCORE_RANGE[0], 0.0))))


def gpu_step(which, args):
    from lgs_amd import abi
    cells, mx, my, ang, cands = scene_inputs(args.candidates)
    ctx = abi.Context(0)
    g = ctx.grid_from_array(cells, mx, my, 0.05)
    cl = [(ctx.scan(r, ang), init, k) for k, (r, init) in enumerate(cands)]
    queries = [(g, None, (0.0, 0.0, 0.0), 0, 0, len(cl))]
    cost = abi.CostGEParams(*COST)
    if which == "gs":
        P = abi.GSParams(*WINDOW, *SCORE_RANGE)
        call = lambda: ctx.loop_detect_gs(P, cost, THRESHOLD, queries, cl)
        kernel = "k_gs_score"
    else:
        P = abi.BBParams(6, WINDOW[0], WINDOW[1], WINDOW[2], 20.0, *SCORE_RANGE)
        call = lambda: ctx.loop_detect_bb(P, cost, THRESHOLD, queries, cl)
        kernel = "k_bb_score"
    for _ in range(args.warmup):
        out = call()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = call()
    ctx.synchronize()
    wall = (time.perf_counter() - t0) / args.steps
    # a profiled pass of its own: the events serialise the stream
    ctx.set_option(abi.LGS_OPT_PROFILE, 1)
    ctx.reset_stats()
    call()
    st = ctx.kernel_stats().get(kernel, dict(launches=0, total_ms=0.0, algo_bytes=0.0))
    ctx.set_option(abi.LGS_OPT_PROFILE, 0)
    line = dict(line=which, candidates=len(cl), beams=len(ang), window=list(WINDOW), threshold=THRESHOLD,
                found=int(sum(o.found for o in list(out)[:len(cl)])), call_ms=round(1e3 * wall, 3),
                candidates_per_s=round(len(cl) / wall, 2), kernel=kernel, launches=int(st["launches"]),
                kernel_ms_per_launch=round(st["total_ms"] / max(1, st["launches"]), 4),
                kernel_ms_per_call=round(st["total_ms"], 4), algo_gb_per_call=round(st["algo_bytes"] / 1e9, 4))
    if which == "gs":
        nx, ny, nt = (len(abi.gs_steps(WINDOW[k], WINDOW[k + 3])) for k in range(3))
        line["poses_per_candidate"] = nx * ny * nt
        line["valid_beams_mean"] = round(float(np.mean([valid_beams(r) for r, _ in cands])), 1)
        tbs = st["algo_bytes"] / 1e12 / max(st["total_ms"] * 1e-3, 1e-12)
        line["algo_tb_per_s"] = round(tbs, 3)
        line["fraction_of_8_tb_s"] = round(tbs / HBM_TBS, 3)
        line["fraction_of_l2_gather"] = [round(tbs / L2_GATHER_TBS[1], 3), round(tbs / L2_GATHER_TBS[0], 3)]
    print(json.dumps(line), flush=True)
    ctx.close()


def cpu_line(args):
    """the reference's loops over the oracle's pinned score, one candidate"""
    import oracle_bind as ob
    cells, mx, my, ang, cands = scene_inputs(1)
    r, init = cands[0]
    L = ob.lib()
    g = ob.OGrid(cells, mx, my, 0.05)
    sc = ob.OScan(r, ang)
    P = ob.BBParams(0, 0, 0, 0, 0, *SCORE_RANGE)

    def steps(rng, step):
        out, d = [], -rng / 2.0
        while d <= rng / 2.0:
            out.append(d)
            d += step
        return out
    xs, ys, ts = (steps(WINDOW[k], WINDOW[k + 3]) for k in range(3))
    best = THRESHOLD * len(r)
    t0 = time.perf_counter()
    for dy in ys:
        for dx in xs:
            for dt in ts:
                s = L.orc_pixel_accurate_score(C.byref(g.g), C.byref(P), C.byref(sc.s),
                                               ob.Pose(init[0] + dx, init[1] + dy, init[2] + dt))
                if s > best:
                    best = s
    wall = time.perf_counter() - t0
    print(json.dumps(dict(line="cpu", candidates=1, poses=len(xs) * len(ys) * len(ts), seconds=round(wall, 3),
                          candidates_per_s=round(1.0 / wall, 4), best_normalized_score=round(best / len(r), 4))),
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=float, default=240.0, help="time limit of each GPU step (s)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--step", choices=["gs", "bb"], help=argparse.SUPPRESS)   # child mode
    args = ap.parse_args()
    if args.step:
        gpu_step(args.step, args)
        return 0
    for which in ("gs", "bb"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", which, "--candidates", str(args.candidates),
               "--steps", str(args.steps), "--warmup", str(args.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(line=which, error="timeout")), flush=True)
            return 124
        if rc != 0:   # nothing more on the GPU after a failed step
            print(json.dumps(dict(line=which, error=f"exit status {rc}")), flush=True)
            return rc if rc > 0 else 1
    if not args.no_cpu:
        cpu_line(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
