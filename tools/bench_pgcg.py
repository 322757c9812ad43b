#!/usr/bin/env python3
"""The pose graph's Levenberg-Marquardt step with its three linear solvers: the
host's conjugate gradients and sparse Cholesky (PoseGraphOptimizerLM as it was)
and the conjugate gradients on the device (lgs_pg_cg_solve, k_pgcg.hip), and
the whole step on the device (lgs_pg_lm_optimize, k_pglm.hip), on
tests/lm_oracle.random_graph at 1000 nodes / 40 loop edges, 5000 / 200 and
20000 / 1000 (Huber loss, lambda 1e-4, the launcher's tolerance-free steps:
every call runs the LM steps it is asked for).

Prints one JSON line per graph size and appends it to --out:
  host_cg_ms_per_step, host_cholesky_ms_per_step, device_cg_ms_per_step
        wall clock of an Optimize of --steps LM steps, per step (linearisation,
        solve, pose update, total error); the device call after a warm-up call
  resident_ms_per_step    the same Optimize with the graph resident on the device
        (lgs_pg_lm_optimize, k_pglm.hip: linearisation, solve, pose update and
        loss on the device), timed in the same run as device_cg_ms_per_step, the
        two calls alternating, the fastest of --repeat each
  resident_abi_ms_per_step   lgs_pg_lm_optimize called on arrays that are already
        flat (no per-call conversion of poses and edges, which both
        io.optimize_lm figures above pay alike)
  device_cg_runs_ms, resident_runs_ms   every timed call, per step (the spread)
  device_cg_remainder_ms, resident_remainder_ms   per step: the step time minus
        cg_passes_per_step x us_per_cg_pass of the variant the library picks
  cg_passes_per_step      CG passes the device solves ran, per LM step
  variant                 which of the two device solves the library picks at
                          this size: one persistent workgroup, or many
                          workgroups with two launches per CG pass ("grid")
  solve.{workgroup,grid}  one lgs_pg_cg_solve call on the first step's system,
                          forced through either variant:
    solve_ms, solve_passes
    one_pass_ms           the same call capped at one pass: what a step pays
                          for the value and right-hand-side upload, the
                          launches, the download and the synchronisation
    us_per_cg_pass        (solve_ms - one_pass_ms) / (solve_passes - 1)
  pose_diff_vs_cholesky   max |pose difference| of the device run against the
                          host Cholesky run after the same steps

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

SIZES = ((1000, 40), (5000, 200), (20000, 1000))
GRID_NODES_DEFAULT = 1280   # LGS_OPT_PGCG_GRID_NODES
LM = dict(tol=0.0, lam=1e-4, loss="huber", scale=1.0)


def first_step_blocks(poses, edges, lam):
    """the blocks of the first LM step's H and its right-hand side, in the
    layout of lgs_pg_cg_solve (tests/pgcg_oracle.linearise without the dense matrix)"""
    import lm_oracle as lo
    _, weight = lo.loss_fn(0, LM["scale"])
    n = len(poses)
    diag = np.zeros((n, 3, 3))
    b = np.zeros(3 * n)
    slot, pairs, off = {}, [], []
    for s, e, z, info in edges:
        info = np.asarray(info, dtype=np.float64)
        sp, ep = poses[s], poses[e]
        dx, dy = ep[0] - sp[0], ep[1] - sp[1]
        st, ct = lo.sincos(sp[2])
        Js = np.array([[-ct, -st, -st * dx + ct * dy], [st, -ct, -ct * dx - st * dy], [0.0, 0.0, -1.0]])
        Je = np.array([[ct, st, 0.0], [-st, ct, 0.0], [0.0, 0.0, 1.0]])
        ev = lo.error(sp, ep, z)
        W = weight(float(ev @ info @ ev)) * info
        JsW, JeW = Js.T @ W, Je.T @ W
        diag[s] += JsW @ Js
        diag[e] += JeW @ Je
        blk = JsW @ Je if s < e else (JsW @ Je).T
        key = (min(s, e), max(s, e))
        if key not in slot:
            slot[key] = len(pairs)
            pairs.append(key)
            off.append(np.zeros((3, 3)))
        off[slot[key]] += blk
        b[3 * s:3 * s + 3] += JsW @ ev
        b[3 * e:3 * e + 3] += JeW @ ev
    diag[0] += 1e9 * np.eye(3)
    diag += lam * np.eye(3)
    return diag, np.array(pairs, dtype=np.int32), np.array(off), -b


def timed(f, repeat):
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = f()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def gpu_step(args):
    import lm_oracle as lo
    from lgs_amd import abi, io
    ctx = abi.Context(0)
    for n, loops in SIZES:
        if n > args.max_nodes:
            continue
        init, edges = lo.random_graph(n, loops, np.random.default_rng(1000 + n), noise=0.01)
        earr = io.edges_array(edges)
        k = args.steps
        opt = lambda solver, steps, c=None: io.optimize_lm(init, earr, solver=solver, iters=steps, ctx=c, **LM)
        host_cg_steps = max(1, min(k, 2 if n >= 5000 else k))
        t_cg, _ = timed(lambda: opt(io.LM_CONJUGATE_GRADIENT, host_cg_steps), 1)
        t_ch, ref = timed(lambda: opt(io.LM_SPARSE_CHOLESKY, k), 2)
        res = lambda steps: io.optimize_lm(init, earr, solver=io.LM_CONJUGATE_GRADIENT, iters=steps, ctx=ctx,
                                           resident=True, **LM)
        opt(io.LM_CONJUGATE_GRADIENT, 1, ctx)   # warm-up: code object, arena, pinned staging
        res(1)
        before = ctx.pg_cg_stats()
        dev_runs, res_runs, abi_runs = [], [], []
        parr = abi.pg_edges(edges)
        for _ in range(args.repeat):             # the two paths alternate
            t, out = timed(lambda: opt(io.LM_CONJUGATE_GRADIENT, k, ctx), 1)
            dev_runs.append(t)
            t, out_res = timed(lambda: res(k), 1)
            res_runs.append(t)
            t, _ = timed(lambda: ctx.pg_lm_optimize(init, parr, iters=k, tol=LM["tol"], lam=LM["lam"], loss=0,
                                                    scale=LM["scale"]), 1)
            abi_runs.append(t)
        t_dev, t_res = min(dev_runs), min(res_runs)
        after = ctx.pg_cg_stats()
        passes_per_step = (after["iterations"] - before["iterations"]) / float(3 * args.repeat * k)
        diag, pairs, off, rhs = first_step_blocks(init, edges, LM["lam"])
        solves = {}
        for how, nodes in (("workgroup", 2 ** 31 - 1), ("grid", 0)):
            ctx.set_option(abi.LGS_OPT_PGCG_GRID_NODES, nodes)
            ctx.pg_cg_solve(diag, pairs, off, rhs, max_iterations=1)
            t_one, _ = timed(lambda: ctx.pg_cg_solve(diag, pairs, off, rhs, max_iterations=1), 5)
            t_full, sol = timed(lambda: ctx.pg_cg_solve(diag, pairs, off, rhs), args.repeat)
            solves[how] = dict(solve_ms=round(1e3 * t_full, 3), solve_passes=int(sol[1]),
                               one_pass_ms=round(1e3 * t_one, 3),
                               us_per_cg_pass=round(1e6 * (t_full - t_one) / max(1, sol[1] - 1), 3))
        ctx.set_option(abi.LGS_OPT_PGCG_GRID_NODES, GRID_NODES_DEFAULT)
        picked = "grid" if n >= GRID_NODES_DEFAULT else "workgroup"
        solve_ms = passes_per_step * solves[picked]["us_per_cg_pass"] * 1e-3
        line = dict(line="pgcg", nodes=n, loop_edges=loops, edges=len(edges), pairs=int(len(pairs)), lm_steps=k,
                    host_cg_ms_per_step=round(1e3 * t_cg / host_cg_steps, 3),
                    host_cholesky_ms_per_step=round(1e3 * t_ch / k, 3),
                    device_cg_ms_per_step=round(1e3 * t_dev / k, 3),
                    resident_ms_per_step=round(1e3 * t_res / k, 3),
                    device_cg_runs_ms=[round(1e3 * t / k, 3) for t in dev_runs],
                    resident_runs_ms=[round(1e3 * t / k, 3) for t in res_runs],
                    device_cg_remainder_ms=round(1e3 * t_dev / k - solve_ms, 3),
                    resident_remainder_ms=round(1e3 * t_res / k - solve_ms, 3),
                    device_over_resident=round(t_dev / t_res, 3),
                    resident_abi_ms_per_step=round(1e3 * min(abi_runs) / k, 3),
                    resident_pose_diff_vs_device=float(np.abs(out_res[0] - out[0]).max()),
                    cg_passes_per_step=round(passes_per_step, 1),
                    host_cg_over_device=round((t_cg / host_cg_steps) / (t_dev / k), 2),
                    host_cholesky_over_device=round((t_ch / k) / (t_dev / k), 3),
                    variant=picked, solve=solves,
                    pose_diff_vs_cholesky=float(np.abs(out[0] - ref[0]).max()))
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3, help="LM steps per Optimize call")
    ap.add_argument("--repeat", type=int, default=3, help="timed device calls (the fastest counts)")
    ap.add_argument("--max-nodes", type=int, default=20000, help="skip larger graphs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pgcg_bench.jsonl"),
                    help="file the JSON lines are appended to ('' for none)")
    ap.add_argument("--timeout", type=float, default=420.0, help="time limit of the GPU step (s)")
    ap.add_argument("--step", choices=["gpu"], help=argparse.SUPPRESS)   # child mode
    args = ap.parse_args()
    if args.step:
        gpu_step(args)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "gpu", "--steps", str(args.steps), "--repeat",
           str(args.repeat), "--max-nodes", str(args.max_nodes), "--out", args.out]
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
