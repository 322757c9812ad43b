"""CPU helpers for the pose-graph conjugate-gradient tests (test
infrastructure only): the linear system of one Levenberg-Marquardt step as
lm_oracle.optimize forms it (C/mapping/pose_graph_optimizer_lm.cpp:68-172), its
3x3 blocks in the layout lgs_pg_cg_solve takes, and Eigen's Jacobi-
preconditioned CG recurrence (Eigen/src/IterativeLinearSolvers/
ConjugateGradient.h) with a tolerance and an iteration cap.
"""
import numpy as np

import lm_oracle as lo


def linearise(poses, edges, lam=1e-4, loss_kind=0, scale=1.0):
    """(H [3n, 3n], b [3n]) of OptimizeStep at `poses`: the edges' blocks, the
    1e9 anchor of node 0 and lam on the diagonal; the step solves H d = -b"""
    _, weight = lo.loss_fn(loss_kind, scale)
    P = np.array(poses, dtype=np.float64)
    n = len(P)
    H = np.zeros((3 * n, 3 * n))
    b = np.zeros(3 * n)
    for s, e, z, info in edges:
        info = np.asarray(info, dtype=np.float64)
        sp, ep = P[s], P[e]
        dx, dy = ep[0] - sp[0], ep[1] - sp[1]
        st, ct = lo.sincos(sp[2])
        Js = np.array([[-ct, -st, -st * dx + ct * dy], [st, -ct, -ct * dx - st * dy], [0.0, 0.0, -1.0]])
        Je = np.array([[ct, st, 0.0], [-st, ct, 0.0], [0.0, 0.0, 1.0]])
        ev = lo.error(sp, ep, z)
        W = weight(float(ev @ info @ ev)) * info
        JsW, JeW = Js.T @ W, Je.T @ W
        H[3 * s:3 * s + 3, 3 * s:3 * s + 3] += JsW @ Js
        H[3 * e:3 * e + 3, 3 * e:3 * e + 3] += JeW @ Je
        H[3 * s:3 * s + 3, 3 * e:3 * e + 3] += JsW @ Je
        H[3 * e:3 * e + 3, 3 * s:3 * s + 3] += (JsW @ Je).T
        b[3 * s:3 * s + 3] += JsW @ ev
        b[3 * e:3 * e + 3] += JeW @ ev
    for i in range(3):
        H[i, i] += 1e9
    H[np.diag_indices(3 * n)] += lam
    return H, b


def blocks(H, edges):
    """(diag [n, 3, 3], pairs [p, 2] int32, off [p, 3, 3]) of H: one pair
    (a, b), a < b, per connected node pair, in the order the edges first name
    it; off[p] is the block at (row a, column b)"""
    n = H.shape[0] // 3
    diag = np.stack([H[3 * v:3 * v + 3, 3 * v:3 * v + 3] for v in range(n)]) if n else np.zeros((0, 3, 3))
    seen, pairs = set(), []
    for s, e, _, _ in edges:
        a, b = min(s, e), max(s, e)
        if a != b and (a, b) not in seen:
            seen.add((a, b))
            pairs.append((a, b))
    off = np.stack([H[3 * a:3 * a + 3, 3 * b:3 * b + 3] for a, b in pairs]) if pairs else np.zeros((0, 3, 3))
    return np.ascontiguousarray(diag), np.array(pairs, dtype=np.int32).reshape(-1, 2), np.ascontiguousarray(off)


def cg(A, b, tol=0.0, max_iterations=0):
    """Eigen's recurrence -> (x, passes run, last |r|^2).  tol 0: machine
    epsilon, max_iterations 0: 2 * len(b).  A pass that ends the loop by the
    residual test counts (Eigen's own counter leaves it out)."""
    n = len(b)
    x = np.zeros(n)
    d = np.diag(A)
    inv = np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 1.0)
    tol = tol or np.finfo(float).eps
    cap = max_iterations or 2 * n
    rhs2 = b @ b
    if rhs2 == 0.0:
        return x, 0, 0.0
    thr = max(tol * tol * rhs2, np.finfo(float).tiny)
    r = b.copy()
    r2 = r @ r
    if r2 < thr:
        return x, 0, r2
    p = inv * r
    abs_new = r @ p
    passes = 0
    for _ in range(cap):
        t = A @ p
        alpha = abs_new / (p @ t)
        x += alpha * p
        r -= alpha * t
        r2 = r @ r
        passes += 1
        if r2 < thr:
            break
        z = inv * r
        abs_old, abs_new = abs_new, r @ z
        p = z + (abs_new / abs_old) * p
    return x, passes, r2


def hub_graph(n, hub, rng):
    """an odometry chain of n nodes plus a loop edge from `hub` to every node
    that is not its chain neighbour: the hub's block row holds n - 1 neighbours"""
    init, edges = lo.random_graph(n, 0, rng)
    info = np.diag([100.0, 100.0, 400.0])
    for j in range(n):
        if abs(j - hub) > 1:
            z = lo.error(init[hub], init[j], (0.0, 0.0, 0.0)) + rng.normal(0.0, [0.01, 0.01, 0.005])
            edges.append((hub, j, tuple(z), info))
    return init, edges
