"""The pose graph's conjugate-gradient step on the device (lgs_pg_cg_solve,
k_pgcg.hip) and the optimizer that uses it (lgs_pose_graph_optimize_lm_device):
single solves against a dense solve, the iteration cap and the tolerance,
run-to-run determinism, and whole Optimize calls against the host solvers.
The solve has two variants, one persistent workgroup and many workgroups that
meet at kernel boundaries; LGS_OPT_PGCG_GRID_NODES moves the switch between
them, so the small systems run through both."""
import contextlib
import functools

import numpy as np
import pytest

import lm_oracle as lo
import pgcg_oracle as po
from lgs_amd import abi, io

pytestmark = pytest.mark.gpu

GRID_NODES_DEFAULT = 1280     # LGS_OPT_PGCG_GRID_NODES: from here on a solve runs over many workgroups
VARIANTS = ["workgroup", "grid"]


@contextlib.contextmanager
def variant(c, name):
    """solves on context c in one persistent workgroup, or over many workgroups, whatever the size"""
    c.set_option(abi.LGS_OPT_PGCG_GRID_NODES, 0 if name == "grid" else 2 ** 31 - 1)
    try:
        yield
    finally:
        c.set_option(abi.LGS_OPT_PGCG_GRID_NODES, GRID_NODES_DEFAULT)


LOSSES = [(0, 1.0), (1, 0.5), (2, 2.0), (3, 1.0), (4, 3.0), (5, 2.0), (6, 1.0)]


def _graph(name):
    if name == "n1":
        return np.array([[0.3, -0.2, 0.1]]), []
    if name == "hub":      # node 5 is linked to every other node: a block row of 329 neighbours
        return po.hub_graph(330, 5, np.random.default_rng(21))
    if name == "dup":      # a pair named in both directions and three times over
        init, edges = lo.random_graph(40, 3, np.random.default_rng(22))
        info = np.diag([50.0, 80.0, 200.0])
        z = tuple(lo.error(init[3], init[17], (0.0, 0.0, 0.0)))
        zi = tuple(lo.error(init[17], init[3], (0.0, 0.0, 0.0)))
        return init, edges + [(3, 17, z, info), (17, 3, zi, info), (3, 17, z, 2.0 * info)]
    n = int(name[1:])
    return lo.random_graph(n, max(1, n // 25), np.random.default_rng(20 + n))


@functools.lru_cache(maxsize=None)
def system(name):
    """(H, rhs, diag, pairs, off, dense solution) of the first LM step of a graph"""
    init, edges = _graph(name)
    H, b = po.linearise(init, edges, lam=1e-4)
    diag, pairs, off = po.blocks(H, edges)
    for a in (H, b, diag, pairs, off):
        a.setflags(write=False)
    return H, -b, diag, pairs, off, np.linalg.solve(H, -b)


@pytest.mark.parametrize("how", VARIANTS)
@pytest.mark.parametrize("name", ["n1", "n2", "n67", "n80", "n1100", "hub", "dup"])
def test_solve_matches_dense(ctx, name, how):
    H, rhs, diag, pairs, off, dense = system(name)
    before = ctx.pg_cg_stats()
    with variant(ctx, how):
        x, it, res = ctx.pg_cg_solve(diag, pairs, off, rhs)
    assert ctx.pg_cg_stats()["grid_solves"] - before["grid_solves"] == (how == "grid")
    err = np.abs(x - dense).max()
    print(f"{name} ({how}): {len(rhs)} rows, {len(pairs)} pairs, {it} passes, |r|^2 {res:.3e}, max|x - dense| {err:.3e}")
    if name == "n1":
        assert not rhs.any() and it == 0 and res == 0.0 and not x.any()
    else:
        assert 0 < it <= 2 * len(rhs)
    if name == "hub":
        assert np.bincount(pairs.reshape(-1)).max() >= 300
    assert err <= 1e-9


@pytest.mark.parametrize("how", VARIANTS)
def test_iteration_cap(ctx, how):
    H, rhs, diag, pairs, off, _ = system("n80")
    with variant(ctx, how):
        x, it, res = ctx.pg_cg_solve(diag, pairs, off, rhs, max_iterations=3)
    y, it_py, res_py = po.cg(H, rhs, max_iterations=3)
    assert it == 3 and it_py == 3
    assert np.abs(x - y).max() <= 1e-12
    assert res == pytest.approx(res_py, rel=1e-9)


@pytest.mark.parametrize("how", VARIANTS)
def test_tolerance(ctx, how):
    H, rhs, diag, pairs, off, _ = system("n80")
    with variant(ctx, how):
        _, it_full, _ = ctx.pg_cg_solve(diag, pairs, off, rhs)
        x, it, res = ctx.pg_cg_solve(diag, pairs, off, rhs, tolerance=1e-3)
    _, it_py, _ = po.cg(H, rhs, tol=1e-3)
    print(f"tolerance 1e-3 ({how}): device {it} passes, restatement {it_py}, default tolerance {it_full}")
    assert 0 < it <= it_py + 1
    assert it < it_full
    assert res < 1e-6 * (rhs @ rhs)


@pytest.mark.parametrize("how", VARIANTS)
def test_nan_runs_to_the_cap_and_returns(ctx, how):
    H, rhs, diag, pairs, off, _ = system("n2")
    bad = rhs.copy()
    bad[4] = np.nan
    with variant(ctx, how):
        x, it, res = ctx.pg_cg_solve(diag, pairs, off, bad)     # status LGS_OK: check() did not raise
        assert it == 2 * len(rhs) == 12
        assert np.isnan(res)
        x, it, res = ctx.pg_cg_solve(diag, pairs, off, bad, max_iterations=5)
        assert it == 5
        # the context is usable afterwards
        x, it, _ = ctx.pg_cg_solve(diag, pairs, off, rhs)
        assert np.isfinite(x).all() and it > 0


def test_malformed_arguments(ctx):
    _, rhs, diag, pairs, off, _ = system("n67")
    before = ctx.pg_cg_stats()
    swapped = pairs.copy()
    swapped[3] = swapped[3][::-1]
    beyond = pairs.copy()
    beyond[5, 1] = 67
    negative = pairs.copy()
    negative[0, 0] = -1
    twice = np.concatenate([pairs, pairs[2:3]])
    for kw in (dict(pairs=swapped), dict(pairs=beyond), dict(pairs=negative),
               dict(pairs=twice, off=np.concatenate([off, off[2:3]])), dict(tolerance=-1e-3),
               dict(tolerance=float("nan")), dict(max_iterations=-1)):
        args = dict(diag=diag, pairs=pairs, off=off, rhs=rhs)
        args.update(kw)
        with pytest.raises(abi.LgsError, match="status 1"):
            ctx.pg_cg_solve(**args)
    with pytest.raises(abi.LgsError, match="status 1"):      # num_nodes < 1
        ctx.pg_cg_solve(np.zeros((0, 3, 3)), np.zeros((0, 2), np.int32), np.zeros((0, 3, 3)), np.zeros(0))
    assert ctx.pg_cg_stats()["solves"] == before["solves"]


@pytest.mark.parametrize("how", VARIANTS)
def test_deterministic(ctx, how):
    _, rhs, diag, pairs, off, _ = system("n1100")
    with variant(ctx, how):
        a = ctx.pg_cg_solve(diag, pairs, off, rhs)
        b = ctx.pg_cg_solve(diag, pairs, off, rhs)
    other = abi.Context(0)
    try:
        with variant(other, how):
            c = other.pg_cg_solve(diag, pairs, off, rhs)
    finally:
        other.close()
    for q in (b, c):
        assert q[0].tobytes() == a[0].tobytes()
        assert q[1] == a[1]
        assert np.float64(q[2]).tobytes() == np.float64(a[2]).tobytes()


def _bits(v):
    return np.float64(v).tobytes()


@pytest.mark.parametrize("case", [f"loss{k}" for k, _ in LOSSES] + ["n300"])
def test_optimize_device_matches_host_cg(ctx, case):
    if case == "n300":
        kind, scale = 0, 1.0
        init, edges = lo.random_graph(300, 40, np.random.default_rng(7))
    else:
        kind, scale = LOSSES[int(case[4:])]
        init, edges = lo.random_graph(80, 12, np.random.default_rng(110 + kind), outliers=2)
    kw = dict(solver=io.LM_CONJUGATE_GRADIENT, iters=10, tol=1e-6, lam=1e-3, loss=kind, scale=scale)
    before = ctx.pg_cg_stats()
    P, it, tot, lam = io.optimize_lm(init, edges, ctx=ctx, **kw)
    after = ctx.pg_cg_stats()
    Q, it2, tot2, lam2 = io.optimize_lm(init, edges, **kw)
    print(f"{case}: {it} LM steps, {after['iterations'] - before['iterations']} CG passes, total error {tot:.9g} "
          f"(host {tot2:.9g}), max pose difference {np.abs(P - Q).max():.3e}")
    assert it == it2 and _bits(lam) == _bits(lam2)
    assert tot == pytest.approx(tot2, rel=1e-9)
    assert np.abs(P - Q).max() <= 1e-9
    # one solve per LM step, the block pattern built once per Optimize
    assert after["solves"] - before["solves"] == it
    assert after["patterns"] - before["patterns"] == 1


def test_cholesky_is_the_host_solver(ctx):
    init, edges = lo.random_graph(80, 12, np.random.default_rng(31), outliers=2)
    kw = dict(solver=io.LM_SPARSE_CHOLESKY, iters=10, tol=1e-6, lam=1e-3, loss=1, scale=0.5)
    before = ctx.pg_cg_stats()
    P, it, tot, lam = io.optimize_lm(init, edges, ctx=ctx, **kw)
    Q, it2, tot2, lam2 = io.optimize_lm(init, edges, **kw)
    assert P.tobytes() == Q.tobytes() and it == it2 and _bits(tot) == _bits(tot2) and _bits(lam) == _bits(lam2)
    assert ctx.pg_cg_stats() == before


@functools.lru_cache(maxsize=None)
def cholesky_steps(n, loops, seed):
    """a graph and the host Cholesky's poses after two LM steps on it"""
    init, edges = lo.random_graph(n, loops, np.random.default_rng(seed), noise=0.01)
    earr = io.edges_array(edges)
    kw = dict(iters=2, tol=0.0, lam=1e-4, loss="huber", scale=1.0)
    Q, it, tot, lam = io.optimize_lm(init, earr, solver=io.LM_SPARSE_CHOLESKY, **kw)
    assert it == 2
    Q.setflags(write=False)
    return init, earr, kw, Q, tot, lam


@pytest.mark.parametrize("n,how", [(1297, "workgroup"), (1298, "workgroup"), (6485, "workgroup"), (6486, "workgroup"),
                                   (7000, "default")])
def test_at_the_lds_bounds(ctx, n, how):
    """two LM steps against the host's sparse Cholesky at the sizes where the
    one-workgroup solve changes its layout: up to 1297 nodes all five vectors
    live in LDS, up to 6485 the search direction alone, beyond that every
    vector sits in global memory.  By default graphs of these sizes run over
    many workgroups, so the option pins the variant; 7000 nodes run as the
    library chooses"""
    init, earr, kw, Q, tot2, lam2 = cholesky_steps(n, n // 28, 32)
    before = ctx.pg_cg_stats()
    with variant(ctx, how) if how != "default" else contextlib.nullcontext():
        P, it, tot, lam = io.optimize_lm(init, earr, solver=io.LM_CONJUGATE_GRADIENT, ctx=ctx, **kw)
    print(f"{n} nodes ({how}): max pose difference {np.abs(P - Q).max():.3e}, total error {tot:.9g} / {tot2:.9g}")
    assert ctx.pg_cg_stats()["grid_solves"] - before["grid_solves"] == (2 if how == "default" else 0)
    assert it == 2 and _bits(lam) == _bits(lam2)
    assert np.abs(P - Q).max() <= 1e-9


@pytest.mark.parametrize("n", [GRID_NODES_DEFAULT - 1, GRID_NODES_DEFAULT])
def test_at_the_switch_between_the_variants(ctx, n):
    """the largest graph solved in one workgroup and the smallest solved over
    many, with the library's own choice: two LM steps against the host Cholesky"""
    init, earr, kw, Q, tot2, lam2 = cholesky_steps(n, 80, 34)
    before = ctx.pg_cg_stats()
    P, it, tot, lam = io.optimize_lm(init, earr, solver=io.LM_CONJUGATE_GRADIENT, ctx=ctx, **kw)
    after = ctx.pg_cg_stats()
    print(f"{n} nodes: {after['iterations'] - before['iterations']} CG passes, max pose difference "
          f"{np.abs(P - Q).max():.3e}")
    assert after["grid_solves"] - before["grid_solves"] == (2 if n >= GRID_NODES_DEFAULT else 0)
    assert it == 2 and _bits(lam) == _bits(lam2)
    assert np.abs(P - Q).max() <= 1e-9


def test_lambda_carries_over(ctx):
    """the damping factor a call leaves is the next call's, on the device as on the host"""
    init, edges = lo.random_graph(80, 12, np.random.default_rng(33), outliers=2)
    kw = dict(solver=io.LM_CONJUGATE_GRADIENT, iters=3, tol=0.0, loss="huber", scale=1.0)
    P1, _, _, lam1 = io.optimize_lm(init, edges, lam=1e-3, ctx=ctx, **kw)
    P2, _, _, lam2 = io.optimize_lm(P1, edges, lam=lam1, ctx=ctx, **kw)
    Q1, _, _, hlam1 = io.optimize_lm(init, edges, lam=1e-3, **kw)
    Q2, _, _, hlam2 = io.optimize_lm(Q1, edges, lam=hlam1, **kw)
    assert lam1 != 1e-3 and _bits(lam1) == _bits(hlam1) and _bits(lam2) == _bits(hlam2)
    assert np.abs(P2 - Q2).max() <= 1e-9
