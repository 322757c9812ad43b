"""The pose graph's Levenberg-Marquardt loop resident on the device
(lgs_pg_lm_optimize, k_pglm.hip; io.optimize_lm(ctx=..., resident=True)).

The linearisation kernel forms every entry of H and b as the sequential sum in
edge order that the host's OptimizeStep forms, in its arithmetic, so the
device's system is compared with lgs_pose_graph_linearize's byte for byte for
every loss whose Weight is IEEE arithmetic only -- all but Welsch, whose exp is
the device's own (DCS is among the exact ones: GCC folds its pow(x, 2.0) to
x * x).  Whole Optimize calls are compared with the path that runs only the
solve on the device (io.optimize_lm(ctx=...)), on the same context and with the
solve variant pinned, so both run the same conjugate-gradient kernels.  The
graphs and seeds are those of tests/test_gpu_pgcg.py."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

import pglm_graphs as pg
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


LGS_ERR_INVALID_ARG, LGS_ERR_INTERNAL = 1, 5
LM = dict(iters=10, tol=1e-6, lam=1e-3)


def _bits(v):
    return np.float64(v).tobytes()


def test_device_sqrt_and_fmod_are_the_hosts(ctx):
    """what the linearisation takes from the device's own library: a byte
    mismatch in H then names its cause"""
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.uniform(0.0, 4.0, 1500), 10.0 ** rng.uniform(-320, 300, 1500),
                         np.array([0.0, 1.0, 2.0, 4.0, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308,
                                   np.inf])])
    dev = ctx.debug_libm(2, xs)
    assert dev.tobytes() == np.sqrt(xs).tobytes()
    two_pi = 2.0 * math.pi
    ys = np.concatenate([rng.uniform(-30.0, 30.0, 2000), rng.uniform(-1e8, 1e8, 1000), 10.0 ** rng.uniform(-300, 300, 500),
                         two_pi * np.arange(-8, 9), np.array([0.0, -0.0, math.pi, -math.pi, 5e-324, 1e300])])
    dev = ctx.debug_libm(3, ys)
    host = np.array([math.fmod(y, two_pi) for y in ys])
    assert dev.tobytes() == host.tobytes()


def _linearise_both(ctx, name, kind, scale, lam=1e-4):
    init, edges = pg.graph(name)
    dev = ctx.pg_lm_linearize(init, edges, lam=lam, loss=kind, scale=scale)
    host = io.linearize(init, edges, lam=lam, loss=kind, scale=scale)
    assert dev[1].tolist() == host[1].tolist()        # the pairs, in first-appearance order
    return dev, host, len(edges)


@pytest.mark.parametrize("name", pg.LINEARISE_GRAPHS)
def test_linearise_is_the_hosts_byte_for_byte(ctx, name):
    (diag, pairs, off, rhs), (hdiag, _, hoff, hrhs), m = _linearise_both(ctx, name, 0, 1.0)
    if name == "n1":
        assert m == 0 and len(pairs) == 0 and not rhs.any()
        assert diag[0].tolist() == (np.eye(3) * (1e9 + 1e-4)).tolist()
    if name == "hub":
        assert np.bincount(pairs.reshape(-1)).max() >= 328     # one thread walks 329 edges
    if name == "dup":
        assert len(pairs) < m
    if name == "n300":
        assert m == 339
    assert diag.tobytes() == hdiag.tobytes()
    assert off.tobytes() == hoff.tobytes()
    assert rhs.tobytes() == hrhs.tobytes()


@pytest.mark.parametrize("kind,scale", pg.LOSSES)
def test_linearise_every_loss(ctx, kind, scale):
    """the 80-node graphs with outliers (weights below 1)"""
    (diag, pairs, off, rhs), (hdiag, _, hoff, hrhs), _ = _linearise_both(ctx, f"loss{kind}", kind, scale)
    if kind in pg.WEIGHT_EXACT:
        assert diag.tobytes() == hdiag.tobytes() and off.tobytes() == hoff.tobytes() and rhs.tobytes() == hrhs.tobytes()
        return
    # Welsch: exp is the device's, a few ulp from glibc's; every entry is a short sum of weighted products
    top = max(np.abs(hdiag[1:]).max(), np.abs(hoff).max())
    d = max(np.abs(diag[1:] - hdiag[1:]).max(), np.abs(off - hoff).max())
    dr = np.abs(rhs - hrhs).max()
    d0 = np.abs(diag[0] - hdiag[0]).max()
    print(f"loss {kind}: max |H - host| {d:.3e} of {top:.3e} ({d / top:.3e} relative), rhs {dr:.3e} of "
          f"{np.abs(hrhs).max():.3e}, node 0's block {d0:.3e}")
    assert d <= 1e-12 * top
    assert dr <= 1e-12 * np.abs(hrhs).max()
    assert d0 <= 1e-12 * np.abs(hdiag[0]).max()


def _case(case):
    if case == "n300":
        return (0, 1.0) + pg.graph("n300")
    kind, scale = pg.LOSSES[int(case[4:])]
    return (kind, scale) + pg.graph(case)


def _run(c, case, resident):
    """(poses, LM steps, total error, lambda, CG passes) of one Optimize on context c"""
    kind, scale, init, edges = _case(case)
    before = c.pg_cg_stats()
    P, it, tot, lam = io.optimize_lm(init, edges, solver=io.LM_CONJUGATE_GRADIENT, loss=kind, scale=scale, ctx=c,
                                     resident=resident, **LM)
    after = c.pg_cg_stats()
    assert after["solves"] - before["solves"] == it
    return P, it, tot, lam, after["iterations"] - before["iterations"]


_solve_only = {}


def solve_only(ctx, case, how):
    """the parent path's result, computed once per case and variant"""
    if (case, how) not in _solve_only:
        with variant(ctx, how):
            r = _run(ctx, case, False)
        r[0].setflags(write=False)
        _solve_only[(case, how)] = r
    return _solve_only[(case, how)]


CASES = [f"loss{k}" for k, _ in pg.LOSSES] + ["n300"]


@pytest.mark.parametrize("how", VARIANTS)
@pytest.mark.parametrize("case", CASES)
def test_optimize_resident_matches_solve_only(ctx, case, how):
    kind = _case(case)[0]
    Q, it2, tot2, lam2, passes2 = solve_only(ctx, case, how)
    grid_before = ctx.pg_cg_stats()["grid_solves"]
    with variant(ctx, how):
        P, it, tot, lam, passes = _run(ctx, case, True)
    assert ctx.pg_cg_stats()["grid_solves"] - grid_before == (it if how == "grid" else 0)
    print(f"{case} ({how}): {it} LM steps, {passes} CG passes (solve only {passes2}), total error {tot:.17g} "
          f"(solve only {tot2:.17g}), max pose difference {np.abs(P - Q).max():.3e}")
    assert it == it2 and _bits(lam) == _bits(lam2) and it > 1
    if kind in pg.WEIGHT_EXACT:
        assert passes == passes2
        assert P.tobytes() == Q.tobytes()
    else:
        assert np.abs(P - Q).max() <= 1e-9
    if kind in pg.LOSS_EXACT:
        assert _bits(tot) == _bits(tot2)
    else:
        assert tot == pytest.approx(tot2, rel=1e-9)


@pytest.fixture(scope="module")
def other():
    c = abi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("kind", [k for k, _ in pg.LOSSES])
def test_deterministic(ctx, other, kind):
    """two runs and two contexts return the same bytes"""
    a = _run(ctx, f"loss{kind}", True)
    for c in (ctx, other):
        b = _run(c, f"loss{kind}", True)
        assert b[0].tobytes() == a[0].tobytes()
        assert b[1] == a[1] and _bits(b[2]) == _bits(a[2]) and _bits(b[3]) == _bits(a[3]) and b[4] == a[4]


def test_one_node(ctx):
    """no edge: a zero right-hand side, no CG pass, the pose as it was"""
    init, edges = pg.graph("n1")
    P, it, tot, lam, passes = ctx.pg_lm_optimize(init, edges, iters=10, tol=1e-6, lam=1e-3, loss=0, scale=1.0)
    Q, it2, tot2, lam2 = io.optimize_lm(init, edges, solver=io.LM_CONJUGATE_GRADIENT, ctx=ctx, **LM)
    assert passes == 0 and tot == 0.0
    assert P.tobytes() == np.asarray(init).tobytes() == Q.tobytes()
    assert it == it2 == 2 and _bits(lam) == _bits(lam2)


def test_at_least_one_step(ctx):
    init, edges = pg.graph("loss0")
    for iters in (1, 0, -3):
        _, it, _, lam, _ = ctx.pg_lm_optimize(init, edges, iters=iters, tol=1e-6, lam=1e-3)
        assert it == 1 and lam == 1e-3


def test_lambda_carries_over(ctx):
    """the damping factor a call leaves is the next call's"""
    init, edges = pg.graph("loss0")
    kw = dict(solver=io.LM_CONJUGATE_GRADIENT, iters=3, tol=0.0, loss="huber", scale=1.0, ctx=ctx)
    P1, _, _, lam1 = io.optimize_lm(init, edges, lam=1e-3, resident=True, **kw)
    P2, _, _, lam2 = io.optimize_lm(P1, edges, lam=lam1, resident=True, **kw)
    Q1, _, _, hlam1 = io.optimize_lm(init, edges, lam=1e-3, **kw)
    Q2, _, _, hlam2 = io.optimize_lm(Q1, edges, lam=hlam1, **kw)
    assert lam1 != 1e-3 and _bits(lam1) == _bits(hlam1) and _bits(lam2) == _bits(hlam2)
    assert P2.tobytes() == Q2.tobytes()


def test_nan_pose_runs_to_the_cap_and_returns(ctx):
    init, edges = pg.graph("n2")
    bad = np.array(init)
    bad[1, 0] = np.nan
    P, it, tot, lam, passes = ctx.pg_lm_optimize(bad, edges, iters=1)      # LGS_OK: check() did not raise
    assert it == 1 and passes == 2 * 3 * 2 == 12
    assert np.isnan(P).any() and np.isnan(tot)
    # the context is usable afterwards
    P, it, tot, lam, passes = ctx.pg_lm_optimize(init, edges, iters=3)
    assert np.isfinite(P).all() and passes > 0


def test_stats(ctx):
    init, edges = pg.graph("loss0")
    b, cb = ctx.pg_lm_stats(), ctx.pg_cg_stats()
    _, it, _, _, passes = ctx.pg_lm_optimize(init, edges, **LM)
    a, ca = ctx.pg_lm_stats(), ctx.pg_cg_stats()
    assert a["optimizes"] - b["optimizes"] == 1
    assert a["pose_uploads"] - b["pose_uploads"] == 1
    assert a["pose_downloads"] - b["pose_downloads"] == 1
    assert a["incidence_builds"] - b["incidence_builds"] == 1
    assert a["steps"] - b["steps"] == it > 1
    assert ca["solves"] - cb["solves"] == it
    assert ca["iterations"] - cb["iterations"] == passes > 0


def _raw(ctx, poses, edges, n=None, m=None, kind=0, lam=1e-3, tol=1e-6, scale=1.0, iters=10):
    """lgs_pg_lm_optimize on the caller's own pose array -> status"""
    prm = abi.PgLmParams(iters, tol, kind, scale)
    earr = abi.pg_edges(edges)
    lam_io, it, tot, passes = C.c_double(lam), C.c_int(), C.c_double(), C.c_longlong()
    return ctx.lib.lgs_pg_lm_optimize(ctx.h, C.byref(prm), C.byref(lam_io), poses.ctypes.data_as(C.POINTER(abi.Pose2D)),
                                      len(poses) if n is None else n, C.cast(earr, C.c_void_p),
                                      len(edges) if m is None else m, C.byref(it), C.byref(tot), C.byref(passes))


def test_invalid_arguments_leave_the_poses(ctx):
    init, edges = pg.graph("loss0")
    poses = np.array(init)
    before_lm, before_cg = ctx.pg_lm_stats(), ctx.pg_cg_stats()
    beyond = list(edges)
    beyond[5] = (5, 80, edges[5][2], edges[5][3])
    negative = list(edges)
    negative[7] = (-1, 8, edges[7][2], edges[7][3])
    for kw in (dict(n=0), dict(n=-2), dict(n=2 ** 27 + 1), dict(m=-1), dict(m=2 ** 27 + 1), dict(edges=beyond),
               dict(edges=negative), dict(kind=-1), dict(kind=7), dict(lam=float("nan")), dict(lam=float("inf")),
               dict(tol=float("nan")), dict(scale=float("inf"))):
        args = dict(edges=edges)
        args.update(kw)
        assert _raw(ctx, poses, **args) == LGS_ERR_INVALID_ARG, kw
        assert poses.tobytes() == np.asarray(init).tobytes(), kw
    # before any device work: nothing was counted
    assert ctx.pg_lm_stats() == before_lm and ctx.pg_cg_stats() == before_cg
    with pytest.raises(RuntimeError, match="status 1"):      # no host fallback
        io.optimize_lm(init, edges, solver=io.LM_SPARSE_CHOLESKY, ctx=ctx, resident=True)


def test_angle_outside_the_sincos_domain(ctx):
    """a start node's angle beyond the restated sincos's range: LGS_ERR_INTERNAL, the poses as they were"""
    init, edges = pg.graph("loss0")
    poses = np.array(init)
    poses[3, 2] = 2.0e8
    keep = poses.copy()
    done = ctx.pg_lm_stats()["optimizes"]
    assert _raw(ctx, poses, edges) == LGS_ERR_INTERNAL
    assert poses.tobytes() == keep.tobytes()
    assert ctx.pg_lm_stats()["optimizes"] == done
    with pytest.raises(abi.LgsError, match="status 5"):
        ctx.pg_lm_linearize(keep, edges)
    # the context is usable afterwards
    assert _raw(ctx, np.array(init), edges) == 0
