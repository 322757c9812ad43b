"""The pose-graph solve (lgs_pg_cg_solve, k_pgcg.hip; lgs_pg_lm_optimize,
k_pglm.hip) on the graphs of tests/pg_cases.py: long chains closed by zero or
one loop edge with row counts either side of a workgroup, node labels and edges
in any order and direction, nodes that no edge names, rotated anisotropic
information, poses far from the origin.

Single solves are held to an extended-precision reference (pg_cases.reference)
in the energy norm: the device's error E_dev may be at most 8 times the larger
of E_cg, the error of the fp64 restatement of the same recurrence
(pgcg_oracle.cg) on the same system, and u, the reference's own uncertainty.
Device and restatement run one recurrence and differ in summation order only,
and the accuracy conjugate gradients attain is a property of the system: three
bits separate reordered rounding from a structural error (a wrong or missing
block, a stale search direction), which leaves errors many orders larger.  The
true residual |rhs - H x|^2 is held to the restatement's in the same way, its
floor being the residual of the reference rounded to fp64.  Nothing here is
bounded by a value the device produced.  Every solve runs in both variants, one
workgroup and many.

With the corridor information the recurrence never meets its tolerance and ends
at the cap of 2 n passes with finite numbers, on the host as on the device; at
ratio 100 it ends unconverged.  That is the reference algorithm's behaviour and
is pinned, not repaired.

The losses are the library's kinds 0 (Huber, scale 1) and 1 (Cauchy, scale
0.5), both with IEEE-only weights (pglm_graphs.WEIGHT_EXACT)."""
import numpy as np
import pytest

import pg_cases as pc
from lgs_amd import abi, io
from test_gpu_pgcg import VARIANTS, variant

pytestmark = pytest.mark.gpu

FACTOR = 8.0
EPS2 = np.finfo(float).eps ** 2
LOSSES = [(0, 1.0), (1, 0.5)]
LM = dict(iters=10, tol=1e-6, lam=1e-3)                              # test_gpu_pglm's Optimize settings
TWO_STEPS = dict(iters=2, tol=0.0, lam=1e-4, loss="huber", scale=1.0)  # test_gpu_pgcg.test_at_the_lds_bounds' settings


def _bits(v):
    return np.float64(v).tobytes()


def _solve(c, S, how):
    """(x, passes, |r|^2) of one solve in the given variant; the context's counters follow it"""
    before = c.pg_cg_stats()
    with variant(c, how):
        x, it, res = c.pg_cg_solve(S.diag, S.pairs, S.off, S.rhs)
    after = c.pg_cg_stats()
    assert after["solves"] - before["solves"] == 1
    assert after["iterations"] - before["iterations"] == it
    assert after["grid_solves"] - before["grid_solves"] == (how == "grid")
    return x, it, res


def _figures(name, how, S, x, it, res):
    """E_dev and the true residual of a device result, printed next to the restatement's"""
    E, R = pc.energy_error(S.H, x, S.ref), pc.true_residual2(S.H, x, S.rhs)
    be, br = max(S.E_cg, S.u), max(S.R_cg, S.R_floor)
    print(f"{name} ({how}): {len(S.rhs)} rows, passes {it} (restatement {S.cg_passes}, cap {2 * len(S.rhs)}), "
          f"E_dev {E:.3e}, E_cg {S.E_cg:.3e}, u {S.u:.3e}, ratio {E / be if be else 0.0:.2f}; "
          f"true |r|^2 {R:.3e}, restatement {S.R_cg:.3e}, floor {S.R_floor:.3e}, ratio {R / br if br else 0.0:.2f}; "
          f"reported |r|^2 {res:.3e}")
    return E, R


def _within_the_rule(S, E, R):
    assert E <= FACTOR * max(S.E_cg, S.u)
    assert R <= FACTOR * max(S.R_cg, S.R_floor)


@pytest.mark.parametrize("how", VARIANTS)
@pytest.mark.parametrize("name", pc.CONVERGING)
def test_solve_against_the_reference(ctx, name, how):
    S = pc.system(name)
    x, it, res = _solve(ctx, S, how)
    E, R = _figures(name, how, S, x, it, res)
    assert 0 < it < 2 * len(S.rhs)
    assert res < EPS2 * (S.rhs @ S.rhs)           # ended by the residual test
    _within_the_rule(S, E, R)
    if name == "isolated90":                      # lambda alone on the diagonal, a zero right-hand side
        assert (x.reshape(-1, 3)[list(pc.ISOLATED)] == 0.0).all()
        assert x.reshape(-1, 3)[1:40].any() and x.reshape(-1, 3)[41:89].any()


@pytest.mark.parametrize("how", VARIANTS)
def test_no_edges(ctx, how):
    S = pc.system("no_edges5")
    assert len(S.pairs) == 0 and not S.rhs.any()
    x, it, res = _solve(ctx, S, how)
    assert it == 0 and res == 0.0
    assert x.shape == (15,) and (x == 0.0).all()


@pytest.mark.parametrize("how", VARIANTS)
def test_deterministic(ctx, how):
    """two runs and a second context return the same bytes, with the pair list unsorted"""
    S = pc.system("relabel150")
    a = _solve(ctx, S, how)
    b = _solve(ctx, S, how)
    other = abi.Context(0)
    try:
        c = _solve(other, S, how)
    finally:
        other.close()
    for q in (b, c):
        assert q[0].tobytes() == a[0].tobytes()
        assert q[1] == a[1]
        assert _bits(q[2]) == _bits(a[2])


@pytest.mark.parametrize("how", VARIANTS)
@pytest.mark.parametrize("name", pc.AT_THE_CAP)
def test_unconverged_solve_ends_at_the_cap(ctx, name, how):
    """finite numbers that never meet the tolerance: 2 n passes, counted, a finite result, the context
    usable afterwards.  corridor10 is accurate all the same and falls under the rule of the converging
    cases.  At corridor100 the iterates of two summation orders need not agree digit for digit; asserted is
    what holds for any correct CG and what the restatement satisfies with room
    (tests/test_pg_cases_cpu.py): the error is below the zero start's, |ref|_H, and the residual the
    recurrence reports is the true one within a factor 2."""
    S = pc.system(name)
    rows = len(S.rhs)
    x, it, res = _solve(ctx, S, how)
    E, R = _figures(name, how, S, x, it, res)
    norm = pc.energy_error(S.H, np.zeros(rows), S.ref)
    print(f"{name} ({how}): |ref|_H {norm:.3e}, E_dev / |ref|_H {E / norm:.3e} (restatement {S.E_cg / norm:.3e}), "
          f"reported / true |r|^2 {res / R:.4f} (restatement {S.cg_res / S.R_cg:.4f})")
    assert it == 2 * rows
    assert np.isfinite(x).all() and np.isfinite(res)
    assert res >= EPS2 * (S.rhs @ S.rhs)
    if name == "corridor10":
        assert E <= FACTOR * max(S.E_cg, S.u)
    else:
        assert E < norm
        assert 0.5 * R <= res <= 2.0 * R
    T = pc.system("oneloop85")
    y, it2, res2 = _solve(ctx, T, how)
    assert 0 < it2 < 2 * len(T.rhs) and res2 < EPS2 * (T.rhs @ T.rhs)
    _within_the_rule(T, pc.energy_error(T.H, y, T.ref), pc.true_residual2(T.H, y, T.rhs))


@pytest.mark.parametrize("kind,scale", LOSSES)
@pytest.mark.parametrize("name", pc.NAMES)
def test_linearise_is_the_hosts_byte_for_byte(ctx, name, kind, scale):
    init, edges = pc.case(name)
    diag, pairs, off, rhs = ctx.pg_lm_linearize(init, edges, lam=1e-4, loss=kind, scale=scale)
    hdiag, hpairs, hoff, hrhs = io.linearize(init, edges, lam=1e-4, loss=kind, scale=scale)
    assert pairs.dtype == hpairs.dtype and pairs.tobytes() == hpairs.tobytes()      # first-appearance order
    assert len(pairs) == len(edges)
    assert diag.tobytes() == hdiag.tobytes()
    assert off.tobytes() == hoff.tobytes()
    assert rhs.tobytes() == hrhs.tobytes()
    if name == "no_edges5":
        assert not rhs.any() and diag[1:].tolist() == [(np.eye(3) * 1e-4).tolist()] * 4
    if name == "isolated90":
        assert not rhs.reshape(-1, 3)[list(pc.ISOLATED)].any()
        assert diag[list(pc.ISOLATED)].tolist() == [(np.eye(3) * 1e-4).tolist()] * 2


def _run(c, name, kind, scale, resident):
    """(poses, LM steps, total error, lambda, CG passes) of one Optimize on context c"""
    init, edges = pc.case(name)
    before = c.pg_cg_stats()
    P, it, tot, lam = io.optimize_lm(init, edges, solver=io.LM_CONJUGATE_GRADIENT, loss=kind, scale=scale, ctx=c,
                                     resident=resident, **LM)
    after = c.pg_cg_stats()
    assert after["solves"] - before["solves"] == it
    return P, it, tot, lam, after["iterations"] - before["iterations"]


@pytest.mark.parametrize("how", VARIANTS)
@pytest.mark.parametrize("kind,scale", LOSSES)
@pytest.mark.parametrize("name", pc.OPTIMIZE)
def test_optimize_resident_matches_solve_only(ctx, name, kind, scale, how):
    """the two paths run the same kernels on the same bytes: steps, lambda, CG passes and poses are equal"""
    with variant(ctx, how):
        Q, it2, tot2, lam2, passes2 = _run(ctx, name, kind, scale, False)
        grid_before = ctx.pg_cg_stats()["grid_solves"]
        P, it, tot, lam, passes = _run(ctx, name, kind, scale, True)
    assert ctx.pg_cg_stats()["grid_solves"] - grid_before == (it if how == "grid" else 0)
    print(f"{name}, loss {kind} ({how}): {it} LM steps, {passes} CG passes (solve only {passes2}), total error {tot:.17g} "
          f"(solve only {tot2:.17g}), max pose difference {np.abs(P - Q).max():.3e}")
    assert it == it2 and _bits(lam) == _bits(lam2) and it > 1
    assert passes == passes2
    assert P.tobytes() == Q.tobytes()
    if kind == 0:                 # Huber's Loss is IEEE arithmetic only (pglm_graphs.LOSS_EXACT)
        assert _bits(tot) == _bits(tot2)
    else:
        assert tot == pytest.approx(tot2, rel=1e-9)


_cholesky = {}


def cholesky_steps(name):
    """the host sparse Cholesky's poses after two LM steps, computed once per case"""
    if name not in _cholesky:
        init, edges = pc.case(name)
        Q, it, tot, lam = io.optimize_lm(init, edges, solver=io.LM_SPARSE_CHOLESKY, **TWO_STEPS)
        assert it == 2
        Q.setflags(write=False)
        _cholesky[name] = (Q, tot, lam)
    return _cholesky[name]


@pytest.mark.parametrize("how", VARIANTS)
@pytest.mark.parametrize("name", pc.OPTIMIZE)
def test_two_steps_against_the_host_cholesky(ctx, name, how):
    init, edges = pc.case(name)
    Q, tot2, lam2 = cholesky_steps(name)
    with variant(ctx, how):
        P, it, tot, lam = io.optimize_lm(init, edges, solver=io.LM_CONJUGATE_GRADIENT, ctx=ctx, **TWO_STEPS)
    print(f"{name} ({how}): max pose difference to the host Cholesky {np.abs(P - Q).max():.3e}, total error {tot:.9g} / "
          f"{tot2:.9g}")
    assert it == 2 and _bits(lam) == _bits(lam2)
    assert np.abs(P - Q).max() <= 1e-9
