"""The pose graphs of tests/pg_cases.py and their extended-precision reference
on their own, without a GPU: every case is what its name says, from fixed
seeds; the reference's two routes agree; the fp64 restatement of Eigen's
conjugate gradients (pgcg_oracle.cg) ends where tests/test_gpu_pg_cases.py
assumes it ends -- by the residual test well inside its cap on the chains, at
the cap on the corridor information; and the host library linearises and
optimises the new cases like the dense restatement.  The pattern builders run
on the same pair and edge lists under the sanitizers in two stand-alone
programs (tests/cpp_pg_cases: pgcg_host_check.cpp and pglm_host_check.cpp, each
compiled in as it stands and extended by the new lists), whose tables
(tests/cpp_pg_cases/pg_case_tables.hpp) are compared with the cases here."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import lm_oracle as lo
import pg_cases as pc
import pglm_graphs as pg
import pgcg_oracle as po
from lgs_amd import io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = os.path.join(ROOT, "tests", "cpp_pg_cases", "pg_case_tables.hpp")
HOST_CHECKS = {"pgcg_cases_check": ("PGCG HOST CHECKS PASSED", "PG CASES PGCG CHECKS PASSED"),
               "pglm_cases_check": ("PGLM HOST CHECKS PASSED", "PG CASES PGLM CHECKS PASSED")}

# name: (nodes, edges, nodes without an edge)
SHAPES = dict(chain200=(200, 199, []), oneloop85=(85, 85, []), oneloop86=(86, 86, []), oneloop341=(341, 341, []),
              oneloop342=(342, 342, []), relabel150=(150, 151, []), isolated90=(90, 89, [40, 89]), far=(150, 151, []),
              no_edges5=(5, 0, [0, 1, 2, 3, 4]), corridor10=(120, 121, []), corridor100=(120, 121, []))
# the node lists of the seeded permutations: sha256 of the int32 (start, end) rows
EDGE_DIGEST = dict(relabel150="ba74a2ca75aa807eaf49a928ecebd5d3037335a1b93eb72210f126cd4e858a29",
                   isolated90="83c6edef8127d6a37d0f9c0e825612074260f36e7c986bb385cffabeeb38a455")


def _index_rows(edges):
    return np.array([(s, e) for s, e, _, _ in edges], dtype=np.int32).reshape(-1, 2)


def test_the_names_are_the_cases():
    assert sorted(SHAPES) == sorted(pc.NAMES)
    assert set(pc.OPTIMIZE) <= set(pc.CONVERGING)


@pytest.mark.parametrize("name", pc.NAMES)
def test_case_is_what_its_name_says(name):
    init, edges = pc.case(name)
    n, m, lonely = SHAPES[name]
    assert init.shape == (n, 3) and len(edges) == m
    assert pc.edgeless_nodes(n, edges) == lonely
    S = pc.system(name)
    assert len(S.rhs) == 3 * n and S.H.shape == (3 * n, 3 * n)
    assert len(S.pairs) == m                      # no pair is named twice in these cases
    assert all(0 <= s < n and 0 <= e < n and s != e for s, e, _, _ in edges)
    for s, e, z, info in edges:
        info = np.asarray(info)
        assert info.shape == (3, 3) and (info == info.T).all() and np.linalg.eigvalsh(info).min() > 0
    comps = pc.components(n, edges)
    if name == "chain200":
        assert [(s, e) for s, e, _, _ in edges] == [(i, i + 1) for i in range(199)]
    if name.startswith("oneloop"):
        assert [(s, e) for s, e, _, _ in edges[:-1]] == [(i, i + 1) for i in range(n - 1)]
        s, e = edges[-1][:2]
        assert s - e > 1
        assert 3 * n in (255, 258, 1023, 1026)
    if name in ("relabel150", "far"):
        at = pc.chain_position_of_node0()
        print(f"{name}: node 0 is position {at} of the chain")
        assert 0 < at < 149                       # the anchor lies inside the chain
        assert sum(1 for g in edges if g[0] == 0 or g[1] == 0) >= 2
        rows = _index_rows(edges)
        assert (np.abs(rows[:, 0] - rows[:, 1]) > 1).sum() > 140          # neighbours far apart
        assert (rows[:, 0] > rows[:, 1]).sum() > 30 and (rows[:, 0] < rows[:, 1]).sum() > 30
        first_as_end = [v for v in range(n) if next(g for g in edges if v in g[:2])[1] == v]
        assert len(first_as_end) > 10             # nodes first named as an edge's end
        assert len(comps) == 1
    if name == "relabel150":
        # every second edge is the reverse of an edge of the unshuffled graph, its z the inverse measurement
        init0, edges0 = lo.random_graph(150, 2, np.random.default_rng(pc.SEEDS[name]))
        perm = np.empty(150, dtype=int)
        for k in range(150):
            perm[k] = int(np.flatnonzero((init == init0[k]).all(axis=1))[0])
        fwd = {(int(perm[s]), int(perm[e])): z for s, e, z, _ in edges0}
        back = 0
        for k, (s, e, z, _) in enumerate(edges):
            if k % 2:
                back += 1
                z0 = fwd[(e, s)]
                assert z == pc.reversed_z(z0)
                assert np.abs(lo.error(_compound(init[e], z0), init[e], z)).max() < 1e-14     # z undoes z0
            else:
                assert tuple(fwd[(s, e)]) == tuple(z)
        assert back == 75
    if name == "far":
        base, base_edges = pc.case("relabel150")
        assert (init == base + np.array(pc.FAR_SHIFT)).all() and np.abs(init[:, :2]).min() > 9.9e3
        assert init[:, 2].min() > 120.0
        assert all(a[:3] == b[:3] and a[3] is b[3] for a, b in zip(edges, base_edges))
    if name == "isolated90":
        assert [len(c) for c in comps] == [88, 1, 1]
        bridges = [(s, e) for s, e, _, _ in edges if (s > 40) != (e > 40)]
        assert len(bridges) == 1                  # what joins the nodes behind node 40 to node 0
        assert not S.rhs.reshape(-1, 3)[list(pc.ISOLATED)].any()
        for v in pc.ISOLATED:
            assert S.diag[v].tolist() == (np.eye(3) * 1e-4).tolist()
    if name == "no_edges5":
        assert not S.rhs.any() and len(comps) == 5
    if name.startswith("corridor"):
        ratio = float(name[8:])
        for _, _, _, info in edges:
            assert info[0, 2] == 3.0 and info[1, 2] == -2.0 and info[2, 2] == 400.0
            w = np.linalg.eigvalsh(info[:2, :2])
            assert w[0] == pytest.approx(100.0, rel=1e-12) and w[1] == pytest.approx(100.0 * ratio, rel=1e-12)
        assert max(abs(info[0, 1]) for _, _, _, info in edges) > 10.0 * ratio      # rotated, not diagonal


def _compound(p, z):
    """the pose that lies at the relative pose z from p"""
    s, c = lo.sincos(p[2])
    return np.array([p[0] + c * z[0] - s * z[1], p[1] + s * z[0] + c * z[1], p[2] + z[2]])


@pytest.mark.parametrize("name", ["relabel150", "isolated90"])
def test_cases_are_deterministic(name):
    """built twice, the same bytes; the integer part (the seeded permutations) is pinned by its digest"""
    a = pc.case.__wrapped__(name)
    b = pc.case.__wrapped__(name)
    assert a[0].tobytes() == b[0].tobytes()
    assert [(s, e, tuple(z), np.asarray(i).tobytes()) for s, e, z, i in a[1]] == \
           [(s, e, tuple(z), np.asarray(i).tobytes()) for s, e, z, i in b[1]]
    assert hashlib.sha256(_index_rows(a[1]).tobytes()).hexdigest() == EDGE_DIGEST[name]


def _table(text, name):
    body = re.search(r"k_" + name + r"_edges\[\]\s*=\s*\{(.*?)\};", text, re.S).group(1)
    return np.array([int(v) for v in re.findall(r"-?\d+", body)], dtype=np.int32).reshape(-1, 2)


def test_host_check_tables_are_the_cases():
    """the edge lists that the sanitizer programs give to the pattern builders"""
    text = open(TABLES).read()
    for name in ("relabel150", "isolated90"):
        assert _table(text, name).tolist() == _index_rows(pc.case(name)[1]).tolist(), name
        n = int(re.search(r"k_" + name + r"_nodes\s*=\s*(\d+)", text).group(1))
        assert n == len(pc.case(name)[0])
    assert int(re.search(r"k_no_edges5_nodes\s*=\s*(\d+)", text).group(1)) == 5


@pytest.mark.parametrize("program", list(HOST_CHECKS))
def test_pattern_builders_under_the_sanitizers(program):
    """the block pattern and the incidence lists of relabel150, isolated90 and no_edges5 against a dense
    matrix and a brute-force scan, compiled with -fsanitize=address,undefined into programs of their own
    (make cpptest); each runs the checks of the program it extends first"""
    path = os.path.join(ROOT, "tests", "cpp_pg_cases", "build", program)
    assert os.path.exists(path), "build first: make -C <repo> all"
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout
    for line in HOST_CHECKS[program]:
        assert line in r.stdout
    for name in ("relabel150", "isolated90", "no_edges5"):
        assert f"[ OK ] {name}:" in r.stdout


@pytest.mark.parametrize("name", pc.NAMES)
def test_reference_routes_agree(name):
    """route (a), refined fp64 LU, against route (b), a longdouble Cholesky of the scaled matrix"""
    S = pc.system(name)
    norm = pc.energy_error(S.H, np.zeros(len(S.rhs)), S.ref)
    if len(S.rhs) > pc.CHOLESKY_MAX_ROWS:
        print(f"{name}: {len(S.rhs)} rows, route (b) not run; last refinement correction u = {S.u:.3e} of |ref|_H {norm:.3e}")
    else:
        xb = pc.reference(S.H, S.rhs).route_b
        print(f"{name}: {len(S.rhs)} rows, |a - b|_H = u = {S.u:.3e} of |ref|_H {norm:.3e}, max|a - b| "
              f"{float(np.abs(xb - S.ref).max(initial=0)):.3e}")
    # either way the reference is far better than what an fp64 solve can reach: eps(fp64) |ref|_H is 2e-15
    assert S.u <= 1e-12 * max(norm, 1.0)
    assert pc.true_residual2(S.H, S.ref, S.rhs) <= (1e-15 ** 2) * max(S.rhs @ S.rhs, 1.0)


@pytest.mark.parametrize("name", pc.NAMES)
def test_restatement_ends_where_the_gpu_tests_assume(name):
    S = pc.system(name)
    cap = 2 * len(S.rhs)
    thr = np.finfo(float).eps ** 2 * (S.rhs @ S.rhs)
    norm = pc.energy_error(S.H, np.zeros(len(S.rhs)), S.ref)
    print(f"{name}: {S.cg_passes} / {cap} passes, |r|^2 {S.cg_res:.3e} (threshold {thr:.3e}), true {S.R_cg:.3e}, "
          f"E_cg {S.E_cg:.3e} of |ref|_H {norm:.3e}, u {S.u:.3e}")
    if name in pc.CONVERGING:
        assert 0 < S.cg_passes <= 0.95 * cap and S.cg_res < thr
    elif name == "no_edges5":
        assert S.cg_passes == 0 and S.cg_res == 0.0 and not S.cg_x.any()
    else:
        assert S.cg_passes == cap and S.cg_res >= thr and np.isfinite(S.cg_x).all()
    if name == "corridor10":          # never meets the tolerance, and has twelve digits all the same
        assert S.E_cg <= 1e-12 * norm
    if name == "corridor100":         # what tests/test_gpu_pg_cases.py asks of the device, with room
        assert S.E_cg < 0.1 * norm
        assert S.cg_res == pytest.approx(S.R_cg, rel=1e-2)


@pytest.mark.parametrize("kind,scale", [(0, 1.0), (1, 0.5)])
@pytest.mark.parametrize("name", pc.NAMES)
def test_host_linearize_matches_dense(name, kind, scale):
    """io.linearize against the dense restatement at the tolerances of tests/test_pglm_cpu.py"""
    init, edges = pc.case(name)
    lam = 1e-4
    diag, pairs, off, rhs = io.linearize(init, edges, lam=lam, loss=kind, scale=scale)
    rdiag, rpairs, roff, rrhs = pg.dense_blocks(init, edges, lam, kind, scale)
    assert pairs.tolist() == rpairs.tolist()      # first-appearance order
    scale_h = max(np.abs(rdiag[1:]).max(initial=0.0), np.abs(roff).max(initial=0.0), lam)
    assert np.abs(diag[1:] - rdiag[1:]).max(initial=0.0) <= 1e-12 * scale_h
    assert np.abs(off - roff).max(initial=0.0) <= 1e-12 * scale_h
    assert np.abs(diag[0] - rdiag[0]).max() <= 1e-12 * np.abs(rdiag[0]).max()
    assert np.abs(rhs - rrhs).max() <= 1e-12 * max(np.abs(rrhs).max(), 1e-300)


TWO_STEPS = dict(iters=2, tol=0.0, lam=1e-4, loss=0, scale=1.0)      # the settings of test_gpu_pgcg.test_at_the_lds_bounds


@pytest.mark.parametrize("name", pc.OPTIMIZE)
def test_host_cholesky_is_the_anchor(name):
    """two LM steps of the host's sparse Cholesky, which tests/test_gpu_pg_cases.py holds the device to,
    against the dense restatement; the host's own conjugate gradients are printed next to it"""
    init, edges = pc.case(name)
    Q, it, tot, lam = io.optimize_lm(init, edges, solver=io.LM_SPARSE_CHOLESKY, **TWO_STEPS)
    R, it_r, tot_r, lam_r = lo.optimize(init, edges, solver=0, iters=2, tol=0.0, lam=1e-4, loss_kind=0, scale=1.0)
    C, it_c, _, lam_c = io.optimize_lm(init, edges, solver=io.LM_CONJUGATE_GRADIENT, **TWO_STEPS)
    print(f"{name}: host Cholesky - dense restatement {np.abs(Q - R).max():.3e}, host CG - host Cholesky "
          f"{np.abs(C - Q).max():.3e}, total error {tot:.9g}")
    assert it == it_r == it_c == 2 and lam == lam_r == lam_c
    assert np.abs(Q - R).max() <= 1e-9
    assert tot == pytest.approx(tot_r, rel=1e-9)
