"""Pose graphs shared by the pose-graph solve's CPU and GPU tests
(tests/test_pg_cases_cpu.py, tests/test_gpu_pg_cases.py): the shapes a SLAM run
produces and lm_oracle.random_graph's closed ellipse does not -- long chains
closed by zero or one loop edge, node labels and edges in any order and
direction, nodes that no edge names, rotated anisotropic information, poses
far from the origin -- and an extended-precision reference for the linear
system of one Levenberg-Marquardt step.  Test infrastructure only; CPU only;
every case is built from fixed seeds.

Each case is (initial poses [n, 3], edges [(start, end, z, info)]) in the form
lm_oracle uses.  Every z comes from lm_oracle.random_graph or, for a reversed
edge, from lm_oracle.error, so it is consistent with its edge's direction."""
import functools
from collections import namedtuple

import numpy as np

import lm_oracle as lo
import pgcg_oracle as po

# The reference is only as good as its residuals: np.longdouble has to be the 80-bit x87 type (64-bit
# significand).  Where it is plain fp64 the module refuses to load; it never falls back.
assert np.finfo(np.longdouble).eps < 2e-19, (
    f"np.longdouble is not an extended-precision type here (eps {np.finfo(np.longdouble).eps}): "
    "pg_cases.reference needs the 80-bit x87 format and does not fall back to fp64")

LD = np.longdouble
ZERO = (0.0, 0.0, 0.0)

CONVERGING = ["chain200", "oneloop85", "oneloop86", "oneloop341", "oneloop342", "relabel150", "isolated90", "far"]
AT_THE_CAP = ["corridor10", "corridor100"]
NAMES = CONVERGING + ["no_edges5"] + AT_THE_CAP
OPTIMIZE = ["chain200", "relabel150", "isolated90", "far", "oneloop342"]    # the whole-Optimize cases
ISOLATED = (40, 89)                             # isolated90: the nodes whose edges are removed
FAR_SHIFT = (1.0e4, -2.0e4, 40.0 * np.pi)       # far: added to every pose of relabel150

# The seed of every case.  Where a seed breaks a condition of tests/test_pg_cases_cpu.py the seed is changed,
# never the condition.  Two are not the first tried: oneloop85's (85 closes the chain over five nodes only
# and the restatement needs 84 % of its cap, too near the 95 % asked for when another BLAS adds the rows
# in another order) and the corridors' (with 126 the restatement would meet corridor10's tolerance at 1.2
# times the cap, with 123 at 1.4 times, so another summation order does not move it inside the cap)
SEEDS = dict(chain200=200, oneloop85=90, oneloop86=86, oneloop341=341, oneloop342=342, relabel150=150,
             isolated90=90, no_edges5=5, corridor=123)


def reversed_z(z):
    """the measurement of the edge end -> start: the inverse of the relative pose z"""
    return tuple(float(v) for v in lo.error(z, ZERO, ZERO))


def _relabel150():
    rng = np.random.default_rng(SEEDS["relabel150"])
    init, edges = lo.random_graph(150, 2, rng)
    perm = rng.permutation(150)                     # chain position -> node label
    poses = np.empty_like(init)
    poses[perm] = init
    edges = [(int(perm[s]), int(perm[e]), z, info) for s, e, z, info in edges]
    edges = [edges[k] for k in rng.permutation(len(edges))]
    out = []
    for k, (s, e, z, info) in enumerate(edges):      # every second edge the other way round, same information
        out.append((e, s, reversed_z(z), info) if k % 2 else (s, e, tuple(float(v) for v in z), info))
    return poses, out, perm


def corridor_information(ratio, a):
    """R(a) diag(100 ratio, 100, 400) R(a)^T with small x-theta and y-theta couplings"""
    s, c = lo.sincos(a)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    info = R @ np.diag([100.0 * ratio, 100.0, 400.0]) @ R.T
    info = 0.5 * (info + info.T)
    info[0, 2] = info[2, 0] = 3.0
    info[1, 2] = info[2, 1] = -2.0
    return info


@functools.lru_cache(maxsize=None)
def case(name):
    """(initial poses [n, 3], edges [(start, end, z, info)]); the poses are read-only"""
    if name == "chain200":
        init, edges = lo.random_graph(200, 0, np.random.default_rng(SEEDS[name]))
    elif name.startswith("oneloop"):
        init, edges = lo.random_graph(int(name[7:]), 1, np.random.default_rng(SEEDS[name]))
    elif name == "relabel150":
        init, edges, _ = _relabel150()
    elif name == "far":
        init, edges = case("relabel150")
        init = init + np.array(FAR_SHIFT)
    elif name == "isolated90":
        init, edges = lo.random_graph(90, 3, np.random.default_rng(SEEDS[name]))
        edges = [g for g in edges if g[0] not in ISOLATED and g[1] not in ISOLATED]
    elif name == "no_edges5":
        init, edges = lo.random_graph(5, 0, np.random.default_rng(SEEDS[name]))[0], []
    elif name.startswith("corridor"):
        rng = np.random.default_rng(SEEDS["corridor"])
        init, edges = lo.random_graph(120, 2, rng)
        ratio = float(name[8:])
        edges = [(s, e, z, corridor_information(ratio, a)) for (s, e, z, _), a in
                 zip(edges, rng.uniform(0.0, np.pi, len(edges)))]
    else:
        raise KeyError(name)
    init = np.array(init, dtype=np.float64)
    init.setflags(write=False)
    return init, list(edges)


def chain_position_of_node0():
    """relabel150 / far: where along the odometry chain (0 .. 149) the anchored node 0 lies"""
    return int(np.flatnonzero(_relabel150()[2] == 0)[0])


def edgeless_nodes(n, edges):
    named = {v for g in edges for v in g[:2]}
    return [v for v in range(n) if v not in named]


def components(n, edges):
    """the connected components of the graph as sorted lists, by smallest node"""
    root = list(range(n))

    def find(v):
        while root[v] != v:
            root[v] = root[root[v]]
            v = root[v]
        return v

    for s, e, _, _ in edges:
        root[find(s)] = find(e)
    out = {}
    for v in range(n):
        out.setdefault(find(v), []).append(v)
    return sorted(out.values())


# ---- the extended-precision reference ----

REFINEMENT_ROUNDS = 4
CHOLESKY_MAX_ROWS = 400


def _energy(H, d):
    d = np.asarray(d, dtype=LD)
    return float(np.sqrt(max(d @ (np.asarray(H, dtype=LD) @ d), LD(0))))


def energy_error(H, x, ref):
    """sqrt((x - ref)^T H (x - ref)), the sums in np.longdouble"""
    return _energy(H, np.asarray(x, dtype=LD) - np.asarray(ref, dtype=LD))


def true_residual2(H, x, rhs):
    """|rhs - H x|^2, the sums in np.longdouble"""
    r = np.asarray(rhs, dtype=LD) - np.asarray(H, dtype=LD) @ np.asarray(x, dtype=LD)
    return float(r @ r)


def refined_lu(H, rhs, rounds=REFINEMENT_ROUNDS):
    """route (a): fp64 LU, then `rounds` rounds of refinement, each residual formed in np.longdouble
    -> (x in np.longdouble, the last correction)"""
    Hl, bl = np.asarray(H, dtype=LD), np.asarray(rhs, dtype=LD)
    x = np.linalg.solve(H, rhs).astype(LD)
    d = np.zeros(len(rhs))
    for _ in range(rounds):
        d = np.linalg.solve(H, (bl - Hl @ x).astype(np.float64))
        x = x + d
    return x, d


def scaled_cholesky(H, rhs):
    """route (b): a np.longdouble Cholesky of the Jacobi-scaled matrix D H D, D = diag(H)^-1/2"""
    Hl, bl = np.asarray(H, dtype=LD), np.asarray(rhs, dtype=LD)
    n = len(bl)
    s = 1 / np.sqrt(np.diag(Hl))
    A = Hl * s[:, None] * s[None, :]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        assert c[0] > 0, "not positive definite"
        L[j:, j] = c / np.sqrt(c[0])
    y = np.zeros(n, dtype=LD)
    for i in range(n):
        y[i] = (s[i] * bl[i] - L[i, :i] @ y[:i]) / L[i, i]
    w = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        w[i] = (y[i] - L[i + 1:, i] @ w[i + 1:]) / L[i, i]
    return s * w


Reference = namedtuple("Reference", "x u route_b")


def reference(H, rhs):
    """the solution of H x = rhs in np.longdouble with its uncertainty u in the energy norm: route (a) is the
    reference; u is |a - b|_H where route (b) runs (up to 400 rows), else the last refinement correction's norm"""
    x, last = refined_lu(H, rhs)
    if len(rhs) <= CHOLESKY_MAX_ROWS:
        xb = scaled_cholesky(H, rhs)
        return Reference(x, energy_error(H, xb, x), xb)
    return Reference(x, _energy(H, last), None)


System = namedtuple("System", "H rhs diag pairs off ref u cg_x cg_passes cg_res E_cg R_cg R_floor")


@functools.lru_cache(maxsize=None)
def system(name, lam=1e-4):
    """the first LM step of a case, as test_gpu_pgcg.system forms it, with the reference and what the fp64
    restatement po.cg makes of it: its energy-norm error E_cg and true residual R_cg = |rhs - H x|^2.
    R_floor is the true residual of the reference rounded to fp64, which no fp64 vector is expected to
    beat: it plays for the residual the part u plays for the error.  Computed once; read-only."""
    init, edges = case(name)
    H, b = po.linearise(init, edges, lam=lam)
    diag, pairs, off = po.blocks(H, edges)
    rhs = -b
    ref = reference(H, rhs)
    x, passes, res = po.cg(H, rhs)
    out = System(H, rhs, diag, pairs, off, ref.x, ref.u, x, passes, res, energy_error(H, x, ref.x),
                 true_residual2(H, x, rhs), true_residual2(H, ref.x.astype(np.float64), rhs))
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
