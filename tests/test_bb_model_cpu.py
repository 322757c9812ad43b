"""CPU checks of the branch-and-bound tests' own models (bb_oracle.py):
exact_search against the oracle's orc_bb_optimize_pose, and the claim of
csrc/k_bb.hip's header that the device's level-by-level superset covers every
node the reference's search expands.  The GPU tests (test_gpu_bb_edges.py)
compare the device's scored-node counts with superset_model, so the model is
pinned here first.

The argument checks of the BB entry points run behind a context and live in
test_gpu_bb_edges.py; only the null-argument rejections need no device.
"""
import ctypes as C

import numpy as np
import pytest

import bb_oracle as bo
from lgs_amd import abi

LGS_ERR_INVALID_ARG = 1
MX, MY, RES = -1.0, -1.4, 0.05


def tiny_case(seed):
    """40 x 56 cells, 9..33 beams, heights 0..4, thresholds DBL_MIN and 0.3"""
    rng = np.random.default_rng(7000 + seed)
    kind = seed % 3
    if kind == 0:    # sparse occupied cells
        cells = np.where(rng.random((56, 40)) < 0.15, rng.choice([0.45, 0.6, 0.8, 0.999], size=(56, 40)), 0.0)
    elif kind == 1:  # dense noise: many close sums
        cells = rng.choice([0.0, 0.3, 0.5, 0.7, 0.9], size=(56, 40)) * rng.uniform(0.9, 1.0, size=(56, 40))
    else:            # few distinct values: ties between nodes
        cells = rng.choice([0.0, 0.5], size=(56, 40))
    n = int(rng.integers(9, 34))
    ang = -np.pi + np.arange(n) * (2 * np.pi / n)
    r = rng.uniform(0.15, 0.9, size=n)
    init = (rng.uniform(-0.2, 0.2), rng.uniform(-0.3, 0.3), rng.uniform(-3, 3))
    hm = seed % 5
    prm = (hm, float(rng.choice([0.25, 0.4, 0.55])), float(rng.choice([0.2, 0.45])), float(rng.choice([0.0, 0.2, 0.35])),
           20.0, 0.01, 20.0)
    thr = None if (seed // 5) % 2 == 0 else 0.3
    rel = (0.0, 0.0, 0.0) if seed % 2 else (0.1, -0.05, 0.02)
    return dict(cells=cells, mx=MX, my=MY, res=RES, prm=prm, ranges=r, angles=ang, init=init, thr=thr, rel=rel)


@pytest.fixture(scope="module")
def solved():
    out = []
    for seed in range(40):
        kw = tiny_case(seed)
        out.append((kw, bo.oracle_bb(**kw), bo.exact_search(**kw), bo.superset_model(**kw)))
    return out


def test_cases_cover_both_thresholds_and_outcomes(solved):
    assert {kw["prm"][0] for kw, *_ in solved} == {0, 1, 2, 3, 4}
    assert {kw["thr"] for kw, *_ in solved} == {None, 0.3}
    assert {o.pose_found for _, o, _, _ in solved} == {0, 1}
    assert {m.path_ok for *_, m in solved} == {False, True}


def test_exact_search_is_the_oracles_search(solved):
    for k, (kw, ora, es, _) in enumerate(solved):
        assert es.visited == ora.coarse_evals, k
        assert list(es.best) == list(ora.best_win), k
        assert es.score_max == ora.score_max, k
        assert es.found == ora.pose_found, k
        assert list(es.win) == list(ora.win), k


def test_superset_covers_the_search(solved):
    """k_bb.hip's header: every node the search expands is expanded by the
    thr_exp rule (and so by the looser thr0 rule); the counts are the top
    nodes plus 4 per expansion and bound the visited count."""
    strict = 0
    for k, (kw, ora, es, m) in enumerate(solved):
        assert es.expanded <= m.expanded, (k, sorted(es.expanded - m.expanded))
        assert m.expanded <= m.expanded_thr0, k
        assert m.count == m.n_top + 4 * len(m.expanded), k
        assert m.count_thr0 == m.n_top + 4 * len(m.expanded_thr0), k
        assert es.visited == m.n_top + 4 * len(es.expanded), k
        assert es.visited <= m.count <= m.count_thr0, k
        if m.path_ok:
            assert m.thr_exp >= m.thr0 and all(nd in m.expanded for nd in m.path[:-1]), k
        else:
            assert m.thr_exp == m.thr0 and m.count == m.count_thr0, k
        strict += m.count < m.count_thr0
    assert strict > 0   # the two rules differ somewhere, or the second count checks nothing


def test_score_maps_replace_the_pyramid():
    """score_maps: all-zero levels expand nothing, whatever the map holds"""
    kw = tiny_case(1)
    zero = [np.zeros((56, 40)) for _ in range(kw["prm"][0] + 1)]
    m = bo.superset_model(**kw, score_maps=zero)
    assert not m.path_ok and m.count == m.count_thr0 == m.n_top and not m.expanded
    es = bo.exact_search(**kw, score_maps=zero)
    assert es.visited == es.n_top and es.found == 0 and es.best == (0, 0, 0)


def test_bb_null_arguments_are_rejected():
    lib = abi.load()
    assert lib.lgs_grid_precompute_pyramid(None, None, 3, None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_bb_optimize_pose_query(None, None, None, None, None, abi.Pose2D(), None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_bb_optimize_pose_batch(None, None, None, None, None, None, None, 0, 0.5, None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_loop_detect_bb(None, None, None, 0.5, None, 0, None, 0, None) == LGS_ERR_INVALID_ARG
