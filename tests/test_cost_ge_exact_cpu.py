"""CPU checks of LGS_COST_GREEDY_ENDPOINT_EXACT (no device): the binding, the
argument checks that run before any device work, and, from the oracle alone,
that the inputs of tests/test_gpu_cost_ge_exact.py can tell an exact cost stage
from an inexact one."""
import ctypes as C
import math

import pytest

import cost_spec_oracle as cso
import ge_exact_oracle as gx
import test_loopbatch_cpu as small
from lgs_amd import abi, scene
from test_gpu_gs import draw
from test_gpu_rtcsm import build_map

LGS_ERR_INVALID_ARG = 1
RT = (5, 0.6, 0.6, 0.4, 20.0)


def test_new_symbols_resolve_and_the_abi_version_stays():
    lib = abi.load()
    for name in ("lgs_cost_ge_exact_batch", "lgs_summaries_apply_cost_ge_exact"):
        assert name in abi.SYMBOLS
        assert getattr(lib, name) is not None, name
    assert lib.lgs_abi_version() == 2
    assert abi.LGS_COST_GREEDY_ENDPOINT_EXACT == 2


def test_kernel_stat_slots():
    assert abi.KERNEL_IDS[:19] == ["k_project", "k_coarse", "k_seed", "k_select", "k_fine", "k_replay", "k_cost",
                                   "k_precompute", "k_linsolve", "k_ray_emit", "k_ray_apply", "k_super",
                                   "k_super_planes", "k_bb_score", "k_bb_expand", "k_coarse_aux", "k_match_small",
                                   "k_gs_score", "k_cost_sq"]   # the existing slots keep their indices
    assert abi.KERNEL_IDS[19] == "k_cost_gx" and len(abi.KERNEL_IDS) == 20


def test_exact_cost_spec():
    ge = abi.CostGEParams(*small.COST)
    spec = abi.cost_spec(ge, exact=True)
    assert spec.kind == abi.LGS_COST_GREEDY_ENDPOINT_EXACT == 2
    assert bytes(spec.ge) == bytes(ge)
    assert C.sizeof(spec) == abi.load().lgs_cost_spec_size()
    # the other kinds are as they were
    assert abi.cost_spec(ge).kind == abi.LGS_COST_GREEDY_ENDPOINT
    assert abi.cost_spec(abi.CostSQParams(0.01, 20.0)).kind == abi.LGS_COST_SQUARE_ERROR
    with pytest.raises(TypeError):
        abi.cost_spec(abi.CostSQParams(0.01, 20.0), exact=True)


@pytest.mark.parametrize("kernel_size,stddev", [(17, 1.0), (-1, 1.0), (1, math.nan), (1, 0.0), (1, -1.0),
                                                (1, math.inf)])
def test_kind_two_caps_are_checked_before_the_context(kernel_size, stddev):
    """the hill-climbing cost's caps, reported for a null context too"""
    lib = abi.load()
    spec = abi.cost_spec(abi.CostGEParams(0.01, 20.0, 0.075, 0.1, kernel_size, 0.05, stddev), exact=True)
    rt, bb, gs = abi.RtcsmParams(*small.PARAMS), abi.BBParams(4, 1.0, 1.0, 0.6, 20.0, 0.01, 20.0), \
        abi.GSParams(0.6, 0.4, 0.1, 0.05, 0.05, 0.01, 0.01, 20.0)
    assert lib.lgs_loop_detect_rtcsm_cost(None, C.byref(rt), C.byref(spec), 0.6, None, 0, None, 0, None) == \
        LGS_ERR_INVALID_ARG
    assert lib.lgs_loop_detect_bb_cost(None, C.byref(bb), C.byref(spec), 0.6, None, 0, None, 0, None) == \
        LGS_ERR_INVALID_ARG
    assert lib.lgs_loop_detect_gs_cost(None, C.byref(gs), C.byref(spec), 0.6, None, 0, None, 0, None) == \
        LGS_ERR_INVALID_ARG
    assert lib.lgs_rtcsm_optimize_pose_query_cost(None, None, C.byref(rt), C.byref(spec), None, abi.Pose2D(),
                                                  None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_bb_optimize_pose_query_cost(None, None, C.byref(bb), C.byref(spec), None, abi.Pose2D(),
                                               None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_gs_optimize_pose_query_cost(None, None, C.byref(gs), C.byref(spec), None, abi.Pose2D(),
                                               None) == LGS_ERR_INVALID_ARG


def test_unknown_kind_is_still_rejected_and_null_arguments_too():
    lib = abi.load()
    spec = abi.CostSpec(3, abi.CostGEParams(*small.COST), abi.CostSQParams(0.01, 20.0))
    assert lib.lgs_loop_detect_rtcsm_cost(None, C.byref(abi.RtcsmParams(*small.PARAMS)), C.byref(spec), 0.6, None, 0,
                                          None, 0, None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_cost_ge_exact_batch(None, None, None, None, None, 0, None, None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_summaries_apply_cost_ge_exact(None, None, None, None, None, 0) == LGS_ERR_INVALID_ARG


# ---- the GPU tests' inputs are not vacuous (the oracle alone) ----
@pytest.fixture(scope="module")
def case(world):
    """the map and the scan test_gpu_cost_ge_exact.py matches, and the oracle's best sensor pose"""
    map3 = build_map(world, 300, gx.RES, 100, scene.arc_poses(24), n_beams=1081)
    r, ang, init = draw(world, 1, 361)
    ref = cso.ref_rtcsm(map3, gx.RES, RT, r, ang, init, rel=gx.REL)
    return map3, r, ang, ref


def test_beams_select_several_table_entries(case):
    map3, r, ang, ref = case
    terms = gx.beam_terms(map3, gx.RES, r, ang, gx.REL, ref.best)
    _, table = abi.hc_term_table(abi.CostGEParams(*gx.LAUNCHER), gx.RES)
    table = list(table)
    assert set(terms) <= set(table) | {0.0}     # every term is a table entry, or +0 for a filtered beam
    chosen = set(terms) & set(table)
    assert len(chosen) >= 3, chosen
    assert table[-1] in chosen                  # the start value: no occupied / free pair in the window
    assert table[4] == 1.0 and 1.0 in chosen    # the centre offset


def test_seven_costs_differ_and_the_covariance_is_theirs(case):
    map3, r, ang, ref = case
    import oracle_bind as ob
    g, sc = ob.OGrid(*map3, gx.RES), ob.OScan(r, ang, gx.REL, 0.0, 30.0)
    c = [gx.oracle_cost(g, sc, p) for p in gx.seven_poses(ref.best, gx.RES)]
    assert len(set(c)) > 1, c
    assert c[0] / len(r) == ref.s.normalized_cost
    grad = [0.5 * (c[1] - c[2]) / gx.RES, 0.5 * (c[3] - c[4]) / gx.RES, 0.5 * (c[5] - c[6]) / 1e-2]
    cov = [grad[a] * grad[b] for a in range(3) for b in range(3)]
    for k in (0, 4, 8):
        cov[k] += 0.01
    assert cov == list(ref.s.covariance) == gx.oracle_covariance(g, sc, ref.best)
    assert any(v != 0.0 for v in grad)


def test_summation_order_shows(case):
    """the beam-order chain of the terms is the oracle's cost; the exactly rounded sum is not"""
    map3, r, ang, ref = case
    terms = gx.beam_terms(map3, gx.RES, r, ang, gx.REL, ref.best)
    chain = 0.0
    for t in terms:
        chain -= t
    chain *= gx.LAUNCHER[5]
    assert chain / len(r) == ref.s.normalized_cost
    assert -math.fsum(terms) * gx.LAUNCHER[5] != chain
