"""CPU checks of the `_cost` entry points' binding and of the oracle-side
square-error record composer the GPU tests compare against (no device)."""
import ctypes as C

import numpy as np

import cost_spec_oracle as cso
import test_loopbatch_cpu as small
from loop_oracle import oracle_detect_fn
from lgs_amd import abi, loopbatch

NEW_SYMBOLS = ["lgs_rtcsm_optimize_pose_cost", "lgs_rtcsm_optimize_pose_query_cost",
               "lgs_rtcsm_optimize_pose_query_batch_cost", "lgs_rtcsm_optimize_pose_batch_cost",
               "lgs_bb_optimize_pose_batch_cost", "lgs_bb_optimize_pose_query_cost",
               "lgs_gs_optimize_pose_batch_cost", "lgs_gs_optimize_pose_query_cost",
               "lgs_loop_detect_rtcsm_cost", "lgs_loop_detect_rtcsm_multi_cost", "lgs_loop_detect_bb_cost",
               "lgs_loop_detect_gs_cost", "lgs_cost_spec_size"]


def test_new_symbols_resolve_and_the_abi_version_stays():
    lib = abi.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None, name
    assert lib.lgs_abi_version() == 2


def test_cost_spec_layout():
    lib = abi.load()
    assert C.sizeof(abi.CostSpec) == lib.lgs_cost_spec_size()
    assert abi.CostSpec.ge.offset == 8 and abi.CostSpec.sq.offset == 8 + C.sizeof(abi.CostGEParams)
    assert loopbatch.RECORD_BYTES == 176
    assert abi.KERNEL_IDS[:18] == ["k_project", "k_coarse", "k_seed", "k_select", "k_fine", "k_replay", "k_cost",
                                   "k_precompute", "k_linsolve", "k_ray_emit", "k_ray_apply", "k_super",
                                   "k_super_planes", "k_bb_score", "k_bb_expand", "k_coarse_aux", "k_match_small",
                                   "k_gs_score"]   # the existing slots keep their indices
    assert abi.KERNEL_IDS[18] == "k_cost_sq"


def test_cost_spec_of_either_parameter_type():
    ge, sq = abi.CostGEParams(*small.COST), abi.CostSQParams(0.01, 20.0)
    a, b = abi.cost_spec(ge), abi.cost_spec(sq)
    assert a.kind == abi.LGS_COST_GREEDY_ENDPOINT and bytes(a.ge) == bytes(ge)
    assert b.kind == abi.LGS_COST_SQUARE_ERROR and bytes(b.sq) == bytes(sq)
    assert abi.cost_spec(b) is b


def test_unknown_kind_and_bad_ranges_are_rejected_without_a_device():
    """the selector is checked before the context is touched: a null context still
    reports the bad spec"""
    lib = abi.load()
    for spec in (abi.CostSpec(7, abi.CostGEParams(*small.COST), abi.CostSQParams(0.01, 20.0)),
                 abi.CostSpec(1, abi.CostGEParams(), abi.CostSQParams(float("nan"), 20.0)),
                 abi.CostSpec(1, abi.CostGEParams(), abi.CostSQParams(0.01, float("inf")))):
        rc = lib.lgs_loop_detect_rtcsm_cost(None, C.byref(abi.RtcsmParams(*small.PARAMS)), C.byref(spec), 0.6, None, 0,
                                            None, 0, None)
        assert rc == 1   # LGS_ERR_INVALID_ARG


def test_sq_record_composer_agrees_with_the_loop_oracle_outside_the_cost_bytes():
    maps, cands = small.make_problem()
    ge = loopbatch.run_sharded(cands, oracle_detect_fn(maps, cands, small.PARAMS, small.COST, small.THR))
    sq = loopbatch.run_sharded(cands, cso.oracle_sq_detect_fn("rtcsm", maps, cands, small.PARAMS, small.THR))
    diff = cso.differing_bytes(ge, sq)
    assert diff and diff <= cso.COST_BYTES, sorted(diff - cso.COST_BYTES)
    found = [r.found for r in loopbatch.decode(sq)]
    assert 0 < sum(found) < len(cands)
    # every record, found or not, carries a square-error cost of its own
    costs = [r.normalized_cost for r in loopbatch.decode(sq)]
    assert len(set(costs)) == len(cands) and all(0.0 < c <= 1.0 for c in costs)
    covs = np.array([list(r.covariance) for r in loopbatch.decode(sq)])
    assert (covs[:, [0, 4, 8]] > 0.01).all()
