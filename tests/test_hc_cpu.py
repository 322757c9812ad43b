"""CPU-side checks of the hill-climbing matcher's host part: lgs_hc_term_table,
the values the greedy-endpoint cost's exp() term can take
(C/mapping/cost_function_greedy_endpoint.cpp:66-101 with GridMap::SquaredDistance,
H/grid_map/grid_map.hpp:894-902), is exported, needs no device and equals the
reference's arithmetic with this machine's libm byte for byte."""
import ctypes as C
import math

import numpy as np
import pytest

from lgs_amd import abi

LGS_ERR_INVALID_ARG = 1
# the launcher's cost (scale 0.05, stddev 1.0: its arguments land swapped) and the other order
ORDERS = [(0.05, 1.0), (1.0, 0.05)]


def cost_params(K, scale, stddev):
    return abi.CostGEParams(0.01, 20.0, 0.075, 0.1, K, scale, stddev)


def literal_table(K, res, stddev):
    var = stddev * stddev
    sq = []
    for ky in range(-K, K + 1):
        for kx in range(-K, K + 1):
            dX, dY = kx * res, ky * res
            sq.append(dX * dX + dY * dY)
    d = (K + 1) * res
    sq.append(d * d + d * d)
    return sq, [math.exp(-0.5 * s / var) for s in sq]


def test_exported_without_a_device():
    lib = C.CDLL(abi.LIB_PATH)
    assert hasattr(lib, "lgs_hc_term_table")
    for name in ("lgs_hc_term_table", "lgs_hc_optimize_pose_query", "lgs_hc_optimize_pose_batch", "lgs_hc_trace",
                 "lgs_cost_ge_exact"):
        assert name in abi.SYMBOLS
    # host only: no context argument, and it answers without a GPU
    assert abi.load().lgs_hc_term_table(C.byref(cost_params(1, 0.05, 1.0)), 0.05, None, None, 0) == 10


@pytest.mark.parametrize("scale,stddev", ORDERS)
@pytest.mark.parametrize("res", [0.05, 0.1])
@pytest.mark.parametrize("K", [0, 1, 2])
def test_table_is_the_reference_arithmetic(K, res, scale, stddev):
    sq, term = abi.hc_term_table(cost_params(K, scale, stddev), res)
    rsq, rterm = literal_table(K, res, stddev)
    assert len(sq) == len(term) == (2 * K + 1) ** 2 + 1
    assert sq.tobytes() == np.array(rsq).tobytes()
    assert term.tobytes() == np.array(rterm).tobytes()
    # the last entry is the start value SquaredDistance(0, 0, K + 1, K + 1)
    d = (K + 1) * res
    assert sq[-1] == d * d + d * d and term[-1] == math.exp(-0.5 * (d * d + d * d) / (stddev * stddev))
    # the centre offset is distance 0, term 1
    assert sq[K * (2 * K + 1) + K] == 0.0 and term[K * (2 * K + 1) + K] == 1.0


def test_cap_limits_what_is_written():
    lib = abi.load()
    sq, term = np.full(12, 7.0), np.full(12, 9.0)
    n = lib.lgs_hc_term_table(C.byref(cost_params(1, 0.05, 1.0)), 0.05, abi.dptr(sq), abi.dptr(term), 3)
    assert n == 10
    rsq, rterm = literal_table(1, 0.05, 1.0)
    assert list(sq[:3]) == rsq[:3] and list(sq[3:]) == [7.0] * 9
    assert list(term[:3]) == rterm[:3] and list(term[3:]) == [9.0] * 9


def test_largest_kernel():
    sq, term = abi.hc_term_table(cost_params(16, 0.05, 1.0), 0.05)
    assert len(sq) == 33 * 33 + 1


@pytest.mark.parametrize("K,res,stddev", [(-1, 0.05, 1.0), (17, 0.05, 1.0), (1, 0.0, 1.0), (1, -0.05, 1.0),
                                          (1, math.nan, 1.0), (1, math.inf, 1.0), (1, 0.05, 0.0), (1, 0.05, -1.0),
                                          (1, 0.05, math.nan), (1, 0.05, math.inf)])
def test_bad_arguments_return_the_negated_code(K, res, stddev):
    assert abi.load().lgs_hc_term_table(C.byref(cost_params(K, 0.05, stddev)), res, None, None, 0) == \
        -LGS_ERR_INVALID_ARG
    with pytest.raises(abi.LgsError):
        abi.hc_term_table(cost_params(K, 0.05, stddev), res)


def test_null_arguments_are_rejected():
    lib = abi.load()
    assert lib.lgs_hc_term_table(None, 0.05, None, None, 0) == -LGS_ERR_INVALID_ARG
    assert lib.lgs_hc_term_table(C.byref(cost_params(1, 0.05, 1.0)), 0.05, None, None, 4) == -LGS_ERR_INVALID_ARG
    assert lib.lgs_hc_optimize_pose_query(None, None, None, None, None, abi.Pose2D(), None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_hc_optimize_pose_batch(None, None, None, None, None, None, 0, None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_hc_trace(None, None, None, None, None, abi.Pose2D(), None, None, 0) == -LGS_ERR_INVALID_ARG
    assert lib.lgs_cost_ge_exact(None, None, None, None, None, 0, None) == LGS_ERR_INVALID_ARG
