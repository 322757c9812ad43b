"""CPU-side checks of the grid-search matcher's host parts: lgs_gs_steps (the
window values of one axis) reproduces the reference's literal
`for (double d = -r; d <= r; d += s)` loop
(C/mapping/scan_matcher_grid_search.cpp:72-74) value for value, is exported,
and needs no device."""
import ctypes as C
import math

import numpy as np
import pytest

from lgs_amd import abi

LGS_ERR_INVALID_ARG = 1

# (range, step, values the loop produces, round(range / step) + 1)
TABLE = [(2.0, 0.05, 40, 41), (0.5, 0.005, 100, 101), (0.6, 0.1, 6, 7), (0.3, 0.05, 6, 7), (0.4, 0.05, 9, 9),
         (0.3, 0.03, 11, 11)]


def literal_loop(rng, step):
    r = rng / 2.0
    out = []
    d = -r
    while d <= r:
        out.append(d)
        d += step
    return out


def test_exported_without_a_device():
    lib = C.CDLL(abi.LIB_PATH)
    assert hasattr(lib, "lgs_gs_steps")
    assert "lgs_gs_steps" in abi.SYMBOLS
    # host only: no context argument, and it answers without a GPU
    assert abi.load().lgs_gs_steps(0.4, 0.05, None, 0) == 9


@pytest.mark.parametrize("rng,step,count,naive", TABLE)
def test_steps_are_the_literal_loop(rng, step, count, naive):
    ref = literal_loop(rng, step)
    assert len(ref) == count                      # the issue's table
    assert round(rng / step) + 1 == naive
    got = abi.gs_steps(rng, step)
    assert len(got) == count
    assert got.tobytes() == np.array(ref).tobytes()   # value for value, bit for bit


def test_accumulated_values_are_not_the_lattice():
    """the loop's values differ from -r + k * s in the last bits: what makes
    the literal loop part of the contract"""
    got = abi.gs_steps(0.6, 0.1)
    lattice = np.array([-0.3 + k * 0.1 for k in range(len(got))])
    assert got.tobytes() != lattice.tobytes()


def test_cap_limits_what_is_written():
    lib = abi.load()
    buf = np.full(8, 7.0)
    n = lib.lgs_gs_steps(2.0, 0.05, abi.dptr(buf), 3)
    assert n == 40
    assert list(buf[:3]) == literal_loop(2.0, 0.05)[:3] and list(buf[3:]) == [7.0] * 5


def test_zero_range_is_one_value():
    assert list(abi.gs_steps(0.0, 0.05)) == [-0.0]


@pytest.mark.parametrize("rng,step", [(1.0, 0.0), (1.0, -0.1), (1.0, math.nan), (1.0, math.inf), (-0.5, 0.1),
                                      (math.nan, 0.1), (math.inf, 0.1), (1.0, 1e-9)])
def test_bad_arguments_return_the_negated_code(rng, step):
    """(1.0, 1e-9): half a billion values, beyond the 4096-per-axis cap"""
    assert abi.load().lgs_gs_steps(rng, step, None, 0) == -LGS_ERR_INVALID_ARG
    with pytest.raises(abi.LgsError):
        abi.gs_steps(rng, step)


def test_null_arguments_are_rejected():
    lib = abi.load()
    assert lib.lgs_gs_steps(1.0, 0.1, None, 4) == -LGS_ERR_INVALID_ARG
    assert lib.lgs_gs_optimize_pose_query(None, None, None, None, None, abi.Pose2D(), None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_gs_optimize_pose_batch(None, None, None, None, None, None, 0, 0.5, None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_gs_dense_scores(None, None, None, None, abi.Pose2D(), None, 0) == LGS_ERR_INVALID_ARG
    assert lib.lgs_loop_detect_gs(None, None, None, 0.5, None, 0, None, 0, None) == LGS_ERR_INVALID_ARG
