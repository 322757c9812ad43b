"""CPU-side checks of the CostSquareError entry points (the hill-climbing walk
over the square-error cost, the batched cost and covariance, and the summaries
of the search matchers): exported, bound, and a NULL argument is rejected
before the context is touched, so they answer without a GPU."""
import ctypes as C

from lgs_amd import abi

LGS_ERR_INVALID_ARG = 1
NEW = ("lgs_cost_square_error_batch", "lgs_summaries_apply_cost_sq", "lgs_hc_sq_optimize_pose_query",
       "lgs_hc_sq_optimize_pose_batch", "lgs_hc_sq_trace")


def test_exported_and_bound():
    lib = C.CDLL(abi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in abi.SYMBOLS, name


def test_params_layout():
    assert C.sizeof(abi.CostSQParams) == 16
    p = abi.CostSQParams(0.01, 20.0)
    assert (p.usable_range_min, p.usable_range_max) == (0.01, 20.0)


def test_abi_version_unchanged():
    assert abi.load().lgs_abi_version() == 2


def test_null_arguments_are_rejected_without_a_device():
    lib = abi.load()
    assert lib.lgs_cost_square_error_batch(None, None, None, None, None, 0, None, None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_summaries_apply_cost_sq(None, None, None, None, None, 0) == LGS_ERR_INVALID_ARG
    assert lib.lgs_hc_sq_optimize_pose_query(None, None, None, None, None, abi.Pose2D(), None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_hc_sq_optimize_pose_batch(None, None, None, None, None, None, 0, None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_hc_sq_trace(None, None, None, None, None, abi.Pose2D(), None, None, 0) == -LGS_ERR_INVALID_ARG
    # a cost without a context, and a context-free n > 0 call with null arrays
    cost = abi.CostSQParams(0.01, 20.0)
    assert lib.lgs_cost_square_error_batch(None, None, C.byref(cost), None, None, 1, None, None) == LGS_ERR_INVALID_ARG
    assert lib.lgs_hc_sq_optimize_pose_batch(None, None, C.byref(abi.HCParams(0.1, 0.1, 100, 5)), C.byref(cost),
                                             None, None, 1, None) == LGS_ERR_INVALID_ARG
