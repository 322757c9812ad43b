"""The loop detectors' argument contract at the C ABI (csrc/loop_host.hpp and
each detector's own early tests): lgs_loop_detect_rtcsm, its multi-context form
with one context and with two contexts on one device (two candidates, so that
the sharding path's own validation runs), lgs_loop_detect_bb and
lgs_loop_detect_gs, each in its plain form and in its `_cost` form with the
greedy-endpoint, square-error and exact greedy-endpoint kinds.

A refused call returns LGS_ERR_INVALID_ARG and leaves every byte of the result
buffer, filled with 0xAB beforehand, in place; an empty batch returns LGS_OK
and leaves it too; a well-formed batch returns LGS_OK and writes it.  Handles
are null or valid, never invented.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import launcher_cost
from hc_sq_oracle import SQ_RANGE
from lgs_amd import abi
from test_gpu_bb_edges import RES, SCORE_RANGE, draw, mini_map

pytestmark = pytest.mark.gpu
LGS_OK, LGS_ERR_INVALID_ARG = 0, 1

# entry -> (plain symbol, parameter type, matcher parameters, contexts, candidates)
ENTRIES = {
    "rtcsm": ("lgs_loop_detect_rtcsm", abi.RtcsmParams, (5, 0.3, 0.3, 0.1, 20.0), 0, 1),
    "multi1": ("lgs_loop_detect_rtcsm_multi", abi.RtcsmParams, (5, 0.3, 0.3, 0.1, 20.0), 1, 1),
    "multi2": ("lgs_loop_detect_rtcsm_multi", abi.RtcsmParams, (5, 0.3, 0.3, 0.1, 20.0), 2, 2),
    "bb": ("lgs_loop_detect_bb", abi.BBParams, (2, 0.3, 0.3, 0.05, 20.0) + SCORE_RANGE, 0, 1),
    "gs": ("lgs_loop_detect_gs", abi.GSParams, (0.2, 0.2, 0.04, 0.05, 0.05, 0.02) + SCORE_RANGE, 0, 1),
}
FORMS = ("plain", "cost_ge", "cost_sq", "cost_ge_exact")
PATTERN = bytes([0xAB]) * C.sizeof(abi.LoopResult)


@pytest.fixture(scope="module")
def setup(ctx):
    mini = mini_map()
    r, ang, init = draw(mini, np.random.default_rng(1), 17)
    other = abi.Context(0)
    yield dict(ctx=ctx, other=other, init=init, scan=ctx.scan(r, ang),
               grid=ctx.grid_from_array(mini.cells, mini.mx, mini.my, RES))
    other.close()


def spec_of(form):
    if form == "cost_sq":
        return abi.cost_spec(abi.CostSQParams(*SQ_RANGE))
    return abi.cost_spec(launcher_cost(), exact=form == "cost_ge_exact")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_loop_arguments(setup, entry, form):
    symbol, ptype, prm, nctx, n = ENTRIES[entry]
    ctx, g, sc, init = setup["ctx"], setup["grid"], setup["scan"], setup["init"]
    fn = getattr(ctx.lib, symbol + ("" if form == "plain" else "_cost"))
    good_params = ptype(*prm)
    good_cost = launcher_cost() if form == "plain" else spec_of(form)
    head = [ctx.h] if nctx == 0 else [(C.c_void_p * nctx)(*[ctx.h, setup["other"].h][:nctx]), nctx]
    DEFAULT = object()

    def call(thr=0.5, first=0, count=n, nq=1, nc=n, gmap=g.h, null_scan=False, results=True, params=good_params,
             cost=DEFAULT):
        """(status, the result buffer kept its 0xAB bytes)"""
        out = (abi.LoopResult * n).from_buffer_copy(PATTERN * n)
        qs = (abi.LoopQuery * 1)(abi.LoopQuery(gmap, None, abi.Pose2D(0, 0, 0), 0, first, count))
        cs = (abi.LoopCandidate * n)(*[abi.LoopCandidate(sc.h, abi.Pose2D(*init), 1 + k, 0) for k in range(n)])
        if null_scan:
            cs[n - 1].scan = None
        cost = good_cost if cost is DEFAULT else cost
        rc = fn(*head, None if params is None else C.byref(params), None if cost is None else C.byref(cost), thr, qs,
                nq, cs, nc, out if results else None)
        return rc, bytes(out) == PATTERN * n

    bad = (LGS_ERR_INVALID_ARG, True)
    for thr in (0.0, -0.1, 1.0 + 1e-9):
        assert call(thr=thr) == bad, thr
    assert call(first=1) == bad                 # a gap before the first candidate
    assert call(count=0) == bad                 # the query covers none of the candidates
    assert call(count=n + 1) == bad             # past the end
    assert call(gmap=None) == bad               # no map
    assert call(null_scan=True) == bad          # a candidate without a scan
    assert call(results=False) == bad           # candidates but no result buffer
    assert call(nc=-1) == bad
    assert call(nq=-1) == bad
    assert call(params=None) == bad
    if form != "plain":
        assert call(cost=None) == bad           # no spec
        unknown = spec_of(form)
        unknown.kind = 99
        assert call(cost=unknown) == bad
    assert call(nq=0, nc=0) == (LGS_OK, True)   # an empty batch
    assert call() == (LGS_OK, False)            # well formed: the records are written
