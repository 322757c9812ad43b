"""The nearest-node loop searcher on the GPU (lgs_loop_graph_*,
lgs_loop_search_nearest, csrc/k_loop_search.hip).  Tolerance:
none -- the device's records and per-map rows equal the host function's
(lgs_loop_search_nearest_host) and the restatement's
(tests/loop_search_oracle.py) byte for byte, whatever the group size, the hint
count, the run or the context.  The group option is set to 64 positions so
that walks of about 300 positions span several groups and, with a map of 100
nodes, a group larger than the option.  The default group size never exceeds
one LDS round (1024 positions) at these sizes -- the 2000-node snapshot runs
in groups of 500 -- so test_groups_above_one_lds_round sets groups of 1100,
1500 and the whole 1975-position walk, with a map across position 1024."""
import numpy as np
import pytest

import loop_search_cases as lc
import loop_search_oracle as orc
from lgs_amd import abi

pytestmark = pytest.mark.gpu

LGS_ERR_INVALID_ARG = 1
CASES = lc.cases()
MAIN = CASES[0]


def params_of(prm):
    return abi.LoopSearchParams(prm.travel_dist_threshold, prm.node_dist_threshold, prm.num_candidate_nodes, 0)


@pytest.fixture(scope="module")
def dctx():
    """a context whose searches always launch, in groups of 64 positions"""
    c = abi.Context(0)
    c.set_option(abi.LGS_OPT_LOOP_SEARCH_MIN_PAIRS, 0)
    c.set_option(abi.LGS_OPT_LOOP_SEARCH_GROUP, 64)
    yield c
    c.close()


@pytest.fixture(scope="module")
def main_reference():
    """the main case's 330 hints through the restatement, once"""
    return orc.search_all(MAIN.poses, MAIN.idx_min, MAIN.idx_max, MAIN.prm, MAIN.hints)


def search_both(ctx, case, hints):
    """device records and table (and the records of a call without the table, which must be the same)"""
    rows = lc.hint_rows(hints, abi.LOOP_HINT_DTYPE)
    g = ctx.loop_graph(case.poses, case.idx_min, case.idx_max)
    try:
        res, tab = g.search(params_of(case.prm), rows, per_map=True)
        only = g.search(params_of(case.prm), rows)
    finally:
        g.close()
    assert only.tobytes() == res.tobytes()
    return res, tab


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_device_equals_host_function_and_restatement(dctx, case):
    before = dctx.loop_search_stats()
    res, tab = search_both(dctx, case, case.hints)
    after = dctx.loop_search_stats()
    assert after["device_calls"] == before["device_calls"] + 2 and after["host_calls"] == before["host_calls"]
    rows = lc.hint_rows(case.hints, abi.LOOP_HINT_DTYPE)
    hres, htab = abi.loop_search_host(case.poses, case.idx_min, case.idx_max, params_of(case.prm), rows, per_map=True)
    ores, otab = orc.search_all(case.poses, case.idx_min, case.idx_max, case.prm, case.hints)
    assert res.tobytes() == hres.tobytes() == ores.tobytes()
    assert tab.tobytes() == htab.tobytes() == otab.tobytes()


def test_graph_info_and_travel(dctx):
    g = dctx.loop_graph(MAIN.poses, MAIN.idx_min, MAIN.idx_max)
    travel = orc.travel_chain(MAIN.poses, MAIN.idx_min, MAIN.idx_max)
    info = g.info()
    assert (info.n, info.m, info.positions) == (330, 12, 330 - 42) and info.walk_travel.hex() == travel[-1].hex()
    assert g.travel().tobytes() == np.array(travel).tobytes()
    g.close()
    one = dctx.loop_graph(MAIN.poses, [0], [329])
    assert one.info() == (330, 1, 0, 0.0) and len(one.travel()) == 0
    one.close()


@pytest.mark.parametrize("q", [1, 63, 64, 65, 257])
def test_hint_counts_around_a_wave_and_a_tile(dctx, main_reference, q):
    """1, one below / at / above a wave, one past the 256-hint workgroup tile; hints taken from all over the
    trajectory so that the cuts inside a tile differ"""
    pick = [(37 * j + 5 * q) % len(MAIN.hints) for j in range(q)]
    res, tab = search_both(dctx, MAIN, [MAIN.hints[j] for j in pick])
    ores, otab = main_reference
    assert res.tobytes() == ores[pick].tobytes()
    assert tab.tobytes() == np.ascontiguousarray(otab[pick]).tobytes()
    rows = lc.hint_rows([MAIN.hints[j] for j in pick], abi.LOOP_HINT_DTYPE)
    hres = abi.loop_search_host(MAIN.poses, MAIN.idx_min, MAIN.idx_max, params_of(MAIN.prm), rows)
    assert res.tobytes() == hres.tobytes()


def test_group_size_64_default_and_one_group_give_identical_bytes(main_reference):
    ctx = abi.Context(0)
    ctx.set_option(abi.LGS_OPT_LOOP_SEARCH_MIN_PAIRS, 0)
    out = {}
    for group in (64, 0, 1, 100, 2 ** 27):      # 0: the default; 1: one map per group; 2^27: one group
        ctx.set_option(abi.LGS_OPT_LOOP_SEARCH_GROUP, group)
        res, tab = search_both(ctx, MAIN, MAIN.hints)
        out[group] = (res.tobytes(), tab.tobytes())
    ctx.close()
    ores, otab = main_reference
    assert all(v == (ores.tobytes(), otab.tobytes()) for v in out.values())


def test_run_against_run_and_context_against_context(dctx, main_reference):
    a = search_both(dctx, MAIN, MAIN.hints)
    b = search_both(dctx, MAIN, MAIN.hints)
    other = abi.Context(0)
    other.set_option(abi.LGS_OPT_LOOP_SEARCH_MIN_PAIRS, 0)
    c = search_both(other, MAIN, MAIN.hints)
    other.close()
    for x in (b, c):
        assert x[0].tobytes() == a[0].tobytes() and x[1].tobytes() == a[1].tobytes()
    assert a[0].tobytes() == main_reference[0].tobytes()


def big_snapshot(n=2000, per_map=25):
    poses = lc.figure_eight(n, step=0.0173)       # a period of 363 nodes: every later lap passes the earlier ones
    lo, hi = lc.ranges_of([per_map] * (n // per_map))
    acc = lc.accum_at(poses)
    return lc.Case("2000 nodes", poses, lo, hi, orc.Params(2.0, 0.3, 5), lc.hints_of_nodes(range(n), lo, hi, acc))


def test_2000_nodes_searched_from_every_node():
    """the default group size (500 positions here) and pairs threshold (4 * 10^6 pairs: the device); against
    the host function, the restatement (every 13th hint) and 2000 lone device calls"""
    case = big_snapshot()
    ctx = abi.Context(0)
    g = ctx.loop_graph(case.poses, case.idx_min, case.idx_max)
    rows = lc.hint_rows(case.hints, abi.LOOP_HINT_DTYPE)
    prm = params_of(case.prm)
    res, tab = g.search(prm, rows, per_map=True)
    st = ctx.loop_search_stats()
    assert st["device_calls"] == 1 and st["host_calls"] == 0 and st["launches"] == 3
    assert st["pairs"] == 2000 * 1975
    hres, htab = abi.loop_search_host(case.poses, case.idx_min, case.idx_max, prm, rows, per_map=True)
    assert res.tobytes() == hres.tobytes() and tab.tobytes() == htab.tobytes()
    assert 1000 < res["found"].sum() < 2000 and (tab["node_idx"] >= 0).sum() > 2 * res["found"].sum()
    sub = list(range(0, 2000, 13)) + [1999]
    ores, otab = orc.search_all(case.poses, case.idx_min, case.idx_max, case.prm, [case.hints[j] for j in sub])
    assert res[sub].tobytes() == ores.tobytes() and np.ascontiguousarray(tab[sub]).tobytes() == otab.tobytes()
    ctx.set_option(abi.LGS_OPT_LOOP_SEARCH_MIN_PAIRS, 0)
    lone = np.concatenate([g.search(prm, rows[j:j + 1]) for j in range(2000)])
    assert lone.tobytes() == res.tobytes()
    assert ctx.loop_search_stats()["device_calls"] == 2001
    g.close()
    ctx.close()


@pytest.mark.parametrize("sizes", [[25] * 80, [300, 1300] + [25] * 16, [37] * 54 + [2]],
                         ids=["maps of 25", "a map of 1300", "maps of 37"])
def test_groups_above_one_lds_round(sizes):
    """2000 nodes searched from every node in groups of more than 1024 positions, the positions a workgroup
    stages in LDS at a time: one group (the whole walk: two rounds), 1500 and 1100 positions per group.  A map
    straddles position 1024 in every shape (25: positions 1000-1024, 1300: 300-1599, 37: 999-1035), so a map's
    best is carried from one round into the next.  Against the host function, with the per-map table"""
    n = sum(sizes)
    poses = lc.figure_eight(n, step=0.0173)
    lo, hi = lc.ranges_of(sizes)
    assert any(a < 1024 <= b for a, b in zip(lo[:-1], hi[:-1])) and hi[-2] >= 1900
    acc = lc.accum_at(poses)
    rows = lc.hint_rows(lc.hints_of_nodes(range(n), lo, hi, acc), abi.LOOP_HINT_DTYPE)
    prm = abi.LoopSearchParams(2.0, 0.3, 5, 0)
    hres, htab = abi.loop_search_host(poses, lo, hi, prm, rows, per_map=True)
    # the shape does what it is for: more than a tile of hints walk into the second round
    assert 1000 < hres["found"].sum() < n and (hres["walked"] > 1024).sum() > 256
    ctx = abi.Context(0)
    ctx.set_option(abi.LGS_OPT_LOOP_SEARCH_MIN_PAIRS, 0)
    g = ctx.loop_graph(poses, lo, hi)
    for group in (2 ** 27, 1500, 1100):
        ctx.set_option(abi.LGS_OPT_LOOP_SEARCH_GROUP, group)
        res, tab = g.search(prm, rows, per_map=True)
        assert res.tobytes() == hres.tobytes() and tab.tobytes() == htab.tobytes(), group
        assert g.search(prm, rows).tobytes() == hres.tobytes(), group
    g.close()
    ctx.close()


def test_more_groups_than_a_launch_takes():
    """70000 one-node maps in groups of one position: more groups than the grid's y dimension holds, so the
    group size is doubled until they fit; the bytes stay the host function's"""
    n = 70000
    poses = lc.figure_eight(n, step=0.0131)
    lo, hi = lc.ranges_of([1] * n)
    acc = lc.accum_at(poses)
    hints = [orc.Hint(k, k, k + 1, acc[k]) for k in (n - 1, n - 700, 40000, 65536, 3, 0)]
    prm = abi.LoopSearchParams(1.0, 0.2, 2, 0)
    rows = lc.hint_rows(hints, abi.LOOP_HINT_DTYPE)
    ctx = abi.Context(0)
    ctx.set_option(abi.LGS_OPT_LOOP_SEARCH_MIN_PAIRS, 0)
    ctx.set_option(abi.LGS_OPT_LOOP_SEARCH_GROUP, 1)
    g = ctx.loop_graph(poses, lo, hi)
    res = g.search(prm, rows)
    assert ctx.loop_search_stats()["launches"] == 3
    assert res.tobytes() == abi.loop_search_host(poses, lo, hi, prm, rows).tobytes()
    assert res["found"].sum() >= 3
    g.close()
    ctx.close()


def test_more_hints_than_one_pass_of_the_table():
    """8200 one-node maps: the per-map table of a pass holds 256 hints, so 300 hints take two passes"""
    n = 8200
    poses = lc.figure_eight(n, step=0.0131)
    lo, hi = lc.ranges_of([1] * n)
    acc = lc.accum_at(poses)
    hints = [orc.Hint(k, k, k + 1, acc[k]) for k in range(n - 300, n)]
    prm = abi.LoopSearchParams(1.0, 0.2, 2, 0)
    rows = lc.hint_rows(hints, abi.LOOP_HINT_DTYPE)
    ctx = abi.Context(0)
    g = ctx.loop_graph(poses, lo, hi)
    res, tab = g.search(prm, rows, per_map=True)
    assert ctx.loop_search_stats()["launches"] == 6
    hres, htab = abi.loop_search_host(poses, lo, hi, prm, rows, per_map=True)
    assert res.tobytes() == hres.tobytes() and tab.tobytes() == htab.tobytes()
    assert res["found"].sum() > 100
    g.close()
    ctx.close()


def test_pairs_option_switches_between_host_loop_and_kernels(main_reference):
    """the same bytes on both sides of the switch; the counters and the kernel statistics show which ran"""
    ctx = abi.Context(0)
    ctx.set_option(abi.LGS_OPT_PROFILE, 1)
    g = ctx.loop_graph(MAIN.poses, MAIN.idx_min, MAIN.idx_max)
    hints = MAIN.hints[300:310]
    rows = lc.hint_rows(hints, abi.LOOP_HINT_DTYPE)
    prm = params_of(MAIN.prm)
    pairs = len(hints) * g.info().positions
    want = (main_reference[0][300:310].tobytes(), np.ascontiguousarray(main_reference[1][300:310]).tobytes())

    def run():
        res, tab = g.search(prm, rows, per_map=True)
        return res.tobytes(), tab.tobytes()

    assert pairs < 65536             # below the default: the host loop
    assert run() == want
    assert ctx.loop_search_stats() == dict(device_calls=0, host_calls=1, launches=0, pairs=0)
    assert "k_loop_search" not in ctx.kernel_stats()
    ctx.set_option(abi.LGS_OPT_LOOP_SEARCH_MIN_PAIRS, pairs + 1)      # still below
    assert run() == want
    assert ctx.loop_search_stats()["host_calls"] == 2 and ctx.loop_search_stats()["device_calls"] == 0
    ctx.set_option(abi.LGS_OPT_LOOP_SEARCH_MIN_PAIRS, pairs)          # not below: the kernels
    assert run() == want
    assert ctx.loop_search_stats() == dict(device_calls=1, host_calls=2, launches=3, pairs=pairs)
    ctx.set_option(abi.LGS_OPT_LOOP_SEARCH_MIN_PAIRS, 0)              # always the kernels
    assert run() == want
    assert ctx.loop_search_stats() == dict(device_calls=2, host_calls=2, launches=6, pairs=2 * pairs)
    ks = ctx.kernel_stats()["k_loop_search"]
    assert ks["launches"] == 2 and ks["total_ms"] > 0.0
    for bad in (-1.0, float("nan")):
        with pytest.raises(abi.LgsError):
            ctx.set_option(abi.LGS_OPT_LOOP_SEARCH_MIN_PAIRS, bad)
        with pytest.raises(abi.LgsError):
            ctx.set_option(abi.LGS_OPT_LOOP_SEARCH_GROUP, bad)
    g.close()
    ctx.close()


def test_invalid_arguments_before_any_device_work(dctx):
    H = orc.Hint
    with pytest.raises(abi.LgsError) as e:
        dctx.loop_graph([[0.0, 0.0], [float("inf"), 1.0]], [0], [1])
    assert e.value.status == LGS_ERR_INVALID_ARG
    with pytest.raises(abi.LgsError) as e:
        dctx.loop_graph([[0.0, 0.0], [1.0, 1.0]], [0, 1], [1, 2])
    assert e.value.status == LGS_ERR_INVALID_ARG
    g = dctx.loop_graph(MAIN.poses, MAIN.idx_min, MAIN.idx_max)
    before = dctx.loop_search_stats()
    good = MAIN.hints[320]
    bad_hints = [H(329, 11, 13, 1.0), H(329, 11, 0, 1.0), H(329, 12, 12, 1.0), H(330, 11, 12, 1.0), H(0, 11, 12, 1.0),
                 H(329, 11, 12, float("nan"))]
    for h in bad_hints:
        rows = lc.hint_rows([good, h], abi.LOOP_HINT_DTYPE)
        with pytest.raises(abi.LgsError) as e:
            g.search(params_of(MAIN.prm), rows)
        assert e.value.status == LGS_ERR_INVALID_ARG, h
    for prm in (abi.LoopSearchParams(float("inf"), 1.0, 1, 0), abi.LoopSearchParams(1.0, float("nan"), 1, 0),
                abi.LoopSearchParams(1.0, 1.0, -1, 0)):
        with pytest.raises(abi.LgsError) as e:
            g.search(prm, lc.hint_rows([good], abi.LOOP_HINT_DTYPE))
        assert e.value.status == LGS_ERR_INVALID_ARG
    assert dctx.loop_search_stats() == before
    assert len(g.search(params_of(MAIN.prm), lc.hint_rows([], abi.LOOP_HINT_DTYPE))) == 0      # q = 0 is legal
    g.close()
