"""The correlative matcher's pruning inequalities, each checked by name against
the CPU oracle's dense scores (tests/prune_oracle.py; DESIGN.md §4.1, §4.1a,
§4.1b).  After a match the device's sbound / L / tedge / cscore buffers are
read back (Context.debug_buffer) and, with exact fp64 comparisons:

  (a) soundness     sbound[t, s] >= cmax[t, s], the best coarse score among the
                    superblock's member blocks;
  (b) seed bound    max(Lc[0..3]) <= fs.max() and Lp <= fs.max();
  (c) edge flags    tedge[t] == edge[t];
  (d) unsafe blocks every block whose fine max exceeds its coarse score lies in
                    a superblock with sbound >= that fine max.  No pruned path
                    scores a block regardless of L: k_coarse_rows' selection
                    ballot, k_keep, unsafe_angle and k_select all take
                    `kp = (bnd > pl.thr) && bnd >= L` (k_rtcsm.hip), so the
                    strip-clamped bound alone keeps such a block alive;
  (e) consistency   the blocks that rule keeps number the record's
                    coarse_blocks, and their cscore entries are cs bit for bit;
  (f) useful        every sbound is finite on in-range maps and at most
                    (U (1 + 2^-10) + Nv (1/255 + 2^-24)) (1 + 1e-9): the fp16
                    round-up (2^-10 relative or 2^-24 absolute per beam), the
                    byte round-up (1/255 per beam) and sb_mult (with the
                    division's 1 + 2^-50).  U reads 0 outside the map, except
                    that the strip left of / below it reads the map's first
                    coarse column / row (prune_oracle's Ustrip): the planes
                    hold it that way and (d) needs it, so a bound that reaches
                    the strip may exceed the plain U's cap.  Ustrip equals the
                    plain U in every angle without an edge beam
                    (tests/test_prune_oracle_cpu.py), where this is the plain cap;
  (g) margin        sbound[t, s] >= fl(cmax[t, s] sb_mult), sb_mult = 1 + 4 (Nv + 1) 2^-53.
                    For cells in [0, 1] the sums of the fp16 round-ups (or of
                    the bytes) are exact in fp64 in any order (24 + log2 Nv
                    bits), so the factor is no longer needed for (a) -- which
                    therefore cannot see it go missing; it is the design's
                    margin for an order-dependent sum, and since the sum before
                    the factor is >= cmax and rounding is monotone, the product
                    is >= fl(cmax sb_mult).  The "ones" scenes hold full
                    superblocks whose sum equals cmax exactly; in the "half062"
                    scenes the ideal bound equals cmax and only the round-ups
                    to fp16 and to bytes keep (a).

A bound that is too low for a block that does not win, or an L that is too
high but still below the winner, fails here and nowhere else in the suite.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_bind as ob
import prune_oracle as po
from conftest import launcher_cost
from lgs_amd import abi

pytestmark = pytest.mark.gpu
DBL_MIN = 2.2250738585072014e-308

DEFAULTS = {abi.LGS_OPT_SUPER_PRUNE: 1, abi.LGS_OPT_LANES_MIN_BATCH: 2, abi.LGS_OPT_LEAN_PROJECT: 1,
            abi.LGS_OPT_FAST_ROWS: 1, abi.LGS_OPT_SEED_WIDE: 12, abi.LGS_OPT_FUSED_PLANES: 1, abi.LGS_OPT_PROFILE: 0}


class options:
    """Context options for one block, the library defaults restored after it."""

    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, {getattr(abi, "LGS_OPT_" + k): v for k, v in kw.items()}

    def __enter__(self):
        for k, v in self.kw.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.ctx.set_option(k, DEFAULTS[k])


def buffers(ctx, item=0):
    b = {n: ctx.debug_buffer(n, item) for n in ("sbound", "L", "tedge", "cscore")}
    b["Lp"], b["Lc"] = b["L"][0], b["L"][8:12]
    b["super_bytes"] = C.c_size_t()
    ctx.check(ctx.lib.lgs_debug_item_buffer(ctx.h, item, abi.Context.DEBUG_BUFFERS["super"][0], None, 0,
                                            C.byref(b["super_bytes"])), "debug_item_buffer")
    b["super_bytes"] = b["super_bytes"].value
    return b


def check_invariants(o, rec, b, tag):
    """(a)-(f) of the module docstring for one match; returns the kept-block count."""
    T, nsb2 = o.T, o.nsb2
    sb = b["sbound"].reshape(T, nsb2)
    thr = rec.score_threshold if rec is not None else b["thr"]
    fsmax = o.fs.max()
    # the layout (and with it the superblock kernel) the search was meant to take
    assert b["super_bytes"] == o.layout["super_bytes"], (tag, b["super_bytes"], o.layout)
    # (a)
    bad = np.argwhere(sb < o.cmax)
    assert not len(bad), (tag, "sbound < cmax at (t, s)", bad[:4].tolist(), sb[tuple(bad[0])], o.cmax[tuple(bad[0])])
    # (g)
    floor_g = o.cmax * (1.0 + 4.0 * (o.Nv + 1) * 2.0 ** -53)
    bad = np.argwhere(sb < floor_g)
    assert not len(bad), (tag, "sbound < cmax sb_mult at (t, s)", bad[:4].tolist(), sb[tuple(bad[0])],
                          floor_g[tuple(bad[0])])
    # (b)
    assert b["Lc"].max() <= fsmax, (tag, "Lc", b["Lc"].tolist(), fsmax)
    assert b["Lp"] <= fsmax, (tag, "Lp", b["Lp"], fsmax)
    assert b["Lp"] == b["Lc"].max(), tag
    # (c)
    assert np.array_equal(b["tedge"] != 0, o.edge), (tag, "tedge", np.flatnonzero((b["tedge"] != 0) != o.edge)[:8])
    # (d)
    un = o.unsafe_blocks()
    s_of = o.super_of_block()
    for t, jx, jy in np.argwhere(un):
        assert sb[t, s_of[jx, jy]] >= o.fmax_B[t, jx, jy], (tag, "unsafe block", (t, jx, jy), sb[t, s_of[jx, jy]],
                                                           o.fmax_B[t, jx, jy], o.c_B[t, jx, jy])
    # (e)
    L = b["Lp"]
    kept = o.kept(sb, L, thr)
    nkept = o.kept_blocks(sb, L, thr)
    if rec is not None:
        assert rec.slow_path == 0, tag
        assert nkept == rec.coarse_blocks, (tag, "coarse_blocks", nkept, rec.coarse_blocks)
    scored = kept[:, s_of]                                   # [T, ncx, ncy]
    csd = b["cscore"].reshape(T, o.ncx, o.ncy)
    assert np.array_equal(csd[scored].view(np.int64), o.cs[scored].view(np.int64)), (tag, "cscore")
    # (f)
    assert np.isfinite(sb).all(), tag
    cap = (o.Ustrip * (1.0 + 2.0 ** -10) + o.Nv * (1.0 / 255.0 + 2.0 ** -24)) * (1.0 + 1e-9)
    bad = np.argwhere(sb > cap)
    assert not len(bad), (tag, "sbound > cap at (t, s)", bad[:4].tolist(), sb[tuple(bad[0])], cap[tuple(bad[0])])
    # the winner survives the restated rule (what the suite checked before, by consequence)
    if fsmax > thr:
        wt, wx, wy = np.unravel_index(np.argmax(o.fs), o.fs.shape)
        assert kept[wt, s_of[wx // o.lr, wy // o.lr]], tag
    return nkept


def ran(stats, *names):
    for n in names:
        assert n in stats and stats[n]["launches"] >= 1, (n, sorted(stats))   # only launched kernels are listed


def device_inputs(ctx, s):
    g = ctx.grid_from_array(s["cells"], s["mx"], s["my"], s["res"])
    return g, ctx.scan(s["ranges"], s["angles"]), abi.RtcsmParams(*s["params"])


def shifted(name, k):
    """The scene with another initial pose (a batch's further items), and its oracle."""
    s = dict(po.scene_inputs(name))
    i = s["init"]
    s["init"] = (i[0] - 0.05 * k, i[1] + 0.1 * k, i[2] + 0.01 * k)
    return s, po.PruneOracle(s["cells"], s["mx"], s["my"], s["res"], s["params"], s["ranges"], s["angles"], s["init"])


_shifted = {}


def shifted_cached(name, k):
    if (name, k) not in _shifted:
        _shifted[(name, k)] = shifted(name, k)
    return _shifted[(name, k)]


# ---------------------------------------------------------------- every scene, lone and batched
@pytest.mark.parametrize("name", sorted(po.SCENE_BUILDERS))
def test_lone_match(ctx, name):
    """n = 1: k_project, k_super_oct / k_super, the one-launch seed
    (k_seed_super<0>), k_coarse_rows, k_select<1024>."""
    s, o = po.scene_inputs(name), po.scene_oracle(name)
    g, sc, P = device_inputs(ctx, s)
    with options(ctx, PROFILE=1):
        ctx.reset_stats()
        rec = ctx.optimize_pose_query(g, P, launcher_cost(), sc, s["init"])
        b = buffers(ctx)
        st = ctx.kernel_stats()
    ran(st, "k_project", "k_precompute", "k_super_planes", "k_super", "k_seed", "k_coarse", "k_select")
    assert "k_coarse_aux" not in st          # no work list: the row kernel scored the blocks
    check_invariants(o, rec, b, name)


@pytest.mark.parametrize("name", sorted(po.SCENE_BUILDERS))
def test_batch(ctx, name):
    """n = 3 (two distinct queries): the work list (k_keep, k_coarse_list_c,
    k_unsafe_list), the wide seed, and on octet layouts the lean rows."""
    s, o = po.scene_inputs(name), po.scene_oracle(name)
    s1, o1 = shifted_cached(name, 1)
    g, sc, P = device_inputs(ctx, s)
    inits = [s["init"], s1["init"], s["init"]]
    with options(ctx, PROFILE=1):
        ctx.reset_stats()
        recs = ctx.optimize_pose_query_batch(g, P, launcher_cost(), [sc, sc, sc], inits)
        bufs = [buffers(ctx, j) for j in range(3)]
        st = ctx.kernel_stats()
    ran(st, "k_project", "k_precompute", "k_super_planes", "k_super", "k_seed", "k_coarse", "k_coarse_aux", "k_select")
    # lean_rows(): octet layout, LowRes 5 and an even map width (the staged fine evaluator) -> the beam
    # tables only (32 B per beam), else 24 B per (angle, beam)
    lean = o.layout["oct"] and o.lr == 5 and s["cells"].shape[1] % 2 == 0
    want = 32.0 * o.Nv * 3 if lean else 24.0 * o.Nv * (2 * o.T + o1.T)
    assert st["k_project"]["algo_bytes"] == want, (name, st["k_project"], want)
    for j, (oo, tag) in enumerate(((o, "item0"), (o1, "item1"), (o, "item2"))):
        check_invariants(oo, recs[j], bufs[j], f"{name} {tag}")


# ---------------------------------------------------------------- the switches
SWITCH_SCENES = ("room", "lowedge", "win6x6", "noise", "half062", "half062_6x6")


@pytest.mark.parametrize("name", SWITCH_SCENES)
def test_lone_match_through_the_work_list_and_batch_through_the_rows(ctx, name):
    """LGS_OPT_LANES_MIN_BATCH 1: a lone match takes the batch's chain; 64: a
    batch of 2 takes the lone chain (k_coarse_rows for every item)."""
    s, o = po.scene_inputs(name), po.scene_oracle(name)
    s1, o1 = shifted_cached(name, 1)
    g, sc, P = device_inputs(ctx, s)
    with options(ctx, PROFILE=1, LANES_MIN_BATCH=1):
        ctx.reset_stats()
        rec = ctx.optimize_pose_query(g, P, launcher_cost(), sc, s["init"])
        b = buffers(ctx)
        st = ctx.kernel_stats()
    ran(st, "k_super", "k_seed", "k_coarse", "k_coarse_aux")
    check_invariants(o, rec, b, f"{name} list")
    with options(ctx, PROFILE=1, LANES_MIN_BATCH=64):
        ctx.reset_stats()
        recs = ctx.optimize_pose_query_batch(g, P, launcher_cost(), [sc, sc], [s["init"], s1["init"]])
        bufs = [buffers(ctx, j) for j in range(2)]
        st = ctx.kernel_stats()
    ran(st, "k_super", "k_seed", "k_coarse")
    assert "k_coarse_aux" not in st
    check_invariants(o, recs[0], bufs[0], f"{name} rows item0")
    check_invariants(o1, recs[1], bufs[1], f"{name} rows item1")


@pytest.mark.parametrize("lean,fast", [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("name", SWITCH_SCENES)
def test_lean_and_fast_rows(ctx, name, lean, fast):
    """LGS_OPT_LEAN_PROJECT / LGS_OPT_FAST_ROWS: k_super_oct forms the
    superblock-base row itself (certified fast chain or exact chain) or reads
    k_project's; the projection's algorithmic bytes tell which ran, and the
    bounds are the same bits either way."""
    s, o = po.scene_inputs(name), po.scene_oracle(name)
    g, sc, P = device_inputs(ctx, s)
    with options(ctx, PROFILE=1, LEAN_PROJECT=lean, FAST_ROWS=fast):
        ctx.reset_stats()
        recs = ctx.optimize_pose_query_batch(g, P, launcher_cost(), [sc, sc], [s["init"], s["init"]])
        b = buffers(ctx, 1)
        st = ctx.kernel_stats()
    assert st["k_project"]["algo_bytes"] == (32.0 * o.Nv * 2 if lean else 24.0 * o.Nv * o.T * 2)
    check_invariants(o, recs[1], b, f"{name} lean{lean} fast{fast}")
    ref = buffers(ctx, 0)
    assert np.array_equal(ref["sbound"].view(np.int64), b["sbound"].view(np.int64))
    if (lean, fast) != (1, 1):
        with options(ctx):
            ctx.optimize_pose_query_batch(g, P, launcher_cost(), [sc, sc], [s["init"], s["init"]])
            d = buffers(ctx, 1)
        for k in ("sbound", "tedge", "L"):
            assert np.array_equal(d[k].view(np.uint8), b[k].view(np.uint8)), (name, k)


@pytest.mark.parametrize("wide", [0, 5, 16])
@pytest.mark.parametrize("name", ("room", "win6x6", "beams181", "half062"))
def test_seed_wide_and_one_launch(ctx, name, wide):
    """LGS_OPT_SEED_WIDE: 0 = the one-launch seed of 4 candidates in a batch
    (k_seed_super<0>), 5 and 16 = k_seed_members + k_seed_super<2>.  L is a
    lower bound of the final score whichever blocks seed it; the wide seed
    never scores more blocks than the narrow one."""
    s, o = po.scene_inputs(name), po.scene_oracle(name)
    s1, o1 = shifted_cached(name, 1)
    g, sc, P = device_inputs(ctx, s)
    with options(ctx, PROFILE=1, SEED_WIDE=wide):
        ctx.reset_stats()
        recs = ctx.optimize_pose_query_batch(g, P, launcher_cost(), [sc, sc], [s["init"], s1["init"]])
        bufs = [buffers(ctx, j) for j in range(2)]
        st = ctx.kernel_stats()
    ran(st, "k_seed", "k_coarse_aux")
    n0 = check_invariants(o, recs[0], bufs[0], f"{name} wide{wide} item0")
    n1 = check_invariants(o1, recs[1], bufs[1], f"{name} wide{wide} item1")
    if wide:
        with options(ctx, SEED_WIDE=0):
            narrow = ctx.optimize_pose_query_batch(g, P, launcher_cost(), [sc, sc], [s["init"], s1["init"]])
        assert n0 + n1 <= narrow[0].coarse_blocks + narrow[1].coarse_blocks


def oracle_fixed(cells, coarse, s, thr):
    g, cg = ob.OGrid(cells, s["mx"], s["my"], s["res"]), ob.OGrid(coarse, s["mx"], s["my"], s["res"])
    out = ob.Summary()
    ob.lib().orc_rtcsm_optimize_pose(C.byref(g.g), C.byref(cg.g), C.byref(ob.RtcsmParams(*s["params"])),
                                     C.byref(launcher_cost(oracle=True)), C.byref(ob.OScan(s["ranges"], s["angles"]).s),
                                     ob.Pose(*s["init"]), thr, C.byref(out))
    return out


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", ("room", "lowedge", "oddmap", "win6x6", "aniso", "lr4", "noise", "ones", "ones_wide",
                                  "half062", "half062_wide"))
def test_query_planes_and_supplied_coarse_map(ctx, name, fused):
    """LGS_OPT_FUSED_PLANES 1: k_super_hv forms the octet units; 0:
    k_super_planes (both its octet and its fp16 branch).  Each with the
    query's own precompute and with a caller-supplied coarse map (the
    phase-plane copy and its fp16 round-ups, k_decimate_jobs), lone and as a
    batch with a fixed threshold."""
    s, o = po.scene_inputs(name), po.scene_oracle(name)
    g, sc, P = device_inputs(ctx, s)
    cg = ctx.grid_from_array(o.coarse, s["mx"], s["my"], s["res"])
    nthr = 0.05
    with options(ctx, PROFILE=1, FUSED_PLANES=fused):
        ctx.reset_stats()
        rec = ctx.optimize_pose_query(g, P, launcher_cost(), sc, s["init"])
        b = buffers(ctx)
        st = ctx.kernel_stats()
        ran(st, "k_precompute", "k_super_planes", "k_super")
        check_invariants(o, rec, b, f"{name} fused{fused} query")
        ctx.reset_stats()
        two = ctx.optimize_pose(g, cg, P, launcher_cost(), sc, s["init"], nthr)
        b2 = buffers(ctx)
        st = ctx.kernel_stats()
        ran(st, "k_super_planes", "k_super")
        assert "k_precompute" not in st     # only launched kernels are listed
        assert two.score_threshold == nthr * len(s["ranges"])
        check_invariants(o, two, b2, f"{name} fused{fused} supplied")
        # the bounds are a function of the coarse map alone: the same bits from either builder
        assert np.array_equal(b["sbound"].view(np.int64), b2["sbound"].view(np.int64))
        recs = ctx.optimize_pose_batch(g, cg, P, launcher_cost(), [sc, sc], [s["init"], s["init"]], nthr)
        check_invariants(o, recs[1], buffers(ctx, 1), f"{name} fused{fused} supplied batch")
    ora = oracle_fixed(s["cells"], o.coarse, s, nthr)
    assert list(two.best_win) == list(ora.best_win) and two.score_max == ora.score_max


def test_loop_detect_batch(ctx):
    """One lgs_loop_detect_rtcsm call: three candidates against one local map
    through the loop detector's 6 x 6-superblock window (k_super_oct<9, 3>),
    the coarse map computed inside the call, a fixed score threshold."""
    s = po.scene_inputs("win6x6")
    g, sc, P = device_inputs(ctx, s)
    thr = 0.3
    cands = [(sc, shifted_cached("win6x6", k)[0]["init"] if k else s["init"], 10 + k) for k in range(3)]
    with options(ctx, PROFILE=1):
        ctx.reset_stats()
        res = ctx.loop_detect(P, launcher_cost(), thr, [(g, None, (0.0, 0.0, 0.0), 0, 0, 3)], cands)
        bufs = [buffers(ctx, j) for j in range(3)]
        st = ctx.kernel_stats()
        cnt = ctx.match_counters()
    ran(st, "k_precompute", "k_super", "k_seed", "k_coarse", "k_coarse_aux")
    total = 0
    for k in range(3):
        o = shifted_cached("win6x6", k)[1] if k else po.scene_oracle("win6x6")
        assert o.layout["unit8"] == 3
        bufs[k]["thr"] = thr * len(s["ranges"])
        total += check_invariants(o, None, bufs[k], f"loop cand{k}")
        assert bool(res[k].found) == bool(o.fs.max() > bufs[k]["thr"]), k
        if res[k].found:
            assert res[k].score == o.fs.max(), k
    assert cnt["matches"] == 3 and cnt["pruned"] == 3 and cnt["coarse_blocks"] == total, (cnt, total)


# ---------------------------------------------------------------- cells outside [0, 1]
def _identical(a, b, tag):
    """test_gpu_rtcsm._identical, with NaN equal to NaN (a NaN cell under the best pose's cost kernel)"""
    assert a.pose_found == b.pose_found, tag
    assert list(a.best_win) == list(b.best_win), tag
    assert np.array_equal(a.score_max, b.score_max, equal_nan=True), tag
    assert np.array_equal(a.normalized_cost, b.normalized_cost, equal_nan=True), tag
    assert np.array_equal(list(a.covariance), list(b.covariance), equal_nan=True), tag


@pytest.mark.parametrize("name", ("room", "aniso"))          # 8-bit octet units / fp16 planes
@pytest.mark.parametrize("where", ("fine", "coarse"))
@pytest.mark.parametrize("value", (1.5, np.inf, -0.25, np.nan), ids=("above1", "inf", "negative", "nan"))
def test_out_of_range_cells_disable_the_bounds(ctx, name, where, value):
    """Anything that is not 0 <= v <= 1 has no valid round-up: the set's flag
    is raised, every bound is +inf, nothing is pruned and the result is the
    unpruned one (and the oracle's, where the reference defines it: a max over
    NaN or a sum with inf depends on its order)."""
    s, o = dict(po.scene_inputs(name)), po.scene_oracle(name)
    ix, iy = o.idx[o.T // 2, o.Nv // 2]                      # a cell the scan hits
    h, w = s["cells"].shape
    ix, iy = int(np.clip(ix, 8, w - 9)), int(np.clip(iy, 8, h - 9))
    cells = s["cells"].copy()
    cells[iy - 6:iy + 6, ix - 6:ix + 6] = value              # wider than a LowRes window: the coarse map holds it too
    s["cells"] = cells
    coarse = ob.precompute(cells, s["params"][0])
    if np.isnan(value):
        coarse[iy, ix] = np.nan                              # whatever the host's window max made of the patch
    assert np.isnan(coarse).any() if np.isnan(value) else (coarse == value).any()
    g, sc, P = device_inputs(ctx, s)
    cg = ctx.grid_from_array(coarse, s["mx"], s["my"], s["res"])

    def run():
        if where == "fine":
            return ctx.optimize_pose_query(g, P, launcher_cost(), sc, s["init"])
        return ctx.optimize_pose(g, cg, P, launcher_cost(), sc, s["init"], DBL_MIN)

    with options(ctx, SUPER_PRUNE=1):
        on = run()
        sb = ctx.debug_buffer("sbound")
        nbytes = buffers(ctx)["super_bytes"]
        with options(ctx, SUPER_PRUNE=0):
            off = run()
    tag = f"{name} {where} {value}"
    assert nbytes == o.layout["super_bytes"], tag
    assert sb.size == o.T * o.nsb2 and (sb == np.inf).all(), (tag, sb[~(sb == np.inf)][:4])
    _identical(on, off, tag)
    assert on.coarse_blocks == off.coarse_blocks == o.T * o.ncx * o.ncy, tag
    if value in (1.5, -0.25):
        ora = oracle_fixed(cells, coarse, s, DBL_MIN)
        assert on.pose_found == ora.pose_found and list(on.best_win) == list(ora.best_win), tag
        assert on.score_max == ora.score_max, tag
