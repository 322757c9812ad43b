"""k_select_list (LGS_OPT_SELECT_LIST): a work-list batch selects its refine
candidates from the kept-superblock list, in reference block order, in one
launch that also writes the dense list -- the same bytes k_select + k_compact
write.

Three contexts run the same calls: A with LGS_OPT_SELECT_LIST 0 (k_select +
k_compact), B with the default (k_select_list), C with the option set just
below the batch's largest K (the host's switch: k_select + k_compact again).
After every call every record field and the selection buffers (debug buffers
12-14: segcnt whole, list up to each segment's count, nsel, dlist[0..nsel))
are compared byte for byte, item by item; buffer 15 tells which kernel wrote
them.  One batched case is also checked against the oracle, so the three
cannot all be wrong together.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_bind as ob
import prune_oracle as po
import test_loopbatch_cpu as small
from conftest import launcher_cost
from lgs_amd import abi, loopbatch, scene
from test_gpu_batch import _queries, small_map  # noqa: F401 (fixture)
from test_gpu_rtcsm import assert_same, oracle_match

pytestmark = pytest.mark.gpu
SEG = 1024   # kSelSeg


@pytest.fixture(scope="module")
def abc():
    a, b, c = abi.Context(0), abi.Context(0), abi.Context(0)
    a.set_option(abi.LGS_OPT_SELECT_LIST, 0)
    yield a, b, c
    for x in (a, b, c):
        x.close()


def fields(rec):
    """every field of a result record, as bytes (NaN equals NaN)"""
    out = []
    for name, _ in rec._fields_:
        v = getattr(rec, name)
        if isinstance(v, C.Structure):
            v = v.tuple()
        out.append((name, np.atleast_1d(np.array(v)).tobytes()))
    return out


def selection(ctx, j):
    """the defined bytes of item j's selection, and its K"""
    seg = ctx.debug_buffer("sel_segcnt", j)
    lst = ctx.debug_buffer("sel_list", j).reshape(-1, SEG)
    dense = ctx.debug_buffer("sel_dense", j)
    K = ctx.debug_buffer("cscore", j).size
    assert len(seg) == len(lst) == -(-K // SEG), (len(seg), len(lst), K)
    assert ((0 <= seg) & (seg <= SEG)).all(), seg
    keys = [lst[s, :seg[s]] for s in range(len(seg))]
    flat = np.concatenate(keys) if keys else np.zeros(0, np.int32)
    # reference block order: ascending, every key in its own segment
    assert (np.diff(flat) > 0).all() and all(((k >= s * SEG) & (k < min((s + 1) * SEG, K))).all()
                                              for s, k in enumerate(keys))
    sel = {"segcnt": seg.tobytes(), "list": flat.tobytes(), "by_list": int(ctx.debug_buffer("sel_by_list", j)[0])}
    if dense.size:   # the batch's fine evaluator takes the dense list
        assert dense.size == 1 + K and dense[0] == flat.size, (dense.size, K, dense[0], flat.size)
        assert np.array_equal(dense[1:1 + dense[0]], flat)
        sel["dense"] = dense[:1 + dense[0]].tobytes()
    return sel, K, seg


def run_abc(abc, call, n_items, first_item=0):
    """call(ctx) on A, B and C (C's option just below the largest K of the
    items the debug buffers hold); returns B's records and selections"""
    a, b, c = abc
    recs, sels, Ks = {}, {}, []
    for name, x in (("A", a), ("B", b), ("C", c)):
        if name == "C":
            c.set_option(abi.LGS_OPT_SELECT_LIST, max(Ks) - 1)
        recs[name] = call(x)
        got = [selection(x, j) for j in range(n_items)]
        sels[name] = [g[0] for g in got]
        Ks = [g[1] for g in got]
        segs = [g[2] for g in got]
    for j in range(n_items):
        assert sels["A"][j]["by_list"] == 0 and sels["B"][j]["by_list"] == 1 and sels["C"][j]["by_list"] == 0, j
        for other in ("B", "C"):
            for k in ("segcnt", "list", "dense"):
                assert sels["A"][j].get(k) == sels[other][j].get(k), (other, j, k)
    for other in ("B", "C"):
        assert len(recs["A"]) == len(recs[other])
        for j, (ra, rb) in enumerate(zip(recs["A"], recs[other])):
            assert fields(ra) == fields(rb), (other, j, [n for (n, u), (_, v) in zip(fields(ra), fields(rb)) if u != v])
    return recs["B"], sels["B"], Ks, segs


def shifted_init(s):
    i = s["init"]   # test_gpu_prune_invariants.shifted(name, 1)
    return (i[0] - 0.05, i[1] + 0.1, i[2] + 0.01)


@pytest.mark.parametrize("name", sorted(po.SCENE_BUILDERS))
def test_every_scene_as_a_batch_of_three(abc, name):
    """lowedge: the cflag branch decides; win6x6: 12-row units, ncx no
    multiple of 4; noise: everything is kept, the list covers all K."""
    s = po.scene_inputs(name)
    inits = [s["init"], shifted_init(s), s["init"]]

    def call(x):
        g = x.grid_from_array(s["cells"], s["mx"], s["my"], s["res"])
        sc = x.scan(s["ranges"], s["angles"])
        return x.optimize_pose_query_batch(g, abi.RtcsmParams(*s["params"]), launcher_cost(), [sc, sc, sc], inits)

    recs, sels, _, _ = run_abc(abc, call, 3)
    assert sels[0] == sels[2] and fields(recs[0]) == fields(recs[2])


def test_constant_map_fills_every_segment(abc, world):
    """Every block ties with the seed's score, so every block of every (kept)
    superblock is selected: full segments, a partial last one, keys on both
    sides of every segment boundary."""
    cells = np.full((400, 400), 0.5)
    ang = scene.beam_angles(181)
    r = np.minimum(scene.ray_cast(world, (0.2, -0.1, 0.4), ang), 4.0)   # every beam and window inside the map
    params = (5, 2.0, 2.0, 1.0, 20.0)   # a window of several thousand blocks: full segments and a partial last one
    inits = [(0.2, -0.1, 0.4), (0.0, 0.3, -1.0)]

    def call(x):
        g = x.grid_from_array(cells, -10.0, -10.0, 0.05)
        sc = x.scan(r, ang)
        return x.optimize_pose_query_batch(g, abi.RtcsmParams(*params), launcher_cost(), [sc, sc], inits)

    recs, sels, Ks, segs = run_abc(abc, call, 2)
    for j in range(2):
        K, seg = Ks[j], segs[j]
        assert K % SEG != 0 and len(seg) >= 3, K
        assert (seg[:-1] == SEG).all() and seg[-1] == K - SEG * (len(seg) - 1), (seg, K)
        assert recs[j].coarse_blocks == K


def _mixed(world, rng):
    ang, qs = _queries(world, rng, 6, 541)
    qs[2] = (np.minimum(qs[2][0], 6.0), qs[2][1])                                    # another T
    qs[4] = (np.where(np.arange(541) % 3 == 0, 25.0, qs[4][0]), qs[4][1])            # another Nv
    return ang, qs


def test_items_of_different_T_and_Nv_and_the_oracle(abc, world, small_map):
    """it.nseg differs from the batch's largest; two items against the oracle."""
    cells, mx, my = small_map
    ang, qs = _mixed(world, np.random.default_rng(31))
    params = (5, 1.0, 1.0, 0.6, 20.0)

    def call(x):
        g = x.grid_from_array(cells, mx, my, 0.05)
        return x.optimize_pose_query_batch(g, abi.RtcsmParams(*params), launcher_cost(), [x.scan(r, ang) for r, _ in qs],
                                           [i for _, i in qs])

    recs, _, Ks, _ = run_abc(abc, call, len(qs))
    assert len({-(-K // SEG) for K in Ks}) > 1, Ks
    for j in (0, 2, 4):
        assert_same(recs[j], oracle_match(cells, mx, my, 0.05, params, qs[j][0], ang, qs[j][1]), f"q{j}")


def test_poisoned_workspace_after_another_window(abc, world, small_map):
    """LGS_OPT_POISON_WS 1, after a call with another window: stale list /
    segcnt / cscore bytes, then 0xFF everywhere the batch does not write."""
    cells, mx, my = small_map
    ang, qs = _mixed(world, np.random.default_rng(32))
    params = (5, 1.0, 1.0, 0.6, 20.0)

    def call(x):
        g = x.grid_from_array(cells, mx, my, 0.05)
        scans = [x.scan(r, ang) for r, _ in qs]
        x.optimize_pose_query_batch(g, abi.RtcsmParams(5, 2.0, 1.5, 0.3, 20.0), launcher_cost(), scans[:3],
                                    [i for _, i in qs][:3])
        x.set_option(abi.LGS_OPT_POISON_WS, 1)
        try:
            return x.optimize_pose_query_batch(g, abi.RtcsmParams(*params), launcher_cost(), scans, [i for _, i in qs])
        finally:
            x.set_option(abi.LGS_OPT_POISON_WS, 0)

    plain = abc[1].optimize_pose_query_batch(abc[1].grid_from_array(cells, mx, my, 0.05), abi.RtcsmParams(*params),
                                             launcher_cost(), [abc[1].scan(r, ang) for r, _ in qs], [i for _, i in qs])
    recs, _, _, _ = run_abc(abc, call, len(qs))
    assert [fields(r) for r in recs] == [fields(r) for r in plain]


def test_an_item_that_keeps_nothing(abc, world, small_map):
    """A fixed threshold of 0.15 per beam of the scan (81.15) and an item with
    one valid beam in ten: every bound of it is at most its 55 valid beams'
    round-ups (55 (1 + 2^-10) + 55 / 255 < 56), below the threshold -- an empty
    list, between items that keep something."""
    cells, mx, my = small_map
    ang, qs = _queries(world, np.random.default_rng(33), 3, 541)
    qs[1] = (np.where(np.arange(541) % 10 == 0, qs[1][0], 25.0), qs[1][1])
    params = (5, 1.0, 1.0, 0.6, 20.0)
    coarse = ob.precompute(cells, 5)

    def call(x):
        g, cg = x.grid_from_array(cells, mx, my, 0.05), x.grid_from_array(coarse, mx, my, 0.05)
        return x.optimize_pose_batch(g, cg, abi.RtcsmParams(*params), launcher_cost(), [x.scan(r, ang) for r, _ in qs],
                                     [i for _, i in qs], 0.15)

    recs, sels, _, segs = run_abc(abc, call, 3)
    assert recs[1].coarse_blocks == 0 and not recs[1].pose_found
    assert (segs[1] == 0).all() and sels[1]["list"] == b"" and np.frombuffer(sels[1]["dense"], np.int32).tolist() == [0]
    assert recs[0].coarse_blocks > 0 and recs[2].coarse_blocks > 0


def test_batch_of_80_two_chunks(abc, world, small_map):
    """Two chunks, both workspace banks; the debug buffers hold the last
    chunk's 16 items."""
    cells, mx, my = small_map
    ang, qs = _queries(world, np.random.default_rng(34), 80, 361)
    params = (5, 2.0, 2.0, 0.5, 20.0)

    def call(x):
        g = x.grid_from_array(cells, mx, my, 0.05)
        return x.optimize_pose_query_batch(g, abi.RtcsmParams(*params), launcher_cost(), [x.scan(r, ang) for r, _ in qs],
                                           [i for _, i in qs])

    recs, _, _, _ = run_abc(abc, call, 16)
    assert len(recs) == 80


def test_loop_detector_batch(abc, world):
    """The loop detector's window (+-2.5 m, +-0.5 rad: 6 x 6 superblocks)
    through loopbatch.hip_detect_fn: the same records with and without the
    list kernel."""
    def build(poses, ang):
        m = ob.OMap(0.05, 100, 300, 300)
        for q in poses:
            m.integrate(q, ob.OScan(scene.ray_cast(world, q, ang), ang), ob.BuilderParams(0.01, 20.0, 0.6, 0.45))
        return m.cells(), m.m.min_x, m.m.min_y, 0.05

    maps, cands = scene.loop_problem(world, build, n_maps=2, nodes_per_map=3, n_beams=181, seed=5, perturb=(1.0, 0.3),
                                     arc_scans=4, map_beams=361)
    p, c = abi.RtcsmParams(5, 5.0, 5.0, 0.5, 20.0), abi.CostGEParams(*small.COST)
    a, b, _ = abc
    ra = loopbatch.run_sharded(cands, loopbatch.hip_detect_fn(a, maps, cands, p, c, 0.6))
    rb = loopbatch.run_sharded(cands, loopbatch.hip_detect_fn(b, maps, cands, p, c, 0.6))
    assert ra.tobytes() == rb.tobytes()
    assert int(a.debug_buffer("sel_by_list", 0)[0]) == 0 and int(b.debug_buffer("sel_by_list", 0)[0]) == 1
