"""Many ICP references in one pass (lgs_icp_ref_set_*, csrc/k_icp_ref.hip,
DESIGN.md 4.5d) on the GPU.  Tolerance: none -- reference i of a set must be,
in everything a caller can observe, lgs_icp_ref_create of its node range: info,
pairs, summary, trajectory and Hessian are compared byte for byte with the lone
handle and with the test-side restatement (tests/icp_ref_oracle.py).
"""
import ctypes as C

import numpy as np
import pytest

import icp_oracle as orc
import icp_ref_oracle as rorc
from lgs_amd import abi, scene

pytestmark = pytest.mark.gpu

LGS_ERR_INVALID_ARG, LGS_ERR_OOM, LGS_ERR_INTERNAL = 1, 4, 5
REL_REF, REL_CUR = (0.1, -0.05, 0.02), (-0.03, 0.08, -0.015)
CUR_ROBOT = (0.65, 0.3, 0.21)
STARTS = [(0.4, 0.1, 0.15), (0.8, 0.45, 0.27)]
O = (0.0, 0.0, 0.0)


def prm_for(n, cap=5, D=1.0):
    return orc.Params(cap, 0.0, 0.01, 20.0, 1e-3, 1e-3, D, 3.0 if n < 100 else 0.5)


def dev_scan(ctx, s: orc.ScanIn):
    return ctx.scan(np.ascontiguousarray(s.ranges, dtype=np.float64), np.ascontiguousarray(s.angles, dtype=np.float64),
                    s.rel, s.min_range, s.max_range)


def bits(x):
    return np.float64(x).tobytes()


def pose_t(p):
    return (p.x, p.y, p.theta)


def assert_summary(dev, ref: orc.Result, init):
    assert (dev.pose_found, dev.iterations, dev.num_pairs, dev.initial_pairs) == \
        (ref.pose_found, ref.iterations, ref.num_pairs, ref.initial_pairs)
    for name in ("cost", "pair_cost", "initial_cost", "normalized_cost"):
        assert bits(getattr(dev, name)) == bits(getattr(ref, name)), name
    for name, want in (("initial_pose", init), ("sensor_pose", ref.sensor_pose),
                       ("best_sensor_pose", ref.best_sensor_pose), ("estimated_pose", ref.estimated_pose)):
        assert bits(pose_t(getattr(dev, name))) == bits(want), name
    assert bits(list(dev.hessian)) == bits(ref.hessian), "hessian"
    assert bits(list(dev.covariance)) == bits(ref.covariance), "covariance"


_SCENES = {}


def scene_scans(world, n, K, near_from=None):
    """K reference scans of n beams at robot poses (0.1 k - 0.4, 0.05 k - 0.2, 0.02 k), cast from their sensor
    poses, and the current scan at CUR_ROBOT; scans from near_from on see 6 m only (their own max_range), so
    a reference made of them has a smaller bounding box and another grid"""
    key = (n, K, near_from)
    if key not in _SCENES:
        ang = scene.beam_angles(n)
        poses = [(0.1 * k - 0.4, 0.05 * k - 0.2, 0.02 * k) for k in range(K)]
        refs = [orc.ScanIn(scene.ray_cast(world, orc.compound(p, REL_REF), ang), ang, REL_REF, 0.0,
                           6.0 if near_from is not None and k >= near_from else 30.0) for k, p in enumerate(poses)]
        cur = orc.ScanIn(scene.ray_cast(world, orc.compound(CUR_ROBOT, REL_CUR), ang), ang, REL_CUR)
        _SCENES[key] = (refs, poses, cur)
    return _SCENES[key]


def check_reference(ctx, prm, view, refs, poses, cur, S, steps):
    """one reference of a set against the lone handle and the restatement"""
    p = abi.IcpParams(*prm)
    lone = ctx.icp_ref([dev_scan(ctx, r) for r in refs], poses, p)
    rt = rorc.concat_tables(prm, refs, poses)
    info = view.info()
    assert info == lone.info()
    assert (info.n_refs, info.entries) == (len(refs), len(rt.k))
    assert info.lines == int(np.count_nonzero(~np.isnan(rt.table.nx)))
    for sensor in (orc.compound(CUR_ROBOT, REL_CUR), orc.compound(STARTS[1], REL_CUR)):
        k, j, e = view.pairs(S, sensor, p)
        lk, lj, le = lone.pairs(S, sensor, p)
        wk, wj, we, _ = rorc.pairs(prm, rt, cur, sensor)
        assert k.tolist() == lk.tolist() == wk.tolist()   # counted from the range's first scan
        assert j.tolist() == lj.tolist() == wj.tolist()
        assert e.tobytes() == le.tobytes() == we.tobytes()
    out, traj = view.refine(S, STARTS[0], p, trajectory=True)
    lout, ltraj = lone.refine(S, STARTS[0], p, trajectory=True)
    assert bytes(out) == bytes(lout)
    assert np.array(traj).tobytes() == np.array(ltraj).tobytes()
    want = rorc.refine(prm, refs, poses, cur, STARTS[0], rt)
    assert len(traj) == out.iterations == want.iterations
    for g, w in zip(traj, want.trajectory):
        assert bits(g) == bits(w)
    assert_summary(out, want, STARTS[0])
    batch = view.refine_batch([S, S], [STARTS[0], STARTS[1]], p)
    assert bytes(batch[0]) == bytes(out) and bytes(batch[1]) == bytes(lone.refine(S, STARTS[1], p))
    lone.close()
    return info, out


# ------------------------------------------------------------------ 1. a set equals lone creates
RANGES_65 = [(0, 1), (1, 3), (5, 5), (2, 2)]


@pytest.mark.parametrize("blind", [None, 5, 2])
def test_a_set_of_four_references_equals_lone_creates(ctx, world, blind):
    """seven 65-beam scans, ranges [0,1] [1,3] [5,5] [2,2]: 130, 195, 65 and 65 entries, so a list of
    256-entry blocks must not run from one reference into the next; scans 1 and 2 are shared, under different
    labels.  blind: that scan's own max_range makes all its beams unusable -- scan 5 empties reference 2, scan 2
    empties reference 3 and leaves a hole in reference 1"""
    refs, poses, cur = scene_scans(world, 65, 7)
    if blind is not None:
        refs = list(refs)
        refs[blind] = refs[blind]._replace(max_range=0.02)
    prm = prm_for(65)
    scans = [dev_scan(ctx, r) for r in refs]
    rset = ctx.icp_ref_set(scans, poses, [a for a, _ in RANGES_65], [b for _, b in RANGES_65], abi.IcpParams(*prm))
    for s in scans:   # the set copied what it needs
        s.close()
    assert len(rset) == 4
    S = dev_scan(ctx, cur)
    entries, found = [], []
    for i, (a, b) in enumerate(RANGES_65):
        info, out = check_reference(ctx, prm, rset[i], refs[a:b + 1], poses[a:b + 1], cur, S, 5)
        entries.append(info.entries)
        found.append(out.pose_found)
    if blind is None:
        assert entries == [130, 195, 65, 65] and found == [1, 1, 1, 1]
    elif blind == 5:
        assert entries == [130, 195, 0, 65] and found == [1, 1, 0, 1]
        assert rset[2].info()[2:5] == (0, 1, 1)
    else:
        assert entries == [130, 130, 65, 0] and found == [1, 1, 1, 0]
    rset.close()


def test_three_references_of_ten_scans_with_grids_of_different_sizes(ctx, world):
    """361 beams, ranges [0,9] [5,14] [10,19]: 15 blocks per reference; scans 10 .. 19 see 6 m only, so the
    three grids differ"""
    refs, poses, cur = scene_scans(world, 361, 20, near_from=10)
    prm = prm_for(361)
    ranges = [(0, 9), (5, 14), (10, 19)]
    rset = ctx.icp_ref_set([dev_scan(ctx, r) for r in refs], poses, [a for a, _ in ranges], [b for _, b in ranges],
                           abi.IcpParams(*prm))
    S = dev_scan(ctx, cur)
    infos = []
    for i, (a, b) in enumerate(ranges):
        info, out = check_reference(ctx, prm, rset[i], refs[a:b + 1], poses[a:b + 1], cur, S, 5)
        assert out.pose_found == 1 and info.entries > 256
        infos.append(info)
    assert infos[0].entries == 3610
    assert (infos[0].cells_x, infos[0].cells_y) != (infos[2].cells_x, infos[2].cells_y)
    assert infos[2].entries < infos[1].entries < infos[0].entries
    rset.close()


# ------------------------------------------------------------------ 2. one reference, mixing, stability
def test_one_reference_set_mixing_runs_contexts_and_lifetimes(ctx, world):
    refs, poses, cur = scene_scans(world, 65, 7)
    prm = prm_for(65)
    p = abi.IcpParams(*prm)
    scans = [dev_scan(ctx, r) for r in refs]
    S = dev_scan(ctx, cur)
    one = ctx.icp_ref_set(scans, poses, [1], [3], p)
    lone = ctx.icp_ref(scans[1:4], poses[1:4], p)
    assert len(one) == 1 and one[0].info() == lone.info() == one[-1].info()
    want = lone.refine(S, STARTS[0], p)
    assert bytes(one[0].refine(S, STARTS[0], p)) == bytes(want)
    with pytest.raises(IndexError):
        one[1]
    assert ctx.lib.lgs_icp_ref_set_ref(one.h, 1) is None and ctx.lib.lgs_icp_ref_set_ref(one.h, -1) is None
    assert ctx.lib.lgs_icp_ref_set_size(None) == 0 and ctx.lib.lgs_icp_ref_set_ref(None, 0) is None

    # one batch of borrowed and created references
    rset = ctx.icp_ref_set(scans, poses, [0, 1, 5, 2], [1, 3, 5, 2], p)
    other = ctx.icp_ref(scans[0:2], poses[0:2], p)
    items = [(rset[1], STARTS[0]), (lone, STARTS[0]), (rset[0], STARTS[1]), (other, STARTS[1]), (rset[3], STARTS[0])]
    got = lone.refine_batch([S] * len(items), [i[1] for i in items], p, refs=[i[0] for i in items])
    assert [bytes(g) for g in got] == [bytes(h.refine(S, ip, p)) for h, ip in items]
    assert bytes(got[0]) == bytes(got[1]) == bytes(want) and bytes(got[2]) == bytes(got[3])

    # two runs, two contexts
    again = ctx.icp_ref_set(scans, poses, [0, 1, 5, 2], [1, 3, 5, 2], p)
    theirs_ctx = abi.Context(0)
    try:
        theirs = theirs_ctx.icp_ref_set([dev_scan(theirs_ctx, r) for r in refs], poses, [0, 1, 5, 2], [1, 3, 5, 2], p)
        T = dev_scan(theirs_ctx, cur)
        for i in range(4):
            a = rset[i].refine(S, STARTS[0], p)
            assert bytes(a) == bytes(again[i].refine(S, STARTS[0], p)) == bytes(theirs[i].refine(T, STARTS[0], p))
            assert rset[i].info() == again[i].info() == theirs[i].info()
            sensor = orc.compound(CUR_ROBOT, REL_CUR)
            assert [x.tobytes() for x in rset[i].pairs(S, sensor, p)] == [x.tobytes() for x in theirs[i].pairs(T, sensor, p)]
        # a borrowed reference belongs to its set's context
        out = abi.IcpSummary()
        assert ctx.lib.lgs_icp_ref_optimize_pose(ctx.h, theirs[0].h, S.h, abi.Pose2D(*STARTS[0]), C.byref(p),
                                                 C.byref(out), None) == LGS_ERR_INVALID_ARG
    finally:
        theirs_ctx.close()
    theirs.close()   # after its context, as an lgs_icp_ref may be

    # lgs_icp_ref_destroy ignores a borrowed reference
    view = rset[1]
    ctx.lib.lgs_icp_ref_destroy(view.h)
    view.close()
    assert view.h and bytes(rset[1].refine(S, STARTS[0], p)) == bytes(want)
    for h in (one, rset, again, lone, other):
        h.close()


# ------------------------------------------------------------------ 3. launch counts
@pytest.mark.parametrize("n_refs", [4, 40])
def test_the_build_is_one_launch_per_kernel_and_two_waits(ctx, world, n_refs):
    refs, poses, _ = scene_scans(world, 65, 7)
    p = abi.IcpParams(*prm_for(65))
    scans = [dev_scan(ctx, r) for r in refs]
    lo = [i % 6 for i in range(n_refs)]
    hi = [min(6, a + i % 3) for i, a in enumerate(lo)]
    before = ctx.icp_ref_set_stats()
    rset = ctx.icp_ref_set(scans, poses, lo, hi, p)
    after = ctx.icp_ref_set_stats()
    delta = [b - a for a, b in zip(before, after)]
    assert delta == [1, 1, 1, 1, 1, 2, 0], dict(zip(after._fields, delta))
    assert len(rset) == n_refs
    # spot checks: the last reference and one in the middle are what create makes of their ranges
    for i in (n_refs - 1, n_refs // 2):
        lone = ctx.icp_ref(scans[lo[i]:hi[i] + 1], poses[lo[i]:hi[i] + 1], p)
        assert rset[i].info() == lone.info()
        lone.close()
    rset.close()


# ------------------------------------------------------------------ 4. argument checks
def raw_create(ctx, scans, poses, lo, hi, prm, null=None, n_scans=None, n_refs=None):
    """lgs_icp_ref_set_create on a poisoned out pointer; (status, untouched)"""
    P = abi.Pose2D
    p = abi.IcpParams(*prm)
    arr = (C.c_void_p * max(1, len(scans)))(*[s.h if s is not None else None for s in scans])
    ps = (P * max(1, len(poses)))(*[P(*q) for q in poses])
    a = dict(ctx=ctx.h, scans=arr, poses=ps, lo=(C.c_int * max(1, len(lo)))(*lo), hi=(C.c_int * max(1, len(hi)))(*hi),
             prm=C.byref(p), out=None)
    out = C.c_void_p(0xABABABAB)
    a["out"] = C.byref(out)
    if null:
        a[null] = None
    st = ctx.lib.lgs_icp_ref_set_create(a["ctx"], a["scans"], a["poses"], len(scans) if n_scans is None else n_scans,
                                        a["lo"], a["hi"], len(lo) if n_refs is None else n_refs, a["prm"], a["out"])
    untouched = out.value == 0xABABABAB
    if st == 0:
        ctx.lib.lgs_icp_ref_set_destroy(out)
    return st, untouched


GOOD = orc.Params(5, 0.0, 0.01, 20.0, 1e-3, 1e-3, 1.0, 0.5)
BAD = (LGS_ERR_INVALID_ARG, True)
NAN, INF = float("nan"), float("inf")


def test_invalid_arguments_are_refused_before_any_device_work(ctx, world):
    refs, poses, _ = scene_scans(world, 65, 7)
    R = [dev_scan(ctx, r) for r in refs[:3]]
    P3 = poses[:3]
    before = ctx.icp_ref_set_stats()
    assert raw_create(ctx, R, P3, [0, 1], [1, 2], GOOD) == (0, False)
    assert ctx.icp_ref_set_stats().builds == before.builds + 1
    before = ctx.icp_ref_set_stats()
    for null in ("ctx", "scans", "poses", "lo", "hi", "prm", "out"):
        st, untouched = raw_create(ctx, R, P3, [0], [1], GOOD, null=null)
        assert st == LGS_ERR_INVALID_ARG and (untouched or null == "out"), null
    assert raw_create(ctx, R, P3, [0], [1], GOOD, n_refs=0) == BAD
    assert raw_create(ctx, R, P3, [0], [1], GOOD, n_refs=-1) == BAD
    assert raw_create(ctx, R, P3, [0] * 4097, [1] * 4097, GOOD) == BAD
    assert raw_create(ctx, R, P3, [0], [1], GOOD, n_scans=0) == BAD
    assert raw_create(ctx, R, P3, [0, 1], [1, 3], GOOD) == BAD      # idx_max == n_scans
    assert raw_create(ctx, R, P3, [-1], [1], GOOD) == BAD
    assert raw_create(ctx, R, P3, [2], [1], GOOD) == BAD            # idx_min > idx_max
    assert raw_create(ctx, [R[0]] * 4097, [O] * 4097, [0], [4096], GOOD) == BAD   # 4097 scans in a reference
    assert raw_create(ctx, [R[0], None, R[2]], P3, [0], [1], GOOD) == BAD         # a NULL scan inside a range
    assert raw_create(ctx, [R[0], None, R[2]], P3, [0, 2], [0, 2], GOOD) == (0, False)   # outside every range
    for bad in ((NAN, 0.0, 0.0), (0.0, INF, 0.0), (0.0, 0.0, NAN)):
        assert raw_create(ctx, R, [P3[0], bad, P3[2]], [0], [1], GOOD) == BAD
    assert raw_create(ctx, R, [P3[0], (NAN, 0.0, 0.0), P3[2]], [0, 2], [0, 2], GOOD) == (0, False)
    for prm in (GOOD._replace(max_correspondence_dist=0.0), GOOD._replace(max_segment_length=NAN),
                GOOD._replace(usable_range_max=INF), GOOD._replace(rotation_regularizer=-1.0)):
        assert raw_create(ctx, R, P3, [0], [1], prm) == BAD
    after = ctx.icp_ref_set_stats()
    assert after.builds == before.builds + 2 and after.table_launches == before.table_launches + 2
    # the sincos domain: LGS_ERR_INTERNAL, as lgs_icp_ref_create
    assert raw_create(ctx, R, [P3[0], (0.0, 0.0, 2.0e8), P3[2]], [0, 1], [0, 1], GOOD) == (LGS_ERR_INTERNAL, True)
    assert raw_create(ctx, R, P3, [0, 1], [1, 2], GOOD) == (0, False)


def test_the_entry_caps(ctx):
    """a scan of 4200 usable beams, 62 times: 260400 entries per reference are legal, 17 such references are
    4426800 > LGS_ICP_REF_SET_MAX_ENTRIES and refused before any device work; 63 copies in one reference exceed
    lgs_icp_ref_create's own cap"""
    ang = np.linspace(-2.0, 2.0, 4203)
    rng = 4.0 + 0.5 * np.sin(7.0 * ang)
    rng[[10, 2000, 4000]] = 25.0
    s = ctx.scan(rng, ang)
    before = ctx.icp_ref_set_stats()
    assert raw_create(ctx, [s] * 62, [O] * 62, [0] * 17, [61] * 17, GOOD) == BAD
    assert raw_create(ctx, [s] * 63, [O] * 63, [0], [62], GOOD) == BAD
    assert ctx.icp_ref_set_stats() == before
    rset = ctx.icp_ref_set([s] * 62, [O] * 62, [0, 60], [61, 61], abi.IcpParams(*GOOD))
    assert rset[0].info().entries == 260400 and rset[1].info().entries == 8400
    lone = ctx.icp_ref([s, s], [O, O], abi.IcpParams(*GOOD))
    assert rset[1].info() == lone.info()
    cur = ctx.scan(rng[::50].copy(), ang[::50].copy())
    p = abi.IcpParams(*GOOD)
    a, b = rset[1].pairs(cur, (0.02, -0.01, 0.003), p), lone.pairs(cur, (0.02, -0.01, 0.003), p)
    assert [x.tobytes() for x in a] == [x.tobytes() for x in b] and (a[0] == 0).sum() > 50   # ties go to copy 0
    k, _, _ = rset[0].pairs(cur, (0.02, -0.01, 0.003), p)
    assert (k == 0).sum() > 50 and set(k[k >= 0].tolist()) == {0}
    rset.close()


def test_the_cell_cap_is_out_of_memory_after_the_table_pass(ctx):
    """a bare 24 m room seen from its centre, D = 1e-3: 1024 cells per axis; 17 such references are more than
    LGS_ICP_REF_SET_MAX_CELLS.  The refusal comes after the table pass, leaks nothing the context needs and
    leaves it usable"""
    h = 12.0
    walls = np.array([(-h, -h, h, -h), (h, -h, h, h), (h, h, -h, h), (-h, h, -h, -h)], dtype=np.float64)
    ang = scene.beam_angles(65)
    s = ctx.scan(scene.ray_cast(walls, O, ang), ang)
    prm = GOOD._replace(max_correspondence_dist=1e-3)
    lone = ctx.icp_ref([s], [O], abi.IcpParams(*prm))
    info = lone.info()
    assert info.entries == 65 and info.cells_x * info.cells_y * 17 > 16777216 >= info.cells_x * info.cells_y * 2
    before = ctx.icp_ref_set_stats()
    assert raw_create(ctx, [s], [O], [0] * 17, [0] * 17, prm) == (LGS_ERR_OOM, True)
    after = ctx.icp_ref_set_stats()
    assert (after.table_launches, after.count_launches, after.build_syncs) == \
        (before.table_launches + 1, before.count_launches, before.build_syncs + 1)
    assert b"LGS_ICP_REF_SET_MAX_CELLS" in ctx.lib.lgs_ctx_last_error(ctx.h)
    # the same context builds the next set, two such references included
    rset = ctx.icp_ref_set([s], [O], [0, 0], [0, 0], abi.IcpParams(*prm))
    assert rset[0].info() == rset[1].info() == info
    cur = ctx.scan(scene.ray_cast(walls, (0.0002, -0.0003, 0.0), ang), ang)
    a, b = rset[1].pairs(cur, (0.0002, -0.0003, 0.0), abi.IcpParams(*prm)), lone.pairs(cur, (0.0002, -0.0003, 0.0), abi.IcpParams(*prm))
    assert [x.tobytes() for x in a] == [x.tobytes() for x in b]
    rset.close()
