"""The host restatement of the pruning bounds (tests/prune_oracle.py) checked
on itself, without a GPU: on every scene of tests/test_gpu_prune_invariants.py
the ideal bound is sound, something can be pruned, and the scenes declared
"low-edge" hold blocks whose coarse score does not bound their fine scores --
all of them in angles the edge rule flags.  Every comparison is exact."""
import numpy as np
import pytest

import prune_oracle as po


@pytest.mark.parametrize("name", sorted(po.SCENE_BUILDERS))
def test_restatement_is_sound_and_not_vacuous(name):
    s, o = po.scene_inputs(name), po.scene_oracle(name)
    assert o.U.shape == o.cmax.shape == o.fmax.shape == (o.T, o.nsb2)
    # the reference itself is sound
    assert (o.U >= o.cmax).all(), np.argwhere(o.U < o.cmax)[:4]
    assert (o.Ustrip >= o.U).all()
    # not vacuous: some superblock can be pruned by a seed that found the final score
    assert (o.U < o.fs.max()).any()
    # the strip changes a bound only where a beam's lattice starts left of / below the map
    assert (o.U[~o.edge] == o.Ustrip[~o.edge]).all()
    # a block's coarse score bounds its fine scores in every angle the edge rule does not flag
    un = o.unsafe_blocks()
    assert not un[~o.edge].any()
    # partial superblocks, and the members' clipping
    assert o.members().sum() == o.ncx * o.ncy
    if s["low_edge"]:
        assert un.any()
        # what keeps the pruning exact there (DESIGN.md §4.1b "Low map edges"): the
        # strip-clamped bound covers the fine scores the coarse score misses
        assert (o.Ustrip >= o.fmax).all()
    else:
        assert not un.any()


def test_scene_table_reaches_the_edges():
    """The shapes the invariant tests rely on: partial superblocks, both octet
    unit sizes and the fp16 planes, a map no multiple of LowRes, a beam count
    that fills neither 64 lanes nor 4 waves, angles with and without edge
    beams in one search, and the noise map's special values."""
    o = {n: po.scene_oracle(n) for n in po.SCENE_BUILDERS}
    assert all(x.ncx % po.SB or x.ncy % po.SB for x in o.values())
    assert (o["room"].layout["oct"], o["room"].layout["unit8"]) == (True, 2)
    assert (o["win6x6"].layout["oct"], o["win6x6"].layout["unit8"]) == (True, 3)
    assert (o["win6x6"].nsbx, o["win6x6"].nsby) == (6, 6)
    assert not o["aniso"].layout["oct"] and (o["aniso"].nsbx, o["aniso"].nsby) == (10, 2)
    h, w = po.scene_inputs("oddmap")["cells"].shape
    assert w % 5 and h % 5
    assert o["noise"].Nv % 64 and o["noise"].Nv % 4 and o["beams181"].Nv < 181
    assert 0 < o["room"].edge.sum() < o["room"].T
    cells = po.scene_inputs("noise")["cells"]
    assert cells.min() == 0.0 and cells.max() == 1.0
    for v in (1.0, 0.0, 2.0 ** -24, 2.0 ** -25, 1e-30):
        assert (cells == v).any(), v
    # no slack between the ideal bound and the best member in some full superblock that is not empty
    for n in ("ones", "ones_wide", "half062", "half062_wide", "half062_6x6"):
        full = (o[n].members() == po.SB * po.SB)[None, :] & (o[n].U == o[n].cmax) & (o[n].U > 0)
        assert full.any(), n
    for n in po.SCENE_BUILDERS:
        h, w = po.scene_inputs(n)["cells"].shape
        assert 200 <= min(h, w) and max(h, w) <= 400, n
