// coarse_pair.hpp -- when k_coarse_list_p (k_rtcsm.hip) may read a pair of
// neighbouring coarse blocks with one 16-byte load.  Shared by the host's
// kernel choice and a stand-alone host check (tests/cpp_coarse_pair), so plain
// C++.
#pragma once

namespace lgs {

// The padded phase-plane layout of a plan (set_plane_layout) and the window's
// coarse lattice, as far as a coarse read depends on them.  `alloc` is the
// number of doubles of one set's plane allocation (plane_bytes / 8).
struct CoarsePairGeom {
    int low_res, Wq, Hq, M, Wqp, Hqp, ncx, ncy;
    long long pstride, alloc;
};

// A pair lane owns blocks (jx, jy) and (jx + 1, jy), jx even, jx < ncx,
// jy < ncy, and reads the two doubles at base + jy * Wqp + jx of its beam;
// with an odd ncx block (ncx, jy) does not exist, its value is read and
// dropped.  A beam's base is 0 (its window misses the map) or plane (ry, rx)
// at (qy0 + M, qx0 + M) with -ncx < qx0 < Wq, -ncy < qy0 < Hq
// (coarse_base_l).  The largest index read is therefore the second double of
// the last pair of the last lattice row, for the last plane's last in-map
// lattice start; every read lies inside the allocation iff that one does.
inline long long coarse_pair_last_read(const CoarsePairGeom& g)
{
    const long long lastpair = (g.ncx - 1) & ~1;   // the largest even jx below ncx
    return (long long)(g.low_res * g.low_res - 1) * g.pstride + (long long)(g.Hq - 1 + g.M + g.ncy - 1) * g.Wqp +
           (g.Wq - 1 + g.M) + lastpair + 1;
}
inline bool coarse_pair_read_inside(const CoarsePairGeom& g)
{
    if (g.low_res < 1 || g.Wq < 1 || g.Hq < 1 || g.ncx < 1 || g.ncy < 1 || g.M < 0) return false;
    return coarse_pair_last_read(g) < g.alloc;
}

}   // namespace lgs
