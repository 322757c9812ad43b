// icp_ref_host.hpp -- the pieces of the multi-scan point-to-line ICP reference
// (k_icp_ref.hip) that need no device: the limits, the
// parameters a reference is bound to, the geometry of the uniform grid over
// the table's points, and the cell function with its clamping, which the
// device uses unchanged (__host__ __device__).  Plain C++ when compiled
// without HIP, so that tests/cpp_icp_ref/icp_ref_host_check.cpp runs it on its
// own under the sanitizers.
//
// Why the 3 x 3 neighbourhood of a hit point's cell holds every entry that can
// be accepted (DESIGN.md 4.5c has the argument in full): per axis the cell of
// x is floor(t(x)), t(x) = fl(fl(x - o) * ic), ic = fl(1 / c).  An accepted
// entry q of hit point h has computed d2 <= D2 = fl(D * D), so fl(dx * dx) <=
// fl(D * D) with dx = fl(hx - qx), hence |hx - qx| <= Dm (1 + 3u), Dm =
// max(D, 2^-400), u = 2^-53.  With c >= Dm (1 + 2^-10)(1 - u) and at most
// 1024 cells per axis, |t(h) - t(q)| <= (1 + 3u) / ((1 + 2^-10)(1 - u)) +
// 3.1 u (2 * 1025 + 1) + 2^-1073 < 1, and two numbers less than 1 apart have
// floors at most 1 apart.
#pragma once

#include <cmath>
#include <cstring>

#include "icp_host.hpp"

#if defined(__HIPCC__)
#define LGS_ICP_HD __host__ __device__
#else
#define LGS_ICP_HD
#endif

namespace lgs {

constexpr int kIcpRefMaxScans = 4096;
constexpr int kIcpRefMaxEntries = LGS_ICP_REF_MAX_ENTRIES;
constexpr int kIcpRefMaxCells = 1024;          // per axis
constexpr double kIcpRefMinDist = 0x1p-400;    // Dm's floor: below it D * D underflows
constexpr double kIcpRefCellFactor = 1.0009765625;   // 1 + 2^-10
constexpr double kIcpRefMaxExtent = 1e300;     // beyond it an axis is one cell (x - o may overflow)

// one axis of the grid
struct IcpRefAxis {
    double o;    // the smallest finite coordinate of the table
    double ic;   // fl(1 / c); 0: the axis is one cell whatever x is (empty table, extent beyond kIcpRefMaxExtent)
    int n;       // cells, 1 .. kIcpRefMaxCells
};

struct IcpRefGrid {
    IcpRefAxis x, y;
    double c;    // the cell side of both axes
};

// t(x), clamped in fp64: the cell of x, -1 .. n for a point that may have an
// entry within reach (its neighbourhood is then clipped to 0 .. n - 1), or
// kIcpRefNoCell for NaN, +-inf and everything farther out.  The conversion to
// int sees only values in [-1, n + 1).
constexpr int kIcpRefNoCell = -2;
LGS_ICP_HD inline int icp_ref_cell(const IcpRefAxis& a, double x)
{
    if (a.ic == 0.0) return x - x == 0.0 ? 0 : kIcpRefNoCell;   // one cell for every finite x
    const double t = (x - a.o) * a.ic;
    if (!(t >= -1.0 && t < (double)(a.n + 1))) return kIcpRefNoCell;
    return (int)floor(t);
}

// The cells a hit point visits: rows y0 .. y1, and in every row the columns
// x0 .. x1 (one contiguous range in row-major cell order).  False: none.
LGS_ICP_HD inline bool icp_ref_visit(const IcpRefGrid& g, double hx, double hy, int& x0, int& x1, int& y0, int& y1)
{
    const int cx = icp_ref_cell(g.x, hx), cy = icp_ref_cell(g.y, hy);
    if (cx == kIcpRefNoCell || cy == kIcpRefNoCell) return false;
    x0 = cx - 1 < 0 ? 0 : cx - 1;
    x1 = cx + 1 > g.x.n - 1 ? g.x.n - 1 : cx + 1;
    y0 = cy - 1 < 0 ? 0 : cy - 1;
    y1 = cy + 1 > g.y.n - 1 ? g.y.n - 1 : cy + 1;
    return x0 <= x1 && y0 <= y1;
}

// cells of [lo, hi] with side c by the cell function itself, so that every
// coordinate of the table lands in 0 .. n - 1 (fl is monotone)
inline double icp_ref_axis_cells(double lo, double hi, double c)
{
    return std::floor((hi - lo) * (1.0 / c)) + 1.0;
}

// The grid of a table whose finite points span [min_x, max_x] x [min_y, max_y]
// (min > max: no finite point) for max_correspondence_dist D.
inline IcpRefGrid icp_ref_geometry(double min_x, double max_x, double min_y, double max_y, double D)
{
    IcpRefGrid g;
    const double dm = D > kIcpRefMinDist ? D : kIcpRefMinDist;
    double c = dm * kIcpRefCellFactor;
    const bool any = min_x <= max_x && min_y <= max_y;
    const double ex = any ? max_x - min_x : 0.0, ey = any ? max_y - min_y : 0.0;
    const bool wide_x = !(ex <= kIcpRefMaxExtent), wide_y = !(ey <= kIcpRefMaxExtent);
    // enlarge c until neither axis needs more than kIcpRefMaxCells
    const double e = std::fmax(wide_x ? 0.0 : ex, wide_y ? 0.0 : ey);
    if (e / (double)kIcpRefMaxCells * kIcpRefCellFactor > c) c = e / (double)kIcpRefMaxCells * kIcpRefCellFactor;
    while ((!wide_x && icp_ref_axis_cells(min_x, max_x, c) > (double)kIcpRefMaxCells) ||
           (!wide_y && icp_ref_axis_cells(min_y, max_y, c) > (double)kIcpRefMaxCells))
        c = c * 2.0;
    g.c = c;
    const double ic = 1.0 / c;
    g.x.o = any ? min_x : 0.0;
    g.y.o = any ? min_y : 0.0;
    g.x.ic = (any && !wide_x) ? ic : 0.0;
    g.y.ic = (any && !wide_y) ? ic : 0.0;
    g.x.n = (any && !wide_x) ? (int)icp_ref_axis_cells(min_x, max_x, c) : 1;
    g.y.n = (any && !wide_y) ? (int)icp_ref_axis_cells(min_y, max_y, c) : 1;
    return g;
}

// the parameters a reference's table and grid were made for
struct IcpRefBound {
    double usable_range_min, usable_range_max, max_segment_length, max_correspondence_dist;
};
inline IcpRefBound icp_ref_bound(const lgs_icp_params* p)
{
    return { p->usable_range_min, p->usable_range_max, p->max_segment_length, p->max_correspondence_dist };
}
// refine-time parameters must carry the same bits
inline bool icp_ref_bound_same(const IcpRefBound& b, const lgs_icp_params* p)
{
    const IcpRefBound q = icp_ref_bound(p);
    return std::memcmp(&b, &q, sizeof(b)) == 0;
}

// LGS_OK or LGS_ERR_INVALID_ARG: lgs_icp_ref_create's checks that need only
// the counts (usable[k]: usable beams of reference scan k, null: not counted yet)
inline int icp_ref_counts_check(int n_refs, const int* usable)
{
    if (n_refs < 1 || n_refs > kIcpRefMaxScans) return LGS_ERR_INVALID_ARG;
    long long total = 0;
    for (int k = 0; usable && k < n_refs; ++k) {
        if (usable[k] < 0) return LGS_ERR_INVALID_ARG;
        total += usable[k];
    }
    return total > (long long)kIcpRefMaxEntries ? LGS_ERR_INVALID_ARG : LGS_OK;
}

}  // namespace lgs
