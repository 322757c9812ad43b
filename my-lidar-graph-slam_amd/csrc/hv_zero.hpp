// hv_zero.hpp -- which precompute tiles a k_super_hv thread's loads can depend
// on (k_rtcsm.hip, "Zero tiles").  Shared by the device (k_hv_inzero) and a
// stand-alone host check (tests/cpp_hv/hv_zero_check.cpp), so plain C++ with
// the HIP qualifiers only where a HIP compiler reads it.
#pragma once

#if defined(__HIPCC__)
#define LGS_HV_HD __host__ __device__
#else
#define LGS_HV_HD
#endif

namespace lgs {

// The tiling of the precompute launch that wrote a set's planes: pgx x pgy
// tiles of pcols fine columns x prows fine rows (pcols = pqx_of(LR) * LR; a
// batch: 8 rows, a lone map: 4), over a W x H map.
struct HvTiling {
    int pgx, pgy, prows, pcols, W, H;
};

// Inclusive tile rows / columns; empty (ty0 > ty1): every load is a margin cell.
struct HvTileRange {
    int ty0, ty1, tx0, tx1;
    LGS_HV_HD bool empty() const { return ty0 > ty1 || tx0 > tx1; }
};

// Fine columns per precompute tile (lgs_core.hip: pqx_of(LR) * LR, asserted there).
LGS_HV_HD constexpr int hv_pcols(int lr) { return (((257 - lr) / lr) & ~1) * lr; }

// One padded axis: cells [a, b] of planes with margin M and n interior cells,
// phase count lr, map extent `ext`, `per` fine cells per tile, `nt` tiles.
// Padded cell Y of phase r is fine cell lr (Y - M) + r, so the fine interval
// is the same for every plane.  Cell M - 1 counts as M: the strip clamp reads
// the map's first coarse row / column there.  Conservative: the interval only
// ever grows (the strip is taken whether or not this thread reads it).
LGS_HV_HD inline void hv_axis_range(int a, int b, int M, int n, int lr, int ext, int per, int nt, int* t0, int* t1)
{
    *t0 = 1;
    *t1 = 0;
    if (b < M - 1 || a >= M + n || n <= 0) return;   // margins only
    const int lo = (a > M ? a : M) - M;
    int hi = (b > M ? b : M);
    if (hi > M + n - 1) hi = M + n - 1;
    hi -= M;
    const int f0 = lo * lr;
    int f1 = hi * lr + lr - 1;
    if (f0 >= ext) return;                           // past the map: never written, +0
    if (f1 > ext - 1) f1 = ext - 1;
    *t0 = f0 / per;
    *t1 = f1 / per;
    if (*t1 > nt - 1) *t1 = nt - 1;                  // (f1 < ext <= nt * per: never taken; keeps the range in the grid)
}

// Thread (quad qt, unit column X4) of k_super_hv<nq>: it loads padded rows
// 16 qt .. 16 qt + 16 nq + 2 at columns 4 X4 .. 4 X4 + 6 of every plane.
LGS_HV_HD inline HvTileRange hv_zero_range(int qt, int X4, int nq, int M, int Wq, int Hq, int lr, const HvTiling& t)
{
    HvTileRange r;
    hv_axis_range(16 * qt, 16 * qt + 16 * nq + 2, M, Hq, lr, t.H, t.prows, t.pgy, &r.ty0, &r.ty1);
    hv_axis_range(4 * X4, 4 * X4 + 6, M, Wq, lr, t.W, t.pcols, t.pgx, &r.tx0, &r.tx1);
    if (r.empty()) {
        r.ty0 = r.tx0 = 1;
        r.ty1 = r.tx1 = 0;
    }
    return r;
}

}  // namespace lgs
