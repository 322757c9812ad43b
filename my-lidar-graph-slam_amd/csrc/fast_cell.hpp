// Certified fast projection of a hit point to its grid cell (DESIGN.md §4.2b
// "certified fast rows").  k_super_oct needs, per (search angle, beam), only
// the integer cell of the hit point and the knowledge that the exact chain
// (k_project's arithmetic, lean_cell) would not have raised a projection
// guard there.  The fast chain below reaches the quotient q' with 3 fp64
// operations per axis instead of 8, |q' - q| <= E against the exact chain's q
// (E derived in DESIGN.md §4.2b), and calls a cell *certain* only when q' is
// farther than band = geps + |q'| 1e-13 + E (+ rounding slack) from both
// neighbouring integers.  Then floor(q') == floor(q) and the exact guard test
// (near_boundary) is false.  Anything else -- NaN, infinities, huge
// magnitudes, a quotient near a cell boundary -- is uncertain, and the caller
// runs the exact chain.
//
// Compiles for the host too (tests/fast_cell_check.cpp compares it with the
// exact chain on the CPU).  Every fused multiply-add is an explicit fma(): the
// library is built with -ffp-contract=off.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LGS_FC_HD __host__ __device__ __forceinline__
#else
#define LGS_FC_HD inline
#endif

namespace lgs_fast {

// magnitudes (in cells) below which the fast chain is used at all: |r / res|,
// |(s - min) / res| and the search window's half-widths.  The cell index is
// then below 2^21 + 1 and a lattice coordinate (index - window start) below
// 2^22 in magnitude: the fp32 floor_divmod below is exact there.
constexpr double kMaxCells = 1048576.0;   // 2^20

// E <= kErr (|r| + |s| + |min|) / res per axis: 16 x 2^-53 (the derivation
// gives 11 x 2^-53 (1 + O(2^-53)))
constexpr double kErr = 0x1p-49;
// the guard's relative term 1e-13, widened so that it also holds for |q| <=
// |q'| + E and for the exact test's own roundings of |q| 1e-13
constexpr double kRel = 1.01e-13;
// absolute slack for the roundings of the band itself, of 1 - e in the exact
// test and of f' - 0.5 here (each <= 2^-53)
constexpr double kAbs = 2e-15;

// Per valid beam (k_beams, the fourth lane of btab): r / res, or NaN when the
// fast chain may not be used for this beam (NaN, infinite or huge range).
LGS_FC_HD double beam_rs(double r, double inv_res)
{
    const double w = r * inv_res;
    return (std::fabs(w) < kMaxCells) ? w : NAN;
}

// Per item: o = (s - min) / res per axis and h0 = 0.5 - (the part of the band
// that does not depend on the beam).  A beam's half-width is then
// hb = h0 - |rs| (kRel + kErr) and a quotient q' is certain on an axis when
// |frac(q') - 0.5| <= hb.  h0 is NaN (nothing is ever certain) when a
// magnitude is outside the fast chain's range.
struct ItemConsts {
    double ox, oy, h0;
};
LGS_FC_HD ItemConsts item_consts(double sx, double sy, double min_x, double min_y, double inv_res, double geps,
                                 int win_x, int win_y)
{
    ItemConsts k;
    k.ox = (sx - min_x) * inv_res;
    k.oy = (sy - min_y) * inv_res;
    const double mo = std::fmax(std::fabs(k.ox), std::fabs(k.oy));
    const double ms = std::fmax(std::fabs(sx) + std::fabs(min_x), std::fabs(sy) + std::fabs(min_y)) * inv_res;
    const double band0 = geps + kAbs + kRel * mo + kErr * ms;
    const bool ok = mo < kMaxCells && ms < 4.0 * kMaxCells && geps >= 0.0 && band0 < 0.5 &&
                    std::fabs((double)win_x) < kMaxCells && std::fabs((double)win_y) < kMaxCells;
    k.h0 = ok ? 0.5 - band0 : NAN;
    return k;
}

// The cell of (search angle (ct, st), beam (ca, sa, rs)); ctca = ct * ca and
// stca = st * ca are passed in (the exact chain forms the same two products,
// so a caller that may need both chains multiplies once).  Returns true when
// the cell is certain on both axes; ix, iy are meaningful only then.
LGS_FC_HD bool cell(double ct, double st, double sa, double ctca, double stca, double rs, double ox, double oy,
                    double h0, int& ix, int& iy)
{
    const double c = fma(-st, sa, ctca);
    const double s = fma(ct, sa, stca);
    const double qx = fma(rs, c, ox);
    const double qy = fma(rs, s, oy);
    const double fx = floor(qx), fy = floor(qy);
    const double hb = fma(-std::fabs(rs), kRel + kErr, h0);
    const double dx = (qx - fx) - 0.5, dy = (qy - fy) - 0.5;
    // NaN anywhere (rs, h0, an infinite quotient's fraction) compares false
    const bool certain = (std::fabs(dx) <= hb) && (std::fabs(dy) <= hb);
    // |q'| <= |rs| + |o| < 2^21 whenever certain: the conversions are exact
    ix = (int)fx;
    iy = (int)fy;
    return certain;
}

// floor(a / b) and the remainder in [0, b) for |a| < 2^22, b >= 1, inv_b =
// 1.0f / (float)b: (float)a is exact, the product's relative error is below
// 3 x 2^-24, so its floor misses floor(a / b) by at most 1, which the
// remainder test repairs (as the fp64 floor_divmod of k_rtcsm.hip does).
LGS_FC_HD void floor_divmod22(int a, int b, float inv_b, int& q, int& r)
{
    q = (int)floorf((float)a * inv_b);
#if defined(__HIP_DEVICE_COMPILE__)
    r = a - __mul24(q, b);   // |q| < 2^22 + 1, b < 2^23: the 24-bit product is the product
#else
    r = a - q * b;
#endif
    const int lo = r < 0 ? 1 : 0, hi = r >= b ? 1 : 0;   // branch-free: at most one is set
    q += hi - lo;
    r += lo ? b : (hi ? -b : 0);
}

}   // namespace lgs_fast
