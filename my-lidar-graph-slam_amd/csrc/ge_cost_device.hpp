// ge_cost_device.hpp -- the per-beam term of CostGreedyEndpoint::Cost
// (C/mapping/cost_function_greedy_endpoint.cpp:32-111) and its beam-order
// chain as device functions, with the host code of the term table.  Shared by
// k_hc.hip (k_hc, k_hc_cost, k_ge_cost_batch) and by the correlative
// pipeline's exact cost stage (k_rtcsm.hip k_cost_gx), so that every caller
// compiles the same arithmetic.  As sq_cost_device.hpp: no relocatable device
// code, everything forced inline, one copy per translation unit.  DESIGN.md
// §4.6c has the exactness argument.
#pragma once

#include "lgs_internal.hpp"
#include "glibc_math.hpp"

#include <cmath>
#include <vector>

namespace {

constexpr int kHCMaxKernel = 16;             // documented cap of kernel_size

// One match of a launch (device memory).
struct HCItem {
    double sx, sy, st;          // sensor pose (Compound(initialPose, relPose))
    double min_x, min_y, res;   // map geometry
    double min_range, max_range;
    int W, H, N, pad;
    const double* map;
    const double* ranges;
    const double* angles;
    double* rows;               // term rows when they do not fit LDS
    int* trace_move;            // [pass cap] or null
    double* trace_cost;
    const double* tab;          // k_ge_cost_batch: the term table of the item's resolution (lgs_ctx::ge_table)
};

// What every match of a launch shares.
struct HCShared {
    double lin_step, ang_step;
    double hit_and_missed_dist, occupancy_threshold, scaling_factor;
    const double* sq;           // lgs_hc_term_table, device copy
    const double* term;
    int max_iterations, max_refinements, K, trace_cap;
    unsigned lds_bytes;         // dynamic LDS of the launch
};

// GridMap::Value(idx, unknown) on the dense view: outside the map unknown (0)
__device__ __forceinline__ double hc_gval(const double* __restrict__ g, int W, int H, int x, int y)
{
    const bool inb = ((unsigned)x < (unsigned)W) & ((unsigned)y < (unsigned)H);
    const size_t off = inb ? (size_t)y * W + x : 0;
    const double v = gload(g + off);
    return inb ? v : 0.0;
}

// WorldCoordinateToGridCellIndex (H/grid_map/grid_map.hpp:779-790) of one
// coordinate.  Quotients beyond +-2^30 (no map has that many cells per axis)
// are held there so that cell + k cannot wrap.
__device__ __forceinline__ int hc_cell(double v, double mn, double res)
{
    const double f = floor((v - mn) / res);
    return (int)fmin(fmax(f, -1073741824.0), 1073741824.0);
}

// The term of beam i at sensor pose (px, py, pt): exp(-0.5 * minSquaredDist /
// variance) as the table holds it (:50-101), +0.0 for a filtered beam
template <int KS>
__device__ __forceinline__ double hc_term(const HCItem& it, const HCShared& sh, int i, double px, double py, double pt,
                                          int* __restrict__ err)
{
    const double r = gload(it.ranges + i);
    if (r >= it.max_range || r <= it.min_range) return 0.0;   // :52-53
    // HitAndMissedPoint (H/sensor/sensor_data.hpp:177-198): one glibc sincos
    const double th = pt + gload(it.angles + i);
    if (!glm::gl_sincos_ok(th)) *err = 1;
    double sn, cs;
    glm::gl_sincos(th, &sn, &cs);
    const double hx = px + r * cs;
    const double hy = py + r * sn;
    const double rm = r - sh.hit_and_missed_dist;
    const double mx = px + rm * cs;
    const double my = py + rm * sn;
    const int hix = hc_cell(hx, it.min_x, it.res), hiy = hc_cell(hy, it.min_y, it.res);
    const int mix = hc_cell(mx, it.min_x, it.res), miy = hc_cell(my, it.min_y, it.res);
    const double* __restrict__ map = it.map;
    const double* __restrict__ tsq = sh.sq;
    const double* __restrict__ tterm = sh.term;
    const int K = KS > 0 ? KS : sh.K;
    const int D = 2 * K + 1;
    double minSq = tsq[D * D];        // SquaredDistance(0, 0, K + 1, K + 1) (:66-67)
    double term = tterm[D * D];
    if constexpr (KS > 0) {
        // every cell value loaded before any test: the loads are independent
        constexpr int DD = (2 * KS + 1) * (2 * KS + 1);
        double hv[DD], mv[DD];
#pragma unroll
        for (int q = 0; q < DD; ++q) {
            hv[q] = hc_gval(map, it.W, it.H, hix + q % (2 * KS + 1) - KS, hiy + q / (2 * KS + 1) - KS);
            mv[q] = hc_gval(map, it.W, it.H, mix + q % (2 * KS + 1) - KS, miy + q / (2 * KS + 1) - KS);
        }
#pragma unroll
        for (int q = 0; q < DD; ++q) {   // ky outer, kx inner
            if (hv[q] == 0.0 || mv[q] == 0.0) continue;                                          // :82-84
            if (hv[q] < sh.occupancy_threshold || mv[q] > sh.occupancy_threshold) continue;      // :89-92
            const double sq = tsq[q];
            if (!(minSq < sq)) {   // std::min(sq, minSq) (:94-96)
                minSq = sq;
                term = tterm[q];
            }
        }
    } else {
        int q = 0;
        for (int ky = -K; ky <= K; ++ky)
            for (int kx = -K; kx <= K; ++kx, ++q) {
                const double hv = hc_gval(map, it.W, it.H, hix + kx, hiy + ky);
                const double mv = hc_gval(map, it.W, it.H, mix + kx, miy + ky);
                if (hv == 0.0 || mv == 0.0) continue;
                if (hv < sh.occupancy_threshold || mv > sh.occupancy_threshold) continue;
                const double sq = tsq[q];
                if (!(minSq < sq)) {
                    minSq = sq;
                    term = tterm[q];
                }
            }
    }
    return term;
}

// costValue = 0; costValue -= term, beams in order; costValue *= scale (:45, :101-104)
__device__ __forceinline__ double hc_chain(const double* __restrict__ row, int N, double scale)
{
    double c = 0.0;
    int i = 0;
    for (; i + 8 <= N; i += 8) {
        double t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = row[i + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) c -= t[j];
    }
    for (; i < N; ++i) c -= row[i];
    c *= scale;
    return c;
}

// ------------------------------------------------------------------ host
// entries of a term table: the (2K + 1)^2 kernel offsets, then the start value
__host__ __device__ inline int hc_table_len(int K) { return (2 * K + 1) * (2 * K + 1) + 1; }

// GridMap::SquaredDistance (H/grid_map/grid_map.hpp:894-902) of every kernel
// offset, then of (K + 1, K + 1); exp(-0.5 * sq / variance) with libm's exp (:101)
inline void hc_table(const lgs_cost_ge_params* c, double res, std::vector<double>& sq, std::vector<double>& term)
{
    const int K = c->kernel_size;
    const double variance = c->standard_deviation * c->standard_deviation;
    sq.clear();
    for (int ky = -K; ky <= K; ++ky)
        for (int kx = -K; kx <= K; ++kx) {
            const double dX = kx * res, dY = ky * res;
            sq.push_back(dX * dX + dY * dY);
        }
    const double d = (K + 1) * res;
    sq.push_back(d * d + d * d);
    term.resize(sq.size());
    for (size_t q = 0; q < sq.size(); ++q) term[q] = std::exp(-0.5 * sq[q] / variance);
}

}  // namespace
