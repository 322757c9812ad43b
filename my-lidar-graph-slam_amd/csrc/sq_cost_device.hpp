// sq_cost_device.hpp -- the per-beam arithmetic of CostSquareError
// (C/mapping/cost_function_square_error.cpp: ComputeSmoothedValue :276-346,
// ComputeMapGradient :172-229) as device functions, shared by k_linsolve.hip,
// k_hc_sq.hip and (through sq_cost_stage.hpp) k_rtcsm.hip.  The library is
// built without relocatable device code, so every translation unit that
// includes this header compiles its own copy; everything here is forced inline.  DESIGN.md §4.5 has the exactness argument.
#pragma once

#include "lgs_internal.hpp"
#include "glibc_math.hpp"

#include <climits>

namespace {

struct LsPlan {
    double min_x, min_y, res;
    int W, H, N;
    int max_iter;
    double conv;
    double step_min, step_max;    // OptimizeStep's beam filter (open interval)
    double cost_min, cost_max;    // CostSquareError's beam filter
    double reg_t, reg_r;
};

// x86-64 cvttsd2si semantics of static_cast<int>(double) (the reference's
// host): out-of-range and NaN give INT_MIN; the GPU conversion would saturate.
__device__ __forceinline__ int host_trunc(double x)
{
    return (x > -2147483649.0 && x < 2147483648.0) ? (int)x : INT_MIN;
}

// bicubic kernel h(t) (:281-295): pow(at, 3.0) is glibc's pow (restated bit-exactly),
// pow(at, 2.0) is at*at after GCC folding
__device__ __forceinline__ double bicubic_h(double t)
{
    const double at = fabs(t);
    if (at <= 1.0) {
        const double at3 = glm::gl_pow3(at);
        const double at2 = at * at;
        return (at3 - 2.0 * at2 + 1.0);
    } else if (at <= 2.0) {
        const double at3 = glm::gl_pow3(at);
        const double at2 = at * at;
        return (-at3 + 5.0 * at2 - 8.0 * at + 4.0);
    }
    return 0.0;
}

// One axis of ComputeSmoothedValue (:276-346) for coordinate v: the four
// sample indices clamp(static_cast<int>(v_i), 0, n-1) of f (:298-310,
// truncation) and the four kernel weights h(v_1..v_4).  The x axis of
// (fx, fy +- d) and the y axis of (fx +- d, fy) are the axes of (fx, fy): the
// reference's "+ 0.0" / "- 0.0" leave every derived quantity unchanged
// (v + 0.0 differs from v only for v = -0.0, which yields the same floor
// differences, indices and weights), so five smoothed values share six axes.
struct Axis {
    int idx[4];
    double w[4];
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (hi < v ? hi : v); }

__device__ __forceinline__ Axis make_axis(double v, int n)
{
    const double fl = floor(v);
    const double v1 = 1.0 + v - fl;
    const double v2 = v - fl;
    const double v3 = fl + 1.0 - v;
    const double v4 = fl + 2.0 - v;
    Axis a;
    a.idx[0] = clampi(host_trunc(v - v1), 0, n - 1);
    a.idx[1] = clampi(host_trunc(v - v2), 0, n - 1);
    a.idx[2] = clampi(host_trunc(v + v3), 0, n - 1);
    a.idx[3] = clampi(host_trunc(v + v4), 0, n - 1);
    a.w[0] = bicubic_h(v1);
    a.w[1] = bicubic_h(v2);
    a.w[2] = bicubic_h(v3);
    a.w[3] = bicubic_h(v4);
    return a;
}

// vecX^T * M * vecY with M(i, j) = f(xs_i, ys_j), evaluated as
// r_j = sum_i vx_i M_ij, then sum_j r_j vy_j (the oracle's order; Eigen's
// own order is not pinned), clamped to [0, 1] (:345)
__device__ __forceinline__ double smoothed(const double* __restrict__ g, int W, const Axis& ax,
                                           const Axis& ay)
{
    double m[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double* row = g + (size_t)ay.idx[j] * W;
#pragma unroll
        for (int i = 0; i < 4; ++i) m[j][i] = gload(row + ax.idx[i]);   // global loads, not flat: the map is device memory
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double acc = ax.w[0] * m[j][0];
#pragma unroll
        for (int i = 1; i < 4; ++i) acc = acc + ax.w[i] * m[j][i];
        s = (j == 0) ? acc * ay.w[0] : s + acc * ay.w[j];
    }
    return s < 0.0 ? 0.0 : (1.0 < s ? 1.0 : s);
}

// Per beam at one sensor pose: residual e = 1 - S(hit point) and the map
// gradient w.r.t. the pose (ComputeMapGradient :172-229: central differences
// of +-0.05 cells, / (0.1 res), dtheta = -r sin gx + r cos gy).
constexpr double kDeltaIdx = 0.1;             // ComputeMapGradient's +- 0.05 cells
constexpr double kHalfDelta = kDeltaIdx / 2.0;

// hit point of a beam in (fractional) cell coordinates
__device__ __forceinline__ void beam_cell(const LsPlan& p, const double pose[3], double r, double a, double& sn,
                                          double& cs, double& fx, double& fy)
{
    glm::gl_sincos(pose[2] + a, &sn, &cs);   // GCC fuses the reference's cos/sin pair into sincos()
    const double hx = pose[0] + r * cs;
    const double hy = pose[1] + r * sn;
    fx = (hx - p.min_x) / p.res;
    fy = (hy - p.min_y) / p.res;
}

// residual and pose gradient from the five smoothed values
__device__ __forceinline__ void beam_finish(const LsPlan& p, double r, double sn, double cs, double s0, double sxp,
                                            double sxm, double syp, double sym, double& e, double gv[3])
{
    const double deltaDist = p.res * kDeltaIdx;
    const double gx = (sxp - sxm) / deltaDist;
    const double gy = (syp - sym) / deltaDist;
    e = 1.0 - s0;
    gv[0] = gx;
    gv[1] = gy;
    gv[2] = -r * sn * gx + r * cs * gy;
}

__device__ __forceinline__ void beam_terms(const LsPlan& p, const double* __restrict__ g,
                                           const double pose[3], double r, double a, double& e,
                                           double gv[3])
{
    double sn, cs, fx, fy;
    beam_cell(p, pose, r, a, sn, cs, fx, fy);
    const double d = kHalfDelta;
    const Axis x0 = make_axis(fx, p.W), xp = make_axis(fx + d, p.W), xm = make_axis(fx - d, p.W);
    const Axis y0 = make_axis(fy, p.H), yp = make_axis(fy + d, p.H), ym = make_axis(fy - d, p.H);
    const double s0 = smoothed(g, p.W, x0, y0);
    const double sxp = smoothed(g, p.W, xp, y0);
    const double sxm = smoothed(g, p.W, xm, y0);
    const double syp = smoothed(g, p.W, x0, yp);
    const double sym = smoothed(g, p.W, x0, ym);
    beam_finish(p, r, sn, cs, s0, sxp, sxm, syp, sym, e, gv);
}

}  // namespace
