// sq_cost_stage.hpp -- CostSquareError's cost and gradient sums at one sensor
// pose as a workgroup-wide device function: the per-beam terms, the term rows
// and the beam-order chains.  Shared by k_hc_sq.hip (k_hc_sq, k_sq_cost_batch)
// and by the correlative pipeline's own cost stage (k_rtcsm.hip k_cost_sq), so
// that every caller compiles the same arithmetic.  As sq_cost_device.hpp:
// no relocatable device code, everything forced inline, one copy per
// translation unit.
#pragma once

#include "sq_cost_device.hpp"

#include <hip/hip_runtime.h>

namespace {

constexpr int kSqThreads = 768;   // 12 waves: with 165 VGPRs a CU holds 3 waves per SIMD, one such workgroup
constexpr int kSqGradRows = 4;               // cost term and the three gradient terms of a beam
constexpr size_t kSqLdsMax = 144 * 1024;     // term rows in LDS up to here, else global rows

// One item of a launch (device memory).
struct SqItem {
    LsPlan p;                   // map geometry; cost_min / cost_max hold the beam filter (:27-30)
    double sx, sy, st;          // sensor pose
    const double* map;
    const double* ranges;
    const double* angles;
    double* rows;               // term rows when they do not fit LDS
    int* trace_move;            // [pass cap] or null
    double* trace_cost;
};

// pow(1.0 - S, 2.0) of beam i at `pose` (:32-55), +0.0 for a filtered beam
__device__ __forceinline__ double sq_term(const SqItem& it, int i, const double pose[3], int* __restrict__ err)
{
    const double r = gload(it.ranges + i);
    if (r >= it.p.cost_max || r <= it.p.cost_min) return 0.0;   // :35-36
    const double a = gload(it.angles + i);
    if (!glm::gl_sincos_ok(pose[2] + a)) *err = 1;
    double sn, cs, fx, fy;
    beam_cell(it.p, pose, r, a, sn, cs, fx, fy);
    const Axis ax = make_axis(fx, it.p.W), ay = make_axis(fy, it.p.H);
    const double e = 1.0 - smoothed(it.map, it.p.W, ax, ay);
    return e * e;   // GCC folds pow(x, 2.0) to the exact product
}

// the cost term and the three terms 2.0 * e * (-g_k) of ComputeGradient (:84-104)
__device__ __forceinline__ void sq_grad_terms(const SqItem& it, int i, const double pose[3], double (&t)[kSqGradRows],
                                              int* __restrict__ err)
{
#pragma unroll
    for (int k = 0; k < kSqGradRows; ++k) t[k] = 0.0;
    const double r = gload(it.ranges + i);
    if (r >= it.p.cost_max || r <= it.p.cost_min) return;
    const double a = gload(it.angles + i);
    if (!glm::gl_sincos_ok(pose[2] + a)) *err = 1;
    double e, gv[3];
    beam_terms(it.p, it.map, pose, r, a, e, gv);
    t[0] = e * e;
    t[1] = 2.0 * e * (-gv[0]);
    t[2] = 2.0 * e * (-gv[1]);
    t[3] = 2.0 * e * (-gv[2]);
}

// c = 0.0; c += term, beams in order (:23, :55; :70-72, :100-104)
__device__ __forceinline__ double sq_chain(const double* __restrict__ row, int N)
{
    double c = 0.0;
    int i = 0;
    for (; i + 8 <= N; i += 8) {
        double t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = row[i + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) c += t[j];
    }
    for (; i < N; ++i) c += row[i];
    return c;
}

// Cost and ComputeGradient's three sums at s_pose[0] into s_cost[0..3]: lanes
// 0..3 of wave 0 add the four rows in beam order.  Every thread of a workgroup
// of kSqThreads calls it; ends with a barrier.
__device__ __forceinline__ void sq_cost_grad(const SqItem& it, double (*s_pose)[3], double* s_cost, double* l_rows,
                                             bool in_lds, int* __restrict__ err)
{
    const int N = it.p.N;
    double* __restrict__ g_rows = it.rows;
    const double pose[3] = { s_pose[0][0], s_pose[0][1], s_pose[0][2] };
    for (int i = threadIdx.x; i < N; i += kSqThreads) {
        double t[kSqGradRows];
        sq_grad_terms(it, i, pose, t, err);
#pragma unroll
        for (int k = 0; k < kSqGradRows; ++k) {
            if (in_lds)
                l_rows[(size_t)k * N + i] = t[k];
            else
                g_rows[(size_t)k * N + i] = t[k];
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < kSqGradRows) {
        const size_t o = (size_t)threadIdx.x * N;
        s_cost[threadIdx.x] = in_lds ? sq_chain(l_rows + o, N) : sq_chain(g_rows + o, N);
    }
    __syncthreads();
}

// ------------------------------------------------------------------ host
// dynamic LDS beyond the 64 KiB default has to be announced; launches report
// what this leaves unsaid
template <class K>
void sq_allow_lds(K kernel, size_t bytes)
{
    if (bytes > 64 * 1024) {
        (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        (void)hipGetLastError();
    }
}

// ComputeCovariance (:112-135): g g^T, + 0.01 on the diagonal
inline void sq_covariance(const double g[3], double* cov)
{
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) cov[3 * a + b] = g[a] * g[b];
    cov[0] += 0.01;
    cov[4] += 0.01;
    cov[8] += 0.01;
}

}  // namespace
