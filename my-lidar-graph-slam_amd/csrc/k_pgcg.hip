// k_pgcg.hip -- the linear solve of a pose-graph Levenberg-Marquardt step,
// H delta = -b, by Jacobi-preconditioned conjugate gradients on MI355X.
//
// Restates Eigen's ConjugateGradient recurrence
// (Eigen/src/IterativeLinearSolvers/ConjugateGradient.h) as the host solver
// of my-lidar-graph-slam_amd/host/lgs_posegraph.cpp (solve_cg) does: the
// preconditioner 1 / d (1 where d == 0), a zero initial guess, the threshold
// max(tol^2 |rhs|^2, DBL_MIN), the early returns on a zero right-hand side and
// on a residual that is already small, the same order of updates and the test
// right after the update of r.  DESIGN.md §4.7b.
//
//   k_pgcg   one persistent workgroup runs the whole solve with workgroup
//            barriers only.  H is a row-compressed matrix of 3x3 blocks
//            (pgcg_pattern.hpp); thread t owns the scalar rows t, t + 1024, ...
//            of every vector.  A row's product adds its blocks in storage
//            order (the diagonal, then the neighbours by ascending node), each
//            block as a k = 0..2 sequential sum: no atomics.  A dot product
//            adds a thread's rows in ascending order, then the 64 lanes of a
//            wave by a shuffle tree, then the 16 wave sums in wave order: the
//            same tree in every run, so x, the pass count and the residual
//            repeat byte for byte.  r.r and r.z share one pass: two reductions
//            and three barriers per CG pass.  While the five vectors fit
//            LDS (5 x 3n doubles, n <= 1297) they all live there and a pass
//            reads only H from global memory; up to n = 6485 the search
//            direction p, which every row gathers from, still does; beyond
//            that every vector sits in global memory.
//   k_pgcg_grid_*  the same recurrence over many workgroups, two launches
//            per pass (below): what graphs of LGS_OPT_PGCG_GRID_NODES nodes
//            and more run, where one compute unit's path to L2 is the limit
//
// Every loop is bounded by max_iterations (a NaN never satisfies the residual
// test and runs to the cap).
#include "lgs_internal.hpp"
#include "pgcg_pattern.hpp"

#include <cfloat>
#include <cstring>

using namespace lgs;

namespace {

constexpr int kPgThreads = 1024;
constexpr int kPgWaves = kPgThreads / 64;
constexpr size_t kPgLdsMax = 152 * 1024;   // dynamic LDS of k_pgcg: all five vectors, or p alone, while they fit

struct PgArgs {
    const int* rowptr;     // [n + 1]
    const int* col;        // [blocks]
    const double* val;     // [blocks][9]
    const double* rhs;     // [3n]
    double *x, *r, *t, *inv, *p;   // [3n] each, global memory: x always (the result), the others when they do not fit LDS
    PgResult* res;
    double tol2;           // tolerance^2
    int n, max_iterations;
};

// lane 0 of the wave: v of lanes 0..63 by a fixed tree
__device__ __forceinline__ double pg_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// the wave sums of one reduction, in wave order (every thread, after the barrier behind the writes)
__device__ __forceinline__ double pg_total(const double* part)
{
    double s = part[0];
#pragma unroll
    for (int w = 1; w < kPgWaves; ++w) s += part[w];
    return s;
}

// the search direction: LDS, or global memory the workgroup's own threads wrote before a barrier
template <bool LDS>
__device__ __forceinline__ double pg_ld(const double* p, int i)
{
    if constexpr (LDS)
        return p[i];
    else
        return gload(p + i);
}
template <bool LDS>
__device__ __forceinline__ void pg_st(double* p, int i, double v)
{
    if constexpr (LDS)
        p[i] = v;
    else
        gstore(p + i, v);
}

// MODE 2: p, r, t, the preconditioner and x in LDS (5 x 3n doubles fit), 1: p in LDS, 0: every vector in global memory
template <int MODE>
__global__ __launch_bounds__(kPgThreads) void k_pgcg(PgArgs a)
{
    constexpr bool PL = MODE >= 1, VL = MODE == 2;
    extern __shared__ double l_vec[];           // [3n] (MODE 1) or [5][3n] (MODE 2)
    // one slot per reduction site: a slot is rewritten only after a barrier
    // that every reader of its previous values has passed
    __shared__ double s_pt[kPgWaves], s_rr[kPgWaves], s_rz[kPgWaves], s_rp[kPgWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = 3 * a.n;
    const int* __restrict__ rowptr = a.rowptr;
    const int* __restrict__ col = a.col;
    const double* __restrict__ val = a.val;
    double* p = PL ? l_vec : a.p;
    double* r = VL ? l_vec + m : a.r;
    double* t = VL ? l_vec + 2 * (size_t)m : a.t;
    double* inv = VL ? l_vec + 3 * (size_t)m : a.inv;
    double* x = VL ? l_vec + 4 * (size_t)m : a.x;

    // x = 0, r = rhs - H 0, the preconditioner, |rhs|^2
    double acc = 0.0;
    for (int row = tid; row < m; row += kPgThreads) {
        const int v = row / 3, c = row - 3 * v;
        const double b = gload(a.rhs + row);
        const double d = gload(val + 9 * (size_t)gload(rowptr + v) + 4 * c);   // the diagonal block comes first
        pg_st<VL>(x, row, 0.0);
        pg_st<VL>(r, row, b);
        pg_st<VL>(inv, row, (d != 0.0) ? 1.0 / d : 1.0);
        acc += b * b;
    }
    acc = pg_wave_sum(acc);
    if (lane == 0) s_rr[wave] = acc;
    __syncthreads();
    const double rhs_norm2 = pg_total(s_rr);
    double r_norm2 = rhs_norm2;
    int passes = 0;
    const double threshold = fmax(a.tol2 * rhs_norm2, DBL_MIN);
    // (a NaN norm takes neither return and runs to the cap)
    if (!(rhs_norm2 == 0.0) && !(r_norm2 < threshold)) {
        // p = M^-1 r, absNew = r . p
        acc = 0.0;
        for (int row = tid; row < m; row += kPgThreads) {
            const double rv = pg_ld<VL>(r, row);
            const double pv = pg_ld<VL>(inv, row) * rv;
            pg_st<PL>(p, row, pv);
            acc += rv * pv;
        }
        acc = pg_wave_sum(acc);
        if (lane == 0) s_rp[wave] = acc;
        __syncthreads();
        double abs_new = pg_total(s_rp);

        for (int it = 0; it < a.max_iterations; ++it) {
            // t = H p, p . t
            acc = 0.0;
            for (int row = tid; row < m; row += kPgThreads) {
                const int v = row / 3, c = row - 3 * v;
                const int e0 = gload(rowptr + v), e1 = gload(rowptr + v + 1);
                double y = 0.0;
                for (int e = e0; e < e1; ++e) {
                    const double* __restrict__ h = val + 9 * (size_t)e + 3 * c;
                    const int cb = 3 * gload(col + e);
                    const double h0 = gload(h), h1 = gload(h + 1), h2 = gload(h + 2);
                    y += h0 * pg_ld<PL>(p, cb) + h1 * pg_ld<PL>(p, cb + 1) + h2 * pg_ld<PL>(p, cb + 2);
                }
                pg_st<VL>(t, row, y);
                acc += pg_ld<PL>(p, row) * y;
            }
            acc = pg_wave_sum(acc);
            if (lane == 0) s_pt[wave] = acc;
            __syncthreads();
            const double alpha = abs_new / pg_total(s_pt);
            // x += alpha p, r -= alpha t, then r . r and r . z with z = M^-1 r (kept in t)
            acc = 0.0;
            double acz = 0.0;
            for (int row = tid; row < m; row += kPgThreads) {
                pg_st<VL>(x, row, pg_ld<VL>(x, row) + alpha * pg_ld<PL>(p, row));
                const double rv = pg_ld<VL>(r, row) - alpha * pg_ld<VL>(t, row);
                pg_st<VL>(r, row, rv);
                const double zv = pg_ld<VL>(inv, row) * rv;
                pg_st<VL>(t, row, zv);
                acc += rv * rv;
                acz += rv * zv;
            }
            acc = pg_wave_sum(acc);
            acz = pg_wave_sum(acz);
            if (lane == 0) {
                s_rr[wave] = acc;
                s_rz[wave] = acz;
            }
            __syncthreads();
            r_norm2 = pg_total(s_rr);
            ++passes;
            if (r_norm2 < threshold) break;   // the same value in every thread
            const double abs_old = abs_new;
            abs_new = pg_total(s_rz);
            const double beta = abs_new / abs_old;
            for (int row = tid; row < m; row += kPgThreads)
                pg_st<PL>(p, row, pg_ld<VL>(t, row) + beta * pg_ld<PL>(p, row));
            __syncthreads();
        }
    }
    if constexpr (VL)   // a thread's own rows
        for (int row = tid; row < m; row += kPgThreads) gstore(a.x + row, x[row]);
    if (tid == 0) {
        a.res->residual_norm2 = (rhs_norm2 == 0.0) ? 0.0 : r_norm2;
        a.res->threshold = threshold;
        a.res->iterations = passes;
        a.res->done = 1;
    }
}

// ---------------------------------------------------------------------------
// The same recurrence over many workgroups, for graphs too large for one
// compute unit to be quick (a pass of k_pgcg reads H and the vectors through
// one unit's path to L2).  Workgroups meet at kernel boundaries only: a pass
// is two launches,
//   k_pgcg_grid_spmv    concludes the pass before (|r|^2 against the
//                       threshold, beta), then p = z + beta p and t = H p.
//                       The rows of p that a product gathers are formed on
//                       the fly from z and the previous p (kept in a second
//                       buffer) by the expression that stores p, so no launch
//                       separates the update of p from the product
//   k_pgcg_grid_update  alpha, x += alpha p, r -= alpha t, z = M^-1 r
// and a dot product is one partial per workgroup (rows in ascending order per
// thread, the wave tree, the wave sums in order) that every workgroup of the
// next launch adds up in the same fixed order: the same bits in every
// workgroup and in every run, no atomics.  The grid is a function of the node
// count alone.  Every workgroup takes the decisions from those sums itself;
// one of them records the end of the solve in PgResult::done, which launches
// already enqueued read first and return on.  The host enqueues chunks of
// passes up to max_iterations and looks at `done` once per chunk.
// ---------------------------------------------------------------------------
constexpr int kPgGridThreads = 256;
constexpr int kPgGridWaves = kPgGridThreads / 64;
constexpr int kPgGridMaxWgs = 1024;
constexpr int kPgGridChunk = 32;         // passes enqueued between two looks at `done`

struct PgGridArgs {
    const int* rowptr;
    const int* col;
    const double* val;
    const double* rhs;
    double *x, *r, *z, *inv, *t;
    double* p[2];            // the direction of even / odd passes
    double* part_pt;         // [G] p . t
    double* part_rr[2];      // [G] r . r as pass parity 0 / 1 reads it
    double* part_rz[2];      // [G] r . z
    PgResult* res;
    double tol2;
    int n, G;
};

// the sum of K values per thread over the workgroup, in every thread
template <int K>
__device__ __forceinline__ void pg_grid_block_sum(double (&v)[K], double (*s_w)[kPgGridWaves])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = pg_wave_sum(v[k]);
        if (lane == 0) s_w[k][wave] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = s_w[k][0];
#pragma unroll
        for (int w = 1; w < kPgGridWaves; ++w) s += s_w[k][w];
        v[k] = s;
    }
    __syncthreads();   // s_w may be written again
}

// the totals of K partial arrays of G entries (null: 0), in every thread of every workgroup
template <int K>
__device__ __forceinline__ void pg_grid_totals(const double* const (&part)[K], int G, double (&out)[K],
                                               double (*s_w)[kPgGridWaves])
{
#pragma unroll
    for (int k = 0; k < K; ++k) {
        out[k] = 0.0;
        if (part[k])
            for (int g = threadIdx.x; g < G; g += kPgGridThreads) out[k] += gload(part[k] + g);
    }
    pg_grid_block_sum<K>(out, s_w);
}

__global__ __launch_bounds__(kPgGridThreads) void k_pgcg_grid_init(PgGridArgs a)
{
    __shared__ double s_w[2][kPgGridWaves];
    const int m = 3 * a.n;
    double acc[2] = { 0.0, 0.0 };
    for (int row = blockIdx.x * kPgGridThreads + threadIdx.x; row < m; row += a.G * kPgGridThreads) {
        const int v = row / 3, c = row - 3 * v;
        const double b = gload(a.rhs + row);
        const double d = gload(a.val + 9 * (size_t)gload(a.rowptr + v) + 4 * c);
        const double iv = (d != 0.0) ? 1.0 / d : 1.0;
        const double zv = iv * b;
        gstore(a.x + row, 0.0);
        gstore(a.r + row, b);
        gstore(a.inv + row, iv);
        gstore(a.z + row, zv);
        acc[0] += b * b;
        acc[1] += b * zv;
    }
    pg_grid_block_sum<2>(acc, s_w);
    if (threadIdx.x == 0) {
        gstore(a.part_rr[0] + blockIdx.x, acc[0]);
        gstore(a.part_rz[0] + blockIdx.x, acc[1]);
    }
}

// pass `it` of at most `cap`; it == cap only concludes the last pass
__global__ __launch_bounds__(kPgGridThreads) void k_pgcg_grid_spmv(PgGridArgs a, int it, int cap)
{
    __shared__ double s_w[3][kPgGridWaves];
    if (gload(&a.res->done)) return;
    const int par = it & 1;
    const bool first = it == 0, lead = blockIdx.x == 0 && threadIdx.x == 0;
    const double* const parts[3] = { a.part_rr[par], a.part_rz[par], first ? nullptr : a.part_rz[par ^ 1] };
    double tot[3];
    pg_grid_totals<3>(parts, a.G, tot, s_w);
    const double r_norm2 = tot[0], abs_new = tot[1], abs_old = tot[2];
    if (first) {
        // |rhs|^2: a zero right-hand side and a residual that is already small end the solve
        const double threshold = fmax(a.tol2 * r_norm2, DBL_MIN);
        if (lead) a.res->threshold = threshold;
        if (r_norm2 == 0.0 || r_norm2 < threshold) {
            if (lead) {
                a.res->residual_norm2 = (r_norm2 == 0.0) ? 0.0 : r_norm2;
                a.res->iterations = 0;
                a.res->done = 1;
            }
            return;
        }
    } else if (r_norm2 < gload(&a.res->threshold) || it == cap) {
        if (lead) {
            a.res->residual_norm2 = r_norm2;
            a.res->iterations = it;
            a.res->done = 1;
        }
        return;
    }
    const double beta = first ? 0.0 : abs_new / abs_old;
    const double* __restrict__ z = a.z;
    const double* __restrict__ po = a.p[par ^ 1];
    double* __restrict__ pn = a.p[par];
    const int m = 3 * a.n;
    double acc[1] = { 0.0 };
    for (int row = blockIdx.x * kPgGridThreads + threadIdx.x; row < m; row += a.G * kPgGridThreads) {
        const int v = row / 3, c = row - 3 * v;
        const int e0 = gload(a.rowptr + v), e1 = gload(a.rowptr + v + 1);
        double y = 0.0;
        for (int e = e0; e < e1; ++e) {
            const double* __restrict__ h = a.val + 9 * (size_t)e + 3 * c;
            const int cb = 3 * gload(a.col + e);
            const double h0 = gload(h), h1 = gload(h + 1), h2 = gload(h + 2);
            double p0 = gload(z + cb), p1 = gload(z + cb + 1), p2 = gload(z + cb + 2);
            if (!first) {   // the expression that stores p below
                p0 = p0 + beta * gload(po + cb);
                p1 = p1 + beta * gload(po + cb + 1);
                p2 = p2 + beta * gload(po + cb + 2);
            }
            y += h0 * p0 + h1 * p1 + h2 * p2;
        }
        double pr = gload(z + row);
        if (!first) pr = pr + beta * gload(po + row);
        gstore(pn + row, pr);
        gstore(a.t + row, y);
        acc[0] += pr * y;
    }
    pg_grid_block_sum<1>(acc, s_w);
    if (threadIdx.x == 0) gstore(a.part_pt + blockIdx.x, acc[0]);
}

__global__ __launch_bounds__(kPgGridThreads) void k_pgcg_grid_update(PgGridArgs a, int it)
{
    __shared__ double s_w[2][kPgGridWaves];
    if (gload(&a.res->done)) return;
    const int par = it & 1;
    const double* const parts[2] = { a.part_rz[par], a.part_pt };
    double tot[2];
    pg_grid_totals<2>(parts, a.G, tot, s_w);
    const double alpha = tot[0] / tot[1];
    const double* __restrict__ pn = a.p[par];
    const int m = 3 * a.n;
    double acc[2] = { 0.0, 0.0 };
    for (int row = blockIdx.x * kPgGridThreads + threadIdx.x; row < m; row += a.G * kPgGridThreads) {
        gstore(a.x + row, gload(a.x + row) + alpha * gload(pn + row));
        const double rv = gload(a.r + row) - alpha * gload(a.t + row);
        gstore(a.r + row, rv);
        const double zv = gload(a.inv + row) * rv;
        gstore(a.z + row, zv);
        acc[0] += rv * rv;
        acc[1] += rv * zv;
    }
    pg_grid_block_sum<2>(acc, s_w);
    if (threadIdx.x == 0) {
        gstore(a.part_rr[par ^ 1] + blockIdx.x, acc[0]);
        gstore(a.part_rz[par ^ 1] + blockIdx.x, acc[1]);
    }
}

// the pattern of the pair list a context solved last
struct PgCache {
    std::vector<int> pairs;
    PgPattern pat;
};

}  // namespace

bool lgs::pg_runs_grid(const lgs_ctx* ctx, int num_nodes) { return num_nodes >= ctx->pg_grid_nodes; }

namespace {
int pg_grid_wgs(size_t m) { return (int)std::min<size_t>((m + kPgGridThreads - 1) / kPgGridThreads, (size_t)kPgGridMaxWgs); }
}  // namespace

size_t lgs::pg_work_bytes(const lgs_ctx* ctx, int num_nodes)
{
    const size_t m = 3 * (size_t)num_nodes, mb = pg_align256(sizeof(double) * m);
    const bool in_lds = sizeof(double) * m <= kPgLdsMax;
    const size_t gb = pg_align256(sizeof(double) * (size_t)pg_grid_wgs(m));
    return pg_runs_grid(ctx, num_nodes) ? 6 * mb + 5 * gb : 3 * mb + (in_lds ? 0 : mb);
}

bool lgs::pg_solve_enqueue(lgs_ctx* ctx, const PgDeviceSystem& s, double tolerance, int max_iterations)
{
    const int num_nodes = s.n;
    const size_t m = 3 * (size_t)num_nodes, mb = pg_align256(sizeof(double) * m);
    const bool grid = pg_runs_grid(ctx, num_nodes);
    const bool in_lds = sizeof(double) * m <= kPgLdsMax;
    const int G = pg_grid_wgs(m);
    const size_t gb = pg_align256(sizeof(double) * (size_t)G);
    double* const d_work = s.work;
    const size_t mw = mb / sizeof(double), gw = gb / sizeof(double);
    const double tol2 = (tolerance == 0.0) ? DBL_EPSILON * DBL_EPSILON : tolerance * tolerance;
    const int cap = max_iterations == 0 ? (int)(2 * m) : max_iterations;
    if (!grid) {
        PgArgs a;
        a.rowptr = s.rowptr;
        a.col = s.col;
        a.val = s.val;
        a.rhs = s.rhs;
        a.x = s.x;
        a.res = s.res;
        a.r = d_work;
        a.t = d_work + mw;
        a.inv = d_work + 2 * mw;
        a.p = in_lds ? nullptr : d_work + 3 * mw;
        a.tol2 = tol2;
        a.n = num_nodes;
        a.max_iterations = cap;
        const int mode = 5 * sizeof(double) * m <= kPgLdsMax ? 2 : in_lds ? 1 : 0;
        const size_t lds = mode == 2 ? 5 * sizeof(double) * m : mode == 1 ? sizeof(double) * m : 0;
        auto launch = [&](auto kernel) {
            if (lds > 64 * 1024) {   // dynamic LDS beyond the 64 KiB default has to be announced
                (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                (void)hipGetLastError();
            }
            hipLaunchKernelGGL(kernel, dim3(1), dim3(kPgThreads), lds, ctx->stream, a);
        };
        if (mode == 2)
            launch(k_pgcg<2>);
        else if (mode == 1)
            launch(k_pgcg<1>);
        else
            launch(k_pgcg<0>);
        LGS_HIP_CHECK(hipGetLastError());
    } else {
        PgGridArgs a;
        a.rowptr = s.rowptr;
        a.col = s.col;
        a.val = s.val;
        a.rhs = s.rhs;
        a.x = s.x;
        a.res = s.res;
        a.r = d_work;
        a.z = d_work + mw;
        a.inv = d_work + 2 * mw;
        a.t = d_work + 3 * mw;
        a.p[0] = d_work + 4 * mw;
        a.p[1] = d_work + 5 * mw;
        double* const parts = d_work + 6 * mw;
        a.part_pt = parts;
        a.part_rr[0] = parts + gw;
        a.part_rr[1] = parts + 2 * gw;
        a.part_rz[0] = parts + 3 * gw;
        a.part_rz[1] = parts + 4 * gw;
        a.tol2 = tol2;
        a.n = num_nodes;
        a.G = G;
        for (hipEvent_t& e : ctx->pg_ev)
            if (!e) LGS_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        LGS_HIP_CHECK(hipMemsetAsync(s.res, 0, sizeof(PgResult), ctx->stream));
        hipLaunchKernelGGL(k_pgcg_grid_init, dim3(G), dim3(kPgGridThreads), 0, ctx->stream, a);
        LGS_HIP_CHECK(hipGetLastError());
        // chunks of passes; the record of chunk k is looked at once chunk k + 1 is enqueued
        PgResult* const seen = s.seen;
        int it = 0;
        for (int chunk = 0;; ++chunk) {
            const int end = (int)std::min<long long>((long long)it + kPgGridChunk, cap);
            for (; it < end; ++it) {
                hipLaunchKernelGGL(k_pgcg_grid_spmv, dim3(G), dim3(kPgGridThreads), 0, ctx->stream, a, it, cap);
                hipLaunchKernelGGL(k_pgcg_grid_update, dim3(G), dim3(kPgGridThreads), 0, ctx->stream, a, it);
            }
            if (it == cap)   // concludes the last pass
                hipLaunchKernelGGL(k_pgcg_grid_spmv, dim3(G), dim3(kPgGridThreads), 0, ctx->stream, a, cap, cap);
            LGS_HIP_CHECK(hipGetLastError());
            if (it == cap) break;
            LGS_HIP_CHECK(hipMemcpyAsync(seen + (chunk & 1), s.res, sizeof(PgResult), hipMemcpyDeviceToHost,
                                         ctx->stream));
            LGS_HIP_CHECK(hipEventRecord(ctx->pg_ev[chunk & 1], ctx->stream));
            if (chunk > 0) {
                ctx->wait_event(ctx->pg_ev[(chunk - 1) & 1]);
                if (seen[(chunk - 1) & 1].done) break;
            }
        }
    }
    return grid;
}

extern "C" int lgs_pg_cg_solve(lgs_ctx* ctx, int num_nodes, const double* diag, int num_pairs, const int* pairs,
                               const double* off, const double* rhs, double tolerance, int max_iterations, double* x,
                               int* iterations, double* residual_norm2)
{
    if (!ctx || !diag || !rhs || !x || !iterations || !residual_norm2 || (num_pairs > 0 && (!pairs || !off)))
        return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        LGS_REQUIRE(pg_args_ok(num_nodes, num_pairs, pairs, tolerance, max_iterations),
                    "pose-graph CG: 1 <= nodes <= 2^27, pairs (a, b) with 0 <= a < b < nodes, tolerance finite and >= 0, "
                    "cap >= 0");
        const size_t m = 3 * (size_t)num_nodes;
        auto cache = std::static_pointer_cast<PgCache>(ctx->pg_cache);
        const bool known = cache && cache->pat.n == num_nodes && cache->pairs.size() == 2 * (size_t)num_pairs &&
                           (num_pairs == 0 ||
                            std::memcmp(cache->pairs.data(), pairs, sizeof(int) * 2 * (size_t)num_pairs) == 0);
        if (!known) {
            ctx->pg_cache.reset();   // the device copy is about to be overwritten
            cache = std::make_shared<PgCache>();
            LGS_REQUIRE(pg_build_pattern(num_nodes, num_pairs, pairs, cache->pat), "pose-graph CG: a pair is listed twice");
            cache->pairs.assign(pairs, pairs + 2 * (size_t)num_pairs);
        }
        const PgPattern& pat = cache->pat;
        const size_t blocks = pat.blocks();
        LGS_HIP_CHECK(hipSetDevice(ctx->device));

        // device layout: S_PG0 = rowptr | col, S_PG1 = val | rhs | x | result | work vectors (| partial sums)
        const size_t rpb = pg_align256(sizeof(int) * ((size_t)num_nodes + 1)), clb = pg_align256(sizeof(int) * blocks);
        const size_t vb = pg_align256(sizeof(double) * 9 * blocks), mb = pg_align256(sizeof(double) * m);
        char* d_pat = (char*)ctx->ensure(S_PG0, rpb + clb);
        char* d_sys = (char*)ctx->ensure(S_PG1, vb + mb + mb + 256 + pg_work_bytes(ctx, num_nodes));
        char* pin = (char*)ctx->ensure_pinned_pg(vb + mb + (known ? 0 : rpb + clb));
        if (!known) {
            std::memcpy(pin + vb + mb, pat.rowptr.data(), sizeof(int) * pat.rowptr.size());
            std::memcpy(pin + vb + mb + rpb, pat.col.data(), sizeof(int) * blocks);
            LGS_HIP_CHECK(hipMemcpyAsync(d_pat, pin + vb + mb, rpb + clb, hipMemcpyHostToDevice, ctx->stream));
            ++ctx->pg_patterns;
        }
        pg_fill_values(pat, diag, off, (double*)pin);
        std::memcpy(pin + vb, rhs, sizeof(double) * m);
        LGS_HIP_CHECK(hipMemcpyAsync(d_sys, pin, vb + mb, hipMemcpyHostToDevice, ctx->stream));

        char* back = (char*)ctx->ensure_pinned(mb + 256 + 2 * sizeof(PgResult));
        PgDeviceSystem sys;
        sys.rowptr = (const int*)d_pat;
        sys.col = (const int*)(d_pat + rpb);
        sys.val = (const double*)d_sys;
        sys.rhs = (const double*)(d_sys + vb);
        sys.x = (double*)(d_sys + vb + mb);
        sys.res = (PgResult*)(d_sys + vb + 2 * mb);
        sys.work = (double*)(d_sys + vb + 2 * mb + 256);
        sys.seen = (PgResult*)(back + mb + 256);
        sys.n = num_nodes;
        const bool grid = pg_solve_enqueue(ctx, sys, tolerance, max_iterations);
        LGS_HIP_CHECK(hipMemcpyAsync(back, sys.x, mb + 256, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        ctx->pg_cache = cache;   // the device holds this pattern now
        PgResult res;
        std::memcpy(&res, back + mb, sizeof(res));
        std::memcpy(x, back, sizeof(double) * m);
        *iterations = res.iterations;
        *residual_norm2 = res.residual_norm2;
        ++ctx->pg_solves;
        if (grid) ++ctx->pg_grid_solves;
        ctx->pg_iterations += res.iterations;
    });
}

extern "C" int lgs_pg_cg_stats(const lgs_ctx* ctx, long long* solves, long long* iterations, long long* patterns,
                               long long* grid_solves)
{
    if (!ctx) return LGS_ERR_INVALID_ARG;
    if (grid_solves) *grid_solves = ctx->pg_grid_solves;
    if (solves) *solves = ctx->pg_solves;
    if (iterations) *iterations = ctx->pg_iterations;
    if (patterns) *patterns = ctx->pg_patterns;
    return LGS_OK;
}
