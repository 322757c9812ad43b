// k_pglm.hip -- PoseGraphOptimizerLM::Optimize resident on MI355X: poses and
// edges go up once, every Levenberg-Marquardt step runs on the device, the
// poses come down once.  DESIGN.md §4.7c.
//
//   k_pg_linearise  H and rhs = -b of one step (C/mapping/
//            pose_graph_optimizer_lm.cpp:84-172, :224-299), written straight
//            into the row-compressed 3x3-block layout k_pgcg walks.  One thread
//            per block entry; it walks the entry's incidence list
//            (pglm_pattern.hpp) and adds the edges' terms by ascending edge
//            index from +0.0 -- the order in which the host's OptimizeStep
//            accumulates that entry -- recomputing each edge it meets.  The
//            diagonal entry's thread also forms its node's rhs, adds the 1e9
//            anchor (node 0) and then the damping factor.  No atomics, no
//            intermediate per-edge buffer.  The arithmetic is the host's,
//            statement for statement: glm::gl_sincos for glibc's sincos, fmod,
//            IEEE division and square root, every 3-term sum in k = 0..2
//            order, no contraction; only Welsch's exp is the device's own.
//   (the solve)     lgs::pg_solve_enqueue, the device side of lgs_pg_cg_solve
//   k_pg_update     poses += delta into the other pose buffer, and per edge
//            Loss(e^T Lambda e) at the new poses (ComputeTotalError, :302-338):
//            an edge's thread forms its two nodes' new poses from the old
//            poses and delta by the expression that stores them, so no launch
//            separates the update from the loss (the device of
//            k_pgcg_grid_spmv).  Thread 0 copies the solve's record behind the
//            loss terms: one device-to-host copy per step.
//
// Per step the host reads the m loss terms and that record, adds the terms in
// edge order (the reference's order) and applies Optimize's rule for the
// damping factor and for stopping (:13-65).
#include "lgs_internal.hpp"
#include "glibc_math.hpp"
#include "pglm_pattern.hpp"

#include <cfloat>
#include <cstring>

using namespace lgs;

namespace {

constexpr int kLmThreads = 256;

// what a step leaves behind the loss terms
struct LmTail {
    PgResult res;
    int err;    // a finite angle outside gl_sincos's domain
    int pad;
};

struct LmArgs {
    const int *rowptr, *col, *src;   // the block pattern and, per entry, -1 (diagonal) / p / -2 - p (PgPattern::src)
    const int *nptr, *ninc;          // per node: edge << 2 | role
    const int *pptr, *pinc;          // per pair: edge << 1 | swapped
    const lgs_pg_edge* edges;        // [m]
    double* val;                     // [blocks][9]
    double* rhs;                     // [3n]
    double* loss;                    // [m]
    LmTail* tail;
    const PgResult* res;             // the solve's record
    double scale;
    int kind, n, m, blocks;
};

struct Edge {
    int s, e;
    double z[3], L[9];
};

__device__ __forceinline__ Edge load_edge(const lgs_pg_edge* edges, int i)
{
    const lgs_pg_edge* g = edges + i;
    Edge d;
    d.s = gload(&g->start_node_index);
    d.e = gload(&g->end_node_index);
    d.z[0] = gload(&g->relative_pose.x);
    d.z[1] = gload(&g->relative_pose.y);
    d.z[2] = gload(&g->relative_pose.theta);
#pragma unroll
    for (int k = 0; k < 9; ++k) d.L[k] = gload(&g->information[k]);
    return d;
}

// H/util.hpp:125-135
__device__ __forceinline__ double normalize_angle(double theta)
{
    double t = fmod(theta, 2.0 * M_PI);
    if (t > M_PI)
        t -= 2.0 * M_PI;
    else if (t < -M_PI)
        t += 2.0 * M_PI;
    return t;
}

// glibc's sincos of a start node's angle; a finite angle outside the restated
// range is reported (NaN and infinity give NaN, as glibc's does)
__device__ __forceinline__ void lm_sincos(double th, double* sn, double* cs, int* err)
{
    if (!glm::gl_sincos_ok(th) && th - th == 0.0) *err = 1;
    glm::gl_sincos(th, sn, cs);
}

// ComputeErrorFunction (:283-299): InverseCompound(start, end) - z, angle normalised
__device__ __forceinline__ void lm_error(const double (&sp)[3], const double (&ep)[3], const double (&z)[3], double sinT,
                                         double cosT, double (&ev)[3])
{
    const double dx = ep[0] - sp[0], dy = ep[1] - sp[1], dt = ep[2] - sp[2];
    const double rx = cosT * dx + sinT * dy, ry = -sinT * dx + cosT * dy;
    ev[0] = rx - z[0];
    ev[1] = ry - z[1];
    ev[2] = normalize_angle(dt - z[2]);
}

// e^T Lambda e as the host's quad(): t = Lambda^T e, then t . e
__device__ __forceinline__ double lm_quad(const double (&e)[3], const double (&L)[9])
{
    const double t0 = L[0] * e[0] + L[3] * e[1] + L[6] * e[2];
    const double t1 = L[1] * e[0] + L[4] * e[1] + L[7] * e[2];
    const double t2 = L[2] * e[0] + L[5] * e[1] + L[8] * e[2];
    return t0 * e[0] + t1 * e[1] + t2 * e[2];
}

// C/mapping/robust_loss_function.cpp, the expressions of host/lgs_posegraph.cpp
__device__ __forceinline__ double lm_weight(int kind, double s, double t)
{
    switch (kind) {
    case 0: return (t <= s) ? 1.0 : sqrt(s / t);
    case 1: return s / (s + t);
    case 2: {
        const double e = sqrt(t / s);
        return 1.0 / (1.0 + e);
    }
    case 3: {
        const double s2 = s * s, st = s + t;
        return s2 / (st * st);
    }
    case 4: return exp(-t / s);
    case 5: {
        const double x = 2.0 * s / (t + s);   // pow(x, 2.0), which GCC folds to x * x
        return (t <= s) ? 1.0 : x * x;
    }
    default: return 1.0;
    }
}

__device__ __forceinline__ double lm_loss(int kind, double s, double t)
{
    switch (kind) {
    case 0: return (t <= s) ? t : (2.0 * sqrt(s * t) - s);
    case 1: return s * log1p(t / s);
    case 2: {
        const double e = sqrt(t / s);
        return 2.0 * s * (e - log1p(e));
    }
    case 3: return s * t / (s + t);
    case 4: return s * (-expm1(-t / s));
    case 5: return s * t / (s + t);
    default: return t;
    }
}

__device__ __forceinline__ void mat_mul(const double (&a)[9], const double (&b)[9], double (&c)[9])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

__device__ __forceinline__ void mat_mul_tn(const double (&a)[9], const double (&b)[9], double (&c)[9])   // a^T b
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[i] * b[j] + a[3 + i] * b[3 + j] + a[6 + i] * b[6 + j];
}

__device__ __forceinline__ void mat_mulv(const double (&a)[9], const double (&x)[3], double (&y)[3])
{
    y[0] = a[0] * x[0] + a[1] * x[1] + a[2] * x[2];
    y[1] = a[3] * x[0] + a[4] * x[1] + a[5] * x[2];
    y[2] = a[6] * x[0] + a[7] * x[1] + a[8] * x[2];
}

// one edge of OptimizeStep up to the products its blocks are made of
struct EdgeLin {
    double Js[9], Je[9], JsW[9], JeW[9], ev[3];
};

__device__ __forceinline__ void linearise_edge(const LmArgs& a, const double* __restrict__ poses, int i, EdgeLin& o)
{
    const Edge d = load_edge(a.edges, i);
    double sp[3], ep[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        sp[k] = gload(poses + 3 * (size_t)d.s + k);
        ep[k] = gload(poses + 3 * (size_t)d.e + k);
    }
    // ComputeErrorJacobians (:224-280)
    const double dx = ep[0] - sp[0], dy = ep[1] - sp[1];
    double sinT, cosT;
    lm_sincos(sp[2], &sinT, &cosT, &a.tail->err);
    const double ex = -sinT * dx + cosT * dy, ey = -cosT * dx - sinT * dy;
    o.Js[0] = -cosT, o.Js[1] = -sinT, o.Js[2] = ex;
    o.Js[3] = sinT, o.Js[4] = -cosT, o.Js[5] = ey;
    o.Js[6] = 0.0, o.Js[7] = 0.0, o.Js[8] = -1.0;
    o.Je[0] = cosT, o.Je[1] = sinT, o.Je[2] = 0.0;
    o.Je[3] = -sinT, o.Je[4] = cosT, o.Je[5] = 0.0;
    o.Je[6] = 0.0, o.Je[7] = 0.0, o.Je[8] = 1.0;
    lm_error(sp, ep, d.z, sinT, cosT, o.ev);
    // robust weight of e^T Lambda e (:113-115)
    const double w = lm_weight(a.kind, a.scale, lm_quad(o.ev, d.L));
    double W[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) W[k] = w * d.L[k];
    mat_mul_tn(o.Js, W, o.JsW);
    mat_mul_tn(o.Je, W, o.JeW);
}

__global__ __launch_bounds__(kLmThreads) void k_pg_linearise(LmArgs a, const double* __restrict__ poses, double lambda)
{
    const int e = blockIdx.x * kLmThreads + threadIdx.x;
    if (e >= a.blocks) return;
    const int s = gload(a.src + e);
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    EdgeLin t;
    double m[9];
    if (s == -1) {
        const int v = gload(a.col + e);
        double b[3] = { 0.0, 0.0, 0.0 }, bv[3];
        const int k0 = gload(a.nptr + v), k1 = gload(a.nptr + v + 1);
        for (int k = k0; k < k1; ++k) {
            const int code = gload(a.ninc + k), role = code & 3;
            linearise_edge(a, poses, code >> 2, t);
            if (role != 1) {   // this node starts the edge
                mat_mul(t.JsW, t.Js, m);
#pragma unroll
                for (int q = 0; q < 9; ++q) acc[q] += m[q];
            }
            if (role != 0) {   // and/or ends it
                mat_mul(t.JeW, t.Je, m);
#pragma unroll
                for (int q = 0; q < 9; ++q) acc[q] += m[q];
            }
            if (role == 2) {   // a self-loop: (s, e) and (e, s) fall on the diagonal block too
                mat_mul(t.JsW, t.Je, m);
#pragma unroll
                for (int q = 0; q < 9; ++q) acc[q] += m[q];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) acc[3 * i + j] += m[3 * j + i];
            }
            if (role != 1) {
                mat_mulv(t.JsW, t.ev, bv);
#pragma unroll
                for (int q = 0; q < 3; ++q) b[q] += bv[q];
            }
            if (role != 0) {
                mat_mulv(t.JeW, t.ev, bv);
#pragma unroll
                for (int q = 0; q < 3; ++q) b[q] += bv[q];
            }
        }
        // :167-172: fix node 0 with 1e9, then lambda on every diagonal entry
        if (v == 0) {
            acc[0] += 1e9;
            acc[4] += 1e9;
            acc[8] += 1e9;
        }
        acc[0] += lambda;
        acc[4] += lambda;
        acc[8] += lambda;
#pragma unroll
        for (int q = 0; q < 9; ++q) gstore(a.val + 9 * (size_t)e + q, acc[q]);
#pragma unroll
        for (int q = 0; q < 3; ++q) gstore(a.rhs + 3 * (size_t)v + q, -b[q]);
    } else {
        // the block (a, b), a < b, of pair p; stored transposed in row b
        const int p = s >= 0 ? s : -2 - s;
        const int k0 = gload(a.pptr + p), k1 = gload(a.pptr + p + 1);
        for (int k = k0; k < k1; ++k) {
            const int code = gload(a.pinc + k);
            linearise_edge(a, poses, code >> 1, t);
            mat_mul(t.JsW, t.Je, m);
            if (code & 1) {   // an edge b -> a: its block is (b, a)
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) acc[3 * j + i] += m[3 * i + j];
            } else {
#pragma unroll
                for (int q = 0; q < 9; ++q) acc[q] += m[q];
            }
        }
        if (s >= 0) {
#pragma unroll
            for (int q = 0; q < 9; ++q) gstore(a.val + 9 * (size_t)e + q, acc[q]);
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) gstore(a.val + 9 * (size_t)e + 3 * i + j, acc[3 * j + i]);
        }
    }
}

// thread i: node i's new pose (i < n) and edge i's loss term at the new poses (i < m)
__global__ __launch_bounds__(kLmThreads) void k_pg_update(LmArgs a, const double* __restrict__ poses,
                                                           const double* __restrict__ delta, double* __restrict__ next)
{
    const int i = blockIdx.x * kLmThreads + threadIdx.x;
    if (i < a.n) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const size_t r = 3 * (size_t)i + k;
            gstore(next + r, gload(poses + r) + gload(delta + r));   // :209-217
        }
    }
    if (i < a.m) {
        const Edge d = load_edge(a.edges, i);
        double sp[3], ep[3], ev[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {   // the expression that stores them above
            const size_t rs = 3 * (size_t)d.s + k, re = 3 * (size_t)d.e + k;
            sp[k] = gload(poses + rs) + gload(delta + rs);
            ep[k] = gload(poses + re) + gload(delta + re);
        }
        double sinT, cosT;
        lm_sincos(sp[2], &sinT, &cosT, &a.tail->err);
        lm_error(sp, ep, d.z, sinT, cosT, ev);
        gstore(a.loss + i, lm_loss(a.kind, a.scale, lm_quad(ev, d.L)));
    }
    if (i == 0) {
        a.tail->res.residual_norm2 = gload(&a.res->residual_norm2);
        a.tail->res.threshold = gload(&a.res->threshold);
        a.tail->res.iterations = gload(&a.res->iterations);
        a.tail->res.done = gload(&a.res->done);
    }
}

// A graph on the device: the pattern, the incidence lists, the edges, two
// pose buffers and the system the solve walks
struct Resident {
    LmArgs a;
    PgDeviceSystem sys;
    double* poses[2];
    size_t vb, mb, lb, pb;   // bytes of val, of a 3n vector, of the loss terms, of the poses (256-aligned)
    char* back;              // pinned: loss terms | LmTail (256) | the solve's two chunk records (256) | poses
    PglmPattern pat;
};

void resident_setup(lgs_ctx* ctx, const lgs_pose2d* poses, int n, const lgs_pg_edge* edges, int m, int kind,
                    double scale, Resident& R)
{
    static_assert(sizeof(lgs_pose2d) == 3 * sizeof(double) && sizeof(lgs_pg_edge) == 104, "poses and edges go up as they are");
    pglm_build(n, m, edges, R.pat);
    const PglmPattern& P = R.pat;
    const size_t blocks = P.pat.blocks(), np = (size_t)P.num_pairs(), mm = 3 * (size_t)n;
    LGS_HIP_CHECK(hipSetDevice(ctx->device));
    auto ib = [](size_t count) { return pg_align256(sizeof(int) * std::max<size_t>(count, 1)); };
    const size_t rpb = ib((size_t)n + 1), clb = ib(blocks);
    const size_t srb = ib(blocks), npb = ib((size_t)n + 1), nib = ib(P.ninc.size()), ppb = ib(np + 1), pib = ib(P.pinc.size());
    const size_t eb = pg_align256(sizeof(lgs_pg_edge) * std::max<size_t>((size_t)m, 1));
    const size_t incb = srb + npb + nib + ppb + pib + eb;
    R.vb = pg_align256(sizeof(double) * 9 * blocks);
    R.mb = pg_align256(sizeof(double) * mm);
    R.pb = R.mb;
    R.lb = pg_align256(sizeof(double) * std::max<size_t>((size_t)m, 1));

    ctx->pg_cache.reset();   // lgs_pg_cg_solve's pattern on the device is about to be overwritten
    // S_PG0 = rowptr | col and S_PG1 = val | rhs | x | result | work as lgs_pg_cg_solve lays them out,
    // S_PG2 = src | nptr | ninc | pptr | pinc | edges, S_PG3 = poses | poses | loss terms | LmTail
    char* d_pat = (char*)ctx->ensure(S_PG0, rpb + clb);
    char* d_sys = (char*)ctx->ensure(S_PG1, R.vb + 2 * R.mb + 256 + pg_work_bytes(ctx, n));
    char* d_inc = (char*)ctx->ensure(S_PG2, incb);
    char* d_pose = (char*)ctx->ensure(S_PG3, 2 * R.pb + R.lb + 256);
    char* pin = (char*)ctx->ensure_pinned_pg(rpb + clb + incb + R.pb);
    R.back = (char*)ctx->ensure_pinned(R.lb + 512 + R.pb);

    auto put = [](char* dst, const std::vector<int>& v) {
        if (!v.empty()) std::memcpy(dst, v.data(), sizeof(int) * v.size());
    };
    char* w = pin;
    put(w, P.pat.rowptr);
    put(w + rpb, P.pat.col);
    w += rpb + clb;
    put(w, P.pat.src);
    put(w + srb, P.nptr);
    put(w + srb + npb, P.ninc);
    put(w + srb + npb + nib, P.pptr);
    put(w + srb + npb + nib + ppb, P.pinc);
    if (m > 0) std::memcpy(w + srb + npb + nib + ppb + pib, edges, sizeof(lgs_pg_edge) * (size_t)m);
    w += incb;
    std::memcpy(w, poses, sizeof(lgs_pose2d) * (size_t)n);
    LGS_HIP_CHECK(hipMemcpyAsync(d_pat, pin, rpb + clb, hipMemcpyHostToDevice, ctx->stream));
    LGS_HIP_CHECK(hipMemcpyAsync(d_inc, pin + rpb + clb, incb, hipMemcpyHostToDevice, ctx->stream));
    LGS_HIP_CHECK(hipMemcpyAsync(d_pose, w, sizeof(lgs_pose2d) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    LGS_HIP_CHECK(hipMemsetAsync(d_pose + 2 * R.pb + R.lb, 0, 256, ctx->stream));
    ++ctx->pg_patterns;

    R.poses[0] = (double*)d_pose;
    R.poses[1] = (double*)(d_pose + R.pb);
    PgDeviceSystem& s = R.sys;
    s.rowptr = (const int*)d_pat;
    s.col = (const int*)(d_pat + rpb);
    s.val = (const double*)d_sys;
    s.rhs = (const double*)(d_sys + R.vb);
    s.x = (double*)(d_sys + R.vb + R.mb);
    s.res = (PgResult*)(d_sys + R.vb + 2 * R.mb);
    s.work = (double*)(d_sys + R.vb + 2 * R.mb + 256);
    s.seen = (PgResult*)(R.back + R.lb + 256);
    s.n = n;
    LmArgs& a = R.a;
    a.rowptr = s.rowptr;
    a.col = s.col;
    a.src = (const int*)d_inc;
    a.nptr = (const int*)(d_inc + srb);
    a.ninc = (const int*)(d_inc + srb + npb);
    a.pptr = (const int*)(d_inc + srb + npb + nib);
    a.pinc = (const int*)(d_inc + srb + npb + nib + ppb);
    a.edges = (const lgs_pg_edge*)(d_inc + srb + npb + nib + ppb + pib);
    a.val = (double*)d_sys;
    a.rhs = (double*)(d_sys + R.vb);
    a.loss = (double*)(d_pose + 2 * R.pb);
    a.tail = (LmTail*)(d_pose + 2 * R.pb + R.lb);
    a.res = s.res;
    a.scale = scale;
    a.kind = kind;
    a.n = n;
    a.m = m;
    a.blocks = (int)blocks;
}

void launch_linearise(lgs_ctx* ctx, const Resident& R, const double* poses, double lambda)
{
    hipLaunchKernelGGL(k_pg_linearise, dim3((R.a.blocks + kLmThreads - 1) / kLmThreads), dim3(kLmThreads), 0, ctx->stream,
                       R.a, poses, lambda);
    LGS_HIP_CHECK(hipGetLastError());
}

const char* const kArgsMessage =
    "pose-graph LM: 1 <= nodes <= 2^27, 0 <= edges <= 2^27, edge indices in [0, nodes), loss kind 0..6, damping "
    "factor, tolerance and loss scale finite";
const char* const kDomainMessage = "pose-graph LM: a start node's angle is outside the restated sincos's domain";

}  // namespace

extern "C" int lgs_pg_lm_optimize(lgs_ctx* ctx, const lgs_pg_lm_params* params, double* lambda, lgs_pose2d* poses, int n,
                                  const lgs_pg_edge* edges, int m, int* iterations, double* total_error,
                                  long long* cg_passes)
{
    if (!ctx || !params || !lambda || !poses || !iterations || !total_error || !cg_passes || (m > 0 && !edges))
        return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        LGS_REQUIRE(pglm_args_ok(n, m, edges, params->loss_kind, *lambda, params->error_tolerance, params->loss_scale),
                    kArgsMessage);
        Resident R;
        resident_setup(ctx, poses, n, edges, m, params->loss_kind, params->loss_scale, R);
        ++ctx->pglm_incidence_builds;
        ++ctx->pglm_pose_uploads;
        const size_t step_bytes = R.lb + sizeof(LmTail);
        const LmTail* const tail = (const LmTail*)(R.back + R.lb);
        const double* const terms = (const double*)R.back;
        const int threads = std::max(n, m);
        // Optimize (:13-65)
        double lam = *lambda, prev = DBL_MAX, total = DBL_MAX;
        int steps = 0, cur = 0;
        long long passes = 0;
        while (true) {
            launch_linearise(ctx, R, R.poses[cur], lam);
            const bool grid = pg_solve_enqueue(ctx, R.sys, 0.0, 0);   // Eigen's defaults
            hipLaunchKernelGGL(k_pg_update, dim3((threads + kLmThreads - 1) / kLmThreads), dim3(kLmThreads), 0,
                               ctx->stream, R.a, (const double*)R.poses[cur], (const double*)R.sys.x, R.poses[cur ^ 1]);
            LGS_HIP_CHECK(hipGetLastError());
            LGS_HIP_CHECK(hipMemcpyAsync(R.back, R.a.loss, step_bytes, hipMemcpyDeviceToHost, ctx->stream));
            ctx->sync();
            cur ^= 1;
            ++ctx->pg_solves;
            if (grid) ++ctx->pg_grid_solves;
            ctx->pg_iterations += tail->res.iterations;
            ++ctx->pglm_steps;
            passes += tail->res.iterations;
            if (tail->err) throw Error(LGS_ERR_INTERNAL, kDomainMessage);
            total = 0.0;
            for (int i = 0; i < m; ++i) total += terms[i];   // ComputeTotalError's order
            if (++steps >= params->num_iterations_max || std::fabs(prev - total) < params->error_tolerance) break;
            if (total < prev)
                lam *= 0.5;
            else
                lam *= 2.0;
            prev = total;
        }
        char* const down = R.back + R.lb + 512;
        LGS_HIP_CHECK(hipMemcpyAsync(down, R.poses[cur], sizeof(lgs_pose2d) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        ++ctx->pglm_pose_downloads;
        ++ctx->pglm_optimizes;
        std::memcpy(poses, down, sizeof(lgs_pose2d) * (size_t)n);
        *lambda = lam;
        *iterations = steps;
        *total_error = total;
        *cg_passes = passes;
    });
}

extern "C" int lgs_pg_lm_linearize(lgs_ctx* ctx, int loss_kind, double loss_scale, double lambda, const lgs_pose2d* poses,
                                   int n, const lgs_pg_edge* edges, int m, double* diag, int* num_pairs, int* pairs,
                                   double* off, double* rhs)
{
    if (!ctx || !poses || !diag || !num_pairs || !rhs || (m > 0 && (!edges || !pairs || !off))) return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        LGS_REQUIRE(pglm_args_ok(n, m, edges, loss_kind, lambda, 0.0, loss_scale), kArgsMessage);
        Resident R;
        resident_setup(ctx, poses, n, edges, m, loss_kind, loss_scale, R);
        launch_linearise(ctx, R, R.poses[0], lambda);
        // val | rhs are neighbours on the device; the step record follows them in the staging
        char* const back = (char*)ctx->ensure_pinned(R.vb + R.mb + 256);
        LGS_HIP_CHECK(hipMemcpyAsync(back, R.a.val, R.vb + R.mb, hipMemcpyDeviceToHost, ctx->stream));
        LGS_HIP_CHECK(hipMemcpyAsync(back + R.vb + R.mb, R.a.tail, sizeof(LmTail), hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        if (((const LmTail*)(back + R.vb + R.mb))->err) throw Error(LGS_ERR_INTERNAL, kDomainMessage);
        const PgPattern& pat = R.pat.pat;
        const double* val = (const double*)back;
        for (int v = 0; v < n; ++v) {
            const size_t e0 = (size_t)pat.rowptr[(size_t)v], e1 = (size_t)pat.rowptr[(size_t)v + 1];
            std::memcpy(diag + 9 * (size_t)v, val + 9 * e0, 9 * sizeof(double));
            for (size_t e = e0 + 1; e < e1; ++e)
                if (pat.src[e] >= 0) std::memcpy(off + 9 * (size_t)pat.src[e], val + 9 * e, 9 * sizeof(double));
        }
        std::memcpy(rhs, back + R.vb, sizeof(double) * 3 * (size_t)n);
        *num_pairs = R.pat.num_pairs();
        if (*num_pairs > 0) std::memcpy(pairs, R.pat.pairs.data(), sizeof(int) * R.pat.pairs.size());
    });
}

extern "C" int lgs_pg_lm_stats(const lgs_ctx* ctx, long long* optimizes, long long* steps, long long* pose_uploads,
                               long long* pose_downloads, long long* incidence_builds)
{
    if (!ctx) return LGS_ERR_INVALID_ARG;
    if (optimizes) *optimizes = ctx->pglm_optimizes;
    if (steps) *steps = ctx->pglm_steps;
    if (pose_uploads) *pose_uploads = ctx->pglm_pose_uploads;
    if (pose_downloads) *pose_downloads = ctx->pglm_pose_downloads;
    if (incidence_builds) *incidence_builds = ctx->pglm_incidence_builds;
    return LGS_OK;
}
