// k_hc.hip -- hill-climbing scan matcher on MI355X, with a greedy-endpoint
// cost that equals the reference's bit for bit.
//
// Restates ScanMatcherHillClimbing::OptimizePose
// (C/mapping/scan_matcher_hill_climbing.cpp:26-109) with CostGreedyEndpoint::Cost
// (C/mapping/cost_function_greedy_endpoint.cpp:32-111) and the poses of its
// ComputeGradient (:114-144).  DESIGN.md §4.6c has the exactness argument:
//
//   lgs_hc_term_table  the argument of the cost's exp() is -0.5 * minSquaredDist
//                 / variance, and minSquaredDist is GridMap::SquaredDistance of
//                 one of the (2K+1)^2 kernel offsets or of the start offset
//                 (K+1, K+1): at most (2K+1)^2 + 1 values.  The host evaluates
//                 them with libm's exp; the device only selects an entry
//   k_hc          one persistent workgroup per match walks the whole
//                 do/while: every thread forms the terms of its (neighbour,
//                 beam) pairs (glibc's sincos restated, IEEE subtraction,
//                 division and floor for the cells, the window scanned ky
//                 outer, kx inner), six lanes add the six rows in beam order,
//                 one lane takes the reference's decision.  The six
//                 central-difference costs of the covariance follow in the
//                 same launch
//   k_hc_cost     the cost code on its own at a list of poses
//   k_ge_cost_batch  one workgroup per (map, scan, sensor pose): the cost there
//                 and at the six poses of ComputeGradient around it -- what the
//                 branch-and-bound and grid-search matchers and their loop
//                 detectors derive from the cost after their search
//                 (LGS_COST_GREEDY_ENDPOINT_EXACT)
//
// The per-beam term and the chain live in ge_cost_device.hpp, which the
// correlative pipeline's exact cost stage (k_rtcsm.hip k_cost_gx) shares.
//
// Workgroups never wait for one another and the walk is bounded by the pass
// cap max(1, max_iterations).  The covariance, the normalized cost and the
// summary's pose algebra are formed on the host with glibc.
#include "ge_cost_device.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace lgs;

namespace {

constexpr int kHCThreads = 1024;
constexpr int kHCPoses = 6;                  // poses per cost pass (the six neighbours)
constexpr int kHCMaxIter = 65536;            // documented cap of max_iterations
constexpr size_t kHCLdsMax = 144 * 1024;     // term rows in LDS up to here (6 N doubles), else global rows
constexpr size_t kHCRowsCap = size_t(1) << 30;   // global term rows of the matches of one launch
constexpr int kHCChunk = 4096;               // matches per launch

struct HCRecord {
    double min_cost;
    double grad[6];          // costs at the poses of ComputeGradient: +x, -x, +y, -y, +theta, -theta
    double best[3];
    double lin_step, ang_step;
    int num_iterations, num_refinements, passes, cost_evals;
};

// Diagnostics build (make probe): thread 0 of block 0 adds up the 100 MHz wall
// clock of the two phases of hc_costs and prints the sums after the walk.
#ifdef LGS_PROBE
__device__ unsigned long long g_hc_probe[2];
#define HC_PROBE_T(k) const unsigned long long hc_pt##k = (threadIdx.x == 0 && blockIdx.x == 0) ? wall_clock64() : 0ull
#define HC_PROBE_ADD(k, a, b) do { if (threadIdx.x == 0 && blockIdx.x == 0) g_hc_probe[k] += hc_pt##b - hc_pt##a; } while (0)
#else
#define HC_PROBE_T(k) do { } while (0)
#define HC_PROBE_ADD(k, a, b) do { } while (0)
#endif

// The costs at np <= 6 sensor poses (s_pose, LDS) into s_cost.  Every thread of
// the workgroup calls it; ends with a workgroup barrier.
template <int KS>
__device__ __forceinline__ void hc_costs(const HCItem& it, const HCShared& sh, double (*s_pose)[3], int np,
                                         double* s_cost, double* l_rows, bool in_lds, int* __restrict__ err)
{
    const int N = it.N;
    const int total = np * N;
    double* __restrict__ g_rows = it.rows;
    HC_PROBE_T(0);
    for (int e = threadIdx.x; e < total; e += kHCThreads) {
        const int p = e / N, i = e - p * N;
        const double t = hc_term<KS>(it, sh, i, s_pose[p][0], s_pose[p][1], s_pose[p][2], err);
        if (in_lds)
            l_rows[e] = t;
        else
            g_rows[e] = t;
    }
    __syncthreads();
    HC_PROBE_T(1);
    if ((int)threadIdx.x < np) {   // lanes 0..np-1 of wave 0, side by side
        const size_t o = (size_t)threadIdx.x * N;
        s_cost[threadIdx.x] = in_lds ? hc_chain(l_rows + o, N, sh.scaling_factor)
                                     : hc_chain(g_rows + o, N, sh.scaling_factor);
    }
    __syncthreads();
    HC_PROBE_T(2);
    HC_PROBE_ADD(0, 0, 1);
    HC_PROBE_ADD(1, 1, 2);
}

// the six neighbour poses of a pass (:62-69): all three additions performed
__device__ __forceinline__ void hc_neighbours(double (*s_pose)[3], const double* best, double lin, double ang)
{
    const double moveX[6] = { 1.0, -1.0, 0.0, 0.0, 0.0, 0.0 };
    const double moveY[6] = { 0.0, 0.0, 1.0, -1.0, 0.0, 0.0 };
    const double moveTheta[6] = { 0.0, 0.0, 0.0, 0.0, 1.0, -1.0 };
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        s_pose[i][0] = best[0] + moveX[i] * lin;
        s_pose[i][1] = best[1] + moveY[i] * lin;
        s_pose[i][2] = best[2] + moveTheta[i] * ang;
    }
}

// the poses of ComputeGradient around (x, y, th) (:119-136)
__device__ __forceinline__ void hc_gradient_poses(double (*s_pose)[3], double x, double y, double th, double dl)
{
    const double da = 1e-2;
    const double v[6][3] = { { x + dl, y + 0.0, th + 0.0 }, { x - dl, y - 0.0, th - 0.0 },
                             { x + 0.0, y + dl, th + 0.0 }, { x - 0.0, y - dl, th - 0.0 },
                             { x + 0.0, y + 0.0, th + da }, { x - 0.0, y - 0.0, th - da } };
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) s_pose[i][j] = v[i][j];
}

template <int KS>
__global__ __launch_bounds__(kHCThreads) void k_hc(const HCItem* __restrict__ items, HCShared sh,
                                                   HCRecord* __restrict__ recs, int* __restrict__ err)
{
    extern __shared__ double l_rows[];   // [6][N] of the launch's largest in-LDS match
    __shared__ double s_pose[kHCPoses][3];
    __shared__ double s_cost[kHCPoses];
    __shared__ double s_best[3];
    __shared__ double s_min, s_lin, s_ang;
    __shared__ int s_iter, s_ref, s_go;
    const HCItem& it = items[blockIdx.x];
    const bool in_lds = sizeof(double) * (size_t)kHCPoses * (size_t)it.N <= (size_t)sh.lds_bytes;
    const bool t0 = threadIdx.x == 0;

    // minCost = Cost(sensorPose), bestPose = sensorPose (:44-45)
    if (t0) {
        s_pose[0][0] = it.sx;
        s_pose[0][1] = it.sy;
        s_pose[0][2] = it.st;
    }
    __syncthreads();
    hc_costs<KS>(it, sh, s_pose, 1, s_cost, l_rows, in_lds, err);
    if (t0) {
        s_min = s_cost[0];
        s_best[0] = it.sx;
        s_best[1] = it.sy;
        s_best[2] = it.st;
        s_lin = sh.lin_step;
        s_ang = sh.ang_step;
        s_iter = 0;
        s_ref = 0;
        hc_neighbours(s_pose, s_best, s_lin, s_ang);
    }
    __syncthreads();
    const int pass_cap = max(sh.max_iterations, 1);   // the do/while cannot run more passes
    int passes = 0;
    for (int pass = 0; pass < pass_cap; ++pass) {
        hc_costs<KS>(it, sh, s_pose, 6, s_cost, l_rows, in_lds, err);
        if (t0) {
            double minLocal = s_min;
            int move = -1;
#pragma unroll
            for (int i = 0; i < 6; ++i)   // strict <, index order (:75-79)
                if (s_cost[i] < minLocal) {
                    minLocal = s_cost[i];
                    move = i;
                }
            const bool updated = move >= 0;
            if (updated) {   // :83-85
                s_min = minLocal;
                s_best[0] = s_pose[move][0];
                s_best[1] = s_pose[move][1];
                s_best[2] = s_pose[move][2];
            } else {         // :86-91
                ++s_ref;
                s_lin *= 0.5;
                s_ang *= 0.5;
            }
            if (it.trace_move && pass < sh.trace_cap) {
                it.trace_move[pass] = move;
                it.trace_cost[pass] = s_min;
            }
            // (poseUpdated || numOfRefinements < max) && (++numOfIterations < max) (:92-93)
            bool go = updated || s_ref < sh.max_refinements;
            if (go) go = ++s_iter < sh.max_iterations;
            s_go = go ? 1 : 0;
            if (go) hc_neighbours(s_pose, s_best, s_lin, s_ang);
        }
        __syncthreads();
        ++passes;
        if (!s_go) break;
    }
    // the poses of ComputeGradient (:119-136)
    if (t0) hc_gradient_poses(s_pose, s_best[0], s_best[1], s_best[2], it.res);
    __syncthreads();
    hc_costs<KS>(it, sh, s_pose, 6, s_cost, l_rows, in_lds, err);
    if (t0) {
        HCRecord r;
        r.min_cost = s_min;
        for (int i = 0; i < 6; ++i) r.grad[i] = s_cost[i];
        for (int j = 0; j < 3; ++j) r.best[j] = s_best[j];
        r.lin_step = s_lin;
        r.ang_step = s_ang;
        r.num_iterations = s_iter;
        r.num_refinements = s_ref;
        r.passes = passes;
        r.cost_evals = 1 + 6 * passes + 6;
        recs[blockIdx.x] = r;
#ifdef LGS_PROBE
        if (blockIdx.x == 0) {
            printf("probe k_hc: %d passes, N %d: terms %.2f chains %.2f us\n", passes, it.N,
                   0.01 * (double)g_hc_probe[0], 0.01 * (double)g_hc_probe[1]);
            g_hc_probe[0] = g_hc_probe[1] = 0ull;
        }
#endif
    }
}

// the cost at poses[3 * k], k < n, of one scan: workgroup b takes poses 6b .. 6b + 5
template <int KS>
__global__ __launch_bounds__(kHCThreads) void k_hc_cost(const HCItem* __restrict__ items, HCShared sh,
                                                        const double* __restrict__ poses, int n,
                                                        double* __restrict__ out, int* __restrict__ err)
{
    extern __shared__ double l_rows[];
    __shared__ double s_pose[kHCPoses][3];
    __shared__ double s_cost[kHCPoses];
    HCItem it = items[0];
    const bool in_lds = sizeof(double) * (size_t)kHCPoses * (size_t)it.N <= (size_t)sh.lds_bytes;
    if (!in_lds) it.rows += (size_t)blockIdx.x * kHCPoses * it.N;
    const int k0 = blockIdx.x * kHCPoses;
    const int np = min(kHCPoses, n - k0);
    if ((int)threadIdx.x < 3 * np) s_pose[threadIdx.x / 3][threadIdx.x % 3] = poses[3 * k0 + threadIdx.x];
    __syncthreads();
    hc_costs<KS>(it, sh, s_pose, np, s_cost, l_rows, in_lds, err);
    if ((int)threadIdx.x < np) out[k0 + threadIdx.x] = s_cost[threadIdx.x];
}

// Item blockIdx.x: Cost at its sensor pose into out[7 b] and, with want_grad,
// at the six poses of ComputeGradient into out[7 b + 1 .. 7 b + 6].  The items
// of a launch may differ in map and resolution: each names its own term table.
template <int KS>
__global__ __launch_bounds__(kHCThreads) void k_ge_cost_batch(const HCItem* __restrict__ items, HCShared sh,
                                                              int want_grad, double* __restrict__ out,
                                                              int* __restrict__ err)
{
    extern __shared__ double l_rows[];
    __shared__ double s_pose[kHCPoses][3];
    __shared__ double s_cost[kHCPoses];
    const HCItem& it = items[blockIdx.x];
    sh.sq = it.tab;
    sh.term = it.tab + hc_table_len(KS > 0 ? KS : sh.K);
    const bool in_lds = sizeof(double) * (size_t)kHCPoses * (size_t)it.N <= (size_t)sh.lds_bytes;
    const bool t0 = threadIdx.x == 0;
    if (t0) {
        s_pose[0][0] = it.sx;
        s_pose[0][1] = it.sy;
        s_pose[0][2] = it.st;
    }
    __syncthreads();
    hc_costs<KS>(it, sh, s_pose, 1, s_cost, l_rows, in_lds, err);
    double* __restrict__ o = out + 7 * (size_t)blockIdx.x;
    if (t0) {
        o[0] = s_cost[0];
        hc_gradient_poses(s_pose, it.sx, it.sy, it.st, it.res);
    }
    if (!want_grad) return;
    __syncthreads();
    hc_costs<KS>(it, sh, s_pose, 6, s_cost, l_rows, in_lds, err);
    if ((int)threadIdx.x < 6) o[1 + threadIdx.x] = s_cost[threadIdx.x];
}

// ------------------------------------------------------------------ host
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

bool hc_cost_ok(const lgs_cost_ge_params* c, double res)
{
    return c && c->kernel_size >= 0 && c->kernel_size <= kHCMaxKernel && std::isfinite(res) && res > 0.0 &&
           std::isfinite(c->standard_deviation) && c->standard_deviation > 0.0;
}

void check_hc(const lgs_hc_params* p)
{
    LGS_REQUIRE(p, "null argument");
    LGS_REQUIRE(std::isfinite(p->linear_step) && p->linear_step > 0.0 && std::isfinite(p->angular_step) &&
                    p->angular_step > 0.0,
                "hill climbing: steps must be finite and > 0");
    LGS_REQUIRE(p->max_iterations <= kHCMaxIter, "hill climbing: more than 65536 iterations");
}

bool pose_finite(const lgs_pose2d& p) { return std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.theta); }

template <class K>
void hc_allow_lds(K kernel, size_t bytes)
{
    // dynamic LDS beyond the 64 KiB default has to be announced; launches
    // report what this leaves unsaid
    if (bytes > 64 * 1024) {
        (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        (void)hipGetLastError();
    }
}

HCItem hc_item(const lgs_grid* g, const lgs_cost_ge_params* cost, const lgs_scan* s, lgs_pose2d sensor)
{
    HCItem it;
    std::memset(&it, 0, sizeof(it));
    it.sx = sensor.x;
    it.sy = sensor.y;
    it.st = sensor.theta;
    it.min_x = g->min_x;
    it.min_y = g->min_y;
    it.res = g->res;
    it.min_range = std::max(cost->usable_range_min, s->min_range);   // :38-41
    it.max_range = std::min(cost->usable_range_max, s->max_range);
    it.W = g->w;
    it.H = g->h;
    it.N = s->n;
    it.map = g->d;
    it.ranges = s->d_ranges;
    it.angles = s->d_angles;
    return it;
}

size_t hc_rows_bytes(int N) { return sizeof(double) * (size_t)kHCPoses * (size_t)N; }

HCShared hc_shared(const lgs_hc_params* p, const lgs_cost_ge_params* cost)
{
    HCShared sh;
    std::memset(&sh, 0, sizeof(sh));
    if (p) {
        sh.lin_step = p->linear_step;
        sh.ang_step = p->angular_step;
        sh.max_iterations = p->max_iterations;
        sh.max_refinements = p->max_num_of_refinements;
    }
    sh.hit_and_missed_dist = cost->hit_and_missed_dist;
    sh.occupancy_threshold = cost->occupancy_threshold;
    sh.scaling_factor = cost->scaling_factor;
    sh.K = cost->kernel_size;
    return sh;
}

// n matches: grids[j], scans[j], init[j].  Matches are grouped by map
// resolution (the term table depends on it) and launched in chunks.  Trace
// (n == 1 only): the per-pass (move, minCost).
void run_hc(lgs_ctx* ctx, const lgs_hc_params* p, const lgs_cost_ge_params* cost, const lgs_grid* const* grids,
            lgs_scan* const* scans, const lgs_pose2d* init, int n, lgs_hc_summary* out, int* trace_moves = nullptr,
            double* trace_costs = nullptr, int trace_cap = 0)
{
    for (int j = 0; j < n; ++j) {
        LGS_REQUIRE(grids[j] && scans[j] && scans[j]->n >= 1, "hill climbing: null map or empty scan");
        LGS_REQUIRE(hc_cost_ok(cost, grids[j]->res), "hill climbing: kernel size in [0, 16], resolution and "
                                                     "standard deviation finite and > 0");
        LGS_REQUIRE(pose_finite(init[j]), "hill climbing: initial pose not finite");
        LGS_REQUIRE((long long)grids[j]->w * grids[j]->h < (1LL << 30), "hill climbing: map of 2^30 cells or more");
    }
    for (int k = 0; k < n; ++k) grid_acquire(ctx, grids[k]);
    LGS_HIP_CHECK(hipSetDevice(ctx->device));
    std::vector<HCRecord> recs((size_t)n);
    std::vector<lgs_pose2d> sensor((size_t)n);
    for (int j = 0; j < n; ++j) sensor[(size_t)j] = compound(init[j], scans[j]->rel);   // :40-41
    const int pass_cap = std::max(p->max_iterations, 1);

    std::vector<char> done((size_t)n, 0);
    for (int j0 = 0; j0 < n; ++j0) {
        if (done[(size_t)j0]) continue;
        // the next chunk: matches of j0's resolution, in order
        const double res = grids[j0]->res;
        std::vector<int> idx;
        size_t rows_total = 0, lds = 0;
        for (int j = j0; j < n && (int)idx.size() < kHCChunk; ++j) {
            if (done[(size_t)j] || grids[j]->res != res) continue;
            const size_t rb = hc_rows_bytes(scans[j]->n);
            if (rb > kHCLdsMax) {
                if (!idx.empty() && rows_total + align256(rb) > kHCRowsCap) break;
                rows_total += align256(rb);
            } else
                lds = std::max(lds, rb);
            idx.push_back(j);
            done[(size_t)j] = 1;
        }
        const int m = (int)idx.size();
        std::vector<const lgs_scan*> sc((size_t)m);
        for (int k = 0; k < m; ++k) sc[(size_t)k] = scans[idx[(size_t)k]];
        scans_to_device(ctx, sc.data(), m);
        char* rows = rows_total ? (char*)ctx->ensure(S_HC0, rows_total) : nullptr;
        const size_t rb = align256(sizeof(HCRecord) * (size_t)m);
        const size_t tmb = trace_moves ? align256(sizeof(int) * (size_t)pass_cap) : 0;
        const size_t tcb = trace_moves ? align256(sizeof(double) * (size_t)pass_cap) : 0;
        char* small = (char*)ctx->ensure(S_HC1, rb + tmb + tcb + 256);
        HCRecord* d_rec = (HCRecord*)small;
        int* d_tm = trace_moves ? (int*)(small + rb) : nullptr;
        double* d_tc = trace_moves ? (double*)(small + rb + tmb) : nullptr;
        int* d_err = (int*)(small + rb + tmb + tcb);
        LGS_HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream));

        std::vector<double> sq, term;
        hc_table(cost, res, sq, term);
        std::vector<HCItem> items((size_t)m);
        size_t roff = 0;
        for (int k = 0; k < m; ++k) {
            const int j = idx[(size_t)k];
            HCItem& it = items[(size_t)k];
            it = hc_item(grids[j], cost, scans[j], sensor[(size_t)j]);
            const size_t b = hc_rows_bytes(scans[j]->n);
            if (b > kHCLdsMax) {
                it.rows = (double*)(rows + roff);
                roff += align256(b);
            }
            it.trace_move = d_tm;
            it.trace_cost = d_tc;
        }
        Upload up(ctx);
        const size_t so = up.append(sq.data(), sq.size());
        const size_t to = up.append(term.data(), term.size());
        const size_t io = up.append(items.data(), items.size());
        up.flush();
        HCShared sh = hc_shared(p, cost);
        sh.sq = up.at<double>(so);
        sh.term = up.at<double>(to);
        sh.trace_cap = trace_moves ? pass_cap : 0;
        sh.lds_bytes = (unsigned)lds;
        if (cost->kernel_size == 1) {
            hc_allow_lds(k_hc<1>, lds);
            hipLaunchKernelGGL(k_hc<1>, dim3(m), dim3(kHCThreads), lds, ctx->stream, up.at<HCItem>(io), sh, d_rec,
                               d_err);
        } else {
            hc_allow_lds(k_hc<0>, lds);
            hipLaunchKernelGGL(k_hc<0>, dim3(m), dim3(kHCThreads), lds, ctx->stream, up.at<HCItem>(io), sh, d_rec,
                               d_err);
        }
        LGS_HIP_CHECK(hipGetLastError());
        const size_t hb = rb + tmb + tcb + 256;
        char* pin = (char*)ctx->ensure_pinned(hb);
        LGS_HIP_CHECK(hipMemcpyAsync(pin, small, hb, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        if (*(const int*)(pin + rb + tmb + tcb) != 0)
            throw Error(LGS_ERR_INTERNAL, "hill climbing: an angle lies outside the restated sincos domain");
        for (int k = 0; k < m; ++k) std::memcpy(&recs[(size_t)idx[(size_t)k]], pin + sizeof(HCRecord) * (size_t)k,
                                                sizeof(HCRecord));
        if (trace_moves) {
            const int np = std::min(recs[(size_t)idx[0]].passes, trace_cap);
            std::memcpy(trace_moves, pin + rb, sizeof(int) * (size_t)np);
            std::memcpy(trace_costs, pin + rb + tmb, sizeof(double) * (size_t)np);
        }
    }

    for (int j = 0; j < n; ++j) {
        const HCRecord& r = recs[(size_t)j];
        lgs_hc_summary& o = out[j];
        std::memset(&o, 0, sizeof(o));
        const lgs_pose2d best{ r.best[0], r.best[1], r.best[2] };
        o.pose_found = 1;                                          // :106-108
        o.normalized_cost = r.min_cost / (double)scans[j]->n;      // :96
        o.initial_pose = init[j];
        o.estimated_pose = move_backward(best, scans[j]->rel);     // :98-99
        // ComputeGradient (:138-141) and ComputeCovariance (:147-171)
        const double dl = grids[j]->res, da = 1e-2;
        const double dX = r.grad[0] - r.grad[1], dY = r.grad[2] - r.grad[3], dT = r.grad[4] - r.grad[5];
        const double gv[3] = { 0.5 * dX / dl, 0.5 * dY / dl, 0.5 * dT / da };
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) o.covariance[3 * a + b] = gv[a] * gv[b];
        o.covariance[0] += 0.01;
        o.covariance[4] += 0.01;
        o.covariance[8] += 0.01;
        o.best_sensor_pose = best;
        o.min_cost = r.min_cost;
        o.final_linear_step = r.lin_step;
        o.final_angular_step = r.ang_step;
        o.num_iterations = r.num_iterations;
        o.num_refinements = r.num_refinements;
        o.passes = r.passes;
        o.cost_evals = r.cost_evals;
    }
}

}  // namespace

extern "C" int lgs_hc_term_table(const lgs_cost_ge_params* cost, double res, double* sq, double* term, int cap)
{
    if (!hc_cost_ok(cost, res) || cap < 0 || (cap > 0 && (!sq || !term))) return -LGS_ERR_INVALID_ARG;
    try {
        std::vector<double> s, t;
        hc_table(cost, res, s, t);
        for (size_t q = 0; q < s.size() && q < (size_t)cap; ++q) {
            sq[q] = s[q];
            term[q] = t[q];
        }
        return (int)s.size();
    } catch (...) {
        return -LGS_ERR_OOM;
    }
}

extern "C" int lgs_hc_optimize_pose_batch(lgs_ctx* ctx, const lgs_grid* const* grids, const lgs_hc_params* params,
                                          const lgs_cost_ge_params* cost, const lgs_scan* const* scans,
                                          const lgs_pose2d* initial, int n, lgs_hc_summary* out)
{
    if (!ctx || !params || !cost || n < 0 || (n > 0 && (!grids || !scans || !initial || !out)))
        return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        check_hc(params);
        LGS_REQUIRE(cost->kernel_size >= 0 && cost->kernel_size <= kHCMaxKernel, "hill climbing: kernel size in [0, 16]");
        if (n == 0) return;
        std::vector<lgs_scan*> sc((size_t)n);
        for (int j = 0; j < n; ++j) sc[(size_t)j] = const_cast<lgs_scan*>(scans[j]);
        run_hc(ctx, params, cost, grids, sc.data(), initial, n, out);
    });
}

extern "C" int lgs_hc_optimize_pose_query(lgs_ctx* ctx, const lgs_grid* grid, const lgs_hc_params* params,
                                          const lgs_cost_ge_params* cost, const lgs_scan* scan, lgs_pose2d initial,
                                          lgs_hc_summary* out)
{
    if (!grid || !scan || !out) return LGS_ERR_INVALID_ARG;
    return lgs_hc_optimize_pose_batch(ctx, &grid, params, cost, &scan, &initial, 1, out);
}

extern "C" int lgs_hc_trace(lgs_ctx* ctx, const lgs_grid* grid, const lgs_hc_params* params,
                            const lgs_cost_ge_params* cost, const lgs_scan* scan, lgs_pose2d initial, int* moves,
                            double* costs, int cap)
{
    if (!ctx || !grid || !params || !cost || !scan || cap < 0 || (cap > 0 && (!moves || !costs)))
        return -LGS_ERR_INVALID_ARG;
    int passes = 0;
    const int rc = guarded(ctx, [&] {
        check_hc(params);
        lgs_scan* s = const_cast<lgs_scan*>(scan);
        lgs_hc_summary sum;
        const int pass_cap = std::max(params->max_iterations, 1);
        std::vector<int> mv((size_t)pass_cap);
        std::vector<double> cs((size_t)pass_cap);
        run_hc(ctx, params, cost, &grid, &s, &initial, 1, &sum, mv.data(), cs.data(), pass_cap);
        passes = sum.passes;
        for (int k = 0; k < passes && k < cap; ++k) {
            moves[k] = mv[(size_t)k];
            costs[k] = cs[(size_t)k];
        }
    });
    return rc == LGS_OK ? passes : -rc;
}

extern "C" int lgs_cost_ge_exact(lgs_ctx* ctx, const lgs_grid* grid, const lgs_cost_ge_params* cost,
                                 const lgs_scan* scan, const lgs_pose2d* poses, int n, double* out)
{
    if (!ctx || !grid || !cost || !scan || n < 0 || (n > 0 && (!poses || !out))) return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        LGS_REQUIRE(hc_cost_ok(cost, grid->res), "exact cost: kernel size in [0, 16], resolution and standard "
                                                 "deviation finite and > 0");
        LGS_REQUIRE(scan->n >= 1, "empty scan");
        LGS_REQUIRE((long long)grid->w * grid->h < (1LL << 30), "exact cost: map of 2^30 cells or more");
        for (int k = 0; k < n; ++k) LGS_REQUIRE(pose_finite(poses[k]), "exact cost: pose not finite");
        if (n == 0) return;
        grid_acquire(ctx, grid);
        LGS_HIP_CHECK(hipSetDevice(ctx->device));
        scans_to_device(ctx, &scan, 1);
        const int nb = (n + kHCPoses - 1) / kHCPoses;
        const size_t rowb = hc_rows_bytes(scan->n);
        const bool in_lds = rowb <= kHCLdsMax;
        const size_t lds = in_lds ? rowb : 0;
        // launches of at most this many workgroups keep the global rows within the cap
        const int nb_launch = in_lds ? nb : (int)std::max<size_t>(1, std::min<size_t>((size_t)nb, kHCRowsCap / rowb));
        HCItem it = hc_item(grid, cost, scan, lgs_pose2d{ 0, 0, 0 });
        if (!in_lds) it.rows = (double*)ctx->ensure(S_HC0, rowb * (size_t)nb_launch);
        const size_t ob = align256(sizeof(double) * (size_t)n);
        char* small = (char*)ctx->ensure(S_HC1, ob + 256);
        double* d_out = (double*)small;
        int* d_err = (int*)(small + ob);
        LGS_HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream));
        std::vector<double> sq, term;
        hc_table(cost, grid->res, sq, term);
        Upload up(ctx);
        const size_t so = up.append(sq.data(), sq.size());
        const size_t to = up.append(term.data(), term.size());
        const size_t io = up.append(&it, 1);
        const size_t po = up.append(poses, (size_t)n);
        up.flush();
        HCShared sh = hc_shared(nullptr, cost);
        sh.sq = up.at<double>(so);
        sh.term = up.at<double>(to);
        sh.lds_bytes = (unsigned)lds;
        for (int b0 = 0; b0 < nb; b0 += nb_launch) {
            const int nbk = std::min(nb_launch, nb - b0);
            const int k0 = b0 * kHCPoses, nk = std::min(n - k0, nbk * kHCPoses);
            const double* d_poses = up.at<double>(po) + 3 * (size_t)k0;
            if (cost->kernel_size == 1) {
                hc_allow_lds(k_hc_cost<1>, lds);
                hipLaunchKernelGGL(k_hc_cost<1>, dim3(nbk), dim3(kHCThreads), lds, ctx->stream, up.at<HCItem>(io), sh,
                                   d_poses, nk, d_out + k0, d_err);
            } else {
                hc_allow_lds(k_hc_cost<0>, lds);
                hipLaunchKernelGGL(k_hc_cost<0>, dim3(nbk), dim3(kHCThreads), lds, ctx->stream, up.at<HCItem>(io), sh,
                                   d_poses, nk, d_out + k0, d_err);
            }
            LGS_HIP_CHECK(hipGetLastError());
        }
        char* pin = (char*)ctx->ensure_pinned(ob + 256);
        LGS_HIP_CHECK(hipMemcpyAsync(pin, small, ob + 256, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        if (*(const int*)(pin + ob) != 0)
            throw Error(LGS_ERR_INTERNAL, "exact cost: an angle lies outside the restated sincos domain");
        std::memcpy(out, pin, sizeof(double) * (size_t)n);
    });
}

// ---------------------------------------------------------------------------
// The cost and its covariance at many (map, scan, sensor pose) items
// (LGS_COST_GREEDY_ENDPOINT_EXACT for the branch-and-bound and grid-search
// matchers)
// ---------------------------------------------------------------------------

// The device term table of (cost, res): lgs_hc_term_table's squared distances,
// then its terms.  Built and uploaded (on the context's stream, ahead of the
// launches that read it) the first time a key is seen.
const double* lgs_ctx::ge_table(const lgs_cost_ge_params* cost, double res)
{
    for (const GeTable& t : ge_tables)
        if (t.K == cost->kernel_size && t.sd == cost->standard_deviation && t.res == res) return t.dev;
    if (ge_tables.size() >= 64) {   // a caller sweeping parameters: start over
        sync();
        if (hi) LGS_HIP_CHECK(hipStreamSynchronize(hi));   // a chunk's tail may still read a table there
        for (GeTable& t : ge_tables) (void)hipFree(t.dev);
        ge_tables.clear();
    }
    GeTable t;
    t.K = cost->kernel_size;
    t.sd = cost->standard_deviation;
    t.res = res;
    t.dev = nullptr;
    std::vector<double> sq, term;
    hc_table(cost, res, sq, term);
    t.host = sq;
    t.host.insert(t.host.end(), term.begin(), term.end());
    LGS_HIP_CHECK(hipSetDevice(device));
    LGS_HIP_CHECK(hipMalloc((void**)&t.dev, sizeof(double) * t.host.size()));
    ge_tables.push_back(std::move(t));
    const GeTable& k = ge_tables.back();   // the vector's buffer moves with it: k.host.data() stays
    LGS_HIP_CHECK(hipMemcpyAsync(k.dev, k.host.data(), sizeof(double) * k.host.size(), hipMemcpyHostToDevice, stream));
    return k.dev;
}

namespace {

// ComputeGradient (:138-141) and ComputeCovariance (:147-171) from the costs at
// the six central-difference poses
void ge_covariance(const double* c7, double res, double* cov)
{
    const double dl = res, da = 1e-2;
    const double g[3] = { 0.5 * (c7[1] - c7[2]) / dl, 0.5 * (c7[3] - c7[4]) / dl, 0.5 * (c7[5] - c7[6]) / da };
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) cov[3 * a + b] = g[a] * g[b];
    cov[0] += 0.01;
    cov[4] += 0.01;
    cov[8] += 0.01;
}

// costs7[7 j ..]: Cost at sensor[j] and (want_grad) at the six gradient poses.
// Chunks are runs of at most kHCChunk items in order, all launched before the
// one synchronisation; they run one after another and share the global rows.
void run_ge_batch(lgs_ctx* ctx, const lgs_cost_ge_params* cost, const lgs_grid* const* grids,
                  const lgs_scan* const* scans, const lgs_pose2d* sensor, int n, bool want_grad, double* costs7)
{
    for (int j = 0; j < n; ++j) {
        LGS_REQUIRE(grids[j] && grids[j]->d && scans[j] && scans[j]->n >= 1, "exact cost: null map or empty scan");
        LGS_REQUIRE(hc_cost_ok(cost, grids[j]->res), "exact cost: kernel size in [0, 16], resolution and standard "
                                                     "deviation finite and > 0");
        LGS_REQUIRE((long long)grids[j]->w * grids[j]->h < (1LL << 30), "exact cost: map of 2^30 cells or more");
        LGS_REQUIRE(pose_finite(sensor[j]), "exact cost: pose not finite");
    }
    if (n == 0) return;
    for (int k = 0; k < n; ++k) grid_acquire(ctx, grids[k]);
    LGS_HIP_CHECK(hipSetDevice(ctx->device));
    struct Chunk { int j0, j1; size_t lds, rows; };
    std::vector<Chunk> chunks;
    size_t rows_max = 0;
    for (int j = 0; j < n;) {
        Chunk c{ j, j, 0, 0 };
        for (; c.j1 < n && c.j1 - c.j0 < kHCChunk; ++c.j1) {
            const size_t rb = hc_rows_bytes(scans[c.j1]->n);
            if (rb > kHCLdsMax) {
                if (c.j1 > c.j0 && c.rows + align256(rb) > kHCRowsCap) break;
                c.rows += align256(rb);
            } else
                c.lds = std::max(c.lds, rb);
        }
        rows_max = std::max(rows_max, c.rows);
        chunks.push_back(c);
        j = c.j1;
    }
    scans_to_device(ctx, scans, n);
    char* rows = rows_max ? (char*)ctx->ensure(S_HC0, rows_max) : nullptr;
    const size_t ob = align256(sizeof(double) * 7 * (size_t)n);
    char* small = (char*)ctx->ensure(S_HC1, ob + 256);
    double* d_out = (double*)small;
    int* d_err = (int*)(small + ob);
    LGS_HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream));
    if (!want_grad) LGS_HIP_CHECK(hipMemsetAsync(d_out, 0, ob, ctx->stream));
    std::vector<HCItem> items((size_t)n);
    for (const Chunk& c : chunks) {
        size_t roff = 0;
        for (int j = c.j0; j < c.j1; ++j) {
            HCItem& it = items[(size_t)j];
            it = hc_item(grids[j], cost, scans[j], sensor[j]);
            it.tab = ctx->ge_table(cost, grids[j]->res);
            const size_t b = hc_rows_bytes(scans[j]->n);
            if (b > kHCLdsMax) {
                it.rows = (double*)(rows + roff);
                roff += align256(b);
            }
        }
    }
    Upload up(ctx);
    const size_t io = up.append(items.data(), items.size());
    up.flush();
    HCShared sh = hc_shared(nullptr, cost);
    for (const Chunk& c : chunks) {
        sh.lds_bytes = (unsigned)c.lds;
        const HCItem* d_items = up.at<HCItem>(io) + c.j0;
        if (cost->kernel_size == 1) {
            hc_allow_lds(k_ge_cost_batch<1>, c.lds);
            hipLaunchKernelGGL(k_ge_cost_batch<1>, dim3(c.j1 - c.j0), dim3(kHCThreads), c.lds, ctx->stream, d_items, sh,
                               want_grad ? 1 : 0, d_out + 7 * (size_t)c.j0, d_err);
        } else {
            hc_allow_lds(k_ge_cost_batch<0>, c.lds);
            hipLaunchKernelGGL(k_ge_cost_batch<0>, dim3(c.j1 - c.j0), dim3(kHCThreads), c.lds, ctx->stream, d_items, sh,
                               want_grad ? 1 : 0, d_out + 7 * (size_t)c.j0, d_err);
        }
        LGS_HIP_CHECK(hipGetLastError());
    }
    char* pin = (char*)ctx->ensure_pinned(ob + 256);
    LGS_HIP_CHECK(hipMemcpyAsync(pin, small, ob + 256, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    if (*(const int*)(pin + ob) != 0)
        throw Error(LGS_ERR_INTERNAL, "exact cost: an angle lies outside the restated sincos domain");
    std::memcpy(costs7, pin, sizeof(double) * 7 * (size_t)n);
}

}  // namespace

namespace lgs {
// What the branch-and-bound and grid-search matchers derive from their cost
// function after the search (scan_matcher_branch_bound.cpp:146-153,
// scan_matcher_grid_search.cpp:97-107), the greedy-endpoint cost bit for bit:
// normalized cost, estimated pose and covariance at best[j]
void cost_summaries_gx(lgs_ctx* ctx, const lgs_grid* const* grids, const lgs_cost_ge_params* cost,
                       lgs_scan* const* scans, const lgs_pose2d* best, int n, lgs_rtcsm_summary* out)
{
    if (n <= 0) return;
    std::vector<double> c7(7 * (size_t)n);
    run_ge_batch(ctx, cost, grids, scans, best, n, true, c7.data());
    for (int j = 0; j < n; ++j) {
        out[j].normalized_cost = c7[7 * (size_t)j] / (double)scans[j]->n;
        out[j].estimated_pose = move_backward(best[j], scans[j]->rel);
        ge_covariance(&c7[7 * (size_t)j], grids[j]->res, out[j].covariance);
    }
}
}  // namespace lgs

extern "C" int lgs_cost_ge_exact_batch(lgs_ctx* ctx, const lgs_grid* const* grids, const lgs_cost_ge_params* cost,
                                       const lgs_scan* const* scans, const lgs_pose2d* sensor_poses, int n,
                                       double* out_cost, double* out_covariance)
{
    if (!ctx || !cost || n < 0 || (n > 0 && (!grids || !scans || !sensor_poses || !out_cost)))
        return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        std::vector<double> c7(7 * (size_t)n);
        run_ge_batch(ctx, cost, grids, scans, sensor_poses, n, out_covariance != nullptr, c7.data());
        for (int j = 0; j < n; ++j) {
            out_cost[j] = c7[7 * (size_t)j];
            if (out_covariance) ge_covariance(&c7[7 * (size_t)j], grids[j]->res, out_covariance + 9 * (size_t)j);
        }
    });
}

extern "C" int lgs_summaries_apply_cost_ge_exact(lgs_ctx* ctx, const lgs_grid* const* grids,
                                                 const lgs_cost_ge_params* cost, const lgs_scan* const* scans,
                                                 lgs_rtcsm_summary* summaries, int n)
{
    if (!ctx || !cost || n < 0 || (n > 0 && (!grids || !scans || !summaries))) return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        std::vector<double> c7(7 * (size_t)n);
        std::vector<lgs_pose2d> poses((size_t)n);
        for (int j = 0; j < n; ++j) poses[(size_t)j] = summaries[j].best_sensor_pose;
        run_ge_batch(ctx, cost, grids, scans, poses.data(), n, true, c7.data());
        for (int j = 0; j < n; ++j) {
            summaries[j].normalized_cost = c7[7 * (size_t)j] / (double)scans[j]->n;
            ge_covariance(&c7[7 * (size_t)j], grids[j]->res, summaries[j].covariance);
        }
    });
}
