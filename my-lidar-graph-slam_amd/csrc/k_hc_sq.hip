// k_hc_sq.hip -- CostSquareError for every scan matcher on MI355X: the
// hill-climbing walk over the square-error cost, and the cost and covariance
// at given sensor poses in batches (what the three search matchers evaluate at
// their best pose).  Every value equals the reference's bit for bit.
//
// Restates ScanMatcherHillClimbing::OptimizePose
// (C/mapping/scan_matcher_hill_climbing.cpp:26-109) with CostSquareError
// (C/mapping/cost_function_square_error.cpp: Cost :21-58, ComputeGradient
// :61-109, ComputeCovariance :112-135).  The per-beam arithmetic is that of
// k_linsolve.hip (sq_cost_device.hpp); DESIGN.md §4.5 and §4.6d have the
// exactness argument.
//
//   k_hc_sq          one persistent workgroup per match walks the whole
//                    do/while, as k_hc does: every thread forms the terms
//                    (1 - S(hit point))^2 of its (neighbour, beam) pairs, six
//                    lanes add the six rows in beam order, one lane takes the
//                    reference's decision.  The gradient sums of the
//                    covariance at the best pose follow in the same launch
//   k_sq_cost_batch  one workgroup per (map, scan, sensor pose): the cost, or
//                    the cost and the three gradient sums
//
// A filtered beam's terms are +0.0.  Every chain starts at +0.0 and a sum of
// two doubles is -0.0 only if both are, so no chain ever holds -0.0 and
// adding +0.0 leaves its bits as they are, also where the gradient terms are
// negative: the same as skipping the beam, which is what the reference does.
//
// Workgroups never wait for one another and the walk is bounded by the pass
// cap max(1, max_iterations).  The covariance, the normalized cost and the
// summary's pose algebra are formed on the host with glibc.
#include "lgs_internal.hpp"
#include "glibc_math.hpp"
#include "sq_cost_stage.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace lgs;

namespace {

constexpr int kSqPoses = 6;                  // poses per cost pass (the six neighbours)
constexpr int kSqMaxIter = 65536;            // documented cap of max_iterations
constexpr size_t kSqRowsCap = size_t(1) << 30;   // global term rows of the matches of one launch
constexpr int kSqChunk = 4096;               // items per launch

struct SqRecord {
    double min_cost;
    double grad[3];          // ComputeGradient's sums of 2 e (-g) at the best pose (:61-109)
    double best[3];
    double lin_step, ang_step;
    int num_iterations, num_refinements, passes, cost_evals;
};

// What every item of a launch shares.
struct SqShared {
    double lin_step, ang_step;
    int max_iterations, max_refinements, trace_cap;
    int nrows;                  // term rows per item: 6 (walk), 4 (cost and gradient), 1 (cost)
    unsigned lds_bytes;         // dynamic LDS of the launch
};

// Diagnostics build (make probe): thread 0 of block 0 adds up the 100 MHz wall
// clock of the two phases of sq_costs and prints the sums after the walk.
#ifdef LGS_PROBE
__device__ unsigned long long g_sq_probe[2];
#define SQ_PROBE_T(k) const unsigned long long sq_pt##k = (threadIdx.x == 0 && blockIdx.x == 0) ? wall_clock64() : 0ull
#define SQ_PROBE_ADD(k, a, b) do { if (threadIdx.x == 0 && blockIdx.x == 0) g_sq_probe[k] += sq_pt##b - sq_pt##a; } while (0)
#else
#define SQ_PROBE_T(k) do { } while (0)
#define SQ_PROBE_ADD(k, a, b) do { } while (0)
#endif

// The costs at np <= 6 sensor poses (s_pose, LDS) into s_cost.  Every thread of
// the workgroup calls it; ends with a workgroup barrier.
__device__ __forceinline__ void sq_costs(const SqItem& it, double (*s_pose)[3], int np, double* s_cost,
                                         double* l_rows, bool in_lds, int* __restrict__ err)
{
    const int N = it.p.N;
    const int total = np * N;
    double* __restrict__ g_rows = it.rows;
    SQ_PROBE_T(0);
    for (int e = threadIdx.x; e < total; e += kSqThreads) {
        const int p = e / N, i = e - p * N;
        const double pose[3] = { s_pose[p][0], s_pose[p][1], s_pose[p][2] };
        const double t = sq_term(it, i, pose, err);
        if (in_lds)
            l_rows[e] = t;
        else
            g_rows[e] = t;
    }
    __syncthreads();
    SQ_PROBE_T(1);
    if ((int)threadIdx.x < np) {   // lanes 0..np-1 of wave 0, side by side
        const size_t o = (size_t)threadIdx.x * N;
        s_cost[threadIdx.x] = in_lds ? sq_chain(l_rows + o, N) : sq_chain(g_rows + o, N);
    }
    __syncthreads();
    SQ_PROBE_T(2);
    SQ_PROBE_ADD(0, 0, 1);
    SQ_PROBE_ADD(1, 1, 2);
}

// the six neighbour poses of a pass (:62-69): all three additions performed
__device__ __forceinline__ void sq_neighbours(double (*s_pose)[3], const double* best, double lin, double ang)
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

__device__ __forceinline__ bool sq_in_lds(const SqItem& it, const SqShared& sh)
{
    return sizeof(double) * (size_t)sh.nrows * (size_t)it.p.N <= (size_t)sh.lds_bytes;
}

__global__ __launch_bounds__(kSqThreads) void k_hc_sq(const SqItem* __restrict__ items, SqShared sh,
                                                      SqRecord* __restrict__ recs, int* __restrict__ err)
{
    extern __shared__ double l_rows[];   // [6][N] of the launch's largest in-LDS match
    __shared__ double s_pose[kSqPoses][3];
    __shared__ double s_cost[kSqPoses];
    __shared__ double s_best[3];
    __shared__ double s_min, s_lin, s_ang;
    __shared__ int s_iter, s_ref, s_go;
    const SqItem& it = items[blockIdx.x];
    const bool in_lds = sq_in_lds(it, sh);
    const bool t0 = threadIdx.x == 0;

    // minCost = Cost(sensorPose), bestPose = sensorPose (:44-45)
    if (t0) {
        s_pose[0][0] = it.sx;
        s_pose[0][1] = it.sy;
        s_pose[0][2] = it.st;
    }
    __syncthreads();
    sq_costs(it, s_pose, 1, s_cost, l_rows, in_lds, err);
    if (t0) {
        s_min = s_cost[0];
        s_best[0] = it.sx;
        s_best[1] = it.sy;
        s_best[2] = it.st;
        s_lin = sh.lin_step;
        s_ang = sh.ang_step;
        s_iter = 0;
        s_ref = 0;
        sq_neighbours(s_pose, s_best, s_lin, s_ang);
    }
    __syncthreads();
    const int pass_cap = max(sh.max_iterations, 1);   // the do/while cannot run more passes
    int passes = 0;
    for (int pass = 0; pass < pass_cap; ++pass) {
        sq_costs(it, s_pose, 6, s_cost, l_rows, in_lds, err);
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
            if (go) sq_neighbours(s_pose, s_best, s_lin, s_ang);
        }
        __syncthreads();
        ++passes;
        if (!s_go) break;
    }
    // ComputeCovariance(bestPose) (:112-135): the gradient sums
    if (t0) {
        s_pose[0][0] = s_best[0];
        s_pose[0][1] = s_best[1];
        s_pose[0][2] = s_best[2];
    }
    __syncthreads();
    sq_cost_grad(it, s_pose, s_cost, l_rows, in_lds, err);
    if (t0) {
        SqRecord r;
        r.min_cost = s_min;
        for (int k = 0; k < 3; ++k) r.grad[k] = s_cost[1 + k];
        for (int j = 0; j < 3; ++j) r.best[j] = s_best[j];
        r.lin_step = s_lin;
        r.ang_step = s_ang;
        r.num_iterations = s_iter;
        r.num_refinements = s_ref;
        r.passes = passes;
        r.cost_evals = 1 + 6 * passes;   // the analytic gradient calls Cost not once
        recs[blockIdx.x] = r;
#ifdef LGS_PROBE
        if (blockIdx.x == 0) {
            printf("probe k_hc_sq: %d passes, N %d: terms %.2f chains %.2f us\n", passes, it.p.N,
                   0.01 * (double)g_sq_probe[0], 0.01 * (double)g_sq_probe[1]);
            g_sq_probe[0] = g_sq_probe[1] = 0ull;
        }
#endif
    }
}

// Cost (sh.nrows == 1) or Cost and the gradient sums (sh.nrows == 4) of item
// blockIdx.x at its sensor pose
__global__ __launch_bounds__(kSqThreads) void k_sq_cost_batch(const SqItem* __restrict__ items, SqShared sh,
                                                              SqRecord* __restrict__ recs, int* __restrict__ err)
{
    extern __shared__ double l_rows[];
    __shared__ double s_pose[kSqPoses][3];
    __shared__ double s_cost[kSqPoses];
    const SqItem& it = items[blockIdx.x];
    const bool in_lds = sq_in_lds(it, sh);
    if (threadIdx.x == 0) {
        s_pose[0][0] = it.sx;
        s_pose[0][1] = it.sy;
        s_pose[0][2] = it.st;
        s_cost[1] = s_cost[2] = s_cost[3] = 0.0;
    }
    __syncthreads();
    if (sh.nrows == kSqGradRows)
        sq_cost_grad(it, s_pose, s_cost, l_rows, in_lds, err);
    else
        sq_costs(it, s_pose, 1, s_cost, l_rows, in_lds, err);
    if (threadIdx.x == 0) {
        SqRecord r = {};
        r.min_cost = s_cost[0];
        for (int k = 0; k < 3; ++k) r.grad[k] = s_cost[1 + k];
        r.best[0] = it.sx;
        r.best[1] = it.sy;
        r.best[2] = it.st;
        recs[blockIdx.x] = r;
    }
}

// ------------------------------------------------------------------ host
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

bool pose_finite(const lgs_pose2d& p) { return std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.theta); }

void check_sq_cost(const lgs_cost_sq_params* c)
{
    LGS_REQUIRE(c && std::isfinite(c->usable_range_min) && std::isfinite(c->usable_range_max),
                "square-error cost: usable ranges must be finite");
}

void check_hc(const lgs_hc_params* p)
{
    LGS_REQUIRE(p, "null argument");
    LGS_REQUIRE(std::isfinite(p->linear_step) && p->linear_step > 0.0 && std::isfinite(p->angular_step) &&
                    p->angular_step > 0.0,
                "hill climbing: steps must be finite and > 0");
    LGS_REQUIRE(p->max_iterations <= kSqMaxIter, "hill climbing: more than 65536 iterations");
}

SqItem sq_item(const lgs_grid* g, const lgs_cost_sq_params* cost, const lgs_scan* s, lgs_pose2d sensor)
{
    SqItem it;
    std::memset(&it, 0, sizeof(it));
    it.p.min_x = g->min_x;
    it.p.min_y = g->min_y;
    it.p.res = g->res;
    it.p.W = g->w;
    it.p.H = g->h;
    it.p.N = s->n;
    it.p.cost_min = std::max(cost->usable_range_min, s->min_range);   // :27-30
    it.p.cost_max = std::min(cost->usable_range_max, s->max_range);
    it.sx = sensor.x;
    it.sy = sensor.y;
    it.st = sensor.theta;
    it.map = g->d;
    it.ranges = s->d_ranges;
    it.angles = s->d_angles;
    return it;
}

// n items: grids[j], scans[j] at sensor[j].  With p the walk (k_hc_sq), else
// the cost (and, with want_grad, the gradient sums) at sensor[j]
// (k_sq_cost_batch).  A square-error term needs no table, so the items of a
// launch may mix maps of any size and resolution: chunks are runs of at most
// 4096 items in order, all launched before the one synchronisation.  Trace
// (n == 1 only): the per-pass (move, minCost).
void run_sq(lgs_ctx* ctx, const lgs_hc_params* p, bool want_grad, const lgs_cost_sq_params* cost,
            const lgs_grid* const* grids, const lgs_scan* const* scans, const lgs_pose2d* sensor, int n,
            SqRecord* recs, int* trace_moves = nullptr, double* trace_costs = nullptr, int trace_cap = 0)
{
    check_sq_cost(cost);
    for (int j = 0; j < n; ++j) {
        LGS_REQUIRE(grids[j] && grids[j]->d && grids[j]->w >= 1 && grids[j]->h >= 1 && scans[j] && scans[j]->n >= 1,
                    "square-error cost: null or empty map, or empty scan");
        LGS_REQUIRE(std::isfinite(grids[j]->res) && grids[j]->res > 0.0,
                    "square-error cost: map resolution finite and > 0");
        LGS_REQUIRE(pose_finite(sensor[j]), "square-error cost: pose not finite");
        LGS_REQUIRE((long long)grids[j]->w * grids[j]->h < (1LL << 30), "square-error cost: map of 2^30 cells or more");
    }
    if (n == 0) return;
    for (int k = 0; k < n; ++k) grid_acquire(ctx, grids[k]);
    LGS_HIP_CHECK(hipSetDevice(ctx->device));
    const int nrows = p ? kSqPoses : (want_grad ? kSqGradRows : 1);
    const int pass_cap = p ? std::max(p->max_iterations, 1) : 1;
    const auto rows_bytes = [&](int j) { return sizeof(double) * (size_t)nrows * (size_t)scans[j]->n; };

    // the chunks: [begin, end), the LDS and the global rows of each
    struct Chunk { int j0, j1; size_t lds, rows; };
    std::vector<Chunk> chunks;
    size_t rows_max = 0;
    for (int j = 0; j < n;) {
        Chunk c{ j, j, 0, 0 };
        for (; c.j1 < n && c.j1 - c.j0 < kSqChunk; ++c.j1) {
            const size_t rb = rows_bytes(c.j1);
            if (rb > kSqLdsMax) {
                if (c.j1 > c.j0 && c.rows + align256(rb) > kSqRowsCap) break;
                c.rows += align256(rb);
            } else
                c.lds = std::max(c.lds, rb);
        }
        rows_max = std::max(rows_max, c.rows);
        chunks.push_back(c);
        j = c.j1;
    }
    scans_to_device(ctx, scans, n);
    // the chunks run one after another on the stream, so they share the rows
    char* rows = rows_max ? (char*)ctx->ensure(S_HC0, rows_max) : nullptr;
    const size_t rb = align256(sizeof(SqRecord) * (size_t)n);
    const size_t tmb = trace_moves ? align256(sizeof(int) * (size_t)pass_cap) : 0;
    const size_t tcb = trace_moves ? align256(sizeof(double) * (size_t)pass_cap) : 0;
    const size_t hb = rb + tmb + tcb + 256;
    char* small = (char*)ctx->ensure(S_HC1, hb);
    SqRecord* d_rec = (SqRecord*)small;
    int* d_tm = trace_moves ? (int*)(small + rb) : nullptr;
    double* d_tc = trace_moves ? (double*)(small + rb + tmb) : nullptr;
    int* d_err = (int*)(small + rb + tmb + tcb);
    LGS_HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream));

    std::vector<SqItem> items((size_t)n);
    for (const Chunk& c : chunks) {
        size_t roff = 0;
        for (int j = c.j0; j < c.j1; ++j) {
            SqItem& it = items[(size_t)j];
            it = sq_item(grids[j], cost, scans[j], sensor[j]);
            const size_t b = rows_bytes(j);
            if (b > kSqLdsMax) {
                it.rows = (double*)(rows + roff);
                roff += align256(b);
            }
            it.trace_move = d_tm;
            it.trace_cost = d_tc;
        }
    }
    Upload up(ctx);
    const size_t io = up.append(items.data(), items.size());
    up.flush();
    SqShared sh;
    std::memset(&sh, 0, sizeof(sh));
    if (p) {
        sh.lin_step = p->linear_step;
        sh.ang_step = p->angular_step;
        sh.max_iterations = p->max_iterations;
        sh.max_refinements = p->max_num_of_refinements;
    }
    sh.trace_cap = trace_moves ? pass_cap : 0;
    sh.nrows = nrows;
    for (const Chunk& c : chunks) {
        sh.lds_bytes = (unsigned)c.lds;
        const SqItem* d_items = up.at<SqItem>(io) + c.j0;
        if (p) {
            sq_allow_lds(k_hc_sq, c.lds);
            hipLaunchKernelGGL(k_hc_sq, dim3(c.j1 - c.j0), dim3(kSqThreads), c.lds, ctx->stream, d_items, sh,
                               d_rec + c.j0, d_err);
        } else {
            sq_allow_lds(k_sq_cost_batch, c.lds);
            hipLaunchKernelGGL(k_sq_cost_batch, dim3(c.j1 - c.j0), dim3(kSqThreads), c.lds, ctx->stream, d_items, sh,
                               d_rec + c.j0, d_err);
        }
        LGS_HIP_CHECK(hipGetLastError());
    }
    char* pin = (char*)ctx->ensure_pinned(hb);
    LGS_HIP_CHECK(hipMemcpyAsync(pin, small, hb, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    if (*(const int*)(pin + rb + tmb + tcb) != 0)
        throw Error(LGS_ERR_INTERNAL, "square-error cost: an angle lies outside the restated sincos domain");
    std::memcpy(recs, pin, sizeof(SqRecord) * (size_t)n);
    if (trace_moves) {
        const int np = std::min(recs[0].passes, trace_cap);
        std::memcpy(trace_moves, pin + rb, sizeof(int) * (size_t)np);
        std::memcpy(trace_costs, pin + rb + tmb, sizeof(double) * (size_t)np);
    }
}

void run_hc_sq(lgs_ctx* ctx, const lgs_hc_params* p, const lgs_cost_sq_params* cost, const lgs_grid* const* grids,
               const lgs_scan* const* scans, const lgs_pose2d* init, int n, lgs_hc_summary* out,
               int* trace_moves = nullptr, double* trace_costs = nullptr, int trace_cap = 0)
{
    for (int j = 0; j < n; ++j) {
        LGS_REQUIRE(grids[j] && scans[j], "hill climbing: null map or scan");
        LGS_REQUIRE(pose_finite(init[j]), "hill climbing: initial pose not finite");
    }
    std::vector<SqRecord> recs((size_t)n);
    std::vector<lgs_pose2d> sensor((size_t)n);
    for (int j = 0; j < n; ++j) sensor[(size_t)j] = compound(init[j], scans[j]->rel);   // :40-41
    run_sq(ctx, p, true, cost, grids, scans, sensor.data(), n, recs.data(), trace_moves, trace_costs, trace_cap);
    for (int j = 0; j < n; ++j) {
        const SqRecord& r = recs[(size_t)j];
        lgs_hc_summary& o = out[j];
        std::memset(&o, 0, sizeof(o));
        const lgs_pose2d best{ r.best[0], r.best[1], r.best[2] };
        o.pose_found = 1;                                          // :106-108
        o.normalized_cost = r.min_cost / (double)scans[j]->n;      // :96
        o.initial_pose = init[j];
        o.estimated_pose = move_backward(best, scans[j]->rel);     // :98-99
        sq_covariance(r.grad, o.covariance);
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

namespace lgs {
// What the branch-and-bound and grid-search matchers derive from their cost
// function after the search (scan_matcher_branch_bound.cpp:146-153,
// scan_matcher_grid_search.cpp:97-107) when that function is CostSquareError:
// normalized cost, estimated pose and covariance at best[j], one
// k_sq_cost_batch launch over all n items (their maps may differ).
void cost_summaries_sq(lgs_ctx* ctx, const lgs_grid* const* grids, const lgs_cost_sq_params* cost,
                       lgs_scan* const* scans, const lgs_pose2d* best, int n, lgs_rtcsm_summary* out)
{
    if (n <= 0) return;
    std::vector<SqRecord> recs((size_t)n);
    run_sq(ctx, nullptr, true, cost, grids, scans, best, n, recs.data());
    for (int j = 0; j < n; ++j) {
        out[j].normalized_cost = recs[(size_t)j].min_cost / (double)scans[j]->n;
        out[j].estimated_pose = move_backward(best[j], scans[j]->rel);
        sq_covariance(recs[(size_t)j].grad, out[j].covariance);
    }
}
}  // namespace lgs

extern "C" int lgs_cost_square_error_batch(lgs_ctx* ctx, const lgs_grid* const* grids, const lgs_cost_sq_params* cost,
                                           const lgs_scan* const* scans, const lgs_pose2d* sensor_poses, int n,
                                           double* out_cost, double* out_covariance)
{
    if (!ctx || !cost || n < 0 || (n > 0 && (!grids || !scans || !sensor_poses || !out_cost)))
        return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        std::vector<SqRecord> recs((size_t)n);
        run_sq(ctx, nullptr, out_covariance != nullptr, cost, grids, scans, sensor_poses, n, recs.data());
        for (int j = 0; j < n; ++j) {
            out_cost[j] = recs[(size_t)j].min_cost;
            if (out_covariance) sq_covariance(recs[(size_t)j].grad, out_covariance + 9 * (size_t)j);
        }
    });
}

extern "C" int lgs_summaries_apply_cost_sq(lgs_ctx* ctx, const lgs_grid* const* grids, const lgs_cost_sq_params* cost,
                                           const lgs_scan* const* scans, lgs_rtcsm_summary* summaries, int n)
{
    if (!ctx || !cost || n < 0 || (n > 0 && (!grids || !scans || !summaries))) return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        std::vector<SqRecord> recs((size_t)n);
        std::vector<lgs_pose2d> poses((size_t)n);
        for (int j = 0; j < n; ++j) poses[(size_t)j] = summaries[j].best_sensor_pose;
        run_sq(ctx, nullptr, true, cost, grids, scans, poses.data(), n, recs.data());
        for (int j = 0; j < n; ++j) {
            summaries[j].normalized_cost = recs[(size_t)j].min_cost / (double)scans[j]->n;
            sq_covariance(recs[(size_t)j].grad, summaries[j].covariance);
        }
    });
}

extern "C" int lgs_hc_sq_optimize_pose_batch(lgs_ctx* ctx, const lgs_grid* const* grids, const lgs_hc_params* params,
                                             const lgs_cost_sq_params* cost, const lgs_scan* const* scans,
                                             const lgs_pose2d* initial, int n, lgs_hc_summary* out)
{
    if (!ctx || !params || !cost || n < 0 || (n > 0 && (!grids || !scans || !initial || !out)))
        return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        check_hc(params);
        check_sq_cost(cost);
        if (n == 0) return;
        run_hc_sq(ctx, params, cost, grids, scans, initial, n, out);
    });
}

extern "C" int lgs_hc_sq_optimize_pose_query(lgs_ctx* ctx, const lgs_grid* grid, const lgs_hc_params* params,
                                             const lgs_cost_sq_params* cost, const lgs_scan* scan, lgs_pose2d initial,
                                             lgs_hc_summary* out)
{
    if (!grid || !scan || !out) return LGS_ERR_INVALID_ARG;
    return lgs_hc_sq_optimize_pose_batch(ctx, &grid, params, cost, &scan, &initial, 1, out);
}

extern "C" int lgs_hc_sq_trace(lgs_ctx* ctx, const lgs_grid* grid, const lgs_hc_params* params,
                               const lgs_cost_sq_params* cost, const lgs_scan* scan, lgs_pose2d initial, int* moves,
                               double* costs, int cap)
{
    if (!ctx || !grid || !params || !cost || !scan || cap < 0 || (cap > 0 && (!moves || !costs)))
        return -LGS_ERR_INVALID_ARG;
    int passes = 0;
    const int rc = guarded(ctx, [&] {
        check_hc(params);
        lgs_hc_summary sum;
        const int pass_cap = std::max(params->max_iterations, 1);
        std::vector<int> mv((size_t)pass_cap);
        std::vector<double> cs((size_t)pass_cap);
        run_hc_sq(ctx, params, cost, &grid, &scan, &initial, 1, &sum, mv.data(), cs.data(), pass_cap);
        passes = sum.passes;
        for (int k = 0; k < passes && k < cap; ++k) {
            moves[k] = mv[(size_t)k];
            costs[k] = cs[(size_t)k];
        }
    });
    return rc == LGS_OK ? passes : -rc;
}
