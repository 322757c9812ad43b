// k_gs.hip -- exhaustive grid-search matcher and loop detector on MI355X.
//
// Restates ScanMatcherGridSearch::OptimizePose
// (C/mapping/scan_matcher_grid_search.cpp:31-114) with ScorePixelAccurate
// (C/mapping/score_function_pixel_accurate.cpp:19-77) and
// LoopDetectorGridSearch::Detect (C/mapping/loop_detector_grid_search.cpp:26-106).
//
// The reference scores every pose (sp.x + dx, sp.y + dy, sp.theta + dt) of a
// window whose offsets come from `for (double d = -r; d <= r; d += s)` loops
// (dy outer, dx middle, dt inner) and keeps the first pose, in that order,
// of the maximum score, if that maximum is > the threshold.  Here
// (DESIGN.md §4.6b):
//
//   lgs_gs_steps  the literal loop on the host: the three offset lists are
//                 what the floating-point accumulation produces
//   k_gs_trig     r cos(theta_t + a_v), r sin(theta_t + a_v) once per (angle,
//                 valid beam) with glibc's sincos restated (glm::gl_sincos);
//                 valid beams (ScorePixelAccurate's strict range filter)
//                 compacted in beam order on the host
//   k_gs_index    the hit cell is separable: its x index depends on (theta,
//                 dx, beam) only, its y index on (theta, dy, beam) only.  Each
//                 is formed once with the reference's arithmetic
//                 floor(((s + d) + r cos) - min) / res) (IEEE division) into
//                 xi[t][v][ix] and the row offset yo[t][iy][v] = y * W;
//                 outside the map either is kOut = -2^30, so xi + yo < 0 is the
//                 one test of the inner loop
//   k_gs_score    lanes along dx, kGSRows dy rows per wave, waves and
//                 workgroups over dy and theta; one fp64 accumulator per
//                 pose, beams strictly in order; workgroup partials of
//                 (score, order index)
//   k_gs_argmax   one workgroup per match: the maximum of the partials, ties
//                 to the lowest (iy, ix, it) order, then the threshold
//
// The greedy-endpoint cost and covariance at the best pose come from k_cost
// (k_rtcsm.hip cost_summaries), the summary's pose algebra from host glibc.
#include "lgs_internal.hpp"
#include "loop_host.hpp"
#include "glibc_math.hpp"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>

using namespace lgs;

namespace lgs {
void cost_summaries(lgs_ctx* ctx, const lgs_grid* grid, const lgs_cost_ge_params* cost, lgs_scan* const* scans,
                    const lgs_pose2d* best, int n, lgs_rtcsm_summary* out);
}  // namespace lgs

namespace {

// documented caps (include/lgs_hip.h)
constexpr int kGSMaxAxis = 4096;                    // window values per axis
constexpr long long kGSMaxPoses = 1LL << 24;        // poses per match
constexpr size_t kGSItemCap = size_t(2) << 30;      // tables of one match
constexpr size_t kGSChunkCap = size_t(1) << 30;     // tables of the matches in flight together

constexpr int kGSRows = 4;     // dy rows per wave (accumulators per lane)
constexpr int kGSWaves = 4;    // waves per workgroup
constexpr int kGSUnroll = 4;   // beams per pipelined step; Nvp is a multiple
constexpr int kOut = -(1 << 30);

// One match of a batched grid-search launch (device memory).
struct GSItem {
    double sx, sy, st;          // sensor pose (Compound(initialPose, relPose))
    double min_x, min_y, res;   // map geometry
    double thr;                 // normalizedScoreThreshold * NumOfScans()
    int W, H;
    int Nv, Nvp;                // valid beams, padded to kGSUnroll
    const double* map;
    const double* ranges;
    const double* angles;
    const int* vidx;            // valid beams in beam order
    double* rc;                 // [nt][Nvp] r cos(theta_t + a_v)
    double* rs;                 // [nt][Nvp] r sin(theta_t + a_v)
    int* xi;                    // [nt][Nvp][nx] x cell or kOut
    int* yo;                    // [nt][ny][Nvp] y cell * W or kOut
};

// The window of a call: the three offset lists (device) and their counts.
struct GSWin {
    const double* dx;
    const double* dy;
    const double* dt;
    int nx, ny, nt;
};

struct GSResult {
    double score;   // the maximum score, or the threshold when nothing exceeds it
    int ord;        // (iy * nx + ix) * nt + it of the best pose, -1: not found
    int found;
};

__global__ __launch_bounds__(256) void k_gs_trig(const GSItem* __restrict__ items, GSWin w, int* __restrict__ err)
{
    const GSItem& it = items[blockIdx.z];
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const int t = blockIdx.y;
    if (v >= it.Nvp) return;
    double c = 0.0, s = 0.0;
    if (v < it.Nv) {
        const int i = it.vidx[v];
        // pose.mTheta = sensorPose.mTheta + dt (:78-80); HitPoint's
        // cos/sin(sensorPose.mTheta + scanAngle) is one glibc sincos
        const double th = (it.st + w.dt[t]) + it.angles[i];
        if (!glm::gl_sincos_ok(th)) *err = 1;
        double sn, cs;
        glm::gl_sincos(th, &sn, &cs);
        const double r = it.ranges[i];
        c = r * cs;
        s = r * sn;
    }
    it.rc[(size_t)t * it.Nvp + v] = c;
    it.rs[(size_t)t * it.Nvp + v] = s;
}

// WorldCoordinateToGridCellIndex (H/grid_map/grid_map.hpp:779-790) of one
// coordinate: floor of the IEEE quotient, negative quotients to negative cells
__device__ __forceinline__ int gs_cell(double hit, double mn, double res, int n)
{
    const double f = floor((hit - mn) / res);
    return (f >= 0.0 && f < (double)n) ? (int)f : -1;
}

__global__ __launch_bounds__(256) void k_gs_index(const GSItem* __restrict__ items, GSWin w)
{
    const GSItem& it = items[blockIdx.z];
    const int t = blockIdx.y;
    const int Nvp = it.Nvp;
    const long long ex = (long long)Nvp * w.nx, ey = (long long)Nvp * w.ny;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < ex) {   // xi[t][v][ix], ix fastest
        const int v = (int)(e / w.nx), ix = (int)(e % w.nx);
        int cell = kOut;
        if (v < it.Nv) {
            const double px = it.sx + w.dx[ix];   // pose.mX (:78)
            const int c = gs_cell(px + it.rc[(size_t)t * Nvp + v], it.min_x, it.res, it.W);
            if (c >= 0) cell = c;
        }
        it.xi[(size_t)t * Nvp * w.nx + e] = cell;
    } else if (e < ex + ey) {   // yo[t][iy][v], v fastest
        const long long k = e - ex;
        const int iy = (int)(k / Nvp), v = (int)(k % Nvp);
        int off = kOut;
        if (v < it.Nv) {
            const double py = it.sy + w.dy[iy];   // pose.mY (:79)
            const int c = gs_cell(py + it.rs[(size_t)t * Nvp + v], it.min_y, it.res, it.H);
            if (c >= 0) off = c * it.W;
        }
        it.yo[(size_t)t * Nvp * w.ny + k] = off;
    }
}

// the better of two (score, order) candidates: the higher score, on a tie the
// lower order -- the pose the reference's strict `>` update would keep
__device__ __forceinline__ void gs_better(double& s, int& o, double s2, int o2)
{
    if (s2 > s || (s2 == s && o2 < o)) {
        s = s2;
        o = o2;
    }
}

// grid: x = x tiles of 64 * y blocks of kGSWaves * kGSRows rows, y = angle,
// z = match.  parts[z][y * gridDim.x + x] receives the workgroup's best.
__global__ __launch_bounds__(64 * kGSWaves) void k_gs_score(const GSItem* __restrict__ items, GSWin w, int nxt,
                                                            double* __restrict__ part_s, int* __restrict__ part_o,
                                                            double* __restrict__ dense)
{
    __shared__ double s_s[kGSWaves];
    __shared__ int s_o[kGSWaves];
    const GSItem& it = items[blockIdx.z];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.y;
    const int bx = blockIdx.x % nxt, by = blockIdx.x / nxt;
    const int ix = bx * 64 + lane;
    const int iy0 = (by * kGSWaves + wave) * kGSRows;
    const int nx = w.nx, ny = w.ny, Nvp = it.Nvp;
    const double* __restrict__ map = it.map;
    const int* __restrict__ xcol = it.xi + (size_t)t * Nvp * nx + min(ix, nx - 1);
    const int* __restrict__ yrow[kGSRows];
#pragma unroll
    for (int k = 0; k < kGSRows; ++k) yrow[k] = it.yo + ((size_t)t * ny + min(iy0 + k, ny - 1)) * Nvp;
    double acc[kGSRows];
#pragma unroll
    for (int k = 0; k < kGSRows; ++k) acc[k] = 0.0;
    if (iy0 < ny) {
        for (int v0 = 0; v0 < Nvp; v0 += kGSUnroll) {
            int x[kGSUnroll];
            double val[kGSUnroll][kGSRows];
#pragma unroll
            for (int j = 0; j < kGSUnroll; ++j) x[j] = gload(xcol + (size_t)(v0 + j) * nx);
#pragma unroll
            for (int j = 0; j < kGSUnroll; ++j)
#pragma unroll
                for (int k = 0; k < kGSRows; ++k) {
                    // GridMap::Value(idx, unknown): outside the map reads
                    // unknown (0.0), which the reference skips (:55-56);
                    // adding 0.0 is the same
                    const int off = x[j] + gload(yrow[k] + v0 + j);
                    const double m = gload(map + max(off, 0));
                    val[j][k] = off >= 0 ? m : 0.0;
                }
#pragma unroll
            for (int j = 0; j < kGSUnroll; ++j)   // beam order per accumulator
#pragma unroll
                for (int k = 0; k < kGSRows; ++k) acc[k] += val[j][k];
        }
    }
    double bs = -INFINITY;
    int bo = INT_MAX;
#pragma unroll
    for (int k = 0; k < kGSRows; ++k) {
        if (ix < nx && iy0 + k < ny) {
            const int ord = ((iy0 + k) * nx + ix) * w.nt + t;
            if (dense) dense[ord] = acc[k];
            gs_better(bs, bo, acc[k], ord);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double s2 = __shfl_xor(bs, d, 64);
        const int o2 = __shfl_xor(bo, d, 64);
        gs_better(bs, bo, s2, o2);
    }
    if (lane == 0) {
        s_s[wave] = bs;
        s_o[wave] = bo;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < kGSWaves; ++k) gs_better(bs, bo, s_s[k], s_o[k]);
        const size_t p = (size_t)blockIdx.z * gridDim.x * gridDim.y + (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        part_s[p] = bs;
        part_o[p] = bo;
    }
}

// scoreMax starts at the threshold and moves on strict `>` (:70, :86-89):
// found iff the maximum is > the threshold (:95-97)
__global__ __launch_bounds__(256) void k_gs_argmax(const GSItem* __restrict__ items, const double* __restrict__ part_s,
                                                   const int* __restrict__ part_o, int nparts,
                                                   GSResult* __restrict__ out)
{
    __shared__ double s_s[4];
    __shared__ int s_o[4];
    const int j = blockIdx.x;
    double bs = -INFINITY;
    int bo = INT_MAX;
    for (int p = threadIdx.x; p < nparts; p += blockDim.x)
        gs_better(bs, bo, part_s[(size_t)j * nparts + p], part_o[(size_t)j * nparts + p]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double s2 = __shfl_xor(bs, d, 64);
        const int o2 = __shfl_xor(bo, d, 64);
        gs_better(bs, bo, s2, o2);
    }
    if ((threadIdx.x & 63) == 0) {
        s_s[threadIdx.x >> 6] = bs;
        s_o[threadIdx.x >> 6] = bo;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) gs_better(bs, bo, s_s[k], s_o[k]);
        const double thr = items[j].thr;
        GSResult r;
        r.found = bs > thr ? 1 : 0;
        r.score = r.found ? bs : thr;
        r.ord = r.found ? bo : -1;
        out[j] = r;
    }
}

// ------------------------------------------------------------------ host
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

bool gs_axis_ok(double range, double step)
{
    return std::isfinite(step) && step > 0.0 && std::isfinite(range) && range >= 0.0;
}

// the literal loop (:72-74); false when it passes kGSMaxAxis values (which
// also ends a loop whose `d += step` no longer moves d)
bool gs_axis(double range, double step, std::vector<double>& out)
{
    out.clear();
    const double r = range / 2.0;
    for (double d = -r; d <= r; d += step) {
        if ((int)out.size() == kGSMaxAxis) return false;
        out.push_back(d);
    }
    return true;
}

struct GSWindow {
    std::vector<double> dx, dy, dt;
    long long poses() const { return (long long)dx.size() * (long long)dy.size() * (long long)dt.size(); }
};

void check_gs(const lgs_gs_params* p, const lgs_cost_ge_params* c, GSWindow& win)
{
    LGS_REQUIRE(p, "null argument");
    LGS_REQUIRE(!c || c->kernel_size >= 0, "negative kernel size");
    LGS_REQUIRE(gs_axis_ok(p->range_x, p->step_x) && gs_axis_ok(p->range_y, p->step_y) &&
                    gs_axis_ok(p->range_theta, p->step_theta),
                "grid search: steps must be finite and > 0, ranges finite and >= 0");
    LGS_REQUIRE(gs_axis(p->range_x, p->step_x, win.dx) && gs_axis(p->range_y, p->step_y, win.dy) &&
                    gs_axis(p->range_theta, p->step_theta, win.dt),
                "grid search: more than 4096 window values on one axis");
    LGS_REQUIRE(win.poses() <= kGSMaxPoses, "grid search: more than 2^24 poses in the window");
}

struct GSHost {   // host plan of one match
    lgs_pose2d sensor;
    double thr;
    std::vector<int> vidx;
    int Nv, Nvp;
    size_t bytes;   // its tables
};

size_t gs_item_bytes(const GSWindow& w, int Nvp)
{
    const size_t nt = w.dt.size(), nx = w.dx.size(), ny = w.dy.size(), nv = (size_t)std::max(Nvp, 1);
    return 2 * align256(sizeof(double) * nt * nv) + align256(sizeof(int) * nt * nv * std::max<size_t>(nx, 1)) +
           align256(sizeof(int) * nt * nv * std::max<size_t>(ny, 1));
}

// n matches of one window: grids[j], scans[j], init[j].  dense (n == 1 only):
// every pose's score in (iy, ix, it) order; no summaries then (cost == null).
void run_gs(lgs_ctx* ctx, const lgs_gs_params* p, const lgs_cost_ge_params* cost, const GSWindow& win,
            const lgs_grid* const* grids, lgs_scan* const* scans, const lgs_pose2d* init, int n, double nthr,
            lgs_rtcsm_summary* out, double* dense_host = nullptr, CostAlt alt = {})
{
    const int nx = (int)win.dx.size(), ny = (int)win.dy.size(), nt = (int)win.dt.size();
    const long long poses = win.poses();
    std::vector<GSHost> plans((size_t)n);
    for (int j = 0; j < n; ++j) {
        GSHost& b = plans[(size_t)j];
        const lgs_scan* s = scans[j];
        LGS_REQUIRE((long long)grids[j]->w * grids[j]->h < (1LL << 30), "grid search: map of 2^30 cells or more");
        b.sensor = compound(init[j], s->rel);           // :52-53
        b.thr = nthr * (double)s->n;                    // :66-68
        // ScorePixelAccurate's beam filter (:27-41), both tests strict
        const double minRange = std::max(p->score_usable_range_min, s->min_range);
        const double maxRange = std::min(p->score_usable_range_max, s->max_range);
        for (int i = 0; i < s->n; ++i) {
            const double r = s->h_ranges[(size_t)i];
            if (r >= maxRange || r <= minRange) continue;
            b.vidx.push_back(i);
        }
        b.Nv = (int)b.vidx.size();
        b.Nvp = (b.Nv + kGSUnroll - 1) / kGSUnroll * kGSUnroll;
        b.bytes = gs_item_bytes(win, b.Nvp);
        LGS_REQUIRE(b.bytes <= kGSItemCap, "grid search: window x beams beyond the 2 GiB table cap");
    }
    for (int k = 0; k < n; ++k) grid_acquire(ctx, grids[k]);
    LGS_HIP_CHECK(hipSetDevice(ctx->device));
    if (out) std::memset(out, 0, sizeof(lgs_rtcsm_summary) * (size_t)n);
    std::vector<GSResult> res((size_t)n);
    for (int j = 0; j < n; ++j) res[(size_t)j] = GSResult{ plans[(size_t)j].thr, -1, 0 };

    // chunks of matches whose tables fit kGSChunkCap together (at least one)
    const int nxt = (nx + 63) / 64, nyb = (ny + kGSWaves * kGSRows - 1) / (kGSWaves * kGSRows);
    const int nparts = nxt * nyb * nt;
    for (int j0 = 0; j0 < n && poses > 0;) {
        int j1 = j0;
        size_t total = 0;
        while (j1 < n && (j1 == j0 || total + plans[(size_t)j1].bytes <= kGSChunkCap)) total += plans[(size_t)j1++].bytes;
        const int m = j1 - j0;
        scans_to_device(ctx, scans + j0, m);
        char* ws = (char*)ctx->ensure(S_GS0, total);
        const size_t pb = align256(sizeof(double) * (size_t)nparts * m), ob = align256(sizeof(int) * (size_t)nparts * m);
        const size_t rb = align256(sizeof(GSResult) * (size_t)m);
        char* small = (char*)ctx->ensure(S_GS1, pb + ob + rb + 256);
        double* d_ps = (double*)small;
        int* d_po = (int*)(small + pb);
        GSResult* d_res = (GSResult*)(small + pb + ob);
        int* d_err = (int*)(small + pb + ob + rb);
        LGS_HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream));

        std::vector<GSItem> items((size_t)m);
        std::vector<int> h_vidx;
        size_t off = 0;
        int NvpMax = 0;
        double lookups = 0.0;
        auto take = [&](size_t bytes) {
            char* q = ws + off;
            off += align256(bytes);
            return q;
        };
        std::vector<size_t> voff((size_t)m);
        for (int k = 0; k < m; ++k) {
            const GSHost& b = plans[(size_t)(j0 + k)];
            const lgs_grid* g = grids[j0 + k];
            GSItem& it = items[(size_t)k];
            std::memset(&it, 0, sizeof(it));
            it.sx = b.sensor.x;
            it.sy = b.sensor.y;
            it.st = b.sensor.theta;
            it.min_x = g->min_x;
            it.min_y = g->min_y;
            it.res = g->res;
            it.thr = b.thr;
            it.W = g->w;
            it.H = g->h;
            it.Nv = b.Nv;
            it.Nvp = b.Nvp;
            it.map = g->d;
            it.ranges = scans[j0 + k]->d_ranges;
            it.angles = scans[j0 + k]->d_angles;
            const size_t nv = (size_t)std::max(b.Nvp, 1);
            it.rc = (double*)take(sizeof(double) * nt * nv);
            it.rs = (double*)take(sizeof(double) * nt * nv);
            it.xi = (int*)take(sizeof(int) * nt * nv * (size_t)nx);
            it.yo = (int*)take(sizeof(int) * nt * nv * (size_t)ny);
            voff[(size_t)k] = h_vidx.size();
            h_vidx.insert(h_vidx.end(), b.vidx.begin(), b.vidx.end());
            NvpMax = std::max(NvpMax, b.Nvp);
            lookups += (double)b.Nv * (double)poses;
        }
        if (h_vidx.empty()) h_vidx.push_back(0);
        Upload up(ctx);
        const size_t xo = up.append(win.dx.data(), win.dx.size());
        const size_t yo = up.append(win.dy.data(), win.dy.size());
        const size_t to = up.append(win.dt.data(), win.dt.size());
        const size_t vo = up.append(h_vidx.data(), h_vidx.size());
        const size_t io = up.append(items.data(), items.size());
        char* dev = up.prepare();
        for (int k = 0; k < m; ++k) up.host_at<GSItem>(io)[k].vidx = (const int*)(dev + vo) + voff[(size_t)k];
        up.copy();
        const GSItem* d_items = up.at<GSItem>(io);
        GSWin w{ up.at<double>(xo), up.at<double>(yo), up.at<double>(to), nx, ny, nt };
        double* d_dense = nullptr;
        if (dense_host) d_dense = (double*)ctx->ensure(S_DENSE_FINE, sizeof(double) * (size_t)poses);
        if (NvpMax > 0) {
            hipLaunchKernelGGL(k_gs_trig, dim3((NvpMax + 255) / 256, nt, m), dim3(256), 0, ctx->stream, d_items, w,
                               d_err);
            LGS_HIP_CHECK(hipGetLastError());
            const long long emax = (long long)NvpMax * (nx + ny);
            hipLaunchKernelGGL(k_gs_index, dim3((unsigned)((emax + 255) / 256), nt, m), dim3(256), 0, ctx->stream,
                               d_items, w);
            LGS_HIP_CHECK(hipGetLastError());
        }
        {
            // algorithmic bytes: 8 B per (pose, valid beam) map lookup
            const int tok = ctx->timing_begin(K_GS_SCORE, 8.0 * lookups);
            hipLaunchKernelGGL(k_gs_score, dim3(nxt * nyb, nt, m), dim3(64 * kGSWaves), 0, ctx->stream, d_items, w,
                               nxt, d_ps, d_po, d_dense);
            ctx->timing_end(tok);
            LGS_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_gs_argmax, dim3(m), dim3(256), 0, ctx->stream, d_items, d_ps, d_po, nparts, d_res);
        LGS_HIP_CHECK(hipGetLastError());
        const size_t hb = align256(sizeof(GSResult) * (size_t)m);
        char* pin = (char*)ctx->ensure_pinned(hb + 256);
        LGS_HIP_CHECK(hipMemcpyAsync(pin, d_res, sizeof(GSResult) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        LGS_HIP_CHECK(hipMemcpyAsync(pin + hb, d_err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        if (ctx->profile) ctx->harvest();
        if (*(const int*)(pin + hb) != 0)
            throw Error(LGS_ERR_INTERNAL, "grid search: an angle lies outside the restated sincos domain");
        std::memcpy(res.data() + j0, pin, sizeof(GSResult) * (size_t)m);
        if (dense_host) LGS_HIP_CHECK(hipMemcpy(dense_host, d_dense, sizeof(double) * (size_t)poses, hipMemcpyDeviceToHost));
        j0 = j1;
    }
    if (!out) return;

    std::vector<lgs_pose2d> best((size_t)n);
    for (int j = 0; j < n; ++j) {
        const GSHost& b = plans[(size_t)j];
        const GSResult& r = res[(size_t)j];
        lgs_rtcsm_summary& o = out[j];
        int bx = -1, by = -1, bt = -1;
        lgs_pose2d bp = b.sensor;   // bestSensorPose stays sensorPose (:71)
        if (r.found) {
            bt = r.ord % nt;
            bx = (r.ord / nt) % nx;
            by = r.ord / nt / nx;
            bp = lgs_pose2d{ b.sensor.x + win.dx[(size_t)bx], b.sensor.y + win.dy[(size_t)by],
                             b.sensor.theta + win.dt[(size_t)bt] };   // :78-80
        }
        o.pose_found = r.found;
        o.initial_pose = init[j];
        o.score_max = r.score;
        o.score_threshold = b.thr;
        o.best_win[0] = bx;
        o.best_win[1] = by;
        o.best_win[2] = bt;
        o.win[0] = nx;
        o.win[1] = ny;
        o.win[2] = nt;
        o.steps[0] = p->step_x;
        o.steps[1] = p->step_y;
        o.steps[2] = p->step_theta;
        o.best_sensor_pose = bp;
        o.coarse_blocks = poses;
        o.fine_blocks = 0;
        best[(size_t)j] = bp;
    }
    if (alt) {
        // CostSquareError or the exact greedy-endpoint cost (:99-110): one launch over every
        // item, whatever its map
        if (alt.sq)
            cost_summaries_sq(ctx, grids, alt.sq, scans, best.data(), n, out);
        else
            cost_summaries_gx(ctx, grids, cost, scans, best.data(), n, out);
        return;
    }
    // cost and covariance at the best poses (:99-110), grouped by map
    std::vector<int> order((size_t)n);
    for (int j = 0; j < n; ++j) order[(size_t)j] = j;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return grids[a] < grids[b]; });
    for (size_t k0 = 0; k0 < order.size();) {
        size_t k1 = k0;
        while (k1 < order.size() && grids[order[k1]] == grids[order[k0]]) ++k1;
        std::vector<lgs_scan*> sc;
        std::vector<lgs_pose2d> bp;
        std::vector<lgs_rtcsm_summary> tmp;
        for (size_t k = k0; k < k1; ++k) {
            sc.push_back(scans[order[k]]);
            bp.push_back(best[(size_t)order[k]]);
            tmp.push_back(out[order[k]]);
        }
        cost_summaries(ctx, grids[order[k0]], cost, sc.data(), bp.data(), (int)sc.size(), tmp.data());
        for (size_t k = k0; k < k1; ++k) out[order[k]] = tmp[k - k0];
        k0 = k1;
    }
}

}  // namespace

extern "C" int lgs_gs_steps(double range, double step, double* out, int cap)
{
    if (!gs_axis_ok(range, step) || cap < 0 || (cap > 0 && !out)) return -LGS_ERR_INVALID_ARG;
    try {
        std::vector<double> v;
        if (!gs_axis(range, step, v)) return -LGS_ERR_INVALID_ARG;
        for (size_t k = 0; k < v.size() && k < (size_t)cap; ++k) out[k] = v[k];
        return (int)v.size();
    } catch (...) {
        return -LGS_ERR_OOM;
    }
}

// alt: the cost step is CostSquareError's (k_sq_cost_batch) or the exact greedy-endpoint one (k_ge_cost_batch)
static int gs_batch_run(lgs_ctx* ctx, const lgs_grid* grid, const lgs_gs_params* params,
                        const lgs_cost_ge_params* cost, CostAlt alt, const lgs_scan* const* scans,
                        const lgs_pose2d* initial, int n, double nthr, lgs_rtcsm_summary* out)
{
    if (!ctx || !grid || !params || !cost || n < 0 || (n > 0 && (!scans || !initial || !out)))
        return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        GSWindow win;
        check_gs(params, cost, win);
        if (n == 0) return;
        std::vector<const lgs_grid*> grids((size_t)n, grid);
        std::vector<lgs_scan*> sc((size_t)n);
        for (int j = 0; j < n; ++j) {
            LGS_REQUIRE(scans[j] && scans[j]->n >= 1, "empty scan");
            sc[(size_t)j] = const_cast<lgs_scan*>(scans[j]);
        }
        run_gs(ctx, params, cost, win, grids.data(), sc.data(), initial, n, nthr, out, nullptr, alt);
    });
}

extern "C" int lgs_gs_optimize_pose_batch(lgs_ctx* ctx, const lgs_grid* grid, const lgs_gs_params* params,
                                          const lgs_cost_ge_params* cost, const lgs_scan* const* scans,
                                          const lgs_pose2d* initial, int n, double nthr, lgs_rtcsm_summary* out)
{
    return gs_batch_run(ctx, grid, params, cost, CostAlt{}, scans, initial, n, nthr, out);
}

// With the square-error cost a failing call leaves `out` as it found it.
extern "C" int lgs_gs_optimize_pose_batch_cost(lgs_ctx* ctx, const lgs_grid* grid, const lgs_gs_params* params,
                                               const lgs_cost_spec* cost, const lgs_scan* const* scans,
                                               const lgs_pose2d* initial, int n, double nthr, lgs_rtcsm_summary* out)
{
    CostSel sel;
    if (const int rc = cost_select(cost, &sel)) return rc;
    if (!sel.alt) return lgs_gs_optimize_pose_batch(ctx, grid, params, sel.ge, scans, initial, n, nthr, out);
    if (n < 0 || (n > 0 && !out)) return LGS_ERR_INVALID_ARG;
    return with_own_output(ctx, out, n, [&](lgs_rtcsm_summary* o) {
        return gs_batch_run(ctx, grid, params, sel.ge, sel.alt, scans, initial, n, nthr, o);
    });
}

extern "C" int lgs_gs_optimize_pose_query_cost(lgs_ctx* ctx, const lgs_grid* grid, const lgs_gs_params* params,
                                               const lgs_cost_spec* cost, const lgs_scan* scan, lgs_pose2d initial,
                                               lgs_rtcsm_summary* out)
{
    if (!scan) return LGS_ERR_INVALID_ARG;
    return lgs_gs_optimize_pose_batch_cost(ctx, grid, params, cost, &scan, &initial, 1, DBL_MIN, out);
}

extern "C" int lgs_gs_optimize_pose_query(lgs_ctx* ctx, const lgs_grid* grid, const lgs_gs_params* params,
                                          const lgs_cost_ge_params* cost, const lgs_scan* scan, lgs_pose2d initial,
                                          lgs_rtcsm_summary* out)
{
    if (!scan) return LGS_ERR_INVALID_ARG;
    return lgs_gs_optimize_pose_batch(ctx, grid, params, cost, &scan, &initial, 1, DBL_MIN, out);   // :39-40
}

extern "C" int lgs_gs_dense_scores(lgs_ctx* ctx, const lgs_grid* grid, const lgs_gs_params* params,
                                   const lgs_scan* scan, lgs_pose2d initial, double* scores, long long cap)
{
    if (!ctx || !grid || !params || !scan || !scores || cap < 0) return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        GSWindow win;
        check_gs(params, nullptr, win);
        LGS_REQUIRE(scan->n >= 1, "empty scan");
        LGS_REQUIRE(win.poses() <= cap, "grid search: score buffer smaller than the window");
        if (win.poses() == 0) return;
        lgs_scan* s = const_cast<lgs_scan*>(scan);
        run_gs(ctx, params, nullptr, win, &grid, &s, &initial, 1, DBL_MIN, nullptr, scores);
    });
}

static int loop_detect_gs_run(lgs_ctx* ctx, const lgs_gs_params* params, const lgs_cost_ge_params* cost,
                              CostAlt alt, double score_threshold, const lgs_loop_query* queries,
                              int num_queries, const lgs_loop_candidate* candidates, int num_candidates,
                              lgs_loop_result* results)
{
    if (!ctx || !params || !cost || (num_queries > 0 && !queries) || num_queries < 0 || num_candidates < 0 ||
        (num_candidates > 0 && (!candidates || !results)))
        return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        GSWindow win;
        check_gs(params, cost, win);
        const std::vector<int> query_of =
            check_loop_batch(score_threshold, queries, num_queries, candidates, num_candidates, ":20-21");
        std::vector<const lgs_grid*> grids;
        std::vector<lgs_scan*> sc;
        std::vector<lgs_pose2d> poses;
        for (int k = 0; k < num_candidates; ++k) {
            const lgs_loop_candidate& c = candidates[k];
            // this matcher's own rule (no scan can be created empty; run_gs relies on it)
            LGS_REQUIRE(c.scan->n >= 1, "empty scan");
            grids.push_back(queries[query_of[(size_t)k]].map);   // the candidates of one query share its map
            sc.push_back(const_cast<lgs_scan*>(c.scan));
            poses.push_back(c.node_pose);
        }
        if (num_candidates == 0) return;
        std::vector<lgs_rtcsm_summary> sums((size_t)num_candidates);
        run_gs(ctx, params, cost, win, grids.data(), sc.data(), poses.data(), num_candidates, score_threshold,
               sums.data(), nullptr, alt);
        for (int k = 0; k < num_candidates; ++k)   // FindCorrespondingPose (:88-106)
            fill_loop_result(results[k], queries[query_of[(size_t)k]], candidates[k], sums[(size_t)k]);
    });
}

extern "C" int lgs_loop_detect_gs(lgs_ctx* ctx, const lgs_gs_params* params, const lgs_cost_ge_params* cost,
                                  double score_threshold, const lgs_loop_query* queries, int num_queries,
                                  const lgs_loop_candidate* candidates, int num_candidates,
                                  lgs_loop_result* results)
{
    return loop_detect_gs_run(ctx, params, cost, CostAlt{}, score_threshold, queries, num_queries, candidates,
                              num_candidates, results);
}

// With the square-error cost a failing call leaves `results` as it found them.
extern "C" int lgs_loop_detect_gs_cost(lgs_ctx* ctx, const lgs_gs_params* params, const lgs_cost_spec* cost,
                                       double score_threshold, const lgs_loop_query* queries, int num_queries,
                                       const lgs_loop_candidate* candidates, int num_candidates,
                                       lgs_loop_result* results)
{
    CostSel sel;
    if (const int rc = cost_select(cost, &sel)) return rc;
    if (!sel.alt)
        return lgs_loop_detect_gs(ctx, params, sel.ge, score_threshold, queries, num_queries, candidates,
                                  num_candidates, results);
    if (num_candidates < 0 || (num_candidates > 0 && !results)) return LGS_ERR_INVALID_ARG;
    return with_own_output(ctx, results, num_candidates, [&](lgs_loop_result* o) {
        return loop_detect_gs_run(ctx, params, sel.ge, sel.alt, score_threshold, queries, num_queries, candidates,
                                  num_candidates, o);
    });
}
