// k_loop_search.hip -- the nearest-node loop searcher, batched over hints
// (LoopSearcherNearest::Search,
// C/mapping/loop_searcher_nearest.cpp:13-108).
//
// A snapshot's walk (positions (map, node) of the maps 0 .. m - 2 in order),
// its travel chain and the maps' first positions are formed on the host
// (loop_search_host.hpp) and live on the device behind an lgs_loop_graph.  A
// search of q hints is three launches on the context's stream:
//
//   k_loop_cut      one thread per hint: cut = the lowest walked position with
//                   accum - travel[p] < threshold, by bisection (travel is
//                   non-decreasing, so the predicate is monotone)
//   k_loop_main     a workgroup owns 256 hints (one per thread) and a group
//                   of whole consecutive maps.  The group's x / y are staged in
//                   LDS in rounds of kLoopRound positions; every lane reads the
//                   same staged position in the same iteration (a same-address
//                   LDS read: a broadcast, no bank conflict) and keeps the
//                   current map's (best d2, position) under a strict <,
//                   predicated on p < cut.  At a map's end (workgroup-uniform)
//                   the map's best is stored as its per-map row when asked,
//                   map-major so that a wave's stores coalesce, and folded
//                   into the group's best under the same strict <.  One
//                   partial per (group, hint)
//   k_loop_combine  one thread per hint folds the partials in group order
//                   under the same strict < and fills the record
//
// Strict < updated in position order is "lowest position wins", an
// associative reduction: the bytes do not depend on the tile, the group size
// or the round.  No atomics, no scratch, nothing ordered between workgroups.
// The host transposes the per-map table into the caller's hint-major layout
// while it copies it out of pinned memory.
#include "lgs_internal.hpp"
#include "loop_search_host.hpp"

using namespace lgs;

struct lgs_loop_graph {
    lgs_ctx* ctx = nullptr;
    int device = 0;
    int n = 0, m = 0;
    std::vector<lgs_pose2d> poses;
    std::vector<int> idx_min, idx_max;
    LoopWalk walk;
    // device: walk x / y, travel, map_start[m], idx_min[m] (one allocation)
    void* mem = nullptr;
    double2* d_xy = nullptr;
    double* d_travel = nullptr;
    int* d_map_start = nullptr;
    int* d_idx_min = nullptr;
};

namespace {

constexpr int kLoopTile = 256;     // hints per workgroup, one per thread
constexpr int kLoopRound = 1024;   // positions staged in LDS per round (16 KiB)
constexpr int kLoopMaxGroups = 65535;   // groups of a launch (gridDim.y)

struct LoopHintDev {
    double rx, ry, accum;   // the latest node's x / y, accumTravelDist
    int limit;              // map_start[num_maps - 1]: positions the hint may walk
    int latest, lm_min, lm_max;   // the latest node and its local map's range
};
struct LoopPartial {
    double d2;
    int p, pad;
};

inline size_t ls_align256(size_t b) { return (b + 255) & ~(size_t)255; }

__global__ __launch_bounds__(256) void k_loop_cut(const LoopHintDev* __restrict__ hints, int q,
                                                  const double* __restrict__ travel, double travel_thr,
                                                  int* __restrict__ cut)
{
    const int h = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (h >= q) return;
    const double accum = hints[h].accum;
    int lo = 0, hi = hints[h].limit;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (accum - travel[mid] < travel_thr) hi = mid;
        else lo = mid + 1;
    }
    cut[h] = lo;
}

__global__ __launch_bounds__(kLoopTile) void k_loop_main(const LoopHintDev* __restrict__ hints,
                                                         const int* __restrict__ cut, int q,
                                                         const double2* __restrict__ wxy,
                                                         const int* __restrict__ map_start,
                                                         const int* __restrict__ idx_min,
                                                         const int* __restrict__ group_first, double min_sq,
                                                         LoopPartial* __restrict__ partials,
                                                         lgs_loop_search_map_best* __restrict__ table)
{
    __shared__ double2 s_xy[kLoopRound];
    __shared__ int s_cut[kLoopTile / 64];
    const int tid = (int)threadIdx.x;
    const int g = (int)blockIdx.y;
    const int h = (int)blockIdx.x * kLoopTile + tid;
    const bool valid = h < q;
    const int map_a = group_first[g], map_b = group_first[g + 1];
    const int p_begin = map_start[map_a], p_end = map_start[map_b];

    const int mycut = valid ? cut[h] : 0;
    const double rx = valid ? hints[h].rx : 0.0, ry = valid ? hints[h].ry : 0.0;
    // the tile's largest cut: no lane takes a position from there on
    int c = mycut;
    for (int d = 32; d >= 1; d >>= 1) c = max(c, __shfl_xor(c, d, 64));
    if ((tid & 63) == 0) s_cut[tid >> 6] = c;
    __syncthreads();
    c = max(max(s_cut[0], s_cut[1]), max(s_cut[2], s_cut[3]));
    const int end = min(p_end, __builtin_amdgcn_readfirstlane(c));

    double gb = min_sq, mb = min_sq;   // the group's and the current map's best
    int gp = -1, mp = -1;
    int cur = map_a;
    int cur_begin = p_begin, cur_end = map_start[cur + 1];
    // the end of map `cur`: its row, its fold into the group's best
    auto flush = [&]() {
        if (table && valid) {
            lgs_loop_search_map_best b;
            b.node_idx = mp >= 0 ? idx_min[cur] + (mp - cur_begin) : -1;
            b.pad_ = 0;
            b.dist_sq = mb;
            table[(size_t)cur * (size_t)q + (size_t)h] = b;
        }
        if (mb < gb) {
            gb = mb;
            gp = mp;
        }
        mb = min_sq;
        mp = -1;
        ++cur;
        cur_begin = cur_end;
        cur_end = cur < map_b ? map_start[cur + 1] : INT_MAX;
    };

    for (int base = p_begin; base < end; base += kLoopRound) {
        const int cnt = min(kLoopRound, end - base);
        __syncthreads();   // the previous round has been read
        for (int i = tid; i < cnt; i += kLoopTile) s_xy[i] = wxy[base + i];
        __syncthreads();
        int p = base;
        while (p < base + cnt) {
            const int seg_end = min(base + cnt, cur_end);
            for (; p < seg_end; ++p) {
                const double2 v = s_xy[p - base];
                const double dx = v.x - rx, dy = v.y - ry;
                const double d2 = dx * dx + dy * dy;
                const bool take = (d2 < mb) && (p < mycut);
                mb = take ? d2 : mb;
                mp = take ? p : mp;
            }
            if (p == cur_end) flush();
        }
    }
    // the map the tile's cut fell in, and the maps past it: nothing more to take
    while (cur < map_b) flush();
    if (valid) {
        LoopPartial o;
        o.d2 = gb;
        o.p = gp;
        o.pad = 0;
        partials[(size_t)g * (size_t)q + (size_t)h] = o;
    }
}

__global__ __launch_bounds__(256) void k_loop_combine(const LoopHintDev* __restrict__ hints,
                                                      const int* __restrict__ cut, int q,
                                                      const LoopPartial* __restrict__ partials, int groups,
                                                      const int* __restrict__ map_start,
                                                      const int* __restrict__ idx_min, int m, double min_sq,
                                                      int num_candidate_nodes,
                                                      lgs_loop_search_result* __restrict__ results,
                                                      lgs_loop_search_map_best* __restrict__ table)
{
    const int h = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (h >= q) return;
    double gb = min_sq;
    int gp = -1;
    for (int g = 0; g < groups; ++g) {
        const LoopPartial part = partials[(size_t)g * (size_t)q + (size_t)h];
        if (part.d2 < gb) {
            gb = part.d2;
            gp = part.p;
        }
    }
    lgs_loop_search_result r;
    r.found = gp >= 0 ? 1 : 0;
    r.local_map_idx = r.local_map_node_idx = r.node_idx_min = r.node_idx_max = -1;
    r.walked = cut[h];
    r.dist_sq = gb;
    if (gp >= 0) {
        // the map of position gp: the last of the maps 0 .. m - 2 that starts at or before it
        int lo = 0, hi = m - 2;
        while (lo < hi) {
            const int mid = lo + ((hi - lo + 1) >> 1);
            if (map_start[mid] <= gp) lo = mid;
            else hi = mid - 1;
        }
        const LoopHintDev H = hints[h];
        r.local_map_idx = lo;
        r.local_map_node_idx = idx_min[lo] + (gp - map_start[lo]);
        const long long a = (long long)H.latest - num_candidate_nodes, b = (long long)H.latest + num_candidate_nodes;
        r.node_idx_min = (int)(a > H.lm_min ? a : (long long)H.lm_min);
        r.node_idx_max = (int)(b < H.lm_max ? b : (long long)H.lm_max);
    }
    results[h] = r;
    // the latest map is in no group: its row is none
    if (table) {
        lgs_loop_search_map_best b;
        b.node_idx = -1;
        b.pad_ = 0;
        b.dist_sq = min_sq;
        table[(size_t)(m - 1) * (size_t)q + (size_t)h] = b;
    }
}

void graph_free(lgs_loop_graph* g)
{
    if (!g) return;
    if (g->mem) {
        hipSetDevice(g->device);
        hipFree(g->mem);
    }
    delete g;
}
struct GraphDeleter {
    void operator()(lgs_loop_graph* g) const { graph_free(g); }
};

lgs_loop_graph* graph_create(lgs_ctx* ctx, const lgs_pose2d* poses, int n, const int* idx_min, const int* idx_max, int m)
{
    // every check before any device work
    LGS_REQUIRE(loop_search_check_graph(poses, n, idx_min, idx_max, m, nullptr) == LGS_OK,
                "loop graph: 1 .. 2^27 nodes and maps, ranges inside [0, n), finite poses");
    std::unique_ptr<lgs_loop_graph, GraphDeleter> g(new lgs_loop_graph());
    g->ctx = ctx;
    g->device = ctx->device;
    g->n = n;
    g->m = m;
    g->poses.assign(poses, poses + n);
    g->idx_min.assign(idx_min, idx_min + m);
    g->idx_max.assign(idx_max, idx_max + m);
    g->walk = loop_walk_build(poses, idx_min, idx_max, m);
    const size_t P = (size_t)g->walk.positions, PP = std::max<size_t>(P, 1);
    const size_t xb = ls_align256(sizeof(double2) * PP), tb = ls_align256(sizeof(double) * PP),
                 ib = ls_align256(sizeof(int) * (size_t)m);
    LGS_HIP_CHECK(hipSetDevice(ctx->device));
    if (hipMalloc(&g->mem, xb + tb + 2 * ib) != hipSuccess) throw Error(LGS_ERR_OOM, "hipMalloc failed for loop graph");
    g->d_xy = (double2*)g->mem;
    g->d_travel = (double*)((char*)g->mem + xb);
    g->d_map_start = (int*)((char*)g->mem + xb + tb);
    g->d_idx_min = (int*)((char*)g->mem + xb + tb + ib);
    // one staged image, one copy
    std::vector<char> img(xb + tb + 2 * ib, 0);
    double2* hx = (double2*)img.data();
    for (size_t p = 0; p < P; ++p) hx[p] = make_double2(g->walk.x[p], g->walk.y[p]);
    if (P) std::memcpy(img.data() + xb, g->walk.travel.data(), sizeof(double) * P);
    std::memcpy(img.data() + xb + tb, g->walk.map_start.data(), sizeof(int) * (size_t)m);
    std::memcpy(img.data() + xb + tb + ib, idx_min, sizeof(int) * (size_t)m);
    LGS_HIP_CHECK(hipMemcpyAsync(g->mem, img.data(), img.size(), hipMemcpyHostToDevice, ctx->stream));
    ctx->sync();
    return g.release();
}

// hints per device pass: the per-map table of a pass stays near 64 MiB
int chunk_hints(int q, int m, bool table)
{
    long long c = table ? std::max<long long>(kLoopTile, ((1LL << 22) / m) / kLoopTile * kLoopTile) : (1LL << 20);
    return (int)std::min<long long>(q, c);
}

int group_positions(const lgs_ctx* ctx, int positions, int chunk)
{
    if (ctx->loop_group > 0) return ctx->loop_group;
    // about 2048 workgroups per pass, groups of at least 512 positions
    const int tiles = (chunk + kLoopTile - 1) / kLoopTile;
    const int wanted = std::max(1, 2048 / tiles);
    return std::max(512, (positions + wanted - 1) / wanted);
}

void search_device(lgs_loop_graph* G, const lgs_loop_search_params* prm, const lgs_loop_search_hint* hints, int q,
                   lgs_loop_search_result* results, lgs_loop_search_map_best* per_map)
{
    lgs_ctx* ctx = G->ctx;
    const int m = G->m, P = G->walk.positions;
    const double min_sq = loop_search_min_sq(prm);
    LGS_HIP_CHECK(hipSetDevice(ctx->device));
    const int Qc = chunk_hints(q, m, per_map != nullptr);
    // the groups are the grid's y dimension: a target too small for that many is doubled until they fit
    int target = group_positions(ctx, P, Qc);
    std::vector<int> first = loop_group_partition(G->walk.map_start, target);
    while ((int)first.size() - 1 > kLoopMaxGroups) {
        target = target > (1 << 29) ? INT_MAX : 2 * target;
        first = loop_group_partition(G->walk.map_start, target);
    }
    const int groups = (int)first.size() - 1;
    std::vector<LoopHintDev> hd;
    for (int q0 = 0; q0 < q; q0 += Qc) {
        const int qc = std::min(Qc, q - q0);
        hd.resize((size_t)qc);
        for (int j = 0; j < qc; ++j) {
            const lgs_loop_search_hint& s = hints[q0 + j];
            LoopHintDev& d = hd[(size_t)j];
            d.rx = G->poses[(size_t)s.latest_node_idx].x;
            d.ry = G->poses[(size_t)s.latest_node_idx].y;
            d.accum = s.accum_travel_dist;
            d.limit = G->walk.map_start[(size_t)s.num_maps - 1];
            d.latest = s.latest_node_idx;
            d.lm_min = G->idx_min[(size_t)s.latest_local_map_idx];
            d.lm_max = G->idx_max[(size_t)s.latest_local_map_idx];
        }
        Upload up(ctx);
        const size_t ho = up.append(hd.data(), hd.size());
        const size_t fo = up.append(first.data(), first.size());
        up.flush();
        const size_t cb = ls_align256(sizeof(int) * (size_t)qc);
        const size_t pb = ls_align256(sizeof(LoopPartial) * (size_t)std::max(groups, 1) * (size_t)qc);
        const size_t rb = ls_align256(sizeof(lgs_loop_search_result) * (size_t)qc);
        const size_t tb = per_map ? ls_align256(sizeof(lgs_loop_search_map_best) * (size_t)m * (size_t)qc) : 0;
        char* w0 = (char*)ctx->ensure(S_LOOPS0, cb + pb);
        char* w1 = (char*)ctx->ensure(S_LOOPS1, rb + tb);
        int* d_cut = (int*)w0;
        LoopPartial* d_part = (LoopPartial*)(w0 + cb);
        lgs_loop_search_result* d_res = (lgs_loop_search_result*)w1;
        lgs_loop_search_map_best* d_tab = per_map ? (lgs_loop_search_map_best*)(w1 + rb) : nullptr;
        const LoopHintDev* d_h = up.at<LoopHintDev>(ho);
        const int blocks = (qc + 255) / 256;
        const int tok = ctx->timing_begin(K_LOOP_SEARCH, 16.0 * (double)qc * (double)P);
        hipLaunchKernelGGL(k_loop_cut, dim3(blocks), dim3(256), 0, ctx->stream, d_h, qc, G->d_travel,
                           prm->travel_dist_threshold, d_cut);
        LGS_HIP_CHECK(hipGetLastError());
        if (groups > 0) {
            hipLaunchKernelGGL(k_loop_main, dim3((qc + kLoopTile - 1) / kLoopTile, groups), dim3(kLoopTile), 0,
                               ctx->stream, d_h, d_cut, qc, G->d_xy, G->d_map_start, G->d_idx_min, up.at<int>(fo),
                               min_sq, d_part, d_tab);
            LGS_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_loop_combine, dim3(blocks), dim3(256), 0, ctx->stream, d_h, d_cut, qc, d_part, groups,
                           G->d_map_start, G->d_idx_min, m, min_sq, prm->num_candidate_nodes, d_res, d_tab);
        LGS_HIP_CHECK(hipGetLastError());
        ctx->timing_end(tok);
        ctx->loop_launches += groups > 0 ? 3 : 2;
        char* pin = (char*)ctx->ensure_pinned(rb + tb);
        LGS_HIP_CHECK(hipMemcpyAsync(pin, w1, rb + tb, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        std::memcpy(results + q0, pin, sizeof(lgs_loop_search_result) * (size_t)qc);
        if (per_map) {
            // map-major on the device, hint-major for the caller
            const lgs_loop_search_map_best* t = (const lgs_loop_search_map_best*)(pin + rb);
            // 256 hints at a time: the device rows are read in runs of 4 KiB, and the 256 cache lines
            // being written (four maps' entries of one hint each) stay in L1 from one map to the next.
            // Measured against 32 x 32 blocks, which were slower at 64 and 1000 hints
            for (int j0 = 0; j0 < qc; j0 += kLoopTile) {
                const int j1 = std::min(qc, j0 + kLoopTile);
                for (int i = 0; i < m; ++i)
                    for (int j = j0; j < j1; ++j)
                        per_map[(size_t)(q0 + j) * (size_t)m + (size_t)i] = t[(size_t)i * (size_t)qc + (size_t)j];
            }
        }
    }
    ctx->loop_device_calls += 1;
    ctx->loop_pairs += (long long)q * (long long)P;
}

}  // namespace

extern "C" int lgs_loop_graph_create(lgs_ctx* ctx, const lgs_pose2d* poses, int n, const int* idx_min,
                                     const int* idx_max, int m, lgs_loop_graph** out)
{
    if (!ctx || !poses || !idx_min || !idx_max || !out) return LGS_ERR_INVALID_ARG;
    *out = nullptr;
    return guarded(ctx, [&] { *out = graph_create(ctx, poses, n, idx_min, idx_max, m); });
}

extern "C" void lgs_loop_graph_destroy(lgs_loop_graph* graph) { graph_free(graph); }

extern "C" int lgs_loop_graph_info(const lgs_loop_graph* graph, int* n, int* m, int* positions, double* walk_travel)
{
    if (!graph) return LGS_ERR_INVALID_ARG;
    if (n) *n = graph->n;
    if (m) *m = graph->m;
    if (positions) *positions = graph->walk.positions;
    if (walk_travel) *walk_travel = graph->walk.positions ? graph->walk.travel.back() : 0.0;
    return LGS_OK;
}

extern "C" int lgs_loop_graph_travel(const lgs_loop_graph* graph, double* out, int cap)
{
    if (!graph || !out || cap < graph->walk.positions) return LGS_ERR_INVALID_ARG;
    if (graph->walk.positions) std::memcpy(out, graph->walk.travel.data(), sizeof(double) * (size_t)graph->walk.positions);
    return LGS_OK;
}

extern "C" int lgs_loop_search_nearest(lgs_loop_graph* graph, const lgs_loop_search_params* params,
                                       const lgs_loop_search_hint* hints, int q, lgs_loop_search_result* results,
                                       lgs_loop_search_map_best* per_map)
{
    if (!graph || !params || !hints || !results || q < 0) return LGS_ERR_INVALID_ARG;
    lgs_loop_graph* G = graph;
    return guarded(G->ctx, [&] {
        // every check before any device work
        LGS_REQUIRE(loop_search_check_params(params) == LGS_OK, "loop search: finite thresholds, num_candidate_nodes >= 0");
        LGS_REQUIRE(loop_search_check_hints(hints, q, G->n, G->idx_min.data(), G->idx_max.data(), G->m) == LGS_OK,
                    "loop search: a hint's num_maps, latest map, latest node or travel distance is out of range");
        if (q == 0) return;
        lgs_ctx* ctx = G->ctx;
        const long long pairs = (long long)q * (long long)G->walk.positions;
        if (pairs < ctx->loop_min_pairs) {
            for (int j = 0; j < q; ++j)
                loop_search_statement(G->poses.data(), G->idx_min.data(), G->idx_max.data(), G->m, params, hints[j],
                                      G->walk.travel.data(), results + j,
                                      per_map ? per_map + (size_t)j * (size_t)G->m : nullptr);
            ctx->loop_host_calls += 1;
            return;
        }
        search_device(G, params, hints, q, results, per_map);
    });
}

extern "C" int lgs_loop_search_nearest_host(const lgs_pose2d* poses, int n, const int* idx_min, const int* idx_max,
                                            int m, const lgs_loop_search_params* params,
                                            const lgs_loop_search_hint* hints, int q, lgs_loop_search_result* results,
                                            lgs_loop_search_map_best* per_map)
{
    if (!poses || !idx_min || !idx_max || !params || !hints || !results || q < 0) return LGS_ERR_INVALID_ARG;
    return guarded(nullptr, [&] {
        const int rc = loop_search_host(poses, n, idx_min, idx_max, m, params, hints, q, results, per_map);
        if (rc != LGS_OK) throw Error(rc, "loop search: invalid argument");
    });
}

extern "C" int lgs_pg_accum_travel_dist(const lgs_pose2d* poses, int n, double* out)
{
    if (!poses || !out || n < 1) return LGS_ERR_INVALID_ARG;
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(poses[k].x) || !std::isfinite(poses[k].y)) return LGS_ERR_INVALID_ARG;
    *out = loop_accum_travel_dist(poses, n);
    return LGS_OK;
}

extern "C" int lgs_loop_search_stats(const lgs_ctx* ctx, long long* out4)
{
    if (!ctx || !out4) return LGS_ERR_INVALID_ARG;
    out4[0] = ctx->loop_device_calls;
    out4[1] = ctx->loop_host_calls;
    out4[2] = ctx->loop_launches;
    out4[3] = ctx->loop_pairs;
    return LGS_OK;
}
