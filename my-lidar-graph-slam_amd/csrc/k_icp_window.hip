// k_icp_window.hip -- the ICP loop detector's window search of start poses
// (DESIGN.md 4.5e): candidates x lattice poses x beams grid searches against
// lgs_icp_ref references, then one refine per candidate from its best pose.
//
//   score   k_icp_window   one workgroup of 256 threads per (candidate, theta
//                          index, slice of 4 .. 64 translations: the plan of
//                          icp_window_host.hpp).
//                          Phase 1, once per workgroup: the robot theta's
//                          sincos and the rotated relPose (Compound's terms),
//                          then per beam its usability and (r cos, r sin) at
//                          sensor theta + a_i into LDS, usability as one bit
//                          per beam.  A translation then costs two adds per
//                          beam and no sincos.
//                          Phase 2: one wave per translation, striding over
//                          the slice.  The wave walks the 1024-thread tree of
//                          icp_pass (icp_device.hpp) by itself: for w = 0 ..
//                          15 lane l adds beams 64 w + l, + 1024, ... from
//                          +0.0, butterflies with masks 32 .. 1, and the
//                          sixteen sums are added in w order.  Only the cost
//                          and the pair count are formed; the search is
//                          icpref_search (icp_ref_device.hpp), the pairing
//                          rule icpref_pair's.  Each wave keeps its
//                          lexicographic minimum of (cost, p); the workgroup
//                          combines four through LDS and writes one partial.
//   (host)                 the minimum of a candidate's partials, the refine
//                          items, run_icp_ref (k_icp_ref.hip), the gate and
//                          the records (icp_window_host.hpp)
//
// No atomics on floating-point data; nothing depends on the order in which
// workgroups finish.
#include "icp_ref_device.hpp"
#include "icp_window_host.hpp"

#include <vector>

using namespace lgs;

namespace {

constexpr int kWinThreads = 256;
constexpr int kWinWaves = kWinThreads / 64;
constexpr size_t kWinLdsDefault = 48 * 1024;   // dynamic LDS a launch may ask for without the attribute

// one candidate of a launch
struct WinItem {
    IcpRefDev ref;
    const double* ranges;
    const double* angles;
    double lo, hi;       // usable range of the scan
    double centre[3];    // the window's centre (robot pose)
    double rel[3];       // the scan's relative sensor pose
    int n, pad;
};

// what every workgroup of a launch shares
struct WinShared {
    double step_xy, step_theta, D2;
    int half_x, half_y, half_theta;
    int nx, ny, nt;
    int slices;   // per theta index
    int slice_len;
    int P;
    int store;    // also write every pose's cost and pairs (the dense entry point)
};

inline size_t win_lds_bytes(int n) { return sizeof(double2) * (size_t)n + sizeof(unsigned) * 2 * (size_t)((n + 63) / 64); }

__global__ __launch_bounds__(kWinThreads) void k_icp_window(const WinItem* __restrict__ items, WinShared W,
                                                            IcpWinPartial* __restrict__ parts,
                                                            double* __restrict__ cost_out, int* __restrict__ pairs_out,
                                                            int* __restrict__ err)
{
    extern __shared__ double2 hit[];   // [n] (r cos, r sin); then one usability bit per beam
    __shared__ IcpWinPartial wbest[kWinWaves];
    const int b = blockIdx.x;
    const int slice = b % W.slices;
    const int it = (b / W.slices) % W.nt;
    const int cand = b / (W.slices * W.nt);
    const WinItem* __restrict__ X = items + cand;
    const IcpRefDev R = X->ref;
    const int n = X->n;
    unsigned* ubits = (unsigned*)(hit + n);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);

    // ---- phase 1: Compound(lattice pose, relPose) without its translation
    const double lt = icp_window_coord(X->centre[2], it, W.half_theta, W.step_theta);
    if (!glm::gl_sincos_ok(lt) && lt - lt == 0.0) *err = 1;
    double sinT, cosT;
    glm::gl_sincos(lt, &sinT, &cosT);
    const double ox = cosT * X->rel[0] - sinT * X->rel[1];
    const double oy = sinT * X->rel[0] + cosT * X->rel[1];
    const double st = lt + X->rel[2];
    {
        const double lo = X->lo, hi = X->hi;
        const double* __restrict__ ranges = X->ranges;
        const double* __restrict__ angles = X->angles;
        for (int i0 = 0; i0 < n; i0 += kWinThreads) {
            const int i = i0 + (int)threadIdx.x;
            bool us = false;
            if (i < n) {
                const double r = gload(ranges + i);
                us = icp_dev_usable(r, lo, hi);
                double2 v = make_double2(0.0, 0.0);
                if (us) {
                    const double th = st + gload(angles + i);
                    if (!glm::gl_sincos_ok(th) && th - th == 0.0) *err = 1;   // icp_hit's rule
                    double sn, cs;
                    glm::gl_sincos(th, &sn, &cs);
                    v = make_double2(r * cs, r * sn);
                }
                hit[i] = v;
            }
            const unsigned long long bal = __ballot(us);
            const int first = i0 + wid * 64;   // the wave's first beam: a multiple of 64
            if (lane == 0 && first < n) {
                ubits[(first >> 5) + 0] = (unsigned)bal;
                ubits[(first >> 5) + 1] = (unsigned)(bal >> 32);
            }
        }
    }
    __syncthreads();

    // ---- phase 2: one wave per translation
    const int nxy = W.nx * W.ny;
    const int t0 = slice * W.slice_len, t1 = min(nxy, t0 + W.slice_len);
    double best = inf;
    int best_p = -1, best_pairs = 0;
    for (int tr = t0 + wid; tr < t1; tr += kWinWaves) {
        const int iy = tr / W.nx, ix = tr - iy * W.nx;
        const double sx = ox + icp_window_coord(X->centre[0], ix, W.half_x, W.step_xy);
        const double sy = oy + icp_window_coord(X->centre[1], iy, W.half_y, W.step_xy);
        double total = 0.0;
        int pairs = 0;
#pragma nounroll
        for (int w = 0; w < kIcpWaves; ++w) {
            double v = 0.0;
            int np = 0;
            if (64 * w < n) {   // else every lane holds +0.0 and no pair
                for (int i = 64 * w + lane; i < n; i += kIcpThreads) {
                    if (((ubits[i >> 5] >> (i & 31)) & 1u) == 0u) continue;
                    const double2 h = hit[i];
                    const double hx = sx + h.x, hy = sy + h.y;
                    double d2;
                    int jb;
                    icpref_search(R, hx, hy, d2, jb);
                    double term = W.D2;   // a usable beam without a pair
                    if (jb >= 0 && d2 <= W.D2) {
                        const double2 nn = gload(R.tn + jb);
                        if (nn.x == nn.x) {   // the entry has a line
                            const double2 q = gload(R.tq + jb);
                            const double dx = hx - q.x, dy = hy - q.y;
                            const double e = nn.x * dx + nn.y * dy;
                            term = e * e;
                            ++np;
                        }
                    }
                    v = v + term;
                }
#pragma unroll
                for (int mask = 32; mask >= 1; mask >>= 1) {
                    v = v + __shfl_xor(v, mask, 64);
                    np += __shfl_xor(np, mask, 64);
                }
            }
            total = (w == 0) ? v : total + v;
            pairs += np;
        }
        const int p = (it * W.ny + iy) * W.nx + ix;
        if (W.store && lane == 0) {
            const size_t at = (size_t)cand * (size_t)W.P + (size_t)p;
            cost_out[at] = total;
            pairs_out[at] = pairs;
        }
        if (icp_window_better(total, p, best, best_p)) {
            best = total;
            best_p = p;
            best_pairs = pairs;
        }
    }
    if (lane == 0) wbest[wid] = IcpWinPartial{ best, best_p, best_pairs };
    __syncthreads();
    if (threadIdx.x == 0) {
        IcpWinPartial o = wbest[0];
        for (int w = 1; w < kWinWaves; ++w)
            if (wbest[w].p >= 0 && icp_window_better(wbest[w].cost, wbest[w].p, o.cost, o.p)) o = wbest[w];
        parts[b] = o;
    }
}

// ------------------------------------------------------------------ host
struct WinJob {
    const lgs_icp_ref* ref;
    const lgs_scan* scan;
    lgs_pose2d centre;
};

// the checks of one window that need no device (throw LGS_ERR_INVALID_ARG)
void win_job_check(const lgs_ctx* ctx, const WinJob& j, const lgs_icp_window* w, const lgs_icp_params* p)
{
    ref_call_check(ctx, j.ref, j.scan, j.centre, p);
    LGS_REQUIRE(j.scan->n <= kIcpWinMaxBeams, "icp window: more than LGS_ICP_WINDOW_MAX_BEAMS beams");
    LGS_REQUIRE(icp_window_finite(*w, j.centre), "icp window: a lattice pose is not finite");
}

// The windows of n checked jobs: best[j] is job j's minimum of (cost, p);
// cost / pairs (null, or P entries per job) receive every pose's score.  One
// launch and one wait per chunk of candidates.
void run_icp_window(lgs_ctx* ctx, const WinJob* jobs, int n, const lgs_icp_window* w, const lgs_icp_params* p,
                    IcpWinPartial* best, double* cost, int* pairs)
{
    const IcpWinDims d = icp_window_dims(*w);
    LGS_HIP_CHECK(hipSetDevice(ctx->device));
    std::vector<const lgs_scan*> scans((size_t)n);
    for (int j = 0; j < n; ++j) scans[(size_t)j] = jobs[j].scan;
    scans_to_device(ctx, scans.data(), n);
    std::vector<WinItem> items((size_t)n);
    int max_n = 1;
    for (int j = 0; j < n; ++j) {
        WinItem& it = items[(size_t)j];
        std::memset(&it, 0, sizeof(it));
        const lgs_scan* s = jobs[j].scan;
        it.ref = jobs[j].ref->dev;
        it.ranges = s->d_ranges;
        it.angles = s->d_angles;
        it.lo = std::max(p->usable_range_min, s->min_range);
        it.hi = std::min(p->usable_range_max, s->max_range);
        it.centre[0] = jobs[j].centre.x;
        it.centre[1] = jobs[j].centre.y;
        it.centre[2] = jobs[j].centre.theta;
        it.rel[0] = s->rel.x;
        it.rel[1] = s->rel.y;
        it.rel[2] = s->rel.theta;
        it.n = s->n;
        max_n = std::max(max_n, s->n);
    }
    const size_t lds = win_lds_bytes(max_n);
    if (lds > kWinLdsDefault)
        LGS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_icp_window),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    Upload up(ctx);
    const size_t io = up.append(items.data(), items.size());
    up.flush();

    WinShared W;
    std::memset(&W, 0, sizeof(W));
    W.step_xy = w->step_xy;
    W.step_theta = w->step_theta;
    W.D2 = p->max_correspondence_dist * p->max_correspondence_dist;   // icp_shared's product
    W.half_x = w->half_x;
    W.half_y = w->half_y;
    W.half_theta = w->half_theta;
    W.nx = d.nx;
    W.ny = d.ny;
    W.nt = d.nt;
    W.P = d.P;
    W.store = cost ? 1 : 0;

    const int chunk = std::min(n, icp_window_chunk_cands(d));
    const size_t cb = cost ? icp_align256(sizeof(double) * (size_t)chunk * (size_t)d.P) : 0;
    const size_t ib = cost ? icp_align256(sizeof(int) * (size_t)chunk * (size_t)d.P) : 0;
    char* dense = cost ? (char*)ctx->ensure(S_ICPW1, cb + ib) : nullptr;
    for (int j0 = 0; j0 < n; j0 += chunk) {
        const int m = std::min(chunk, n - j0);
        const IcpWinPlan pl = icp_window_plan(d, m);
        W.slices = pl.slices;
        W.slice_len = pl.slice_len;
        const size_t pb = icp_align256(sizeof(IcpWinPartial) * (size_t)m * (size_t)pl.groups);
        char* small = (char*)ctx->ensure(S_ICPW0, pb + 256);
        IcpWinPartial* d_parts = (IcpWinPartial*)small;
        int* d_err = (int*)(small + pb);
        LGS_HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream));
        // at most 2^26 / slice_len + m * nt workgroups where slices are long, about kIcpWinTargetGroups where short
        const unsigned groups = (unsigned)m * (unsigned)pl.groups;
        hipLaunchKernelGGL(k_icp_window, dim3(groups), dim3(kWinThreads), lds, ctx->stream, up.at<WinItem>(io) + j0, W,
                           d_parts, (double*)dense, (int*)(dense ? dense + cb : nullptr), d_err);
        LGS_HIP_CHECK(hipGetLastError());
        ctx->icpwin_score_launches += 1;
        char* pin = (char*)ctx->ensure_pinned(pb + 256 + cb + ib);
        LGS_HIP_CHECK(hipMemcpyAsync(pin, small, pb + 256, hipMemcpyDeviceToHost, ctx->stream));
        if (cost) LGS_HIP_CHECK(hipMemcpyAsync(pin + pb + 256, dense, cb + ib, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        ctx->icpwin_syncs += 1;
        if (*(const int*)(pin + pb) != 0) throw Error(LGS_ERR_INTERNAL, kSincosMsg);
        const IcpWinPartial* hp = (const IcpWinPartial*)pin;
        for (int j = 0; j < m; ++j)
            best[j0 + j] = icp_window_combine(hp + (size_t)j * (size_t)pl.groups, (size_t)pl.groups);
        if (cost) {
            std::memcpy(cost + (size_t)j0 * (size_t)d.P, pin + pb + 256, sizeof(double) * (size_t)m * (size_t)d.P);
            std::memcpy(pairs + (size_t)j0 * (size_t)d.P, pin + pb + 256 + cb, sizeof(int) * (size_t)m * (size_t)d.P);
        }
    }
}

// lgs_loop_detect_icp: results, best_index and summaries are written only when the whole call succeeded
void loop_detect_icp(lgs_ctx* ctx, const lgs_icp_ref* const* refs, const lgs_loop_query* queries, int num_queries,
                     const lgs_loop_candidate* candidates, int num_candidates, const lgs_icp_params* p,
                     const lgs_icp_window* w, const lgs_loop_refine_gate* gate, lgs_loop_result* results,
                     int* best_index, lgs_icp_summary* summaries)
{
    // every check before any device work
    std::vector<int> query_of;
    LGS_REQUIRE(loop_refine_ranges_check(queries, num_queries, num_candidates, query_of) == LGS_OK,
                "loop queries must cover the candidates contiguously, in order and completely");
    for (int q = 0; q < num_queries; ++q) LGS_REQUIRE(refs[q], "loop detect icp: a query without a reference");
    const int n = num_candidates;
    std::vector<WinJob> jobs((size_t)n);
    for (int c = 0; c < n; ++c) {
        LGS_REQUIRE(candidates[c].scan, "loop candidate without a scan");
        jobs[(size_t)c] = WinJob{ refs[query_of[(size_t)c]], candidates[c].scan, candidates[c].node_pose };
        win_job_check(ctx, jobs[(size_t)c], w, p);
    }
    if (n == 0) return;
    ctx->icpwin_calls += 1;
    std::vector<IcpWinPartial> best((size_t)n);
    run_icp_window(ctx, jobs.data(), n, w, p, best.data(), nullptr, nullptr);

    // one refine per candidate whose window has a winner, from that lattice pose
    std::vector<int> item_of;
    std::vector<const lgs_icp_ref*> irefs;
    std::vector<const lgs_scan*> iscans;
    std::vector<lgs_pose2d> init;
    for (int c = 0; c < n; ++c) {
        if (best[(size_t)c].p < 0) continue;
        item_of.push_back(c);
        irefs.push_back(jobs[(size_t)c].ref);
        iscans.push_back(jobs[(size_t)c].scan);
        init.push_back(icp_window_pose_of(*w, jobs[(size_t)c].centre, best[(size_t)c].p));
    }
    std::vector<lgs_icp_summary> sums(item_of.size());
    if (!item_of.empty()) {
        const long long before = ctx->icpref_refine_launches;
        run_icp_ref(ctx, irefs.data(), iscans.data(), init.data(), (int)item_of.size(), p, sums.data(), nullptr);
        ctx->icpwin_syncs += 1;
        ctx->icpwin_refine_launches += ctx->icpref_refine_launches - before;
    }
    // nothing can fail from here on
    std::vector<int> item_at((size_t)n, -1);
    for (size_t k = 0; k < item_of.size(); ++k) item_at[(size_t)item_of[k]] = (int)k;
    for (int c = 0; c < n; ++c) {
        const int k = item_at[(size_t)c];
        const lgs_icp_summary* s = k >= 0 ? &sums[(size_t)k] : nullptr;
        const bool ok = s && loop_refine_accept(*gate, *s, init[(size_t)k]);
        icp_window_record(results[c], queries[query_of[(size_t)c]], candidates[c], s, ok, candidates[c].scan->n);
        if (best_index) best_index[c] = best[(size_t)c].p;
        if (summaries) {
            if (s) summaries[c] = *s;
            else std::memset(&summaries[c], 0, sizeof(lgs_icp_summary));
        }
    }
}

}  // namespace

extern "C" size_t lgs_icp_window_size(void) { return sizeof(lgs_icp_window); }

extern "C" int lgs_icp_ref_window_scores(lgs_ctx* ctx, const lgs_icp_ref* ref, const lgs_scan* scan, lgs_pose2d centre,
                                         const lgs_icp_window* window, const lgs_icp_params* params, double* cost,
                                         int* pairs)
{
    if (!ctx || !ref || !scan || !window || !params || !cost || !pairs) return LGS_ERR_INVALID_ARG;
    if (icp_params_check(params) != LGS_OK || icp_window_check(window) != LGS_OK) return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        const WinJob job{ ref, scan, centre };
        win_job_check(ctx, job, window, params);
        ctx->icpwin_calls += 1;
        // a failing call writes nothing: the scores are formed aside
        const size_t P = (size_t)icp_window_dims(*window).P;
        std::vector<double> c(P);
        std::vector<int> n(P);
        IcpWinPartial best;
        run_icp_window(ctx, &job, 1, window, params, &best, c.data(), n.data());
        std::memcpy(cost, c.data(), sizeof(double) * P);
        std::memcpy(pairs, n.data(), sizeof(int) * P);
    });
}

extern "C" int lgs_loop_detect_icp(lgs_ctx* ctx, const lgs_icp_ref* const* refs, const lgs_loop_query* queries,
                                   int num_queries, const lgs_loop_candidate* candidates, int num_candidates,
                                   const lgs_icp_params* params, const lgs_icp_window* window,
                                   const lgs_loop_refine_gate* gate, lgs_loop_result* results, int* best_index,
                                   lgs_icp_summary* summaries)
{
    if (!ctx || !refs || !queries || !candidates || !params || !window || !gate || !results) return LGS_ERR_INVALID_ARG;
    if (icp_params_check(params) != LGS_OK || icp_window_check(window) != LGS_OK ||
        loop_refine_gate_check(gate) != LGS_OK)
        return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        loop_detect_icp(ctx, refs, queries, num_queries, candidates, num_candidates, params, window, gate, results,
                        best_index, summaries);
    });
}

extern "C" int lgs_icp_window_stats(const lgs_ctx* ctx, long long* calls, long long* score_launches, long long* syncs,
                                    long long* refine_launches)
{
    if (!ctx) return LGS_ERR_INVALID_ARG;
    if (calls) *calls = ctx->icpwin_calls;
    if (score_launches) *score_launches = ctx->icpwin_score_launches;
    if (syncs) *syncs = ctx->icpwin_syncs;
    if (refine_launches) *refine_launches = ctx->icpwin_refine_launches;
    return LGS_OK;
}
