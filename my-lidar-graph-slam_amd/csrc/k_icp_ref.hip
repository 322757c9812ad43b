// k_icp_ref.hip -- point-to-line ICP against a set of reference scans: the
// table of DESIGN.md 4.5b over scans R_0 .. R_{K-1}, built once on the device,
// kept in global memory behind an lgs_icp_ref, and searched through a uniform
// grid that returns the brute-force answer.
//
//   build   k_icpref_table   one workgroup per reference scan: icp_table_entry
//                            per beam, compaction in beam order at the scan's
//                            base (the host counted the usable beams), the
//                            scan's bounding box (finite points) and lines
//           (host)           boxes -> grid geometry (icp_ref_host.hpp)
//           k_icpref_count   entries per cell (integer atomics)
//           k_icpref_scan    exclusive prefix: cell starts, row-major cells
//           k_icpref_scatter the cell-ordered copy of (q, index); the order
//                            inside a cell is whatever the atomics gave
//   refine  k_icp_ref        one workgroup of 1024 threads per item for the
//                            whole loop (icp_refine of icp_device.hpp: the
//                            pass, the tree, the stopping rule and the solve
//                            of k_icp.hip).  Thread t owns beams t, t + 1024,
//                            ...; a beam walks the three rows around its hit
//                            point's cell, in each the contiguous range of
//                            cells cx - 1 .. cx + 1, and keeps the
//                            lexicographic minimum of (d2, index) -- so the
//                            order inside the cells does not matter and the
//                            result is a function of the inputs alone.
//   pairs   k_icp_ref_pairs  the search alone
//
// Many references in one pass (lgs_icp_ref_set_create): the
// same table kernel over all (reference, scan) jobs, then
//           k_icpref_count_set    k_icpref_count over a flat list of 256-entry
//                                 blocks, none of which straddles two references
//           k_icpref_scan_set     k_icpref_scan's body, one workgroup per reference
//           k_icpref_scatter_set  k_icpref_scatter over the same block list
// into two allocations that every reference's IcpRefDev points into.
#include "icp_ref_device.hpp"
#include "icp_ref_set_host.hpp"

#include <chrono>
#include <memory>
#include <vector>

using namespace lgs;

namespace {

constexpr int kRefChunk = 4096;   // items per launch

}  // namespace

struct lgs_icp_ref_set {
    int device = 0;
    void* mem_table = nullptr;   // every reference's tq, tn, tkj
    void* mem_cells = nullptr;   // every reference's cq, cidx, starts
    std::vector<lgs_icp_ref> refs;   // borrowed views into the two
};

namespace {

struct RefScanJob {
    const double* ranges;
    const double* angles;
    double pose[3];    // Compound(P_k, rel_k), glibc on the host
    double lo, hi;
    int n;
    int base, count;   // the scan's first entry and its usable beams (host count)
    int label, pad;    // the scan's index within its own reference (tkj.x)
};

using RefScanBox = IcpRefScanBox;

struct IcpRefItem {
    IcpItem it;        // the current scan's half (r_* unused)
    IcpRefDev ref;
};

__global__ __launch_bounds__(kIcpThreads) void k_icpref_table(const RefScanJob* __restrict__ jobs, double S2,
                                                              double2* __restrict__ tq, double2* __restrict__ tn,
                                                              int2* __restrict__ tkj, RefScanBox* __restrict__ boxes,
                                                              int* __restrict__ err)
{
    __shared__ int wcnt[kIcpWaves];
    __shared__ double wbox[kIcpWaves][4];
    __shared__ int wlines[kIcpWaves];
    const RefScanJob job = jobs[blockIdx.x];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    double mnx = inf, mxx = -inf, mny = inf, mxy = -inf;
    int lines = 0, base = 0;
    for (int j0 = 0; j0 < job.n; j0 += kIcpThreads) {
        const int j = j0 + (int)threadIdx.x;
        bool us = false;
        double qx = 0.0, qy = 0.0, nx = nan, ny = nan;
        if (j < job.n)
            us = icp_table_entry(job.ranges, job.angles, job.n, job.pose, job.lo, job.hi, S2, j, qx, qy, nx, ny, err);
        const unsigned long long bal = __ballot(us);
        if (lane == 0) wcnt[wid] = __popcll(bal);
        __syncthreads();
        int off = base, total = 0;
#pragma unroll
        for (int w = 0; w < kIcpWaves; ++w) {
            const int c = wcnt[w];
            off += (w < wid) ? c : 0;
            total += c;
        }
        off += __popcll(bal & ((1ull << lane) - 1ull));
        if (us && off < job.count) {
            const int e = job.base + off;
            tq[e] = make_double2(qx, qy);
            tn[e] = make_double2(nx, ny);
            tkj[e] = make_int2(job.label, j);
            if (qx - qx == 0.0 && qy - qy == 0.0) {
                mnx = fmin(mnx, qx);
                mxx = fmax(mxx, qx);
                mny = fmin(mny, qy);
                mxy = fmax(mxy, qy);
            }
            lines += (nx == nx) ? 1 : 0;
        }
        base += total;
        __syncthreads();
    }
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) {
        mnx = fmin(mnx, __shfl_xor(mnx, mask, 64));
        mxx = fmax(mxx, __shfl_xor(mxx, mask, 64));
        mny = fmin(mny, __shfl_xor(mny, mask, 64));
        mxy = fmax(mxy, __shfl_xor(mxy, mask, 64));
        lines += __shfl_xor(lines, mask, 64);
    }
    if (lane == 0) {
        wbox[wid][0] = mnx;
        wbox[wid][1] = mxx;
        wbox[wid][2] = mny;
        wbox[wid][3] = mxy;
        wlines[wid] = lines;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        RefScanBox b;
        b.min_x = wbox[0][0];
        b.max_x = wbox[0][1];
        b.min_y = wbox[0][2];
        b.max_y = wbox[0][3];
        b.lines = wlines[0];
        b.pad = 0;
        for (int w = 1; w < kIcpWaves; ++w) {
            b.min_x = fmin(b.min_x, wbox[w][0]);
            b.max_x = fmax(b.max_x, wbox[w][1]);
            b.min_y = fmin(b.min_y, wbox[w][2]);
            b.max_y = fmax(b.max_y, wbox[w][3]);
            b.lines += wlines[w];
        }
        boxes[blockIdx.x] = b;
    }
}

// the row-major cell of a table point, -1: none (a point that is not finite)
__device__ __forceinline__ int icpref_cell_of(const IcpRefGrid& g, double2 q)
{
    const int cx = icp_ref_cell(g.x, q.x), cy = icp_ref_cell(g.y, q.y);
    if (cx < 0 || cx >= g.x.n || cy < 0 || cy >= g.y.n) return -1;
    return cy * g.x.n + cx;
}

__global__ __launch_bounds__(256) void k_icpref_count(const double2* __restrict__ tq, int m, IcpRefGrid g,
                                                      int* __restrict__ counts)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    const int c = icpref_cell_of(g, tq[e]);
    if (c >= 0) atomicAdd(counts + c, 1);
}

// starts[c] = sum of counts[< c], starts[ncell] = the total; one workgroup,
// thread t owns the cells [t * chunk, (t + 1) * chunk)
__device__ __forceinline__ void icpref_scan_body(const int* __restrict__ counts, int ncell, int* __restrict__ starts,
                                                 int* part)
{
    const int t = threadIdx.x;
    const int chunk = (ncell + kIcpThreads - 1) / kIcpThreads;
    const int c0 = min(ncell, t * chunk), c1 = min(ncell, c0 + chunk);
    int s = 0;
    for (int c = c0; c < c1; ++c) s += counts[c];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < kIcpThreads; d <<= 1) {
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;   // exclusive
    for (int c = c0; c < c1; ++c) {
        starts[c] = run;
        run += counts[c];
    }
    if (t == kIcpThreads - 1) starts[ncell] = part[t];
}

__global__ __launch_bounds__(kIcpThreads) void k_icpref_scan(const int* __restrict__ counts, int ncell,
                                                             int* __restrict__ starts)
{
    __shared__ int part[kIcpThreads];
    icpref_scan_body(counts, ncell, starts, part);
}

// consumes counts (each cell's falls to 0)
__global__ __launch_bounds__(256) void k_icpref_scatter(const double2* __restrict__ tq, int m, IcpRefGrid g,
                                                        const int* __restrict__ starts, int* __restrict__ counts,
                                                        double2* __restrict__ cq, int* __restrict__ cidx)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    const double2 q = tq[e];
    const int c = icpref_cell_of(g, q);
    if (c < 0) return;
    const int p = starts[c] + atomicSub(counts + c, 1) - 1;
    if (p < 0 || p >= m) return;
    cq[p] = q;
    cidx[p] = e;
}

// ---- the set's grids: reference i's entries from ebase on in the table and
// cell-order arrays, its counts and starts from cbase on; m entries, ncell cells
struct IcpRefSeg {
    IcpRefGrid g;
    int ebase, cbase, m, ncell;
};

__global__ __launch_bounds__(kIcpRefSetBlock) void k_icpref_count_set(const IcpRefSetBlock* __restrict__ blocks,
                                                                     const IcpRefSeg* __restrict__ segs,
                                                                     const double2* __restrict__ tq,
                                                                     int* __restrict__ counts)
{
    const IcpRefSetBlock b = blocks[blockIdx.x];
    if ((int)threadIdx.x >= b.count) return;
    const IcpRefSeg s = segs[b.ref];
    const int e = b.first + (int)threadIdx.x;
    if (e >= s.m) return;
    const int c = icpref_cell_of(s.g, tq[s.ebase + e]);
    if (c >= 0) atomicAdd(counts + s.cbase + c, 1);
}

__global__ __launch_bounds__(kIcpThreads) void k_icpref_scan_set(const IcpRefSeg* __restrict__ segs,
                                                                 const int* __restrict__ counts,
                                                                 int* __restrict__ starts)
{
    __shared__ int part[kIcpThreads];
    const IcpRefSeg s = segs[blockIdx.x];
    icpref_scan_body(counts + s.cbase, s.ncell, starts + s.cbase, part);
}

// consumes counts; cell indices and cidx are local to the reference
__global__ __launch_bounds__(kIcpRefSetBlock) void k_icpref_scatter_set(const IcpRefSetBlock* __restrict__ blocks,
                                                                       const IcpRefSeg* __restrict__ segs,
                                                                       const double2* __restrict__ tq,
                                                                       const int* __restrict__ starts,
                                                                       int* __restrict__ counts,
                                                                       double2* __restrict__ cq, int* __restrict__ cidx)
{
    const IcpRefSetBlock b = blocks[blockIdx.x];
    if ((int)threadIdx.x >= b.count) return;
    const IcpRefSeg s = segs[b.ref];
    const int e = b.first + (int)threadIdx.x;
    if (e >= s.m) return;
    const double2 q = tq[s.ebase + e];
    const int c = icpref_cell_of(s.g, q);
    if (c < 0) return;
    const int p = starts[s.cbase + c] + atomicSub(counts + s.cbase + c, 1) - 1;
    if (p < 0 || p >= s.m) return;
    cq[s.ebase + p] = q;
    cidx[s.ebase + p] = e;
}

__global__ __launch_bounds__(kIcpThreads) void k_icp_ref(const IcpRefItem* __restrict__ items, IcpShared sh,
                                                         IcpRecord* __restrict__ recs, int* __restrict__ err)
{
    __shared__ IcpStatic L;
    const IcpItem it = items[blockIdx.x].it;
    const IcpRefDev R = items[blockIdx.x].ref;
    icp_refine(it, sh, L, recs + blockIdx.x,
               [&](const double pose[3], int i, double& e, double2& n, double& rc, double& rs) {
                   return icpref_pair(it, R, sh.D2, pose, i, e, n, rc, rs, err);
               });
}

// the search alone at it.spose
__global__ __launch_bounds__(kIcpThreads) void k_icp_ref_pairs(IcpRefItem X, IcpShared sh, int* __restrict__ ref_index,
                                                               int* __restrict__ beam_index,
                                                               double* __restrict__ residual, int* __restrict__ err)
{
    for (int i = threadIdx.x; i < X.it.sn; i += kIcpThreads) {
        double e = 0.0, rc, rs;
        double2 n;
        const int j = icpref_pair(X.it, X.ref, sh.D2, X.it.spose, i, e, n, rc, rs, err);
        const int2 kj = j >= 0 ? gload(X.ref.tkj + j) : make_int2(j, j);
        ref_index[i] = kj.x;
        beam_index[i] = kj.y;
        residual[i] = j >= 0 ? e : 0.0;
    }
}

// ------------------------------------------------------------------ host
void icp_ref_free(lgs_icp_ref* r)
{
    if (!r || r->borrowed) return;
    // hipFree synchronises with the device; the creating context may already
    // be gone, so it is not touched here
    if (r->mem_table || r->mem_cells) {
        hipSetDevice(r->device);
        if (r->mem_table) hipFree(r->mem_table);
        if (r->mem_cells) hipFree(r->mem_cells);
    }
    delete r;
}

struct RefDeleter {
    void operator()(lgs_icp_ref* r) const { icp_ref_free(r); }
};

}  // namespace

const char* const lgs::kSincosMsg = "icp: an angle lies outside the restated sincos domain";

namespace {

lgs_icp_ref* ref_create(lgs_ctx* ctx, const lgs_scan* const* scans, const lgs_pose2d* poses, int K,
                        const lgs_icp_params* p)
{
    // every check before any device work
    LGS_REQUIRE(icp_ref_counts_check(K, nullptr) == LGS_OK, "icp ref: 1 .. 4096 reference scans");
    std::vector<RefScanJob> jobs((size_t)K);
    std::vector<int> usable((size_t)K);
    for (int k = 0; k < K; ++k) {
        LGS_REQUIRE(scans[k], "icp ref: null scan");
        LGS_REQUIRE(scans[k]->n >= 1, "icp ref: empty scan");
        LGS_REQUIRE(icp_pose_finite(poses[k]), "icp ref: pose not finite");
        const lgs_pose2d sp = compound(poses[k], scans[k]->rel);
        LGS_REQUIRE(icp_pose_finite(sp), "icp ref: pose not finite");
        RefScanJob& j = jobs[(size_t)k];
        std::memset(&j, 0, sizeof(j));
        j.pose[0] = sp.x;
        j.pose[1] = sp.y;
        j.pose[2] = sp.theta;
        j.lo = std::max(p->usable_range_min, scans[k]->min_range);
        j.hi = std::min(p->usable_range_max, scans[k]->max_range);
        j.n = scans[k]->n;
        j.label = k;
        usable[(size_t)k] = icp_usable_count(scans[k]->h_ranges.data(), scans[k]->n, j.lo, j.hi);
    }
    LGS_REQUIRE(icp_ref_counts_check(K, usable.data()) == LGS_OK,
                "icp ref: more than LGS_ICP_REF_MAX_ENTRIES usable reference beams");
    int m = 0;
    for (int k = 0; k < K; ++k) {
        jobs[(size_t)k].base = m;
        jobs[(size_t)k].count = usable[(size_t)k];
        m += usable[(size_t)k];
    }

    LGS_HIP_CHECK(hipSetDevice(ctx->device));
    std::unique_ptr<lgs_icp_ref, RefDeleter> ref(new lgs_icp_ref());
    ref->ctx = ctx;
    ref->device = ctx->device;
    ref->bound = icp_ref_bound(p);
    ref->n_refs = K;
    ref->entries = m;
    const size_t mm = (size_t)std::max(m, 1);
    const size_t qb = icp_align256(sizeof(double2) * mm), kb = icp_align256(sizeof(int2) * mm);
    if (hipMalloc(&ref->mem_table, 2 * qb + kb) != hipSuccess) throw Error(LGS_ERR_OOM, "hipMalloc failed for icp ref");
    double2* tq = (double2*)ref->mem_table;
    double2* tn = (double2*)((char*)ref->mem_table + qb);
    int2* tkj = (int2*)((char*)ref->mem_table + 2 * qb);

    // the table, the boxes
    const size_t bb = icp_align256(sizeof(RefScanBox) * (size_t)K);
    double bx[4] = { INFINITY, -INFINITY, INFINITY, -INFINITY };
    if (m > 0) {
        scans_to_device(ctx, scans, K);
        for (int k = 0; k < K; ++k) {
            jobs[(size_t)k].ranges = scans[k]->d_ranges;
            jobs[(size_t)k].angles = scans[k]->d_angles;
        }
        char* small = (char*)ctx->ensure(S_ICP0, bb + 256);
        int* d_err = (int*)(small + bb);
        LGS_HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream));
        Upload up(ctx);
        const size_t jo = up.append(jobs.data(), jobs.size());
        up.flush();
        hipLaunchKernelGGL(k_icpref_table, dim3(K), dim3(kIcpThreads), 0, ctx->stream, up.at<RefScanJob>(jo),
                           p->max_segment_length * p->max_segment_length, tq, tn, tkj, (RefScanBox*)small, d_err);
        LGS_HIP_CHECK(hipGetLastError());
        char* pin = (char*)ctx->ensure_pinned(bb + 256);
        LGS_HIP_CHECK(hipMemcpyAsync(pin, small, bb + 256, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        if (*(const int*)(pin + bb) != 0) throw Error(LGS_ERR_INTERNAL, kSincosMsg);
        const RefScanBox* box = (const RefScanBox*)pin;
        for (int k = 0; k < K; ++k) {
            bx[0] = std::fmin(bx[0], box[k].min_x);
            bx[1] = std::fmax(bx[1], box[k].max_x);
            bx[2] = std::fmin(bx[2], box[k].min_y);
            bx[3] = std::fmax(bx[3], box[k].max_y);
            ref->lines += box[k].lines;
        }
    }

    // the grid
    const IcpRefGrid g = icp_ref_geometry(bx[0], bx[1], bx[2], bx[3], p->max_correspondence_dist);
    const size_t ncell = (size_t)g.x.n * (size_t)g.y.n;
    const size_t ib = icp_align256(sizeof(int) * mm), sb = icp_align256(sizeof(int) * (ncell + 1));
    if (hipMalloc(&ref->mem_cells, qb + ib + sb) != hipSuccess) throw Error(LGS_ERR_OOM, "hipMalloc failed for icp ref");
    double2* cq = (double2*)ref->mem_cells;
    int* cidx = (int*)((char*)ref->mem_cells + qb);
    int* starts = (int*)((char*)ref->mem_cells + qb + ib);
    // (entries without a cell leave the tail of cq / cidx unused: defined bytes all the same)
    LGS_HIP_CHECK(hipMemsetAsync(ref->mem_cells, 0, qb + ib + sb, ctx->stream));
    if (m > 0) {
        int* counts = (int*)ctx->ensure(S_ICPR0, sizeof(int) * ncell);
        LGS_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int) * ncell, ctx->stream));
        const int blocks = (m + 255) / 256;
        hipLaunchKernelGGL(k_icpref_count, dim3(blocks), dim3(256), 0, ctx->stream, tq, m, g, counts);
        LGS_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_icpref_scan, dim3(1), dim3(kIcpThreads), 0, ctx->stream, counts, (int)ncell, starts);
        LGS_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_icpref_scatter, dim3(blocks), dim3(256), 0, ctx->stream, tq, m, g, starts, counts, cq, cidx);
        LGS_HIP_CHECK(hipGetLastError());
    }
    ctx->sync();
    ref->dev = IcpRefDev{ tq, tn, tkj, cq, cidx, starts, g, m };
    return ref.release();
}

}  // namespace

namespace lgs {

// the checks of a refine-time call that need no device (throw LGS_ERR_INVALID_ARG)
void ref_call_check(const lgs_ctx* ctx, const lgs_icp_ref* ref, const lgs_scan* scan, lgs_pose2d pose,
                    const lgs_icp_params* p)
{
    LGS_REQUIRE(ref && scan, "icp ref: null argument");
    LGS_REQUIRE(ref->ctx == ctx, "icp ref: the reference belongs to another context");
    LGS_REQUIRE(icp_ref_bound_same(ref->bound, p),
                "icp ref: usable range, max_segment_length and max_correspondence_dist must be the reference's");
    LGS_REQUIRE(scan->n >= 1, "icp ref: empty scan");
    LGS_REQUIRE(icp_pose_finite(pose), "icp ref: pose not finite");
}

IcpItem ref_item_host(const lgs_scan* scan, lgs_pose2d sensor, const lgs_icp_params* p)
{
    LGS_REQUIRE(icp_pose_finite(sensor), "icp ref: pose not finite");
    IcpItem it;
    std::memset(&it, 0, sizeof(it));
    it.spose[0] = sensor.x;
    it.spose[1] = sensor.y;
    it.spose[2] = sensor.theta;
    it.slo = std::max(p->usable_range_min, scan->min_range);
    it.shi = std::min(p->usable_range_max, scan->max_range);
    it.sn = scan->n;
    return it;
}

void run_icp_ref(lgs_ctx* ctx, const lgs_icp_ref* const* refs, const lgs_scan* const* scans, const lgs_pose2d* init,
                 int n, const lgs_icp_params* p, lgs_icp_summary* out, double* traj)
{
    // every check before any device work
    std::vector<IcpRefItem> items((size_t)n);
    std::vector<lgs_pose2d> sensor((size_t)n);
    for (int j = 0; j < n; ++j) {
        ref_call_check(ctx, refs[j], scans[j], init[j], p);
        sensor[(size_t)j] = compound(init[j], scans[j]->rel);
        items[(size_t)j].it = ref_item_host(scans[j], sensor[(size_t)j], p);
        items[(size_t)j].ref = refs[j]->dev;
    }
    LGS_HIP_CHECK(hipSetDevice(ctx->device));
    scans_to_device(ctx, scans, n);
    const int steps = std::max(1, p->num_iterations_max);
    const size_t rb = icp_align256(sizeof(IcpRecord) * (size_t)n);
    const size_t tb = traj ? icp_align256(sizeof(double) * 5 * (size_t)steps) : 0;
    const size_t hb = rb + tb + 256;
    char* small = (char*)ctx->ensure(S_ICP0, hb);
    IcpRecord* d_rec = (IcpRecord*)small;
    double* d_traj = traj ? (double*)(small + rb) : nullptr;
    int* d_err = (int*)(small + rb + tb);
    LGS_HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream));
    for (int j = 0; j < n; ++j) {
        IcpItem& it = items[(size_t)j].it;
        it.s_ranges = scans[j]->d_ranges;
        it.s_angles = scans[j]->d_angles;
        it.traj = d_traj;   // lone calls only (n == 1)
    }
    Upload up(ctx);
    const size_t io = up.append(items.data(), items.size());
    up.flush();
    const IcpShared sh = icp_shared(p);
    for (int j0 = 0; j0 < n; j0 += kRefChunk) {
        const int m = std::min(kRefChunk, n - j0);
        hipLaunchKernelGGL(k_icp_ref, dim3(m), dim3(kIcpThreads), 0, ctx->stream, up.at<IcpRefItem>(io) + j0, sh,
                           d_rec + j0, d_err);
        LGS_HIP_CHECK(hipGetLastError());
        ctx->icpref_refine_launches += 1;
    }
    char* pin = (char*)ctx->ensure_pinned(hb);
    LGS_HIP_CHECK(hipMemcpyAsync(pin, small, hb, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    if (*(const int*)(pin + rb + tb) != 0) throw Error(LGS_ERR_INTERNAL, kSincosMsg);
    const IcpRecord* rec = (const IcpRecord*)pin;
    for (int j = 0; j < n; ++j)
        icp_summary_of(rec[j], p, init[j], sensor[(size_t)j], scans[j]->rel, scans[j]->n, out[j]);
    if (traj) std::memcpy(traj, pin + rb, sizeof(double) * 5 * (size_t)out[0].iterations);
}

}  // namespace lgs

namespace {

// ------------------------------------------------------------------ the set
void icp_ref_set_free(lgs_icp_ref_set* s)
{
    if (!s) return;
    if (s->mem_table || s->mem_cells) {
        hipSetDevice(s->device);
        if (s->mem_table) hipFree(s->mem_table);
        if (s->mem_cells) hipFree(s->mem_cells);
    }
    delete s;
}

struct RefSetDeleter {
    void operator()(lgs_icp_ref_set* s) const { icp_ref_set_free(s); }
};

lgs_icp_ref_set* ref_set_create(lgs_ctx* ctx, const lgs_scan* const* scans, const lgs_pose2d* poses, int n_scans,
                                const int* idx_min, const int* idx_max, int n_refs, const lgs_icp_params* p)
{
    // every check before any device work
    LGS_REQUIRE(icp_ref_set_ranges_check(n_scans, idx_min, idx_max, n_refs) == LGS_OK,
                "icp ref set: 1 .. 4096 ranges of 1 .. 4096 scans inside [0, n_scans), idx_min <= idx_max");
    // per scan of some range: the job's scan half and the usable beams
    std::vector<char> in_range((size_t)n_scans, 0);
    for (int i = 0; i < n_refs; ++i)
        for (int k = idx_min[i]; k <= idx_max[i]; ++k) in_range[(size_t)k] = 1;
    std::vector<RefScanJob> of_scan((size_t)n_scans);
    std::vector<int> usable((size_t)n_scans, 0);
    std::vector<const lgs_scan*> used;
    for (int k = 0; k < n_scans; ++k) {
        if (!in_range[(size_t)k]) continue;
        LGS_REQUIRE(scans[k], "icp ref set: null scan");
        LGS_REQUIRE(scans[k]->n >= 1, "icp ref set: empty scan");
        LGS_REQUIRE(icp_pose_finite(poses[k]), "icp ref set: pose not finite");
        const lgs_pose2d sp = compound(poses[k], scans[k]->rel);
        LGS_REQUIRE(icp_pose_finite(sp), "icp ref set: pose not finite");
        RefScanJob& j = of_scan[(size_t)k];
        std::memset(&j, 0, sizeof(j));
        j.pose[0] = sp.x;
        j.pose[1] = sp.y;
        j.pose[2] = sp.theta;
        j.lo = std::max(p->usable_range_min, scans[k]->min_range);
        j.hi = std::min(p->usable_range_max, scans[k]->max_range);
        j.n = scans[k]->n;
        usable[(size_t)k] = icp_usable_count(scans[k]->h_ranges.data(), scans[k]->n, j.lo, j.hi);
        used.push_back(scans[k]);
    }
    IcpRefSetLayout L;
    LGS_REQUIRE(icp_ref_set_layout(usable.data(), idx_min, idx_max, n_refs, L) == LGS_OK,
                "icp ref set: more than LGS_ICP_REF_MAX_ENTRIES usable beams in a reference or "
                "LGS_ICP_REF_SET_MAX_ENTRIES in the set");
    // the jobs, reference by reference; a scan without a usable beam writes no
    // entry, has no box and no line and forms no angle, so it needs no job
    std::vector<RefScanJob> jobs;
    std::vector<int> job_ref;
    for (int i = 0; i < n_refs; ++i) {
        int at = L.entry_base[(size_t)i];
        for (int k = idx_min[i]; k <= idx_max[i]; ++k) {
            if (usable[(size_t)k] == 0) continue;
            RefScanJob j = of_scan[(size_t)k];
            j.label = k - idx_min[i];
            j.base = at;
            j.count = usable[(size_t)k];
            at += j.count;
            jobs.push_back(j);
            job_ref.push_back(i);
        }
    }

    const auto t0 = std::chrono::steady_clock::now();
    LGS_HIP_CHECK(hipSetDevice(ctx->device));
    std::unique_ptr<lgs_icp_ref_set, RefSetDeleter> set(new lgs_icp_ref_set());
    set->device = ctx->device;
    set->refs.resize((size_t)n_refs);
    const size_t T = (size_t)L.entry_total;
    const size_t qb = sizeof(double2) * T, kb = sizeof(int2) * T, ib = sizeof(int) * T;   // multiples of 256
    if (hipMalloc(&set->mem_table, 2 * qb + kb) != hipSuccess)
        throw Error(LGS_ERR_OOM, "hipMalloc failed for icp ref set");
    double2* tq = (double2*)set->mem_table;
    double2* tn = (double2*)((char*)set->mem_table + qb);
    int2* tkj = (int2*)((char*)set->mem_table + 2 * qb);
    // (the slots between references are never read: defined bytes all the same)
    LGS_HIP_CHECK(hipMemsetAsync(set->mem_table, 0, 2 * qb + kb, ctx->stream));
    if (!jobs.empty()) ctx->icpset_builds += 1;

    // the table, the boxes: one launch, one wait
    std::vector<IcpRefSetBox> boxes((size_t)n_refs);
    if (!jobs.empty()) {
        scans_to_device(ctx, used.data(), (int)used.size());
        for (size_t j = 0; j < jobs.size(); ++j) {
            const int k = idx_min[job_ref[j]] + jobs[j].label;   // the scan the job was made from
            jobs[j].ranges = scans[k]->d_ranges;
            jobs[j].angles = scans[k]->d_angles;
        }
        const size_t bb = icp_align256(sizeof(RefScanBox) * jobs.size());
        char* small = (char*)ctx->ensure(S_ICP0, bb + 256);
        int* d_err = (int*)(small + bb);
        LGS_HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream));
        Upload up(ctx);
        const size_t jo = up.append(jobs.data(), jobs.size());
        up.flush();
        hipLaunchKernelGGL(k_icpref_table, dim3((unsigned)jobs.size()), dim3(kIcpThreads), 0, ctx->stream,
                           up.at<RefScanJob>(jo), p->max_segment_length * p->max_segment_length, tq, tn, tkj,
                           (RefScanBox*)small, d_err);
        LGS_HIP_CHECK(hipGetLastError());
        ctx->icpset_launches[0] += 1;
        char* pin = (char*)ctx->ensure_pinned(bb + 256);
        LGS_HIP_CHECK(hipMemcpyAsync(pin, small, bb + 256, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        ctx->icpset_syncs += 1;
        if (*(const int*)(pin + bb) != 0) throw Error(LGS_ERR_INTERNAL, kSincosMsg);
        boxes = icp_ref_set_boxes((const RefScanBox*)pin, job_ref.data(), jobs.size(), n_refs);
    }

    const auto t1 = std::chrono::steady_clock::now();

    // the grids
    std::vector<IcpRefGrid> grids((size_t)n_refs);
    for (int i = 0; i < n_refs; ++i) {
        const double* bx = boxes[(size_t)i].bx;
        grids[(size_t)i] = icp_ref_geometry(bx[0], bx[1], bx[2], bx[3], p->max_correspondence_dist);
    }
    IcpRefSetCells Cl;
    if (icp_ref_set_cells(grids, Cl) != LGS_OK)
        throw Error(LGS_ERR_OOM, "icp ref set: more than LGS_ICP_REF_SET_MAX_CELLS grid cells over the set");
    const size_t sb = sizeof(int) * (size_t)Cl.segment_total;
    if (hipMalloc(&set->mem_cells, qb + ib + sb) != hipSuccess)
        throw Error(LGS_ERR_OOM, "hipMalloc failed for icp ref set");
    double2* cq = (double2*)set->mem_cells;
    int* cidx = (int*)((char*)set->mem_cells + qb);
    int* starts = (int*)((char*)set->mem_cells + qb + ib);
    LGS_HIP_CHECK(hipMemsetAsync(set->mem_cells, 0, qb + ib + sb, ctx->stream));
    if (!jobs.empty()) {
        std::vector<IcpRefSeg> segs((size_t)n_refs);
        for (int i = 0; i < n_refs; ++i)
            segs[(size_t)i] = IcpRefSeg{ grids[(size_t)i], L.entry_base[(size_t)i], Cl.cell_base[(size_t)i],
                                         L.entries[(size_t)i], Cl.cells[(size_t)i] };
        const std::vector<IcpRefSetBlock> blocks = icp_ref_set_blocks(L.entries);
        int* counts = (int*)ctx->ensure(S_ICPR0, sb);
        LGS_HIP_CHECK(hipMemsetAsync(counts, 0, sb, ctx->stream));
        Upload up(ctx);
        const size_t so = up.append(segs.data(), segs.size());
        const size_t bo = up.append(blocks.data(), blocks.size());
        up.flush();
        const IcpRefSeg* d_segs = up.at<IcpRefSeg>(so);
        const IcpRefSetBlock* d_blocks = up.at<IcpRefSetBlock>(bo);
        const dim3 bg((unsigned)blocks.size());
        hipLaunchKernelGGL(k_icpref_count_set, bg, dim3(kIcpRefSetBlock), 0, ctx->stream, d_blocks, d_segs, tq, counts);
        LGS_HIP_CHECK(hipGetLastError());
        ctx->icpset_launches[1] += 1;
        hipLaunchKernelGGL(k_icpref_scan_set, dim3((unsigned)n_refs), dim3(kIcpThreads), 0, ctx->stream, d_segs, counts,
                           starts);
        LGS_HIP_CHECK(hipGetLastError());
        ctx->icpset_launches[2] += 1;
        hipLaunchKernelGGL(k_icpref_scatter_set, bg, dim3(kIcpRefSetBlock), 0, ctx->stream, d_blocks, d_segs, tq, starts,
                           counts, cq, cidx);
        LGS_HIP_CHECK(hipGetLastError());
        ctx->icpset_launches[3] += 1;
    }
    ctx->sync();
    ctx->icpset_syncs += 1;
    ctx->icpset_last_ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    ctx->icpset_last_ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    for (int i = 0; i < n_refs; ++i) {
        lgs_icp_ref& r = set->refs[(size_t)i];
        const int eb = L.entry_base[(size_t)i], cb = Cl.cell_base[(size_t)i];
        r.ctx = ctx;
        r.device = ctx->device;
        r.borrowed = true;
        r.bound = icp_ref_bound(p);
        r.n_refs = idx_max[i] - idx_min[i] + 1;
        r.entries = L.entries[(size_t)i];
        r.lines = boxes[(size_t)i].lines;
        r.dev = IcpRefDev{ tq + eb, tn + eb, tkj + eb, cq + eb, cidx + eb, starts + cb, grids[(size_t)i], r.entries };
    }
    return set.release();
}

// lgs_loop_refine_icp: results, refined and summaries are written only when the whole call succeeded
void loop_refine_icp(lgs_ctx* ctx, const lgs_icp_ref* const* refs, const lgs_loop_query* queries, int num_queries,
                     const lgs_loop_candidate* candidates, int num_candidates, const lgs_icp_params* p,
                     const lgs_loop_refine_gate* gate, lgs_loop_result* results, int* refined,
                     lgs_icp_summary* summaries)
{
    // every check before any device work
    std::vector<int> query_of;
    LGS_REQUIRE(loop_refine_ranges_check(queries, num_queries, num_candidates, query_of) == LGS_OK,
                "loop queries must cover the candidates contiguously, in order and completely");
    for (int q = 0; q < num_queries; ++q) LGS_REQUIRE(refs[q], "loop refine: a query without a reference");
    std::vector<int> item_of;
    std::vector<const lgs_icp_ref*> irefs;
    std::vector<const lgs_scan*> iscans;
    std::vector<lgs_pose2d> init;
    for (int c = 0; c < num_candidates; ++c) {
        LGS_REQUIRE(candidates[c].scan, "loop candidate without a scan");
        if (!loop_refine_runs(results[c])) continue;
        item_of.push_back(c);
        irefs.push_back(refs[query_of[(size_t)c]]);
        iscans.push_back(candidates[c].scan);
        init.push_back(results[c].estimated_pose);
    }
    std::vector<lgs_icp_summary> sums(item_of.size());
    if (!item_of.empty())
        run_icp_ref(ctx, irefs.data(), iscans.data(), init.data(), (int)item_of.size(), p, sums.data(), nullptr);
    // nothing can fail from here on
    for (int c = 0; c < num_candidates; ++c) refined[c] = 0;
    if (summaries && num_candidates > 0) std::memset(summaries, 0, sizeof(lgs_icp_summary) * (size_t)num_candidates);
    for (size_t k = 0; k < item_of.size(); ++k) {
        const int c = item_of[k];
        if (summaries) summaries[c] = sums[k];
        if (!loop_refine_accept(*gate, sums[k], results[c].estimated_pose)) continue;
        loop_refine_update(results[c], queries[query_of[(size_t)c]].local_map_node_pose, sums[k]);
        refined[c] = 1;
    }
}

}  // namespace

extern "C" int lgs_icp_ref_set_create(lgs_ctx* ctx, const lgs_scan* const* scans, const lgs_pose2d* poses, int n_scans,
                                      const int* idx_min, const int* idx_max, int n_refs, const lgs_icp_params* params,
                                      lgs_icp_ref_set** out)
{
    if (!ctx || !scans || !poses || !idx_min || !idx_max || !params || !out) return LGS_ERR_INVALID_ARG;
    if (icp_params_check(params) != LGS_OK) return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] { *out = ref_set_create(ctx, scans, poses, n_scans, idx_min, idx_max, n_refs, params); });
}

extern "C" void lgs_icp_ref_set_destroy(lgs_icp_ref_set* set) { icp_ref_set_free(set); }

extern "C" int lgs_icp_ref_set_size(const lgs_icp_ref_set* set) { return set ? (int)set->refs.size() : 0; }

extern "C" const lgs_icp_ref* lgs_icp_ref_set_ref(const lgs_icp_ref_set* set, int i)
{
    if (!set || i < 0 || i >= (int)set->refs.size()) return nullptr;
    return &set->refs[(size_t)i];
}

extern "C" int lgs_icp_ref_set_stats(const lgs_ctx* ctx, long long* builds, long long* table_launches,
                                     long long* count_launches, long long* scan_launches, long long* scatter_launches,
                                     long long* build_syncs, long long* refine_launches)
{
    if (!ctx) return LGS_ERR_INVALID_ARG;
    if (builds) *builds = ctx->icpset_builds;
    if (table_launches) *table_launches = ctx->icpset_launches[0];
    if (count_launches) *count_launches = ctx->icpset_launches[1];
    if (scan_launches) *scan_launches = ctx->icpset_launches[2];
    if (scatter_launches) *scatter_launches = ctx->icpset_launches[3];
    if (build_syncs) *build_syncs = ctx->icpset_syncs;
    if (refine_launches) *refine_launches = ctx->icpref_refine_launches;
    return LGS_OK;
}

extern "C" int lgs_icp_ref_set_last_build_ms(const lgs_ctx* ctx, double* table_ms, double* grids_ms)
{
    if (!ctx) return LGS_ERR_INVALID_ARG;
    if (table_ms) *table_ms = ctx->icpset_last_ms[0];
    if (grids_ms) *grids_ms = ctx->icpset_last_ms[1];
    return LGS_OK;
}

extern "C" int lgs_loop_refine_icp(lgs_ctx* ctx, const lgs_icp_ref* const* refs, const lgs_loop_query* queries,
                                   int num_queries, const lgs_loop_candidate* candidates, int num_candidates,
                                   const lgs_icp_params* params, const lgs_loop_refine_gate* gate,
                                   lgs_loop_result* results, int* refined, lgs_icp_summary* summaries)
{
    if (!ctx || !refs || !queries || !candidates || !params || !gate || !results || !refined)
        return LGS_ERR_INVALID_ARG;
    if (icp_params_check(params) != LGS_OK || loop_refine_gate_check(gate) != LGS_OK) return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        loop_refine_icp(ctx, refs, queries, num_queries, candidates, num_candidates, params, gate, results, refined,
                        summaries);
    });
}

extern "C" int lgs_icp_ref_create(lgs_ctx* ctx, const lgs_scan* const* ref_scans, const lgs_pose2d* ref_poses,
                                  int n_refs, const lgs_icp_params* params, lgs_icp_ref** out)
{
    if (!ctx || !ref_scans || !ref_poses || !params || !out) return LGS_ERR_INVALID_ARG;
    if (icp_params_check(params) != LGS_OK) return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] { *out = ref_create(ctx, ref_scans, ref_poses, n_refs, params); });
}

extern "C" void lgs_icp_ref_destroy(lgs_icp_ref* ref) { icp_ref_free(ref); }

extern "C" int lgs_icp_ref_info(const lgs_icp_ref* ref, int* n_refs, int* entries, int* lines, int* cells_x,
                                int* cells_y, double* cell_size)
{
    if (!ref) return LGS_ERR_INVALID_ARG;
    if (n_refs) *n_refs = ref->n_refs;
    if (entries) *entries = ref->entries;
    if (lines) *lines = ref->lines;
    if (cells_x) *cells_x = ref->dev.g.x.n;
    if (cells_y) *cells_y = ref->dev.g.y.n;
    if (cell_size) *cell_size = ref->dev.g.c;
    return LGS_OK;
}

extern "C" int lgs_icp_ref_optimize_pose_batch(lgs_ctx* ctx, const lgs_icp_ref* const* refs,
                                               const lgs_scan* const* scans, const lgs_pose2d* initial_poses, int n,
                                               const lgs_icp_params* params, lgs_icp_summary* out)
{
    if (!ctx || !refs || !scans || !initial_poses || !params || !out || n < 0) return LGS_ERR_INVALID_ARG;
    if (icp_params_check(params) != LGS_OK) return LGS_ERR_INVALID_ARG;
    if (n == 0) return LGS_OK;
    return guarded(ctx, [&] {
        // a failing call writes nothing: the summaries are formed aside
        std::vector<lgs_icp_summary> tmp((size_t)n);
        run_icp_ref(ctx, refs, scans, initial_poses, n, params, tmp.data(), nullptr);
        std::memcpy(out, tmp.data(), sizeof(lgs_icp_summary) * (size_t)n);
    });
}

extern "C" int lgs_icp_ref_optimize_pose(lgs_ctx* ctx, const lgs_icp_ref* ref, const lgs_scan* scan,
                                         lgs_pose2d initial_pose, const lgs_icp_params* params, lgs_icp_summary* out,
                                         double* trajectory)
{
    if (!ctx || !ref || !scan || !params || !out) return LGS_ERR_INVALID_ARG;
    if (icp_params_check(params) != LGS_OK) return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        lgs_icp_summary tmp;
        std::vector<double> tr(trajectory ? 5 * (size_t)std::max(1, params->num_iterations_max) : 0);
        run_icp_ref(ctx, &ref, &scan, &initial_pose, 1, params, &tmp, trajectory ? tr.data() : nullptr);
        if (trajectory) std::memcpy(trajectory, tr.data(), sizeof(double) * 5 * (size_t)tmp.iterations);
        *out = tmp;
    });
}

extern "C" int lgs_icp_ref_pairs(lgs_ctx* ctx, const lgs_icp_ref* ref, const lgs_scan* scan, lgs_pose2d sensor_pose,
                                 const lgs_icp_params* params, int* ref_index, int* beam_index, double* residual)
{
    if (!ctx || !ref || !scan || !params || !ref_index || !beam_index || !residual) return LGS_ERR_INVALID_ARG;
    if (icp_params_check(params) != LGS_OK) return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        ref_call_check(ctx, ref, scan, sensor_pose, params);
        IcpRefItem X;
        X.it = ref_item_host(scan, sensor_pose, params);
        X.ref = ref->dev;
        LGS_HIP_CHECK(hipSetDevice(ctx->device));
        scans_to_device(ctx, &scan, 1);
        X.it.s_ranges = scan->d_ranges;
        X.it.s_angles = scan->d_angles;
        const size_t ib = icp_align256(sizeof(int) * (size_t)scan->n), eb = icp_align256(sizeof(double) * (size_t)scan->n);
        const size_t hb = eb + 2 * ib + 256;
        char* d = (char*)ctx->ensure(S_ICP1, hb);
        int* d_err = (int*)(d + eb + 2 * ib);
        LGS_HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream));
        hipLaunchKernelGGL(k_icp_ref_pairs, dim3(1), dim3(kIcpThreads), 0, ctx->stream, X, icp_shared(params),
                           (int*)(d + eb), (int*)(d + eb + ib), (double*)d, d_err);
        LGS_HIP_CHECK(hipGetLastError());
        char* pin = (char*)ctx->ensure_pinned(hb);
        LGS_HIP_CHECK(hipMemcpyAsync(pin, d, hb, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        if (*(const int*)(pin + eb + 2 * ib) != 0) throw Error(LGS_ERR_INTERNAL, kSincosMsg);
        std::memcpy(residual, pin, sizeof(double) * (size_t)scan->n);
        std::memcpy(ref_index, pin + eb, sizeof(int) * (size_t)scan->n);
        std::memcpy(beam_index, pin + eb + ib, sizeof(int) * (size_t)scan->n);
    });
}
