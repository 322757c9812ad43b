// k_icp.hip -- point-to-line ICP: a scan matched against another scan, the
// nearest-neighbour search and the Gauss-Newton loop on the device.
//
// The reference has no scan-to-scan matcher (SURVEY finding 1), so the
// algorithm is the project's own: DESIGN.md §4.5b states it statement for
// statement, tests/icp_oracle.py restates it, and the two agree byte for byte.
//
// One workgroup of 1024 threads runs one whole refine (table, every pass,
// every solve) without returning to the host; a batch launches one workgroup
// per item.
//   table   every usable beam j of the reference scan, in index order:
//           q_j (ScanData::HitPoint at the reference sensor pose) and the unit
//           normal of its line to the nearer qualifying neighbour j-1 / j+1
//           (NaN: no line).  Dynamic LDS: double2 q[cap] then double2 n[cap],
//           cap = the launch's largest usable count rounded up to 8, the tail
//           filled with NaN points, which never win a strict minimum -- the
//           search loop has no remainder.
//   search  thread t owns beams t, t + 1024, ...; it walks the table in index
//           order, eight entries per trip: every lane of a wave reads the same
//           16-byte entry (an LDS broadcast), the best (d2, j) stays in
//           registers.
//   sums    eleven fp64 sums and the pair count: per thread in beam order
//           from +0.0, six xor-butterfly steps per wave (masks 32 .. 1), the
//           sixteen wave sums added in wave order by thread 0, which then runs
//           the stopping rule and the 3x3 column-pivoting QR solve
//           (solve3_device.hpp) and hands the new pose back through LDS.
// No atomics: a refine's bytes depend on its inputs alone.
// The hit point, the line rule of a table entry, the pass with its tree, the
// stopping rule and the solve live in icp_device.hpp, shared with
// k_icp_ref.hip (a set of reference scans, the table in global memory behind
// a grid); this file keeps the LDS table and the brute-force search.
#include "icp_device.hpp"

#include <vector>

using namespace lgs;

namespace {

constexpr int kIcpUnroll = 8;     // table entries per search trip
constexpr int kIcpChunk = 4096;   // items per launch

// The reference table of one item into LDS; returns the number of entries
// (usable beams, at most cap).  orig (kOrig) receives each entry's beam index.
template <bool kOrig>
__device__ int icp_build_table(const IcpItem& it, double S2, int cap, double2* __restrict__ q,
                               double2* __restrict__ nrm, int* __restrict__ orig, int* __restrict__ wcnt,
                               int* __restrict__ err)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    int base = 0;
    for (int j0 = 0; j0 < it.rn; j0 += kIcpThreads) {
        const int j = j0 + (int)threadIdx.x;
        bool us = false;
        double qx = 0.0, qy = 0.0, nx = nan, ny = nan;
        if (j < it.rn)
            us = icp_table_entry(it.r_ranges, it.r_angles, it.rn, it.rpose, it.rlo, it.rhi, S2, j, qx, qy, nx, ny, err);
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
        if (us && off < cap) {
            q[off] = make_double2(qx, qy);
            nrm[off] = make_double2(nx, ny);
            if (kOrig) orig[off] = j;
        }
        base += total;
        __syncthreads();
    }
    const int m = min(base, cap);
    for (int k = m + (int)threadIdx.x; k < cap; k += kIcpThreads) q[k] = make_double2(nan, nan);
    __syncthreads();
    return m;
}

// the first strict minimum of d2 over the table, in index order; jb = -1 if
// nothing is nearer than +inf (an empty table, NaN everywhere)
__device__ __forceinline__ void icp_search(const double2* __restrict__ q, int m8, double hx, double hy, double& best,
                                           int& jb)
{
    best = __longlong_as_double(0x7ff0000000000000LL);
    jb = -1;
    for (int j = 0; j < m8; j += kIcpUnroll) {
        double2 v[kIcpUnroll];
#pragma unroll
        for (int u = 0; u < kIcpUnroll; ++u) v[u] = q[j + u];
#pragma unroll
        for (int u = 0; u < kIcpUnroll; ++u) {
            const double dx = hx - v[u].x, dy = hy - v[u].y;
            const double d2 = dx * dx + dy * dy;
            const bool lt = d2 < best;
            best = lt ? d2 : best;
            jb = lt ? j + u : jb;
        }
    }
}

// beam i of the current scan at `pose`: -2 unusable, -1 rejected, else the
// table entry it pairs with (e, rc, rs then valid)
__device__ __forceinline__ int icp_pair(const IcpItem& it, double D2, const double pose[3], int i,
                                        const double2* __restrict__ q, const double2* __restrict__ nrm, int m8,
                                        double& e, double2& n, double& rc, double& rs, int* __restrict__ err)
{
    const double r = gload(it.s_ranges + i);
    if (!icp_dev_usable(r, it.slo, it.shi)) return -2;
    double hx, hy;
    icp_hit(pose, r, gload(it.s_angles + i), hx, hy, rc, rs, err);
    double best;
    int jb;
    icp_search(q, m8, hx, hy, best, jb);
    if (jb < 0 || !(best <= D2)) return -1;
    n = nrm[jb];
    if (n.x != n.x) return -1;   // no line
    const double2 p = q[jb];
    const double dx = hx - p.x, dy = hy - p.y;
    e = n.x * dx + n.y * dy;
    return jb;
}

extern __shared__ __attribute__((aligned(16))) unsigned char icp_dyn[];

__global__ __launch_bounds__(kIcpThreads) void k_icp(const IcpItem* __restrict__ items, IcpShared sh,
                                                     IcpRecord* __restrict__ recs, int* __restrict__ err)
{
    __shared__ IcpStatic L;
    const IcpItem it = items[blockIdx.x];
    double2* q = (double2*)icp_dyn;
    double2* nrm = q + sh.cap;
    const int m = icp_build_table<false>(it, sh.S2, sh.cap, q, nrm, nullptr, L.wcnt, err);
    const int m8 = (m + kIcpUnroll - 1) & ~(kIcpUnroll - 1);

    icp_refine(it, sh, L, recs + blockIdx.x,
               [&](const double pose[3], int i, double& e, double2& n, double& rc, double& rs) {
                   return icp_pair(it, sh.D2, pose, i, q, nrm, m8, e, n, rc, rs, err);
               });
}

// the search alone at it.spose: index / residual per beam of the current scan
__global__ __launch_bounds__(kIcpThreads) void k_icp_pairs(IcpItem it, IcpShared sh, int* __restrict__ index,
                                                           double* __restrict__ residual, int* __restrict__ err)
{
    __shared__ IcpStatic L;
    double2* q = (double2*)icp_dyn;
    double2* nrm = q + sh.cap;
    int* orig = (int*)(nrm + sh.cap);
    const int m = icp_build_table<true>(it, sh.S2, sh.cap, q, nrm, orig, L.wcnt, err);
    const int m8 = (m + kIcpUnroll - 1) & ~(kIcpUnroll - 1);
    for (int i = threadIdx.x; i < it.sn; i += kIcpThreads) {
        double e = 0.0, rc, rs;
        double2 n;
        const int j = icp_pair(it, sh.D2, it.spose, i, q, nrm, m8, e, n, rc, rs, err);
        index[i] = j >= 0 ? orig[j] : j;
        residual[i] = j >= 0 ? e : 0.0;
    }
}

// ------------------------------------------------------------------ host
inline size_t align256(size_t b) { return icp_align256(b); }

template <class K>
void icp_allow_lds(K kernel, size_t bytes)
{
    // dynamic LDS beyond the 64 KiB default has to be announced
    if (bytes > 64 * 1024) {
        (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        (void)hipGetLastError();
    }
}

// the item without its device pointers, and the reference's usable count
// (every check that needs no device; throws LGS_ERR_INVALID_ARG)
IcpItem icp_item_host(const lgs_scan* ref, lgs_pose2d ref_sensor, const lgs_scan* scan, lgs_pose2d sensor,
                      const lgs_icp_params* p, int* usable)
{
    LGS_REQUIRE(ref && scan, "icp: null scan");
    LGS_REQUIRE(ref->n >= 1 && scan->n >= 1, "icp: empty scan");
    LGS_REQUIRE(icp_pose_finite(ref_sensor) && icp_pose_finite(sensor), "icp: pose not finite");
    IcpItem it;
    std::memset(&it, 0, sizeof(it));
    it.rpose[0] = ref_sensor.x;
    it.rpose[1] = ref_sensor.y;
    it.rpose[2] = ref_sensor.theta;
    it.rlo = std::max(p->usable_range_min, ref->min_range);
    it.rhi = std::min(p->usable_range_max, ref->max_range);
    it.spose[0] = sensor.x;
    it.spose[1] = sensor.y;
    it.spose[2] = sensor.theta;
    it.slo = std::max(p->usable_range_min, scan->min_range);
    it.shi = std::min(p->usable_range_max, scan->max_range);
    it.rn = ref->n;
    it.sn = scan->n;
    *usable = icp_usable_count(ref->h_ranges.data(), ref->n, it.rlo, it.rhi);
    LGS_REQUIRE(*usable <= kIcpTableCap, "icp: more than 4096 usable reference beams");
    return it;
}

int icp_cap_of(int usable) { return std::max(kIcpUnroll, (usable + kIcpUnroll - 1) & ~(kIcpUnroll - 1)); }

void run_icp(lgs_ctx* ctx, const lgs_scan* const* refs, const lgs_pose2d* ref_poses, const lgs_scan* const* scans,
             const lgs_pose2d* init, int n, const lgs_icp_params* p, lgs_icp_summary* out, double* traj)
{
    // every check before any device work
    std::vector<IcpItem> items((size_t)n);
    std::vector<int> usable((size_t)n);
    std::vector<lgs_pose2d> sensor((size_t)n);
    for (int j = 0; j < n; ++j) {
        LGS_REQUIRE(refs[j] && scans[j], "icp: null scan");
        LGS_REQUIRE(icp_pose_finite(ref_poses[j]) && icp_pose_finite(init[j]), "icp: pose not finite");
        sensor[(size_t)j] = compound(init[j], scans[j]->rel);
        items[(size_t)j] = icp_item_host(refs[j], compound(ref_poses[j], refs[j]->rel), scans[j], sensor[(size_t)j], p,
                                         &usable[(size_t)j]);
    }
    LGS_HIP_CHECK(hipSetDevice(ctx->device));
    std::vector<const lgs_scan*> all((size_t)2 * n);
    for (int j = 0; j < n; ++j) {
        all[(size_t)j] = refs[j];
        all[(size_t)n + j] = scans[j];
    }
    scans_to_device(ctx, all.data(), 2 * n);
    const int steps = std::max(1, p->num_iterations_max);
    const size_t rb = align256(sizeof(IcpRecord) * (size_t)n);
    const size_t tb = traj ? align256(sizeof(double) * 5 * (size_t)steps) : 0;
    const size_t hb = rb + tb + 256;
    char* small = (char*)ctx->ensure(S_ICP0, hb);
    IcpRecord* d_rec = (IcpRecord*)small;
    double* d_traj = traj ? (double*)(small + rb) : nullptr;
    int* d_err = (int*)(small + rb + tb);
    LGS_HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream));
    for (int j = 0; j < n; ++j) {
        IcpItem& it = items[(size_t)j];
        it.r_ranges = refs[j]->d_ranges;
        it.r_angles = refs[j]->d_angles;
        it.s_ranges = scans[j]->d_ranges;
        it.s_angles = scans[j]->d_angles;
        it.traj = d_traj;   // lone calls only (n == 1)
    }
    Upload up(ctx);
    const size_t io = up.append(items.data(), items.size());
    up.flush();
    // one launch per chunk, one workgroup per item
    for (int j0 = 0; j0 < n; j0 += kIcpChunk) {
        const int m = std::min(kIcpChunk, n - j0);
        IcpShared sh = icp_shared(p);
        int cap = kIcpUnroll;
        for (int j = j0; j < j0 + m; ++j) cap = std::max(cap, icp_cap_of(usable[(size_t)j]));
        sh.cap = cap;
        const size_t lds = (size_t)cap * 2 * sizeof(double2);
        icp_allow_lds(k_icp, lds);
        hipLaunchKernelGGL(k_icp, dim3(m), dim3(kIcpThreads), lds, ctx->stream, up.at<IcpItem>(io) + j0, sh, d_rec + j0,
                           d_err);
        LGS_HIP_CHECK(hipGetLastError());
    }
    char* pin = (char*)ctx->ensure_pinned(hb);
    LGS_HIP_CHECK(hipMemcpyAsync(pin, small, hb, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    if (*(const int*)(pin + rb + tb) != 0)
        throw Error(LGS_ERR_INTERNAL, "icp: an angle lies outside the restated sincos domain");
    const IcpRecord* rec = (const IcpRecord*)pin;
    for (int j = 0; j < n; ++j) {
        icp_summary_of(rec[j], p, init[j], sensor[(size_t)j], scans[j]->rel, scans[j]->n, out[j]);
    }
    if (traj) std::memcpy(traj, pin + rb, sizeof(double) * 5 * (size_t)out[0].iterations);
}

}  // namespace

extern "C" size_t lgs_icp_params_size(void) { return sizeof(lgs_icp_params); }
extern "C" size_t lgs_icp_summary_size(void) { return sizeof(lgs_icp_summary); }

extern "C" int lgs_icp_optimize_pose_batch(lgs_ctx* ctx, const lgs_scan* const* ref_scans, const lgs_pose2d* ref_poses,
                                           const lgs_scan* const* scans, const lgs_pose2d* initial_poses, int n,
                                           const lgs_icp_params* params, lgs_icp_summary* out)
{
    if (!ctx || !ref_scans || !ref_poses || !scans || !initial_poses || !params || !out || n < 0)
        return LGS_ERR_INVALID_ARG;
    if (icp_params_check(params) != LGS_OK) return LGS_ERR_INVALID_ARG;
    if (n == 0) return LGS_OK;
    return guarded(ctx, [&] {
        // a failing call writes nothing: the summaries are formed aside
        std::vector<lgs_icp_summary> tmp((size_t)n);
        run_icp(ctx, ref_scans, ref_poses, scans, initial_poses, n, params, tmp.data(), nullptr);
        std::memcpy(out, tmp.data(), sizeof(lgs_icp_summary) * (size_t)n);
    });
}

extern "C" int lgs_icp_optimize_pose(lgs_ctx* ctx, const lgs_scan* ref_scan, lgs_pose2d ref_pose, const lgs_scan* scan,
                                     lgs_pose2d initial_pose, const lgs_icp_params* params, lgs_icp_summary* out,
                                     double* trajectory)
{
    if (!ctx || !ref_scan || !scan || !params || !out) return LGS_ERR_INVALID_ARG;
    if (icp_params_check(params) != LGS_OK) return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        lgs_icp_summary tmp;
        std::vector<double> tr(trajectory ? 5 * (size_t)std::max(1, params->num_iterations_max) : 0);
        run_icp(ctx, &ref_scan, &ref_pose, &scan, &initial_pose, 1, params, &tmp, trajectory ? tr.data() : nullptr);
        if (trajectory) std::memcpy(trajectory, tr.data(), sizeof(double) * 5 * (size_t)tmp.iterations);
        *out = tmp;
    });
}

extern "C" int lgs_icp_pairs(lgs_ctx* ctx, const lgs_scan* ref_scan, lgs_pose2d ref_pose, const lgs_scan* scan,
                             lgs_pose2d sensor_pose, const lgs_icp_params* params, int* index, double* residual)
{
    if (!ctx || !ref_scan || !scan || !params || !index || !residual) return LGS_ERR_INVALID_ARG;
    if (icp_params_check(params) != LGS_OK) return LGS_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        LGS_REQUIRE(icp_pose_finite(ref_pose), "icp: pose not finite");
        int usable = 0;
        IcpItem it = icp_item_host(ref_scan, compound(ref_pose, ref_scan->rel), scan, sensor_pose, params, &usable);
        LGS_HIP_CHECK(hipSetDevice(ctx->device));
        const lgs_scan* both[2] = { ref_scan, scan };
        scans_to_device(ctx, both, 2);
        it.r_ranges = ref_scan->d_ranges;
        it.r_angles = ref_scan->d_angles;
        it.s_ranges = scan->d_ranges;
        it.s_angles = scan->d_angles;
        const size_t ib = align256(sizeof(int) * (size_t)scan->n), eb = align256(sizeof(double) * (size_t)scan->n);
        const size_t hb = eb + ib + 256;
        char* d = (char*)ctx->ensure(S_ICP1, hb);
        int* d_err = (int*)(d + eb + ib);
        LGS_HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream));
        IcpShared sh = icp_shared(params);
        sh.cap = icp_cap_of(usable);
        const size_t lds = (size_t)sh.cap * (2 * sizeof(double2) + sizeof(int));
        icp_allow_lds(k_icp_pairs, lds);
        hipLaunchKernelGGL(k_icp_pairs, dim3(1), dim3(kIcpThreads), lds, ctx->stream, it, sh, (int*)(d + eb), (double*)d,
                           d_err);
        LGS_HIP_CHECK(hipGetLastError());
        char* pin = (char*)ctx->ensure_pinned(hb);
        LGS_HIP_CHECK(hipMemcpyAsync(pin, d, hb, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        if (*(const int*)(pin + eb + ib) != 0)
            throw Error(LGS_ERR_INTERNAL, "icp: an angle lies outside the restated sincos domain");
        std::memcpy(residual, pin, sizeof(double) * (size_t)scan->n);
        std::memcpy(index, pin + eb, sizeof(int) * (size_t)scan->n);
    });
}
