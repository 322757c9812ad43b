// icp_device.hpp -- the device code and records that the two point-to-line ICP
// files share: k_icp.hip (one reference scan, its table in LDS, brute force)
// and k_icp_ref.hip (a set of reference scans, the table in global memory
// behind a uniform grid).  Everything that decides a refine's bytes is here
// once: the hit point, the line rule of a table entry, a beam's terms, the
// summation tree, the stopping rule and the solve.  The two files differ only
// in how a beam finds its table entry (the `pair` argument below).
#pragma once

#include "lgs_internal.hpp"
#include "glibc_math.hpp"
#include "icp_host.hpp"
#include "solve3_device.hpp"

#include <cfloat>
#include <cmath>
#include <cstring>

namespace lgs {

constexpr int kIcpThreads = 1024;
constexpr int kIcpWaves = kIcpThreads / 64;
constexpr int kIcpSums = 11;      // cost, pair_cost, H upper triangle (6), b (3)

struct IcpItem {
    const double* r_ranges;
    const double* r_angles;
    const double* s_ranges;
    const double* s_angles;
    double rpose[3];     // Compound(ref pose, ref scan's relPose), glibc on the host
    double rlo, rhi;     // usable range of the reference scan
    double spose[3];     // Compound(initial pose, scan's relPose)
    double slo, shi;
    double* traj;        // lone call: 5 doubles per step (null: none)
    int rn, sn;
};

struct IcpShared {
    double conv, reg_t, reg_r;
    double D2, S2;       // max_correspondence_dist^2, max_segment_length^2 (host products)
    int max_iter;
    int cap;             // k_icp.hip: table entries in LDS, a multiple of its unroll
};

struct IcpRecord {
    double pose[3];
    double sums[kIcpSums];   // the last pass
    double initial_cost;
    int pairs, initial_pairs, iterations, found;
};

struct IcpStatic {
    double wsum[kIcpWaves][kIcpSums + 1];
    int wcnt[kIcpWaves];
    double pose[3];
    int stop;
};

#ifdef __HIPCC__
__device__ __forceinline__ bool icp_dev_usable(double r, double lo, double hi) { return !(r >= hi || r <= lo); }

// ScanData::HitPoint of beam j at `pose`
__device__ __forceinline__ void icp_hit(const double pose[3], double r, double a, double& hx, double& hy, double& rc,
                                        double& rs, int* __restrict__ err)
{
    const double th = pose[2] + a;
    if (!glm::gl_sincos_ok(th) && th - th == 0.0) *err = 1;   // a finite angle outside the restated domain
    double sn, cs;
    glm::gl_sincos(th, &sn, &cs);
    rc = r * cs;
    rs = r * sn;
    hx = pose[0] + rc;
    hy = pose[1] + rs;
}

// Beam j (< rn) of a reference scan at sensor pose `rpose`: whether it is
// usable and, if so, its table entry: the point and the unit normal of its
// line (NaN: no line).
__device__ __forceinline__ bool icp_table_entry(const double* __restrict__ r_ranges, const double* __restrict__ r_angles,
                                                int rn, const double rpose[3], double rlo, double rhi, double S2, int j,
                                                double& qx, double& qy, double& nx, double& ny, int* __restrict__ err)
{
    const double r = gload(r_ranges + j);
    const bool us = icp_dev_usable(r, rlo, rhi);
    if (us) {
        double rc, rs;
        icp_hit(rpose, r, gload(r_angles + j), qx, qy, rc, rs, err);
        // the line: j - 1 first, then j + 1; the smaller l2, a tie to j - 1
        bool have = false;
        double bux = 0.0, buy = 0.0, bl2 = 0.0;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int k = side ? j + 1 : j - 1;
            if (k < 0 || k >= rn) continue;
            const double rk = gload(r_ranges + k);
            if (!icp_dev_usable(rk, rlo, rhi)) continue;
            double kx, ky;
            icp_hit(rpose, rk, gload(r_angles + k), kx, ky, rc, rs, err);
            const double ux = kx - qx, uy = ky - qy;
            const double l2 = ux * ux + uy * uy;
            if (l2 > 0.0 && l2 <= S2 && (!have || l2 < bl2)) {
                have = true;
                bux = ux;
                buy = uy;
                bl2 = l2;
            }
        }
        if (have) {
            const double l = sqrt(bl2);
            nx = (-buy) / l;
            ny = bux / l;
        }
    }
    return us;
}

// One pass at `pose`: thread 0 returns the eleven sums and the pair count.
// pair(pose, i, e, n, rc, rs) is beam i's search: -2 unusable, -1 rejected,
// else its table entry (e, n, rc, rs then valid).  Ends with a barrier behind
// thread 0's reads of L.wsum.
template <class Pair>
__device__ __forceinline__ void icp_pass(const IcpItem& it, const IcpShared& sh, const double pose[3], IcpStatic& L,
                                         double (&out)[kIcpSums], int& out_pairs, Pair pair)
{
    double a[kIcpSums];
#pragma unroll
    for (int k = 0; k < kIcpSums; ++k) a[k] = 0.0;
    int np = 0;
    for (int i = threadIdx.x; i < it.sn; i += kIcpThreads) {
        double e, rc, rs;
        double2 n;
        const int j = pair(pose, i, e, n, rc, rs);
        if (j == -2) continue;
        if (j == -1) {
            a[0] = a[0] + sh.D2;
            continue;
        }
        const double g0 = n.x, g1 = n.y, g2 = n.x * (-rs) + n.y * rc;
        const double ee = e * e, me = -e;
        a[0] = a[0] + ee;
        a[1] = a[1] + ee;
        a[2] = a[2] + g0 * g0;
        a[3] = a[3] + g0 * g1;
        a[4] = a[4] + g0 * g2;
        a[5] = a[5] + g1 * g1;
        a[6] = a[6] + g1 * g2;
        a[7] = a[7] + g2 * g2;
        a[8] = a[8] + me * g0;
        a[9] = a[9] + me * g1;
        a[10] = a[10] + me * g2;
        ++np;
    }
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) {
#pragma unroll
        for (int k = 0; k < kIcpSums; ++k) a[k] = a[k] + __shfl_xor(a[k], mask, 64);
        np += __shfl_xor(np, mask, 64);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kIcpSums; ++k) L.wsum[wid][k] = a[k];
        L.wcnt[wid] = np;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int pairs = L.wcnt[0];
#pragma unroll
        for (int k = 0; k < kIcpSums; ++k) out[k] = L.wsum[0][k];
        for (int w = 1; w < kIcpWaves; ++w) {
#pragma unroll
            for (int k = 0; k < kIcpSums; ++k) out[k] = out[k] + L.wsum[w][k];
            pairs += L.wcnt[w];
        }
        out_pairs = pairs;
    }
    __syncthreads();
}

// The whole refine of one workgroup from it.spose: passes, the stopping rule,
// the solve; thread 0 writes *rec (and it.traj).
template <class Pair>
__device__ __forceinline__ void icp_refine(const IcpItem& it, const IcpShared& sh, IcpStatic& L,
                                           IcpRecord* __restrict__ rec_out, Pair pair)
{
    double pose[3] = { it.spose[0], it.spose[1], it.spose[2] };
    double s[kIcpSums];
    int pairs = 0;
    // thread 0's loop state
    double prevCost = DBL_MAX, initial_cost = 0.0;
    int iterations = 0, found = 1, initial_pairs = 0;
    for (int pass = 0;; ++pass) {
        icp_pass(it, sh, pose, L, s, pairs, pair);
        if (threadIdx.x == 0) {
            int stop = 0;
            if (pass == 0) {
                initial_cost = s[0];
                initial_pairs = pairs;
            } else {
                ++iterations;
                if (it.traj) {
                    double* tr = it.traj + (size_t)(iterations - 1) * 5;
                    tr[0] = pose[0];
                    tr[1] = pose[1];
                    tr[2] = pose[2];
                    tr[3] = s[0];
                    tr[4] = (double)pairs;
                }
            }
            if (pairs < 3) {
                found = 0;
                stop = 1;
            } else if (pass > 0) {
                if (iterations >= sh.max_iter || fabs(prevCost - s[0]) < sh.conv) stop = 1;
                prevCost = s[0];
            }
            if (!stop) {
                const double H[9] = { s[2] + sh.reg_t, s[3], s[4],
                                      s[3], s[5] + sh.reg_t, s[6],
                                      s[4], s[6], s[7] + sh.reg_r };
                const double b[3] = { s[8], s[9], s[10] };
                double d[3];
                solve3_colpiv_qr(H, b, d);
                L.pose[0] = pose[0] + d[0];
                L.pose[1] = pose[1] + d[1];
                L.pose[2] = pose[2] + d[2];
            }
            L.stop = stop;
        }
        __syncthreads();
        if (L.stop) break;
        pose[0] = L.pose[0];
        pose[1] = L.pose[1];
        pose[2] = L.pose[2];
        // (the next pass's first barrier stands between these reads and thread 0's next writes)
    }
    if (threadIdx.x == 0) {
        IcpRecord rec;
        rec.pose[0] = pose[0];
        rec.pose[1] = pose[1];
        rec.pose[2] = pose[2];
#pragma unroll
        for (int k = 0; k < kIcpSums; ++k) rec.sums[k] = s[k];
        rec.initial_cost = initial_cost;
        rec.pairs = pairs;
        rec.initial_pairs = initial_pairs;
        rec.iterations = iterations;
        rec.found = found;
        *rec_out = rec;
    }
}
#endif  // __HIPCC__

// ------------------------------------------------------------------ host
inline size_t icp_align256(size_t b) { return (b + 255) & ~(size_t)255; }

inline IcpShared icp_shared(const lgs_icp_params* p)
{
    IcpShared sh;
    std::memset(&sh, 0, sizeof(sh));
    sh.conv = p->convergence_threshold;
    sh.reg_t = p->translation_regularizer;
    sh.reg_r = p->rotation_regularizer;
    sh.D2 = p->max_correspondence_dist * p->max_correspondence_dist;
    sh.S2 = p->max_segment_length * p->max_segment_length;
    sh.max_iter = p->num_iterations_max;
    return sh;
}

// lgs_icp_summary of one refine's record (sensor = Compound(init, rel))
inline void icp_summary_of(const IcpRecord& r, const lgs_icp_params* p, lgs_pose2d init, lgs_pose2d sensor,
                           lgs_pose2d rel, int scan_n, lgs_icp_summary& o)
{
    std::memset(&o, 0, sizeof(o));
    o.pose_found = r.found;
    o.iterations = r.iterations;
    o.num_pairs = r.pairs;
    o.initial_pairs = r.initial_pairs;
    o.cost = r.sums[0];
    o.pair_cost = r.sums[1];
    o.initial_cost = r.initial_cost;
    o.normalized_cost = o.cost / (double)scan_n;
    o.initial_pose = init;
    o.sensor_pose = sensor;
    o.best_sensor_pose = { r.pose[0], r.pose[1], r.pose[2] };
    o.estimated_pose = move_backward(o.best_sensor_pose, rel);
    const double H[9] = { r.sums[2], r.sums[3], r.sums[4], r.sums[3], r.sums[5], r.sums[6],
                          r.sums[4], r.sums[6], r.sums[7] };
    std::memcpy(o.hessian, H, sizeof(H));
    for (int k = 0; k < 3; ++k) o.rhs[k] = r.sums[8 + k];
    icp_covariance(H, p->translation_regularizer, p->rotation_regularizer, o.pair_cost, o.num_pairs, o.pose_found,
                   o.covariance);
}

}  // namespace lgs
