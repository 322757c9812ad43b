// icp_ref_device.hpp -- what the files that search an lgs_icp_ref share:
// k_icp_ref.hip (build, refine, pairs) and k_icp_window.hip (the window search
// of start poses).  The reference as the kernels read it, the
// handle, the grid search that returns the brute-force answer
// and a beam's pairing are here once, so that a score of the window search and
// a pass of the refine cannot differ in a byte; and the refine-time host code
// of k_icp_ref.hip that the window search runs its refines through.
#pragma once

#include "icp_device.hpp"
#include "icp_ref_host.hpp"

namespace lgs {

constexpr int kRefWalk = 4;       // cell entries in flight per search trip

// what the kernels read of a reference
struct IcpRefDev {
    const double2* tq;     // table order: points
    const double2* tn;     //              normals (NaN: no line)
    const int2* tkj;       //              (reference scan, beam)
    const double2* cq;     // cell order: points
    const int* cidx;       //             their table indices
    const int* starts;     // [cells + 1], row-major cells
    IcpRefGrid g;
    int m;
};

}  // namespace lgs

struct lgs_icp_ref {
    lgs_ctx* ctx = nullptr;   // creating context (compared, never used after its destruction)
    int device = 0;
    bool borrowed = false;    // a member of an lgs_icp_ref_set: the set owns the memory, destroy is a no-op
    lgs::IcpRefBound bound{};
    int n_refs = 0, entries = 0, lines = 0;
    void* mem_table = nullptr;   // tq, tn, tkj
    void* mem_cells = nullptr;   // cq, cidx, starts
    lgs::IcpRefDev dev{};
};

namespace lgs {

#ifdef __HIPCC__
// the lexicographic minimum of (d2, index) over the cells a hit point visits;
// jb = -1 if nothing there is nearer than +inf
__device__ __forceinline__ void icpref_search(const IcpRefDev& R, double hx, double hy, double& best, int& jb)
{
    best = __longlong_as_double(0x7ff0000000000000LL);
    jb = -1;
    int x0, x1, y0, y1;
    if (!icp_ref_visit(R.g, hx, hy, x0, x1, y0, y1)) return;
    for (int y = y0; y <= y1; ++y) {
        const int row = y * R.g.x.n;
        const int p0 = gload(R.starts + row + x0), p1 = gload(R.starts + row + x1 + 1);
        for (int p = p0; p < p1; p += kRefWalk) {
            double2 v[kRefWalk];
            int id[kRefWalk];
            // past the range's end the last entry again: it never beats itself
#pragma unroll
            for (int u = 0; u < kRefWalk; ++u) {
                const int pu = min(p + u, p1 - 1);
                v[u] = gload(R.cq + pu);
                id[u] = gload(R.cidx + pu);
            }
#pragma unroll
            for (int u = 0; u < kRefWalk; ++u) {
                const double dx = hx - v[u].x, dy = hy - v[u].y;
                const double d2 = dx * dx + dy * dy;
                const bool lt = d2 < best || (d2 == best && id[u] < jb);
                best = lt ? d2 : best;
                jb = lt ? id[u] : jb;
            }
        }
    }
}

// beam i of the current scan at `pose`: -2 unusable, -1 rejected, else the
// table entry it pairs with (e, n, rc, rs then valid)
__device__ __forceinline__ int icpref_pair(const IcpItem& it, const IcpRefDev& R, double D2, const double pose[3], int i,
                                           double& e, double2& n, double& rc, double& rs, int* __restrict__ err)
{
    const double r = gload(it.s_ranges + i);
    if (!icp_dev_usable(r, it.slo, it.shi)) return -2;
    double hx, hy;
    icp_hit(pose, r, gload(it.s_angles + i), hx, hy, rc, rs, err);
    double best;
    int jb;
    icpref_search(R, hx, hy, best, jb);
    if (jb < 0 || !(best <= D2)) return -1;
    n = gload(R.tn + jb);
    if (n.x != n.x) return -1;   // no line
    const double2 p = gload(R.tq + jb);
    const double dx = hx - p.x, dy = hy - p.y;
    e = n.x * dx + n.y * dy;
    return jb;
}
#endif  // __HIPCC__

// ------------------------------------------------------------------ host (k_icp_ref.hip)
extern const char* const kSincosMsg;

// the checks of a refine-time call that need no device (throw LGS_ERR_INVALID_ARG)
void ref_call_check(const lgs_ctx* ctx, const lgs_icp_ref* ref, const lgs_scan* scan, lgs_pose2d pose,
                    const lgs_icp_params* p);

// n refines as one batch, the code behind lgs_icp_ref_optimize_pose_batch:
// item j is scans[j] from init[j] against refs[j]; one wait on the stream
void run_icp_ref(lgs_ctx* ctx, const lgs_icp_ref* const* refs, const lgs_scan* const* scans, const lgs_pose2d* init,
                 int n, const lgs_icp_params* p, lgs_icp_summary* out, double* traj);

}  // namespace lgs
