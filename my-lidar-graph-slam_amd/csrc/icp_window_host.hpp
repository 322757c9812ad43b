// icp_window_host.hpp -- the pieces of lgs_icp_ref_window_scores and
// lgs_loop_detect_icp (k_icp_window.hip) that need no device:
// the window's checks, the lattice pose and its index, how the translations
// of one theta are cut into slices and the candidates into chunks, the
// lexicographic minimum over the workgroups' partials, and the loop record.
// The coordinate and the comparison are __host__ __device__: the kernel uses
// them unchanged.  Plain C++ when compiled without HIP, so that
// tests/cpp_icp_window/icp_window_host_check.cpp runs it on its own under the
// sanitizers.
#pragma once

#include <cmath>
#include <cstring>
#include <vector>

#include "icp_ref_set_host.hpp"

namespace lgs {

constexpr int kIcpWinMaxHalf = 512;
constexpr long long kIcpWinMaxPoses = LGS_ICP_WINDOW_MAX_POSES;
constexpr int kIcpWinMaxBeams = LGS_ICP_WINDOW_MAX_BEAMS;
constexpr int kIcpWinSlice = 64;                    // translations of one theta per workgroup, at most
constexpr int kIcpWinSliceMin = 4;                  // ... and at least: one per wave of the workgroup
constexpr int kIcpWinTargetGroups = 2048;           // workgroups a launch should have before slices grow
constexpr long long kIcpWinChunkPoses = 67108864;   // lattice poses per score launch (candidates x P)

// LGS_OK or LGS_ERR_INVALID_ARG: the rules that need only the window
inline int icp_window_check(const lgs_icp_window* w)
{
    if (!w) return LGS_ERR_INVALID_ARG;
    const int h[3] = { w->half_x, w->half_y, w->half_theta };
    for (int v : h)
        if (v < 0 || v > kIcpWinMaxHalf) return LGS_ERR_INVALID_ARG;
    if (!std::isfinite(w->step_xy) || !std::isfinite(w->step_theta)) return LGS_ERR_INVALID_ARG;
    if (!(w->step_xy > 0.0) || !(w->step_theta > 0.0)) return LGS_ERR_INVALID_ARG;
    const long long P = (long long)(2 * w->half_x + 1) * (2 * w->half_y + 1) * (2 * w->half_theta + 1);
    return P > kIcpWinMaxPoses ? LGS_ERR_INVALID_ARG : LGS_OK;
}

struct IcpWinDims {
    int nx, ny, nt;
    int P;   // nx * ny * nt <= LGS_ICP_WINDOW_MAX_POSES (a checked window)
};

inline IcpWinDims icp_window_dims(const lgs_icp_window& w)
{
    IcpWinDims d;
    d.nx = 2 * w.half_x + 1;
    d.ny = 2 * w.half_y + 1;
    d.nt = 2 * w.half_theta + 1;
    d.P = d.nx * d.ny * d.nt;
    return d;
}

// one coordinate of a lattice pose: the product and the sum rounded once each
// (the files that include this are compiled without contraction); the centre
// index gives c itself, -0.0 included
LGS_ICP_HD inline double icp_window_coord(double c, int i, int half, double step)
{
    return i == half ? c : c + (double)(i - half) * step;
}

inline lgs_pose2d icp_window_pose(const lgs_icp_window& w, const lgs_pose2d& c, int ix, int iy, int it)
{
    return { icp_window_coord(c.x, ix, w.half_x, w.step_xy), icp_window_coord(c.y, iy, w.half_y, w.step_xy),
             icp_window_coord(c.theta, it, w.half_theta, w.step_theta) };
}

// p = (it * ny + iy) * nx + ix
inline int icp_window_index(const IcpWinDims& d, int ix, int iy, int it) { return (it * d.ny + iy) * d.nx + ix; }

inline void icp_window_decode(const IcpWinDims& d, int p, int& ix, int& iy, int& it)
{
    ix = p % d.nx;
    iy = (p / d.nx) % d.ny;
    it = p / (d.nx * d.ny);
}

inline lgs_pose2d icp_window_pose_of(const lgs_icp_window& w, const lgs_pose2d& c, int p)
{
    int ix, iy, it;
    icp_window_decode(icp_window_dims(w), p, ix, iy, it);
    return icp_window_pose(w, c, ix, iy, it);
}

// whether every lattice pose around c is finite: the outermost ones are
inline bool icp_window_finite(const lgs_icp_window& w, const lgs_pose2d& c)
{
    const IcpWinDims d = icp_window_dims(w);
    return icp_pose_finite(c) && icp_pose_finite(icp_window_pose(w, c, 0, 0, 0)) &&
           icp_pose_finite(icp_window_pose(w, c, d.nx - 1, d.ny - 1, d.nt - 1));
}

// The launch plan of `cands` candidates (one chunk).  Workgroup b scores slice
// b % slices of theta index (b / slices) % nt of the chunk's candidate
// b / (slices * nt); slice s holds the translations tr = iy * nx + ix in
// [s * slice_len, min(nx * ny, (s + 1) * slice_len)), so every translation lies
// in exactly one slice and no slice is empty.  slice_len is the largest of 64,
// 32, 16, 8 that still gives kIcpWinTargetGroups workgroups, else 4: a long
// slice spreads a workgroup's per-beam sincos over many translations, but a
// lone window must still fill the device.  The scores and the selection do not
// depend on it.  A chunk holds at most chunk_cands candidates: at most
// kIcpWinChunkPoses lattice poses per launch.
struct IcpWinPlan {
    int slice_len;
    int slices;        // per theta index
    int groups;        // workgroups (and partials) per candidate: nt * slices
    int chunk_cands;   // >= 64
};

inline int icp_window_chunk_cands(const IcpWinDims& d)
{
    const long long c = kIcpWinChunkPoses / (long long)d.P;
    return (int)(c < 1 ? 1 : c);
}

inline IcpWinPlan icp_window_plan(const IcpWinDims& d, int cands)
{
    IcpWinPlan pl;
    const int nxy = d.nx * d.ny;
    pl.chunk_cands = icp_window_chunk_cands(d);
    pl.slice_len = kIcpWinSlice;
    for (;;) {
        pl.slices = (nxy + pl.slice_len - 1) / pl.slice_len;
        pl.groups = d.nt * pl.slices;
        if (pl.slice_len <= kIcpWinSliceMin || (long long)cands * pl.groups >= kIcpWinTargetGroups) break;
        pl.slice_len /= 2;
    }
    return pl;
}

inline void icp_window_slice(const IcpWinDims& d, const IcpWinPlan& pl, int s, int& t0, int& t1)
{
    const int nxy = d.nx * d.ny;
    t0 = s * pl.slice_len;
    t1 = t0 + pl.slice_len < nxy ? t0 + pl.slice_len : nxy;
}

// what a workgroup reports: its lexicographic minimum of (cost, p) and the
// pairs there; nothing won: (+inf, -1, 0)
struct IcpWinPartial {
    double cost;
    int p, pairs;
};

// the selection rule; NaN and +inf never win from (+inf, -1)
LGS_ICP_HD inline bool icp_window_better(double cost, int p, double best, int best_p)
{
    return cost < best || (cost == best && p < best_p);
}

inline IcpWinPartial icp_window_none() { return { INFINITY, -1, 0 }; }

// the minimum of n partials (those that hold nothing never win)
inline IcpWinPartial icp_window_combine(const IcpWinPartial* parts, size_t n)
{
    IcpWinPartial b = icp_window_none();
    for (size_t k = 0; k < n; ++k)
        if (parts[k].p >= 0 && icp_window_better(parts[k].cost, parts[k].p, b.cost, b.p)) b = parts[k];
    return b;
}

// Candidate c's record as fill_loop_result (loop_host.hpp) writes one.  s: the
// summary of the refine from the window's best pose, null if none ran;
// accepted: the gate's answer for it; scan_n: NumOfScans()
inline void icp_window_record(lgs_loop_result& r, const lgs_loop_query& Q, const lgs_loop_candidate& c,
                              const lgs_icp_summary* s, bool accepted, int scan_n)
{
    std::memset(&r, 0, sizeof(r));
    r.start_node_index = Q.local_map_node_index;
    r.end_node_index = c.node_index;
    r.start_node_pose = Q.local_map_node_pose;
    if (!s) return;
    r.found = accepted ? 1 : 0;
    r.estimated_pose = s->estimated_pose;
    r.score = (double)s->num_pairs / (double)scan_n;
    r.normalized_cost = s->normalized_cost;
    if (r.found) r.relative_pose = inverse_compound(Q.local_map_node_pose, s->estimated_pose);
    std::memcpy(r.covariance, s->covariance, sizeof(r.covariance));
}

}  // namespace lgs
