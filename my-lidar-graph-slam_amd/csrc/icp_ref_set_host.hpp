// icp_ref_set_host.hpp -- the pieces of lgs_icp_ref_set_create and
// lgs_loop_refine_icp (k_icp_ref.hip) that need no device:
// the range and count checks of a set, where every reference's entries and
// cells start inside the set's two allocations, the flat list of 256-entry
// blocks the grid kernels run over, the per-reference reduction of the table
// pass's boxes, the cell cap, and the gate and record update of the loop
// refinement.  Plain C++ when compiled without HIP, so that
// tests/cpp_icp_ref_set/icp_ref_set_host_check.cpp runs it on its own under
// the sanitizers.
#pragma once

#include <cmath>
#include <cstring>
#include <vector>

#include "icp_ref_host.hpp"
#include "pose_host.hpp"

namespace lgs {

constexpr int kIcpRefSetMaxRefs = 4096;
constexpr long long kIcpRefSetMaxEntries = LGS_ICP_REF_SET_MAX_ENTRIES;
constexpr long long kIcpRefSetMaxCells = LGS_ICP_REF_SET_MAX_CELLS;
constexpr int kIcpRefSetBlock = 256;   // entries per block of the count and scatter launches
// A reference's first entry and first cell are multiples of this: 64 ints are
// 256 bytes, and so is every multiple of 64 of the wider element types
constexpr int kIcpRefSetAlign = 64;

// LGS_OK or LGS_ERR_INVALID_ARG: the rules that need only the numbers
inline int icp_ref_set_ranges_check(int n_scans, const int* idx_min, const int* idx_max, int n_refs)
{
    if (!idx_min || !idx_max || n_scans < 1) return LGS_ERR_INVALID_ARG;
    if (n_refs < 1 || n_refs > kIcpRefSetMaxRefs) return LGS_ERR_INVALID_ARG;
    for (int i = 0; i < n_refs; ++i) {
        if (idx_min[i] < 0 || idx_max[i] >= n_scans || idx_min[i] > idx_max[i]) return LGS_ERR_INVALID_ARG;
        // lgs_icp_ref_create's 1 .. 4096 scans
        if (icp_ref_counts_check(idx_max[i] - idx_min[i] + 1, nullptr) != LGS_OK) return LGS_ERR_INVALID_ARG;
    }
    return LGS_OK;
}

// Where the references lie.  entries[i]: usable beams of reference i (each at
// most LGS_ICP_REF_MAX_ENTRIES); entry_base[i]: its first entry in the set's
// table arrays, a multiple of kIcpRefSetAlign; entry_total: the arrays' length
struct IcpRefSetLayout {
    std::vector<int> entries, entry_base;
    long long usable_total = 0;
    int entry_total = 0;
};

inline long long icp_ref_set_align(long long v)
{
    return (v + (kIcpRefSetAlign - 1)) / kIcpRefSetAlign * kIcpRefSetAlign;
}

// LGS_OK or LGS_ERR_INVALID_ARG.  usable[k]: usable beams of scan k under the
// set's parameters (only scans inside some range are read)
inline int icp_ref_set_layout(const int* usable, const int* idx_min, const int* idx_max, int n_refs,
                              IcpRefSetLayout& L)
{
    L.entries.assign((size_t)n_refs, 0);
    L.entry_base.assign((size_t)n_refs, 0);
    L.usable_total = 0;
    long long base = 0;
    for (int i = 0; i < n_refs; ++i) {
        if (icp_ref_counts_check(idx_max[i] - idx_min[i] + 1, usable + idx_min[i]) != LGS_OK)
            return LGS_ERR_INVALID_ARG;
        long long m = 0;
        for (int k = idx_min[i]; k <= idx_max[i]; ++k) m += usable[k];
        L.usable_total += m;
        if (L.usable_total > kIcpRefSetMaxEntries) return LGS_ERR_INVALID_ARG;
        L.entries[(size_t)i] = (int)m;
        L.entry_base[(size_t)i] = (int)base;
        base += icp_ref_set_align(m > 0 ? m : 1);   // an empty reference still owns one aligned slot
    }
    L.entry_total = (int)base;   // <= 4194304 + 4096 * 64
    return LGS_OK;
}

// one block of the count and scatter launches: `count` entries (1 .. 256) of
// reference `ref` from its entry `first` on
struct IcpRefSetBlock {
    int ref, first, count, pad;
};

// No block straddles two references and none is empty; every entry of every
// reference lies in exactly one block; blocks in (reference, entry) order
inline std::vector<IcpRefSetBlock> icp_ref_set_blocks(const std::vector<int>& entries)
{
    std::vector<IcpRefSetBlock> b;
    for (size_t i = 0; i < entries.size(); ++i)
        for (int first = 0; first < entries[i]; first += kIcpRefSetBlock) {
            const int left = entries[i] - first;
            b.push_back({ (int)i, first, left < kIcpRefSetBlock ? left : kIcpRefSetBlock, 0 });
        }
    return b;
}

// what the table pass reports per (reference, scan) job
struct IcpRefScanBox {
    double min_x, max_x, min_y, max_y;   // over finite points; min > max: none
    int lines, pad;
};

struct IcpRefSetBox {
    double bx[4] = { INFINITY, -INFINITY, INFINITY, -INFINITY };   // lgs_icp_ref_create's reduction, in its order
    int lines = 0;
};

// job_ref[j]: the reference of job j (jobs in reference order, then scan order)
inline std::vector<IcpRefSetBox> icp_ref_set_boxes(const IcpRefScanBox* box, const int* job_ref, size_t n_jobs,
                                                   int n_refs)
{
    std::vector<IcpRefSetBox> out((size_t)n_refs);
    for (size_t j = 0; j < n_jobs; ++j) {
        IcpRefSetBox& r = out[(size_t)job_ref[j]];
        r.bx[0] = std::fmin(r.bx[0], box[j].min_x);
        r.bx[1] = std::fmax(r.bx[1], box[j].max_x);
        r.bx[2] = std::fmin(r.bx[2], box[j].min_y);
        r.bx[3] = std::fmax(r.bx[3], box[j].max_y);
        r.lines += box[j].lines;
    }
    return out;
}

// The cell segments: reference i's starts are cells[i] + 1 ints from
// cell_base[i] (a multiple of kIcpRefSetAlign) on, its counts the first
// cells[i] ints of the same segment of the scratch array.  LGS_OK, or
// LGS_ERR_OOM beyond LGS_ICP_REF_SET_MAX_CELLS cells over the set
struct IcpRefSetCells {
    std::vector<int> cells, cell_base;
    long long cells_total = 0;
    int segment_total = 0;
};

inline int icp_ref_set_cells(const std::vector<IcpRefGrid>& grids, IcpRefSetCells& C)
{
    C.cells.assign(grids.size(), 0);
    C.cell_base.assign(grids.size(), 0);
    C.cells_total = 0;
    long long base = 0;
    for (size_t i = 0; i < grids.size(); ++i) {
        const long long n = (long long)grids[i].x.n * (long long)grids[i].y.n;   // <= 1024 * 1024
        C.cells_total += n;
        if (C.cells_total > kIcpRefSetMaxCells) return LGS_ERR_OOM;
        C.cells[i] = (int)n;
        C.cell_base[i] = (int)base;
        base += icp_ref_set_align(n + 1);
    }
    C.segment_total = (int)base;   // <= 16777216 + 4096 * 128
    return LGS_OK;
}

// ------------------------------------------------------------------ lgs_loop_refine_icp
// LGS_OK or LGS_ERR_INVALID_ARG
inline int loop_refine_gate_check(const lgs_loop_refine_gate* g)
{
    if (!g || g->min_pairs < 3) return LGS_ERR_INVALID_ARG;
    const double v[3] = { g->max_normalized_cost, g->max_translation, g->max_rotation };
    for (double x : v)
        if (!(x >= 0.0)) return LGS_ERR_INVALID_ARG;   // NaN or negative; +inf passes
    return LGS_OK;
}

// The detectors' rule (loop_host.hpp check_loop_batch) without the map: the
// queries cover the candidates contiguously, in order and completely.
// query_of[c]: the query of candidate c
inline int loop_refine_ranges_check(const lgs_loop_query* queries, int num_queries, int num_candidates,
                                    std::vector<int>& query_of)
{
    query_of.clear();
    if (num_queries < 0 || num_candidates < 0 || (num_queries > 0 && !queries)) return LGS_ERR_INVALID_ARG;
    int covered = 0;
    for (int q = 0; q < num_queries; ++q) {
        const lgs_loop_query& Q = queries[q];
        if (Q.first_candidate != covered || Q.num_candidates < 0 || Q.num_candidates > num_candidates - covered)
            return LGS_ERR_INVALID_ARG;
        covered += Q.num_candidates;
        query_of.insert(query_of.end(), (size_t)Q.num_candidates, q);
    }
    return covered == num_candidates ? LGS_OK : LGS_ERR_INVALID_ARG;
}

// whether the record's estimate can start an item at all
inline bool loop_refine_runs(const lgs_loop_result& r) { return r.found != 0 && icp_pose_finite(r.estimated_pose); }

// the gate, comparison by comparison (a NaN fails each)
inline bool loop_refine_accept(const lgs_loop_refine_gate& g, const lgs_icp_summary& s, const lgs_pose2d& recorded)
{
    if (s.pose_found == 0) return false;
    if (!(s.num_pairs >= g.min_pairs)) return false;
    if (!(s.normalized_cost <= g.max_normalized_cost)) return false;
    const double dx = s.estimated_pose.x - recorded.x, dy = s.estimated_pose.y - recorded.y;
    if (!(dx * dx + dy * dy <= g.max_translation * g.max_translation)) return false;
    if (!(std::fabs(normalize_angle(s.estimated_pose.theta - recorded.theta)) <= g.max_rotation)) return false;
    return true;
}

// an accepted record: the estimate, the loop edge, the covariance and the
// cost become the ICP's; every other byte stays
inline void loop_refine_update(lgs_loop_result& r, const lgs_pose2d& local_map_node_pose, const lgs_icp_summary& s)
{
    r.estimated_pose = s.estimated_pose;
    r.relative_pose = inverse_compound(local_map_node_pose, s.estimated_pose);
    std::memcpy(r.covariance, s.covariance, sizeof(r.covariance));
    r.normalized_cost = s.normalized_cost;
}

}  // namespace lgs
