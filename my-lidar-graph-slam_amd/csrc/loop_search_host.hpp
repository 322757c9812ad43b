// loop_search_host.hpp -- the nearest-node loop searcher (DESIGN.md 4.6g,
// LoopSearcherNearest::Search, C/mapping/loop_searcher_nearest.cpp:13-108)
// as far as it needs no device: validation, the walk and its travel chain, the
// partition of the walk into groups of whole maps, the candidate node range
// and the reference's loop, statement for statement.  Plain C++ over
// lgs_hip.h's structs: k_loop_search.hip shares all of it with
// lgs_loop_search_nearest_host, and tests/cpp_loop_search/ compiles it on its
// own under the sanitizers.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "lgs_hip.h"

namespace lgs {

constexpr long long kLoopSearchMaxSize = 1LL << 27;   // nodes, maps, walk positions, hints

// the none entry of a result record or a per-map row
inline lgs_loop_search_result loop_search_none(int walked, double node_dist_min_sq)
{
    lgs_loop_search_result r;
    std::memset(&r, 0, sizeof(r));
    r.found = 0;
    r.local_map_idx = r.local_map_node_idx = r.node_idx_min = r.node_idx_max = -1;
    r.walked = walked;
    r.dist_sq = node_dist_min_sq;
    return r;
}
inline lgs_loop_search_map_best loop_search_map_none(double node_dist_min_sq)
{
    lgs_loop_search_map_best b;
    std::memset(&b, 0, sizeof(b));
    b.node_idx = -1;
    b.dist_sq = node_dist_min_sq;
    return b;
}

// nodeDistMinSq's initial value (:33)
inline double loop_search_min_sq(const lgs_loop_search_params* p) { return std::pow(p->node_dist_threshold, 2.0); }

// LGS_OK or LGS_ERR_INVALID_ARG: the snapshot's rules.  *positions: the walk's length
inline int loop_search_check_graph(const lgs_pose2d* poses, int n, const int* idx_min, const int* idx_max, int m,
                                   long long* positions)
{
    if (!poses || !idx_min || !idx_max) return LGS_ERR_INVALID_ARG;
    if (n < 1 || m < 1 || n > kLoopSearchMaxSize || m > kLoopSearchMaxSize) return LGS_ERR_INVALID_ARG;
    long long total = 0;
    for (int i = 0; i < m; ++i) {
        if (idx_min[i] < 0 || idx_max[i] >= n || idx_min[i] > idx_max[i]) return LGS_ERR_INVALID_ARG;
        if (i < m - 1) total += (long long)idx_max[i] - idx_min[i] + 1;
        if (total > kLoopSearchMaxSize) return LGS_ERR_INVALID_ARG;
    }
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(poses[k].x) || !std::isfinite(poses[k].y)) return LGS_ERR_INVALID_ARG;
    if (positions) *positions = total;
    return LGS_OK;
}

inline int loop_search_check_params(const lgs_loop_search_params* p)
{
    if (!p) return LGS_ERR_INVALID_ARG;
    if (!std::isfinite(p->travel_dist_threshold) || !std::isfinite(p->node_dist_threshold)) return LGS_ERR_INVALID_ARG;
    if (p->num_candidate_nodes < 0) return LGS_ERR_INVALID_ARG;
    return LGS_OK;
}

// one hint against a snapshot of n nodes and m maps (GetLoopSearchHint's
// assertion, C/mapping/lidar_graph_slam.cpp:142-143, included)
inline int loop_search_check_hint(const lgs_loop_search_hint& h, int n, const int* idx_min, const int* idx_max, int m)
{
    if (h.num_maps < 1 || h.num_maps > m) return LGS_ERR_INVALID_ARG;
    if (h.latest_local_map_idx < 0 || h.latest_local_map_idx >= h.num_maps) return LGS_ERR_INVALID_ARG;
    if (h.latest_node_idx < 0 || h.latest_node_idx >= n) return LGS_ERR_INVALID_ARG;
    if (h.latest_node_idx < idx_min[h.latest_local_map_idx] || h.latest_node_idx > idx_max[h.latest_local_map_idx])
        return LGS_ERR_INVALID_ARG;
    if (!std::isfinite(h.accum_travel_dist)) return LGS_ERR_INVALID_ARG;
    return LGS_OK;
}

inline int loop_search_check_hints(const lgs_loop_search_hint* hints, long long q, int n, const int* idx_min,
                                   const int* idx_max, int m)
{
    if (q < 0 || q > kLoopSearchMaxSize || (q > 0 && !hints)) return LGS_ERR_INVALID_ARG;
    for (long long j = 0; j < q; ++j)
        if (loop_search_check_hint(hints[j], n, idx_min, idx_max, m) != LGS_OK) return LGS_ERR_INVALID_ARG;
    return LGS_OK;
}

// The walk of a checked snapshot: positions (map i, node k), i = 0 .. m - 2,
// k = idx_min[i] .. idx_max[i]; map_start[i] = map i's first position, i < m
// (map_start[m - 1] = the walk's length); travel[p] = nodeTravelDist after
// position p (:40-41, :59-60).
struct LoopWalk {
    std::vector<double> x, y, travel;
    std::vector<int> map_start;
    int positions = 0;
};
inline LoopWalk loop_walk_build(const lgs_pose2d* poses, const int* idx_min, const int* idx_max, int m)
{
    LoopWalk w;
    w.map_start.resize((size_t)m);
    long long total = 0;
    for (int i = 0; i < m; ++i) {
        w.map_start[(size_t)i] = (int)total;
        if (i < m - 1) total += (long long)idx_max[i] - idx_min[i] + 1;
    }
    w.positions = (int)total;
    w.x.resize((size_t)total);
    w.y.resize((size_t)total);
    w.travel.resize((size_t)total);
    double t = 0.0;
    lgs_pose2d prev = poses[0];
    size_t p = 0;
    for (int i = 0; i < m - 1; ++i)
        for (int k = idx_min[i]; k <= idx_max[i]; ++k, ++p) {
            t += std::hypot(prev.x - poses[k].x, prev.y - poses[k].y);
            prev = poses[k];
            w.x[p] = poses[k].x;
            w.y[p] = poses[k].y;
            w.travel[p] = t;
        }
    return w;
}

// The walk's maps 0 .. m - 2 cut into groups of whole consecutive maps of
// about `target` positions: a map joins the open group unless that would
// take the group past `target` (a group always takes its first map, however
// large).  Returns first[g], g <= G: group g is the maps first[g] ..
// first[g + 1] - 1; G = 0 for an empty walk.
inline std::vector<int> loop_group_partition(const std::vector<int>& map_start, int target)
{
    const int walked = (int)map_start.size() - 1;   // maps in the walk
    std::vector<int> first;
    if (walked < 1) {
        first.push_back(0);
        return first;
    }
    const long long tgt = std::max(1, target);
    first.push_back(0);
    long long count = 0;
    for (int i = 0; i < walked; ++i) {
        const long long len = (long long)map_start[(size_t)i + 1] - map_start[(size_t)i];
        if (count > 0 && count + len > tgt) {
            first.push_back(i);
            count = 0;
        }
        count += len;
    }
    first.push_back(walked);
    return first;
}

// nodeIdxMin / nodeIdxMax of the candidate (:93-98); 64-bit, so that
// latest + K cannot wrap
inline void loop_node_range(int latest, int map_min, int map_max, int K, int* lo, int* hi)
{
    *lo = (int)std::max<long long>(map_min, (long long)latest - K);
    *hi = (int)std::min<long long>(map_max, (long long)latest + K);
}

// The reference's loop for one checked hint, statement for statement
// (:26-108).  travel: null, or the snapshot's chain (LoopWalk::travel), whose
// entries are the values the loop's own chain takes.  row: null, or the
// hint's m per-map entries.
inline void loop_search_statement(const lgs_pose2d* poses, const int* idx_min, const int* idx_max, int m,
                                  const lgs_loop_search_params* prm, const lgs_loop_search_hint& hint,
                                  const double* travel, lgs_loop_search_result* out, lgs_loop_search_map_best* row)
{
    const int numOfMaps = hint.num_maps;
    const int latestNodeIdx = hint.latest_node_idx;
    const lgs_pose2d robotPose = poses[latestNodeIdx];
    const double minSq0 = loop_search_min_sq(prm);
    double nodeDistMinSq = minSq0;
    int candidateMapIdx = -1, candidateNodeIdx = -1;
    const double accumTravelDist = hint.accum_travel_dist;
    double nodeTravelDist = 0.0;
    lgs_pose2d prevPose = poses[0];
    int walked = 0;
    if (row)
        for (int i = 0; i < m; ++i) row[i] = loop_search_map_none(minSq0);

    for (int mapIdx = 0; mapIdx < numOfMaps - 1; ++mapIdx) {
        double mapMinSq = minSq0;
        for (int nodeIdx = idx_min[mapIdx]; nodeIdx <= idx_max[mapIdx]; ++nodeIdx) {
            const lgs_pose2d nodePose = poses[nodeIdx];
            if (travel) {
                nodeTravelDist = travel[walked];
            } else {
                nodeTravelDist += std::hypot(prevPose.x - nodePose.x, prevPose.y - nodePose.y);
                prevPose = nodePose;
            }
            if (accumTravelDist - nodeTravelDist < prm->travel_dist_threshold) goto Done;
            ++walked;
            const double nodeDistSq = (nodePose.x - robotPose.x) * (nodePose.x - robotPose.x) +
                                      (nodePose.y - robotPose.y) * (nodePose.y - robotPose.y);
            if (nodeDistSq < nodeDistMinSq) {
                nodeDistMinSq = nodeDistSq;
                candidateMapIdx = mapIdx;
                candidateNodeIdx = nodeIdx;
            }
            if (row && nodeDistSq < mapMinSq) {
                mapMinSq = nodeDistSq;
                row[mapIdx].node_idx = nodeIdx;
                row[mapIdx].dist_sq = nodeDistSq;
            }
        }
    }
Done:
    *out = loop_search_none(walked, minSq0);
    if (candidateMapIdx < 0) return;
    out->found = 1;
    out->local_map_idx = candidateMapIdx;
    out->local_map_node_idx = candidateNodeIdx;
    loop_node_range(latestNodeIdx, idx_min[hint.latest_local_map_idx], idx_max[hint.latest_local_map_idx],
                    prm->num_candidate_nodes, &out->node_idx_min, &out->node_idx_max);
    out->dist_sq = nodeDistMinSq;
}

// GridMapBuilder::UpdateAccumTravelDist (C/mapping/grid_map_builder.cpp:210-224)
inline double loop_accum_travel_dist(const lgs_pose2d* poses, int n)
{
    double t = 0.0;
    for (int i = 1; i < n; ++i) t += std::hypot(poses[i - 1].x - poses[i].x, poses[i - 1].y - poses[i].y);
    return t;
}

// every check of a search that needs no device, then the loop per hint
inline int loop_search_host(const lgs_pose2d* poses, int n, const int* idx_min, const int* idx_max, int m,
                            const lgs_loop_search_params* prm, const lgs_loop_search_hint* hints, long long q,
                            lgs_loop_search_result* results, lgs_loop_search_map_best* per_map)
{
    if (loop_search_check_graph(poses, n, idx_min, idx_max, m, nullptr) != LGS_OK) return LGS_ERR_INVALID_ARG;
    if (loop_search_check_params(prm) != LGS_OK) return LGS_ERR_INVALID_ARG;
    if (loop_search_check_hints(hints, q, n, idx_min, idx_max, m) != LGS_OK) return LGS_ERR_INVALID_ARG;
    if (q > 0 && !results) return LGS_ERR_INVALID_ARG;
    for (long long j = 0; j < q; ++j)
        loop_search_statement(poses, idx_min, idx_max, m, prm, hints[j], nullptr, results + j,
                              per_map ? per_map + j * (long long)m : nullptr);
    return LGS_OK;
}

}  // namespace lgs
