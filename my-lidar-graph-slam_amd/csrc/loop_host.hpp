// loop_host.hpp -- the batch contract of the loop detectors (correlative, its
// multi-context form, branch-and-bound, grid search), stated once: which
// (queries, candidates) batches are accepted, and how a matcher's summary
// becomes a candidate's lgs_loop_result.  Free of the HIP runtime; maps and
// scans are opaque here and never dereferenced.
#pragma once

#include <cstring>
#include <string>
#include <vector>

#include "lgs_error.hpp"
#include "lgs_hip.h"
#include "pose_host.hpp"

namespace lgs {

// The rules every detector shares: the threshold is in (0, 1] (the reference
// asserts it at `cite`, a line citation of that detector's source), every
// query has a map, the queries cover the candidates contiguously and in order,
// every candidate has a scan, and every candidate is covered.  Returns the
// query index of every candidate.  What only one matcher requires (its map
// caps, non-empty scans) it checks itself, after this.
inline std::vector<int> check_loop_batch(double score_threshold, const lgs_loop_query* queries, int num_queries,
                                         const lgs_loop_candidate* candidates, int num_candidates, const char* cite)
{
    LGS_REQUIRE(score_threshold > 0.0 && score_threshold <= 1.0,
                std::string("score threshold must be in (0, 1] (") + cite + ")");
    std::vector<int> query_of;
    int covered = 0;
    for (int q = 0; q < num_queries; ++q) {
        const lgs_loop_query& Q = queries[q];
        LGS_REQUIRE(Q.map, "loop query without a local map");
        LGS_REQUIRE(Q.first_candidate == covered && Q.num_candidates >= 0 &&
                        Q.num_candidates <= num_candidates - covered,
                    "loop queries must cover the candidates contiguously and in order");
        covered += Q.num_candidates;
        for (int j = 0; j < Q.num_candidates; ++j) {
            LGS_REQUIRE(candidates[Q.first_candidate + j].scan, "loop candidate without a scan");
            query_of.push_back(q);
        }
    }
    LGS_REQUIRE(covered == num_candidates, "loop queries must cover every candidate");
    return query_of;
}

// FindCorrespondingPose's result for one candidate: found == 0 where the
// reference appends none, and then relative_pose -- like the padding -- is
// zero bytes; found: the loop edge InverseCompound(localMapNode.Pose(), estimatedPose).
inline void fill_loop_result(lgs_loop_result& r, const lgs_loop_query& Q, const lgs_loop_candidate& c,
                             const lgs_rtcsm_summary& s)
{
    std::memset(&r, 0, sizeof(r));
    r.found = s.pose_found;
    r.start_node_index = Q.local_map_node_index;
    r.end_node_index = c.node_index;
    r.start_node_pose = Q.local_map_node_pose;
    r.estimated_pose = s.estimated_pose;
    r.score = s.score_max;
    r.normalized_cost = s.normalized_cost;
    if (s.pose_found) r.relative_pose = inverse_compound(Q.local_map_node_pose, s.estimated_pose);
    std::memcpy(r.covariance, s.covariance, sizeof(r.covariance));
}

}  // namespace lgs
