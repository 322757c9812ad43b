// loop_search_host_check.cpp -- the host-only code of the nearest-node loop
// searcher (my-lidar-graph-slam_amd/csrc/loop_search_host.hpp) in a program of
// its own, built with -fsanitize=address,undefined: the walk builder, the group
// partition (every position in exactly one group, groups end at map
// boundaries), validation, and the loop with the snapshot's travel chain
// against the loop with its own, all against brute force.  Prints one line per
// check; exit status 1 if any check fails.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "loop_search_host.hpp"

namespace {

int g_failed = 0;

void check(bool ok, const std::string& name, const std::string& detail = "")
{
    std::printf("[%s] %s%s%s\n", ok ? " OK " : "FAIL", name.c_str(), detail.empty() ? "" : ": ", detail.c_str());
    if (!ok) ++g_failed;
}

struct Rng {
    uint64_t s;
    double uni()   // [0, 1)
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) * 0x1p-53;
    }
    int below(int n) { return (int)(uni() * n); }
};

struct Snapshot {
    std::vector<lgs_pose2d> poses;
    std::vector<int> lo, hi;
};

// ranges that may overlap, repeat and leave gaps
Snapshot random_snapshot(Rng& r, int n, int m)
{
    Snapshot s;
    s.poses.resize((size_t)n);
    for (int k = 0; k < n; ++k) s.poses[(size_t)k] = { 4.0 * std::sin(0.13 * k) + r.uni(), 3.0 * std::sin(0.29 * k), r.uni() };
    for (int i = 0; i < m; ++i) {
        const int a = r.below(n), len = 1 + r.below(i % 5 == 0 ? 90 : 12);
        s.lo.push_back(a);
        s.hi.push_back(std::min(n - 1, a + len - 1));
    }
    return s;
}

void walk_and_partition()
{
    using namespace lgs;
    Rng r{ 7 };
    bool walk_ok = true, part_ok = true, single_big = false;
    long long groups_seen = 0;
    for (int rep = 0; rep < 60; ++rep) {
        const int n = 1 + r.below(300), m = 1 + r.below(40);
        const Snapshot s = random_snapshot(r, n, m);
        long long positions = -1;
        walk_ok = walk_ok && loop_search_check_graph(s.poses.data(), n, s.lo.data(), s.hi.data(), m, &positions) == LGS_OK;
        const LoopWalk w = loop_walk_build(s.poses.data(), s.lo.data(), s.hi.data(), m);
        // brute force: the list of (map, node), the chain restarted from scratch
        std::vector<int> node_of;
        for (int i = 0; i < m - 1; ++i) {
            walk_ok = walk_ok && w.map_start[(size_t)i] == (int)node_of.size();
            for (int k = s.lo[(size_t)i]; k <= s.hi[(size_t)i]; ++k) node_of.push_back(k);
        }
        walk_ok = walk_ok && w.map_start[(size_t)m - 1] == (int)node_of.size() && w.positions == (int)node_of.size() &&
                  positions == w.positions && w.x.size() == node_of.size() && w.travel.size() == node_of.size();
        double t = 0.0;
        lgs_pose2d prev = s.poses[0];
        for (size_t p = 0; p < node_of.size() && walk_ok; ++p) {
            const lgs_pose2d q = s.poses[(size_t)node_of[p]];
            t += std::hypot(prev.x - q.x, prev.y - q.y);
            prev = q;
            walk_ok = std::memcmp(&w.x[p], &q.x, 8) == 0 && std::memcmp(&w.y[p], &q.y, 8) == 0 &&
                      std::memcmp(&w.travel[p], &t, 8) == 0 && (p == 0 || w.travel[p] >= w.travel[p - 1]);
        }
        for (int target : { 1, 7, 64, 100000 }) {
            const std::vector<int> first = loop_group_partition(w.map_start, target);
            const int G = (int)first.size() - 1;
            groups_seen += G;
            part_ok = part_ok && first.front() == 0 && (m == 1 ? G == 0 : (G >= 1 && first.back() == m - 1));
            std::vector<int> owner((size_t)w.positions, 0);
            for (int g = 0; g < G; ++g) {
                part_ok = part_ok && first[(size_t)g] < first[(size_t)g + 1];   // whole maps, at least one
                const int a = w.map_start[(size_t)first[(size_t)g]], b = w.map_start[(size_t)first[(size_t)g + 1]];
                for (int p = a; p < b; ++p) owner[(size_t)p] += 1;
                // above the target only as one single map
                if (b - a > target) {
                    part_ok = part_ok && first[(size_t)g + 1] - first[(size_t)g] == 1;
                    single_big = true;
                }
                // a group is closed only when the next map would not fit
                if (g + 1 < G) {
                    const int next = w.map_start[(size_t)first[(size_t)g + 1] + 1] - b;
                    part_ok = part_ok && (b - a) + next > target;
                }
            }
            for (int c : owner) part_ok = part_ok && c == 1;
        }
    }
    check(walk_ok, "walk builder == brute force over 60 random snapshots", "positions, map_start, x / y, travel bit for bit");
    check(part_ok && single_big && groups_seen > 0, "group partition: every position in exactly one group, whole maps",
          std::to_string(groups_seen) + " groups, targets 1, 7, 64, 100000; a map above the target stands alone");
}

void statement_with_and_without_chain()
{
    using namespace lgs;
    Rng r{ 11 };
    bool ok = true, invariant = true;
    long long found = 0, total = 0;
    for (int rep = 0; rep < 30; ++rep) {
        const int n = 20 + r.below(200), m = 2 + r.below(12);
        Snapshot s = random_snapshot(r, n, m);
        const LoopWalk w = loop_walk_build(s.poses.data(), s.lo.data(), s.hi.data(), m);
        const lgs_loop_search_params prm = { 2.0 * r.uni(), 0.2 + 2.0 * r.uni(), r.below(6), 0 };
        for (int j = 0; j < 40; ++j) {
            const int lm = r.below(m);
            lgs_loop_search_hint h = { s.lo[(size_t)lm] + r.below(s.hi[(size_t)lm] - s.lo[(size_t)lm] + 1), lm,
                                       lm + 1 + r.below(m - lm), 0, 40.0 * r.uni() };
            if (loop_search_check_hint(h, n, s.lo.data(), s.hi.data(), m) != LGS_OK) {
                ok = false;
                continue;
            }
            lgs_loop_search_result a, b;
            std::vector<lgs_loop_search_map_best> ra((size_t)m), rb((size_t)m);
            loop_search_statement(s.poses.data(), s.lo.data(), s.hi.data(), m, &prm, h, nullptr, &a, ra.data());
            loop_search_statement(s.poses.data(), s.lo.data(), s.hi.data(), m, &prm, h, w.travel.data(), &b, rb.data());
            ok = ok && std::memcmp(&a, &b, sizeof(a)) == 0 &&
                 std::memcmp(ra.data(), rb.data(), sizeof(lgs_loop_search_map_best) * (size_t)m) == 0;
            // the record is the lowest map with the strictly smallest entry of the row
            int bi = -1;
            double bd = loop_search_min_sq(&prm);
            for (int i = 0; i < m; ++i)
                if (ra[(size_t)i].dist_sq < bd) {
                    bd = ra[(size_t)i].dist_sq;
                    bi = i;
                }
            invariant = invariant && (bi < 0 ? a.found == 0 : (a.found == 1 && a.local_map_idx == bi &&
                                                               a.local_map_node_idx == ra[(size_t)bi].node_idx &&
                                                               std::memcmp(&a.dist_sq, &bd, 8) == 0));
            for (int i = h.num_maps - 1; i < m; ++i) invariant = invariant && ra[(size_t)i].node_idx == -1;
            found += a.found;
            ++total;
        }
    }
    check(ok, "the loop with the snapshot's chain == the loop with its own", std::to_string(found) + " of " +
                                                                              std::to_string(total) + " hints found a node");
    check(invariant && found > 0 && found < total, "a record == the lowest-map strict minimum of its per-map row");
}

void validation()
{
    using namespace lgs;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<lgs_pose2d> poses(10);
    for (int k = 0; k < 10; ++k) poses[(size_t)k] = { 1.0 * k, 0.5 * k, nan };   // theta is not read
    const int lo[3] = { 0, 4, 7 }, hi[3] = { 3, 6, 9 };
    auto graph = [&](const lgs_pose2d* p, int n, const int* a, const int* b, int m) {
        return loop_search_check_graph(p, n, a, b, m, nullptr);
    };
    bool ok = graph(poses.data(), 10, lo, hi, 3) == LGS_OK;
    ok = ok && graph(nullptr, 10, lo, hi, 3) != LGS_OK && graph(poses.data(), 10, nullptr, hi, 3) != LGS_OK &&
         graph(poses.data(), 10, lo, nullptr, 3) != LGS_OK;
    ok = ok && graph(poses.data(), 0, lo, hi, 3) != LGS_OK && graph(poses.data(), 10, lo, hi, 0) != LGS_OK;
    ok = ok && graph(poses.data(), 9, lo, hi, 3) != LGS_OK;   // idx_max == n
    const int neg[3] = { -1, 4, 7 }, swapped[3] = { 0, 7, 7 };
    ok = ok && graph(poses.data(), 10, neg, hi, 3) != LGS_OK && graph(poses.data(), 10, swapped, hi, 3) != LGS_OK;
    for (double bad : { inf, -inf, nan }) {
        std::vector<lgs_pose2d> p = poses;
        p[5].x = bad;
        ok = ok && graph(p.data(), 10, lo, hi, 3) != LGS_OK;
        p = poses;
        p[9].y = bad;
        ok = ok && graph(p.data(), 10, lo, hi, 3) != LGS_OK;
    }
    check(ok, "snapshot validation", "null, n < 1, m < 1, ranges outside [0, n), min > max, non-finite x / y");

    lgs_loop_search_params prm = { 1.0, 2.0, 3, 0 };
    ok = loop_search_check_params(&prm) == LGS_OK && loop_search_check_params(nullptr) != LGS_OK;
    for (double bad : { inf, nan }) {
        lgs_loop_search_params q = prm;
        q.travel_dist_threshold = bad;
        ok = ok && loop_search_check_params(&q) != LGS_OK;
        q = prm;
        q.node_dist_threshold = bad;
        ok = ok && loop_search_check_params(&q) != LGS_OK;
    }
    prm.num_candidate_nodes = -1;
    ok = ok && loop_search_check_params(&prm) != LGS_OK;
    check(ok, "parameter validation", "non-finite thresholds, num_candidate_nodes < 0");

    auto hint = [&](int node, int lm, int nm, double acc) {
        const lgs_loop_search_hint h = { node, lm, nm, 0, acc };
        return loop_search_check_hint(h, 10, lo, hi, 3);
    };
    ok = hint(8, 2, 3, 5.0) == LGS_OK && hint(5, 1, 2, 0.0) == LGS_OK && hint(5, 1, 3, -1.0) == LGS_OK;
    ok = ok && hint(8, 2, 0, 5.0) != LGS_OK && hint(8, 2, 4, 5.0) != LGS_OK;      // num_maps outside 1 .. m
    ok = ok && hint(8, 2, 2, 5.0) != LGS_OK && hint(8, -1, 3, 5.0) != LGS_OK;     // latest map outside [0, num_maps)
    ok = ok && hint(-1, 0, 3, 5.0) != LGS_OK && hint(10, 2, 3, 5.0) != LGS_OK;    // node outside [0, n)
    ok = ok && hint(6, 2, 3, 5.0) != LGS_OK && hint(4, 0, 3, 5.0) != LGS_OK;      // node outside its latest map
    ok = ok && hint(8, 2, 3, inf) != LGS_OK && hint(8, 2, 3, nan) != LGS_OK;
    check(ok, "hint validation", "num_maps, latest map, latest node, its map's range, accum_travel_dist");

    // a failing batch leaves its outputs as they were
    lgs_loop_search_hint hs[2] = { { 8, 2, 3, 0, 5.0 }, { 6, 2, 3, 0, 5.0 } };
    lgs_loop_search_result out[2];
    std::memset(out, 0x55, sizeof(out));
    prm.num_candidate_nodes = 1;
    const int rc = loop_search_host(poses.data(), 10, lo, hi, 3, &prm, hs, 2, out, nullptr);
    bool untouched = true;
    for (size_t i = 0; i < sizeof(out); ++i) untouched = untouched && ((const unsigned char*)out)[i] == 0x55;
    check(rc == LGS_ERR_INVALID_ARG && untouched, "a batch with one bad hint fails whole and writes nothing");

    int a = 0, b = 0;
    loop_node_range(2147483000, 5, 2147483600, 2147483647, &a, &b);
    check(a == 5 && b == 2147483600, "the candidate node range does not wrap at INT_MAX");
    check(loop_accum_travel_dist(poses.data(), 1) == 0.0 && loop_accum_travel_dist(poses.data(), 3) ==
              std::hypot(-1.0, -0.5) + std::hypot(-1.0, -0.5), "accumulated travel distance of 1 and 3 nodes");
}

}  // namespace

int main()
{
    walk_and_partition();
    statement_with_and_without_chain();
    validation();
    std::printf(g_failed ? "LOOP SEARCH HOST CHECKS FAILED (%d)\n" : "LOOP SEARCH HOST CHECKS PASSED\n", g_failed);
    return g_failed ? 1 : 0;
}
