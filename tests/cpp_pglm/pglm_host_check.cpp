// pglm_host_check.cpp -- the host code of lgs_pg_lm_optimize
// (my-lidar-graph-slam_amd/csrc/pglm_pattern.hpp: argument checks, pair list,
// incidence lists) in a program of its own, built with
// -fsanitize=address,undefined (tests/cpp_pglm/Makefile).  Every buffer is a
// heap allocation of exactly the needed size, so an access past one is
// reported.  Every list is checked against a brute-force scan of the edges.
// Exit status 0 and "PGLM HOST CHECKS PASSED" when all hold.
#include <cmath>
#include <cstdio>
#include <limits>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "pglm_pattern.hpp"

namespace {

int g_failed = 0;

void check(bool ok, const std::string& name)
{
    std::printf("[%s] %s\n", ok ? " OK " : "FAIL", name.c_str());
    if (!ok) ++g_failed;
}

lgs_pg_edge edge(int s, int e)
{
    lgs_pg_edge g{};
    g.start_node_index = s;
    g.end_node_index = e;
    g.information[0] = g.information[4] = g.information[8] = 1.0;
    return g;
}

// an odometry chain, `loops` loop edges from the higher node to the lower, and extras
std::vector<lgs_pg_edge> chain(int n, int loops, unsigned seed)
{
    std::mt19937_64 rng(seed);
    std::vector<lgs_pg_edge> v;
    for (int i = 0; i + 1 < n; ++i) v.push_back(edge(i, i + 1));
    for (int k = 0; k < loops; ++k) {
        int a = (int)(rng() % (unsigned)n), b = (int)(rng() % (unsigned)n);
        if (a == b) continue;
        v.push_back(edge(std::max(a, b), std::min(a, b)));
    }
    return v;
}

bool lists_match_scan(int n, const std::vector<lgs_pg_edge>& edges)
{
    const int m = (int)edges.size();
    const lgs_pg_edge* e = edges.empty() ? nullptr : edges.data();
    if (!lgs::pglm_args_ok(n, m, e, 0, 1e-4, 1e-6, 1.0)) return false;
    lgs::PglmPattern P;
    lgs::pglm_build(n, m, e, P);
    if (P.n != n || P.m != m || (int)P.nptr.size() != n + 1) return false;
    // nodes: every (edge, role) by ascending edge
    for (int v = 0; v < n; ++v) {
        std::vector<int> want;
        for (int i = 0; i < m; ++i) {
            const int s = edges[(size_t)i].start_node_index, t = edges[(size_t)i].end_node_index;
            if (s == v && t == v)
                want.push_back(i << 2 | 2);
            else if (s == v)
                want.push_back(i << 2);
            else if (t == v)
                want.push_back(i << 2 | 1);
        }
        const std::vector<int> got(P.ninc.begin() + P.nptr[(size_t)v], P.ninc.begin() + P.nptr[(size_t)v + 1]);
        if (got != want) return false;
    }
    if ((size_t)P.nptr[(size_t)n] != P.ninc.size()) return false;
    // pairs: first-appearance order, every (edge, swapped) by ascending edge
    std::vector<std::pair<int, int>> order;
    std::map<std::pair<int, int>, std::vector<int>> lists;
    for (int i = 0; i < m; ++i) {
        const int s = edges[(size_t)i].start_node_index, t = edges[(size_t)i].end_node_index;
        if (s == t) continue;
        const std::pair<int, int> key(std::min(s, t), std::max(s, t));
        if (!lists.count(key)) order.push_back(key);
        lists[key].push_back(i << 1 | (s > t ? 1 : 0));
    }
    if (P.num_pairs() != (int)order.size() || P.pptr.size() != order.size() + 1) return false;
    for (size_t p = 0; p < order.size(); ++p) {
        if (P.pairs[2 * p] != order[p].first || P.pairs[2 * p + 1] != order[p].second) return false;
        const std::vector<int> got(P.pinc.begin() + P.pptr[p], P.pinc.begin() + P.pptr[p + 1]);
        if (got != lists[order[p]]) return false;
    }
    if ((size_t)P.pptr[order.size()] != P.pinc.size()) return false;
    // the block pattern is the one of that pair list: every entry names its source
    if (P.pat.blocks() != (size_t)n + 2 * order.size()) return false;
    for (int v = 0; v < n; ++v) {
        const int e0 = P.pat.rowptr[(size_t)v], e1 = P.pat.rowptr[(size_t)v + 1];
        if (P.pat.col[(size_t)e0] != v || P.pat.src[(size_t)e0] != -1) return false;
        for (int k = e0 + 1; k < e1; ++k) {
            const int s = P.pat.src[(size_t)k], p = s >= 0 ? s : -2 - s, u = P.pat.col[(size_t)k];
            if (p < 0 || p >= (int)order.size()) return false;
            if (s >= 0 ? (order[(size_t)p] != std::make_pair(v, u)) : (order[(size_t)p] != std::make_pair(u, v))) return false;
        }
    }
    return true;
}

}  // namespace

int main()
{
    check(lists_match_scan(1, {}), "n1: one node, no edge");
    check(lists_match_scan(2, { edge(0, 1) }), "n2: one edge");
    {
        std::vector<lgs_pg_edge> dup = chain(40, 3, 22);
        dup.push_back(edge(3, 17));
        dup.push_back(edge(17, 3));
        dup.push_back(edge(3, 17));
        check(lists_match_scan(40, dup), "dup: a pair three times over, in both directions");
    }
    {
        std::vector<lgs_pg_edge> hub = chain(330, 0, 21);
        for (int j = 0; j < 330; ++j)
            if (std::abs(j - 5) > 1) hub.push_back(edge(5, j));
        check(lists_match_scan(330, hub), "hub: 330 nodes, one node on 329 edges");
    }
    {
        std::vector<lgs_pg_edge> loop = chain(80, 14, 110);
        loop.push_back(edge(9, 9));
        check(lists_match_scan(80, loop), "80 nodes with a self-loop edge (9, 9)");
        loop.insert(loop.begin(), edge(0, 0));
        loop.push_back(edge(9, 9));
        check(lists_match_scan(80, loop), "self-loops first, last and twice on a node");
    }
    check(lists_match_scan(300, chain(300, 40, 7)), "n300: 339 edges");

    // what lgs_pg_lm_optimize refuses
    const std::vector<lgs_pg_edge> g = chain(50, 8, 5);
    const int m = (int)g.size();
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    check(lgs::pglm_args_ok(50, m, g.data(), 0, 1e-4, 1e-6, 1.0) && lgs::pglm_args_ok(1, 0, nullptr, 6, 0.0, 0.0, 1.0),
          "valid arguments pass");
    check(!lgs::pglm_args_ok(0, 0, nullptr, 0, 1e-4, 1e-6, 1.0) && !lgs::pglm_args_ok(-3, 0, nullptr, 0, 1e-4, 1e-6, 1.0) &&
              !lgs::pglm_args_ok(lgs::kPgMaxNodes + 1, 0, nullptr, 0, 1e-4, 1e-6, 1.0),
          "nodes < 1 or beyond the cap");
    check(!lgs::pglm_args_ok(50, -1, g.data(), 0, 1e-4, 1e-6, 1.0) &&
              !lgs::pglm_args_ok(50, lgs::kPglmMaxEdges + 1, g.data(), 0, 1e-4, 1e-6, 1.0) &&
              !lgs::pglm_args_ok(50, 3, nullptr, 0, 1e-4, 1e-6, 1.0),
          "edge count and NULL list");
    check(!lgs::pglm_args_ok(50, m, g.data(), -1, 1e-4, 1e-6, 1.0) && !lgs::pglm_args_ok(50, m, g.data(), 7, 1e-4, 1e-6, 1.0),
          "loss kind outside 0..6");
    check(!lgs::pglm_args_ok(50, m, g.data(), 0, nan, 1e-6, 1.0) && !lgs::pglm_args_ok(50, m, g.data(), 0, inf, 1e-6, 1.0) &&
              !lgs::pglm_args_ok(50, m, g.data(), 0, 1e-4, nan, 1.0) && !lgs::pglm_args_ok(50, m, g.data(), 0, 1e-4, -inf, 1.0) &&
              !lgs::pglm_args_ok(50, m, g.data(), 0, 1e-4, 1e-6, nan) && !lgs::pglm_args_ok(50, m, g.data(), 0, 1e-4, 1e-6, inf),
          "damping factor, tolerance or scale not finite");
    {
        bool ok = true;
        for (int which = 0; which < 4; ++which) {
            std::vector<lgs_pg_edge> bad(g);
            lgs_pg_edge& q = bad[(size_t)(m / 2)];
            if (which == 0) q.start_node_index = -1;
            if (which == 1) q.start_node_index = 50;
            if (which == 2) q.end_node_index = -1;
            if (which == 3) q.end_node_index = 50;
            ok = ok && !lgs::pglm_args_ok(50, m, bad.data(), 0, 1e-4, 1e-6, 1.0);
        }
        check(ok, "an edge index outside [0, nodes)");
        check(!lgs::pglm_args_ok(49, m, g.data(), 0, 1e-4, 1e-6, 1.0), "the edge list of a larger graph");
    }
    std::printf(g_failed ? "PGLM HOST CHECKS FAILED (%d)\n" : "PGLM HOST CHECKS PASSED\n", g_failed);
    return g_failed ? 1 : 0;
}
