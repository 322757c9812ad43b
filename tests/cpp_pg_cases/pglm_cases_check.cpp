// pglm_cases_check.cpp -- the incidence-list builder of lgs_pg_lm_optimize
// (my-lidar-graph-slam_amd/csrc/pglm_pattern.hpp) on the edge lists of three
// graphs of tests/pg_cases.py (pg_case_tables.hpp), under
// -fsanitize=address,undefined.  It is tests/cpp_pglm/pglm_host_check.cpp
// extended: that program's source is compiled in as it stands, its own checks
// run first, and the new lists go through its lists_match_scan, the brute-force
// scan of the edges.  Exit status 0 and "PG CASES PGLM CHECKS PASSED" when all
// hold.
#define main pglm_host_check_main
#include "../cpp_pglm/pglm_host_check.cpp"
#undef main

#include "pg_case_tables.hpp"

namespace {

// the edges of a table of (start, end) rows
std::vector<lgs_pg_edge> table(const int* rows, size_t m)
{
    std::vector<lgs_pg_edge> v;
    for (size_t i = 0; i < m; ++i) v.push_back(edge(rows[2 * i], rows[2 * i + 1]));
    return v;
}

// the nodes whose incidence list pglm_build leaves empty and whose block row holds the diagonal block alone
std::vector<int> nodes_without_edges(int n, const std::vector<lgs_pg_edge>& edges)
{
    lgs::PglmPattern P;
    lgs::pglm_build(n, (int)edges.size(), edges.empty() ? nullptr : edges.data(), P);
    std::vector<int> out;
    for (int v = 0; v < n; ++v)
        if (P.nptr[(size_t)v + 1] == P.nptr[(size_t)v] && P.pat.rowptr[(size_t)v + 1] - P.pat.rowptr[(size_t)v] == 1)
            out.push_back(v);
    return out;
}

}  // namespace

int main()
{
    if (pglm_host_check_main() != 0) return 1;
    namespace t = pg_case_tables;
    const std::vector<lgs_pg_edge> relabel = table(t::k_relabel150_edges, sizeof t::k_relabel150_edges / sizeof(int) / 2);
    check(relabel.size() == 151 && lists_match_scan(t::k_relabel150_nodes, relabel) &&
              nodes_without_edges(t::k_relabel150_nodes, relabel) == std::vector<int>{},
          "relabel150: labels permuted, edges shuffled and reversed");
    const std::vector<lgs_pg_edge> isolated = table(t::k_isolated90_edges, sizeof t::k_isolated90_edges / sizeof(int) / 2);
    check(isolated.size() == 89 && lists_match_scan(t::k_isolated90_nodes, isolated) &&
              nodes_without_edges(t::k_isolated90_nodes, isolated) == std::vector<int>{ 40, 89 },
          "isolated90: nodes 40 and 89, the last, on no edge");
    check(lists_match_scan(t::k_no_edges5_nodes, {}) &&
              nodes_without_edges(t::k_no_edges5_nodes, {}) == std::vector<int>{ 0, 1, 2, 3, 4 },
          "no_edges5: five nodes, no edge");
    std::printf(g_failed ? "PG CASES PGLM CHECKS FAILED (%d)\n" : "PG CASES PGLM CHECKS PASSED\n", g_failed);
    return g_failed ? 1 : 0;
}
