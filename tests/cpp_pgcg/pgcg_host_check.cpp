// pgcg_host_check.cpp -- the host code of lgs_pg_cg_solve
// (my-lidar-graph-slam_amd/csrc/pgcg_pattern.hpp: argument checks, block
// pattern, value scatter) in a program of its own, built with
// -fsanitize=address,undefined (tests/cpp_pgcg/Makefile).  Every buffer is a
// heap allocation of exactly the documented size, so an access past one is
// reported.  The pattern is checked against a dense matrix assembled from the
// same blocks.  Exit status 0 and "PGCG HOST CHECKS PASSED" when all hold.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "pgcg_pattern.hpp"

namespace {

int g_failed = 0;

void check(bool ok, const std::string& name)
{
    std::printf("[%s] %s\n", ok ? " OK " : "FAIL", name.c_str());
    if (!ok) ++g_failed;
}

struct System {
    int n = 0;
    std::vector<int> pairs;
    std::vector<double> diag, off;
};

// a chain, `loops` random extra pairs and, when hub >= 0, every pair with that node
System make_system(int n, int loops, int hub, unsigned seed)
{
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> val(-1.0, 1.0);
    std::set<std::pair<int, int>> have;
    System s;
    s.n = n;
    auto add = [&](int a, int b) {
        if (a == b) return;
        if (a > b) std::swap(a, b);
        if (!have.insert({ a, b }).second) return;
        s.pairs.push_back(a);
        s.pairs.push_back(b);
    };
    for (int v = n - 1; v > 0; --v) add(v - 1, v);   // descending: rows arrive unsorted
    for (int k = 0; k < loops; ++k) add((int)(rng() % (unsigned)n), (int)(rng() % (unsigned)n));
    if (hub >= 0)
        for (int v = 0; v < n; ++v) add(hub, v);
    s.diag.resize(9 * (size_t)n);
    s.off.resize(9 * (s.pairs.size() / 2));
    for (double& d : s.diag) d = val(rng);
    for (double& d : s.off) d = val(rng);
    return s;
}

bool pattern_matches_dense(const System& s)
{
    const int n = s.n, np = (int)(s.pairs.size() / 2);
    lgs::PgPattern pat;
    if (!lgs::pg_args_ok(n, np, s.pairs.data(), 0.0, 0)) return false;
    if (!lgs::pg_build_pattern(n, np, s.pairs.data(), pat)) return false;
    if ((int)pat.rowptr.size() != n + 1 || pat.blocks() != (size_t)n + 2 * (size_t)np) return false;
    std::vector<double> val(9 * pat.blocks(), std::numeric_limits<double>::quiet_NaN());
    lgs::pg_fill_values(pat, s.diag.data(), s.off.empty() ? nullptr : s.off.data(), val.data());
    const size_t m = 3 * (size_t)n;
    std::vector<double> dense(m * m, 0.0), rebuilt(m * m, 0.0);
    auto put = [&](std::vector<double>& M, int r, int c, const double* b, bool transposed) {
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) M[(3 * (size_t)r + i) * m + 3 * (size_t)c + j] = transposed ? b[3 * j + i] : b[3 * i + j];
    };
    for (int v = 0; v < n; ++v) put(dense, v, v, &s.diag[9 * (size_t)v], false);
    for (int p = 0; p < np; ++p) {
        put(dense, s.pairs[2 * p], s.pairs[2 * p + 1], &s.off[9 * (size_t)p], false);
        put(dense, s.pairs[2 * p + 1], s.pairs[2 * p], &s.off[9 * (size_t)p], true);
    }
    for (int v = 0; v < n; ++v) {
        const int e0 = pat.rowptr[(size_t)v], e1 = pat.rowptr[(size_t)v + 1];
        if (e1 <= e0 || pat.col[(size_t)e0] != v) return false;   // the diagonal block first
        for (int e = e0; e < e1; ++e) {
            if (pat.col[(size_t)e] < 0 || pat.col[(size_t)e] >= n) return false;
            if (e > e0 + 1 && pat.col[(size_t)e] <= pat.col[(size_t)e - 1]) return false;   // ascending neighbours
            put(rebuilt, v, pat.col[(size_t)e], &val[9 * (size_t)e], false);
        }
    }
    for (size_t k = 0; k < m * m; ++k)
        if (!(dense[k] == rebuilt[k])) return false;
    return true;
}

}  // namespace

int main()
{
    check(pattern_matches_dense(make_system(1, 0, -1, 1)), "one node, no pair");
    check(pattern_matches_dense(make_system(2, 0, -1, 2)), "two nodes, one pair");
    check(pattern_matches_dense(make_system(67, 9, -1, 3)), "67 nodes, chain and loops");
    check(pattern_matches_dense(make_system(400, 60, 17, 4)), "400 nodes with a hub of degree 399");

    // what lgs_pg_cg_solve refuses
    const System s = make_system(50, 8, -1, 5);
    const int np = (int)(s.pairs.size() / 2);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    check(lgs::pg_args_ok(50, np, s.pairs.data(), 0.0, 0) && lgs::pg_args_ok(50, np, s.pairs.data(), 1e-3, 7) &&
              lgs::pg_args_ok(1, 0, nullptr, 0.0, 0),
          "valid arguments pass");
    check(!lgs::pg_args_ok(0, 0, nullptr, 0.0, 0) && !lgs::pg_args_ok(-4, 0, nullptr, 0.0, 0) &&
              !lgs::pg_args_ok(lgs::kPgMaxNodes + 1, 0, nullptr, 0.0, 0),
          "num_nodes < 1 or beyond the cap");
    check(!lgs::pg_args_ok(50, -1, s.pairs.data(), 0.0, 0) && !lgs::pg_args_ok(50, 3, nullptr, 0.0, 0), "pair count and NULL list");
    check(!lgs::pg_args_ok(50, np, s.pairs.data(), -1e-9, 0) && !lgs::pg_args_ok(50, np, s.pairs.data(), nan, 0) &&
              !lgs::pg_args_ok(50, np, s.pairs.data(), inf, 0) && !lgs::pg_args_ok(50, np, s.pairs.data(), 0.0, -1),
          "tolerance negative or not finite, negative cap");
    {
        bool ok = true;
        for (int which = 0; which < 4; ++which) {
            std::vector<int> bad(s.pairs);
            int* q = &bad[2 * (size_t)(np / 2)];
            if (which == 0) std::swap(q[0], q[1]);   // a > b
            if (which == 1) q[1] = q[0];             // a == b
            if (which == 2) q[1] = 50;               // beyond the last node
            if (which == 3) q[0] = -1;
            ok = ok && !lgs::pg_args_ok(50, np, bad.data(), 0.0, 0);
        }
        check(ok, "a pair with a >= b or an index out of range");
        check(!lgs::pg_args_ok(49, np, s.pairs.data(), 0.0, 0), "the pair list of a larger graph");
    }
    {
        std::vector<int> twice(s.pairs);
        twice.push_back(s.pairs[6]);
        twice.push_back(s.pairs[7]);
        lgs::PgPattern pat;
        check(lgs::pg_args_ok(50, np + 1, twice.data(), 0.0, 0) && !lgs::pg_build_pattern(50, np + 1, twice.data(), pat),
              "a pair listed twice is refused by the pattern builder");
    }
    std::printf(g_failed ? "PGCG HOST CHECKS FAILED (%d)\n" : "PGCG HOST CHECKS PASSED\n", g_failed);
    return g_failed ? 1 : 0;
}
