// pgcg_pattern.hpp -- host side of the pose-graph conjugate-gradient solve
// (k_pgcg.hip): the argument checks of lgs_pg_cg_solve and the row-compressed
// 3x3-block pattern the kernel walks.  Plain C++ (no HIP), so that a
// stand-alone host program can run it under the sanitizers
// (tests/cpp_pgcg/pgcg_host_check.cpp).
//
// The caller hands H as one diagonal block per node and one block (a, b),
// a < b, per connected node pair.  The device stores every block row whole:
// row v holds its diagonal block first, then the blocks of its neighbours by
// ascending node index; the block of a pair (a, b) appears as it stands in row
// a and transposed in row b.  The pattern depends on the pair list only; the
// values are scattered into it for every solve (pg_fill_values).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

namespace lgs {

constexpr int kPgMaxNodes = 1 << 27;   // 3n rows, 2 * 3n passes and 9 * blocks stay far inside int / size_t
constexpr int kPgMaxPairs = 1 << 27;

struct PgPattern {
    int n = 0;
    std::vector<int> rowptr;   // [n + 1] block entries of row v: rowptr[v] .. rowptr[v + 1]
    std::vector<int> col;      // [blocks] node index of the entry's column
    std::vector<int> src;      // [blocks] -1: diag[v]; p >= 0: off[p] as it stands; -2 - p: off[p] transposed
    size_t blocks() const { return col.size(); }
};

// What lgs_pg_cg_solve refuses before it touches the device (pointers aside):
// true when the sizes, the pair list, the tolerance and the cap are usable.
inline bool pg_args_ok(int num_nodes, int num_pairs, const int* pairs, double tolerance, int max_iterations)
{
    if (num_nodes < 1 || num_nodes > kPgMaxNodes || num_pairs < 0 || num_pairs > kPgMaxPairs) return false;
    if (!(tolerance >= 0.0) || !std::isfinite(tolerance) || max_iterations < 0) return false;
    if (num_pairs > 0 && !pairs) return false;
    for (int p = 0; p < num_pairs; ++p) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        if (a < 0 || b >= num_nodes || a >= b) return false;
    }
    return true;
}

// The pattern of a checked pair list (pg_args_ok).  False when a pair is
// listed twice.
inline bool pg_build_pattern(int num_nodes, int num_pairs, const int* pairs, PgPattern& out)
{
    out.n = num_nodes;
    out.rowptr.assign((size_t)num_nodes + 1, 0);
    for (int v = 0; v < num_nodes; ++v) out.rowptr[(size_t)v + 1] = 1;   // the diagonal block
    for (int p = 0; p < num_pairs; ++p) {
        ++out.rowptr[(size_t)pairs[2 * p] + 1];
        ++out.rowptr[(size_t)pairs[2 * p + 1] + 1];
    }
    for (int v = 0; v < num_nodes; ++v) out.rowptr[(size_t)v + 1] += out.rowptr[(size_t)v];
    const size_t blocks = (size_t)out.rowptr[(size_t)num_nodes];
    out.col.assign(blocks, 0);
    out.src.assign(blocks, 0);
    std::vector<int> fill(out.rowptr.begin(), out.rowptr.end() - 1);
    for (int v = 0; v < num_nodes; ++v) {
        const size_t e = (size_t)fill[(size_t)v]++;
        out.col[e] = v;
        out.src[e] = -1;
    }
    for (int p = 0; p < num_pairs; ++p) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        const size_t ea = (size_t)fill[(size_t)a]++, eb = (size_t)fill[(size_t)b]++;
        out.col[ea] = b;
        out.src[ea] = p;
        out.col[eb] = a;
        out.src[eb] = -2 - p;
    }
    // neighbours by ascending node index behind the diagonal block
    std::vector<std::pair<int, int>> row;
    for (int v = 0; v < num_nodes; ++v) {
        const size_t e0 = (size_t)out.rowptr[(size_t)v] + 1, e1 = (size_t)out.rowptr[(size_t)v + 1];
        if (e1 - e0 < 2) continue;
        row.clear();
        for (size_t e = e0; e < e1; ++e) row.emplace_back(out.col[e], out.src[e]);
        std::sort(row.begin(), row.end());
        for (size_t e = e0; e < e1; ++e) {
            out.col[e] = row[e - e0].first;
            out.src[e] = row[e - e0].second;
            if (e > e0 && out.col[e] == out.col[e - 1]) return false;
        }
    }
    return true;
}

// val[9 * e ..] = the block of entry e, row-major
inline void pg_fill_values(const PgPattern& pat, const double* diag, const double* off, double* val)
{
    for (int v = 0; v < pat.n; ++v) {
        size_t e = (size_t)pat.rowptr[(size_t)v];
        const size_t e1 = (size_t)pat.rowptr[(size_t)v + 1];
        const double* d = diag + 9 * (size_t)v;
        for (int k = 0; k < 9; ++k) val[9 * e + k] = d[k];
        for (++e; e < e1; ++e) {
            const int s = pat.src[e];
            double* o = val + 9 * e;
            if (s >= 0) {
                const double* m = off + 9 * (size_t)s;
                for (int k = 0; k < 9; ++k) o[k] = m[k];
            } else {
                const double* m = off + 9 * (size_t)(-2 - s);
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) o[3 * i + j] = m[3 * j + i];
            }
        }
    }
}

}  // namespace lgs
