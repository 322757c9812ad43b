// pglm_pattern.hpp -- host side of the device-resident pose-graph
// Levenberg-Marquardt loop (k_pglm.hip): the argument checks of
// lgs_pg_lm_optimize / lgs_pg_lm_linearize and, from the edge list alone, what
// the linearisation kernel walks.  Plain C++ (no HIP), so that a stand-alone
// host program can run it under the sanitizers
// (tests/cpp_pglm/pglm_host_check.cpp).
//
// The host's OptimizeStep adds every edge's terms into H and b one edge after
// the other.  The kernel forms every entry of H as that same sequential sum:
// a thread owns one 3x3 block of the row-compressed matrix (pgcg_pattern.hpp)
// and walks the edges that touch it by ascending edge index,
//   nodes   node v: (edge, role) of every edge that starts (role 0) or ends
//           (role 1) at v, or does both (role 2, a self-loop: four terms)
//   pairs   pair p = (a, b), a < b, in the order the edges first name it:
//           (edge, swapped) of every edge a -> b (0) or b -> a (1: its block
//           is added transposed)
// both as CSR arrays.  The block pattern is the one of that pair list.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

#include "lgs_hip.h"
#include "pgcg_pattern.hpp"

namespace lgs {

constexpr int kPglmMaxEdges = 1 << 27;   // edge << 2 | role stays inside int

struct PglmPattern {
    int n = 0, m = 0;
    std::vector<int> pairs;   // [2 * np] (a, b), a < b, first-appearance order
    PgPattern pat;            // the block pattern of `pairs`
    std::vector<int> nptr;    // [n + 1]
    std::vector<int> ninc;    // [nptr[n]] edge << 2 | role, ascending per node
    std::vector<int> pptr;    // [np + 1]
    std::vector<int> pinc;    // [pptr[np]] edge << 1 | swapped, ascending per pair
    int num_pairs() const { return (int)(pairs.size() / 2); }
};

// What the resident entry points refuse before they touch the device
// (pointers aside): sizes, edge indices, the loss kind, and a damping factor,
// tolerance or scale that is not finite.
inline bool pglm_args_ok(int n, int m, const lgs_pg_edge* edges, int loss_kind, double lambda, double tolerance,
                         double loss_scale)
{
    if (n < 1 || n > kPgMaxNodes || m < 0 || m > kPglmMaxEdges) return false;
    if (m > 0 && !edges) return false;
    if (loss_kind < 0 || loss_kind > 6) return false;
    if (!std::isfinite(lambda) || !std::isfinite(tolerance) || !std::isfinite(loss_scale)) return false;
    for (int i = 0; i < m; ++i)
        if (edges[i].start_node_index < 0 || edges[i].start_node_index >= n || edges[i].end_node_index < 0 ||
            edges[i].end_node_index >= n)
            return false;
    return true;
}

// The lists of a checked edge list (pglm_args_ok)
inline void pglm_build(int n, int m, const lgs_pg_edge* edges, PglmPattern& out)
{
    out.n = n;
    out.m = m;
    // nodes: a counting pass, then the edges in order
    out.nptr.assign((size_t)n + 1, 0);
    for (int i = 0; i < m; ++i) {
        const int s = edges[i].start_node_index, e = edges[i].end_node_index;
        ++out.nptr[(size_t)s + 1];
        if (e != s) ++out.nptr[(size_t)e + 1];
    }
    for (int v = 0; v < n; ++v) out.nptr[(size_t)v + 1] += out.nptr[(size_t)v];
    out.ninc.assign((size_t)out.nptr[(size_t)n], 0);
    {
        std::vector<int> fill(out.nptr.begin(), out.nptr.end() - 1);
        for (int i = 0; i < m; ++i) {
            const int s = edges[i].start_node_index, e = edges[i].end_node_index;
            if (s == e) {
                out.ninc[(size_t)fill[(size_t)s]++] = i << 2 | 2;
            } else {
                out.ninc[(size_t)fill[(size_t)s]++] = i << 2;
                out.ninc[(size_t)fill[(size_t)e]++] = i << 2 | 1;
            }
        }
    }
    // pairs: the edges by (pair, edge); a pair's slot is the rank of its first edge
    struct Item {
        long long key;
        int edge;
    };
    std::vector<Item> items;
    items.reserve((size_t)m);
    for (int i = 0; i < m; ++i) {
        const int s = edges[i].start_node_index, e = edges[i].end_node_index;
        if (s != e) items.push_back(Item{ (long long)std::min(s, e) * n + std::max(s, e), i });
    }
    std::sort(items.begin(), items.end(),
              [](const Item& x, const Item& y) { return x.key != y.key ? x.key < y.key : x.edge < y.edge; });
    std::vector<std::pair<int, size_t>> first;   // (first edge, position in items) of every pair
    for (size_t k = 0; k < items.size(); ++k)
        if (k == 0 || items[k].key != items[k - 1].key) first.emplace_back(items[k].edge, k);
    std::sort(first.begin(), first.end());
    const size_t np = first.size();
    out.pairs.assign(2 * np, 0);
    out.pptr.assign(np + 1, 0);
    out.pinc.assign(items.size(), 0);
    size_t w = 0;
    for (size_t p = 0; p < np; ++p) {
        const size_t k0 = first[p].second;
        const int a = (int)(items[k0].key / n), b = (int)(items[k0].key % n);
        out.pairs[2 * p] = a;
        out.pairs[2 * p + 1] = b;
        for (size_t k = k0; k < items.size() && items[k].key == items[k0].key; ++k)
            out.pinc[w++] = items[k].edge << 1 | (edges[items[k].edge].start_node_index == a ? 0 : 1);
        out.pptr[p + 1] = (int)w;
    }
    pg_build_pattern(n, (int)np, out.pairs.data(), out.pat);   // no pair twice by construction
}

}  // namespace lgs
