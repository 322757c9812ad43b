// coarse_pair_check.cpp -- the "pair read stays inside the allocation"
// condition of my-lidar-graph-slam_amd/csrc/coarse_pair.hpp in a program of
// its own, built with -fsanitize=address,undefined.  For every layout it
// restates the paired coarse kernel's reads by brute force -- every plane,
// every lattice start coarse_base_l can return (and the base 0 of a window
// that misses the map), every pair lane -- marks both doubles of every read
// in a byte map of the planes plus a tail, and checks that the largest index
// the function names is the largest one read and that it says "inside"
// exactly when that index lies below the allocation's size.  Layouts: square and
// oblong maps of 100..1010 cells, LowRes 3 and 5, windows with odd and even
// lattices; each also with the allocation cut short, so that the function
// must answer "no" somewhere.  Prints one line per configuration; exit
// status 1 if any check fails.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "coarse_pair.hpp"

namespace {

int g_failed = 0;

void check(bool ok, const std::string& name)
{
    std::printf("[%s] %s\n", ok ? " OK " : "FAIL", name.c_str());
    if (!ok) ++g_failed;
}

constexpr int kSB = 4;

// k_rtcsm.hip set_plane_layout / plane_bytes, restated
lgs::CoarsePairGeom layout(int W, int H, int lr, int ncx, int ncy)
{
    lgs::CoarsePairGeom g{};
    g.low_res = lr;
    g.ncx = ncx;
    g.ncy = ncy;
    g.Wq = (W + lr - 1) / lr;
    g.Hq = (H + lr - 1) / lr;
    const int nsbx = (ncx + kSB - 1) / kSB, nsby = (ncy + kSB - 1) / kSB;
    g.M = std::max(kSB * nsbx, kSB * nsby);
    g.Wqp = (g.Wq + 2 * g.M + 3) & ~3;
    g.Hqp = g.Hq + 2 * g.M;
    g.pstride = (long long)g.Wqp * g.Hqp;
    const long long bytes = ((long long)sizeof(double) * lr * lr * g.pstride + 255) & ~255LL;
    g.alloc = bytes / (long long)sizeof(double);
    return g;
}

// The largest index any pair lane reads, by enumeration: reads do not depend
// on the allocation's size, so one enumeration serves every size tried.
long long brute_last(const lgs::CoarsePairGeom& g)
{
    const long long tail = (long long)g.Wqp * (g.ncy + 2) + 64;   // room for reads that leave the planes
    std::vector<unsigned char> seen((size_t)((long long)g.low_res * g.low_res * g.pstride + tail), 0);
    const int npair = (g.ncx + 1) / 2;   // pairs (jx, jx + 1), jx = 0, 2, ..: the last jx + 1 possibly past the lattice
    auto lanes = [&](long long base) {
        for (int jy = 0; jy < g.ncy; ++jy)   // a row's pairs are 2 * npair consecutive doubles
            std::memset(&seen[(size_t)(base + (long long)jy * g.Wqp)], 1, (size_t)(2 * npair));
    };
    lanes(0);   // a window that misses the map
    for (int p = 0; p < g.low_res * g.low_res; ++p)
        for (int qy0 = -g.ncy + 1; qy0 < g.Hq; ++qy0)
            for (int qx0 = -g.ncx + 1; qx0 < g.Wq; ++qx0)
                lanes(p * g.pstride + (long long)(qy0 + g.M) * g.Wqp + (qx0 + g.M));
    long long last = -1;
    for (size_t i = 0; i < seen.size(); ++i)
        if (seen[i]) last = (long long)i;
    return last;
}

// expect: 1 inside, 0 not, -1 either (the brute-force answer decides)
void one(const char* what, const lgs::CoarsePairGeom& g, long long last, int expect, int* yes, int* no)
{
    const bool inside = last < g.alloc;
    const bool f = lgs::coarse_pair_read_inside(g);
    char name[256];
    std::snprintf(name, sizeof name, "%s lr %d Wq %d Hq %d ncx %d ncy %d M %d Wqp %d alloc %lld: last %lld (function %lld), inside %d",
                  what, g.low_res, g.Wq, g.Hq, g.ncx, g.ncy, g.M, g.Wqp, g.alloc, last, lgs::coarse_pair_last_read(g),
                  (int)inside);
    check(f == inside && lgs::coarse_pair_last_read(g) == last && (expect < 0 || inside == (expect != 0)), name);
    ++*(inside ? yes : no);
}

}   // namespace

int main()
{
    int yes = 0, no = 0;
    const int sizes[][2] = { { 100, 100 }, { 101, 137 }, { 250, 103 }, { 400, 400 }, { 641, 322 }, { 1010, 1010 }, { 1007, 100 } };
    const int lattices[][2] = { { 9, 9 }, { 8, 8 }, { 17, 17 }, { 12, 7 }, { 5, 6 }, { 1, 1 }, { 2, 3 }, { 21, 20 } };
    for (const int lr : { 3, 5 })
        for (const auto& s : sizes)
            for (const auto& l : lattices) {
                const lgs::CoarsePairGeom g = layout(s[0], s[1], lr, l[0], l[1]);
                const long long last = brute_last(g);
                one("layout", g, last, 1, &yes, &no);
                // the same reads against shorter allocations: through the last
                // read, one short of it, and short by the bottom margin
                lgs::CoarsePairGeom c = g;
                c.alloc = last + 1;
                one("exact", c, last, 1, &yes, &no);
                c.alloc = last;
                one("one short", c, last, 0, &yes, &no);
                c.alloc = g.alloc - g.Wqp * (long long)g.M;
                one("margin short", c, last, -1, &yes, &no);
            }
    // a layout without the right and bottom margins: the last rows of the
    // last plane's windows leave the planes
    {
        lgs::CoarsePairGeom g = layout(100, 100, 5, 9, 9);
        g.Wqp = g.Wq + g.M;
        g.Hqp = g.Hq + g.M;
        g.pstride = (long long)g.Wqp * g.Hqp;
        g.alloc = (long long)g.low_res * g.low_res * g.pstride;
        one("no far margins", g, brute_last(g), 0, &yes, &no);
    }
    check(yes > 0 && no > 0, "both answers occurred");
    std::printf("%d inside, %d not, %d failed\n", yes, no, g_failed);
    if (!g_failed) std::printf("COARSE PAIR CHECKS PASSED\n");
    return g_failed ? 1 : 0;
}
