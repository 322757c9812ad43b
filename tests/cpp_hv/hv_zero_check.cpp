// hv_zero_check.cpp -- the footprint -> precompute-tile range of
// my-lidar-graph-slam_amd/csrc/hv_zero.hpp in a program of its own, built with
// -fsanitize=address,undefined.  For every live thread of k_super_hv<1> and
// <2> it restates the kernel's loads (both strips included), cell by cell and
// plane by plane, and checks that every loaded cell is either a margin cell
// (never written, +0) or an output of a precompute tile inside the range the
// function returns, and that the range never leaves the tile grid.  Where no
// strip widens it the range must equal the brute-force one exactly, so a
// function that answers "every tile" does not pass.  Prints one line per
// configuration; exit status 1 if any check fails.
#include <algorithm>
#include <cstdio>
#include <string>

#include "hv_zero.hpp"

namespace {

int g_failed = 0;

void check(bool ok, const std::string& name)
{
    std::printf("[%s] %s\n", ok ? " OK " : "FAIL", name.c_str());
    if (!ok) ++g_failed;
}

struct Geom {
    int W, H, lr, M, Wq, Hq, Wqp, Hqp;
    int X4lo, ncol, qlo, nqt;   // k_rtcsm.hip super_geom
};

Geom geom(int W, int H, int lr, int M)
{
    Geom g{};
    g.W = W;
    g.H = H;
    g.lr = lr;
    g.M = M;
    g.Wq = (W + lr - 1) / lr;
    g.Hq = (H + lr - 1) / lr;
    g.Wqp = (g.Wq + 2 * M + 3) & ~3;
    g.Hqp = g.Hq + 2 * M;
    g.X4lo = (M - 4) >> 2;
    g.ncol = ((M + g.Wq - 1) >> 2) - g.X4lo + 1;
    g.qlo = (M - 4) >> 4;
    g.nqt = ((M + g.Hq - 1) >> 4) - g.qlo + 1;
    return g;
}

struct Brute {
    int ty0 = 1 << 30, ty1 = -1, tx0 = 1 << 30, tx1 = -1;
    bool any = false;
};

// one loaded cell: padded (Y, X) of plane (py, px)
void cell(const Geom& g, const lgs::HvTiling& t, int py, int px, int Y, int X, Brute& b)
{
    if (Y < g.M || Y >= g.M + g.Hq || X < g.M || X >= g.M + g.Wq) return;   // margin
    const int fy = g.lr * (Y - g.M) + py, fx = g.lr * (X - g.M) + px;
    if (fy >= g.H || fx >= g.W) return;   // past the map: no tile writes it
    const int ty = fy / t.prows, tx = fx / t.pcols;
    b.any = true;
    b.ty0 = std::min(b.ty0, ty);
    b.ty1 = std::max(b.ty1, ty);
    b.tx0 = std::min(b.tx0, tx);
    b.tx1 = std::max(b.tx1, tx);
}

// k_super_hv<nq>, thread (qt, X4): the loads whose values reach a maximum, in
// every plane.  (Each row's second 8-byte load also fetches column 4 X4 + 7,
// which no maximum uses.)
Brute loads(const Geom& g, const lgs::HvTiling& t, int qt, int X4, int nq)
{
    Brute b;
    const int NR = 16 * nq + 3;
    for (int ry = 0; ry < g.lr; ++ry)
        for (int rx = 0; rx < g.lr; ++rx) {
            const bool cstrip = rx > 0 && 4 * X4 + 3 == g.M - 1;
            for (int k = 0; k < NR; ++k) {
                const int Y = 16 * qt + k;
                if (Y >= g.Hqp) continue;   // loaded from the clamped row, then zeroed
                const bool rs = Y == g.M - 1 && ry > 0;
                // the row: plane (0, rx) row M on the row strip, else the thread's own
                const int py = rs ? 0 : ry, Yr = rs ? g.M : Y;
                for (int i = 0; i < 7; ++i) cell(g, t, py, rx, Yr, 4 * X4 + i, b);
                if (cstrip) {   // column M - 1 takes column M of plane (ry, 0) (row strip: plane 0's (M, M))
                    if (rs)
                        cell(g, t, 0, 0, g.M, g.M, b);
                    else
                        cell(g, t, ry, 0, Y, g.M, b);
                }
            }
        }
    return b;
}

void run(int W, int H, int lr, int M, int prows, int nq)
{
    const Geom g = geom(W, H, lr, M);
    lgs::HvTiling t{};
    t.pcols = lgs::hv_pcols(lr);
    t.prows = prows;
    t.pgx = (W + t.pcols - 1) / t.pcols;
    t.pgy = (H + prows - 1) / prows;
    t.W = W;
    t.H = H;
    long live = 0, empty = 0, covered = 0, in_grid = 0, exact = 0, plain = 0;
    const int slots = (g.ncol * (g.nqt + nq - 1) + 255) / 256 * 256;
    for (int tq = 0; tq < slots; ++tq) {
        const int qi = tq / g.ncol, c = tq - qi * g.ncol;
        const int qt = g.qlo + qi - (nq - 1);
        if (!(qi < g.nqt + nq - 1 && qt >= 0)) continue;
        ++live;
        const int X4 = g.X4lo + c;
        const lgs::HvTileRange r = lgs::hv_zero_range(qt, X4, nq, g.M, g.Wq, g.Hq, lr, t);
        const Brute b = loads(g, t, qt, X4, nq);
        if (r.empty()) {
            ++empty;
            ++in_grid;
            covered += !b.any;
        } else {
            in_grid += r.ty0 >= 0 && r.tx0 >= 0 && r.ty1 < t.pgy && r.tx1 < t.pgx;
            covered += !b.any || (r.ty0 <= b.ty0 && b.ty1 <= r.ty1 && r.tx0 <= b.tx0 && b.tx1 <= r.tx1);
        }
        // no strip in the footprint: nothing to be conservative about
        const int Ya = 16 * qt, Yb = 16 * qt + 16 * nq + 2, Xa = 4 * X4, Xb = 4 * X4 + 6;
        if (!(Ya <= g.M - 1 && g.M - 1 <= Yb) && !(Xa <= g.M - 1 && g.M - 1 <= Xb)) {
            ++plain;
            exact += r.empty() ? !b.any
                               : (b.any && r.ty0 == b.ty0 && r.ty1 == b.ty1 && r.tx0 == b.tx0 && r.tx1 == b.tx1);
        }
    }
    char name[160];
    std::snprintf(name, sizeof(name), "map %dx%d LowRes %d M %d rows/tile %d NQ %d: %ld live, %ld empty, %ld plain", W, H,
                  lr, M, prows, nq, live, empty, plain);
    check(live > 0 && covered == live && in_grid == live && exact == plain, name);
}

}  // namespace

int main()
{
    const int sizes[] = { 100, 105, 600, 1000, 1010 };
    const int lrs[] = { 5, 3 };
    const int margins[] = { 4, 8, 20, 36 };
    for (int s : sizes)
        for (int lr : lrs)
            for (int M : margins) {
                if (s > 105 && (M == 4 || M == 36)) continue;   // every margin on the small maps only (run time)
                for (int prows : { 8, 4 })
                    for (int nq : { 1, 2 }) run(s, s, lr, M, prows, nq);
            }
    // not square, and a map narrower than one tile
    for (int nq : { 1, 2 }) {
        run(1000, 105, 5, 8, 8, nq);
        run(105, 1010, 3, 20, 4, nq);
        run(30, 30, 5, 4, 8, nq);
    }
    if (g_failed) {
        std::printf("%d HV ZERO CHECKS FAILED\n", g_failed);
        return 1;
    }
    std::printf("HV ZERO CHECKS PASSED\n");
    return 0;
}
