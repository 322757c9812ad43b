// Host check of the certified fast cell (my-lidar-graph-slam_amd/csrc/fast_cell.hpp)
// against the exact projection chain of k_project / lean_cell, restated here
// operation for operation.  Built by tests/test_fast_cell_cpu.py with g++ and
// -ffp-contract=off (the library's own setting).
//
// For every case: if the fast cell is certain, the exact chain must give the
// same cell on both axes and raise no guard.  Prints one JSON line with the
// counts per family; exit status 1 on any violation.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "fast_cell.hpp"

namespace {

struct Rng {
    uint64_t s;
    uint64_t next()
    {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 0x2545F4914F6CDD1Dull;
    }
    double uni() { return (double)(next() >> 11) * 0x1p-53; }             // [0, 1)
    double range(double a, double b) { return a + (b - a) * uni(); }
    int below(int n) { return (int)(next() % (uint64_t)n); }
};

// k_rtcsm.hip near_boundary
bool near_boundary(double q, double eps)
{
    const double f = q - floor(q);
    const double e = eps + fabs(q) * 1e-13;
    return f < e || f > 1.0 - e;
}

struct Item {
    double sx, sy, min_x, min_y, res, geps;
    int win_x, win_y;
};

struct Counts {
    long long cases = 0, certain = 0, bad = 0;
};

struct Bad {
    double v[10];
};
std::vector<Bad> g_bad;

// one (item, angle, beam): exact chain vs fast cell
void check(const Item& it, double ct, double st, double ca, double sa, double r, Counts& n)
{
    const double inv_res = 1.0 / it.res;
    // exact chain (lean_cell)
    const double c = ct * ca - st * sa;
    const double s = st * ca + ct * sa;
    const double hx = it.sx + r * c;
    const double hy = it.sy + r * s;
    const double qx = (hx - it.min_x) * inv_res;
    const double qy = (hy - it.min_y) * inv_res;
    const bool guarded = near_boundary(qx, it.geps) || near_boundary(qy, it.geps);
    // fast chain
    const lgs_fast::ItemConsts k =
        lgs_fast::item_consts(it.sx, it.sy, it.min_x, it.min_y, inv_res, it.geps, it.win_x, it.win_y);
    const double rs = lgs_fast::beam_rs(r, inv_res);
    int ix = 0, iy = 0;
    const bool certain = lgs_fast::cell(ct, st, sa, ct * ca, st * ca, rs, k.ox, k.oy, k.h0, ix, iy);
    ++n.cases;
    if (!certain) return;
    ++n.certain;
    const bool same = floor(qx) == (double)ix && floor(qy) == (double)iy;
    if (!same || guarded) {
        ++n.bad;
        if (g_bad.size() < 4) g_bad.push_back({ { it.sx, it.sy, it.min_x, it.min_y, it.res, ct, st, ca, sa, r } });
    }
}

const double kOrigins[] = { 0.0, -6.0, 1e4, -1e4, 8192.0, -4096.0 };
const double kRes[] = { 0.05, 0.01 };

Item random_item(Rng& g, double geps)
{
    Item it;
    it.res = kRes[g.below(2)];
    it.min_x = kOrigins[g.below(6)] + g.range(-1.0, 1.0);
    it.min_y = kOrigins[g.below(6)] + g.range(-1.0, 1.0);
    it.sx = it.min_x + g.range(-5.0, 45.0);   // the sensor in or near a map of some 40 m
    it.sy = it.min_y + g.range(-5.0, 45.0);
    it.geps = geps;
    it.win_x = g.below(200) - 100;
    it.win_y = g.below(200) - 100;
    return it;
}

}   // namespace

int main(int argc, char** argv)
{
    const long long scale = argc > 1 ? atoll(argv[1]) : 1;   // 1: 1.2e7 cases
    Rng g{ 0x9E3779B97F4A7C15ull };
    // trig tables: unit vectors as the device tables hold them (sincos of an angle)
    const int NT = 8192;
    std::vector<double> tc(NT), ts(NT);
    for (int i = 0; i < NT; ++i) {
        const double a = i < 8 ? i * (M_PI / 4) : g.range(-M_PI, M_PI);   // the axes' angles among them
        sincos(a, &ts[i], &tc[i]);
    }
    Counts rnd, edge, ints, wild, big;

    // A. random, non-adversarial input, the default guard (geps = 1e-9)
    for (long long n = 0; n < 60000 * scale; ++n) {
        const Item it = random_item(g, 1e-9);
        for (int j = 0; j < 100; ++j) {
            const int a = g.below(NT), b = g.below(NT);
            check(it, tc[a], ts[a], tc[b], ts[b], g.range(0.0, 30.0), rnd);
        }
    }
    // B. quotients placed 1e-15 .. 1e-8 cells from a cell boundary, either side,
    // on x or on y; guards of 0, 1e-9 and 1e-5
    const double kEps[] = { 0.0, 1e-9, 1e-5 };
    for (long long n = 0; n < 30000 * scale; ++n) {
        const Item it = random_item(g, kEps[g.below(3)]);
        for (int j = 0; j < 100; ++j) {
            const int a = g.below(NT), b = g.below(NT);
            const double c = tc[a] * tc[b] - ts[a] * ts[b], s = ts[a] * tc[b] + tc[a] * ts[b];
            const bool on_x = g.below(2) == 0;
            const double dir = on_x ? c : s;
            if (fabs(dir) < 1e-3) continue;
            const double delta = (g.below(2) ? 1.0 : -1.0) * exp(g.range(log(1e-15), log(1e-8)));
            const double cellq = floor(g.range(-200.0, 900.0)) + delta;   // the wanted quotient
            const double r = (cellq * it.res + (on_x ? it.min_x - it.sx : it.min_y - it.sy)) / dir;
            if (!(r >= 0.0 && r < 200.0)) continue;
            check(it, tc[a], ts[a], tc[b], ts[b], r, edge);
        }
    }
    // C. quotients that are exact integers: the sensor on a cell corner of a
    // map at the origin, axis-aligned beams of a whole number of cells
    for (long long n = 0; n < 20000 * scale; ++n) {
        Item it = random_item(g, kEps[g.below(3)]);
        it.min_x = floor(it.min_x);
        it.min_y = floor(it.min_y);
        it.sx = it.min_x + g.below(800) * it.res;
        it.sy = it.min_y + g.below(800) * it.res;
        for (int j = 0; j < 100; ++j) {
            const int a = g.below(8);   // 0, 45, 90, ... degrees
            check(it, tc[a], ts[a], 1.0, 0.0, g.below(600) * it.res, ints);
        }
    }
    // D. NaN and infinite ranges; E. ranges that put |q| past 2^31
    const double inf = std::numeric_limits<double>::infinity();
    const double kWild[] = { std::numeric_limits<double>::quiet_NaN(), inf, -inf };
    for (long long n = 0; n < 5000 * scale; ++n) {
        Item it = random_item(g, 1e-9);
        for (int j = 0; j < 100; ++j) {
            const int a = g.below(NT), b = g.below(NT);
            check(it, tc[a], ts[a], tc[b], ts[b], kWild[g.below(3)], wild);
            check(it, tc[a], ts[a], tc[b], ts[b], (g.below(2) ? 1.0 : -1.0) * exp(g.range(log(2.2e8), log(1e300))), big);
        }
        it.sx = (g.below(2) ? 1.0 : -1.0) * exp(g.range(log(2.2e8), log(1e300)));   // a pose past 2^31 cells
        for (int j = 0; j < 20; ++j) {
            const int a = g.below(NT), b = g.below(NT);
            check(it, tc[a], ts[a], tc[b], ts[b], g.range(0.0, 30.0), big);
        }
    }
    // floor_divmod22 against integer division
    long long dm_cases = 0, dm_bad = 0;
    for (long long n = 0; n < 2000000 * scale; ++n) {
        const int b = (n & 1) ? 1 + g.below(64) : 1 + g.below(1 << 12);
        int a = g.below(1 << 23) - (1 << 22) + 1;   // (-2^22, 2^22)
        if ((n & 15) == 0) a = (g.below(1 << 10) - (1 << 9)) * b + g.below(3) - 1;   // around multiples of b
        if (a <= -(1 << 22) || a >= (1 << 22)) continue;
        int q, r;
        lgs_fast::floor_divmod22(a, b, 1.0f / (float)b, q, r);
        const int qe = (a >= 0) ? a / b : -((-a + b - 1) / b);
        ++dm_cases;
        if (q != qe || r != a - qe * b) ++dm_bad;
    }

    const long long bad = rnd.bad + edge.bad + ints.bad + wild.bad + big.bad + dm_bad;
    printf("{\"random\": [%lld, %lld, %lld], \"edge\": [%lld, %lld, %lld], \"ints\": [%lld, %lld, %lld], "
           "\"wild\": [%lld, %lld, %lld], \"big\": [%lld, %lld, %lld], \"divmod\": [%lld, %lld], \"bad\": %lld}\n",
           rnd.cases, rnd.certain, rnd.bad, edge.cases, edge.certain, edge.bad, ints.cases, ints.certain, ints.bad,
           wild.cases, wild.certain, wild.bad, big.cases, big.certain, big.bad, dm_cases, dm_bad, bad);
    for (const Bad& b : g_bad)
        fprintf(stderr, "violation: sx %.17g sy %.17g min %.17g %.17g res %.17g ct %.17g st %.17g ca %.17g sa %.17g r %.17g\n",
                b.v[0], b.v[1], b.v[2], b.v[3], b.v[4], b.v[5], b.v[6], b.v[7], b.v[8], b.v[9]);
    return bad ? 1 : 0;
}
