// icp_window_host_check.cpp -- the host-only code of lgs_icp_ref_window_scores
// and lgs_loop_detect_icp (my-lidar-graph-slam_amd/csrc/icp_window_host.hpp) in
// a program of its own, built with -fsanitize=address,undefined: the window's
// checks, index <-> (ix, iy, it) at every cap, the lattice pose, the slice plan,
// the combine of the workgroups' partials against brute force (ties, NaN and
// +inf included) and the record against a byte-wise restatement.  Prints one
// line per check; exit status 1 if any check fails.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "icp_window_host.hpp"

namespace {

int g_failed = 0;

void check(bool ok, const std::string& name, const std::string& detail = "")
{
    std::printf("[%s] %s%s%s\n", ok ? " OK " : "FAIL", name.c_str(), detail.empty() ? "" : ": ", detail.c_str());
    if (!ok) ++g_failed;
}

struct Rng {
    uint64_t s;
    uint64_t next()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return s >> 33;
    }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    double uni() { return (double)next() * 0x1p-31; }
};

using namespace lgs;

const double kInf = std::numeric_limits<double>::infinity();
const double kNan = std::numeric_limits<double>::quiet_NaN();

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

// ---- the window's rules
void window_rules()
{
    lgs_icp_window w{ 2, 2, 1, 0.05, 0.02 };
    check(icp_window_check(&w) == LGS_OK && icp_window_check(nullptr) == LGS_ERR_INVALID_ARG,
          "window: a legal window passes, null does not");
    bool ok = true;
    for (int axis = 0; axis < 3; ++axis)
        for (int v : { -1, 513, std::numeric_limits<int>::max(), std::numeric_limits<int>::min() }) {
            lgs_icp_window b{ 0, 0, 0, 0.05, 0.02 };
            (axis == 0 ? b.half_x : axis == 1 ? b.half_y : b.half_theta) = v;
            ok = ok && icp_window_check(&b) == LGS_ERR_INVALID_ARG;
            (axis == 0 ? b.half_x : axis == 1 ? b.half_y : b.half_theta) = 512;
            ok = ok && icp_window_check(&b) == LGS_OK;
        }
    check(ok, "window: a half of -1, 513, INT_MAX or INT_MIN is refused on every axis, 512 passes");
    ok = true;
    for (double s : { 0.0, -0.0, -1.0, kInf, -kInf, kNan }) {
        lgs_icp_window a = w, b = w;
        a.step_xy = s;
        b.step_theta = s;
        ok = ok && icp_window_check(&a) == LGS_ERR_INVALID_ARG && icp_window_check(&b) == LGS_ERR_INVALID_ARG;
    }
    lgs_icp_window tiny = w;
    tiny.step_xy = tiny.step_theta = std::numeric_limits<double>::denorm_min();
    check(ok && icp_window_check(&tiny) == LGS_OK, "window: a step of 0, -0, -1, +-inf or NaN is refused, the smallest positive passes");
    const lgs_icp_window at_cap{ 512, 511, 0, 0.1, 0.1 }, over{ 512, 512, 0, 0.1, 0.1 }, cube{ 50, 50, 50, 0.1, 0.1 },
        cube_over{ 51, 50, 50, 0.1, 0.1 }, all{ 512, 512, 512, 0.1, 0.1 };
    check(icp_window_check(&at_cap) == LGS_OK && icp_window_dims(at_cap).P == 1048575 &&
              icp_window_check(&over) == LGS_ERR_INVALID_ARG && icp_window_check(&cube) == LGS_OK &&
              icp_window_dims(cube).P == 1030301 && icp_window_check(&cube_over) == LGS_ERR_INVALID_ARG &&
              icp_window_check(&all) == LGS_ERR_INVALID_ARG,
          "window: 1025 x 1023 and 101^3 poses pass, 1025 x 1025, 103 x 101 x 101 and 1025^3 do not");
}

// ---- index <-> (ix, iy, it), the slices
void index_and_slices()
{
    const lgs_icp_window ws[] = { { 0, 0, 0, 1, 1 },   { 512, 0, 0, 1, 1 },  { 0, 512, 0, 1, 1 },  { 0, 0, 512, 1, 1 },
                                  { 512, 511, 0, 1, 1 }, { 0, 511, 512, 1, 1 }, { 50, 50, 50, 1, 1 }, { 2, 2, 1, 1, 1 },
                                  { 10, 10, 10, 1, 1 }, { 31, 0, 3, 1, 1 },  { 32, 0, 3, 1, 1 },  { 5, 5, 3, 1, 1 } };
    bool round = true, order = true, cover = true, plan = true;
    for (const lgs_icp_window& w : ws) {
        const IcpWinDims d = icp_window_dims(w);
        int p = 0;
        for (int it = 0; it < d.nt; ++it)
            for (int iy = 0; iy < d.ny; ++iy)
                for (int ix = 0; ix < d.nx; ++ix, ++p) {
                    order = order && icp_window_index(d, ix, iy, it) == p;   // theta outermost, x innermost
                    int ax, ay, at;
                    icp_window_decode(d, p, ax, ay, at);
                    round = round && ax == ix && ay == iy && at == it;
                }
        round = round && p == d.P;
        for (int cands : { 1, 2, 5, 64, 4096, 1 << 20 }) {
            const IcpWinPlan pl = icp_window_plan(d, cands);
            std::vector<int> seen((size_t)d.nx * d.ny, 0);
            for (int s = 0; s < pl.slices; ++s) {
                int t0, t1;
                icp_window_slice(d, pl, s, t0, t1);
                cover = cover && t0 < t1 && t1 - t0 <= pl.slice_len && t1 <= d.nx * d.ny;
                for (int t = t0; t < t1 && t < d.nx * d.ny; ++t) ++seen[(size_t)t];
            }
            for (int v : seen) cover = cover && v == 1;
            const int in_launch = cands < pl.chunk_cands ? cands : pl.chunk_cands;
            plan = plan && pl.groups == d.nt * pl.slices && pl.chunk_cands >= 64 &&
                   pl.chunk_cands == icp_window_chunk_cands(d) && (long long)pl.chunk_cands * d.P <= kIcpWinChunkPoses &&
                   (long long)in_launch * pl.groups < (1ll << 31) && pl.slice_len >= kIcpWinSliceMin &&
                   pl.slice_len <= kIcpWinSlice && (pl.slice_len & (pl.slice_len - 1)) == 0;
            // a slice is as long as the target of workgroups allows
            if (pl.slice_len < kIcpWinSlice) {
                const int longer = (d.nx * d.ny + 2 * pl.slice_len - 1) / (2 * pl.slice_len);
                plan = plan && (long long)cands * d.nt * longer < kIcpWinTargetGroups;
            }
            if (pl.slice_len > kIcpWinSliceMin) plan = plan && (long long)cands * pl.groups >= kIcpWinTargetGroups;
        }
    }
    check(round, "index: decode(index(ix, iy, it)) is the identity over whole windows, every cap included");
    check(order, "index: theta outermost, x innermost");
    check(cover, "slices: every translation in exactly one slice, none empty, none above the plan's length");
    check(plan, "plan: at least 64 candidates and at most 2^26 poses per launch, fewer than 2^31 workgroups, the longest slice that fills the device");
}

// ---- the lattice pose
void lattice_pose()
{
    const lgs_icp_window w{ 2, 3, 1, 0.1, 0.05 };
    const lgs_pose2d c{ -0.0, 1e5 + 0.3, -0.2 };
    const lgs_pose2d at = icp_window_pose(w, c, 2, 3, 1);
    check(std::memcmp(&at, &c, sizeof(c)) == 0 && std::signbit(at.x), "pose: the centre index gives the centre, -0.0 included");
    bool ok = true;
    for (int it = 0; it < 3; ++it)
        for (int iy = 0; iy < 7; ++iy)
            for (int ix = 0; ix < 5; ++ix) {
                const lgs_pose2d p = icp_window_pose(w, c, ix, iy, it);
                // the product and the sum rounded separately
                volatile double mx = (double)(ix - 2) * 0.1, my = (double)(iy - 3) * 0.1, mt = (double)(it - 1) * 0.05;
                volatile double sx = c.x + mx, sy = c.y + my, st = c.theta + mt;
                ok = ok && (ix == 2 || same_bits(p.x, sx)) && (iy == 3 || same_bits(p.y, sy)) &&
                     (it == 1 || same_bits(p.theta, st));
                const lgs_pose2d q = icp_window_pose_of(w, c, icp_window_index(icp_window_dims(w), ix, iy, it));
                ok = ok && std::memcmp(&p, &q, sizeof(p)) == 0;
            }
    check(ok, "pose: c + (double)(i - half) * step per coordinate, by index and by (ix, iy, it)");
    const lgs_icp_window big{ 512, 512, 0, 1e305, 1.0 };
    check(icp_window_finite(w, c) && !icp_window_finite(w, { kNan, 0, 0 }) && !icp_window_finite(w, { 0, kInf, 0 }) &&
              !icp_window_finite(w, { 0, 0, -kInf }) && !icp_window_finite(big, { 1.7e308, 0, 0 }) &&
              icp_window_finite(big, { 0, 0, 0 }),
          "pose: a centre or an outermost pose that is not finite is seen");
}

// ---- the combine against brute force
IcpWinPartial brute(const std::vector<double>& cost, const std::vector<int>& pairs, const std::vector<int>& idx)
{
    IcpWinPartial b{ kInf, -1, 0 };
    for (int p : idx)
        if (cost[(size_t)p] < b.cost || (cost[(size_t)p] == b.cost && p < b.p)) b = { cost[(size_t)p], p, pairs[(size_t)p] };
    return b;
}

void combine()
{
    Rng rng{ 777 };
    bool ok = true;
    int with_ties = 0, none = 0;
    for (int trial = 0; trial < 400; ++trial) {
        const int P = 1 + rng.below(200);
        std::vector<double> cost((size_t)P);
        std::vector<int> pairs((size_t)P), all((size_t)P);
        const int mode = trial % 4;   // 0: distinct, 1: few values (ties), 2: with NaN and +inf, 3: only NaN and +inf
        for (int p = 0; p < P; ++p) {
            all[(size_t)p] = p;
            pairs[(size_t)p] = rng.below(100);
            double v = mode == 0 ? rng.uni() : (double)rng.below(3);
            if (mode == 2 && rng.below(3) == 0) v = rng.below(2) ? kNan : kInf;
            if (mode == 3) v = rng.below(2) ? kNan : kInf;
            cost[(size_t)p] = v;
        }
        // groups in a random order, each a random subset: what workgroups report, in whatever order
        const int G = 1 + rng.below(12);
        std::vector<std::vector<int>> groups((size_t)G);
        for (int p = P - 1; p >= 0; --p) groups[(size_t)rng.below(G)].push_back(p);
        std::vector<IcpWinPartial> parts;
        for (const auto& g : groups) parts.push_back(brute(cost, pairs, g));
        const IcpWinPartial want = brute(cost, pairs, all), got = icp_window_combine(parts.data(), parts.size());
        ok = ok && got.p == want.p && got.pairs == want.pairs && (want.p < 0 || same_bits(got.cost, want.cost));
        if (want.p < 0) {
            ++none;
            ok = ok && mode >= 2 && got.pairs == 0 && got.cost == kInf;   // a short mode-2 trial may hold nothing else either
        } else {
            int ties = 0;
            for (int p = 0; p < P; ++p) ties += cost[(size_t)p] == want.cost ? 1 : 0;
            with_ties += ties > 1 ? 1 : 0;
            for (int p = 0; p < want.p; ++p) ok = ok && !(cost[(size_t)p] <= want.cost);   // the lowest index of the minimum
        }
    }
    check(ok && with_ties >= 50 && none >= 100, "combine: the lexicographic minimum of brute force over 400 random partitions",
          std::to_string(with_ties) + " with ties, " + std::to_string(none) + " with nothing but NaN and +inf");
    check(icp_window_combine(nullptr, 0).p == -1 && !icp_window_better(kNan, 0, kInf, -1) &&
              !icp_window_better(kInf, 0, kInf, -1) && icp_window_better(1e308, 5, kInf, -1) &&
              icp_window_better(1.0, 2, 1.0, 3) && !icp_window_better(1.0, 3, 1.0, 2) && !icp_window_better(1.0, 3, 1.0, 3),
          "combine: nothing wins from no partial; NaN and +inf never win; a tie goes to the lower index");
}

// ---- the record
void record()
{
    lgs_loop_query Q{};
    Q.local_map_node_pose = { 0.4, -0.3, 0.7 };
    Q.local_map_node_index = 17;
    Q.first_candidate = 3;
    Q.num_candidates = 9;
    lgs_loop_candidate c{};
    c.node_pose = { 9.0, 9.0, 9.0 };
    c.node_index = 123;
    lgs_icp_summary s;
    std::memset(&s, 0, sizeof(s));
    s.pose_found = 1;
    s.num_pairs = 57;
    s.normalized_cost = 0.0123;
    s.estimated_pose = { 1.25, -0.75, 0.31 };
    for (int k = 0; k < 9; ++k) s.covariance[k] = 0.01 * (k + 1);
    bool ok = true;
    for (int mode = 0; mode < 3; ++mode) {   // no refine, rejected, accepted
        lgs_loop_result got;
        std::memset(&got, 0xAB, sizeof(got));
        icp_window_record(got, Q, c, mode == 0 ? nullptr : &s, mode == 2, 65);
        unsigned char want[sizeof(lgs_loop_result)];
        std::memset(want, 0, sizeof(want));
        const int found = mode == 2 ? 1 : 0;
        std::memcpy(want + offsetof(lgs_loop_result, start_node_index), &Q.local_map_node_index, 4);
        std::memcpy(want + offsetof(lgs_loop_result, end_node_index), &c.node_index, 4);
        std::memcpy(want + offsetof(lgs_loop_result, start_node_pose), &Q.local_map_node_pose, 24);
        if (mode > 0) {
            std::memcpy(want + offsetof(lgs_loop_result, found), &found, 4);
            std::memcpy(want + offsetof(lgs_loop_result, estimated_pose), &s.estimated_pose, 24);
            std::memcpy(want + offsetof(lgs_loop_result, covariance), s.covariance, 72);
            volatile double score = 57.0 / 65.0;
            const double sc = score;
            std::memcpy(want + offsetof(lgs_loop_result, score), &sc, 8);
            std::memcpy(want + offsetof(lgs_loop_result, normalized_cost), &s.normalized_cost, 8);
        }
        if (mode == 2) {
            // InverseCompound(localMapNode.Pose(), estimatedPose), glibc's sincos
            double sn, cs;
            sincos(0.7, &sn, &cs);
            const double dx = 1.25 - 0.4, dy = -0.75 - -0.3;
            const lgs_pose2d rel{ cs * dx + sn * dy, -sn * dx + cs * dy, 0.31 - 0.7 };
            std::memcpy(want + offsetof(lgs_loop_result, relative_pose), &rel, 24);
        }
        ok = ok && std::memcmp(&got, want, sizeof(want)) == 0;
    }
    check(ok && sizeof(lgs_loop_result) == 176, "record: all 176 bytes equal the restatement: no refine, rejected, accepted");
}

}  // namespace

int main()
{
    window_rules();
    index_and_slices();
    lattice_pose();
    combine();
    record();
    std::printf(g_failed ? "%d CHECK(S) FAILED\n" : "ICP WINDOW HOST CHECKS PASSED\n", g_failed);
    return g_failed ? 1 : 0;
}
