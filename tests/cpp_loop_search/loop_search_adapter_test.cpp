// loop_search_adapter_test.cpp -- LoopSearcherNearestHip, LoopGraphHip and
// GetLoopDetectionQueries (my-lidar-graph-slam_amd/host/lgs_slam_hip.hpp) on
// the GPU: a 12-node trajectory whose last four nodes come back to the first
// two local maps.  Search (the host loop), SearchBatch and SearchAllMaps (the
// device) against brute force written out here, and end to end: SearchAllMaps
// -> GetLoopDetectionQueries -> LoopDetectorGridSearchHip::Detect gives the
// loop records of the same queries written by hand.  Prints one line per
// check; exit status 1 if any check fails, 77 without a GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "lgs_slam_hip.hpp"

using namespace MyLidarGraphSlam::Hip;

namespace {

int g_failed = 0;

void check(bool ok, const std::string& name, const std::string& detail = "")
{
    std::printf("[%s] %s%s%s\n", ok ? " OK " : "FAIL", name.c_str(), detail.empty() ? "" : ": ", detail.c_str());
    if (!ok) ++g_failed;
}

struct Seg { double x0, y0, x1, y1; };

// a room with a few boxes away from the trajectory
std::vector<Seg> make_world()
{
    const double h = 6.0;
    std::vector<Seg> s = { { -h, -h, h, -h }, { h, -h, h, h }, { h, h, -h, h }, { -h, h, -h, -h } };
    const double boxes[5][4] = { { 3.0, 2.0, 1.0, 0.6 }, { -3.5, 1.0, 0.8, 1.4 }, { 2.5, -3.0, 1.2, 0.7 },
                                 { -2.0, -3.5, 0.9, 0.9 }, { 0.0, 4.0, 1.6, 0.5 } };
    for (const auto& b : boxes) {
        const double x0 = b[0] - b[2] / 2, x1 = b[0] + b[2] / 2, y0 = b[1] - b[3] / 2, y1 = b[1] + b[3] / 2;
        s.push_back({ x0, y0, x1, y0 });
        s.push_back({ x1, y0, x1, y1 });
        s.push_back({ x1, y1, x0, y1 });
        s.push_back({ x0, y1, x0, y0 });
    }
    return s;
}

std::vector<double> beam_angles(int n)
{
    const double fov = 270.0 * M_PI / 180.0;
    std::vector<double> a((size_t)n);
    for (int i = 0; i < n; ++i) a[(size_t)i] = -fov / 2 + i * (fov / (n - 1));
    return a;
}

std::vector<double> ray_cast(const std::vector<Seg>& w, const RobotPose2D<double>& p, const std::vector<double>& ang)
{
    std::vector<double> r(ang.size(), 30.0);
    for (std::size_t i = 0; i < ang.size(); ++i) {
        const double dx = std::cos(p.mTheta + ang[i]), dy = std::sin(p.mTheta + ang[i]);
        for (const Seg& s : w) {
            const double ex = s.x1 - s.x0, ey = s.y1 - s.y0;
            const double den = dx * ey - dy * ex;
            if (std::fabs(den) < 1e-12) continue;
            const double t = ((s.x0 - p.mX) * ey - (s.y0 - p.mY) * ex) / den;
            const double u = ((s.x0 - p.mX) * dy - (s.y0 - p.mY) * dx) / den;
            if (t > 0 && u >= 0 && u <= 1 && t < r[i]) r[i] = t;
        }
    }
    return r;
}

bool same_candidates(const LoopCandidateVector& a, const LoopCandidateVector& b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].mNodeIndices != b[i].mNodeIndices || a[i].mLocalMapIdx != b[i].mLocalMapIdx ||
            a[i].mLocalMapNodeIdx != b[i].mLocalMapNodeIdx)
            return false;
    return true;
}

bool same_bits(const RobotPose2D<double>& a, const RobotPose2D<double>& b)
{
    return std::memcmp(&a.mX, &b.mX, 8) == 0 && std::memcmp(&a.mY, &b.mY, 8) == 0 &&
           std::memcmp(&a.mTheta, &b.mTheta, 8) == 0;
}

}  // namespace

int main()
{
    std::shared_ptr<Device> dev;
    try {
        dev = std::make_shared<Device>(0);
    } catch (const Error& e) {
        std::printf("no GPU: %s\n", e.what());
        return 77;   // skip: the adapter and the C-ABI loaded, there is no device to run on
    }
    const auto world = make_world();
    const auto ang = beam_angles(181);

    // nodes 0 .. 7 go along an arc (maps 0 and 1), nodes 8 .. 11 (the latest map) come back along it
    std::vector<RobotPose2D<double>> poses;
    for (int k = 0; k < 8; ++k) {
        const double phi = -0.6 + 0.24 * k;
        poses.push_back({ std::cos(phi), std::sin(phi), phi + M_PI / 2 });
    }
    for (int k = 0; k < 4; ++k) {
        const double phi = -0.5 + 0.45 * k;
        poses.push_back({ 1.05 * std::cos(phi), 1.05 * std::sin(phi), phi + M_PI / 2 + 0.02 });
    }
    const int n = (int)poses.size();
    const std::vector<LocalMapNodeRange> ranges = { { 0, 3 }, { 4, 7 }, { 8, 11 } };
    std::vector<LoopCandidateNode> nodes;
    for (int k = 0; k < n; ++k)
        nodes.push_back({ std::make_shared<ScanData>(dev, ang, ray_cast(world, poses[(size_t)k], ang)), poses[(size_t)k], k });
    const GridMapBuilderParams bp;
    std::vector<std::unique_ptr<GridMapHip>> maps;
    std::vector<DeviceGridPtr> grids;
    for (int i = 0; i < 2; ++i) {
        std::vector<ScanDataPtr> sc;
        std::vector<RobotPose2D<double>> ps;
        for (int k = ranges[(size_t)i].mPoseGraphNodeIdxMin; k <= ranges[(size_t)i].mPoseGraphNodeIdxMax; ++k) {
            sc.push_back(nodes[(size_t)k].mScanData);
            ps.push_back(poses[(size_t)k]);
        }
        maps.push_back(std::make_unique<GridMapHip>(dev, 0.05, 64, 64, 64));
        maps.back()->ConstructMapFromScans(sc, ps, bp);
        grids.push_back(maps.back()->Grid());
    }
    grids.push_back(nullptr);   // the latest map is never a candidate

    // accumTravelDist when node k was the latest one
    std::vector<double> accum((size_t)n, 0.0);
    std::vector<lgs_pose2d> cp;
    for (const auto& p : poses) cp.push_back({ p.mX, p.mY, p.mTheta });
    bool acc_ok = true;
    for (int k = 0; k < n; ++k) acc_ok = acc_ok && lgs_pg_accum_travel_dist(cp.data(), k + 1, &accum[(size_t)k]) == LGS_OK;
    check(acc_ok && accum[0] == 0.0 && accum[(size_t)n - 1] > accum[1], "lgs_pg_accum_travel_dist over every prefix");

    const double travelThr = 0.5, nodeThr = 0.35;
    const int K = 1;
    const LoopSearcherNearestHip searcher(travelThr, nodeThr, K);
    std::vector<LoopSearchBatchHint> hints;
    for (int k = 8; k < n; ++k) hints.push_back({ k, 2, 3, accum[(size_t)k] });

    // brute force: per hint and finished map the nearest node inside the threshold (lowest node on ties)
    const double thrSq = nodeThr * nodeThr;
    std::vector<LoopCandidateVector> all_expect, one_expect;
    for (const auto& h : hints) {
        LoopCandidateVector all, one;
        double best = thrSq;
        std::vector<int> idx;
        for (int k = std::max(8, h.mLatestNodeIdx - K); k <= std::min(11, h.mLatestNodeIdx + K); ++k) idx.push_back(k);
        for (int i = 0; i < 2; ++i) {
            double mb = thrSq;
            int mk = -1;
            for (int k = ranges[(size_t)i].mPoseGraphNodeIdxMin; k <= ranges[(size_t)i].mPoseGraphNodeIdxMax; ++k) {
                // (the travel cut never falls inside maps 0 and 1 here: accum - travel >= 0.5 for every hint)
                const double dx = poses[(size_t)k].mX - poses[(size_t)h.mLatestNodeIdx].mX,
                             dy = poses[(size_t)k].mY - poses[(size_t)h.mLatestNodeIdx].mY;
                const double d2 = dx * dx + dy * dy;
                if (d2 < mb) {
                    mb = d2;
                    mk = k;
                }
            }
            if (mk < 0) continue;
            all.push_back({ idx, i, mk });
            if (mb < best) {
                best = mb;
                one.assign(1, LoopCandidate{ idx, i, mk });
            }
        }
        all_expect.push_back(all);
        one_expect.push_back(one);
    }
    size_t near_maps = 0, two = 0;
    for (const auto& v : all_expect) {
        near_maps += v.size();
        two += v.size() == 2;
    }

    // Search: the host loop, one hint with its own snapshot
    bool ok = true;
    for (size_t j = 0; j < hints.size(); ++j) {
        LoopSearchHint h;
        h.mPoseGraphNodes = poses;
        h.mLocalMapPositions = ranges;
        h.mAccumTravelDist = hints[j].mAccumTravelDist;
        h.mLatestNodeIdx = hints[j].mLatestNodeIdx;
        h.mLatestLocalMapIdx = 2;
        ok = ok && same_candidates(searcher.Search(h), one_expect[j]);
    }
    check(ok, "LoopSearcherNearestHip::Search == brute force", std::to_string(hints.size()) + " hints");

    // SearchBatch / SearchAllMaps: the device (the pairs threshold off, so that four hints launch)
    dev->Check(lgs_ctx_set_option(dev->Handle(), LGS_OPT_LOOP_SEARCH_MIN_PAIRS, 0.0), "lgs_ctx_set_option");
    const LoopGraphHip graph(dev, poses, ranges);
    const std::vector<LoopCandidateVector> batch = searcher.SearchBatch(graph, hints);
    const std::vector<LoopCandidateVector> all = searcher.SearchAllMaps(graph, hints);
    ok = batch.size() == hints.size() && all.size() == hints.size();
    for (size_t j = 0; ok && j < hints.size(); ++j)
        ok = same_candidates(batch[j], one_expect[j]) && same_candidates(all[j], all_expect[j]);
    long long st[4] = {};
    lgs_loop_search_stats(dev->Handle(), st);
    check(ok && near_maps >= 4 && two >= 1 && st[0] == 2 && st[1] == 0,
          "SearchBatch and SearchAllMaps on the device == brute force",
          std::to_string(near_maps) + " near maps, " + std::to_string(two) + " hints near both maps, " +
              std::to_string(st[2]) + " launches");

    // end to end: the candidates through the query helper and the grid-search loop detector
    const ScorePixelAccurateParams sf;
    const CostGreedyEndpointParams cost;
    auto matcher = std::make_shared<ScanMatcherGridSearchHip>(dev, sf, cost, 0.3, 0.3, 0.06, 0.05, 0.05, 0.01);
    LoopDetectorGridSearchHip detector(matcher, 0.4);
    LoopCandidateVector flat;
    for (const auto& v : all) flat.insert(flat.end(), v.begin(), v.end());
    std::vector<LoopDetectionQuery> queries = GetLoopDetectionQueries(flat, nodes, grids);
    std::vector<LoopDetectionQuery> by_hand;
    for (const auto& v : all_expect)
        for (const LoopCandidate& c : v) {
            LoopDetectionQuery q;
            for (int k : c.mNodeIndices) q.mPoseGraphNodes.push_back({ nodes[(size_t)k].mScanData, poses[(size_t)k], k });
            q.mLocalMap = grids[(size_t)c.mLocalMapIdx];
            q.mLocalMapNodePose = poses[(size_t)c.mLocalMapNodeIdx];
            q.mLocalMapNodeIndex = c.mLocalMapNodeIdx;
            by_hand.push_back(q);
        }
    ok = queries.size() == by_hand.size();
    for (size_t i = 0; ok && i < queries.size(); ++i) {
        ok = queries[i].mLocalMap == by_hand[i].mLocalMap && queries[i].mLocalMapNodeIndex == by_hand[i].mLocalMapNodeIndex &&
             same_bits(queries[i].mLocalMapNodePose, by_hand[i].mLocalMapNodePose) &&
             queries[i].mPoseGraphNodes.size() == by_hand[i].mPoseGraphNodes.size();
        for (size_t k = 0; ok && k < queries[i].mPoseGraphNodes.size(); ++k)
            ok = queries[i].mPoseGraphNodes[k].mIndex == by_hand[i].mPoseGraphNodes[k].mIndex &&
                 queries[i].mPoseGraphNodes[k].mScanData == by_hand[i].mPoseGraphNodes[k].mScanData &&
                 same_bits(queries[i].mPoseGraphNodes[k].mPose, by_hand[i].mPoseGraphNodes[k].mPose);
    }
    check(ok, "GetLoopDetectionQueries == the queries written by hand", std::to_string(queries.size()) + " queries");
    std::vector<LoopDetectionResult> ra, rb;
    detector.Detect(queries, ra);
    detector.Detect(by_hand, rb);
    ok = ra.size() == rb.size() && !ra.empty();
    for (size_t i = 0; ok && i < ra.size(); ++i)
        ok = ra[i].mStartNodeIdx == rb[i].mStartNodeIdx && ra[i].mEndNodeIdx == rb[i].mEndNodeIdx &&
             same_bits(ra[i].mRelativePose, rb[i].mRelativePose) && same_bits(ra[i].mStartNodePose, rb[i].mStartNodePose) &&
             std::memcmp(ra[i].mEstimatedCovMat.m.data(), rb[i].mEstimatedCovMat.m.data(), 72) == 0;
    check(ok, "SearchAllMaps -> GetLoopDetectionQueries -> Detect == the hand-written queries' loop records",
          std::to_string(ra.size()) + " loops detected");

    bool threw = false;
    try {
        std::vector<LoopSearchBatchHint> bad = { { 3, 2, 3, 1.0 } };   // node 3 is not in the latest map
        searcher.SearchBatch(graph, bad);
    } catch (const Error& e) {
        threw = e.status == LGS_ERR_INVALID_ARG;
    }
    check(threw, "a latest node outside its latest map throws Error(LGS_ERR_INVALID_ARG)");

    std::printf(g_failed ? "LOOP SEARCH ADAPTER TESTS FAILED (%d)\n" : "LOOP SEARCH ADAPTER TESTS PASSED\n", g_failed);
    return g_failed ? 1 : 0;
}
