// icp_ref_adapter_test.cpp -- ScanMatcherIcpPointToLineHip's multi-scan
// SetReference (my-lidar-graph-slam_amd/host/lgs_slam_hip.hpp) on the GPU
// against values the caller passes in: argv[1] names a text file of
// whitespace-separated numbers (hex floats), written by
// tests/test_gpu_icp_ref.py from the Python bindings' result:
//   K n iterations_max, the 7 doubles of lgs_icp_params,
//   the scans' relative sensor pose (3), the n beam angles,
//   per reference scan: its robot pose (3) and n ranges,
//   the current scan's n ranges and the initial robot pose (3),
//   expected: pose_found, normalized_cost, estimated pose (3), covariance (9).
// The adapter's OptimizePose(query) after SetReference(scans, poses) must
// give those bytes; the one-scan SetReference must still take its own path
// and setting it must drop the multi-scan reference.  Prints one line per
// check; exit status 1 if any check fails, 77 without a GPU, 2 for a bad file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
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

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

struct Reader {
    std::ifstream in;
    bool ok = true;
    double num()
    {
        std::string t;
        if (!(in >> t)) {
            ok = false;
            return 0.0;
        }
        char* end = nullptr;
        const double v = std::strtod(t.c_str(), &end);
        if (end == t.c_str() || *end) ok = false;
        return v;
    }
    std::vector<double> nums(int n)
    {
        std::vector<double> v((size_t)n);
        for (double& x : v) x = num();
        return v;
    }
    RobotPose2D<double> pose()
    {
        const double x = num(), y = num(), th = num();
        return RobotPose2D<double>(x, y, th);
    }
};

}  // namespace

int main(int argc, char** argv)
{
    std::shared_ptr<Device> dev;
    try {
        dev = std::make_shared<Device>(0);
    } catch (const Error& e) {
        std::printf("no GPU: %s\n", e.what());
        return 77;   // skip: the adapter and the C-ABI loaded, there is no device to run on
    }
    if (argc < 2) {
        std::printf("usage: icp_ref_adapter_test <case file>\n");
        return 2;
    }
    Reader r;
    r.in.open(argv[1]);
    const int K = (int)r.num(), n = (int)r.num();
    IcpPointToLineParams prm;
    prm.mNumOfIterationsMax = (int)r.num();
    prm.mConvergenceThreshold = r.num();
    prm.mUsableRangeMin = r.num();
    prm.mUsableRangeMax = r.num();
    prm.mTranslationRegularizer = r.num();
    prm.mRotationRegularizer = r.num();
    prm.mMaxCorrespondenceDist = r.num();
    prm.mMaxSegmentLength = r.num();
    if (!r.ok || K < 1 || K > 64 || n < 1 || n > 100000) {
        std::printf("bad case file\n");
        return 2;
    }
    const RobotPose2D<double> rel = r.pose();
    const std::vector<double> ang = r.nums(n);
    std::vector<ScanDataPtr> refs;
    std::vector<RobotPose2D<double>> poses;
    for (int k = 0; k < K; ++k) {
        poses.push_back(r.pose());
        refs.push_back(std::make_shared<ScanData>(dev, ang, r.nums(n), rel));
    }
    const ScanDataPtr cur = std::make_shared<ScanData>(dev, ang, r.nums(n), rel);
    const RobotPose2D<double> init = r.pose();
    const bool found = r.num() != 0.0;
    const double ncost = r.num();
    const RobotPose2D<double> est = r.pose();
    const std::vector<double> cov = r.nums(9);
    if (!r.ok) {
        std::printf("bad case file\n");
        return 2;
    }

    ScanMatcherIcpPointToLineHip matcher(dev, prm);
    matcher.SetReference(refs, poses);
    refs.clear();   // the reference keeps what it needs
    const ScanMatchingSummary a = matcher.OptimizePose(ScanMatchingQuery(nullptr, cur, init));
    bool ok = a.mPoseFound == found && same_bits(a.mNormalizedCost, ncost) && same_bits(a.mEstimatedPose.mX, est.mX) &&
              same_bits(a.mEstimatedPose.mY, est.mY) && same_bits(a.mEstimatedPose.mTheta, est.mTheta) &&
              same_bits(a.mInitialPose.mX, init.mX) && same_bits(a.mInitialPose.mY, init.mY) &&
              same_bits(a.mInitialPose.mTheta, init.mTheta);
    for (int k = 0; k < 9; ++k) ok = ok && same_bits(a.mEstimatedCovariance.m[k], cov[(size_t)k]);
    check(ok, "SetReference(scans, poses) + OptimizePose(query) == the values passed in",
          std::to_string(K) + " scans of " + std::to_string(n) + " beams, " + std::to_string(matcher.LastSummary().num_pairs) +
              " pairs");
    const ScanMatchingSummary b = matcher.OptimizePose(ScanMatchingQuery(nullptr, cur, init));
    check(same_bits(b.mNormalizedCost, a.mNormalizedCost) && same_bits(b.mEstimatedPose.mX, a.mEstimatedPose.mX),
          "a second query gives the same bytes");

    // the one-scan SetReference keeps its own path and replaces the set
    const ScanDataPtr one = std::make_shared<ScanData>(dev, ang, cur->Ranges(), rel);
    matcher.SetReference(one, poses[0]);
    const ScanMatchingSummary c = matcher.OptimizePose(ScanMatchingQuery(nullptr, cur, init));
    lgs_icp_summary cabi;
    std::memset(&cabi, 0, sizeof(cabi));
    const int rc = lgs_icp_optimize_pose(dev->Handle(), one->Handle(), { poses[0].mX, poses[0].mY, poses[0].mTheta },
                                         cur->Handle(), { init.mX, init.mY, init.mTheta }, &matcher.Params(), &cabi, nullptr);
    check(rc == LGS_OK && std::memcmp(&matcher.LastSummary(), &cabi, sizeof(cabi)) == 0 &&
              same_bits(c.mNormalizedCost, cabi.normalized_cost),
          "SetReference(scan, pose) afterwards == lgs_icp_optimize_pose's bytes");

    bool threw = false;
    try {
        matcher.SetReference(std::vector<ScanDataPtr>{}, std::vector<RobotPose2D<double>>{});
    } catch (const Error& e) {
        threw = e.status == LGS_ERR_INVALID_ARG;
    }
    check(threw, "an empty set throws Error(LGS_ERR_INVALID_ARG)");

    std::printf(g_failed ? "ICP REF ADAPTER TESTS FAILED (%d)\n" : "ICP REF ADAPTER TESTS PASSED\n", g_failed);
    return g_failed ? 1 : 0;
}
