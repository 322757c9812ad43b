// pglm_adapter_test.cpp -- PoseGraphOptimizerLM
// (my-lidar-graph-slam_amd/host/lgs_posegraph.hpp) constructed with a Device
// and DevicePath::Resident against the same optimizer with
// DevicePath::SolveOnly: a pose graph built through PoseGraph::AppendNode /
// AppendEdge (a noisy odometry chain around a closed trajectory, loop edges,
// two outliers) is optimized by both.  The resident path forms the host's
// system byte for byte, so step count, damping factor, CG passes and poses
// are equal bitwise (Huber, Cauchy, Squared), the total error too where the
// loss is IEEE-only (Huber, Squared; Cauchy's log1p: 1e-9 relative).  A
// resident optimizer refuses SolverType::SparseCholesky and a loss of the
// caller's own.  Prints one line per check; exit status 1 if any check fails,
// 77 without a GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "lgs_posegraph.hpp"

using namespace MyLidarGraphSlam::Hip;
using Mapping::PoseGraph;
using Mapping::PoseGraphOptimizerLM;

namespace {

int g_failed = 0;

void check(bool ok, const std::string& name, const std::string& detail = "")
{
    std::printf("[%s] %s%s%s\n", ok ? " OK " : "FAIL", name.c_str(), detail.empty() ? "" : ": ", detail.c_str());
    if (!ok) ++g_failed;
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

Matrix3d information(double xy, double th)
{
    Matrix3d m;
    m.m[0] = m.m[4] = xy;
    m.m[8] = th;
    return m;
}

PoseGraph make_graph(int n, int loops, int outliers, unsigned seed)
{
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> gauss(0.0, 1.0);
    std::uniform_int_distribution<int> node(0, n - 1);
    std::uniform_real_distribution<double> wild(-2.0, 2.0);
    std::vector<RobotPose2D<double>> truth;
    for (int i = 0; i < n; ++i) {
        const double t = 2.0 * M_PI * i / n;
        truth.emplace_back(5.0 * std::cos(t), 3.0 * std::sin(t), t + M_PI / 2.0);
    }
    auto rel = [&](int a, int b) {
        RobotPose2D<double> d = Mapping::InverseCompound(truth[a], truth[b]);
        d.mTheta = Mapping::NormalizeAngle(d.mTheta);
        return d;
    };
    PoseGraph g;
    RobotPose2D<double> pose = truth[0];
    g.AppendNode(pose, 0.0);
    for (int i = 0; i + 1 < n; ++i) {
        RobotPose2D<double> z = rel(i, i + 1);
        z = RobotPose2D<double>(z.mX + 0.01 * gauss(rng), z.mY + 0.01 * gauss(rng), z.mTheta + 0.005 * gauss(rng));
        g.AppendEdge(i, i + 1, z, information(100.0, 400.0));
        pose = Mapping::Compound(pose, RobotPose2D<double>(z.mX + 0.05 * gauss(rng), z.mY + 0.05 * gauss(rng),
                                                           z.mTheta + 0.01 * gauss(rng)));
        g.AppendNode(pose, 0.1 * (i + 1));
    }
    for (int k = 0; k < loops + outliers; ++k) {
        int a = node(rng), b = node(rng);
        while (b == a) b = node(rng);
        if (k < loops)
            g.AppendEdge(a, b, rel(a, b), information(200.0, 800.0));
        else
            g.AppendEdge(a, b, RobotPose2D<double>(wild(rng), wild(rng), wild(rng)), information(100.0, 400.0));
    }
    return g;
}

bool poses_same_bits(const std::vector<PoseGraph::Node>& a, const std::vector<PoseGraph::Node>& b)
{
    bool ok = a.size() == b.size();
    for (std::size_t i = 0; ok && i < a.size(); ++i)
        ok = same_bits(a[i].Pose().mX, b[i].Pose().mX) && same_bits(a[i].Pose().mY, b[i].Pose().mY) &&
             same_bits(a[i].Pose().mTheta, b[i].Pose().mTheta);
    return ok;
}

// a loss the library does not know: Kind() stays -1
class LossOfMyOwn final : public Mapping::LossFunction {
public:
    double Loss(double t) const override { return 0.5 * t; }
    double Weight(double) const override { return 0.5; }
};

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
    using Solver = PoseGraphOptimizerLM::SolverType;
    using Path = PoseGraphOptimizerLM::DevicePath;
    const PoseGraph graph = make_graph(200, 25, 2, 11);

    for (int kind : { 0, 1, 6 }) {   // Huber, Cauchy, Squared
        const std::string tag = "loss " + std::to_string(kind);
        PoseGraphOptimizerLM solve(dev, Solver::ConjugateGradient, 10, 1e-6, 1e-3, Mapping::CreateLossFunction(kind, 1.0));
        PoseGraphOptimizerLM resident(dev, Solver::ConjugateGradient, 10, 1e-6, 1e-3, Mapping::CreateLossFunction(kind, 1.0),
                                      Path::Resident);
        std::vector<PoseGraph::Node> a = graph.Nodes(), b = graph.Nodes();
        solve.Optimize(a, graph.Edges());
        resident.Optimize(b, graph.Edges());
        check(resident.LastIterations() == solve.LastIterations() && same_bits(resident.Lambda(), solve.Lambda()) &&
                  resident.LastSolverIterations() == solve.LastSolverIterations() && resident.LastSolverIterations() > 0,
              tag + ": the resident Optimize takes SolveOnly's LM steps and CG passes and leaves its damping factor",
              std::to_string(resident.LastIterations()) + " steps, " + std::to_string(resident.LastSolverIterations()) +
                  " CG passes");
        check(poses_same_bits(a, b), tag + ": poses equal bitwise");
        if (kind == 1)
            check(std::fabs(resident.LastTotalError() - solve.LastTotalError()) <= 1e-9 * std::fabs(solve.LastTotalError()),
                  tag + ": total error within 1e-9 relative");
        else
            check(same_bits(resident.LastTotalError(), solve.LastTotalError()), tag + ": total error equal bitwise");

        // the damping factor is a member: a second Optimize starts from it
        const double lambdaAfterFirst = resident.Lambda();
        solve.Optimize(a, graph.Edges());
        resident.Optimize(b, graph.Edges());
        check(!same_bits(lambdaAfterFirst, 1e-3) && resident.LastIterations() == solve.LastIterations() &&
                  same_bits(resident.Lambda(), solve.Lambda()) && poses_same_bits(a, b),
              tag + ": a second Optimize carries the damping factor over");
    }
    {
        bool threw = false;
        try {
            PoseGraphOptimizerLM bad(dev, Solver::SparseCholesky, 10, 1e-6, 1e-3, Mapping::CreateLossFunction(0, 1.0),
                                     Path::Resident);
        } catch (const Error& e) {
            threw = e.status == LGS_ERR_INVALID_ARG;
        }
        check(threw, "a resident optimizer refuses SolverType::SparseCholesky");
        threw = false;
        try {
            PoseGraphOptimizerLM bad(dev, Solver::ConjugateGradient, 10, 1e-6, 1e-3, std::make_shared<LossOfMyOwn>(),
                                     Path::Resident);
        } catch (const Error& e) {
            threw = e.status == LGS_ERR_INVALID_ARG;
        }
        check(threw, "a resident optimizer refuses a loss whose Kind() is -1");
        // the same loss is fine where the host evaluates it
        PoseGraphOptimizerLM fine(dev, Solver::ConjugateGradient, 2, 1e-6, 1e-3, std::make_shared<LossOfMyOwn>());
        std::vector<PoseGraph::Node> nodes = graph.Nodes();
        fine.Optimize(nodes, graph.Edges());
        check(fine.LastIterations() > 0, "SolveOnly takes any loss");
    }
    {
        // an edge that names a missing node is refused before anything runs
        PoseGraph bad = make_graph(10, 0, 0, 3);
        bad.AppendEdge(2, 10, RobotPose2D<double>(0, 0, 0), information(1.0, 1.0));
        PoseGraphOptimizerLM resident(dev, Solver::ConjugateGradient, 10, 1e-6, 1e-3, Mapping::CreateLossFunction(0, 1.0),
                                      Path::Resident);
        std::vector<PoseGraph::Node> nodes = bad.Nodes();
        bool threw = false;
        try {
            resident.Optimize(nodes, bad.Edges());
        } catch (const std::out_of_range&) {
            threw = true;
        }
        check(threw && poses_same_bits(nodes, bad.Nodes()), "an edge to a missing node throws std::out_of_range");
    }

    std::printf(g_failed ? "PGLM ADAPTER TESTS FAILED (%d)\n" : "PGLM ADAPTER TESTS PASSED\n", g_failed);
    return g_failed ? 1 : 0;
}
