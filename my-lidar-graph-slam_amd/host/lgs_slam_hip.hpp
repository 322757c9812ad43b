// lgs_slam_hip.hpp -- C++ host side of the MI355X hot path, mirroring the
// reference's plugin interfaces so a caller of Forrest-Z/my-lidar-graph-slam
// finds the same names, argument meanings and error behaviour.
//
//   reference (H/ = include/my_lidar_graph_slam/)          here
//   Mapping::ScanMatcher (H/mapping/scan_matcher.hpp:83-103) ScanMatcher
//   ScanMatchingQuery / ScanMatchingSummary (:20-77)        same names
//   ScanMatcherRealTimeCorrelative
//     (H/mapping/scan_matcher_real_time_correlative.hpp:15-48)
//                                                           ScanMatcherRealTimeCorrelativeHip
//   ScanMatcherLinearSolver (H/mapping/scan_matcher_linear_solver.hpp:15-56)
//                                                           ScanMatcherLinearSolverHip
//   GridMap<BinaryBayesGridCell> + GridMapBuilder's scan insert / ConstructMapFromScans
//     (H/grid_map/grid_map.hpp, C/mapping/grid_map_builder.cpp:98-332)
//                                                           GridMapHip
//   LoopDetectorRealTimeCorrelative::Detect
//     (C/mapping/loop_detector_real_time_correlative.cpp:26-125)
//                                                           LoopDetectorRealTimeCorrelativeHip
//   ScanMatcherGridSearch (H/mapping/scan_matcher_grid_search.hpp)
//                                                           ScanMatcherGridSearchHip
//   LoopDetectorGridSearch::Detect
//     (C/mapping/loop_detector_grid_search.cpp:26-106)     LoopDetectorGridSearchHip
//   ScanMatcherHillClimbing (H/mapping/scan_matcher_hill_climbing.hpp)
//                                                           ScanMatcherHillClimbingHip
//   (no counterpart: a scan matched against another scan)
//                                                           ScanMatcherIcpPointToLineHip
//
// Everything is a thin RAII layer over the C-ABI (include/lgs_hip.h); the
// compute runs in HIP kernels on the GPU.  Value types are self-contained
// (no Eigen): Matrix3d is a row-major std::array.  INTEGRATION.md shows the
// glue that plugs these classes into the reference itself (flattening its
// patch-based GridMapType into a dense DeviceGrid, Eigen conversions).
//
// Errors: every non-zero status of the C-ABI is thrown as lgs::hip::Error
// (std::runtime_error) with the context's message -- the reference uses
// asserts/exceptions for misuse; no exception crosses the C-ABI itself.
#pragma once

#include <array>
#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "lgs_hip.h"

namespace MyLidarGraphSlam {
namespace Hip {

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string& m) : std::runtime_error(m), status(s) {}
};

// H/pose.hpp RobotPose2D<double> (mX, mY, mTheta)
template <typename T>
struct RobotPose2D {
    T mX = 0, mY = 0, mTheta = 0;
    RobotPose2D() = default;
    RobotPose2D(T x, T y, T theta) : mX(x), mY(y), mTheta(theta) {}
};

// Eigen::Matrix3d stand-in (row-major)
struct Matrix3d {
    std::array<double, 9> m{};
    double operator()(int r, int c) const { return m[3 * r + c]; }
};

// One GPU + HIP stream + scratch (lgs_ctx).  One per matcher instance, like
// the reference's distinct frontend / loop-detector matchers.
class Device {
public:
    explicit Device(int device = 0);
    // a context the caller created and keeps (the C entry points of lgs_io.h): not destroyed here
    explicit Device(lgs_ctx* borrowed) : mCtx(borrowed), mOwned(false) {}
    ~Device();
    Device(const Device&) = delete;
    Device& operator=(const Device&) = delete;
    lgs_ctx* Handle() const { return mCtx; }
    void Check(int status, const char* what) const;
    void Synchronize() const;

private:
    lgs_ctx* mCtx = nullptr;
    bool mOwned = true;
};
using DevicePtr = std::shared_ptr<Device>;

// GridMapBase<double> flattened to a dense row-major fp64 grid in HBM
// (cell (x, y) at y*w + x; 0.0 = Unknown = unallocated patch).
class DeviceGrid {
public:
    DeviceGrid(DevicePtr dev, int w, int h, double minX, double minY, double res);
    DeviceGrid(DevicePtr dev, const std::vector<double>& cells, int w, int h, double minX, double minY,
               double res);
    ~DeviceGrid();
    DeviceGrid(const DeviceGrid&) = delete;
    DeviceGrid& operator=(const DeviceGrid&) = delete;
    DeviceGrid(DeviceGrid&& o) noexcept;
    void Upload(const std::vector<double>& cells);
    // GridMapType ingest without Flatten: patches[py * npx + px] =
    // PatchAt(px, py).Data() or nullptr (lgs_grid_upload_patches); the grid
    // must be npx*patchSize x npy*patchSize
    void UploadPatches(const void* const* patches, int npx, int npy, int patchSize, int cellBytes = 16,
                       int valueOffset = 8);
    std::vector<double> Download() const;
    int NumCellsX() const { return mW; }
    int NumCellsY() const { return mH; }
    double Resolution() const { return mRes; }
    double MinX() const { return mMinX; }
    double MinY() const { return mMinY; }
    const lgs_grid* Handle() const { return mGrid; }
    const DevicePtr& Dev() const { return mDev; }

private:
    friend class GridMapHip;
    DeviceGrid(DevicePtr dev, lgs_grid* borrowed, int w, int h, double minX, double minY, double res);
    DevicePtr mDev;
    lgs_grid* mGrid = nullptr;
    bool mBorrowed = false;
    int mW = 0, mH = 0;
    double mMinX = 0, mMinY = 0, mRes = 0;
};
using DeviceGridPtr = std::shared_ptr<const DeviceGrid>;

// Sensor::ScanData<double> (H/sensor/sensor_data.hpp:65-158), uploaded once.
class ScanData {
public:
    ScanData(DevicePtr dev, const std::vector<double>& angles, const std::vector<double>& ranges,
             const RobotPose2D<double>& relPose = {}, double minRange = 0.0, double maxRange = 30.0);
    ~ScanData();
    ScanData(const ScanData&) = delete;
    ScanData& operator=(const ScanData&) = delete;
    std::size_t NumOfScans() const { return mRanges.size(); }
    const RobotPose2D<double>& RelativeSensorPose() const { return mRelPose; }
    const std::vector<double>& Ranges() const { return mRanges; }
    const std::vector<double>& Angles() const { return mAngles; }
    const lgs_scan* Handle() const { return mScan; }

private:
    friend class ScanInterpolatorHip;
    ScanData(DevicePtr dev, lgs_scan* adopted, const RobotPose2D<double>& relPose);  // takes ownership
    DevicePtr mDev;
    std::vector<double> mAngles, mRanges;
    RobotPose2D<double> mRelPose;
    lgs_scan* mScan = nullptr;
};
using ScanDataPtr = std::shared_ptr<const ScanData>;

// Mapping::ScanInterpolator (H/mapping/scan_interpolator.hpp,
// C/mapping/scan_interpolator.cpp:9-98): the interpolated scan is created
// device-resident directly.
class ScanInterpolatorHip {
public:
    ScanInterpolatorHip(DevicePtr dev, double distScans = 0.05, double distThresholdEmpty = 0.25)
        : mDev(std::move(dev)), mDistScans(distScans), mDistThresholdEmpty(distThresholdEmpty) {}
    ScanDataPtr Interpolate(const ScanDataPtr& scanData) const;

private:
    DevicePtr mDev;
    double mDistScans, mDistThresholdEmpty;
};

// H/mapping/scan_matcher.hpp:20-77
struct ScanMatchingQuery {
    ScanMatchingQuery(DeviceGridPtr gridMap, ScanDataPtr scanData, const RobotPose2D<double>& initialPose)
        : mGridMap(std::move(gridMap)), mScanData(std::move(scanData)), mInitialPose(initialPose) {}
    const DeviceGridPtr mGridMap;
    const ScanDataPtr mScanData;
    const RobotPose2D<double> mInitialPose;
};

struct ScanMatchingSummary {
    bool mPoseFound = false;
    double mNormalizedCost = 0.0;
    RobotPose2D<double> mInitialPose;
    RobotPose2D<double> mEstimatedPose;
    Matrix3d mEstimatedCovariance;
};

// Mapping::ScanMatcher (H/mapping/scan_matcher.hpp:83-103)
class ScanMatcher {
public:
    ScanMatcher() = default;
    virtual ~ScanMatcher() = default;
    ScanMatcher(const ScanMatcher&) = delete;
    ScanMatcher& operator=(const ScanMatcher&) = delete;
    virtual ScanMatchingSummary OptimizePose(const ScanMatchingQuery& queryInfo) = 0;
};
using ScanMatcherPtr = std::shared_ptr<ScanMatcher>;

// CostGreedyEndpoint members (the values the object ends up holding; the
// launcher passes (stddev, scale) into the (scale, stddev) slots, SURVEY
// finding 6 -- FromLauncherJson reproduces that).
struct CostGreedyEndpointParams {
    double mUsableRangeMin = 0.01, mUsableRangeMax = 20.0;
    double mHitAndMissedDist = 0.075, mOccupancyThreshold = 0.1;
    int mKernelSize = 1;
    double mScalingFactor = 0.05, mStandardDeviation = 1.0;
    // The search matchers (correlative, branch-and-bound, grid search) and the
    // loop detectors over them evaluate this cost after their search.  false:
    // the pipeline's default stage, normalized cost and covariance within 1e-5
    // of the reference's.  true: the reference's bytes (the `_cost` entry
    // points with LGS_COST_GREEDY_ENDPOINT_EXACT; kernel
    // size at most 16).  The hill-climbing matcher is exact either way.
    bool mExact = false;
    static CostGreedyEndpointParams FromLauncherJson(double usableMin, double usableMax, double hitMissed,
                                                     double occThr, int kernelSize, double jsonStdDev,
                                                     double jsonScale);
};

// CostSquareError (C/mapping/cost_function_square_error.cpp:10-17).  The
// launcher's CreateCostFunction (C/slam_launcher.cpp:96-107) gives a matcher
// either cost; every matcher below has a constructor for each.  A search
// matcher (correlative, branch-and-bound, grid search) constructed with this
// one runs its search as ever and evaluates Cost and ComputeCovariance of
// this cost at the best sensor pose, as the reference does, in the place of
// the greedy-endpoint cost (the `_cost` entry points with
// LGS_COST_SQUARE_ERROR; the correlative matcher as a stage of its pipeline).
// A loop detector uses the cost function of the matcher it is given
// (matcher->CostSquareError() when non-null, else Cost()), so its loop edges'
// mEstimatedCovMat is that cost function's, as in the reference.
struct CostSquareErrorParams {
    double mUsableRangeMin = 0.01, mUsableRangeMax = 20.0;
};

// ScanMatcherRealTimeCorrelative (C/mapping/scan_matcher_real_time_correlative.cpp:14-256)
class ScanMatcherRealTimeCorrelativeHip final : public ScanMatcher {
public:
    ScanMatcherRealTimeCorrelativeHip(DevicePtr dev, const CostGreedyEndpointParams& costFunc,
                                      int lowResolution, double rangeX, double rangeY, double rangeTheta,
                                      double scanRangeMax);
    ScanMatcherRealTimeCorrelativeHip(DevicePtr dev, const CostSquareErrorParams& costFunc,
                                      int lowResolution, double rangeX, double rangeY, double rangeTheta,
                                      double scanRangeMax);
    // OptimizePose(query): coarse map + search with threshold DBL_MIN (:31-47)
    ScanMatchingSummary OptimizePose(const ScanMatchingQuery& queryInfo) override;
    // the const overload used by loop detectors (:50-145)
    ScanMatchingSummary OptimizePose(const DeviceGrid& gridMap, const DeviceGrid& precompMap,
                                     const ScanDataPtr& scanData, const RobotPose2D<double>& initialPose,
                                     double normalizedScoreThreshold) const;
    // ComputeCoarserMap (:148-153)
    DeviceGrid ComputeCoarserMap(const DeviceGrid& gridMap) const;
    // full device summary of the last OptimizePose (diagnostics: score, window, ...)
    const lgs_rtcsm_summary& LastSummary() const { return mLast; }
    const lgs_rtcsm_params& Params() const { return mParams; }
    const lgs_cost_ge_params& Cost() const { return mCost; }
    // the square-error cost of a matcher constructed with one, else null
    const lgs_cost_sq_params* CostSquareError() const { return mSquareError ? &mCostSq : nullptr; }
    // constructed with CostGreedyEndpointParams::mExact
    bool Exact() const { return mExact; }
    const DevicePtr& Dev() const { return mDev; }

private:
    DevicePtr mDev;
    bool mExact = false;
    lgs_rtcsm_params mParams{};
    lgs_cost_ge_params mCost{};
    lgs_cost_sq_params mCostSq{};
    bool mSquareError = false;
    mutable lgs_rtcsm_summary mLast{};
};

// ScorePixelAccurate (C/mapping/score_function_pixel_accurate.cpp:9-17)
struct ScorePixelAccurateParams {
    double mUsableRangeMin = 0.01, mUsableRangeMax = 20.0;
};

// ScanMatcherBranchBound (C/mapping/scan_matcher_branch_bound.cpp:8-200): the
// device scores every node the reference's search can visit, the host
// replays the search.
class ScanMatcherBranchBoundHip final : public ScanMatcher {
public:
    ScanMatcherBranchBoundHip(DevicePtr dev, const ScorePixelAccurateParams& scoreFunc,
                              const CostGreedyEndpointParams& costFunc, int nodeHeightMax, double rangeX,
                              double rangeY, double rangeTheta, double scanRangeMax);
    ScanMatcherBranchBoundHip(DevicePtr dev, const ScorePixelAccurateParams& scoreFunc,
                              const CostSquareErrorParams& costFunc, int nodeHeightMax, double rangeX,
                              double rangeY, double rangeTheta, double scanRangeMax);
    // OptimizePose(query): pyramid + search with threshold DBL_MIN (:29-44)
    ScanMatchingSummary OptimizePose(const ScanMatchingQuery& queryInfo) override;
    // the const overload used by the loop detector (:47-154)
    ScanMatchingSummary OptimizePose(const DeviceGrid& gridMap, const std::vector<DeviceGridPtr>& precompMaps,
                                     const ScanDataPtr& scanData, const RobotPose2D<double>& initialPose,
                                     double normalizedScoreThreshold) const;
    // ComputeCoarserMaps (:157-165): heights 0..NodeHeightMax
    std::vector<DeviceGridPtr> ComputeCoarserMaps(const DeviceGrid& gridMap) const;
    const lgs_rtcsm_summary& LastSummary() const { return mLast; }
    const lgs_bb_params& Params() const { return mParams; }
    const lgs_cost_ge_params& Cost() const { return mCost; }
    // the square-error cost of a matcher constructed with one, else null
    const lgs_cost_sq_params* CostSquareError() const { return mSquareError ? &mCostSq : nullptr; }
    // constructed with CostGreedyEndpointParams::mExact
    bool Exact() const { return mExact; }
    const DevicePtr& Dev() const { return mDev; }

private:
    DevicePtr mDev;
    bool mExact = false;
    lgs_bb_params mParams{};
    lgs_cost_ge_params mCost{};
    lgs_cost_sq_params mCostSq{};
    bool mSquareError = false;
    mutable lgs_rtcsm_summary mLast{};
};

// ScanMatcherGridSearch (C/mapping/scan_matcher_grid_search.cpp:9-114): every
// pose of the window scored on the device.
class ScanMatcherGridSearchHip final : public ScanMatcher {
public:
    ScanMatcherGridSearchHip(DevicePtr dev, const ScorePixelAccurateParams& scoreFunc,
                             const CostGreedyEndpointParams& costFunc, double rangeX, double rangeY,
                             double rangeTheta, double stepX, double stepY, double stepTheta);
    ScanMatcherGridSearchHip(DevicePtr dev, const ScorePixelAccurateParams& scoreFunc,
                             const CostSquareErrorParams& costFunc, double rangeX, double rangeY,
                             double rangeTheta, double stepX, double stepY, double stepTheta);
    // OptimizePose(query): threshold DBL_MIN (:31-41)
    ScanMatchingSummary OptimizePose(const ScanMatchingQuery& queryInfo) override;
    // the const overload used by the loop detector (:44-114)
    ScanMatchingSummary OptimizePose(const DeviceGrid& gridMap, const ScanDataPtr& scanData,
                                     const RobotPose2D<double>& initialPose,
                                     double normalizedScoreThreshold) const;
    const lgs_rtcsm_summary& LastSummary() const { return mLast; }
    const lgs_gs_params& Params() const { return mParams; }
    const lgs_cost_ge_params& Cost() const { return mCost; }
    // the square-error cost of a matcher constructed with one, else null
    const lgs_cost_sq_params* CostSquareError() const { return mSquareError ? &mCostSq : nullptr; }
    // constructed with CostGreedyEndpointParams::mExact
    bool Exact() const { return mExact; }
    const DevicePtr& Dev() const { return mDev; }

private:
    DevicePtr mDev;
    bool mExact = false;
    lgs_gs_params mParams{};
    lgs_cost_ge_params mCost{};
    lgs_cost_sq_params mCostSq{};
    bool mSquareError = false;
    mutable lgs_rtcsm_summary mLast{};
};

// ScanMatcherHillClimbing (C/mapping/scan_matcher_hill_climbing.cpp:10-109),
// the launcher's fall-back matcher: the whole walk on the device, its summary
// equal to the reference's bit for bit.  Argument order as
// the reference's constructor, the cost function last.
class ScanMatcherHillClimbingHip final : public ScanMatcher {
public:
    ScanMatcherHillClimbingHip(DevicePtr dev, double linearStep, double angularStep, int maxIterations,
                               int maxNumOfRefinements, const CostGreedyEndpointParams& costFunc);
    // the walk over CostSquareError (lgs_hc_sq_optimize_pose_query)
    ScanMatcherHillClimbingHip(DevicePtr dev, double linearStep, double angularStep, int maxIterations,
                               int maxNumOfRefinements, const CostSquareErrorParams& costFunc);
    ScanMatchingSummary OptimizePose(const ScanMatchingQuery& queryInfo) override;
    // full device summary of the last OptimizePose (best sensor pose, counters, final steps)
    const lgs_hc_summary& LastSummary() const { return mLast; }
    const lgs_hc_params& Params() const { return mParams; }
    const lgs_cost_ge_params& Cost() const { return mCost; }
    // the square-error cost of a matcher constructed with one, else null
    const lgs_cost_sq_params* CostSquareError() const { return mSquareError ? &mCostSq : nullptr; }
    const DevicePtr& Dev() const { return mDev; }

private:
    DevicePtr mDev;
    lgs_hc_params mParams{};
    lgs_cost_ge_params mCost{};
    lgs_cost_sq_params mCostSq{};
    bool mSquareError = false;
    lgs_hc_summary mLast{};
};

// ScanMatcherLinearSolver (C/mapping/scan_matcher_linear_solver.cpp:38-148)
// with CostSquareError(usableRangeMin, usableRangeMax).
class ScanMatcherLinearSolverHip final : public ScanMatcher {
public:
    ScanMatcherLinearSolverHip(DevicePtr dev, int numOfIterationsMax, double convergenceThreshold,
                               double usableRangeMin, double usableRangeMax, double translationRegularizer,
                               double rotationRegularizer, double costUsableRangeMin,
                               double costUsableRangeMax);
    ScanMatchingSummary OptimizePose(const ScanMatchingQuery& queryInfo) override;
    const lgs_linsolve_summary& LastSummary() const { return mLast; }

private:
    DevicePtr mDev;
    lgs_linsolve_params mParams{};
    lgs_linsolve_summary mLast{};
};

// Point-to-line ICP: a scan matched against another scan (lgs_icp_*,
// DESIGN.md §4.5b).  The reference has no such matcher; the parameter order
// follows ScanMatcherLinearSolver's constructor, then the two ICP distances.
struct IcpPointToLineParams {
    int mNumOfIterationsMax = 50;
    double mConvergenceThreshold = 1e-6;
    double mUsableRangeMin = 0.01, mUsableRangeMax = 20.0;
    double mTranslationRegularizer = 1e-3, mRotationRegularizer = 1e-3;
    double mMaxCorrespondenceDist = 1.0;
    double mMaxSegmentLength = 0.5;
};

class ScanMatcherIcpPointToLineHip final : public ScanMatcher {
public:
    ScanMatcherIcpPointToLineHip(DevicePtr dev, const IcpPointToLineParams& params);
    // the scan later queries are matched against, and its robot pose
    void SetReference(ScanDataPtr refScan, const RobotPose2D<double>& refPose);
    // a set of scans at their robot poses as the reference (lgs_icp_ref_*,
    // DESIGN.md §4.5c): the table is built here, once, and the scans are not
    // kept; later queries run against it.  Replaces any earlier reference
    void SetReference(const std::vector<ScanDataPtr>& refScans, const std::vector<RobotPose2D<double>>& refPoses);
    ~ScanMatcherIcpPointToLineHip() override;
    ScanMatcherIcpPointToLineHip(const ScanMatcherIcpPointToLineHip&) = delete;
    ScanMatcherIcpPointToLineHip& operator=(const ScanMatcherIcpPointToLineHip&) = delete;
    ScanMatchingSummary OptimizePose(const ScanDataPtr& refScan, const RobotPose2D<double>& refPose,
                                     const ScanDataPtr& scan, const RobotPose2D<double>& initialPose);
    // the query's scan against the reference (the query's grid map is not
    // read); Error(LGS_ERR_INVALID_ARG) when no reference has been set
    ScanMatchingSummary OptimizePose(const ScanMatchingQuery& queryInfo) override;
    const lgs_icp_summary& LastSummary() const { return mLast; }
    const lgs_icp_params& Params() const { return mParams; }

private:
    DevicePtr mDev;
    lgs_icp_params mParams{};
    ScanDataPtr mRefScan;
    RobotPose2D<double> mRefPose;
    lgs_icp_ref* mRef = nullptr;   // the multi-scan reference, when that was set last
    lgs_icp_summary mLast{};
};

// GridMap<BinaryBayesGridCell<double>> with cells on the device and the
// reference's geometry; UpdateScan = GridMapBuilder::UpdateGridMap's insert of
// one scan into the current local map (:149-186), ConstructMapFromScans =
// :227-332 (the latest map).
struct GridMapBuilderParams {
    double mUsableRangeMin = 0.01, mUsableRangeMax = 20.0;
    double mProbHit = 0.6, mProbMiss = 0.45;
};

class GridMapHip {
public:
    GridMapHip(DevicePtr dev, double resolution, int patchSize, int numCellsX, int numCellsY,
               const RobotPose2D<double>& centerPos = {});
    ~GridMapHip();
    GridMapHip(const GridMapHip&) = delete;
    GridMapHip& operator=(const GridMapHip&) = delete;
    void UpdateScan(const ScanData& scan, const RobotPose2D<double>& robotPose, const GridMapBuilderParams& p);
    void ConstructMapFromScans(const std::vector<ScanDataPtr>& scans,
                               const std::vector<RobotPose2D<double>>& robotPoses,
                               const GridMapBuilderParams& p);
    // GridMapBuilder::AppendScan (C/mapping/grid_map_builder.cpp:48-59): the
    // newest scan (scans.back() at robotPoses.back()) into `localMap` as
    // UpdateScan does, and `latestMap` rebuilt from all of `scans` as
    // ConstructMapFromScans does -- one fused device pass for both maps.
    static void AppendScan(GridMapHip& localMap, GridMapHip& latestMap, const std::vector<ScanDataPtr>& scans,
                           const std::vector<RobotPose2D<double>>& robotPoses, const GridMapBuilderParams& p);
    // GridMapBuilder::AfterLoopClosure's rebuild of every local map
    // (C/mapping/grid_map_builder.cpp:62-80): maps[i] from the pose-graph
    // nodes nodeIdxMin[i]..nodeIdxMax[i] of (scans, robotPoses), one fused
    // device pass for all maps.
    static void ConstructMapsFromScans(const std::vector<GridMapHip*>& maps, const std::vector<int>& nodeIdxMin,
                                       const std::vector<int>& nodeIdxMax, const std::vector<ScanDataPtr>& scans,
                                       const std::vector<RobotPose2D<double>>& robotPoses,
                                       const GridMapBuilderParams& p);
    // GridMapBuilder::ConstructGlobalMap (C/mapping/grid_map_builder.cpp:83-95)
    static std::unique_ptr<GridMapHip> ConstructGlobalMap(DevicePtr dev, double resolution, int patchSize,
                                                          const std::vector<ScanDataPtr>& scans,
                                                          const std::vector<RobotPose2D<double>>& robotPoses,
                                                          const GridMapBuilderParams& p);
    lgs_map_geometry Geometry() const;
    // non-owning view of the current cells (valid until the next geometry change)
    DeviceGridPtr Grid() const;
    void Download(std::vector<double>* cells, std::vector<uint32_t>* hits, std::vector<uint32_t>* misses) const;
    lgs_map* Handle() const { return mMap; }
    const DevicePtr& Dev() const { return mDev; }

private:
    GridMapHip(DevicePtr dev, lgs_map* map) : mDev(std::move(dev)), mMap(map) {}
    DevicePtr mDev;
    lgs_map* mMap = nullptr;
};

// LoopDetectionQuery / LoopDetectionResult (H/mapping/loop_detector.hpp:26-87)
struct LoopCandidateNode {
    ScanDataPtr mScanData;
    RobotPose2D<double> mPose;
    int mIndex = 0;
};
struct LoopDetectionQuery {
    std::vector<LoopCandidateNode> mPoseGraphNodes;
    DeviceGridPtr mLocalMap;
    std::shared_ptr<DeviceGrid> mPrecomputedMap;   // LocalMapInfo::mPrecomputedMaps[0]; filled lazily
    RobotPose2D<double> mLocalMapNodePose;
    int mLocalMapNodeIndex = 0;
};
struct LoopDetectionResult {
    RobotPose2D<double> mRelativePose;
    RobotPose2D<double> mStartNodePose;
    int mStartNodeIdx = 0;
    int mEndNodeIdx = 0;
    Matrix3d mEstimatedCovMat;
};

class LoopDetectorRealTimeCorrelativeHip {
public:
    // extraDevices: more GPUs of this process to shard the candidates over
    // (lgs_loop_detect_rtcsm_multi); the matcher's own device is shard 0 and
    // holds the queries' maps and scans.  Results are the same with or without.
    LoopDetectorRealTimeCorrelativeHip(std::shared_ptr<ScanMatcherRealTimeCorrelativeHip> scanMatcher,
                                       double scoreThreshold, std::vector<DevicePtr> extraDevices = {});
    // Detect (:26-92): coarse maps computed once per query, every node matched,
    // found ones appended in query -> node order.
    void Detect(std::vector<LoopDetectionQuery>& queries, std::vector<LoopDetectionResult>& results);
    int NumDevices() const { return 1 + (int)mExtraDevices.size(); }

private:
    std::shared_ptr<ScanMatcherRealTimeCorrelativeHip> mScanMatcher;
    double mScoreThreshold;
    std::vector<DevicePtr> mExtraDevices;
};

// One ICP reference per local map (lgs_icp_ref_set_*): map i
// is built from the pose-graph nodes nodeIdxMin[i]..nodeIdxMax[i] of (scans,
// robotPoses), the ranges of GridMapHip::ConstructMapsFromScans, all maps in
// one device pass.  The scans are not kept.
class IcpReferenceSetHip {
public:
    IcpReferenceSetHip(DevicePtr dev, const IcpPointToLineParams& params, const std::vector<ScanDataPtr>& scans,
                       const std::vector<RobotPose2D<double>>& robotPoses, const std::vector<int>& nodeIdxMin,
                       const std::vector<int>& nodeIdxMax);
    ~IcpReferenceSetHip();
    IcpReferenceSetHip(const IcpReferenceSetHip&) = delete;
    IcpReferenceSetHip& operator=(const IcpReferenceSetHip&) = delete;
    int Size() const { return lgs_icp_ref_set_size(mSet); }
    // borrowed: valid while this object lives
    const lgs_icp_ref* Reference(int i) const { return lgs_icp_ref_set_ref(mSet, i); }
    const lgs_icp_params& Params() const { return mParams; }
    const DevicePtr& Dev() const { return mDev; }
    lgs_icp_ref_set* Handle() const { return mSet; }

private:
    DevicePtr mDev;
    lgs_icp_params mParams{};
    lgs_icp_ref_set* mSet = nullptr;
};

// What an ICP refinement of a detected loop must meet to replace the
// detector's estimate (lgs_loop_refine_gate); the defaults accept every refine
// that found a pose
struct LoopRefineGate {
    int mMinPairs = 3;
    double mMaxNormalizedCost = HUGE_VAL;
    double mMaxTranslation = HUGE_VAL;
    double mMaxRotation = HUGE_VAL;
};

// Detected loops refined by point-to-line ICP against their local maps'
// references (lgs_loop_refine_icp).  `results` are those a
// detector's Detect(queries, results) appended: the found nodes in query ->
// node order, each recognised by (mStartNodeIdx, mEndNodeIdx).  A result's
// estimate is Compound(query.mLocalMapNodePose, mRelativePose); query q is
// refined against set.Reference(mapIndexOfQuery[q]).  An accepted result gets
// the ICP's mRelativePose and mEstimatedCovMat, every other stays as it is.
// Returns one flag per result: 1 refined, 0 kept.
class LoopRefinerIcpHip {
public:
    explicit LoopRefinerIcpHip(const LoopRefineGate& gate = {});
    std::vector<int> Refine(const IcpReferenceSetHip& set, const std::vector<int>& mapIndexOfQuery,
                            const std::vector<LoopDetectionQuery>& queries,
                            std::vector<LoopDetectionResult>& results);
    // per result of the last Refine: the ICP's summary
    const std::vector<lgs_icp_summary>& LastSummaries() const { return mLast; }
    const lgs_loop_refine_gate& Gate() const { return mGate; }

private:
    lgs_loop_refine_gate mGate{};
    std::vector<lgs_icp_summary> mLast;
};

// The lattice of start poses of the ICP loop detector (lgs_icp_window):
// 2 * half + 1 poses per axis around a candidate's node pose
struct IcpWindow {
    int mHalfX = 0, mHalfY = 0, mHalfTheta = 0;
    double mStepXY = 0.05, mStepTheta = 0.005;
};

// A loop detector that needs no grid (lgs_loop_detect_icp):
// every node's scan is scored by one ICP pass at each pose of the window around
// its pose against set.Reference(mapIndexOfQuery[q]), refined from the best of
// them and accepted by the gate; the found ones are appended in query -> node
// order, like the other detectors'.  Of a query mLocalMap and mPrecomputedMap
// are not read.
class LoopDetectorIcpHip {
public:
    LoopDetectorIcpHip(const IcpPointToLineParams& params, const IcpWindow& window, const LoopRefineGate& gate = {});
    void Detect(const IcpReferenceSetHip& set, const std::vector<int>& mapIndexOfQuery,
                const std::vector<LoopDetectionQuery>& queries, std::vector<LoopDetectionResult>& results);
    // per candidate node of the last Detect, in query -> node order: the best
    // lattice index (-1: none) and the refine's summary (zero: none ran)
    const std::vector<int>& LastBestIndices() const { return mLastBest; }
    const std::vector<lgs_icp_summary>& LastSummaries() const { return mLast; }
    const lgs_icp_params& Params() const { return mParams; }
    const lgs_icp_window& Window() const { return mWindow; }
    const lgs_loop_refine_gate& Gate() const { return mGate; }

private:
    lgs_icp_params mParams{};
    lgs_icp_window mWindow{};
    lgs_loop_refine_gate mGate{};
    std::vector<int> mLastBest;
    std::vector<lgs_icp_summary> mLast;
};

// LoopDetectorBranchBound (C/mapping/loop_detector_branch_bound.cpp:10-117):
// pyramids computed per query (LocalMapInfo caches them, :45-55), every node
// matched, found ones appended in query -> node order.
class LoopDetectorBranchBoundHip {
public:
    LoopDetectorBranchBoundHip(std::shared_ptr<ScanMatcherBranchBoundHip> scanMatcher, double scoreThreshold);
    void Detect(std::vector<LoopDetectionQuery>& queries, std::vector<LoopDetectionResult>& results);

private:
    std::shared_ptr<ScanMatcherBranchBoundHip> mScanMatcher;
    double mScoreThreshold;
};

// LoopDetectorGridSearch (C/mapping/loop_detector_grid_search.cpp:10-106):
// every node matched against its query's local map, found ones appended in
// query -> node order; one batched device call for all of them.
class LoopDetectorGridSearchHip {
public:
    LoopDetectorGridSearchHip(std::shared_ptr<ScanMatcherGridSearchHip> scanMatcher, double scoreThreshold);
    void Detect(std::vector<LoopDetectionQuery>& queries, std::vector<LoopDetectionResult>& results);

private:
    std::shared_ptr<ScanMatcherGridSearchHip> mScanMatcher;
    double mScoreThreshold;
};

// LoopSearcherNearest (C/mapping/loop_searcher_nearest.cpp:13-108; lgs_loop_*,
// DESIGN.md §4.6g).  LoopSearchHint and LoopCandidate are H/mapping/
// loop_searcher.hpp:24-82 with vectors in place of the std::maps: node k at
// index k, local map i at index i.
struct LocalMapNodeRange {
    int mPoseGraphNodeIdxMin = 0, mPoseGraphNodeIdxMax = 0;   // LocalMapPosition's, inclusive
};
struct LoopSearchHint {
    std::vector<RobotPose2D<double>> mPoseGraphNodes;
    std::vector<LocalMapNodeRange> mLocalMapPositions;
    double mAccumTravelDist = 0.0;
    int mLatestNodeIdx = 0;
    int mLatestLocalMapIdx = 0;
};
struct LoopCandidate {
    std::vector<int> mNodeIndices;
    int mLocalMapIdx = 0;
    int mLocalMapNodeIdx = 0;
};
using LoopCandidateVector = std::vector<LoopCandidate>;

// A graph snapshot on the device (lgs_loop_graph): the poses of all nodes and
// the node ranges of all local maps, the last one the latest, unfinished map.
class LoopGraphHip {
public:
    LoopGraphHip(DevicePtr dev, const std::vector<RobotPose2D<double>>& poseGraphNodes,
                 const std::vector<LocalMapNodeRange>& localMapPositions);
    ~LoopGraphHip();
    LoopGraphHip(const LoopGraphHip&) = delete;
    LoopGraphHip& operator=(const LoopGraphHip&) = delete;
    lgs_loop_graph* Handle() const { return mGraph; }
    int NumOfNodes() const { return mNumOfNodes; }
    int NumOfMaps() const { return mNumOfMaps; }
    const DevicePtr& Dev() const { return mDev; }

private:
    DevicePtr mDev;
    lgs_loop_graph* mGraph = nullptr;
    int mNumOfNodes = 0, mNumOfMaps = 0;
};

// One hint of a batch against a snapshot: what LoopSearchHint holds besides the snapshot
struct LoopSearchBatchHint {
    int mLatestNodeIdx = 0;
    int mLatestLocalMapIdx = 0;
    int mNumOfMaps = 0;              // mLocalMapPositions.size() when the node was the latest one
    double mAccumTravelDist = 0.0;
};

class LoopSearcherNearestHip {
public:
    LoopSearcherNearestHip(double travelDistThreshold, double nodeDistThreshold, int numOfCandidateNodes);
    // the reference's Search: one hint, the loop on the host (no device work);
    // empty when no node is near
    LoopCandidateVector Search(const LoopSearchHint& searchHint) const;
    // many hints against one snapshot on the device: out[j] is Search's answer for hints[j]
    std::vector<LoopCandidateVector> SearchBatch(const LoopGraphHip& graph,
                                                 const std::vector<LoopSearchBatchHint>& hints) const;
    // one LoopCandidate per finished local map the node is near (the nearest
    // node inside that map), in map order, from the per-map table
    std::vector<LoopCandidateVector> SearchAllMaps(const LoopGraphHip& graph,
                                                   const std::vector<LoopSearchBatchHint>& hints) const;
    const lgs_loop_search_params& Params() const { return mParams; }

private:
    lgs_loop_search_params mParams{};
};

// LidarGraphSlam::GetLoopDetectionQueries (C/mapping/lidar_graph_slam.cpp:155-188):
// per candidate its nodes (nodes[k] is node k), its local map (localMaps[i] is
// map i) and the local map's node
std::vector<LoopDetectionQuery> GetLoopDetectionQueries(const LoopCandidateVector& loopCandidates,
                                                        const std::vector<LoopCandidateNode>& nodes,
                                                        const std::vector<DeviceGridPtr>& localMaps);

}  // namespace Hip
}  // namespace MyLidarGraphSlam
