// lgs_slam_hip.cpp -- the reference-shaped C++ classes over the C-ABI (see the header).
#include "lgs_slam_hip.hpp"

#include <cfloat>
#include <cstring>

namespace MyLidarGraphSlam {
namespace Hip {

namespace {

lgs_pose2d to_c(const RobotPose2D<double>& p) { return { p.mX, p.mY, p.mTheta }; }
RobotPose2D<double> from_c(const lgs_pose2d& p) { return { p.x, p.y, p.theta }; }

Matrix3d cov_of(const double* c)
{
    Matrix3d m;
    for (int i = 0; i < 9; ++i) m.m[i] = c[i];
    return m;
}

ScanMatchingSummary summary_of(const lgs_rtcsm_summary& s)
{
    ScanMatchingSummary o;
    o.mPoseFound = s.pose_found != 0;
    o.mNormalizedCost = s.normalized_cost;
    o.mInitialPose = from_c(s.initial_pose);
    o.mEstimatedPose = from_c(s.estimated_pose);
    o.mEstimatedCovariance = cov_of(s.covariance);
    return o;
}

}  // namespace

// ------------------------------------------------------------------ Device
Device::Device(int device)
{
    const int rc = lgs_ctx_create(device, &mCtx);
    if (rc != LGS_OK) throw Error(rc, "lgs_ctx_create(" + std::to_string(device) + ") failed");
}

Device::~Device()
{
    if (mCtx && mOwned) lgs_ctx_destroy(mCtx);
}

void Device::Check(int status, const char* what) const
{
    if (status == LGS_OK) return;
    const char* m = lgs_ctx_last_error(mCtx);
    throw Error(status, std::string(what) + ": " + (m ? m : "") + " (status " + std::to_string(status) + ")");
}

void Device::Synchronize() const { Check(lgs_ctx_synchronize(mCtx), "lgs_ctx_synchronize"); }

// -------------------------------------------------------------- DeviceGrid
DeviceGrid::DeviceGrid(DevicePtr dev, int w, int h, double minX, double minY, double res)
    : mDev(std::move(dev)), mW(w), mH(h), mMinX(minX), mMinY(minY), mRes(res)
{
    mDev->Check(lgs_grid_create(mDev->Handle(), w, h, minX, minY, res, &mGrid), "lgs_grid_create");
}

DeviceGrid::DeviceGrid(DevicePtr dev, const std::vector<double>& cells, int w, int h, double minX,
                       double minY, double res)
    : DeviceGrid(std::move(dev), w, h, minX, minY, res)
{
    Upload(cells);
}

DeviceGrid::DeviceGrid(DevicePtr dev, lgs_grid* borrowed, int w, int h, double minX, double minY, double res)
    : mDev(std::move(dev)), mGrid(borrowed), mBorrowed(true), mW(w), mH(h), mMinX(minX), mMinY(minY), mRes(res)
{
}

DeviceGrid::DeviceGrid(DeviceGrid&& o) noexcept
    : mDev(std::move(o.mDev)), mGrid(o.mGrid), mBorrowed(o.mBorrowed), mW(o.mW), mH(o.mH), mMinX(o.mMinX),
      mMinY(o.mMinY), mRes(o.mRes)
{
    o.mGrid = nullptr;
}

DeviceGrid::~DeviceGrid()
{
    if (mGrid && !mBorrowed) lgs_grid_destroy(mGrid);
}

void DeviceGrid::Upload(const std::vector<double>& cells)
{
    if (cells.size() != (std::size_t)mW * mH) throw Error(LGS_ERR_INVALID_ARG, "DeviceGrid::Upload: size mismatch");
    mDev->Check(lgs_grid_upload(mDev->Handle(), mGrid, cells.data()), "lgs_grid_upload");
}

void DeviceGrid::UploadPatches(const void* const* patches, int npx, int npy, int patchSize, int cellBytes,
                               int valueOffset)
{
    mDev->Check(lgs_grid_upload_patches(mDev->Handle(), mGrid, patches, npx, npy, patchSize, cellBytes, valueOffset),
                "lgs_grid_upload_patches");
}

std::vector<double> DeviceGrid::Download() const
{
    std::vector<double> out((std::size_t)mW * mH);
    mDev->Check(lgs_grid_download(mDev->Handle(), mGrid, out.data()), "lgs_grid_download");
    return out;
}

// ---------------------------------------------------------------- ScanData
ScanData::ScanData(DevicePtr dev, const std::vector<double>& angles, const std::vector<double>& ranges,
                   const RobotPose2D<double>& relPose, double minRange, double maxRange)
    : mDev(std::move(dev)), mAngles(angles), mRanges(ranges), mRelPose(relPose)
{
    if (angles.size() != ranges.size()) throw Error(LGS_ERR_INVALID_ARG, "ScanData: angles/ranges size mismatch");
    lgs_scan_host h{ mRanges.data(), mAngles.data(), (int)mRanges.size(), to_c(relPose), minRange, maxRange };
    mDev->Check(lgs_scan_create(mDev->Handle(), &h, &mScan), "lgs_scan_create");
}

ScanData::ScanData(DevicePtr dev, lgs_scan* adopted, const RobotPose2D<double>& relPose)
    : mDev(std::move(dev)), mRelPose(relPose), mScan(adopted)
{
    int n = 0;
    mDev->Check(lgs_scan_get(mScan, &n, nullptr, nullptr), "lgs_scan_get");
    mRanges.resize(n);
    mAngles.resize(n);
    mDev->Check(lgs_scan_get(mScan, &n, mRanges.data(), mAngles.data()), "lgs_scan_get");
}

ScanData::~ScanData()
{
    if (mScan) lgs_scan_destroy(mScan);
}

ScanDataPtr ScanInterpolatorHip::Interpolate(const ScanDataPtr& scanData) const
{
    if (!scanData) throw Error(LGS_ERR_INVALID_ARG, "Interpolate: null scan");
    lgs_scan* out = nullptr;
    mDev->Check(lgs_scan_interpolate(mDev->Handle(), scanData->Handle(), mDistScans, mDistThresholdEmpty, &out),
                "lgs_scan_interpolate");
    return ScanDataPtr(new ScanData(mDev, out, scanData->RelativeSensorPose()));
}

// ------------------------------------------------------ cost parameters
CostGreedyEndpointParams CostGreedyEndpointParams::FromLauncherJson(double usableMin, double usableMax,
                                                                    double hitMissed, double occThr,
                                                                    int kernelSize, double jsonStdDev,
                                                                    double jsonScale)
{
    // CreateCostGreedyEndpoint (C/slam_launcher.cpp:54-76) passes
    // (..., kernelSize, standardDeviation, scalingFactor) into the constructor
    // (..., kernelSize, scalingFactor, standardDeviation)
    CostGreedyEndpointParams p;
    p.mUsableRangeMin = usableMin;
    p.mUsableRangeMax = usableMax;
    p.mHitAndMissedDist = hitMissed;
    p.mOccupancyThreshold = occThr;
    p.mKernelSize = kernelSize;
    p.mScalingFactor = jsonStdDev;
    p.mStandardDeviation = jsonScale;
    return p;
}

static lgs_cost_ge_params ge_of(const CostGreedyEndpointParams& c)
{
    return { c.mUsableRangeMin, c.mUsableRangeMax, c.mHitAndMissedDist, c.mOccupancyThreshold,
             c.mKernelSize, c.mScalingFactor, c.mStandardDeviation };
}

// a search matcher or loop detector constructed with CostSquareError: the
// `_cost` entry points evaluate Cost / NumOfScans() and ComputeCovariance at
// the best sensor pose in the place of the greedy-endpoint cost
static lgs_cost_spec sq_spec(const lgs_cost_sq_params* cost)
{
    lgs_cost_spec spec{};
    spec.kind = LGS_COST_SQUARE_ERROR;
    spec.sq = *cost;
    return spec;
}

// the cost function a search matcher was constructed with; a loop detector
// uses its matcher's: the reference's detector calls its matcher's
// OptimizePose, so that cost function produces mEstimatedCovMat
// (C/mapping/loop_detector_real_time_correlative.cpp:96-125).  A greedy-endpoint
// cost built with mExact selects the bit-exact kind.
template <class Matcher>
static lgs_cost_spec spec_of(const Matcher& m)
{
    if (m.CostSquareError()) return sq_spec(m.CostSquareError());
    lgs_cost_spec spec{};
    spec.kind = m.Exact() ? LGS_COST_GREEDY_ENDPOINT_EXACT : LGS_COST_GREEDY_ENDPOINT;
    spec.ge = m.Cost();
    return spec;
}

// ------------------------------------------ ScanMatcherRealTimeCorrelativeHip
ScanMatcherRealTimeCorrelativeHip::ScanMatcherRealTimeCorrelativeHip(DevicePtr dev,
                                                                     const CostGreedyEndpointParams& c,
                                                                     int lowResolution, double rangeX,
                                                                     double rangeY, double rangeTheta,
                                                                     double scanRangeMax)
    : mDev(std::move(dev))
{
    // the reference's constructor only stores its arguments (:13-27); invalid
    // values surface as LGS_ERR_INVALID_ARG from the first OptimizePose
    mParams = { lowResolution, rangeX, rangeY, rangeTheta, scanRangeMax };
    mCost = ge_of(c);
    mExact = c.mExact;
}

ScanMatcherRealTimeCorrelativeHip::ScanMatcherRealTimeCorrelativeHip(DevicePtr dev, const CostSquareErrorParams& c,
                                                                     int lowResolution, double rangeX,
                                                                     double rangeY, double rangeTheta,
                                                                     double scanRangeMax)
    : ScanMatcherRealTimeCorrelativeHip(std::move(dev), CostGreedyEndpointParams(), lowResolution, rangeX, rangeY,
                                        rangeTheta, scanRangeMax)
{
    mCostSq = { c.mUsableRangeMin, c.mUsableRangeMax };
    mSquareError = true;
}

ScanMatchingSummary ScanMatcherRealTimeCorrelativeHip::OptimizePose(const ScanMatchingQuery& q)
{
    if (CostSquareError() || mExact) {
        const lgs_cost_spec spec = spec_of(*this);
        mDev->Check(lgs_rtcsm_optimize_pose_query_cost(mDev->Handle(), q.mGridMap->Handle(), &mParams, &spec,
                                                       q.mScanData->Handle(), to_c(q.mInitialPose), &mLast),
                    "lgs_rtcsm_optimize_pose_query_cost");
        return summary_of(mLast);
    }
    mDev->Check(lgs_rtcsm_optimize_pose_query(mDev->Handle(), q.mGridMap->Handle(), &mParams, &mCost,
                                              q.mScanData->Handle(), to_c(q.mInitialPose), &mLast),
                "lgs_rtcsm_optimize_pose_query");
    return summary_of(mLast);
}

ScanMatchingSummary ScanMatcherRealTimeCorrelativeHip::OptimizePose(const DeviceGrid& gridMap,
                                                                    const DeviceGrid& precompMap,
                                                                    const ScanDataPtr& scanData,
                                                                    const RobotPose2D<double>& initialPose,
                                                                    double thr) const
{
    if (CostSquareError() || mExact) {
        const lgs_cost_spec spec = spec_of(*this);
        mDev->Check(lgs_rtcsm_optimize_pose_cost(mDev->Handle(), gridMap.Handle(), precompMap.Handle(), &mParams,
                                                 &spec, scanData->Handle(), to_c(initialPose), thr, &mLast),
                    "lgs_rtcsm_optimize_pose_cost");
        return summary_of(mLast);
    }
    mDev->Check(lgs_rtcsm_optimize_pose(mDev->Handle(), gridMap.Handle(), precompMap.Handle(), &mParams, &mCost,
                                        scanData->Handle(), to_c(initialPose), thr, &mLast),
                "lgs_rtcsm_optimize_pose");
    return summary_of(mLast);
}

DeviceGrid ScanMatcherRealTimeCorrelativeHip::ComputeCoarserMap(const DeviceGrid& g) const
{
    DeviceGrid out(mDev, g.NumCellsX(), g.NumCellsY(), g.MinX(), g.MinY(), g.Resolution());
    mDev->Check(lgs_grid_precompute_max(mDev->Handle(), g.Handle(), mParams.low_resolution,
                                        const_cast<lgs_grid*>(out.Handle())),
                "lgs_grid_precompute_max");
    return out;
}

// ------------------------------------------------ ScanMatcherBranchBoundHip
ScanMatcherBranchBoundHip::ScanMatcherBranchBoundHip(DevicePtr dev, const ScorePixelAccurateParams& sf,
                                                     const CostGreedyEndpointParams& c, int nodeHeightMax,
                                                     double rangeX, double rangeY, double rangeTheta,
                                                     double scanRangeMax)
    : mDev(std::move(dev))
{
    mParams = { nodeHeightMax, rangeX, rangeY, rangeTheta, scanRangeMax, sf.mUsableRangeMin, sf.mUsableRangeMax };
    mCost = ge_of(c);
    mExact = c.mExact;
}

ScanMatcherBranchBoundHip::ScanMatcherBranchBoundHip(DevicePtr dev, const ScorePixelAccurateParams& sf,
                                                     const CostSquareErrorParams& c, int nodeHeightMax,
                                                     double rangeX, double rangeY, double rangeTheta,
                                                     double scanRangeMax)
    : ScanMatcherBranchBoundHip(std::move(dev), sf, CostGreedyEndpointParams(), nodeHeightMax, rangeX, rangeY,
                                rangeTheta, scanRangeMax)
{
    mCostSq = { c.mUsableRangeMin, c.mUsableRangeMax };
    mSquareError = true;
}

ScanMatchingSummary ScanMatcherBranchBoundHip::OptimizePose(const ScanMatchingQuery& q)
{
    if (CostSquareError() || mExact) {
        const lgs_cost_spec spec = spec_of(*this);
        mDev->Check(lgs_bb_optimize_pose_query_cost(mDev->Handle(), q.mGridMap->Handle(), &mParams, &spec,
                                                    q.mScanData->Handle(), to_c(q.mInitialPose), &mLast),
                    "lgs_bb_optimize_pose_query_cost");
        return summary_of(mLast);
    }
    mDev->Check(lgs_bb_optimize_pose_query(mDev->Handle(), q.mGridMap->Handle(), &mParams, &mCost,
                                           q.mScanData->Handle(), to_c(q.mInitialPose), &mLast),
                "lgs_bb_optimize_pose_query");
    return summary_of(mLast);
}

ScanMatchingSummary ScanMatcherBranchBoundHip::OptimizePose(const DeviceGrid& gridMap,
                                                            const std::vector<DeviceGridPtr>& precompMaps,
                                                            const ScanDataPtr& scanData,
                                                            const RobotPose2D<double>& initialPose, double thr) const
{
    std::vector<const lgs_grid*> pyr;
    for (const auto& m : precompMaps) pyr.push_back(m->Handle());
    if ((int)pyr.size() != mParams.node_height_max + 1)
        throw Error(LGS_ERR_INVALID_ARG, "ScanMatcherBranchBoundHip: one precomputed map per node height needed");
    const lgs_scan* s = scanData->Handle();
    const lgs_pose2d p = to_c(initialPose);
    if (CostSquareError() || mExact) {
        const lgs_cost_spec spec = spec_of(*this);
        mDev->Check(lgs_bb_optimize_pose_batch_cost(mDev->Handle(), gridMap.Handle(), pyr.data(), &mParams, &spec, &s,
                                                    &p, 1, thr, &mLast),
                    "lgs_bb_optimize_pose_batch_cost");
        return summary_of(mLast);
    }
    mDev->Check(lgs_bb_optimize_pose_batch(mDev->Handle(), gridMap.Handle(), pyr.data(), &mParams, &mCost, &s, &p,
                                           1, thr, &mLast),
                "lgs_bb_optimize_pose_batch");
    return summary_of(mLast);
}

std::vector<DeviceGridPtr> ScanMatcherBranchBoundHip::ComputeCoarserMaps(const DeviceGrid& g) const
{
    std::vector<DeviceGridPtr> out;
    std::vector<lgs_grid*> hs;
    for (int h = 0; h <= mParams.node_height_max; ++h) {
        out.push_back(std::make_shared<DeviceGrid>(mDev, g.NumCellsX(), g.NumCellsY(), g.MinX(), g.MinY(),
                                                   g.Resolution()));
        hs.push_back(const_cast<lgs_grid*>(out.back()->Handle()));
    }
    mDev->Check(lgs_grid_precompute_pyramid(mDev->Handle(), g.Handle(), mParams.node_height_max, hs.data()),
                "lgs_grid_precompute_pyramid");
    return out;
}

// ------------------------------------------------- ScanMatcherGridSearchHip
ScanMatcherGridSearchHip::ScanMatcherGridSearchHip(DevicePtr dev, const ScorePixelAccurateParams& sf,
                                                   const CostGreedyEndpointParams& c, double rangeX, double rangeY,
                                                   double rangeTheta, double stepX, double stepY, double stepTheta)
    : mDev(std::move(dev))
{
    // the reference's constructor only stores its arguments (:9-27); invalid
    // values surface as LGS_ERR_INVALID_ARG from the first OptimizePose
    mParams = { rangeX, rangeY, rangeTheta, stepX, stepY, stepTheta, sf.mUsableRangeMin, sf.mUsableRangeMax };
    mCost = ge_of(c);
    mExact = c.mExact;
}

ScanMatcherGridSearchHip::ScanMatcherGridSearchHip(DevicePtr dev, const ScorePixelAccurateParams& sf,
                                                   const CostSquareErrorParams& c, double rangeX, double rangeY,
                                                   double rangeTheta, double stepX, double stepY, double stepTheta)
    : ScanMatcherGridSearchHip(std::move(dev), sf, CostGreedyEndpointParams(), rangeX, rangeY, rangeTheta, stepX,
                               stepY, stepTheta)
{
    mCostSq = { c.mUsableRangeMin, c.mUsableRangeMax };
    mSquareError = true;
}

ScanMatchingSummary ScanMatcherGridSearchHip::OptimizePose(const ScanMatchingQuery& q)
{
    if (CostSquareError() || mExact) {
        const lgs_cost_spec spec = spec_of(*this);
        mDev->Check(lgs_gs_optimize_pose_query_cost(mDev->Handle(), q.mGridMap->Handle(), &mParams, &spec,
                                                    q.mScanData->Handle(), to_c(q.mInitialPose), &mLast),
                    "lgs_gs_optimize_pose_query_cost");
        return summary_of(mLast);
    }
    mDev->Check(lgs_gs_optimize_pose_query(mDev->Handle(), q.mGridMap->Handle(), &mParams, &mCost,
                                           q.mScanData->Handle(), to_c(q.mInitialPose), &mLast),
                "lgs_gs_optimize_pose_query");
    return summary_of(mLast);
}

ScanMatchingSummary ScanMatcherGridSearchHip::OptimizePose(const DeviceGrid& gridMap, const ScanDataPtr& scanData,
                                                           const RobotPose2D<double>& initialPose, double thr) const
{
    const lgs_scan* s = scanData->Handle();
    const lgs_pose2d p = to_c(initialPose);
    if (CostSquareError() || mExact) {
        const lgs_cost_spec spec = spec_of(*this);
        mDev->Check(lgs_gs_optimize_pose_batch_cost(mDev->Handle(), gridMap.Handle(), &mParams, &spec, &s, &p, 1, thr,
                                                    &mLast),
                    "lgs_gs_optimize_pose_batch_cost");
        return summary_of(mLast);
    }
    mDev->Check(lgs_gs_optimize_pose_batch(mDev->Handle(), gridMap.Handle(), &mParams, &mCost, &s, &p, 1, thr,
                                           &mLast),
                "lgs_gs_optimize_pose_batch");
    return summary_of(mLast);
}

// ----------------------------------------------- ScanMatcherHillClimbingHip
ScanMatcherHillClimbingHip::ScanMatcherHillClimbingHip(DevicePtr dev, double linearStep, double angularStep,
                                                       int maxIterations, int maxNumOfRefinements,
                                                       const CostGreedyEndpointParams& c)
    : mDev(std::move(dev))
{
    // the reference's constructor only stores its arguments (:10-23); invalid
    // values surface as LGS_ERR_INVALID_ARG from the first OptimizePose
    mParams = { linearStep, angularStep, maxIterations, maxNumOfRefinements };
    mCost = ge_of(c);
}

ScanMatcherHillClimbingHip::ScanMatcherHillClimbingHip(DevicePtr dev, double linearStep, double angularStep,
                                                       int maxIterations, int maxNumOfRefinements,
                                                       const CostSquareErrorParams& c)
    : ScanMatcherHillClimbingHip(std::move(dev), linearStep, angularStep, maxIterations, maxNumOfRefinements,
                                 CostGreedyEndpointParams())
{
    mCostSq = { c.mUsableRangeMin, c.mUsableRangeMax };
    mSquareError = true;
}

ScanMatchingSummary ScanMatcherHillClimbingHip::OptimizePose(const ScanMatchingQuery& q)
{
    if (mSquareError)
        mDev->Check(lgs_hc_sq_optimize_pose_query(mDev->Handle(), q.mGridMap->Handle(), &mParams, &mCostSq,
                                                  q.mScanData->Handle(), to_c(q.mInitialPose), &mLast),
                    "lgs_hc_sq_optimize_pose_query");
    else
        mDev->Check(lgs_hc_optimize_pose_query(mDev->Handle(), q.mGridMap->Handle(), &mParams, &mCost,
                                               q.mScanData->Handle(), to_c(q.mInitialPose), &mLast),
                    "lgs_hc_optimize_pose_query");
    ScanMatchingSummary o;
    o.mPoseFound = mLast.pose_found != 0;
    o.mNormalizedCost = mLast.normalized_cost;
    o.mInitialPose = from_c(mLast.initial_pose);
    o.mEstimatedPose = from_c(mLast.estimated_pose);
    o.mEstimatedCovariance = cov_of(mLast.covariance);
    return o;
}

// ------------------------------------------------ ScanMatcherLinearSolverHip
ScanMatcherLinearSolverHip::ScanMatcherLinearSolverHip(DevicePtr dev, int numOfIterationsMax,
                                                       double convergenceThreshold, double usableRangeMin,
                                                       double usableRangeMax, double translationRegularizer,
                                                       double rotationRegularizer, double costUsableRangeMin,
                                                       double costUsableRangeMax)
    : mDev(std::move(dev))
{
    mParams = { numOfIterationsMax, convergenceThreshold, usableRangeMin, usableRangeMax,
                translationRegularizer, rotationRegularizer, costUsableRangeMin, costUsableRangeMax };
}

ScanMatchingSummary ScanMatcherLinearSolverHip::OptimizePose(const ScanMatchingQuery& q)
{
    mDev->Check(lgs_linsolve_optimize_pose(mDev->Handle(), q.mGridMap->Handle(), &mParams, q.mScanData->Handle(),
                                           to_c(q.mInitialPose), &mLast, nullptr),
                "lgs_linsolve_optimize_pose");
    ScanMatchingSummary o;
    o.mPoseFound = mLast.pose_found != 0;
    o.mNormalizedCost = mLast.normalized_cost;
    o.mInitialPose = from_c(mLast.initial_pose);
    o.mEstimatedPose = from_c(mLast.estimated_pose);
    o.mEstimatedCovariance = cov_of(mLast.covariance);
    return o;
}

// ---------------------------------------------- ScanMatcherIcpPointToLineHip
ScanMatcherIcpPointToLineHip::ScanMatcherIcpPointToLineHip(DevicePtr dev, const IcpPointToLineParams& p)
    : mDev(std::move(dev))
{
    mParams = { p.mNumOfIterationsMax, p.mConvergenceThreshold, p.mUsableRangeMin, p.mUsableRangeMax,
                p.mTranslationRegularizer, p.mRotationRegularizer, p.mMaxCorrespondenceDist, p.mMaxSegmentLength };
}

void ScanMatcherIcpPointToLineHip::SetReference(ScanDataPtr refScan, const RobotPose2D<double>& refPose)
{
    mRefScan = std::move(refScan);
    mRefPose = refPose;
    if (mRef) lgs_icp_ref_destroy(mRef);
    mRef = nullptr;
}

void ScanMatcherIcpPointToLineHip::SetReference(const std::vector<ScanDataPtr>& refScans,
                                                const std::vector<RobotPose2D<double>>& refPoses)
{
    if (refScans.empty() || refScans.size() != refPoses.size())
        throw Error(LGS_ERR_INVALID_ARG, "ScanMatcherIcpPointToLineHip: need as many reference poses as scans, at least one");
    std::vector<const lgs_scan*> scans;
    std::vector<lgs_pose2d> poses;
    for (std::size_t k = 0; k < refScans.size(); ++k) {
        if (!refScans[k]) throw Error(LGS_ERR_INVALID_ARG, "ScanMatcherIcpPointToLineHip: null scan");
        scans.push_back(refScans[k]->Handle());
        poses.push_back(to_c(refPoses[k]));
    }
    lgs_icp_ref* ref = nullptr;
    mDev->Check(lgs_icp_ref_create(mDev->Handle(), scans.data(), poses.data(), (int)scans.size(), &mParams, &ref),
                "lgs_icp_ref_create");
    if (mRef) lgs_icp_ref_destroy(mRef);
    mRef = ref;
    mRefScan.reset();
}

ScanMatcherIcpPointToLineHip::~ScanMatcherIcpPointToLineHip()
{
    if (mRef) lgs_icp_ref_destroy(mRef);
}

ScanMatchingSummary ScanMatcherIcpPointToLineHip::OptimizePose(const ScanDataPtr& refScan,
                                                               const RobotPose2D<double>& refPose,
                                                               const ScanDataPtr& scan,
                                                               const RobotPose2D<double>& initialPose)
{
    if (!refScan || !scan) throw Error(LGS_ERR_INVALID_ARG, "ScanMatcherIcpPointToLineHip: null scan");
    mDev->Check(lgs_icp_optimize_pose(mDev->Handle(), refScan->Handle(), to_c(refPose), scan->Handle(),
                                      to_c(initialPose), &mParams, &mLast, nullptr),
                "lgs_icp_optimize_pose");
    ScanMatchingSummary o;
    o.mPoseFound = mLast.pose_found != 0;
    o.mNormalizedCost = mLast.normalized_cost;
    o.mInitialPose = from_c(mLast.initial_pose);
    o.mEstimatedPose = from_c(mLast.estimated_pose);
    o.mEstimatedCovariance = cov_of(mLast.covariance);
    return o;
}

ScanMatchingSummary ScanMatcherIcpPointToLineHip::OptimizePose(const ScanMatchingQuery& q)
{
    if (mRef) {
        if (!q.mScanData) throw Error(LGS_ERR_INVALID_ARG, "ScanMatcherIcpPointToLineHip: null scan");
        mDev->Check(lgs_icp_ref_optimize_pose(mDev->Handle(), mRef, q.mScanData->Handle(), to_c(q.mInitialPose), &mParams,
                                              &mLast, nullptr),
                    "lgs_icp_ref_optimize_pose");
        ScanMatchingSummary o;
        o.mPoseFound = mLast.pose_found != 0;
        o.mNormalizedCost = mLast.normalized_cost;
        o.mInitialPose = from_c(mLast.initial_pose);
        o.mEstimatedPose = from_c(mLast.estimated_pose);
        o.mEstimatedCovariance = cov_of(mLast.covariance);
        return o;
    }
    if (!mRefScan) throw Error(LGS_ERR_INVALID_ARG, "ScanMatcherIcpPointToLineHip: no reference scan set");
    return OptimizePose(mRefScan, mRefPose, q.mScanData, q.mInitialPose);
}

// --------------------------------------------------------------- GridMapHip
GridMapHip::GridMapHip(DevicePtr dev, double resolution, int patchSize, int numCellsX, int numCellsY,
                       const RobotPose2D<double>& c)
    : mDev(std::move(dev))
{
    mDev->Check(lgs_map_create(mDev->Handle(), resolution, patchSize, numCellsX, numCellsY, c.mX, c.mY, &mMap),
                "lgs_map_create");
}

GridMapHip::~GridMapHip()
{
    if (mMap) lgs_map_destroy(mMap);
}

static lgs_builder_params bp_of(const GridMapBuilderParams& p)
{
    return { p.mUsableRangeMin, p.mUsableRangeMax, p.mProbHit, p.mProbMiss };
}

void GridMapHip::UpdateScan(const ScanData& scan, const RobotPose2D<double>& pose, const GridMapBuilderParams& p)
{
    const lgs_builder_params bp = bp_of(p);
    mDev->Check(lgs_map_update_scan(mDev->Handle(), mMap, scan.Handle(), to_c(pose), &bp), "lgs_map_update_scan");
}

void GridMapHip::ConstructMapFromScans(const std::vector<ScanDataPtr>& scans,
                                       const std::vector<RobotPose2D<double>>& poses,
                                       const GridMapBuilderParams& p)
{
    if (scans.size() != poses.size()) throw Error(LGS_ERR_INVALID_ARG, "ConstructMapFromScans: size mismatch");
    std::vector<const lgs_scan*> hs;
    std::vector<lgs_pose2d> ps;
    for (std::size_t i = 0; i < scans.size(); ++i) {
        hs.push_back(scans[i]->Handle());
        ps.push_back(to_c(poses[i]));
    }
    const lgs_builder_params bp = bp_of(p);
    mDev->Check(lgs_map_construct_from_scans(mDev->Handle(), mMap, hs.data(), ps.data(), (int)hs.size(), &bp),
                "lgs_map_construct_from_scans");
}

static void scan_arrays(const std::vector<ScanDataPtr>& scans, const std::vector<RobotPose2D<double>>& poses,
                        std::vector<const lgs_scan*>& hs, std::vector<lgs_pose2d>& ps, const char* what)
{
    if (scans.size() != poses.size()) throw Error(LGS_ERR_INVALID_ARG, std::string(what) + ": size mismatch");
    for (std::size_t i = 0; i < scans.size(); ++i) {
        hs.push_back(scans[i]->Handle());
        ps.push_back(to_c(poses[i]));
    }
}

void GridMapHip::AppendScan(GridMapHip& localMap, GridMapHip& latestMap, const std::vector<ScanDataPtr>& scans,
                            const std::vector<RobotPose2D<double>>& poses, const GridMapBuilderParams& p)
{
    if (localMap.mDev != latestMap.mDev) throw Error(LGS_ERR_INVALID_ARG, "AppendScan: maps of one device");
    std::vector<const lgs_scan*> hs;
    std::vector<lgs_pose2d> ps;
    scan_arrays(scans, poses, hs, ps, "AppendScan");
    const lgs_builder_params bp = bp_of(p);
    localMap.mDev->Check(lgs_map_append_scan(localMap.mDev->Handle(), localMap.mMap, latestMap.mMap, hs.data(),
                                             ps.data(), (int)hs.size(), &bp),
                         "lgs_map_append_scan");
}

void GridMapHip::ConstructMapsFromScans(const std::vector<GridMapHip*>& maps, const std::vector<int>& nodeIdxMin,
                                        const std::vector<int>& nodeIdxMax, const std::vector<ScanDataPtr>& scans,
                                        const std::vector<RobotPose2D<double>>& poses,
                                        const GridMapBuilderParams& p)
{
    if (maps.empty()) return;
    if (nodeIdxMin.size() != maps.size() || nodeIdxMax.size() != maps.size())
        throw Error(LGS_ERR_INVALID_ARG, "ConstructMapsFromScans: size mismatch");
    std::vector<const lgs_scan*> hs;
    std::vector<lgs_pose2d> ps;
    scan_arrays(scans, poses, hs, ps, "ConstructMapsFromScans");
    std::vector<lgs_map*> ms;
    for (GridMapHip* m : maps) {
        if (!m || m->mDev != maps[0]->mDev)
            throw Error(LGS_ERR_INVALID_ARG, "ConstructMapsFromScans: maps of one device");
        ms.push_back(m->mMap);
    }
    const lgs_builder_params bp = bp_of(p);
    const DevicePtr& dev = maps[0]->mDev;
    dev->Check(lgs_maps_construct_from_scans(dev->Handle(), ms.data(), nodeIdxMin.data(), nodeIdxMax.data(),
                                             (int)ms.size(), hs.data(), ps.data(), (int)hs.size(), &bp),
               "lgs_maps_construct_from_scans");
}

std::unique_ptr<GridMapHip> GridMapHip::ConstructGlobalMap(DevicePtr dev, double resolution, int patchSize,
                                                           const std::vector<ScanDataPtr>& scans,
                                                           const std::vector<RobotPose2D<double>>& poses,
                                                           const GridMapBuilderParams& p)
{
    std::vector<const lgs_scan*> hs;
    std::vector<lgs_pose2d> ps;
    scan_arrays(scans, poses, hs, ps, "ConstructGlobalMap");
    const lgs_builder_params bp = bp_of(p);
    lgs_map* m = nullptr;
    dev->Check(lgs_map_construct_global(dev->Handle(), resolution, patchSize, hs.data(), ps.data(), (int)hs.size(),
                                        &bp, &m),
               "lgs_map_construct_global");
    return std::unique_ptr<GridMapHip>(new GridMapHip(std::move(dev), m));
}

lgs_map_geometry GridMapHip::Geometry() const
{
    lgs_map_geometry g{};
    mDev->Check(lgs_map_get_geometry(mMap, &g), "lgs_map_get_geometry");
    return g;
}

DeviceGridPtr GridMapHip::Grid() const
{
    lgs_grid* g = nullptr;
    mDev->Check(lgs_map_grid(mMap, &g), "lgs_map_grid");
    const lgs_map_geometry geo = Geometry();
    return DeviceGridPtr(new DeviceGrid(mDev, g, geo.num_cells_x, geo.num_cells_y, geo.min_x, geo.min_y,
                                        geo.resolution));
}

void GridMapHip::Download(std::vector<double>* cells, std::vector<uint32_t>* hits,
                          std::vector<uint32_t>* misses) const
{
    const lgs_map_geometry g = Geometry();
    const std::size_t n = (std::size_t)g.num_cells_x * g.num_cells_y;
    if (cells) cells->resize(n);
    if (hits) hits->resize(n);
    if (misses) misses->resize(n);
    mDev->Check(lgs_map_download(mDev->Handle(), mMap, cells ? cells->data() : nullptr,
                                 hits ? hits->data() : nullptr, misses ? misses->data() : nullptr),
                "lgs_map_download");
}

// ------------------------------------------------------------ loop detectors
namespace {

// The Detect() of every loop detector: the queries and their candidate nodes
// as the C-ABI's arrays, one call, and the detected loops appended in query ->
// node order (the reference appends only those).  coarse_of(q) is the query's
// coarse map handle (null: the detector takes none); call(qs, cs, out) makes
// the C call.
template <class CoarseOf, class Call>
void detect_loops(std::vector<LoopDetectionQuery>& queries, std::vector<LoopDetectionResult>& results,
                  CoarseOf&& coarse_of, Call&& call)
{
    results.clear();
    if (queries.empty()) return;
    std::vector<lgs_loop_query> qs;
    std::vector<lgs_loop_candidate> cs;
    for (auto& q : queries) {
        lgs_loop_query c{};
        c.coarse = coarse_of(q);
        c.map = q.mLocalMap->Handle();
        c.local_map_node_pose = to_c(q.mLocalMapNodePose);
        c.local_map_node_index = q.mLocalMapNodeIndex;
        c.first_candidate = (int)cs.size();
        c.num_candidates = (int)q.mPoseGraphNodes.size();
        qs.push_back(c);
        for (const auto& n : q.mPoseGraphNodes)
            cs.push_back(lgs_loop_candidate{ n.mScanData->Handle(), to_c(n.mPose), n.mIndex, 0 });
    }
    std::vector<lgs_loop_result> out(cs.size());
    call(qs, cs, out);
    for (const auto& r : out) {
        if (!r.found) continue;
        LoopDetectionResult o;
        o.mRelativePose = from_c(r.relative_pose);
        o.mStartNodePose = from_c(r.start_node_pose);
        o.mStartNodeIdx = r.start_node_index;
        o.mEndNodeIdx = r.end_node_index;
        o.mEstimatedCovMat = cov_of(r.covariance);
        results.push_back(o);
    }
}
const lgs_grid* no_coarse(const LoopDetectionQuery&) { return nullptr; }

}  // namespace

// ------------------------------------------ LoopDetectorRealTimeCorrelativeHip
LoopDetectorRealTimeCorrelativeHip::LoopDetectorRealTimeCorrelativeHip(
    std::shared_ptr<ScanMatcherRealTimeCorrelativeHip> m, double thr, std::vector<DevicePtr> extra)
    : mScanMatcher(std::move(m)), mScoreThreshold(thr), mExtraDevices(std::move(extra))
{
    for (const auto& d : mExtraDevices)
        if (!d) throw Error(LGS_ERR_INVALID_ARG, "LoopDetectorRealTimeCorrelativeHip: null device");
    if (!(thr > 0.0 && thr <= 1.0))   // the reference asserts this (:21-22)
        throw Error(LGS_ERR_INVALID_ARG, "LoopDetectorRealTimeCorrelativeHip: score threshold must be in (0, 1]");
}

void LoopDetectorRealTimeCorrelativeHip::Detect(std::vector<LoopDetectionQuery>& queries,
                                                std::vector<LoopDetectionResult>& results)
{
    detect_loops(
        queries, results,
        [&](LoopDetectionQuery& q) {
            if (!q.mPrecomputedMap)   // LocalMapInfo caches the coarse map (:52-60)
                q.mPrecomputedMap = std::make_shared<DeviceGrid>(mScanMatcher->ComputeCoarserMap(*q.mLocalMap));
            return q.mPrecomputedMap->Handle();
        },
        [&](auto& qs, auto& cs, auto& out) {   // detected loops in order (:77-88)
            const DevicePtr& dev = mScanMatcher->Dev();
            std::vector<lgs_ctx*> ctxs{ dev->Handle() };
            for (const auto& d : mExtraDevices) ctxs.push_back(d->Handle());
            const lgs_cost_spec spec = spec_of(*mScanMatcher);
            dev->Check(lgs_loop_detect_rtcsm_multi_cost(ctxs.data(), (int)ctxs.size(), &mScanMatcher->Params(), &spec,
                                                        mScoreThreshold, qs.data(), (int)qs.size(), cs.data(),
                                                        (int)cs.size(), out.data()),
                       "lgs_loop_detect_rtcsm_multi_cost");
        });
}

// ------------------------------------------------ LoopDetectorBranchBoundHip
LoopDetectorBranchBoundHip::LoopDetectorBranchBoundHip(std::shared_ptr<ScanMatcherBranchBoundHip> m, double thr)
    : mScanMatcher(std::move(m)), mScoreThreshold(thr)
{
    if (!(thr > 0.0 && thr <= 1.0))   // the reference asserts this (:18-19)
        throw Error(LGS_ERR_INVALID_ARG, "LoopDetectorBranchBoundHip: score threshold must be in (0, 1]");
}

void LoopDetectorBranchBoundHip::Detect(std::vector<LoopDetectionQuery>& queries,
                                        std::vector<LoopDetectionResult>& results)
{
    // lgs_loop_detect_bb builds each map's pyramid (:45-55); detected loops in order (:61-84)
    detect_loops(queries, results, no_coarse, [&](auto& qs, auto& cs, auto& out) {
        const DevicePtr& dev = mScanMatcher->Dev();
        const lgs_cost_spec spec = spec_of(*mScanMatcher);
        dev->Check(lgs_loop_detect_bb_cost(dev->Handle(), &mScanMatcher->Params(), &spec, mScoreThreshold, qs.data(),
                                           (int)qs.size(), cs.data(), (int)cs.size(), out.data()),
                   "lgs_loop_detect_bb_cost");
    });
}

// ------------------------------------------------- LoopDetectorGridSearchHip
LoopDetectorGridSearchHip::LoopDetectorGridSearchHip(std::shared_ptr<ScanMatcherGridSearchHip> m, double thr)
    : mScanMatcher(std::move(m)), mScoreThreshold(thr)
{
    if (!(thr > 0.0 && thr <= 1.0))   // the reference asserts this (:20-21)
        throw Error(LGS_ERR_INVALID_ARG, "LoopDetectorGridSearchHip: score threshold must be in (0, 1]");
}

void LoopDetectorGridSearchHip::Detect(std::vector<LoopDetectionQuery>& queries,
                                       std::vector<LoopDetectionResult>& results)
{
    detect_loops(queries, results, no_coarse, [&](auto& qs, auto& cs, auto& out) {   // loops in order (:58-80)
        const DevicePtr& dev = mScanMatcher->Dev();
        const lgs_cost_spec spec = spec_of(*mScanMatcher);
        dev->Check(lgs_loop_detect_gs_cost(dev->Handle(), &mScanMatcher->Params(), &spec, mScoreThreshold, qs.data(),
                                           (int)qs.size(), cs.data(), (int)cs.size(), out.data()),
                   "lgs_loop_detect_gs_cost");
    });
}

// -------------------------------------------------------- IcpReferenceSetHip
IcpReferenceSetHip::IcpReferenceSetHip(DevicePtr dev, const IcpPointToLineParams& p,
                                       const std::vector<ScanDataPtr>& scans,
                                       const std::vector<RobotPose2D<double>>& robotPoses,
                                       const std::vector<int>& nodeIdxMin, const std::vector<int>& nodeIdxMax)
    : mDev(std::move(dev))
{
    mParams = { p.mNumOfIterationsMax, p.mConvergenceThreshold, p.mUsableRangeMin, p.mUsableRangeMax,
                p.mTranslationRegularizer, p.mRotationRegularizer, p.mMaxCorrespondenceDist, p.mMaxSegmentLength };
    if (scans.empty() || scans.size() != robotPoses.size())
        throw Error(LGS_ERR_INVALID_ARG, "IcpReferenceSetHip: need as many poses as scans, at least one");
    if (nodeIdxMin.empty() || nodeIdxMin.size() != nodeIdxMax.size())
        throw Error(LGS_ERR_INVALID_ARG, "IcpReferenceSetHip: need as many range ends as range starts, at least one");
    std::vector<const lgs_scan*> hs;
    std::vector<lgs_pose2d> poses;
    for (std::size_t k = 0; k < scans.size(); ++k) {
        hs.push_back(scans[k] ? scans[k]->Handle() : nullptr);   // a scan outside every range may be missing
        poses.push_back(to_c(robotPoses[k]));
    }
    mDev->Check(lgs_icp_ref_set_create(mDev->Handle(), hs.data(), poses.data(), (int)hs.size(), nodeIdxMin.data(),
                                       nodeIdxMax.data(), (int)nodeIdxMin.size(), &mParams, &mSet),
                "lgs_icp_ref_set_create");
}

IcpReferenceSetHip::~IcpReferenceSetHip()
{
    if (mSet) lgs_icp_ref_set_destroy(mSet);
}

// --------------------------------------------------------- LoopRefinerIcpHip
LoopRefinerIcpHip::LoopRefinerIcpHip(const LoopRefineGate& g)
{
    mGate = { g.mMinPairs, g.mMaxNormalizedCost, g.mMaxTranslation, g.mMaxRotation };
}

std::vector<int> LoopRefinerIcpHip::Refine(const IcpReferenceSetHip& set, const std::vector<int>& mapIndexOfQuery,
                                           const std::vector<LoopDetectionQuery>& queries,
                                           std::vector<LoopDetectionResult>& results)
{
    if (mapIndexOfQuery.size() != queries.size())
        throw Error(LGS_ERR_INVALID_ARG, "LoopRefinerIcpHip: need one map index per query");
    std::vector<const lgs_icp_ref*> refs;
    std::vector<lgs_loop_query> qs;
    std::vector<lgs_loop_candidate> cs;
    std::vector<lgs_loop_result> recs;
    std::vector<std::size_t> result_of;   // per candidate: its result, or results.size()
    std::size_t next = 0;
    for (std::size_t q = 0; q < queries.size(); ++q) {
        const LoopDetectionQuery& Q = queries[q];
        const lgs_icp_ref* ref = set.Reference(mapIndexOfQuery[q]);
        if (!ref) throw Error(LGS_ERR_INVALID_ARG, "LoopRefinerIcpHip: map index outside the reference set");
        refs.push_back(ref);
        lgs_loop_query c{};
        c.local_map_node_pose = to_c(Q.mLocalMapNodePose);
        c.local_map_node_index = Q.mLocalMapNodeIndex;
        c.first_candidate = (int)cs.size();
        c.num_candidates = (int)Q.mPoseGraphNodes.size();
        qs.push_back(c);
        for (const auto& n : Q.mPoseGraphNodes) {
            if (!n.mScanData) throw Error(LGS_ERR_INVALID_ARG, "LoopRefinerIcpHip: null scan");
            cs.push_back(lgs_loop_candidate{ n.mScanData->Handle(), to_c(n.mPose), n.mIndex, 0 });
            lgs_loop_result r{};
            r.start_node_index = Q.mLocalMapNodeIndex;
            r.end_node_index = n.mIndex;
            std::size_t k = results.size();
            if (next < results.size() && results[next].mStartNodeIdx == Q.mLocalMapNodeIndex &&
                results[next].mEndNodeIdx == n.mIndex) {
                k = next++;
                const LoopDetectionResult& R = results[k];
                r.found = 1;
                r.relative_pose = to_c(R.mRelativePose);
                r.start_node_pose = to_c(R.mStartNodePose);
                // Compound(localMapNode.Pose(), relativePose), glibc's sincos as everywhere on the host
                double sinT, cosT;
                sincos(Q.mLocalMapNodePose.mTheta, &sinT, &cosT);
                r.estimated_pose = { cosT * R.mRelativePose.mX - sinT * R.mRelativePose.mY + Q.mLocalMapNodePose.mX,
                                     sinT * R.mRelativePose.mX + cosT * R.mRelativePose.mY + Q.mLocalMapNodePose.mY,
                                     Q.mLocalMapNodePose.mTheta + R.mRelativePose.mTheta };
                for (int i = 0; i < 9; ++i) r.covariance[i] = R.mEstimatedCovMat.m[i];
            }
            recs.push_back(r);
            result_of.push_back(k);
        }
    }
    if (next != results.size())
        throw Error(LGS_ERR_INVALID_ARG, "LoopRefinerIcpHip: the results are not those of these queries, in order");
    std::vector<int> refined(cs.size(), 0), flags(results.size(), 0);
    std::vector<lgs_icp_summary> sums(cs.size());
    mLast.assign(results.size(), lgs_icp_summary{});
    if (results.empty()) return flags;
    set.Dev()->Check(lgs_loop_refine_icp(set.Dev()->Handle(), refs.data(), qs.data(), (int)qs.size(), cs.data(),
                                         (int)cs.size(), &set.Params(), &mGate, recs.data(), refined.data(), sums.data()),
                     "lgs_loop_refine_icp");
    for (std::size_t c = 0; c < cs.size(); ++c) {
        const std::size_t k = result_of[c];
        if (k == results.size()) continue;
        mLast[k] = sums[c];
        flags[k] = refined[c];
        if (!refined[c]) continue;
        results[k].mRelativePose = from_c(recs[c].relative_pose);
        results[k].mEstimatedCovMat = cov_of(recs[c].covariance);
    }
    return flags;
}

// -------------------------------------------------------- LoopDetectorIcpHip
LoopDetectorIcpHip::LoopDetectorIcpHip(const IcpPointToLineParams& p, const IcpWindow& w, const LoopRefineGate& g)
{
    mParams = { p.mNumOfIterationsMax, p.mConvergenceThreshold, p.mUsableRangeMin, p.mUsableRangeMax,
                p.mTranslationRegularizer, p.mRotationRegularizer, p.mMaxCorrespondenceDist, p.mMaxSegmentLength };
    mWindow = { w.mHalfX, w.mHalfY, w.mHalfTheta, w.mStepXY, w.mStepTheta };
    mGate = { g.mMinPairs, g.mMaxNormalizedCost, g.mMaxTranslation, g.mMaxRotation };
}

void LoopDetectorIcpHip::Detect(const IcpReferenceSetHip& set, const std::vector<int>& mapIndexOfQuery,
                                const std::vector<LoopDetectionQuery>& queries,
                                std::vector<LoopDetectionResult>& results)
{
    if (mapIndexOfQuery.size() != queries.size())
        throw Error(LGS_ERR_INVALID_ARG, "LoopDetectorIcpHip: need one map index per query");
    results.clear();
    mLastBest.clear();
    mLast.clear();
    std::vector<const lgs_icp_ref*> refs;
    std::vector<lgs_loop_query> qs;
    std::vector<lgs_loop_candidate> cs;
    for (std::size_t q = 0; q < queries.size(); ++q) {
        const LoopDetectionQuery& Q = queries[q];
        const lgs_icp_ref* ref = set.Reference(mapIndexOfQuery[q]);
        if (!ref) throw Error(LGS_ERR_INVALID_ARG, "LoopDetectorIcpHip: map index outside the reference set");
        refs.push_back(ref);
        lgs_loop_query c{};
        c.local_map_node_pose = to_c(Q.mLocalMapNodePose);
        c.local_map_node_index = Q.mLocalMapNodeIndex;
        c.first_candidate = (int)cs.size();
        c.num_candidates = (int)Q.mPoseGraphNodes.size();
        qs.push_back(c);
        for (const auto& n : Q.mPoseGraphNodes) {
            if (!n.mScanData) throw Error(LGS_ERR_INVALID_ARG, "LoopDetectorIcpHip: null scan");
            cs.push_back(lgs_loop_candidate{ n.mScanData->Handle(), to_c(n.mPose), n.mIndex, 0 });
        }
    }
    if (cs.empty()) return;
    std::vector<lgs_loop_result> out(cs.size());
    std::vector<int> best(cs.size(), -1);
    std::vector<lgs_icp_summary> sums(cs.size());
    set.Dev()->Check(lgs_loop_detect_icp(set.Dev()->Handle(), refs.data(), qs.data(), (int)qs.size(), cs.data(),
                                         (int)cs.size(), &mParams, &mWindow, &mGate, out.data(), best.data(),
                                         sums.data()),
                     "lgs_loop_detect_icp");
    mLastBest = std::move(best);
    mLast = std::move(sums);
    for (const auto& r : out) {
        if (!r.found) continue;
        LoopDetectionResult o;
        o.mRelativePose = from_c(r.relative_pose);
        o.mStartNodePose = from_c(r.start_node_pose);
        o.mStartNodeIdx = r.start_node_index;
        o.mEndNodeIdx = r.end_node_index;
        o.mEstimatedCovMat = cov_of(r.covariance);
        results.push_back(o);
    }
}

// ---------------------------------------------------- LoopSearcherNearestHip
namespace {

void snapshot_arrays(const std::vector<RobotPose2D<double>>& nodes, const std::vector<LocalMapNodeRange>& maps,
                     std::vector<lgs_pose2d>& poses, std::vector<int>& lo, std::vector<int>& hi)
{
    poses.reserve(nodes.size());
    for (const auto& p : nodes) poses.push_back(to_c(p));
    for (const auto& m : maps) {
        lo.push_back(m.mPoseGraphNodeIdxMin);
        hi.push_back(m.mPoseGraphNodeIdxMax);
    }
}

std::vector<lgs_loop_search_hint> batch_hints(const std::vector<LoopSearchBatchHint>& hints)
{
    std::vector<lgs_loop_search_hint> hs;
    hs.reserve(hints.size());
    for (const auto& h : hints)
        hs.push_back({ h.mLatestNodeIdx, h.mLatestLocalMapIdx, h.mNumOfMaps, 0, h.mAccumTravelDist });
    return hs;
}

// nodeIndices = nodeIdxMin .. nodeIdxMax (:100-102)
LoopCandidate candidate_of(const lgs_loop_search_result& r, int mapIdx, int mapNodeIdx)
{
    LoopCandidate c;
    c.mNodeIndices.resize((size_t)(r.node_idx_max - r.node_idx_min + 1));
    for (size_t i = 0; i < c.mNodeIndices.size(); ++i) c.mNodeIndices[i] = r.node_idx_min + (int)i;
    c.mLocalMapIdx = mapIdx;
    c.mLocalMapNodeIdx = mapNodeIdx;
    return c;
}

}  // namespace

LoopGraphHip::LoopGraphHip(DevicePtr dev, const std::vector<RobotPose2D<double>>& nodes,
                           const std::vector<LocalMapNodeRange>& maps)
    : mDev(std::move(dev)), mNumOfNodes((int)nodes.size()), mNumOfMaps((int)maps.size())
{
    std::vector<lgs_pose2d> poses;
    std::vector<int> lo, hi;
    snapshot_arrays(nodes, maps, poses, lo, hi);
    mDev->Check(lgs_loop_graph_create(mDev->Handle(), poses.data(), mNumOfNodes, lo.data(), hi.data(), mNumOfMaps,
                                      &mGraph),
                "lgs_loop_graph_create");
}

LoopGraphHip::~LoopGraphHip()
{
    if (mGraph) lgs_loop_graph_destroy(mGraph);
}

LoopSearcherNearestHip::LoopSearcherNearestHip(double travelDistThreshold, double nodeDistThreshold,
                                               int numOfCandidateNodes)
{
    mParams.travel_dist_threshold = travelDistThreshold;
    mParams.node_dist_threshold = nodeDistThreshold;
    mParams.num_candidate_nodes = numOfCandidateNodes;
    mParams.pad_ = 0;
}

LoopCandidateVector LoopSearcherNearestHip::Search(const LoopSearchHint& hint) const
{
    std::vector<lgs_pose2d> poses;
    std::vector<int> lo, hi;
    snapshot_arrays(hint.mPoseGraphNodes, hint.mLocalMapPositions, poses, lo, hi);
    const lgs_loop_search_hint h = { hint.mLatestNodeIdx, hint.mLatestLocalMapIdx, (int)lo.size(), 0,
                                     hint.mAccumTravelDist };
    lgs_loop_search_result r;
    const int rc = lgs_loop_search_nearest_host(poses.data(), (int)poses.size(), lo.data(), hi.data(), (int)lo.size(),
                                                &mParams, &h, 1, &r, nullptr);
    if (rc != LGS_OK) throw Error(rc, "lgs_loop_search_nearest_host: invalid loop search hint");
    LoopCandidateVector out;
    if (r.found) out.push_back(candidate_of(r, r.local_map_idx, r.local_map_node_idx));
    return out;
}

std::vector<LoopCandidateVector> LoopSearcherNearestHip::SearchBatch(const LoopGraphHip& graph,
                                                                     const std::vector<LoopSearchBatchHint>& hints) const
{
    const std::vector<lgs_loop_search_hint> hs = batch_hints(hints);
    std::vector<lgs_loop_search_result> res(hs.size());
    std::vector<LoopCandidateVector> out(hs.size());
    if (hs.empty()) return out;
    graph.Dev()->Check(lgs_loop_search_nearest(graph.Handle(), &mParams, hs.data(), (int)hs.size(), res.data(), nullptr),
                       "lgs_loop_search_nearest");
    for (size_t j = 0; j < hs.size(); ++j)
        if (res[j].found) out[j].push_back(candidate_of(res[j], res[j].local_map_idx, res[j].local_map_node_idx));
    return out;
}

std::vector<LoopCandidateVector> LoopSearcherNearestHip::SearchAllMaps(const LoopGraphHip& graph,
                                                                       const std::vector<LoopSearchBatchHint>& hints) const
{
    const std::vector<lgs_loop_search_hint> hs = batch_hints(hints);
    const size_t m = (size_t)graph.NumOfMaps();
    std::vector<lgs_loop_search_result> res(hs.size());
    std::vector<lgs_loop_search_map_best> rows(hs.size() * m);
    std::vector<LoopCandidateVector> out(hs.size());
    if (hs.empty()) return out;
    graph.Dev()->Check(lgs_loop_search_nearest(graph.Handle(), &mParams, hs.data(), (int)hs.size(), res.data(),
                                               rows.data()),
                       "lgs_loop_search_nearest");
    for (size_t j = 0; j < hs.size(); ++j)
        for (size_t i = 0; i < m && res[j].found; ++i)
            if (rows[j * m + i].node_idx >= 0) out[j].push_back(candidate_of(res[j], (int)i, rows[j * m + i].node_idx));
    return out;
}

std::vector<LoopDetectionQuery> GetLoopDetectionQueries(const LoopCandidateVector& loopCandidates,
                                                        const std::vector<LoopCandidateNode>& nodes,
                                                        const std::vector<DeviceGridPtr>& localMaps)
{
    std::vector<LoopDetectionQuery> queries;
    queries.reserve(loopCandidates.size());
    for (const LoopCandidate& c : loopCandidates) {
        LoopDetectionQuery q;
        q.mPoseGraphNodes.reserve(c.mNodeIndices.size());
        for (const int k : c.mNodeIndices) q.mPoseGraphNodes.push_back(nodes.at((size_t)k));
        q.mLocalMap = localMaps.at((size_t)c.mLocalMapIdx);
        const LoopCandidateNode& node = nodes.at((size_t)c.mLocalMapNodeIdx);
        q.mLocalMapNodePose = node.mPose;
        q.mLocalMapNodeIndex = node.mIndex;
        queries.push_back(std::move(q));
    }
    return queries;
}

}  // namespace Hip
}  // namespace MyLidarGraphSlam
