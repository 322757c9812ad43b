/*
 * lgs_hip.h -- C-ABI of the MI355X-native scan-matching + grid-update hot path.
 *
 * This is the drop-in boundary.  Every entry point is plain C:
 * opaque handles, plain pointers and sizes, an int status (LGS_OK == 0), no
 * exceptions and no torch/HIP types in the signatures.  A C++ adapter above this
 * ABI mirrors the reference's plugin interface (my-lidar-graph-slam_amd/host/);
 * INTEGRATION.md shows the reference-side registration.
 *
 * Reference interfaces each entry point replaces (paths relative to the
 * reference root; H/ = include/my_lidar_graph_slam/, C/ = src/my_lidar_graph_slam/):
 *
 *   lgs_grid_precompute_max      PrecomputeGridMap(gridMap, winSize)
 *                                C/mapping/grid_map_builder.cpp:518-536 (via
 *                                ScanMatcherRealTimeCorrelative::ComputeCoarserMap
 *                                C/mapping/scan_matcher_real_time_correlative.cpp:148-153)
 *   lgs_rtcsm_optimize_pose      ScanMatcherRealTimeCorrelative::OptimizePose(
 *                                gridMap, precompMap, scanData, initialPose, thr) const
 *                                C/mapping/scan_matcher_real_time_correlative.cpp:50-145
 *   lgs_rtcsm_optimize_pose_query  ScanMatcherRealTimeCorrelative::OptimizePose(query)
 *                                C/mapping/scan_matcher_real_time_correlative.cpp:31-47
 *                                (the ScanMatcher plugin entry, H/mapping/scan_matcher.hpp:198-199)
 *   lgs_rtcsm_optimize_pose_query_batch  n independent OptimizePose(query) calls
 *                                (C/mapping/scan_matcher_real_time_correlative.cpp:31-47 each)
 *                                as one batched device pipeline
 *   lgs_rtcsm_optimize_pose_batch  LoopDetectorRealTimeCorrelative::Detect's per-node
 *                                loop C/mapping/loop_detector_real_time_correlative.cpp:66-92
 *   lgs_loop_detect_rtcsm        LoopDetectorRealTimeCorrelative::Detect + FindCorrespondingPose
 *                                C/mapping/loop_detector_real_time_correlative.cpp:26-125
 *   lgs_cost_greedy_endpoint     CostGreedyEndpoint::Cost
 *                                C/mapping/cost_function_greedy_endpoint.cpp:32-111
 *   lgs_map_update_scan          GridMapBuilder::UpdateGridMap's insert of one scan
 *                                (bounding box, Expand, per-beam Bresenham + Bayes update)
 *                                C/mapping/grid_map_builder.cpp:149-186
 *   lgs_map_construct_from_scans GridMapBuilder::ConstructMapFromScans
 *                                C/mapping/grid_map_builder.cpp:227-332 (UpdateLatestMap :196-207)
 *   lgs_map_render_gray          MapSaver::DrawMap C/io/map_saver.cpp:276-313
 *   lgs_map_render_gray_region   MapSaver::SaveMapCore's DrawMap of the actual map size
 *                                C/io/map_saver.cpp:413-437
 *   lgs_map_actual_size          GridMap::ComputeActualMapSize H/grid_map/grid_map.hpp:969-1015
 *   lgs_map_download_patches     Patch::IsAllocated H/grid_map/grid_map_patch.hpp:40
 *   lgs_scan_interpolate         ScanInterpolator::Interpolate
 *                                C/mapping/scan_interpolator.cpp:9-98
 *   lgs_maps_construct_from_scans GridMapBuilder::AfterLoopClosure's rebuild of every
 *                                local map C/mapping/grid_map_builder.cpp:62-80
 *   lgs_map_construct_global     GridMapBuilder::ConstructGlobalMap
 *                                C/mapping/grid_map_builder.cpp:83-95
 *   lgs_linsolve_optimize_pose   ScanMatcherLinearSolver::OptimizePose(query)
 *                                C/mapping/scan_matcher_linear_solver.cpp:38-148
 *   lgs_cost_square_error        CostSquareError::Cost / ComputeCovariance
 *                                C/mapping/cost_function_square_error.cpp:21-58, :112-135
 *   lgs_cost_square_error_batch  the same at n (map, scan, sensor pose) items in one launch
 *   lgs_summaries_apply_cost_sq  what the correlative, branch-and-bound and grid-search matchers
 *                                return when constructed with CostSquareError
 *   lgs_hc_sq_optimize_pose_query ScanMatcherHillClimbing::OptimizePose(query) with CostSquareError
 *                                C/mapping/scan_matcher_hill_climbing.cpp:26-109
 *   lgs_grid_precompute_pyramid  PrecomputeGridMaps C/mapping/grid_map_builder.cpp:471-495
 *   lgs_bb_optimize_pose_batch   ScanMatcherBranchBound::OptimizePose(map, pyramid, scan, pose, thr)
 *                                C/mapping/scan_matcher_branch_bound.cpp:47-154
 *   lgs_bb_optimize_pose_query   ScanMatcherBranchBound::OptimizePose(query) :29-44
 *   lgs_loop_detect_bb           LoopDetectorBranchBound::Detect + FindCorrespondingPose
 *                                C/mapping/loop_detector_branch_bound.cpp:26-117
 *   lgs_gs_optimize_pose_batch   ScanMatcherGridSearch::OptimizePose(map, scan, pose, thr)
 *                                C/mapping/scan_matcher_grid_search.cpp:44-114
 *   lgs_gs_optimize_pose_query   ScanMatcherGridSearch::OptimizePose(query) :31-41
 *   lgs_loop_detect_gs           LoopDetectorGridSearch::Detect + FindCorrespondingPose
 *                                C/mapping/loop_detector_grid_search.cpp:26-106
 *
 * Threading: one lgs_ctx per matcher instance (the reference's frontend and
 * loop detector own distinct matchers, C/slam_launcher.cpp:774-775, :835).  A
 * context owns one HIP stream and its scratch; calls on one context must not
 * overlap, calls on different contexts may.
 *
 * Numerics: fp64 throughout.  Cell indices, hit/miss counts, map cells, the
 * correlative argmax/score and the Gauss-Newton refine (glibc's
 * sincos/pow restated on the device, sums in beam order) are bit-exact with the
 * reference CPU path; greedy-endpoint costs/covariances agree to within 1e-5
 * (device exp differs from glibc in the last ulp).
 */
#ifndef LGS_HIP_H
#define LGS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: lgs_carmen_load gained ids_bytes (include/lgs_io.h), options 6/12/14/16
 * retired, options 22/23 and lgs_loop_records_allgather added */
#define LGS_ABI_VERSION 2

/* status codes */
#define LGS_OK               0
#define LGS_ERR_INVALID_ARG  1
#define LGS_ERR_HIP          2
#define LGS_ERR_NO_DEVICE    3
#define LGS_ERR_OOM          4
#define LGS_ERR_INTERNAL     5

typedef struct lgs_ctx  lgs_ctx;   /* device, stream, scratch arena */
typedef struct lgs_grid lgs_grid;  /* device-resident dense fp64 grid */
typedef struct lgs_scan lgs_scan;  /* device-resident scan (ScanData<double>) */

/* RobotPose2D<double> (H/pose.hpp:14-42) */
typedef struct { double x, y, theta; } lgs_pose2d;

/* Host view of a ScanData<double> (H/sensor/sensor_data.hpp:65-158) */
typedef struct {
    const double* ranges;        /* n */
    const double* angles;        /* n */
    int n;
    lgs_pose2d rel_sensor_pose;  /* RelativeSensorPose() */
    double min_range, max_range; /* MinRange(), MaxRange() */
} lgs_scan_host;

/* ScanMatcherRealTimeCorrelative ctor arguments
 * (H/mapping/scan_matcher_real_time_correlative.hpp:19-25) */
typedef struct {
    int low_resolution;
    double range_x, range_y, range_theta;
    double scan_range_max;
} lgs_rtcsm_params;

/* CostGreedyEndpoint *member* values (C/mapping/cost_function_greedy_endpoint.cpp:10-28).
 * The reference launcher passes (stddev, scale) into the (scale, stddev) slots
 * (C/slam_launcher.cpp:70-72); callers fill these with the members as constructed. */
typedef struct {
    double usable_range_min, usable_range_max;
    double hit_and_missed_dist, occupancy_threshold;
    int kernel_size;
    double scaling_factor;
    double standard_deviation;
} lgs_cost_ge_params;

/* ScanMatchingSummary (H/mapping/scan_matcher.hpp:147-174) + diagnostics */
typedef struct {
    int pose_found;
    double normalized_cost;
    lgs_pose2d initial_pose;
    lgs_pose2d estimated_pose;
    double covariance[9];         /* row-major 3x3 */
    /* diagnostics */
    double score_max;             /* best (fine) score, sequential fp64 beam-order sum */
    double score_threshold;       /* normalizedScoreThreshold * NumOfScans() */
    int best_win[3];              /* x, y, theta window indices of the argmax */
    int win[3];                   /* winX, winY, winTheta */
    double steps[3];              /* stepX, stepY, stepTheta */
    lgs_pose2d best_sensor_pose;
    int64_t coarse_blocks;        /* coarse blocks scored: all of them, or those superblock pruning kept */
    int64_t fine_blocks;          /* coarse blocks refined on the fine map */
    int guard_hits;               /* projections near a cell boundary re-checked on host */
    int fixups;                   /* 1 if any device index differed from glibc and was patched */
    int slow_path;                /* 1 if the exact dense fallback was taken */
} lgs_rtcsm_summary;

/* ---- context ---- */
int  lgs_ctx_create(int device, lgs_ctx** out);
void lgs_ctx_destroy(lgs_ctx* ctx);
const char* lgs_ctx_last_error(const lgs_ctx* ctx);
int  lgs_ctx_synchronize(lgs_ctx* ctx);
void* lgs_ctx_stream(lgs_ctx* ctx);       /* hipStream_t, for interop (torch) */
int  lgs_abi_version(void);

/* Test/diagnostic knobs (never needed in production):
 *  LGS_OPT_GUARD_EPS     boundary guard in cells (default 1e-9)
 *  LGS_OPT_FORCE_DENSE   1 = refine every coarse block above threshold
 *  LGS_OPT_INJECT_INDEX  1 = corrupt every guarded device index (exercises the fix-up path)
 *  LGS_OPT_GUARD_CAP     max guard records inspected before full host re-projection */
#define LGS_OPT_GUARD_EPS     1
#define LGS_OPT_FORCE_DENSE   2
#define LGS_OPT_INJECT_INDEX  3
#define LGS_OPT_GUARD_CAP     4
#define LGS_OPT_PROFILE       5   /* 1 = time every kernel launch with HIP events on the ctx stream */
#define LGS_OPT_PROFILE_MASK  7   /* time only the kernels whose lgs_kernel_stat index bit is set (0 = off) */
#define LGS_OPT_SPIN_SYNC     8   /* 1 (default) = spin on the stream when waiting for results, 0 = blocking wait */
#define LGS_OPT_SKIP_MASK     10  /* diagnostics only: bitmask of kernels (lgs_ctx_kernel_stats order) not launched -- results are invalid */
#define LGS_OPT_SUPER_PRUNE   9   /* 1 (default) = skip coarse blocks whose 4x4-superblock bound is below the seed score, 0 = evaluate every coarse block */
#define LGS_OPT_RAY_CHUNK_KEYS 13  /* ray-cast keys per emit/sort/apply pass (default 2^28, max 2^30); more keys are cast in scan order over several passes */
#define LGS_OPT_LANES_MIN_BATCH 11 /* pruned coarse stage: the kept-superblock work list (lane-per-block sums) for batches of at least this many matches (default 2; 1 = always), else the row kernel */
#define LGS_OPT_LINSOLVE_SPLIT 17 /* 1 (default) = a lone ScanMatcherLinearSolver refine of <= 1280 beams runs one workgroup per 64 beams (in-launch hand-off per pass) when they fit the device at once, 0 = one workgroup */
#define LGS_OPT_HANDOFF_SPIN_US 18 /* split refine: bound of a workgroup's wait for the others (default 200000 us); on time-out the refine is rerun on one workgroup.  0 = force that fallback (tests) */
#define LGS_OPT_PEER_COPY     19  /* lgs_loop_detect_rtcsm_multi, on the shard's ctx: 0 (default) = maps copied device to device (peer access enabled when the devices differ and allow it, else staged through pinned host memory), 1 = always staged through host memory */
#define LGS_OPT_PRUNE_MIN_SUPER 21 /* superblock pruning only for windows of at least this many superblocks per angle (default 1); smaller windows score every coarse block */
#define LGS_OPT_COOP_TILES    22  /* K3 one-launch sort (k_sort_wide): at most this many tiles for this ctx's launches (default -1 = the device's co-residency capacity, shared by every ctx of the process; 0 = always the multi-pass sort) */
#define LGS_OPT_SORT_BARRIER_US 23 /* bound of a one-launch sort tile's wait at its grid barrier (default 50000 us); on time-out the call reports LGS_ERR_INTERNAL.  0 = time out at once (tests) */
#define LGS_OPT_FINE_STAGED   24  /* 1 (default) = batched fine evaluation of LowRes-5 blocks stages each beam's window in LDS (k_fine_regs), 0 = per-beam gathers (k_fine_lanes) */
#define LGS_OPT_SMALL_WINDOW  25  /* 1 (default) = windows with one coarse block per angle (2 winX < LowRes, 2 winY < LowRes, LowRes 2..7, map width >= LowRes, <= 2048 valid beams) search in one launch (k_match_small: no coarse map), 0 = the general path */
#define LGS_OPT_POST_RECORDS  26  /* 1 (default) = a match call's result records reach the host through a kernel that writes them (and a completion flag) into pinned memory, the host spinning on the flag; 0 = a device-to-host copy and a stream event */
#define LGS_OPT_FUSED_PLANES  27  /* 1 (default) = the per-query coarse-map precompute writes the phase planes AND the octet superblock units in one pass from the fine map (k_planes_super, LowRes 5), 0 = the precompute + k_super_planes passes */
#define LGS_OPT_PRIORITY_TAIL 28  /* 0 (default) = one stream; 1 = a correlative batch's stages after the coarse-map builds run on a second stream of the device's highest priority (behind an event), so that other contexts' plane builds cannot queue ahead of its latency-bound tail */
#define LGS_OPT_HV_FULL       29  /* A/B: 1 = the superblock pass (k_super_hv) stores each 16-byte unit whole from two quads' maxima; 0 (default) = each quad's halves */
#define LGS_OPT_SPLIT_CHUNKS  30  /* A/B: 1 = a correlative call of 32..64 matches runs as two chunks of half the size (the two buffer banks overlap); 0 (default) = one chunk per 64 */
#define LGS_OPT_DEVICE_HITS   31  /* 1 (default) = lgs_maps_construct_from_scans / lgs_map_construct_global form the hit points (glibc sincos restated), boxes, ray cells and key offsets on the device; 0 = on the host */
#define LGS_OPT_SEED_WIDE     32  /* batches: the pruning bound seeded from the best members of this many candidate superblocks (5..16, default 12; the 4 best members fine-scored); 0..4 = 4 candidates in one launch */
#define LGS_OPT_ZERO_TILES    33  /* 1 (default) = the per-map passes of a correlative batch skip the stores of a tile whose inputs are all +0 when that set's buffer already holds the tile's +0 outputs (the precompute: one word per tile; the superblock pass k_super_hv: one bit per thread, a 64-bit word per set, plane and wave; kept per bank, set and layout); 0 = everything stored */
#define LGS_OPT_DEVICE_TIMING 34  /* 1 = while LGS_OPT_PROFILE(_MASK) times a kernel of a correlative batch chunk, time it on the device instead of with stream events: its workgroups stamp s_memrealtime (100 MHz) at start and end into per-chunk words (two relaxed atomic maxima per workgroup), copied back with the chunk's records; a launch's time is its first workgroup's start to its last workgroup's end (the execution span rocprofv3 reports, not the wait of a stream event for the CUs).  Launches outside a chunk's main chain keep event timing.  0 (default) = events */
#define LGS_OPT_LEAN_PROJECT  35  /* 1 (default) = batched pruned correlative chunks (work list, wide seed, staged fine evaluation) write only the superblock base of every (angle, beam) plus per-beam / per-angle trig tables, and the kernels that stage a coarse-base or cell row form it themselves with the projection's own arithmetic (bit-identical); 0 = every row materialised (the guard fix-up reruns and lone matches always materialise) */
#define LGS_OPT_PGCG_GRID_NODES 36 /* lgs_pg_cg_solve: systems of at least this many nodes run over many workgroups, two launches per CG pass (default 1280: up to there the vectors of the one-workgroup solve fit LDS and it is the faster one); smaller ones in one persistent workgroup.  0 = always the grid, 2^31 - 1 = never */
#define LGS_OPT_FAST_ROWS     37  /* 1 (default) = a lean batch's superblock pass forms a wave's 64 hit-point cells with a shorter fp64 chain (csrc/fast_cell.hpp) wherever every lane's cell is certified equal to the exact chain's and unguarded, and with the exact chain otherwise (bit-identical records); 0 = the exact chain always */
#define LGS_OPT_HV_INZERO     38  /* 1 (default) = a thread of the superblock pass (k_super_hv) whose whole input footprint lies in precompute tiles that read all-(+0) inputs this call (k_hv_inzero: one 64-bit lane mask per set and wave) issues none of its loads; 0 = no mask, every thread loads (A/B inside one build, tests).  Batches of two or more maps only (a lone call is latency-bound and takes no mask); needs LGS_OPT_ZERO_TILES 1 */
#define LGS_OPT_SELECT_LIST   41  /* batched pruned correlative chunks that take the kept-superblock work list (LGS_OPT_LANES_MIN_BATCH): the largest number of coarse blocks per match (K = angles x blocks per angle) up to which the refine candidates are selected from the listed superblocks' blocks alone, in one launch of one workgroup per match that also writes the dense list (k_select_list); above it, and with 0 = never, k_select rules on every coarse block and k_compact writes the dense list (the same bytes either way).  Default 524288, what the kernel's 64 KB of LDS hold (larger values mean the same) */
#define LGS_OPT_LIST_ORDER    42  /* batched pruned correlative chunks that take the kept-superblock work list: 1 = the list is written superblock-major with the angles ascending within a superblock, and the edge angles ascending, by one workgroup per match with prefix sums (k_keep_ord: no atomics on the list, the same list every run; batches whose keep masks, 8 bytes per search angle, exceed 32 KB keep k_keep); 0 = k_keep appends each angle's kept superblocks with an atomic add, in the completion order of its workgroups.  The same entries, counters and records either way.  Default 1 */
#define LGS_OPT_LIST_PAIRS    43  /* the same batches: 1 = the exact coarse pass gives a lane two neighbouring blocks of a superblock row and gathers both with one 16-byte load per beam, 8 listed superblocks per wave (k_coarse_list_p), wherever every pair's read stays inside the match's phase planes (csrc/coarse_pair.hpp); 0 = one block and one 8-byte load per lane, 4 superblocks per wave (k_coarse_list_c).  The same scores and flags either way.  Default 0 (measured slower: the exact coarse pass +24 % on the default workload) */
#define LGS_OPT_POISON_WS     15/* diagnostics: 1 = fill every match workspace and record with 0xFF bytes before the batch runs (any read-before-write shows up) */
int  lgs_ctx_set_option(lgs_ctx* ctx, int option, double value);

/* Diagnostics: copy one intermediate buffer of item `item` of the context's
 * last correlative batch to `out` (at most cap bytes; *bytes = its full size).
 * which: 0 sbound [T*nsb2 f64], 1 part_c [nparts f64], 2 part_k [nparts i64],
 * 3 Lp at byte 0, Lc[4] f64 at byte 64, 4 tedge [T i32] (1 = flagged by
 * the last enqueue of item 0, else 0), 5 cbase [2*(T*Nv+pad) i32],
 * 6 idx [T*Nv int2], 7 cscore [K f64], 8 coarse phase planes [lr*lr planes
 * of Hqp x Wqp f64, DESIGN.md §2], 9 superblock planes [fp16], 10 the
 * in-masks of the item's set after the last batch [one u64 per wave of a
 * plane's k_super_hv threads: bit l = lane l loaded nothing; empty when the set
 * had none], 11 its out-masks [lr*lr planes x waves u64: bit l = everything
 * lane l stores holds +0; empty without LGS_OPT_ZERO_TILES].
 * The selection of the refine candidates (empty for one-block windows):
 * 12 list [nseg segments of 1024 i32: the first segcnt[s] of segment s are its
 * selected blocks, ascending], 13 segcnt [nseg i32], 14 nsel [i32] followed
 * by dlist [K i32: the first nsel are the selected blocks, ascending; empty
 * when the batch's fine evaluator takes no dense list], 15 one i32: 1 when
 * k_select_list wrote the item's selection, 0 when k_select (+ k_compact) did.
 * 16 cflag [K u8].  The kept-superblock work list (empty when the batch took
 * none): 17 the item's entries [region i32, t << 6 | superblock: the first
 * cnt[0] are listed], 18 its counters [16 i32: 0 entries, 1 edge angles],
 * 19 its edge angles [Tmax i32: the first cnt[1] are listed]. */
int  lgs_debug_item_buffer(lgs_ctx* ctx, int item, int which, void* out, size_t cap, size_t* bytes);

/* Diagnostics: the device's restatements of glibc's sincos() (op 0: out[2i] =
 * sin x[i], out[2i+1] = cos x[i]) and pow(x, 3.0) (op 1: out[i]) evaluated on
 * the GPU for n host inputs (csrc/glibc_math.hpp; tests compare them with the
 * host libm bit for bit).  Ops 2 and 3 are the device's own sqrt(x[i]) and
 * fmod(x[i], 2 pi), which the pose-graph linearisation (k_pglm.hip) relies on
 * being the host's bits. */
int  lgs_debug_libm(lgs_ctx* ctx, int op, const double* x, int n, double* out);

/* Diagnostics: the K3 sort (csrc/k_sort.hip, the stable radix sort behind
 * every ray-cast pass) of n host keys on bits [lo, lo + bits), through the
 * device; out receives the sorted keys. */
int  lgs_debug_keysort(lgs_ctx* ctx, const unsigned* keys, unsigned* out, long long n, int lo, int bits);

/* Diagnostics: cross-context copies made by lgs_loop_detect_rtcsm_multi onto
 * this context since it was created: device to device (same device or peer
 * access over xGMI) and staged through pinned host memory. */
int  lgs_debug_copy_counters(const lgs_ctx* ctx, long long* direct, long long* staged);

/* Diagnostics, checked build only (liblgs_hip_checked.so, compiled with
 * LGS_CHECK_OFFSETS): the correlative consumers test every
 * coarse / superblock plane offset they form or read against its padded
 * plane.  out[0] = offsets checked, out[1] = violations, out[2] = the first
 * violation (kind << 60 | angle << 32 | beam; kind 1 coarse, 2 superblock),
 * out[3] = its offset; since the last reset (reset != 0 zeroes them after
 * the read).  The product build returns LGS_ERR_INVALID_ARG (no checks). */
int  lgs_debug_offset_checks(lgs_ctx* ctx, int reset, unsigned long long* out);

/* Per-kernel statistics gathered while LGS_OPT_PROFILE is on.  algo_bytes is
 * the algorithmic byte count of DESIGN.md §Roofline (e.g. 8 B per coarse-score
 * lookup), summed over launches; total_ms sums hipEventElapsedTime, or with
 * LGS_OPT_DEVICE_TIMING each launch's execution span (first workgroup start to
 * last workgroup end); dispatch_ms (device timing only, else = total_ms) sums
 * the span from the end of the chunk's previous device-timed launch on the
 * same stream to the launch's end -- what a stream event or a rocprofv3
 * dispatch duration counts: the execution plus the wait for CUs held by other
 * streams' kernels (r06). */
typedef struct {
    char name[32];
    int64_t launches;
    double total_ms;
    double algo_bytes;
    double dispatch_ms;
} lgs_kernel_stat;
int  lgs_ctx_kernel_stats(lgs_ctx* ctx, lgs_kernel_stat* out, int cap);  /* returns count (>=0) or -status */
int  lgs_ctx_reset_stats(lgs_ctx* ctx);
/* Correlative-match counters since the last lgs_ctx_reset_stats, over every
 * OptimizePose / loop-detect match on the context (always collected):
 * out4 = {matches, coarse blocks scored, coarse blocks a dense search scores
 * (sum of the plans' K), matches that used superblock pruning}. */
int  lgs_ctx_match_counters(lgs_ctx* ctx, int64_t* out4);

/* ---- grids: dense row-major fp64, cell (x,y) at y*w+x, 0.0 = unknown ---- */
int  lgs_grid_create(lgs_ctx* ctx, int w, int h, double min_x, double min_y,
                     double resolution, lgs_grid** out);
/* non-owning view over existing device memory (e.g. a torch tensor) */
int  lgs_grid_wrap(lgs_ctx* ctx, double* device_cells, int w, int h, double min_x,
                   double min_y, double resolution, lgs_grid** out);
void lgs_grid_destroy(lgs_grid* grid);
int  lgs_grid_upload(lgs_ctx* ctx, lgs_grid* grid, const double* host_cells);
/* Patch-native upload of a reference GridMapType (GridMap<BinaryBayesGridCell
 * <double>>, H/grid_map/grid_map.hpp:295-317 mPatches, H/grid_map/
 * grid_map_patch.hpp:15-193): patches[py * npx + px] = PatchAt(px, py).Data()
 * (its patch_size^2 cells, cell (x, y) of the patch at y * patch_size + x) or
 * NULL for an unallocated patch (reads Unknown = 0.0, as GridMap::Value
 * does).  Each cell is cell_bytes bytes with its fp64 value at value_offset
 * (BinaryBayesGridCell<double>: 16 and 8 -- vptr, mValue).  The grid must be
 * npx*patch_size x npy*patch_size.  Only allocated patches cross PCIe, as
 * their raw cells (host copies into pinned staging overlap the DMA); a kernel
 * extracts the values into the dense grid and zero-fills unallocated patches.
 * Replaces INTEGRATION.md §2's Flatten (one virtual Value() per cell) +
 * lgs_grid_upload of the whole dense map. */
int  lgs_grid_upload_patches(lgs_ctx* ctx, lgs_grid* grid, const void* const* patches, int npx, int npy,
                             int patch_size, int cell_bytes, int value_offset);
int  lgs_grid_download(lgs_ctx* ctx, const lgs_grid* grid, double* host_cells);
int  lgs_grid_fill(lgs_ctx* ctx, lgs_grid* grid, double value);
int  lgs_grid_info(const lgs_grid* grid, int* w, int* h, double* min_x, double* min_y,
                   double* resolution);
double* lgs_grid_device_ptr(lgs_grid* grid);

/* PrecomputeGridMap(grid, win) into `out` (same geometry). */
int  lgs_grid_precompute_max(lgs_ctx* ctx, const lgs_grid* in, int win, lgs_grid* out);

/* ---- scans: a host copy, and a device copy resident in HBM once made ----
 * lgs_scan_create copies the ranges/angles (host memory only: no device
 * work, no synchronisation).  The first call that reads the scan on the
 * device copies it there, on that call's context (pooled device buffers), and
 * it stays resident until lgs_scan_destroy.  A scan belongs to the context
 * that created it; other contexts use clones (lgs_loop_detect_rtcsm_multi
 * re-creates them from the host copy).  Copies are waited for where a scan is
 * read on a context other than the one that made them. */
int  lgs_scan_create(lgs_ctx* ctx, const lgs_scan_host* host, lgs_scan** out);
void lgs_scan_destroy(lgs_scan* scan);
/* Number of beams, and (if the pointers are non-null) a copy of the ranges and
 * angles of `scan` into caller arrays of at least that many doubles. */
int  lgs_scan_get(const lgs_scan* scan, int* n, double* ranges, double* angles);
/* ScanInterpolator::Interpolate (C/mapping/scan_interpolator.cpp:9-98): a new
 * device-resident scan whose points are spaced dist_scans apart along the
 * polyline of `in`'s points, except across gaps of >= dist_threshold_empty
 * (launcher JSON "ScanInterpolator": DistScans 0.05, DistThresholdEmpty 0.25).
 * The relative sensor pose and min/max range are copied.  The recurrence is
 * sequential and uses glibc sincos/atan2/sqrt, so it runs on the host; the
 * result is a scan like lgs_scan_create's.  LGS_ERR_INVALID_ARG unless
 * 0 < dist_scans <= dist_threshold_empty (both finite) and every point of
 * `in` is finite: the reference's loop would never end otherwise. */
int  lgs_scan_interpolate(lgs_ctx* ctx, const lgs_scan* in, double dist_scans, double dist_threshold_empty,
                          lgs_scan** out);

/* ---- correlative scan matcher ---- */
int  lgs_rtcsm_optimize_pose(lgs_ctx* ctx, const lgs_grid* grid, const lgs_grid* coarse,
                             const lgs_rtcsm_params* params,
                             const lgs_cost_ge_params* cost,
                             const lgs_scan* scan, lgs_pose2d initial_pose,
                             double normalized_score_threshold,
                             lgs_rtcsm_summary* out);
/* OptimizePose(query): coarse map computed on device, threshold DBL_MIN */
int  lgs_rtcsm_optimize_pose_query(lgs_ctx* ctx, const lgs_grid* grid,
                                   const lgs_rtcsm_params* params,
                                   const lgs_cost_ge_params* cost,
                                   const lgs_scan* scan, lgs_pose2d initial_pose,
                                   lgs_rtcsm_summary* out);
/* n independent OptimizePose(query) calls (each query: its map, scan and
 * initial pose; every query computes its own coarse map, as the reference's
 * OptimizePose(query) does, even when two queries pass the same map).  One
 * batched device pipeline: every stage is a single launch over all n queries.
 * The maps of one call must share size and resolution.  out[j] is
 * bit-identical to lgs_rtcsm_optimize_pose_query on query j. */
int  lgs_rtcsm_optimize_pose_query_batch(lgs_ctx* ctx, const lgs_grid* const* grids,
                                         const lgs_rtcsm_params* params,
                                         const lgs_cost_ge_params* cost,
                                         const lgs_scan* const* scans,
                                         const lgs_pose2d* initial_poses, int n,
                                         lgs_rtcsm_summary* out);
/* n independent matches against one grid and its coarse map, as one batched
 * device pipeline (loop-closure candidates, C/.../loop_detector_real_time_correlative.cpp:66) */
int  lgs_rtcsm_optimize_pose_batch(lgs_ctx* ctx, const lgs_grid* grid, const lgs_grid* coarse,
                                   const lgs_rtcsm_params* params,
                                   const lgs_cost_ge_params* cost,
                                   const lgs_scan* const* scans, const lgs_pose2d* initial_poses,
                                   int n, double normalized_score_threshold,
                                   lgs_rtcsm_summary* out);
/* Every coarse and fine score of the search window (kernel-level parity).
 * dims[7] = {winX, winY, winTheta, ncx, ncy, nfx, nfy}; pass NULL score
 * buffers to query dims.  coarse_scores[T][ncx][ncy], fine_scores[T][nfx][nfy]. */
int  lgs_rtcsm_dense_scores(lgs_ctx* ctx, const lgs_grid* grid, const lgs_grid* coarse,
                            const lgs_rtcsm_params* params, const lgs_scan* scan,
                            lgs_pose2d initial_pose, double* coarse_scores,
                            double* fine_scores, int* dims);

/* ---- occupancy-grid maps: GridMap<BinaryBayesGridCell<double>> ----
 * Geometry follows the reference exactly (H/grid_map/grid_map.hpp): square
 * patches of patch_size cells, minPos anchoring, Resize/Expand with the
 * negative patch-index quirk (:905-915).  Cells live on the device (dense,
 * row-major over the whole patch grid, 0.0 = unknown); the per-beam
 * Bresenham ray-cast and binary Bayes update run on the device in the
 * reference's update order (beam order; misses along a ray before its hit),
 * so every cell value is bit-exact. */
typedef struct lgs_map lgs_map;

/* GridMapBuilder ctor arguments used by the ray-cast (C/mapping/grid_map_builder.cpp:20-45) */
typedef struct {
    double usable_range_min, usable_range_max;
    double prob_hit, prob_miss;
} lgs_builder_params;

typedef struct {
    double resolution;
    int patch_size;
    int num_patches_x, num_patches_y;
    int num_cells_x, num_cells_y;
    double min_x, min_y;
} lgs_map_geometry;

/* GridMap(res, patchSize, numCellsX, numCellsY, centerPos) (H/grid_map/grid_map.hpp:337-391) */
int  lgs_map_create(lgs_ctx* ctx, double resolution, int patch_size, int num_cells_x,
                    int num_cells_y, double center_x, double center_y, lgs_map** out);
void lgs_map_destroy(lgs_map* map);
int  lgs_map_get_geometry(const lgs_map* map, lgs_map_geometry* out);
/* Non-owning grid view of the map's cells (valid until the next geometry change
 * or lgs_map_destroy); lgs_grid_destroy on a view is a no-op. */
int  lgs_map_grid(lgs_map* map, lgs_grid** out);
/* One scan into the map as GridMapBuilder::UpdateGridMap does after choosing
 * the local map (C/mapping/grid_map_builder.cpp:149-186): bounding box,
 * Expand(.., 5.0), then the ray-cast update. */
int  lgs_map_update_scan(lgs_ctx* ctx, lgs_map* map, const lgs_scan* scan, lgs_pose2d robot_pose,
                         const lgs_builder_params* params);
/* GridMapBuilder::ConstructMapFromScans (C/mapping/grid_map_builder.cpp:227-332):
 * Resize to the bounding box of all scans (topRight starts at DBL_MIN), Reset,
 * then ray-cast every scan in order.  Called again on the same map with the
 * window of UpdateLatestMap (:196-207: the previous scans, less at most the
 * oldest, plus one new scan; same poses, parameters and geometry), only the
 * cells the new or the dropped scan touch are recomputed (DESIGN.md §4.4b;
 * same cells, counts and patch flags as a full rebuild).  Such an incremental
 * call returns before its device work has finished: reads of the map through
 * this library wait for it (on any context); lgs_grid_device_ptr users
 * synchronise the context first.  An internal error of that work is reported
 * by the map's next rebuild (LGS_ERR_INTERNAL, e.g. "grid barrier timed out"
 * when the one-launch sort's tiles could not be co-resident): the update
 * kernels of that step have then run over unsorted keys, so the cells of this
 * map AND of the local map an lgs_map_append_scan step inserted into are
 * undefined.  The library drops the latest map's incremental state (its next
 * call rebuilds it in full); the caller must rebuild the local map
 * (lgs_map_construct_from_scans) before reading it again. */
int  lgs_map_construct_from_scans(lgs_ctx* ctx, lgs_map* map, const lgs_scan* const* scans,
                                  const lgs_pose2d* robot_poses, int n,
                                  const lgs_builder_params* params);
/* GridMapBuilder::AppendScan (C/mapping/grid_map_builder.cpp:48-59): the
 * newest scan scans[n-1] at robot_poses[n-1] inserted into `local` exactly as
 * lgs_map_update_scan does (UpdateGridMap :98-193), and `latest` rebuilt from
 * all n scans exactly as lgs_map_construct_from_scans does (UpdateLatestMap
 * :196-207; n = min(node count, NumOfScansForLatestMap)).  Same results as the
 * two calls; both ray-casts share one device pass (one cast of the new scan
 * when the two maps' cells of it differ by a whole-cell shift).  Incremental
 * and asynchronous as lgs_map_construct_from_scans.  local != latest. */
int  lgs_map_append_scan(lgs_ctx* ctx, lgs_map* local, lgs_map* latest, const lgs_scan* const* scans,
                         const lgs_pose2d* robot_poses, int n, const lgs_builder_params* params);

/* Diagnostics: how a map's ConstructMapFromScans / AppendScan rebuilds ran
 * (DESIGN.md §4.4b): incremental steps (the window gained one scan and lost
 * at most its oldest, same geometry: only the touched cells recomputed) and
 * full rebuilds.  Both zero for a map never rebuilt. */
int  lgs_debug_map_rebuilds(const lgs_map* m, long long* incremental, long long* full);

/* GridMapBuilder::AfterLoopClosure's map loop (C/mapping/grid_map_builder.cpp:62-80):
 * ConstructMapFromScans(maps[i], poseGraph, idx_min[i], idx_max[i]) for every
 * i, where node k of the pose graph is (scans[k], robot_poses[k]) and
 * idx_min[i] <= idx_max[i] < n_nodes (inclusive ranges; they may overlap).
 * The maps must be distinct.  Each map is resized and reset as
 * lgs_map_construct_from_scans does; all maps then share one ray-cast pass,
 * which gives the same cells as constructing them one after another. */
int  lgs_maps_construct_from_scans(lgs_ctx* ctx, lgs_map* const* maps, const int* idx_min,
                                   const int* idx_max, int n_maps, const lgs_scan* const* scans,
                                   const lgs_pose2d* robot_poses, int n_nodes,
                                   const lgs_builder_params* params);
/* GridMapBuilder::ConstructGlobalMap (C/mapping/grid_map_builder.cpp:83-95): a
 * new map of (resolution, patch_size) with 0 x 0 cells centred at (0, 0),
 * then ConstructMapFromScans over all n nodes.  Any number of scans: the
 * ray-cast runs in passes of at most LGS_OPT_RAY_CHUNK_KEYS keys. */
int  lgs_map_construct_global(lgs_ctx* ctx, double resolution, int patch_size,
                              const lgs_scan* const* scans, const lgs_pose2d* robot_poses, int n,
                              const lgs_builder_params* params, lgs_map** out);
/* MapSaver::DrawMap (C/io/map_saver.cpp:276-313) over the whole map: one gray
 * byte per cell, (uint8)((1 - p) * 255) for 0 < p <= 1 and 192 otherwise, rows
 * flipped up-down as the reference writes its PNG (:455-456); image holds
 * num_cells_x * num_cells_y bytes.  The reference crops the image to the
 * allocated patches (GridMap::ComputeActualMapSize); the caller crops with
 * the hit/miss counts if it needs that extent. */
int  lgs_map_render_gray(lgs_ctx* ctx, const lgs_map* map, uint8_t* image);
/* MapSaver::DrawMap for the w x h cells starting at cell (x0, y0) -- the
 * region SaveMapCore draws (C/io/map_saver.cpp:413-437): gray bytes as
 * lgs_map_render_gray, rows flipped up-down if flip_rows.  The region must lie
 * inside the map. */
int  lgs_map_render_gray_region(lgs_ctx* ctx, const lgs_map* map, int x0, int y0, int w, int h,
                                int flip_rows, uint8_t* image);
/* Patch::IsAllocated per patch (H/grid_map/grid_map_patch.hpp:40), row-major
 * num_patches_x * num_patches_y bytes: a patch is allocated by the first
 * update of one of its cells (GridMap::GridCellAt, H/grid_map/grid_map.hpp:807-823),
 * moves with Resize (:652-711) and stays allocated across Reset. */
int  lgs_map_download_patches(lgs_ctx* ctx, const lgs_map* map, uint8_t* flags);
/* GridMap::ComputeActualMapSize (H/grid_map/grid_map.hpp:969-1015): the
 * bounding box of the allocated patches.  out[12] = patchIdxMin x, y;
 * patchIdxMax x, y (exclusive, after the reference's +1); gridCellIdxMin x, y;
 * gridCellIdxMax x, y; mapSizeInPatches x, y; mapSizeInGridCells x, y.
 * *num_allocated = allocated patches; with none the reference's bounds are
 * INT_MAX/INT_MIN (undefined sizes) and out is all zero here. */
int  lgs_map_actual_size(lgs_ctx* ctx, const lgs_map* map, int* num_allocated, int* out);
/* Copy cells and per-cell hit/miss update counts (since create/construct) to
 * the host; any pointer may be NULL.  Sizes: num_cells_x * num_cells_y. */
int  lgs_map_download(lgs_ctx* ctx, const lgs_map* map, double* cells, uint32_t* hit_count,
                      uint32_t* miss_count);

/* CostGreedyEndpoint::Cost at one sensor pose */
int  lgs_cost_greedy_endpoint(lgs_ctx* ctx, const lgs_grid* grid,
                              const lgs_cost_ge_params* cost, const lgs_scan* scan,
                              lgs_pose2d sensor_pose, double* out_cost);

/* ---- loop-closure batch (LoopDetectorRealTimeCorrelative::Detect) ----
 * C/mapping/loop_detector_real_time_correlative.cpp:26-125.  A query is one
 * local map (LoopDetectionQuery::mLocalMapInfo / mLocalMapNode) and the
 * contiguous range of candidates (its mPoseGraphNodes) matched against it. */
typedef struct {
    const lgs_grid* map;            /* local grid map */
    const lgs_grid* coarse;         /* its cached coarse map, or NULL = compute (:52-60) */
    lgs_pose2d local_map_node_pose; /* mLocalMapNode.Pose() */
    int local_map_node_index;       /* mLocalMapNode.Index() */
    int first_candidate, num_candidates;
} lgs_loop_query;

typedef struct {
    const lgs_scan* scan;           /* poseGraphNode.ScanData() */
    lgs_pose2d node_pose;           /* poseGraphNode.Pose() (initial pose) */
    int node_index;                 /* poseGraphNode.Index() */
    int pad;
} lgs_loop_candidate;

/* LoopDetectionResult (H/mapping/loop_detector.hpp:60-87) + diagnostics; a
 * fixed 176-byte record (22 x 8 B) so shards can be all-gathered as a flat array. */
typedef struct {
    int found;                      /* 0: the reference appends no result */
    int start_node_index, end_node_index;
    int pad;
    lgs_pose2d relative_pose;       /* InverseCompound(localMapNode.Pose(), estimated) */
    lgs_pose2d start_node_pose;
    lgs_pose2d estimated_pose;      /* matcher's estimate (world frame) */
    double covariance[9];
    double score;                   /* correlative score of the best pose */
    double normalized_cost;
} lgs_loop_result;

/* One result per candidate, in candidate order. */
int  lgs_loop_detect_rtcsm(lgs_ctx* ctx, const lgs_rtcsm_params* params, const lgs_cost_ge_params* cost,
                           double score_threshold, const lgs_loop_query* queries, int num_queries,
                           const lgs_loop_candidate* candidates, int num_candidates,
                           lgs_loop_result* results);

/* Multi-GPU Detect for a caller that owns several GPUs in one
 * process (the reference's backend calls Detect once,
 * C/mapping/lidar_graph_slam_backend.cpp:39-40): the same contract and the
 * same results, byte for byte, as lgs_loop_detect_rtcsm on ctxs[0].  The
 * candidates are split into num_ctx contiguous shards, shard k =
 * [k*n/N, (k+1)*n/N) runs on ctxs[k] on its own host thread; maps, coarse maps
 * and scans owned by another context are copied to ctxs[k] first (peer copy
 * over xGMI; scans re-uploaded from their host copy).  Errors of any shard are
 * reported on ctxs[0]. */
int  lgs_loop_detect_rtcsm_multi(lgs_ctx* const* ctxs, int num_ctx, const lgs_rtcsm_params* params,
                                 const lgs_cost_ge_params* cost, double score_threshold,
                                 const lgs_loop_query* queries, int num_queries,
                                 const lgs_loop_candidate* candidates, int num_candidates,
                                 lgs_loop_result* results);

/* ---- the loop batch over several processes (one per GPU) ----
 * Candidates are independent (C/mapping/loop_detector_real_time_correlative.cpp:38, :66):
 * rank r of `world` matches the contiguous block [lo_r, hi_r) of the n
 * candidates (lgs_loop_shard_bounds: block sizes differ by at most one, the
 * larger blocks first) with lgs_loop_detect_rtcsm, then
 * lgs_loop_records_allgather gathers every rank's records into `all` (host,
 * n records, candidate order -- the order the reference's
 * LoopDetectionResultVector keeps) with ONE ncclAllGather of fixed-size rows
 * on ctx's stream (RCCL over xGMI), and synchronises the stream.  `comm` is an
 * ncclComm_t of `world` ranks whose rank `rank` lives on ctx's device (made
 * by the caller, or with lgs_rccl_comm_init).  RCCL is resolved at run time
 * (librccl.so.1, an already loaded copy first). */
int  lgs_loop_shard_bounds(int n, int world, int rank, int* lo, int* hi);
int  lgs_loop_records_allgather(lgs_ctx* ctx, void* comm, int rank, int world, int n,
                                const lgs_loop_result* local, lgs_loop_result* all);
/* RCCL communicator helpers: a 128-byte ncclUniqueId made on one rank and
 * sent to the others by the caller, then one lgs_rccl_comm_init per rank. */
int  lgs_rccl_unique_id(unsigned char* id128);
int  lgs_rccl_comm_init(lgs_ctx* ctx, const unsigned char* id128, int world, int rank, void** comm);
int  lgs_rccl_comm_destroy(void* comm);

/* ---- branch-and-bound matcher ----
 * ScanMatcherBranchBound (C/mapping/scan_matcher_branch_bound.cpp:8-200,
 * H/mapping/scan_matcher_branch_bound.hpp) with ScorePixelAccurate
 * (C/mapping/score_function_pixel_accurate.cpp:19-77) and the grid-map
 * pyramid PrecomputeGridMaps (C/mapping/grid_map_builder.cpp:471-495).
 * The device scores every node the reference's depth-first search can visit
 * (level by level, a superset bounded by the threshold argument of
 * DESIGN.md §4.6); the host then replays the reference's LIFO search over
 * those scores, so the result is the reference's own (best node, score,
 * nodes visited).  Field order follows the constructor (nodeHeightMax,
 * rangeX, rangeY, rangeTheta, scanRangeMax) then ScorePixelAccurate
 * (usableRangeMin, usableRangeMax). */
typedef struct {
    int    node_height_max;
    double range_x, range_y, range_theta;
    double scan_range_max;
    double score_usable_range_min, score_usable_range_max;
} lgs_bb_params;

/* PrecomputeGridMaps: pyramid[h] = window-max map with window 2^h,
 * h = 0..node_height_max (node_height_max + 1 grids of the input's geometry,
 * created by the caller). */
int  lgs_grid_precompute_pyramid(lgs_ctx* ctx, const lgs_grid* in, int node_height_max,
                                 lgs_grid* const* pyramid);
/* OptimizePose(gridMap, precompMaps, scan, pose, thr) (:47-154) for n scans
 * against one pyramid (loop-closure candidates); summaries as the RTCSM
 * ones, with best_win = the best node's (x, y, theta), coarse_blocks = nodes
 * scored on the device, fine_blocks = nodes the reference's search visits. */
int  lgs_bb_optimize_pose_batch(lgs_ctx* ctx, const lgs_grid* grid, const lgs_grid* const* pyramid,
                                const lgs_bb_params* params, const lgs_cost_ge_params* cost,
                                const lgs_scan* const* scans, const lgs_pose2d* initial_poses, int n,
                                double normalized_score_threshold, lgs_rtcsm_summary* out);
/* OptimizePose(query) (:29-44): pyramid of the query's map, threshold DBL_MIN */
int  lgs_bb_optimize_pose_query(lgs_ctx* ctx, const lgs_grid* grid, const lgs_bb_params* params,
                                const lgs_cost_ge_params* cost, const lgs_scan* scan,
                                lgs_pose2d initial_pose, lgs_rtcsm_summary* out);
/* LoopDetectorBranchBound::Detect + FindCorrespondingPose
 * (C/mapping/loop_detector_branch_bound.cpp:26-117): per query the pyramid of
 * its local map (computed here; lgs_loop_query.coarse is ignored), then every
 * candidate matched with the score threshold.  One result per candidate. */
int  lgs_loop_detect_bb(lgs_ctx* ctx, const lgs_bb_params* params, const lgs_cost_ge_params* cost,
                        double score_threshold, const lgs_loop_query* queries, int num_queries,
                        const lgs_loop_candidate* candidates, int num_candidates,
                        lgs_loop_result* results);

/* ---- exhaustive grid-search matcher ----
 * ScanMatcherGridSearch (C/mapping/scan_matcher_grid_search.cpp:9-114,
 * H/mapping/scan_matcher_grid_search.hpp) with ScorePixelAccurate
 * (C/mapping/score_function_pixel_accurate.cpp:19-77).  Every pose
 * (sp.x + dx, sp.y + dy, sp.theta + dt), sp = Compound(initialPose,
 * relativeSensorPose), of the window is scored on the device; the offsets are
 * the values of the reference's `for (double d = -range / 2; d <= range / 2;
 * d += step)` loops (lgs_gs_steps), dy outermost, dt innermost; the result is
 * the first pose in that order of the maximum score, if that maximum is > the
 * threshold.  Field order follows the constructor (rangeX,
 * rangeY, rangeTheta, stepX, stepY, stepTheta) then ScorePixelAccurate
 * (usableRangeMin, usableRangeMax).
 * Caps (LGS_ERR_INVALID_ARG beyond them): 4096 values per window axis, 2^24
 * poses per window, 2 GiB of index tables per match (4 B x angles x valid
 * beams x (x values + y values), plus 16 B x angles x valid beams), maps of
 * fewer than 2^30 cells.  A call of many matches runs in chunks whose tables
 * fit 1 GiB together.  Steps must be finite and > 0, ranges finite and >= 0
 * (the reference would loop forever or not at all). */
typedef struct {
    double range_x, range_y, range_theta;
    double step_x, step_y, step_theta;
    double score_usable_range_min, score_usable_range_max;
} lgs_gs_params;

/* The window values of one axis: the literal loop above, on the host (no
 * context, no device).  Returns their count and writes the first
 * min(count, cap) of them to out (out may be NULL when cap is 0); on bad
 * arguments (step <= 0 or not finite, range negative or not finite, more than
 * 4096 values) returns -LGS_ERR_INVALID_ARG: negative, so that a status can
 * never be taken for a count.  The matcher calls the same loop. */
int  lgs_gs_steps(double range, double step, double* out, int cap);
/* OptimizePose(gridMap, scanData, initialPose, thr) (:44-114) for n scans
 * against one map.  Summaries as the RTCSM ones with win = (nx, ny, nt) the
 * window's value counts, best_win = the best pose's (ix, iy, it) or
 * (-1, -1, -1) when nothing is found (cost, covariance and estimate are then
 * evaluated at sp, as the reference does), steps = the three steps, score_max
 * and score_threshold raw sums, coarse_blocks = poses scored, fine_blocks = 0. */
int  lgs_gs_optimize_pose_batch(lgs_ctx* ctx, const lgs_grid* grid, const lgs_gs_params* params,
                                const lgs_cost_ge_params* cost, const lgs_scan* const* scans,
                                const lgs_pose2d* initial_poses, int n, double normalized_score_threshold,
                                lgs_rtcsm_summary* out);
/* OptimizePose(query) (:31-41): threshold DBL_MIN */
int  lgs_gs_optimize_pose_query(lgs_ctx* ctx, const lgs_grid* grid, const lgs_gs_params* params,
                                const lgs_cost_ge_params* cost, const lgs_scan* scan, lgs_pose2d initial_pose,
                                lgs_rtcsm_summary* out);
/* Diagnostics: every pose's score in (iy, ix, it) order (nx * ny * nt doubles;
 * cap = the room in `scores`, LGS_ERR_INVALID_ARG when smaller). */
int  lgs_gs_dense_scores(lgs_ctx* ctx, const lgs_grid* grid, const lgs_gs_params* params, const lgs_scan* scan,
                         lgs_pose2d initial_pose, double* scores, long long cap);
/* LoopDetectorGridSearch::Detect + FindCorrespondingPose
 * (C/mapping/loop_detector_grid_search.cpp:26-106): every candidate matched
 * against its query's local map with the score threshold (lgs_loop_query.coarse
 * is ignored); lgs_loop_result.score is the best raw score.  One result per
 * candidate, as lgs_loop_detect_bb. */
int  lgs_loop_detect_gs(lgs_ctx* ctx, const lgs_gs_params* params, const lgs_cost_ge_params* cost,
                        double score_threshold, const lgs_loop_query* queries, int num_queries,
                        const lgs_loop_candidate* candidates, int num_candidates,
                        lgs_loop_result* results);

/* ---- hill-climbing matcher (ScanMatcherHillClimbing + CostGreedyEndpoint) ----
 * Replaces ScanMatcherHillClimbing::OptimizePose
 * (C/mapping/scan_matcher_hill_climbing.cpp:26-109), the matcher the launcher
 * falls back to (C/slam_launcher.cpp:769-772).  The walk runs on the device,
 * one workgroup per match, and every value of its ScanMatchingSummary equals
 * the reference's bit for bit: the cost's exp() term takes one of at most
 * (2K+1)^2 + 1 values (lgs_hc_term_table), which the host evaluates with libm
 * and the device selects from.  Field order follows the
 * constructor (linearStep, angularStep, maxIterations, maxNumOfRefinements).
 * Caps (LGS_ERR_INVALID_ARG beyond them): steps finite and > 0, initial poses
 * finite, max_iterations <= 65536 (values <= 1 run one pass, as the
 * reference's do/while does), kernel_size in [0, 16], standard deviation and
 * map resolution finite and > 0.  An angle outside the restated sincos domain
 * (|theta + angle| >= 105414350) fails with LGS_ERR_INTERNAL. */
typedef struct {
    double linear_step, angular_step;
    int max_iterations, max_num_of_refinements;
} lgs_hc_params;

typedef struct {
    /* ScanMatchingSummary (H/mapping/scan_matcher.hpp:147-174) */
    int pose_found;                 /* always 1 (:106-108) */
    double normalized_cost;         /* minCost / NumOfScans() (:96) */
    lgs_pose2d initial_pose, estimated_pose;   /* MoveBackward(bestPose, relPose) (:98-99) */
    double covariance[9];           /* CostGreedyEndpoint::ComputeCovariance at bestPose, row-major */
    /* diagnostics */
    lgs_pose2d best_sensor_pose;
    double min_cost;
    double final_linear_step, final_angular_step;
    int num_iterations;             /* the reference's variables at exit (:48-50) */
    int num_refinements;
    int passes;                     /* bodies of the do/while run */
    int cost_evals;                 /* 1 + 6 per pass + 6 for the gradient */
} lgs_hc_summary;

/* The values the cost's exp() term can take (no context, no device): entry
 * q = (ky + K) * (2K+1) + (kx + K) holds GridMap::SquaredDistance of the kernel
 * offset (H/grid_map/grid_map.hpp:894-902: dX = kx * res, dY = ky * res,
 * sq = dX * dX + dY * dY), entry (2K+1)^2 the start value with dX = dY =
 * (K+1) * res (C/mapping/cost_function_greedy_endpoint.cpp:66-67), and
 * term = exp(-0.5 * sq / variance) with libm's exp (:101), variance =
 * standard_deviation^2.  Returns the entry count and writes the first
 * min(count, cap) entries (sq and term may be NULL when cap is 0); on bad
 * arguments returns -LGS_ERR_INVALID_ARG. */
int  lgs_hc_term_table(const lgs_cost_ge_params* cost, double res, double* sq, double* term, int cap);
/* OptimizePose(query) (:26-109) */
int  lgs_hc_optimize_pose_query(lgs_ctx* ctx, const lgs_grid* grid, const lgs_hc_params* params,
                                const lgs_cost_ge_params* cost, const lgs_scan* scan, lgs_pose2d initial_pose,
                                lgs_hc_summary* out);
/* n scans and poses, one grid per item; pointers may repeat.  One launch per
 * chunk (4096 matches of one map resolution).  Equal to n lone calls. */
int  lgs_hc_optimize_pose_batch(lgs_ctx* ctx, const lgs_grid* const* grids, const lgs_hc_params* params,
                                const lgs_cost_ge_params* cost, const lgs_scan* const* scans,
                                const lgs_pose2d* initial_poses, int n, lgs_hc_summary* out);
/* Diagnostics: the walk's per-pass (accepted move index 0..5 in the order of
 * :30-32, or -1; minCost after the pass) of one match.  Returns the pass count
 * and writes the first min(count, cap) passes; a failure returns the negated
 * status. */
int  lgs_hc_trace(lgs_ctx* ctx, const lgs_grid* grid, const lgs_hc_params* params, const lgs_cost_ge_params* cost,
                  const lgs_scan* scan, lgs_pose2d initial_pose, int* moves, double* costs, int cap);
/* CostGreedyEndpoint::Cost (:32-111) at n sensor poses of one scan, equal to
 * the reference's bit for bit: the matcher's cost code on its own
 * (lgs_cost_greedy_endpoint keeps its 1e-5 contract). */
int  lgs_cost_ge_exact(lgs_ctx* ctx, const lgs_grid* grid, const lgs_cost_ge_params* cost, const lgs_scan* scan,
                       const lgs_pose2d* poses, int n, double* out);

/* ---- K4: Gauss-Newton refine (ScanMatcherLinearSolver + CostSquareError) ----
 * Replaces ScanMatcherLinearSolver::OptimizePose (C/mapping/scan_matcher_linear_solver.cpp:38-85,
 * H/mapping/scan_matcher_linear_solver.hpp:15-56) with its CostSquareError
 * (C/mapping/cost_function_square_error.cpp).  Field order follows the
 * constructor (numOfIterationsMax, convergenceThreshold, usableRangeMin/Max,
 * translation/rotation regularizer) then CostSquareError(usableRangeMin/Max). */
typedef struct {
    int    num_iterations_max;
    double convergence_threshold;
    double usable_range_min, usable_range_max;
    double translation_regularizer, rotation_regularizer;
    double cost_usable_range_min, cost_usable_range_max;
} lgs_linsolve_params;

/* ScanMatchingSummary (H/mapping/scan_matcher.hpp:26-77) plus diagnostics */
typedef struct {
    int pose_found;               /* always 1, as the reference */
    int iterations;               /* OptimizeStep calls made */
    double normalized_cost;       /* cost / NumOfScans() */
    lgs_pose2d initial_pose;
    lgs_pose2d estimated_pose;    /* MoveBackward(bestSensorPose, relPose) */
    double covariance[9];         /* CostSquareError::ComputeCovariance, row-major */
    lgs_pose2d sensor_pose;       /* Compound(initialPose, relPose) */
    lgs_pose2d best_sensor_pose;
    double cost;                  /* un-normalized final cost */
} lgs_linsolve_summary;

/* One refine; trajectory (may be NULL; room for 4 * max(1, num_iterations_max)
 * doubles) receives, after every OptimizeStep, the sensor pose (x, y, theta)
 * and the cost the convergence test sees at it. */
int  lgs_linsolve_optimize_pose(lgs_ctx* ctx, const lgs_grid* grid, const lgs_linsolve_params* params,
                                const lgs_scan* scan, lgs_pose2d initial_pose,
                                lgs_linsolve_summary* out, double* trajectory);
/* n independent refines against one grid (one workgroup each), one sync */
int  lgs_linsolve_optimize_pose_batch(lgs_ctx* ctx, const lgs_grid* grid,
                                      const lgs_linsolve_params* params,
                                      const lgs_scan* const* scans, const lgs_pose2d* initial_poses,
                                      int n, lgs_linsolve_summary* out);
/* CostSquareError::Cost (C/mapping/cost_function_square_error.cpp:21-58) and,
 * if out_covariance is not NULL, ComputeCovariance (:112-135) at one sensor pose */
int  lgs_cost_square_error(lgs_ctx* ctx, const lgs_grid* grid, double usable_range_min,
                           double usable_range_max, const lgs_scan* scan, lgs_pose2d sensor_pose,
                           double* out_cost, double* out_covariance);

/* ---- CostSquareError for every scan matcher ----
 * The reference builds each matcher's cost through CreateCostFunction
 * (C/slam_launcher.cpp:96-107): "GreedyEndpoint" or "SquareError".  The entry
 * points above take the greedy-endpoint cost; these give a matcher constructed
 * with CostSquareError.  Every value equals the reference's
 * bit for bit (the arithmetic of lgs_cost_square_error).  A square-error term
 * needs no per-resolution table, so one call, and one launch, may mix maps of
 * different size and resolution.
 * Caps (LGS_ERR_INVALID_ARG beyond them): usable ranges, poses and map
 * resolutions finite (resolution > 0), maps of fewer than 2^30 cells, scans
 * of at least one beam.  An angle outside the restated sincos domain
 * (|theta + angle| >= 105414350) fails with LGS_ERR_INTERNAL. */

/* CostSquareError(usableRangeMin, usableRangeMax), cost_function_square_error.cpp:10-17 */
typedef struct { double usable_range_min, usable_range_max; } lgs_cost_sq_params;

/* Cost (:21-58) and, if out_covariance != NULL, ComputeCovariance (:112-135) of item j at
 * sensor_poses[j] on grids[j] with scans[j]; pointers may repeat, grids may differ in size
 * and resolution.  One launch per chunk (4096 items), one synchronisation per call.  Equal
 * to n calls of lgs_cost_square_error byte for byte. */
int  lgs_cost_square_error_batch(lgs_ctx* ctx, const lgs_grid* const* grids, const lgs_cost_sq_params* cost,
                                 const lgs_scan* const* scans, const lgs_pose2d* sensor_poses, int n,
                                 double* out_cost /* n */, double* out_covariance /* 9 n or NULL */);

/* What a matcher constructed with CostSquareError returns: summaries[j].normalized_cost =
 * Cost(best_sensor_pose) / NumOfScans() and .covariance = ComputeCovariance(best_sensor_pose);
 * every other field is left as it is.  For the summaries of the rtcsm, bb and gs entry points,
 * which evaluate the cost after the search, at best_sensor_pose, whether or not a pose was found
 * (scan_matcher_real_time_correlative.cpp:128-138, scan_matcher_grid_search.cpp:97-107). */
int  lgs_summaries_apply_cost_sq(lgs_ctx* ctx, const lgs_grid* const* grids, const lgs_cost_sq_params* cost,
                                 const lgs_scan* const* scans, lgs_rtcsm_summary* summaries, int n);

/* ---- the greedy-endpoint cost bit for bit, for the search matchers ----
 * Item j: CostGreedyEndpoint::Cost (cost_function_greedy_endpoint.cpp:32-111) at sensor_poses[j]
 * on grids[j] with scans[j] and, if out_covariance != NULL, ComputeCovariance (:114-171) there
 * (the six central-difference costs in the same launch, the covariance formed on the host in the
 * reference's expression order).  Pointers may repeat; grids may differ in size and resolution
 * (one term table per distinct resolution, cached on the context).  One launch per chunk (4096
 * items), one synchronisation per call.  Equal to n calls of lgs_cost_ge_exact at the seven
 * poses byte for byte.  Caps and status codes of lgs_cost_ge_exact; a failing call writes
 * nothing. */
int  lgs_cost_ge_exact_batch(lgs_ctx* ctx, const lgs_grid* const* grids, const lgs_cost_ge_params* cost,
                             const lgs_scan* const* scans, const lgs_pose2d* sensor_poses, int n,
                             double* out_cost /* n */, double* out_covariance /* 9 n or NULL */);
/* summaries[j].normalized_cost = Cost(best_sensor_pose) / NumOfScans() and .covariance =
 * ComputeCovariance(best_sensor_pose), both the reference's bytes; every other field is left as
 * it is.  What LGS_COST_GREEDY_ENDPOINT_EXACT gives through the `_cost` entry points below. */
int  lgs_summaries_apply_cost_ge_exact(lgs_ctx* ctx, const lgs_grid* const* grids, const lgs_cost_ge_params* cost,
                                       const lgs_scan* const* scans, lgs_rtcsm_summary* summaries, int n);

/* ScanMatcherHillClimbing with CostSquareError: the contracts, caps and status
 * codes of the lgs_hc_* trio (kernel size and standard deviation apart), plus
 * finite usable ranges.  lgs_hc_summary is reused with two differences:
 * covariance is CostSquareError::ComputeCovariance at bestPose (the analytic
 * gradient g, g g^T, + 0.01 on the diagonal), and cost_evals counts Cost calls
 * only, 1 + 6 per pass: the square-error covariance calls Cost not once.
 * lgs_hc_sq_trace returns the pass count, or the negated status. */
int  lgs_hc_sq_optimize_pose_query(lgs_ctx* ctx, const lgs_grid* grid, const lgs_hc_params* params,
                                   const lgs_cost_sq_params* cost, const lgs_scan* scan, lgs_pose2d initial_pose,
                                   lgs_hc_summary* out);
int  lgs_hc_sq_optimize_pose_batch(lgs_ctx* ctx, const lgs_grid* const* grids, const lgs_hc_params* params,
                                   const lgs_cost_sq_params* cost, const lgs_scan* const* scans,
                                   const lgs_pose2d* initial_poses, int n, lgs_hc_summary* out);
int  lgs_hc_sq_trace(lgs_ctx* ctx, const lgs_grid* grid, const lgs_hc_params* params, const lgs_cost_sq_params* cost,
                     const lgs_scan* scan, lgs_pose2d initial_pose, int* moves, double* costs, int cap);

/* ---- search matchers and loop detectors with either cost function ----
 * The `_cost` entry points take an lgs_cost_spec where their namesakes take
 * an lgs_cost_ge_params; every other argument is the namesake's.
 *   kind == LGS_COST_GREEDY_ENDPOINT  the namesake's path and the namesake's
 *     bytes (spec->ge is what it would have been given).
 *   kind == LGS_COST_SQUARE_ERROR     normalized_cost = CostSquareError::Cost(
 *     best_sensor_pose) / NumOfScans() and covariance = ComputeCovariance(
 *     best_sensor_pose) with spec->sq, whether or not a pose was found (as
 *     lgs_summaries_apply_cost_sq gives, bit for bit); every other summary
 *     field is the namesake's, except the diagnostic counters guard_hits and
 *     fixups, which no longer count the greedy-endpoint stage's cells.  A loop
 *     record differs from the namesake's in normalized_cost and covariance
 *     only.  The correlative matcher evaluates the cost as a stage of its own
 *     pipeline, at the best pose the search left on the device (k_cost_sq: no
 *     greedy-endpoint stage, no second synchronisation); the branch-and-bound
 *     and grid-search matchers run one k_sq_cost_batch launch per call.
 *   kind == LGS_COST_GREEDY_ENDPOINT_EXACT  the greedy-endpoint cost of
 *     spec->ge bit for bit: normalized_cost = CostGreedyEndpoint::Cost(
 *     best_sensor_pose) / NumOfScans() and covariance = ComputeCovariance(
 *     best_sensor_pose) with the reference's bytes, whether or not a pose was
 *     found (as lgs_summaries_apply_cost_ge_exact gives); kind 0 holds both to
 *     1e-5 only.  Every other summary field and every other byte of a loop
 *     record is kind 0's, except guard_hits and fixups as for kind 1.  The
 *     correlative matcher runs the stage k_cost_gx in k_cost's place (the
 *     hill-climbing cost's code: restated sincos, table terms, beam-order
 *     sums; no guard records, no host fix-up); the branch-and-bound and
 *     grid-search matchers run one k_ge_cost_batch launch per chunk.  The
 *     hill-climbing cost's caps apply: kernel_size in [0, 16], standard
 *     deviation and map resolution finite and > 0, maps of fewer than 2^30
 *     cells, scans of at least one beam.
 * An unknown kind, non-finite usable ranges or a kind-2 cost beyond its caps:
 * LGS_ERR_INVALID_ARG before any device work.  The caps and status codes of
 * lgs_cost_square_error_batch apply to kind 1 (a map of 2^30 cells or more:
 * LGS_ERR_INVALID_ARG); an angle outside the restated sincos domain fails a
 * kind-1 or kind-2 call with LGS_ERR_INTERNAL; with kinds 1 and 2 a failing
 * call writes nothing to `out` / `results`. */
#define LGS_COST_GREEDY_ENDPOINT 0
#define LGS_COST_SQUARE_ERROR    1
#define LGS_COST_GREEDY_ENDPOINT_EXACT 2   /* reads spec->ge */
typedef struct {
    int kind;                 /* LGS_COST_* */
    lgs_cost_ge_params ge;    /* read when kind == 0 or 2 */
    lgs_cost_sq_params sq;    /* read when kind == 1 */
} lgs_cost_spec;
size_t lgs_cost_spec_size(void);   /* sizeof(lgs_cost_spec), for bindings */

int  lgs_rtcsm_optimize_pose_cost(lgs_ctx* ctx, const lgs_grid* grid, const lgs_grid* coarse,
                                  const lgs_rtcsm_params* params, const lgs_cost_spec* cost,
                                  const lgs_scan* scan, lgs_pose2d initial_pose,
                                  double normalized_score_threshold, lgs_rtcsm_summary* out);
int  lgs_rtcsm_optimize_pose_query_cost(lgs_ctx* ctx, const lgs_grid* grid, const lgs_rtcsm_params* params,
                                        const lgs_cost_spec* cost, const lgs_scan* scan,
                                        lgs_pose2d initial_pose, lgs_rtcsm_summary* out);
int  lgs_rtcsm_optimize_pose_query_batch_cost(lgs_ctx* ctx, const lgs_grid* const* grids,
                                              const lgs_rtcsm_params* params, const lgs_cost_spec* cost,
                                              const lgs_scan* const* scans, const lgs_pose2d* initial_poses,
                                              int n, lgs_rtcsm_summary* out);
int  lgs_rtcsm_optimize_pose_batch_cost(lgs_ctx* ctx, const lgs_grid* grid, const lgs_grid* coarse,
                                        const lgs_rtcsm_params* params, const lgs_cost_spec* cost,
                                        const lgs_scan* const* scans, const lgs_pose2d* initial_poses,
                                        int n, double normalized_score_threshold, lgs_rtcsm_summary* out);
int  lgs_bb_optimize_pose_batch_cost(lgs_ctx* ctx, const lgs_grid* grid, const lgs_grid* const* pyramid,
                                     const lgs_bb_params* params, const lgs_cost_spec* cost,
                                     const lgs_scan* const* scans, const lgs_pose2d* initial_poses, int n,
                                     double normalized_score_threshold, lgs_rtcsm_summary* out);
int  lgs_bb_optimize_pose_query_cost(lgs_ctx* ctx, const lgs_grid* grid, const lgs_bb_params* params,
                                     const lgs_cost_spec* cost, const lgs_scan* scan,
                                     lgs_pose2d initial_pose, lgs_rtcsm_summary* out);
int  lgs_gs_optimize_pose_batch_cost(lgs_ctx* ctx, const lgs_grid* grid, const lgs_gs_params* params,
                                     const lgs_cost_spec* cost, const lgs_scan* const* scans,
                                     const lgs_pose2d* initial_poses, int n, double normalized_score_threshold,
                                     lgs_rtcsm_summary* out);
int  lgs_gs_optimize_pose_query_cost(lgs_ctx* ctx, const lgs_grid* grid, const lgs_gs_params* params,
                                     const lgs_cost_spec* cost, const lgs_scan* scan, lgs_pose2d initial_pose,
                                     lgs_rtcsm_summary* out);
int  lgs_loop_detect_rtcsm_cost(lgs_ctx* ctx, const lgs_rtcsm_params* params, const lgs_cost_spec* cost,
                                double score_threshold, const lgs_loop_query* queries, int num_queries,
                                const lgs_loop_candidate* candidates, int num_candidates,
                                lgs_loop_result* results);
int  lgs_loop_detect_rtcsm_multi_cost(lgs_ctx* const* ctxs, int num_ctx, const lgs_rtcsm_params* params,
                                      const lgs_cost_spec* cost, double score_threshold,
                                      const lgs_loop_query* queries, int num_queries,
                                      const lgs_loop_candidate* candidates, int num_candidates,
                                      lgs_loop_result* results);
int  lgs_loop_detect_bb_cost(lgs_ctx* ctx, const lgs_bb_params* params, const lgs_cost_spec* cost,
                             double score_threshold, const lgs_loop_query* queries, int num_queries,
                             const lgs_loop_candidate* candidates, int num_candidates, lgs_loop_result* results);
int  lgs_loop_detect_gs_cost(lgs_ctx* ctx, const lgs_gs_params* params, const lgs_cost_spec* cost,
                             double score_threshold, const lgs_loop_query* queries, int num_queries,
                             const lgs_loop_candidate* candidates, int num_candidates, lgs_loop_result* results);

/* ---- the pose graph's conjugate-gradient step (k_pgcg.hip) ----
 * H x = rhs for the symmetric matrix of a pose-graph Levenberg-Marquardt step
 * (PoseGraphOptimizerLM::OptimizeStep, C/mapping/pose_graph_optimizer_lm.cpp:
 * 175-207 with SolverType::ConjugateGradient), 3x3 blocks over num_nodes nodes:
 * diag[v] is the block (v, v), off[p] the block (a, b) of pairs[p] = (a, b),
 * a < b, every pair listed once; the block (b, a) is its transpose.  The solver
 * is Eigen's ConjugateGradient recurrence with its Jacobi preconditioner (1 / d,
 * 1 where d == 0) from a zero initial guess: it stops after the pass that
 * brings |r|^2 below max(tolerance^2 |rhs|^2, DBL_MIN), or after
 * max_iterations passes.  tolerance 0 selects DBL_EPSILON and max_iterations 0
 * selects 2 * 3 num_nodes, Eigen's defaults.  *iterations receives the passes
 * run (0 for a zero right-hand side, whose solution is x = 0) and
 * *residual_norm2 the last |r|^2.  Systems below LGS_OPT_PGCG_GRID_NODES
 * nodes are solved by one persistent workgroup in one launch and one stream
 * synchronisation; larger ones over many workgroups that meet at kernel
 * boundaries only, two launches per pass, enqueued in chunks of 32 passes
 * with one event wait per chunk.  Either way the summation order is fixed by
 * the node count, so a system gives the same bytes in every run and on every
 * context (the two variants differ from each other, and from a serial sum, in
 * the last bits); a system that holds a NaN runs to the cap and returns LGS_OK
 * with NaNs in x.  The block pattern is built and uploaded when the pair list
 * differs from the previous call's on this context, the values and the
 * right-hand side on every call.
 * LGS_ERR_INVALID_ARG, before any device work: a NULL argument (pairs and off
 * may be NULL when num_pairs is 0), num_nodes < 1 or > 2^27, num_pairs < 0 or
 * > 2^27, a pair with an index outside [0, num_nodes), with a >= b or listed
 * twice, a tolerance that is negative or not finite, max_iterations < 0. */
int  lgs_pg_cg_solve(lgs_ctx* ctx, int num_nodes, const double* diag /*[n][9] row-major*/,
                     int num_pairs, const int* pairs /*[p][2], a < b, unique*/, const double* off /*[p][9], block (a,b)*/,
                     const double* rhs /*[3n]*/, double tolerance /*0: DBL_EPSILON*/, int max_iterations /*0: 2*3n*/,
                     double* x /*[3n]*/, int* iterations, double* residual_norm2);
/* Counters of lgs_pg_cg_solve on this context since its creation: solves, CG
 * passes over all of them, block patterns built, solves that ran over many
 * workgroups (each may be NULL). */
int  lgs_pg_cg_stats(const lgs_ctx* ctx, long long* solves, long long* iterations, long long* patterns,
                     long long* grid_solves);

/* ---- the pose graph's Levenberg-Marquardt loop, resident on the device
 * (k_pglm.hip) ----
 * PoseGraphOptimizerLM::Optimize (C/mapping/pose_graph_optimizer_lm.cpp:13-338)
 * with SolverType::ConjugateGradient and every step on the device: poses and
 * edges go up once, each step linearises every edge (k_pg_linearise writes H
 * straight into the layout the solve walks, and rhs = -b), solves as
 * lgs_pg_cg_solve does (Eigen's defaults; counted by lgs_pg_cg_stats), adds
 * the increment to the poses and evaluates Loss(e^T Lambda e) per edge; the
 * host adds those terms in edge order and applies Optimize's rule for the
 * damping factor and for stopping.  The poses come down once at the end.
 * Every entry of H and b is the sequential sum in edge order that the host's
 * OptimizeStep forms, in its arithmetic (glibc's sincos restated, IEEE
 * division and square root, no contraction), so for the losses whose Weight is
 * IEEE-only (all but Welsch, whose exp is the device's) the system, and with
 * it every pose, equals lgs_pose_graph_optimize_lm_device's byte for byte; the
 * total error does for the losses whose Loss is IEEE-only too (Huber,
 * GemanMcClure, DCS, Squared).
 * LGS_ERR_INVALID_ARG, before any device work: a NULL argument (edges may be
 * NULL when m is 0), n < 1 or > 2^27, m < 0 or > 2^27, an edge index outside
 * [0, n), a loss kind outside 0..6, a damping factor, tolerance or scale that
 * is not finite.  LGS_ERR_INTERNAL when a finite start-node angle leaves the
 * restated sincos's domain (|theta| >= 105414350).  The caller's poses are
 * written only by a call that returns LGS_OK.  A NaN pose is no error: the
 * solves run to their cap and NaNs come back. */
/* PoseGraph::Edge: the layout of lgs_pose_graph_edge (include/lgs_io.h) */
typedef struct {
    int start_node_index, end_node_index;
    lgs_pose2d relative_pose;
    double information[9];          /* row-major 3x3 */
} lgs_pg_edge;
typedef struct {
    int num_iterations_max;         /* at least one step runs whatever this is, as in the reference */
    double error_tolerance;
    int loss_kind;                  /* 0 Huber, 1 Cauchy, 2 Fair, 3 GemanMcClure, 4 Welsch, 5 DCS, 6 Squared (LGS_LOSS_*) */
    double loss_scale;
} lgs_pg_lm_params;
/* *lambda: in, the damping factor; out, what Optimize leaves for the next call.
 * *iterations LM steps, *total_error after the last, *cg_passes over all solves. */
int  lgs_pg_lm_optimize(lgs_ctx* ctx, const lgs_pg_lm_params* params, double* lambda /*in/out*/, lgs_pose2d* poses,
                        int n, const lgs_pg_edge* edges, int m, int* iterations, double* total_error,
                        long long* cg_passes);
/* Diagnostics: the device's H and right-hand side of one step at the given
 * poses.  *num_pairs pairs (a, b), a < b, in the order the edges first name
 * them (at most m: size pairs and off for m); off[p] is the block (a, b). */
int  lgs_pg_lm_linearize(lgs_ctx* ctx, int loss_kind, double loss_scale, double lambda, const lgs_pose2d* poses, int n,
                         const lgs_pg_edge* edges, int m, double* diag /*[n][9]*/, int* num_pairs,
                         int* pairs /*[<= m][2]*/, double* off /*[<= m][9]*/, double* rhs /*[3n]*/);
/* Counters of lgs_pg_lm_optimize on this context since its creation: calls
 * that ran, LM steps, uploads and downloads of the poses, incidence-list
 * builds (each may be NULL). */
int  lgs_pg_lm_stats(const lgs_ctx* ctx, long long* optimizes, long long* steps, long long* pose_uploads,
                     long long* pose_downloads, long long* incidence_builds);

/* ---- point-to-line ICP: one scan matched against another (k_icp.hip) ----
 * The reference has no scan-to-scan matcher, so the algorithm is the project's
 * own and DESIGN.md 4.5b states it statement for statement; a test-side
 * restatement (tests/icp_oracle.py) and the device agree byte for byte.  In
 * short: every usable beam of the reference scan gives a point q_j at the
 * reference sensor pose and, with its nearer usable neighbour j-1 / j+1 no
 * farther than max_segment_length, a unit normal; every usable beam of the
 * current scan is paired with its nearest q_j (brute force, ties to the lowest
 * j) if that lies within max_correspondence_dist and has a normal; the
 * point-to-line residuals give the Gauss-Newton normal equations, solved with
 * the linear solver's column-pivoting QR, in OptimizePose's loop shape.  All
 * arithmetic is fp64 without contraction, sin/cos are glibc's sincos, and every
 * sum is a fixed tree of the beam count alone, so a refine gives the same bytes
 * in every run, on every context, alone or in a batch.
 * A beam is usable iff !(r >= hi || r <= lo), lo = max(usable_range_min, scan
 * min_range), hi = min(usable_range_max, scan max_range).
 * LGS_ERR_INVALID_ARG, before any device work: a NULL argument (trajectory
 * apart), n < 0, a parameter or pose that is not finite,
 * max_correspondence_dist <= 0 or max_segment_length <= 0, a negative
 * regularizer, an empty scan, more than 4096 usable reference beams (the table
 * lives in LDS).  An angle outside the restated sincos domain
 * (|theta + angle| >= 105414350) fails with LGS_ERR_INTERNAL.  A failing call
 * writes nothing to its outputs. */
typedef struct {
    int    num_iterations_max;        /* at least one step runs whatever this is */
    double convergence_threshold;
    double usable_range_min, usable_range_max;
    double translation_regularizer, rotation_regularizer;
    double max_correspondence_dist;
    double max_segment_length;
} lgs_icp_params;

typedef struct {
    int pose_found;               /* 0 when a pass paired fewer than 3 beams */
    int iterations;               /* steps made */
    int num_pairs;                /* pairs of the last pass */
    int initial_pairs;            /* pairs at the initial pose */
    double normalized_cost;       /* cost / NumOfScans() */
    lgs_pose2d initial_pose;
    lgs_pose2d estimated_pose;    /* MoveBackward(best_sensor_pose, relPose) */
    /* inv(H + diag(regularizers)) by the closed-form adjugate, scaled by
     * pair_cost / max(1, num_pairs - 3); all zero when pose_found == 0 or the
     * determinant is 0 or not finite.  With A = H + diag, row-major a0..a8:
     *   c00 = a4*a8 - a5*a7   c01 = a2*a7 - a1*a8   c02 = a1*a5 - a2*a4
     *   c10 = a5*a6 - a3*a8   c11 = a0*a8 - a2*a6   c12 = a2*a3 - a0*a5
     *   c20 = a3*a7 - a4*a6   c21 = a1*a6 - a0*a7   c22 = a0*a4 - a1*a3
     *   det = (a0*c00 + a1*c10) + a2*c20
     *   covariance[3r+c] = (c_rc / det) * (pair_cost / max(1, num_pairs - 3)) */
    double covariance[9];
    lgs_pose2d sensor_pose;       /* Compound(initial_pose, relPose) */
    lgs_pose2d best_sensor_pose;  /* the last pose */
    double cost;                  /* last pass: e^2 per pair, max_correspondence_dist^2 per usable unpaired beam */
    double pair_cost;             /* last pass: e^2 per pair */
    double initial_cost;
    double hessian[9];            /* last pass's H, row-major, without the regularizers */
    double rhs[3];                /* last pass's b = sum of (-e) g */
} lgs_icp_summary;
size_t lgs_icp_params_size(void);    /* sizeof, for bindings */
size_t lgs_icp_summary_size(void);

/* One refine of `scan` from initial_pose (robot poses; the sensor poses are
 * Compound(pose, the scan's relative sensor pose)) against ref_scan at
 * ref_pose.  trajectory (may be NULL; room for 5 * max(1, num_iterations_max)
 * doubles) receives after every step the sensor pose (x, y, theta), the cost
 * at it and the pairs there (as a double). */
int  lgs_icp_optimize_pose(lgs_ctx* ctx, const lgs_scan* ref_scan, lgs_pose2d ref_pose, const lgs_scan* scan,
                           lgs_pose2d initial_pose, const lgs_icp_params* params, lgs_icp_summary* out,
                           double* trajectory);
/* n refines, item j: scans[j] from initial_poses[j] against ref_scans[j] at
 * ref_poses[j]; pointers may repeat, scans may differ in size.  One workgroup
 * per item, one launch per chunk (4096 items), one synchronisation per call.
 * Equal to n lone calls byte for byte. */
int  lgs_icp_optimize_pose_batch(lgs_ctx* ctx, const lgs_scan* const* ref_scans, const lgs_pose2d* ref_poses,
                                 const lgs_scan* const* scans, const lgs_pose2d* initial_poses, int n,
                                 const lgs_icp_params* params, lgs_icp_summary* out);
/* Diagnostics: the search alone at one *sensor* pose of `scan`.  Per beam of
 * `scan`: index[i] = the paired reference beam j*, -1 for a usable beam that
 * was rejected, -2 for an unusable one; residual[i] = e for a pair, else 0. */
int  lgs_icp_pairs(lgs_ctx* ctx, const lgs_scan* ref_scan, lgs_pose2d ref_pose, const lgs_scan* scan,
                   lgs_pose2d sensor_pose, const lgs_icp_params* params, int* index, double* residual);

/* ---- point-to-line ICP against a set of reference scans (k_icp_ref.hip) ----
 * A reference is the table of 4.5b built once from scans R_0 .. R_{K-1} at
 * robot poses P_k: the table of R_0 at Compound(P_0, rel_0), then that of R_1,
 * and so on; entries in scan order, then beam order; lines never cross scans;
 * each scan's usable interval is its own.  An entry's index is its position in
 * this concatenation.  It lives in global memory behind the handle, together
 * with a uniform grid over its points.  Pass, sums, tree, loop, summary and
 * covariance are those of lgs_icp_* over that table: a beam pairs with the
 * entry of the smallest computed d2 (ties to the lowest index; +inf and NaN
 * never win) and the pair is accepted iff d2 <= D^2 and the entry has a line.
 * The grid only changes the order in which entries are looked at (an entry
 * with d2 <= D^2 always lies in the 3 x 3 cells around the hit point's), so
 * the bytes are those of the brute-force search, and with one reference scan
 * those of lgs_icp_optimize_pose / _batch / _pairs.
 * LGS_ERR_INVALID_ARG, before any device work: a NULL argument (trajectory
 * apart), n_refs < 1 or > 4096, n < 0, the parameter and pose rules of
 * lgs_icp_*, an empty scan, more than LGS_ICP_REF_MAX_ENTRIES usable reference
 * beams in total, a reference of another context, and refine-time params whose
 * usable_range_min/max, max_segment_length or max_correspondence_dist differ
 * bitwise from those the reference was created with.  A reference whose beams
 * are all unusable is legal (an empty table: pose_found = 0).  An angle outside
 * the restated sincos domain fails with LGS_ERR_INTERNAL, at create for the
 * reference scans' and at refine for the scan's.  A failing call writes
 * nothing to its outputs. */
#define LGS_ICP_REF_MAX_ENTRIES 262144
typedef struct lgs_icp_ref lgs_icp_ref;
/* Copies what it needs: the scans may be destroyed afterwards.  The reference
 * belongs to ctx; like an lgs_grid it owns its device memory and may be
 * destroyed after its context. */
int  lgs_icp_ref_create(lgs_ctx* ctx, const lgs_scan* const* ref_scans, const lgs_pose2d* ref_poses, int n_refs,
                        const lgs_icp_params* params, lgs_icp_ref** out);
void lgs_icp_ref_destroy(lgs_icp_ref* ref);
/* Reference scans, table entries, entries with a line, the grid's cells per
 * axis and its cell side (each may be NULL). */
int  lgs_icp_ref_info(const lgs_icp_ref* ref, int* n_refs, int* entries, int* lines, int* cells_x, int* cells_y,
                      double* cell_size);
/* lgs_icp_optimize_pose against the reference */
int  lgs_icp_ref_optimize_pose(lgs_ctx* ctx, const lgs_icp_ref* ref, const lgs_scan* scan, lgs_pose2d initial_pose,
                               const lgs_icp_params* params, lgs_icp_summary* out, double* trajectory);
/* n refines, item j: scans[j] from initial_poses[j] against refs[j]; pointers
 * may repeat.  Equal to n lone calls byte for byte. */
int  lgs_icp_ref_optimize_pose_batch(lgs_ctx* ctx, const lgs_icp_ref* const* refs, const lgs_scan* const* scans,
                                     const lgs_pose2d* initial_poses, int n, const lgs_icp_params* params,
                                     lgs_icp_summary* out);
/* The search alone at one *sensor* pose.  Per beam of `scan`: for a pair the
 * reference scan ref_index[i] = k and its beam beam_index[i] = j; -1 / -1 for
 * a usable beam that was rejected, -2 / -2 for an unusable one; residual[i] =
 * e for a pair, else 0. */
int  lgs_icp_ref_pairs(lgs_ctx* ctx, const lgs_icp_ref* ref, const lgs_scan* scan, lgs_pose2d sensor_pose,
                       const lgs_icp_params* params, int* ref_index, int* beam_index, double* residual);

/* ---- many ICP references in one pass, one per local map (k_icp_ref.hip) ----
 * The graph snapshot is that of lgs_maps_construct_from_scans: scans[n_scans] at
 * robot poses[n_scans] and n_refs inclusive node ranges idx_min[i] <= idx_max[i]
 * < n_scans, which may overlap (a scan may belong to several references).
 * Reference i of the set is, in everything a caller can observe,
 *   lgs_icp_ref_create(scans[idx_min[i] .. idx_max[i]], poses[same], params):
 * lgs_icp_ref_info, lgs_icp_ref_pairs (ref_index counted from the range's first
 * scan) and lgs_icp_ref_optimize_pose / _batch (summary, trajectory, Hessian)
 * give the same bytes; the order inside a grid cell stays free, as in 4.5c.  A
 * range whose beams are all unusable gives an empty reference, legal as there.
 * The build is one pass over the whole set: two device allocations (tables,
 * cells) that every reference's arrays point into at 256-byte-aligned offsets,
 * one launch of each of four kernels (table; count, scan, scatter of the
 * grids) and two host waits on the stream, whatever n_refs is.
 * lgs_icp_ref_set_ref(set, i) is borrowed: valid until the set is destroyed,
 * ignored by lgs_icp_ref_destroy, accepted by every lgs_icp_ref_* refine-time
 * call and free to share a batch with references lgs_icp_ref_create made; NULL
 * for an index outside 0 .. size - 1.  Like an lgs_icp_ref the set copies what
 * it needs and may be destroyed after its context.
 * LGS_ERR_INVALID_ARG, before any device work: a NULL argument, n_refs < 1 or
 * > 4096, a range outside [0, n_scans) or idx_min > idx_max, every
 * per-reference rule of lgs_icp_ref_create (1 .. 4096 scans, at most
 * LGS_ICP_REF_MAX_ENTRIES usable beams, finite poses, no NULL or empty scan,
 * the parameter rules), more than LGS_ICP_REF_SET_MAX_ENTRIES usable beams over
 * the whole set.  LGS_ERR_OOM, after the table pass (the grids are known only
 * then): more than LGS_ICP_REF_SET_MAX_CELLS grid cells over the whole set;
 * nothing leaks and the context stays usable.  An angle outside the restated
 * sincos domain: LGS_ERR_INTERNAL.  A failing call writes nothing to *out. */
#define LGS_ICP_REF_SET_MAX_ENTRIES 4194304   /* over the whole set */
#define LGS_ICP_REF_SET_MAX_CELLS   16777216  /* grid cells over the whole set */
typedef struct lgs_icp_ref_set lgs_icp_ref_set;
int  lgs_icp_ref_set_create(lgs_ctx* ctx, const lgs_scan* const* scans, const lgs_pose2d* poses, int n_scans,
                            const int* idx_min, const int* idx_max, int n_refs, const lgs_icp_params* params,
                            lgs_icp_ref_set** out);
void lgs_icp_ref_set_destroy(lgs_icp_ref_set* set);
int  lgs_icp_ref_set_size(const lgs_icp_ref_set* set);   /* 0 for NULL */
const lgs_icp_ref* lgs_icp_ref_set_ref(const lgs_icp_ref_set* set, int i);
/* Counters of this context since its creation (each may be NULL): set builds
 * that reached the device; launches of the build's table, count, scan and
 * scatter kernels; host waits on the stream made by set builds; launches of
 * the refine kernel by any lgs_icp_ref_optimize_pose / _batch or
 * lgs_loop_refine_icp call. */
int  lgs_icp_ref_set_stats(const lgs_ctx* ctx, long long* builds, long long* table_launches,
                           long long* count_launches, long long* scan_launches, long long* scatter_launches,
                           long long* build_syncs, long long* refine_launches);
/* Diagnostics: the host clock of this context's last successful set build, in
 * milliseconds (each may be NULL): from the call's first device work to the
 * end of the wait behind the table pass (allocation, uploads, the table
 * kernel, the boxes' download), and from there to the end of the build (the
 * grids' geometry, allocation, count, scan, scatter, the final wait). */
int  lgs_icp_ref_set_last_build_ms(const lgs_ctx* ctx, double* table_ms, double* grids_ms);

/* ---- loop records refined by ICP against those references ----
 * results[num_candidates] are a loop detector's records (in/out), queries and
 * candidates the batch that made them; of a query only local_map_node_pose,
 * first_candidate and num_candidates are read (map and coarse may be NULL), of
 * a candidate only its scan.  refs[q] is query q's reference.  Every candidate
 * c of query q with results[c].found != 0 and a finite results[c].estimated_pose
 * becomes one item -- candidates[c].scan from that pose against refs[q] -- and
 * all items run as one lgs_icp_ref_optimize_pose_batch (one launch per 4096
 * items, one synchronisation; no item: no device work at all).
 * The item is accepted iff, in fp64 without contraction on the host,
 *   pose_found != 0, num_pairs >= min_pairs, normalized_cost <= max_normalized_cost,
 *   dx * dx + dy * dy <= max_translation * max_translation   (refined estimate minus the record's),
 *   fabs(NormalizeAngle(theta' - theta)) <= max_rotation      (H/util.hpp:125-135);
 * a NaN fails every comparison.  An accepted record gets estimated_pose,
 * covariance and normalized_cost of the item's summary and relative_pose =
 * InverseCompound(queries[q].local_map_node_pose, estimated_pose); every other
 * byte stays (found, the indices, start_node_pose, score, pad) and refined[c] =
 * 1.  Every other record -- not found, estimate not finite, rejected -- keeps
 * its 176 bytes and refined[c] = 0.  summaries (may be NULL; num_candidates
 * entries) receives each item's summary, zero bytes for a candidate that did
 * not run.
 * LGS_ERR_INVALID_ARG, before any device work: a NULL argument (summaries
 * apart; a NULL refs[q] or candidate scan included), num_queries or
 * num_candidates < 0, queries that do not cover the candidates contiguously,
 * in order and completely (the rule of lgs_loop_detect_rtcsm), min_pairs < 3, a
 * gate value that is NaN or negative (+inf is legal), and for every item the
 * refine-time rules of lgs_icp_ref_*.  A failing call leaves results, refined
 * and summaries untouched. */
typedef struct {
    int    min_pairs;
    double max_normalized_cost, max_translation, max_rotation;
} lgs_loop_refine_gate;
int  lgs_loop_refine_icp(lgs_ctx* ctx, const lgs_icp_ref* const* refs, const lgs_loop_query* queries, int num_queries,
                         const lgs_loop_candidate* candidates, int num_candidates, const lgs_icp_params* params,
                         const lgs_loop_refine_gate* gate, lgs_loop_result* results, int* refined,
                         lgs_icp_summary* summaries);

/* ---- ICP loop detector: a window search of start poses (k_icp_window.hip) ----
 * The lattice.  nx = 2 * half_x + 1 poses along x, ny and nt likewise,
 * P = nx * ny * nt per candidate.  Lattice index p = (it * ny + iy) * nx + ix
 * (theta outermost, x innermost).  The robot pose of p around a centre c is
 *   ( c.x     + (double)(ix - half_x)     * step_xy,
 *     c.y     + (double)(iy - half_y)     * step_xy,
 *     c.theta + (double)(it - half_theta) * step_theta ),
 * each product and each sum rounded once, nothing contracted; the coordinate
 * of the centre index (ix == half_x, ...) is c's own, bit for bit.  The sensor
 * pose is Compound(lattice pose, the scan's relative sensor pose) with glibc's
 * sincos.
 * The score.  cost[p] and pairs[p] are byte for byte the initial_cost and
 * initial_pairs that lgs_icp_ref_optimize_pose(ctx, ref, scan, lattice pose p,
 * params, ...) returns: the first pass of 4.5b at that sensor pose over the
 * table of 4.5c, summed in 4.5b's tree.
 * The selection.  The best pose p* is the lexicographic minimum of (cost, p):
 * p wins iff cost < best || (cost == best && p < p*), from (+inf, -1).  Ties go
 * to the lowest index, neither NaN nor +inf wins, and p* = -1 if nothing wins.
 * LGS_ERR_INVALID_ARG, before any device work: a NULL argument (the optional
 * outputs apart), a half outside 0 .. 512, a step that is not finite or <= 0,
 * P > LGS_ICP_WINDOW_MAX_POSES, a scan of more than LGS_ICP_WINDOW_MAX_BEAMS
 * beams, a centre or an outermost lattice coordinate that is not finite, the
 * refine-time rules of lgs_icp_ref_* (context, bitwise-equal table parameters,
 * an empty scan), and for the detector the query-cover rule and the gate rules
 * of lgs_loop_refine_icp.  An angle outside the restated sincos domain (a
 * lattice theta included) fails with LGS_ERR_INTERNAL.  A failing call writes
 * nothing to its outputs. */
typedef struct {
    int    half_x, half_y, half_theta;   /* 2h + 1 poses per axis, each h in 0 .. 512 */
    double step_xy, step_theta;          /* finite, > 0 */
} lgs_icp_window;
#define LGS_ICP_WINDOW_MAX_POSES 1048576  /* per candidate */
#define LGS_ICP_WINDOW_MAX_BEAMS 4096     /* beams of the scanned scan */
size_t lgs_icp_window_size(void);    /* sizeof, for bindings */
/* The dense scores of one window: cost[P] and pairs[P] in lattice order.  One
 * launch and one wait on the stream. */
int  lgs_icp_ref_window_scores(lgs_ctx* ctx, const lgs_icp_ref* ref, const lgs_scan* scan, lgs_pose2d centre,
                               const lgs_icp_window* window, const lgs_icp_params* params, double* cost, int* pairs);
/* The detector.  Queries and candidates follow the rules of
 * lgs_loop_refine_icp; of a query only local_map_node_pose,
 * local_map_node_index, first_candidate and num_candidates are read (map and
 * coarse may be NULL).  For candidate c of query q the window is centred on
 * candidates[c].node_pose against refs[q]; that gives p*.  If p* >= 0 one
 * refine starts from lattice pose p*, and all candidates' refines run as one
 * lgs_icp_ref_optimize_pose_batch.  The gate is lgs_loop_refine_icp's, with the
 * start lattice pose in the place of the record's estimate, so max_translation
 * and max_rotation bound how far the refine may wander from where the window
 * put it.  results[c], as the other detectors write one: all 176 bytes zero,
 * then start_node_index, end_node_index and start_node_pose; if a refine ran,
 * estimated_pose, normalized_cost and covariance of its summary and score =
 * (double)num_pairs / (double)NumOfScans(); found = 1 iff the gate accepts, and
 * only then relative_pose = InverseCompound(local_map_node_pose,
 * estimated_pose).  best_index (may be NULL) receives p* per candidate,
 * summaries (may be NULL) the refines' summaries, zero bytes where none ran.
 * With all three halves 0 the detector is "refine from the node pose".
 * One score launch and one wait per chunk of candidates (a chunk holds
 * max(1, 67108864 / P) candidates: 64 or more), then one wait for the refines:
 * two waits per call below that cap, whatever the number of candidates.
 * num_candidates = 0 is legal and does no device work. */
int  lgs_loop_detect_icp(lgs_ctx* ctx, const lgs_icp_ref* const* refs, const lgs_loop_query* queries, int num_queries,
                         const lgs_loop_candidate* candidates, int num_candidates, const lgs_icp_params* params,
                         const lgs_icp_window* window, const lgs_loop_refine_gate* gate, lgs_loop_result* results,
                         int* best_index, lgs_icp_summary* summaries);
/* Counters of this context since its creation (each may be NULL): calls of the
 * two entry points above that reached the device, launches of the score
 * kernel, host waits on the stream made by those calls (refines included), and
 * launches of the refine kernel made by lgs_loop_detect_icp. */
int  lgs_icp_window_stats(const lgs_ctx* ctx, long long* calls, long long* score_launches, long long* syncs,
                          long long* refine_launches);

/* ---- nearest-node loop searcher (k_loop_search.hip) ----
 * LoopSearcherNearest::Search (C/mapping/loop_searcher_nearest.cpp:13-108) over
 * flat arrays, batched over hints.  A graph snapshot is poses[n] (node k has
 * index k) and m local maps with inclusive node ranges idx_min[i] <= idx_max[i]
 * < n (they may overlap and need not be contiguous: the convention of
 * lgs_maps_construct_from_scans).  The walk is the list of positions (map i,
 * node k), i = 0 .. m - 2, k = idx_min[i] .. idx_max[i], in that order;
 * travel[p] is the reference's nodeTravelDist after position p (t = 0,
 * prev = poses[0]; per position t += hypot(prev.x - x, prev.y - y), prev =
 * pose), formed on the host with the C library's hypot.
 * Per hint: only the positions of maps 0 .. num_maps - 2 are walked; cut is
 * the lowest of them with accum_travel_dist - travel[p] < travel_dist_threshold
 * (or their count); the winner is the lowest position p < cut that minimises
 * d2 = (x_k - x_r) * (x_k - x_r) + (y_k - y_r) * (y_k - y_r) (r the latest node;
 * no contraction) among those with d2 < pow(node_dist_threshold, 2.0).
 * Device, host function and reference agree byte for byte, whatever the
 * tiling: the reduction is an argmin under a strict <.
 * LGS_ERR_INVALID_ARG, before any device work: a NULL argument (per_map
 * apart), n < 1, m < 1, n, m, q or the walk's length above 2^27, a range outside
 * [0, n) or idx_min > idx_max, a non-finite pose x / y, threshold or
 * accum_travel_dist, num_candidate_nodes < 0, num_maps outside 1 .. m,
 * latest_local_map_idx outside [0, num_maps), a latest node outside [0, n) or
 * outside its latest local map's range.  A failing call writes nothing. */
typedef struct {
    int latest_node_idx;        /* LoopSearchHint::mLatestNodeIdx */
    int latest_local_map_idx;   /* mLatestLocalMapIdx */
    int num_maps;               /* mLocalMapPositions.size(): 1 .. m */
    int pad_;                   /* 0 */
    double accum_travel_dist;   /* mAccumTravelDist */
} lgs_loop_search_hint;
/* LoopSearcherNearest's constructor arguments */
typedef struct {
    double travel_dist_threshold;
    double node_dist_threshold;
    int num_candidate_nodes;
    int pad_;
} lgs_loop_search_params;
/* One record per hint; every byte is defined, so records compare bytewise.
 * Nothing found: found = 0, the four indices -1, dist_sq = pow(node_dist_threshold, 2.0). */
typedef struct {
    int found;
    int local_map_idx;          /* LoopCandidate::mLocalMapIdx */
    int local_map_node_idx;     /* mLocalMapNodeIdx */
    int node_idx_min;           /* mNodeIndices = node_idx_min .. node_idx_max: */
    int node_idx_max;           /* max(latest map's min, latest - K), min(its max, latest + K) */
    int walked;                 /* cut */
    double dist_sq;             /* the winner's d2 */
} lgs_loop_search_result;
/* Per-map table entry: the lowest-position minimiser inside one map's segment
 * of the walk under the same cut and threshold; none = {-1, 0, pow(thr, 2.0)}.
 * Row j * m + i is hint j's entry for map i; maps the hint does not walk
 * (num_maps - 1 .. m - 1) hold none.  The record's winner is the lowest map
 * with the strictly smallest dist_sq of its hint's row. */
typedef struct {
    int node_idx;
    int pad_;
    double dist_sq;
} lgs_loop_search_map_best;
typedef struct lgs_loop_graph lgs_loop_graph;
/* The snapshot behind a handle: the walk and travel[] are formed here, on the
 * host, and uploaded once.  Copies what it needs.  The handle belongs to ctx
 * and, like an lgs_grid, may be destroyed after it. */
int  lgs_loop_graph_create(lgs_ctx* ctx, const lgs_pose2d* poses, int n, const int* idx_min, const int* idx_max,
                           int m, lgs_loop_graph** out);
void lgs_loop_graph_destroy(lgs_loop_graph* graph);
/* Nodes, maps, walk positions and travel[positions - 1] (0 for an empty walk); each may be NULL */
int  lgs_loop_graph_info(const lgs_loop_graph* graph, int* n, int* m, int* positions, double* walk_travel);
/* Diagnostics: travel[0 .. positions) into out (cap doubles at least positions) */
int  lgs_loop_graph_travel(const lgs_loop_graph* graph, double* out, int cap);
/* q hints against the snapshot: results[q], and per_map[q * m] unless NULL.
 * Below LGS_OPT_LOOP_SEARCH_MIN_PAIRS hint x position pairs the host loop runs
 * instead of the kernels (same bytes).  q = 0 is legal. */
int  lgs_loop_search_nearest(lgs_loop_graph* graph, const lgs_loop_search_params* params,
                             const lgs_loop_search_hint* hints, int q, lgs_loop_search_result* results,
                             lgs_loop_search_map_best* per_map);
/* The reference's loop, statement for statement, per hint: no context, no GPU */
int  lgs_loop_search_nearest_host(const lgs_pose2d* poses, int n, const int* idx_min, const int* idx_max, int m,
                                  const lgs_loop_search_params* params, const lgs_loop_search_hint* hints, int q,
                                  lgs_loop_search_result* results, lgs_loop_search_map_best* per_map);
/* GridMapBuilder::UpdateAccumTravelDist (C/mapping/grid_map_builder.cpp:210-224):
 * the hypot chain over all nodes, on the host */
int  lgs_pg_accum_travel_dist(const lgs_pose2d* poses, int n, double* out);
/* Searches on this context since its creation: out4 = {calls that ran the
 * kernels, calls that ran the host loop, kernel launches, hint x position
 * pairs of the device calls} */
int  lgs_loop_search_stats(const lgs_ctx* ctx, long long* out4);
#define LGS_OPT_LOOP_SEARCH_MIN_PAIRS 39 /* lgs_loop_search_nearest: calls of fewer hint x walk-position pairs run the host loop instead of launching (default 65536, the measured crossover rounded down to a power of two); 0 = always the device */
#define LGS_OPT_LOOP_SEARCH_GROUP     40 /* tests: walk positions per workgroup group of the search's main pass (groups are whole maps; results do not depend on it; a size that gives more than 65535 groups is doubled until they fit); 0 (default) = chosen from the walk's length and the hint count */

#ifdef __cplusplus
}
#endif

#endif /* LGS_HIP_H */
