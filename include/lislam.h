/*
 * lislam — MI355X (gfx950) implementation of the per-scan hot path of
 * himhan34/Intensity_based_LiDAR_SLAM_for_me-: Ouster cloud -> range/intensity images ->
 * LOAM curvature features -> scan-to-scan kNN association -> point-to-line / point-to-plane
 * residual + Jacobian -> Ceres-semantics pose solve.
 *
 * C ABI (plain pointers and sizes; no C++ or torch types).  Every function returns an int
 * status (LISLAM_OK == 0); lislam_last_error() describes the last failure of a context.
 * A context owns one HIP device + stream and is not internally thread safe; use one context
 * per callback thread / GPU (the reference runs one ROS node per process, scanRegistration.cpp:738).
 *
 * Reference interfaces replaced (file:line in the reference tree):
 *   lislam_scan_registration  <- ImageHandler::cloud_handler        src/image_handler.h_ouster:103
 *                                + laserCloudHandler                   src/scanRegistration.cpp:189-658
 *   lislam_odom_step          <- laserOdometry main-loop body          src/laserOdometry.cpp:313-808
 *   lislam_batch_*            <- the same two stages for a batch of scans resident in HBM
 *                                (independent scans / chains of scans)
 *   lislam_eval_factors       <- ceres::CostFunction::Evaluate of LidarEdgeFactor /
 *                                LidarPlaneFactor / LidarPlaneNormFactor
 *                                                                      src/lidarFeaturePointsFunction.hpp:143-293
 *   lislam_map_*              <- KD_TREE Build / Add_Points / Nearest_Search / size / flatten
 *                                                                      src/ikd-Tree/ikd_Tree.h:256-279
 *   lislam_map_associate      <- 5-NN line / plane association        src/laserMapping.cpp:668-796,
 *                                                                      src/mapOptimization.cpp:376-429
 *   lislam_normal_equations / lislam_pose_solve
 *                             <- ceres::Solve(DENSE_QR) of those blocks (laserMapping.cpp:836-845,
 *                                mapOptimization.cpp:433-442)
 *   lislam_voxel_grid         <- pcl::VoxelGrid::filter                (scanRegistration.cpp:583-586,
 *                                laserMapping.cpp:608-616, mapOptimization.cpp:368-370)
 *   lislam_mapopt_step        <- mapOptimization::mapOptimizationCallback ground-map stage
 *                                                                      src/mapOptimization.cpp:99-479
 *   lislam_laser_mapping      <- laserMapping::process optimization    src/laserMapping.cpp:620-850
 *   lislam_lmap_*             <- laserMapping::process with its cube map src/laserMapping.cpp:319-1002
 *   lislam_batch_intensity_odometry / lislam_intensity_tracker_*
 *                             <- feature_tracker::detectfeatures       src/intensity_feature_tracker.cpp:597-738
 *   lislam_ground_extract / lislam_batch_ground
 *                             <- ImageHandler::groundPlaneExtraction   src/image_handler.h_ouster:41-100
 *   lislam_batch_upload / lislam_batch_download_cloud
 *                             <- pcl::fromROSMsg / toROSMsg            src/image_handler.h_ouster:105-106,
 *                                                                      src/scanRegistration.cpp:592-642
 *   lislam_loop_icp           <- loopClosureThread's USE_ICP block     src/intensity_feature_tracker.cpp:217-366
 *   lislam_keyframes_* / lislam_loop_verify
 *                             <- keyframe_pool_[i].cloud_track_ + the same block for a batch of candidates
 *   lislam_odom_fuse          <- odomHandler callback                src/odom_handler_node.cpp:44-132
 *   lislam_place_*            <- SCManager (Scan Context)             src/Scancontext.cpp:126-344
 *   lislam_bow_*              <- detectLoop's DBoW3 query (ORB words)  src/loop_closure_handler.cpp:127-188
 *   lislam_bow_train(er_*)    <- DBoW3::Vocabulary::create: the tree    src/loop_closure_handler.cpp:12-17 loads from a file
 *   lislam_pgo_*              <- the gtsam factor graph + updatePoses  src/intensity_feature_tracker.cpp:110-145,
 *                                                                      :314-381, :395-583
 *   lislam_keysel_*           <- feature_tracker::getKeyframe          src/intensity_feature_tracker.cpp:741-815
 *   (lislam_feeds.h)          <- the same feeds for a list of selected scans; mapOdomHandle's keyframe-to-keyframe edges :395-514
 */
#ifndef LISLAM_H_
#define LISLAM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LISLAM_OK 0
#define LISLAM_ERR_ARG (-1)      /* invalid argument / unsupported configuration */
#define LISLAM_ERR_DEVICE (-2)   /* HIP runtime error */
#define LISLAM_ERR_CAPACITY (-3) /* caller buffer too small */
#define LISLAM_ERR_STATE (-4)    /* call out of order */

typedef struct lislam_ctx lislam_ctx;
typedef struct lislam_batch lislam_batch;
typedef struct lislam_odom lislam_odom;

/* Parameters the reference reads from the ROS parameter server / compile-time constants. */
typedef struct {
  int32_t n_scans;        /* N_SCANS = image_height (scanRegistration.cpp:692; spot.yaml:8): 16/32/64/128 */
  int32_t width;          /* image_width (spot.yaml:7) */
  float min_range;        /* MINIMUM_RANGE = remove_radius (scanRegistration.cpp:695; spot.yaml:49) */
  int32_t max_iterations; /* ceres max_num_iterations of the odometry solve (laserOdometry.cpp:707) */
  int32_t want_images;    /* materialize image_range / image_intensity / cloud_track (a1) */
} lislam_config;

/* Field layout of a sensor_msgs/PointCloud2 point (fromROSMsg, image_handler.h_ouster:106). */
typedef struct {
  uint32_t point_step; /* bytes per point (Ouster: 48; PCL PointXYZI: 32; packed xyzI: 16) */
  uint32_t off_x, off_y, off_z, off_intensity; /* byte offsets of the float32 fields */
} lislam_point_layout;

/* Features of one scan as published by scanRegistration (scanRegistration.cpp:592-642).
 * Points are float32 (x, y, z, intensity) quadruples; intensity = scanID + 0.1 * relTime.
 * Capacities are in points; on return n_* hold the counts.  Null pointers are skipped. */
typedef struct {
  float* laser_cloud; int32_t cap_laser_cloud; int32_t n_laser_cloud;   /* /velodyne_cloud_2 */
  float* sharp; int32_t cap_sharp; int32_t n_sharp;                     /* /laser_cloud_sharp */
  float* less_sharp; int32_t cap_less_sharp; int32_t n_less_sharp;      /* /laser_cloud_less_sharp */
  float* flat; int32_t cap_flat; int32_t n_flat;                        /* /laser_cloud_flat */
  float* less_flat; int32_t cap_less_flat; int32_t n_less_flat;         /* /laser_cloud_less_flat */
  uint8_t* image_range; uint8_t* image_intensity;                       /* H*W each (cloud_handler) */
  float* cloud_track;                                                   /* H*W*4 (cloud_handler) */
} lislam_scan_out;

/* One frame of features as consumed by laserOdometry (laserOdometry.cpp:336-377). */
typedef struct {
  const float* sharp; int32_t n_sharp;
  const float* less_sharp; int32_t n_less_sharp;
  const float* flat; int32_t n_flat;
  const float* less_flat; int32_t n_less_flat;
} lislam_frame;

/* ---------------------------------------------------------------- context */
int lislam_ctx_create(const lislam_config* cfg, int32_t device, lislam_ctx** out);
int lislam_ctx_destroy(lislam_ctx* ctx);
const char* lislam_last_error(const lislam_ctx* ctx);
int lislam_synchronize(lislam_ctx* ctx);
/* Use an external hipStream_t (e.g. a torch stream) instead of the context's own. */
int lislam_set_stream(lislam_ctx* ctx, void* hip_stream);
int lislam_get_stream(lislam_ctx* ctx, void** hip_stream);

/* ---------------------------------------------------------------- single scan (drop-in) */
/* laserCloudHandler: one organized cloud of n_scans*width points (host memory) -> features. */
int lislam_scan_registration(lislam_ctx* ctx, const void* points, const lislam_point_layout* layout,
                             lislam_scan_out* out);

/* laserOdometry node: state = last corner/surf clouds, para_q/para_t, q_w_curr/t_w_curr. */
int lislam_odom_create(lislam_ctx* ctx, lislam_odom** out);
int lislam_odom_destroy(lislam_odom* od);
/* Process one frame.  para_out[7] = (q_last_curr x,y,z,w, t_last_curr), pose_out[7] = (q_w_curr,
 * t_w_curr), stats_out[8] = corner/plane correspondences of the two outer passes, LM iterations
 * of each pass, termination of each pass (0 max-iterations, 1 convergence, 2 failure). */
int lislam_odom_step(lislam_odom* od, const lislam_frame* frame, double* para_out, double* pose_out,
                     int32_t* stats_out);
/* The reference's default gating (laserOdometry.cpp:403-417): the frame is associated and
 * optimized only when use_aloam != 0 (its sharp cloud's frame_id == "skip_intensity"); otherwise
 * para_q/para_t carry over and the pose accumulates them (:716-717). */
int lislam_odom_step_gated(lislam_odom* od, const lislam_frame* frame, int32_t use_aloam, double* para_out,
                           double* pose_out, int32_t* stats_out);
/* lislam_batch_odometry_status for the node: engine launches of its steps that gave up (each was
 * re-run on the per-round schedule within the step) since the previous call; the call clears it. */
int lislam_odom_status(lislam_odom* od, int32_t* status);

/* ---------------------------------------------------------------- batch (device resident) */
int lislam_batch_create(lislam_ctx* ctx, int32_t max_scans, lislam_batch** out);
int lislam_batch_destroy(lislam_batch* b);
/* Copy n_scans clouds from host memory (contiguous, n_scans*n_scans_cfg*width points). */
int lislam_batch_upload(lislam_batch* b, const void* points, int32_t n_scans, const lislam_point_layout* layout);
/* The same ingest without blocking the host: the bytes go to the device on the batch's copy
 * stream in chunks of 16 scans, and each chunk is parsed (k_unpack_layout) on the context stream
 * as soon as it has landed, after whatever the context stream was doing before (the previous
 * batch's extraction still reading the input buffer).  So the transfer of the next batch overlaps
 * the processing of the current one.  `points` must stay valid and unchanged until the context
 * stream has passed the upload (lislam_synchronize, or any download); pinned memory makes the
 * copies asynchronous. */
int lislam_batch_upload_async(lislam_batch* b, const void* points, int32_t n_scans, const lislam_point_layout* layout);
/* Device pointer of the packed float4 (x,y,z,intensity) input buffer [max_scans][H*W]. */
int lislam_batch_input_device_ptr(lislam_batch* b, void** dptr);
/* a1..a7 for scans [0, n_scans) of the batch. */
int lislam_batch_extract(lislam_batch* b, int32_t n_scans);
/* a12..a18 for scans [0, n_scans): ceil((n_scans-1)/chain_len) independent chains, chain c is a
 * fresh laserOdometry node over scans [c*chain_len, min((c+1)*chain_len, n_scans-1)]. */
int lislam_batch_odometry(lislam_batch* b, int32_t n_scans, int32_t chain_len);
/* The reference's default gating (laserOdometry.cpp:403-417): pair (k-1, k) is associated and
 * optimized only when use_aloam[k] != 0 — the sharp cloud's frame_id is "skip_intensity", i.e.
 * the intensity tracker skipped scan k (scanRegistration.cpp:603-609; LISLAM_OUT_ORB_STATS[0] ==
 * 0).  Otherwise para keeps the previous estimate and the pose accumulates it (:716-717).
 * use_aloam[n_scans]: host or device memory; a host array is copied before the call returns, so
 * it may be freed then.  lislam_batch_odometry = every use_aloam set. */
int lislam_batch_odometry_gated(lislam_batch* b, int32_t n_scans, int32_t chain_len, const int32_t* use_aloam);
/* Enable per-kernel HIP-event timing: every following extract / odometry call records events on
 * the stream (no host synchronization). */
int lislam_batch_set_timing(lislam_batch* b, int32_t enable);
/* Kernels timed by lislam_batch_kernel_times, in this order. */
#define LISLAM_NUM_KERNELS 9 /* k_scan_front, k_scan_lines, k_scan_compact, k_target_index,
                                k_odom_assoc, k_odom_lm (the latter includes k_odom_init),
                                k_odom_chain (the persistent engine of few long chains: association
                                and solve of every round in one launch), k_odom_to_end and
                                k_target_index_round (LISLAM_DISTORTION_TO_END: TransformToEnd of the
                                scans a round solved and the index of their to-end clouds) */
/* Synchronize, then return, over the calls recorded since the previous read, the average ms
 * per call spent in each kernel (ms_per_call[LISLAM_NUM_KERNELS]) and the launches per call of
 * each kernel (launches_per_call[LISLAM_NUM_KERNELS], may be null); calls[2] (may be null) =
 * extract / odometry calls averaged.  Clears the record.  (LISLAM_NUM_KERNELS was 6 before the
 * chain engine and 7 before lislam_set_distortion: size the arrays from the macro.) */
int lislam_batch_kernel_times(lislam_batch* b, float* ms_per_call, int32_t* launches_per_call, int32_t* calls);

#define LISLAM_OUT_IMAGE_RANGE 0     /* uint8  [H*W] */
#define LISLAM_OUT_IMAGE_INTENSITY 1 /* uint8  [H*W] */
#define LISLAM_OUT_CLOUD_TRACK 2     /* float4 [H*W] */
#define LISLAM_OUT_LASER_CLOUD 3     /* float4 [n]   */
#define LISLAM_OUT_CURVATURE 4       /* float  [n]   */
#define LISLAM_OUT_LABEL 5           /* int8   [n]   */
#define LISLAM_OUT_LINE_OFFSETS 6    /* int32  [H+1] */
#define LISLAM_OUT_SHARP 7           /* float4 [n]   */
#define LISLAM_OUT_LESS_SHARP 8      /* float4 [n]   */
#define LISLAM_OUT_FLAT 9            /* float4 [n]   */
#define LISLAM_OUT_LESS_FLAT 10      /* float4 [n]   */
#define LISLAM_OUT_PARA 11           /* double [7]   */
#define LISLAM_OUT_POSE 12           /* double [7]   */
#define LISLAM_OUT_STATS 13          /* int32  [8]   */
#define LISLAM_OUT_ORB_T 14          /* double [7]   T_s2s of pair (scan-1, scan) (q x,y,z,w, t) */
#define LISLAM_OUT_ORB_STATS 15      /* int32  [8]   see lislam_intensity_tracker_step */
#define LISLAM_OUT_ORB_KEYPOINTS 16  /* float  [n][6] of the nfeatures detection */
#define LISLAM_OUT_ORB_POINTS 17     /* float4 [n]   their cloud_track points */
#define LISLAM_OUT_ORB_DESCRIPTORS 18 /* uint8 [n][32] */
#define LISLAM_OUT_GROUND 19         /* float4 [n]   ground cloud x, y, z, 1 (lislam_batch_ground) */
#define LISLAM_OUT_GROUND_PLANE 20   /* float  [4]   segmented plane A, B, C, D */
#define LISLAM_OUT_GROUND_INFO 21    /* int32  [4]   status (1 ground, 0 plane rejected by the n.z >
                                        cos 15 deg test, -1 < 3 candidates, -2 no model, -3 sampling
                                        beyond the device map), RANSAC iterations, best inliers,
                                        refit inliers */
/* 22..24: the clouds TransformToEnd leaves (laserOdometry.cpp:176-194, the block :762-790): they exist
 * only after an odometry call in LISLAM_DISTORTION_TO_END (lislam_set_distortion), for the scans of
 * that call; otherwise a download returns LISLAM_ERR_STATE with a lislam_last_error text.  Outputs
 * 3, 8 and 10 stay as extraction left them. */
#define LISLAM_OUT_CORNER_LAST 22    /* float4 [n]   less-sharp cloud at the scan's end, intensity = int()
                                        (/laser_cloud_corner_last) */
#define LISLAM_OUT_SURF_LAST 23      /* float4 [n]   less-flat cloud, likewise (/laser_cloud_surf_last) */
#define LISLAM_OUT_FULL_RES_END 24   /* float4 [n]   laser cloud, likewise (/velodyne_cloud_3) */
/* Copy one output of one scan to host memory; cap/n count elements of the listed type.  dst null:
 * only *n is set (the element count). */
int lislam_batch_download(lislam_batch* b, int32_t what, int32_t scan, void* dst, int32_t cap, int32_t* n);
/* toROSMsg of a point-cloud output (laser cloud, the four feature clouds, cloud_track, ground,
 * ORB points, the three to-end clouds; scanRegistration.cpp:592-642): cap / n points written into dst in the given
 * PointCloud2 layout (e.g. PCL PointXYZI: point_step 32, x 0, y 4, z 8, intensity 16), packed on
 * the device; bytes outside the four fields are zero.  lislam_batch_upload parses any layout on
 * the device the same way (fromROSMsg). */
int lislam_batch_download_cloud(lislam_batch* b, int32_t what, int32_t scan, void* dst, const lislam_point_layout* layout,
                                int32_t cap, int32_t* n);

/* Odometry schedule of lislam_batch_odometry (results are the same): LISLAM_ENGINE_OFF issues one
 * association and one solve launch per round (chains advance together, one workgroup per chain's
 * solve); LISLAM_ENGINE_ON runs every round of every chain inside ONE persistent launch
 * (k_odom_chain: a device ticket queue orders the association and solve items, no host round trip
 * between scans) — the schedule of few long chains, e.g. the reference's single continuous chain;
 * LISLAM_ENGINE_AUTO (default) picks ON for at most 4 chains. */
#define LISLAM_ENGINE_OFF 0
#define LISLAM_ENGINE_AUTO 1
#define LISLAM_ENGINE_ON 2
int lislam_set_odometry_schedule(lislam_ctx* ctx, int32_t mode);
/* Motion de-skew of the scan-to-scan odometry: the reference's `#define DISTORTION`
 * (laserOdometry.cpp:82) for lislam_batch_odometry(_gated) and lislam_odom_step(_gated).
 * OFF (default): DISTORTION 0, s = 1, today's results bit for bit.
 * QUERIES: the file compiled with DISTORTION 1 as it stands: TransformToStart (:147-172) and every
 *   LidarEdgeFactor / LidarPlaneFactor (:548-556, :671-679) take s = (intensity - int(intensity)) /
 *   SCAN_PERIOD of the query point (float subtraction, fp64 division) and interpolate the pose,
 *   Identity.slerp(s, q_last_curr) and s t_last_curr.  A negative relTime leaves int(intensity) on the
 *   line below (s near 10, or slightly negative on line 0); that is the reference's behaviour and kept.
 * TO_END: QUERIES plus the block :762-790, which the reference keeps under `if (0)`, enabled:
 *   TransformToEnd (:176-194) moves every frame's less-sharp, less-flat and laser clouds to the scan's
 *   end with the para the frame ends with (a first frame: the identity; a gated-off frame: the carried
 *   para), so pair k searches scan k - 1's de-skewed clouds.  They are LISLAM_OUT_CORNER_LAST /
 *   SURF_LAST / FULL_RES_END.  A chain of a batch starts from its first scan as extraction left it (the
 *   identity para: the same xyz); a scan that ends one chain and starts the next holds the outputs
 *   of the chain that solved it, and the batch's scan 0 its identity version.
 * Modes other than OFF run on the per-round launches: LISLAM_ENGINE_AUTO and LISLAM_ENGINE_ON then
 * resolve to LISLAM_ENGINE_OFF and lislam_batch_odometry_engine reports 0.  As everywhere, the schedule
 * does not change results; the chain engine itself is DISTORTION 0 only. */
#define LISLAM_DISTORTION_OFF 0
#define LISLAM_DISTORTION_QUERIES 1
#define LISLAM_DISTORTION_TO_END 2
int lislam_set_distortion(lislam_ctx* ctx, int32_t mode);
/* The chain engine's shape for this context's launches (results are the same).
 * queries_per_wave: 1 = one association query per wavefront (64-lane searches: the shortest chain,
 * but one engine's association waves fill half of every CU); 2, 3 = that many 64-lane queries one
 * after another per wavefront; 4 = four at once, one per 16-lane row.  Above 1 each chain is
 * slower but an engine holds a fraction of the waves, so several engines and the next batches'
 * extraction share the GPU.  0 = keep.  depth = engines in flight per device when a launch of this
 * context enters the device's queue (1..6; a launch waits for the one `depth` launches before it);
 * 0 = keep.  Latency (one sequence at a time): 1 / 1, the default (one engine in flight, its item
 * workgroups 12 waves: a pass's queries in one round).  Throughput (several pipelined
 * contexts, e.g. bench.py): 3 / 5.  LISLAM_ENGINE_QPW / LISLAM_ENGINE_DEPTH seed a new context's
 * shape. */
int lislam_set_engine_shape(lislam_ctx* ctx, int32_t queries_per_wave, int32_t depth);
/* Engine pairing (results are the same).  At depth > 1 the library's engine dispatcher (a host thread per device) may run the
 * chains of two batches (of different contexts, or of one) as ONE engine launch: while one chain's
 * role solves a pass, the launch's item workgroups associate the other chain's, so the pair holds
 * the CUs of one launch and counts as one engine in flight.  Only compatible requests are paired:
 * one chain each, the same engine shape, scan geometry and iteration limit.
 * OFF: never.  AUTO (the default; no effect at depth 1): two requests that are ready together, or a
 * ready one with a partner whose inputs are about to exist (a short bounded hold, only while another
 * engine runs).  REQUIRE: a lone request is held until a compatible partner is ready, at most for
 * the engine's wait bound (2 s), then runs alone (tests: deterministic pairs). */
#define LISLAM_PAIRING_OFF 0
#define LISLAM_PAIRING_AUTO 1
#define LISLAM_PAIRING_REQUIRE 2
int lislam_set_engine_pairing(lislam_ctx* ctx, int32_t mode);
/* Engine segments (results are the same).  pairs > 0: at depth > 1 a one-chain odometry call of this
 * context runs as engine launches of `pairs` scan pairs each (the last one shorter), each starting
 * from the state the previous one left, and the dispatcher chooses the chain's partner
 * (lislam_set_engine_pairing) anew for every launch: a chain that becomes ready while another runs
 * joins it at its next segment, and one whose partner ends takes the next.  A launch that gives up
 * ends the chain there and the whole chain is re-run as ever (lislam_batch_odometry_status).
 * 0: whole chains, one launch each.  A new context starts from the build's LISLAM_ENGINE_SEGMENT (50).
 * No effect at depth 1, on several chains per call or under lislam_set_distortion. */
int lislam_set_engine_segment(lislam_ctx* ctx, int32_t pairs);
/* *paired = 1 if the batch's last engine launch (any segment of its last chain) was shared with
 * another batch's chain, else 0 (a settling call, see lislam_batch_odometry_status). */
int lislam_batch_odometry_paired(lislam_batch* b, int32_t* paired);
/* status = the number of engine launches of the batch that gave up since the previous status call
 * (one of the engine's bounded device waits expired, e.g. when its two launches could not run
 * together).  An aborted launch is recovered, not refused: the next call that reads or replaces the
 * batch's outputs waits for the engine on the host and re-runs that launch's chains on the
 * per-round schedule (LISLAM_ENGINE_OFF, no device waits) before it goes on, so the outputs are
 * always those of a complete schedule.  Those calls ("settling" calls): lislam_batch_extract,
 * lislam_batch_odometry(_gated), lislam_batch_download, lislam_batch_download_cloud,
 * lislam_batch_kernel_times, lislam_batch_odometry_status / _engine / _abort_code,
 * lislam_batch_mapopt(_corner), lislam_odom_step(_gated) and lislam_synchronize.  The calls that
 * touch only the input points or the ORB / ground stages do not wait for the engine:
 * lislam_batch_upload(_async), lislam_batch_input_device_ptr, lislam_batch_set_timing,
 * lislam_batch_ground, lislam_batch_intensity_odometry.  Reading the count clears it. */
int lislam_batch_odometry_status(lislam_batch* b, int32_t* status);
/* Which schedule the batch's last odometry call ran: 0 per-round launches, 1 the single-launch
 * engine (k_odom_chain), 2 the split engine (k_odom_roles + k_odom_items on CU-masked streams). */
int lislam_batch_odometry_engine(lislam_batch* b, int32_t* kind);
/* The error word of the batch's last aborted engine launch (0: none since the batch's creation):
 * which bounded wait gave up — 1 an association item waiting for the previous pass's items, 2 an
 * item waiting for its pass's pose, 3 a solve role waiting for its pass's items, 4 / 5 the
 * progressive gather's poll / loads, 0x57xx an overflow query out of range. */
int lislam_batch_odometry_abort_code(lislam_batch* b, int32_t* code);
/* The CU-masked streams the library holds on a device (*masked_queues).  Each is a hardware queue
 * of its own, and past about 20 of them in one process every launch slows: a context holds one
 * (its stream, which its ORB front end shares), the chain engine's 4 stream pairs and the per-round
 * schedule's group stream belong to the device (shared by all batches). */
int lislam_device_queue_count(int32_t device, int32_t* masked_queues);

/* Order of equal sort keys in the two std::sort calls of the feature extraction:
 * - each segment's sort by curvature (scanRegistration.cpp:445), which decides which of two
 *   points of equal curvature the sharp / flat walks (:450-568) reach first;
 * - the scan-line VoxelGrid(0.2) of the less-flat cloud (a7, :583-586): PCL 1.10's VoxelGrid
 *   sorts (voxel, point) pairs with std::sort by voxel alone, so a voxel's points are summed in
 *   the order libstdc++'s introsort leaves them.
 * LISLAM_TIES_REFERENCE (the default) replays libstdc++'s order exactly in both (bit-exact
 * selections and centroids); LISLAM_TIES_INDEX breaks ties by point index (faster; centroids
 * differ by float rounding, poses by up to 1e-4 on the bench data, tests/test_oracle.py).
 * Applies to later extractions of ctx. */
#define LISLAM_TIES_REFERENCE 0
#define LISLAM_TIES_INDEX 1
int lislam_set_tie_order(lislam_ctx* ctx, int32_t order);

/* ---------------------------------------------------------------- cost functors */
/* Evaluate n residual blocks at (q[4] = x,y,z,w, t[3]) on the GPU.  kind[i]: 0 LidarEdgeFactor
 * (pts: curr, a, b), 1 LidarPlaneFactor (curr, j, l, m), 2 LidarPlaneNormFactor (curr, n, d);
 * pts holds 12 doubles per block.  Outputs residuals[3n] (unused entries 0) and local-
 * parameterization Jacobians jac[3n x 6] (d/d delta-theta, d/d t), both optional. */
int lislam_eval_factors(lislam_ctx* ctx, int32_t n, const int32_t* kind, const double* pts, const double* q,
                        const double* t, double* residuals, double* jac);
/* ceres::AutoDiffCostFunction<F, R, 4, 3>::Evaluate of the reference functors on the GPU: the
 * Jacobians w.r.t. the raw parameter blocks, jac_q[n][3][4] (q x, y, z, w) and jac_t[n][3][3],
 * as Ceres' Jet differentiation gives them (lidarFeaturePointsFunction.hpp:29,49-54,157,183-190,
 * 208,228-234,252,282-288).  kind[i]: 0 LidarEdgeFactor (pts: curr, a, b), 1 LidarPlaneFactor
 * (curr, j, l, m), 2 LidarPlaneNormFactor (curr, n, d), 3 front_end_residual /
 * FeatureMatchingResidual (curr / src, dst; :21-99), 4 LidarGroundPlaneNormFactor (curr, n, d;
 * q block only, jac_t rows zero; :101-141), 5 LidarEdgeFactor with s != 1 (curr, a, b, s) and
 * 6 LidarPlaneFactor with s != 1 (curr, j, unit normal, s): DISTORTION 1, Identity.slerp(s, q)
 * and s t (:155-162,255-262).  Residual rows past the block's size are zero.  All
 * pointers may be host or device memory; outputs are optional.  include/lislam_factors.h wraps
 * this behind the reference's functor structs and their Create(). */
int lislam_eval_factors_raw(lislam_ctx* ctx, int32_t n, const int32_t* kind, const double* pts, const double* q,
                            const double* t, double* residuals, double* jac_q, double* jac_t);

/* ---------------------------------------------------------------- ORB intensity front end (a8-a11) */
/* cv::ORB::create(nfeatures, 1.2f, 8, 1) detect (with the feature_tracker MASK, H x W u8, 0 =
 * blocked; null = none) + extractPointsAndFilterZeroValue + compute on one intensity image
 * (intensity_feature_tracker.cpp:609-628, :1071-1099).  kp[n][6] = x, y, size, angle (deg),
 * response, octave; desc[n][32]; p3d[n][4] = the cloud_track point (x, y, z, 0).  cloud_track is
 * the organized H*W float4 cloud of ImageHandler::cloud_handler.  Host or device pointers.
 * H, W >= 8, nfeatures 1..16384.
 * Capacity: pyramid level l, whose share of the budget is n_l (nfeaturesPerLevel), keeps at most
 * 2 * n_l + 64 keypoints.  The reference is unbounded there: KeyPointsFilter::retainBest keeps every
 * response tied with the n_l-th, so an image that repeats a pattern can carry a level past any
 * fixed room.  Beyond it the call fails with LISLAM_ERR_CAPACITY (lislam_last_error names the ORB
 * level keypoint capacity) and returns no keypoints; it never returns a cut set. */
int lislam_orb_detect(lislam_ctx* ctx, const uint8_t* image, const float* cloud_track, const uint8_t* mask, int32_t H,
                      int32_t W, int32_t nfeatures, float* kp, uint8_t* desc, float* p3d, int32_t cap, int32_t* n);
/* BFMatcher(NORM_HAMMING, crossCheck=true).match(query, train) (:631): matches[m][3] = query,
 * train, distance in query order (capacity nq). */
int lislam_orb_match(lislam_ctx* ctx, const uint8_t* qdesc, int32_t nq, const uint8_t* tdesc, int32_t nt,
                     int32_t* matches, int32_t* n_matches);
/* feature_tracker::detectfeatures (intensity_feature_tracker.cpp:597-738): one frame per step,
 * state = the previous frame.  T_s2s[7] = (q x,y,z,w, t) of p2p_calculateRandT (identity when
 * the frame is skipped); stats[8] = good (1) / skipped (0) / first frame (-1), re-detected,
 * keypoints, matches, good matches, LM iterations, LM termination, previous keypoints.
 * A frame one of whose levels outgrows the capacity of lislam_orb_detect (2 * n_l + 64 keypoints,
 * in its n-feature or its 2n-feature detection) fails the step with LISLAM_ERR_CAPACITY; T_s2s and
 * stats are not written, the frame is not kept, and the next frame is treated as a first frame. */
typedef struct lislam_intensity_tracker lislam_intensity_tracker;
int lislam_intensity_tracker_create(lislam_ctx* ctx, int32_t H, int32_t W, int32_t nfeatures, const uint8_t* mask,
                                    lislam_intensity_tracker** out);
int lislam_intensity_tracker_destroy(lislam_intensity_tracker* t);
int lislam_intensity_tracker_step(lislam_intensity_tracker* t, const uint8_t* image, const float* cloud_track,
                                  double* T_s2s, int32_t* stats);
/* detectfeatures over scans [0, n_scans) of a batch (its a1 images, want_images = 1): scan k is
 * matched against scan k-1 exactly as the tracker would; outputs LISLAM_OUT_ORB_*.  Asynchronous:
 * it returns once its work is queued (on a side stream the context stream then waits for); the
 * sequential re-detection rule (intensity_feature_tracker.cpp:652-687) is decided on the device in
 * LISLAM_ORB_ROUNDS passes (default 1).  Reading an ORB output first checks that the device
 * decision converged, and redoes the batch with host-decided rounds if it did not.
 * Capacity: a scan one of whose levels outgrows the room of lislam_orb_detect (2 * n_l + 64
 * keypoints; the reference is unbounded), in its n-feature or a 2n-feature detection, fails the
 * batch with LISLAM_ERR_CAPACITY.  The call is asynchronous, so the failure is reported where the
 * batch's ORB outputs are first brought to the host: every lislam_batch_download of a
 * LISLAM_OUT_ORB_* output (and every other reader of the batch's ORB sets) fails with it until the
 * next lislam_batch_intensity_odometry, which starts clean. */
int lislam_batch_intensity_odometry(lislam_batch* b, int32_t n_scans, int32_t nfeatures, const uint8_t* mask);
/* The last lislam_batch_intensity_odometry's cascade, after its outputs were read: info[0] = 1
 * device-decided and converged, 0 redone with host rounds, -1 host rounds from the start
 * (LISLAM_ORB_HOST_CASCADE=1 or fewer than 2 scans); info[1] = device decision passes. */
int lislam_batch_orb_cascade_info(lislam_batch* b, int32_t* info);

/* ---- ground plane (ImageHandler::groundPlaneExtraction, src/image_handler.h_ouster:41-100):
 * z-band screening [-2, -0.45], PCL SACSegmentation(SACMODEL_PLANE, SAC_RANSAC, 0.01, optimized
 * coefficients) with PCL 1.10's single-thread sampling sequence, the n.z > cos(15 deg) test and
 * the points within 0.03 m of the plane with z < 0 — the GroundPointOut cloud mapOptimization
 * merges with the less-flat cloud (mapOptimization.cpp:136,148).  Outputs LISLAM_OUT_GROUND*. */
int lislam_batch_ground(lislam_batch* b, int32_t n_scans);
/* One organized cloud (the context's n_scans x width, any point layout): ground cloud out[cap][4]
 * (x, y, z, 1), *n_out, plane[4] (A, B, C, D) and info[4] as LISLAM_OUT_GROUND_INFO (each
 * nullable).  Replaces ImageHandler::groundPlaneExtraction's body. */
int lislam_ground_extract(lislam_ctx* ctx, const void* points, const lislam_point_layout* layout, float* out,
                          int32_t cap, int32_t* n_out, float* plane, int32_t* info);

/* ---------------------------------------------------------------- scan-to-map (a19-a21) */
/* A device-resident point map with the semantics of the vendored ikd-Tree
 * (src/ikd-Tree/ikd_Tree.h:256-279): Build, Add_Points with box downsampling, exact k-NN
 * Nearest_Search, and the mapping stages that consume it.  Points are float32 x, y, z; input
 * arrays are n points of `stride` floats (3 = PointXYZ packed, 4 = PointXYZ / PointXYZI as PCL
 * stores them).  Pointers may be host or device memory (copied with hipMemcpyDefault). */
typedef struct lislam_map lislam_map;

typedef struct {
  float downsample_size; /* ikd KD_TREE(delete_param, balance_param, box_length): 0.4 ground map,
                            0.8 corner map (mapOptimization.cpp:504-505) */
  float cell_size;       /* edge of the hash-grid cells the search walks (0: downsample_size);
                            a search accelerator only, results do not depend on it */
} lislam_map_config;

int lislam_map_create(lislam_ctx* ctx, const lislam_map_config* cfg, lislam_map** out);
int lislam_map_destroy(lislam_map* m);
/* KD_TREE::Build (ikd_Tree.cpp:470-492): the map holds exactly these points (ids 0..n-1). */
int lislam_map_build(lislam_map* m, const float* pts, int64_t n, int32_t stride);
/* KD_TREE::Add_Points (ikd_Tree.cpp:569-706).  downsample_on: per box of edge downsample_size
 * only the point nearest the box centre survives, as the reference's sequential loop leaves it.
 * Inputs take ids next_id .. next_id+n-1.  n_added (nullable) = inputs that entered the map. */
int lislam_map_add_points(lislam_map* m, const float* pts, int64_t n, int32_t stride, int32_t downsample_on,
                          int64_t* n_added);
/* KD_TREE::size / validnum. */
int lislam_map_size(lislam_map* m, int64_t* n);
/* KD_TREE::flatten / PCL_Storage: live points as (x, y, z, id bits), storage order. */
int lislam_map_points(lislam_map* m, float* out_xyzi, int64_t cap, int64_t* n);
/* KD_TREE::Nearest_Search (ikd_Tree.cpp:494-547) for n queries: up to k (<= 8) points with
 * squared distance <= max_dist^2 (max_dist <= 0: unbounded), ascending (squared float distance,
 * id).  out_pts[n][k][4] = x, y, z, id bits; out_d2[n][k]; out_found[n] (all nullable). */
int lislam_map_nearest_search(lislam_map* m, const float* queries, int32_t n, int32_t stride, int32_t k,
                              float max_dist, float* out_pts, float* out_d2, int32_t* out_found);

#define LISLAM_MATCH_LINE 0  /* laserMapping corner: 5-NN, PCA line, LidarEdgeFactor (laserMapping.cpp:668-723) */
#define LISLAM_MATCH_PLANE 1 /* 5-NN, QR plane, LidarPlaneNormFactor (laserMapping.cpp:744-796,
                                mapOptimization.cpp:376-429) */
/* Associate n sensor-frame points at pose x = (q x,y,z,w, t) against the map: out_rec[n][9]
 * (line: curr, a, b; plane: curr, n, d, 0, 0) and out_kind[n] (0 edge, 2 plane-norm, -1 none). */
int lislam_map_associate(lislam_map* m, int32_t kind, const float* pts, int32_t n, int32_t stride, const double* x,
                         double* out_rec, int32_t* out_kind);
/* Cost, J^T J (upper, 21) and J^T r (6) = 28 doubles of n records (kinds 0 edge / 1 plane /
 * 2 plane-norm, -1 skipped) under HuberLoss(0.1) at x (SURVEY.md §8(b) eval_normal_eq). */
int lislam_normal_equations(lislam_ctx* ctx, const double* rec, const int32_t* kind, int32_t n, const double* x,
                            double* out28);
/* ceres::Solve (DENSE_QR, max_iterations) of n records at x (in/out, 7 doubles).
 * summary[4] (nullable) = iterations, termination (0 no-convergence, 1 convergence, 2 failure),
 * edge blocks, plane blocks. */
int lislam_pose_solve(lislam_ctx* ctx, const double* rec, const int32_t* kind, int32_t n, double* x,
                      int32_t max_iterations, int32_t* summary);
/* pcl::VoxelGrid (leaf) of n points (x, y, z, intensity, stride 4): per-voxel centroid of all four
 * fields, output ordered by voxel index; points of a voxel summed in input order.  out holds up
 * to n points. */
int lislam_voxel_grid(lislam_ctx* ctx, const float* pts, int32_t n, float leaf, float* out, int32_t* n_out);

/* mapOptimization::mapOptimizationCallback ground-map stage (mapOptimization.cpp:99-479 without
 * the ORB / keyframe-image logic): ground = GroundPointOut (sensor frame, stride 4), odom =
 * q_wodom_curr, t_wodom_curr (7); state = q_wmap_wodom, t_wmap_wodom (7, in/out).  Empty map:
 * Build with the transformed cloud.  Otherwise VoxelGrid(0.8), plane association, Ceres(10 it),
 * transformUpdate on CONVERGENCE, Add_Points(downsample) at the keyframe pose.
 * out_pose = q_w_curr, t_w_curr; summary[3] = planes, iterations, termination (-1: built). */
int lislam_mapopt_step(lislam_map* m, const float* ground, int32_t n, const double* odom, double* state,
                       double* out_pose, int32_t* summary);
/* The same stage with mapOptimization's corner ikd-Tree (corner_ikdtree_, KD_TREE(0.3, 0.6, 0.8),
 * mapOptimization.cpp:195,479,505): the sensor-frame corner cloud (pc_corner, stride 4) goes in
 * at the ground cloud's keyframe pose, Build while that tree is empty, else Add_Points with
 * downsampling (create corner_map with downsample_size 0.8).  corner_map may be null. */
int lislam_mapopt_step_corner(lislam_map* m, lislam_map* corner_map, const float* ground, int32_t n,
                              const float* corner, int32_t nc, const double* odom, double* state, double* out_pose,
                              int32_t* summary);
/* The same stage fed from a batch without a host round trip: GroundPointOut of `scan`
 * (lislam_batch_ground) followed by its less-flat cloud, concatenated on the device
 * (mapOptimization.cpp:136-150).  The map's context must be the batch's. */
int lislam_batch_mapopt(lislam_batch* b, lislam_map* m, int32_t scan, const double* odom, double* state,
                        double* out_pose, int32_t* summary);
/* As lislam_batch_mapopt, with mapOptimization's corner ikd-Tree (corner_map, see
 * lislam_mapopt_step_corner) fed the scan's less-sharp cloud (/laser_cloud_less_sharp, the
 * pc_corner topic, mapOptimizationNode.cpp:63). corner_map NULL = lislam_batch_mapopt. */
int lislam_batch_mapopt_corner(lislam_batch* b, lislam_map* m, lislam_map* corner_map, int32_t scan,
                               const double* odom, double* state, double* out_pose, int32_t* summary);
/* ---- mapOptimization's ORB keyframe sliding window (keyframe_sliding_window_,
 * mapOptimization.cpp:155-169, :295-361, :481-493; SLIDING_WINDOW_SIZE = config sliding_window_size).
 * A keyframe is its ORB descriptors desc[n][32], their sensor-frame points p3d[n][4] (x, y, z, -)
 * and a pose (q x,y,z,w, t).  Device resident; pointers may be host or device memory. */
typedef struct lislam_mapwin lislam_mapwin;
/* window_size 0..16 (0: the window is always empty when it is read, :491-493), feature_capacity
 * 1..4096 per keyframe; anything else LISLAM_ERR_ARG.  A call with more than feature_capacity
 * features returns LISLAM_ERR_CAPACITY and changes nothing. */
int lislam_mapwin_create(lislam_ctx* ctx, int32_t window_size, int32_t feature_capacity, lislam_mapwin** out);
int lislam_mapwin_destroy(lislam_mapwin* win);
int lislam_mapwin_size(lislam_mapwin* win, int32_t* n);
/* emplace_back, then pop_front while the size exceeds window_size (:488-493). */
int lislam_mapwin_push(lislam_mapwin* win, const uint8_t* desc, const float* p3d, int32_t n, const double* pose);
/* Keyframe `index` (0 = oldest): up to cap features into desc / p3d (nullable), *n, pose[7] (nullable). */
int lislam_mapwin_keyframe(lislam_mapwin* win, int32_t index, uint8_t* desc, float* p3d, int32_t cap, int32_t* n,
                           double* pose);
/* cv::BFMatcher().match(desc, keyframe descriptors) (:305-307: NORM_L2, no cross-check) against
 * every window keyframe, newest first: matches[window][n][2] = train index (the first of equal
 * distances) and the integer sum of squared byte differences (the DMatch distance is its sqrtf);
 * both -1 when the keyframe has no descriptors. */
int lislam_mapwin_match(lislam_mapwin* win, const uint8_t* desc, int32_t n, int32_t* matches);
/* The window loop (:295-361) for a current keyframe (desc, p3d, n) at `pose`, against the whole
 * window in one set of launches.  Per window keyframe, newest first: the matches (M = n, or 0 when
 * either side is empty), used only if M > 100 (:309); std::sort by distance, equal distances in
 * query order (:312); G = #{i >= 0 : i < (double)M * 0.2} (:314); used only if G > 50, G != M and
 * the two descriptor counts differ (:327); of the first G matches those whose map-frame points
 * (each keyframe's own pose, :339-340) lie within 0.3 m (:342-346) give a
 * FeatureMatchingResidual(current point (sensor frame), window point (map frame)) (:348-354).
 * rec[cap][9] = kind-3 records (src, dst, 0, 0, 0), window keyframes newest to oldest, matches in
 * sorted order; *n_rec their number (more than cap: LISLAM_ERR_CAPACITY).  info[window_size][6]
 * (nullable), a row per window keyframe, newest first: train descriptors, M, G, used (0 / 1),
 * blocks kept, offset of its first block.  pairs[cap][3] (nullable) = window row, query index,
 * train index of each block. */
int lislam_mapwin_records(lislam_mapwin* win, const uint8_t* desc, const float* p3d, int32_t n, const double* pose,
                          double* rec, int32_t cap, int32_t* n_rec, int32_t* info, int32_t* pairs);
/* lislam_mapopt_step_corner with the window: the FeatureMatchingResiduals of (desc, p3d, nf) at the
 * initial guess (:112, :168-169) join the ground planes' problem, feature blocks first; after the
 * solve the keyframe enters the window with the optimised pose on CONVERGENCE, else with the
 * initial guess (:481-493).  The first call (empty map, Build) pushes nothing (:173-196, :218).
 * summary[5] = planes, iterations, termination (-1: built), feature blocks, window keyframes used.
 * win NULL or of window_size 0: lislam_mapopt_step_corner's outputs, bit for bit. */
int lislam_mapopt_step_window(lislam_map* m, lislam_map* corner_map, lislam_mapwin* win, const float* ground, int32_t n,
                              const float* corner, int32_t nc, const uint8_t* desc, const float* p3d, int32_t nf,
                              const double* odom, double* state, double* out_pose, int32_t* summary);
/* lislam_orb_detect with mapOptimization's extractPointsAndFilterZeroValue (mapOptimization.cpp:
 * 604-632): a keypoint is dropped only when |x|, |y| and |z| of its point are all below 0.01
 * (the feature tracker's drops on |x| alone).  The same level capacity and LISLAM_ERR_CAPACITY. */
int lislam_orb_detect_map(lislam_ctx* ctx, const uint8_t* image, const float* cloud_track, const uint8_t* mask,
                          int32_t H, int32_t W, int32_t nfeatures, float* kp, uint8_t* desc, float* p3d, int32_t cap,
                          int32_t* n);
/* lislam_batch_mapopt_corner with the window: cv::ORB::create(nfeatures, ...) features of the
 * scan's a1 intensity image and cloud_track (want_images = 1) as lislam_orb_detect_map finds them
 * (mask H x W, nullable) never leave the device.  Pass NUM_ORB_FEATURES * 2 as nfeatures (:155).
 * summary[5] as lislam_mapopt_step_window. */
int lislam_batch_mapopt_window(lislam_batch* b, lislam_map* m, lislam_map* corner_map, lislam_mapwin* win, int32_t scan,
                               int32_t nfeatures, const uint8_t* mask, const double* odom, double* state,
                               double* out_pose, int32_t* summary);

/* laserMapping::process optimization (laserMapping.cpp:620-850) against a corner map and a surf
 * map: the downsampled current corner / surf clouds (stride 4), pose x (in/out), two outer
 * passes of association + Ceres(4 it).  stats[4] = corner / surf blocks of each pass. */
int lislam_laser_mapping(lislam_map* corner_map, lislam_map* surf_map, const float* corner, int32_t n_corner,
                         const float* surf, int32_t n_surf, double* x, int32_t* stats);

/* ---- laserMapping's cube map (laserMapping.cpp:70-99, 319-1002), device
 * resident: 21 x 21 x 11 cubes of 50 m holding the corner / surf points in map frame. */
typedef struct lislam_lmap lislam_lmap;
/* line_res / plane_res: mapping_line_resolution / mapping_plane_resolution (spot.launch: 0.4 / 0.8). */
int lislam_lmap_create(lislam_ctx* ctx, float line_res, float plane_res, lislam_lmap** out);
int lislam_lmap_destroy(lislam_lmap* m);
/* One laserMapping::process frame without publishing: corner_last / surf_last (stride 4, sensor
 * frame, host or device), odom = q_wodom_curr, t_wodom_curr (7); state (in/out) = q_wmap_wodom,
 * t_wmap_wodom (7); out_pose = q_w_curr, t_w_curr (7).  transformAssociateToMap, cube re-centring,
 * the local map of the valid cubes, VoxelGrid of the current clouds, the optimization of
 * lislam_laser_mapping when the map holds > 10 corner and > 50 surf points, transformUpdate,
 * insertion and the VoxelGrid of every valid cube.  stats[8] (nullable) = corner / surf local-map
 * sizes, corner / surf stack sizes, lislam_laser_mapping's stats (-1 when not optimized). */
int lislam_lmap_step(lislam_lmap* m, const float* corner_last, int32_t nc, const float* surf_last, int32_t ns,
                     const double* odom, double* state, double* out_pose, int32_t* stats);
/* Points per cube (cube index order, 4851 each; either nullable) and a whole cloud (0 corner,
 * 1 surf) as x, y, z, intensity in cube order (out nullable: *n only). */
int lislam_lmap_counts(lislam_lmap* m, int32_t* corner_counts, int32_t* surf_counts);
int lislam_lmap_points(lislam_lmap* m, int32_t which, float* out, int64_t cap, int64_t* n);

/* ---- loop closure and odometry fusion */
/* loop_closure_parameters (config/spot.yaml:26-33) + the ICP settings of
 * intensity_feature_tracker.cpp:219-232. */
typedef struct {
  int32_t use_crop;                   /* USE_CROP (spot.yaml: false) */
  float crop_size;                    /* CROP_SIZE: CropBox [-c, c]^3 (spot.yaml: 200) */
  int32_t use_downsample;             /* USE_DOWNSAMPLE (true) */
  float voxel_size;                   /* VOXEL_SIZE = vf_scan_res (0.25) */
  float max_correspondence_distance;  /* setMaxCorrespondenceDistance (100) */
  int32_t max_iterations;             /* setMaximumIterations (100) */
  double transformation_epsilon;      /* setTransformationEpsilon (1e-6) */
  double euclidean_fitness_epsilon;   /* setEuclideanFitnessEpsilon (1e-6) */
  double fitness_threshold;           /* FITNESS_SCORE = icp_fitness_score (0.5) */
} lislam_icp_config;
/* The USE_ICP block of feature_tracker::loopClosureThread (intensity_feature_tracker.cpp:217-366)
 * with tranformCurrentScanToMap (:167-172) and getSubmapOfhistory (:174-193): cur = the new
 * keyframe's cloud_track (n_cur x, y, z, intensity), T_cur = getTransformMatrix(keyframeId)
 * (row-major 4x4); hist = the history keyframes' clouds concatenated (hist_counts[n_hist]) with
 * their poses T_hist[n_hist][16].  removeNaN, CropBox, VoxelGrid, pcl::IterativeClosestPoint and
 * getFitnessScore on the device.  Outputs (each nullable): T_icp[16] = getFinalTransformation,
 * T_cur2map[16] = T_icp * T_cur (the loop factor's pose_from, :316-321), fitness, info[8] =
 * accepted (1 converged and fitness <= threshold, 0 not, -1 empty submap, -2 <= 10 points after
 * filtering), converged, convergence state (0 none, 1 iterations, 2 transform, 3 absolute MSE,
 * 4 relative MSE, 5 < 3 correspondences), iterations, source points, target points, last
 * correspondences, 0.  Point arrays may be host or device memory. */
int lislam_loop_icp(lislam_ctx* ctx, const lislam_icp_config* cfg, const float* cur, int32_t n_cur, const double* T_cur,
                    const float* hist, const int32_t* hist_counts, int32_t n_hist, const double* T_hist, double* T_icp,
                    double* T_cur2map, double* fitness, int32_t* info);
/* loopClosureProcessor_.keyframe_pool_[i].cloud_track_ as a device-resident pool: keyframe ids are
 * consecutive from 0 in the order added (keyframeId_).  capacity = the most keyframes, point_capacity
 * the most points (x, y, z, intensity) it holds; going over either is LISLAM_ERR_CAPACITY and adds
 * nothing.  A cloud of 0 points is a valid keyframe. */
typedef struct lislam_keyframes lislam_keyframes;
int lislam_keyframes_create(lislam_ctx* ctx, int32_t capacity, int64_t point_capacity, lislam_keyframes** out);
int lislam_keyframes_destroy(lislam_keyframes* kf);
int lislam_keyframes_size(lislam_keyframes* kf, int32_t* n_keyframes, int64_t* n_points);
/* n_clouds clouds: points = their float quadruples one cloud after the other (host or device
 * memory), counts[n_clouds] (host) their sizes. */
int lislam_keyframes_add_clouds(lislam_keyframes* kf, const void* points, const int32_t* counts, int32_t n_clouds);
/* cloud_track of scans [first_scan, first_scan + n_scans) of an extracted batch of the same context
 * (want_images = 1), copied device to device; preconditions and error codes as lislam_place_add_batch. */
int lislam_keyframes_add_batch(lislam_keyframes* kf, lislam_batch* b, int32_t first_scan, int32_t n_scans);
/* Keyframe index into dst (cap_points quadruples, host); *n (nullable) = its points. */
int lislam_keyframes_download(lislam_keyframes* kf, int32_t index, float* dst, int32_t cap_points, int32_t* n);
/* lislam_loop_icp for n_loops candidates in one set of launches, the clouds read from the pool.
 * Candidate k = (cur_id[k], loop_id[k]) (host arrays); T_kf[pool size][16] = getTransformMatrix(i)
 * of every keyframe, row-major (host or device memory).  The submap (getSubmapOfhistory, :174-193)
 * is the keyframes i in [max(0, loop - submap_window), loop + submap_window] with i <= cur (the
 * reference's i < keyframe_pool_.size() when cur was the newest), ascending, each under T_kf[i];
 * submap_window in 0..4 (the reference compiles 1).  Row k of T_icp[n][16], T_cur2map[n][16],
 * fitness[n], info[n][8] (host, each nullable) is exactly what
 *   lislam_loop_icp(ctx, cfg, pool[cur], n, T_kf[cur], submap clouds, counts, n_hist, their T_kf rows, ...)
 * returns, bit for bit.  loop_id[k] < 0 (the "no loop" of lislam_place_detect / lislam_bow_detect)
 * gives info[0] = -3, T_icp = identity, T_cur2map = T_kf[cur], fitness = DBL_MAX, the other info
 * fields 0.  cur_id out of range, loop_id >= pool size, loop_id > cur_id or submap_window out of
 * range: LISLAM_ERR_ARG with a lislam_last_error text, nothing computed, outputs untouched.  More
 * than 0x3fffffff raw points over all candidates: LISLAM_ERR_CAPACITY.  n_loops == 0 is a no-op.
 * The same keyframe may appear in any number of candidates. */
int lislam_loop_verify(lislam_keyframes* kf, const lislam_icp_config* cfg, int32_t submap_window, const int32_t* cur_id,
                       const int32_t* loop_id, int32_t n_loops, const double* T_kf, double* T_icp, double* T_cur2map,
                       double* fitness, int32_t* info);
/* odomHandler's callback (src/odom_handler_node.cpp:44-132) over n synchronized pairs in order:
 * aloam[n][7] = /laser_odom_to_init_aloam, intensity[n][7] = /laser_odom_to_init_intensity
 * (q x,y,z,w, t), skip[n] = 1 when the intensity message's child_frame_id is "/odom_skip";
 * fused[n][7] = the published /laser_odom_to_init.  The fuser keeps the previous poses and
 * odom_cur on the device between calls.  Pointers may be host or device memory. */
typedef struct lislam_odom_fuser lislam_odom_fuser;
int lislam_odom_fuser_create(lislam_ctx* ctx, lislam_odom_fuser** out);
int lislam_odom_fuser_destroy(lislam_odom_fuser* f);
int lislam_odom_fuse(lislam_odom_fuser* f, const double* aloam, const double* intensity, const int32_t* skip, int32_t n,
                     double* fused);

/* ---- Scan Context place recognition: SCManager (include/Scancontext.h, src/Scancontext.cpp) as a
 * device-resident database.  Entry k is the k-th cloud added (the reference's polarcontexts_[k]). */
typedef struct lislam_place lislam_place;
typedef struct {
  double lidar_height;        /* LIDAR_HEIGHT (2.0) */
  double max_radius;          /* PC_MAX_RADIUS (80.0) */
  double search_ratio;        /* SEARCH_RATIO (0.1) */
  double dist_thres;          /* SC_DIST_THRES (0.13) */
  int32_t num_ring;           /* PC_NUM_RING (20), 1..40 */
  int32_t num_sector;         /* PC_NUM_SECTOR (60), 1..120 */
  int32_t num_exclude_recent; /* NUM_EXCLUDE_RECENT (50) */
  int32_t num_candidates;     /* NUM_CANDIDATES_FROM_TREE (10), 1..32 */
  int32_t tree_making_period; /* TREE_MAKING_PERIOD_ (50) */
} lislam_place_config;
/* cfg == NULL: the values above (Scancontext.h:77-96).  capacity = the most entries the database holds. */
int lislam_place_create(lislam_ctx* ctx, const lislam_place_config* cfg, int32_t capacity, lislam_place** out);
int lislam_place_destroy(lislam_place* p);
int lislam_place_size(lislam_place* p, int32_t* n);
/* makeAndSaveScancontextAndKeys (:237-251) of n_clouds clouds: points = their float (x, y, z,
 * intensity) quadruples one cloud after the other (host or device memory), counts[n_clouds] (host)
 * their sizes.  A point with a NaN x or y is skipped (undefined in the reference). */
int lislam_place_add_clouds(lislam_place* p, const void* points, const int32_t* counts, int32_t n_clouds);
/* The same for cloud_track of scans [first_scan, first_scan + n_scans) of an extracted batch of the
 * same context (want_images = 1), read where it lies on the device. */
int lislam_place_add_batch(lislam_place* p, lislam_batch* b, int32_t first_scan, int32_t n_scans);
/* detectLoopClosureID (:253-344) as it returned when entry k was the newest and had been called once
 * per entry before, for k in [first, first + n): loop_id (-1: none), yaw = deg2rad(nn_align * 360 / S),
 * and its internals min_dist, nn_idx, nn_align (1e7, 0, 0 while k < num_exclude_recent).  Host
 * arrays of n, each nullable.  The candidates are the exact nearest ring keys, equal distances by
 * lower index. */
int lislam_place_detect(lislam_place* p, int32_t first, int32_t n, int32_t* loop_id, float* yaw, double* min_dist,
                        int32_t* nn_idx, int32_t* nn_align);
/* distanceBtnScanContext (:126-157) of entries a[k] and b[k] (host arrays): dist, shift (nullable). */
int lislam_place_distance(lislam_place* p, const int32_t* a, const int32_t* b, int32_t n_pairs, double* dist, int32_t* shift);
#define LISLAM_PLACE_DESC 0       /* double [R * S], row-major ring x sector */
#define LISLAM_PLACE_RING_KEY 1   /* float [R] */
#define LISLAM_PLACE_SECTOR_KEY 2 /* double [S] */
/* One output of entry index into dst (cap elements); *n = the element count. */
int lislam_place_download(lislam_place* p, int32_t what, int32_t index, void* dst, int32_t cap, int32_t* n);

/* ---- ORB bag-of-words loop detection: loopClosureHandler::detectLoop (src/loop_closure_handler.cpp:127-188,
 * USE_ORBLOOP, called at :108-111) with its DBoW3 database device-resident.  DBoW3 is restated from the
 * published library for the combination the reference runs: TF_IDF weights, L1_NORM scoring, no direct
 * index (db_.setVocabulary(*voc_, false, 0)).  Entry k is the k-th image added (DBoW3's EntryId).
 *
 * The vocabulary is handed in as three host arrays over its n_nodes tree nodes, node 0 the root.  From a
 * loaded DBoW3::Vocabulary (config/orbvoc.dbow3; reading its file formats is the caller's host-side work):
 * parent[i] = m_nodes[i].parent (-1 for the root), descriptor[i] = the 32 bytes of m_nodes[i].descriptor
 * (CV_8U 1 x 32; unused for the root), weight[i] = m_nodes[i].weight (read for leaves only).  A node's
 * children are visited in ascending node id; a leaf's word id is its rank among leaves in ascending node
 * id (createWords).  Required: parent[0] == -1, 0 <= parent[i] < i, 1..64 children per inner node, finite
 * weights >= 0; otherwise LISLAM_ERR_ARG with a lislam_last_error text. */
typedef struct lislam_bow lislam_bow;
typedef struct {
  double min_loop_bow_threshold; /* th: detectLoop's MIN_LOOP_BOW_TH (0.0155) */
  double index_score_threshold;  /* the score a lower id must exceed to take over (0.015) */
  int32_t min_loop_search_gap;   /* gap: MIN_LOOP_SEARCH_GAP (50) */
  int32_t max_results;           /* results per query (4), 1..16 */
  int32_t min_frame_index;       /* a loop is reported only when i > this (5) */
  int32_t loop_index_bound;      /* ... and only to an entry id below this (6) */
} lislam_bow_config;
/* cfg == NULL: the values in brackets, the ones detectLoop compiles with (config/spot.yaml's 0.013 and 20
 * are a caller's choice).  capacity = the most entries; max_features = the most descriptors of one image
 * (1..2048). */
int lislam_bow_create(lislam_ctx* ctx, int32_t n_nodes, const int32_t* parent, const uint8_t* descriptor, const double* weight,
                      const lislam_bow_config* cfg, int32_t capacity, int32_t max_features, lislam_bow** out);
int lislam_bow_destroy(lislam_bow* p);
int lislam_bow_size(lislam_bow* p, int32_t* n);
/* Database::add of n_images images: desc = their packed 32-byte descriptor rows one image after the other
 * (host or device memory), counts[n_images] (host) their row counts.  An image without descriptors, or
 * whose words all weigh 0, still takes an id (an empty vector).  counts[k] > max_features is
 * LISLAM_ERR_ARG, more entries than the capacity LISLAM_ERR_CAPACITY; neither adds anything. */
int lislam_bow_add(lislam_bow* p, const void* desc, const int32_t* counts, int32_t n_images);
/* The same for the descriptors LISLAM_OUT_ORB_DESCRIPTORS reports of scans [first_scan, first_scan +
 * n_scans) of a batch of the same context, read (count included) where they lie on the device.
 * LISLAM_ERR_STATE unless lislam_batch_intensity_odometry has run over those scans; LISLAM_ERR_ARG for a
 * batch of another context or one that detects more than max_features features.  Asynchronous. */
int lislam_bow_add_batch(lislam_bow* p, lislam_batch* b, int32_t first_scan, int32_t n_scans);
/* detectLoop as it returned when entry k was the newest and had been called once per entry before, for k
 * in [first, first + n): loop_id[n] (-1: none) and the query behind it, db_.query(desc, ret, max_results,
 * k - gap): n_ret[n] results, ret_id / ret_score [n][max_results] best first (unused slots -1 / 0).
 * Equal scores come lower id first (DBoW3 leaves them to std::sort).  At k - gap == -1 the query is
 * unrestricted (Database::query's max_id == -1) and its results are reported although loop_id is -1.
 * Host arrays, each nullable.  The result for k depends on entries < k only. */
int lislam_bow_detect(lislam_bow* p, int32_t first, int32_t n, int32_t* loop_id, int32_t* n_ret, int32_t* ret_id,
                      double* ret_score);
/* L1Scoring::score of the vectors of entries a[k] and b[k] (host arrays), in [0, 1]. */
int lislam_bow_score(lislam_bow* p, const int32_t* a, const int32_t* b, int32_t n_pairs, double* score);
/* Vocabulary::transform(feature, id, weight) of n descriptors (host or device memory): word_id[n],
 * weight[n] (host, nullable). */
int lislam_bow_transform(lislam_bow* p, const void* desc, int32_t n, int32_t* word_id, double* weight);
#define LISLAM_BOW_WORDS 0  /* int32  [len] ascending word ids of one entry's BoW vector */
#define LISLAM_BOW_VALUES 1 /* double [len] their L1-normalized values */
/* One output of entry index into dst (cap elements); *n = the element count. */
int lislam_bow_download(lislam_bow* p, int32_t what, int32_t index, void* dst, int32_t cap, int32_t* n);

/* ---- Vocabulary training: DBoW3::Vocabulary::create (hierarchical k-means++ over the binary descriptors,
 * then TF_IDF word weights), restated from the published library (Vocabulary.cpp: HKmeansStep,
 * initiateClustersKMpp, createWords, setNodeWeights; DescManip::meanValue).  A trainer collects the
 * descriptors of many images on the device; lislam_bow_train turns them into the (parent, descriptor,
 * weight) arrays lislam_bow_create takes, node ids in DBoW3's order (a step appends all its children,
 * then recurses into child 0, child 1, ...: parent[i] < i, the children of a node consecutive).
 *
 * One step, on a node's descriptors in their original order (image, then row): with at most k of them
 * each becomes its own child; otherwise k-means++ seeds up to k centres (plain Hamming distances, all
 * integers; it stops early when every descriptor equals a centre), every descriptor goes to the first
 * centre at the smallest distance, and (bit-majority means, assignment) repeat until an assignment
 * equals the one before.  A child is clustered in turn if it holds more than one descriptor and its
 * level is below L.  weight = log(N / Ni), N = the images added (empty ones too), Ni = the images in
 * which the word occurs; 0 for Ni == 0 and for inner nodes.
 *
 * Three points are this library's own, because DBoW3 leaves them open or cannot be replayed in parallel:
 *  - random draws do not follow rand() in visiting order but a counter-based generator keyed by the node:
 *      splitmix64(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *                     z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)
 *      key(root) = splitmix64(seed), key(child slot c) = splitmix64(key(parent) ^ (c + 1)),
 *      draw j of a node = splitmix64(key + j * 0x9E3779B97F4A7C15), reduced to [0, n) as
 *      ((x >> 32) * n) >> 32.  Draw 0 picks the first centre, draw j >= 1 the value r in [1, S] that
 *      picks centre j (the first descriptor whose inclusive prefix sum of min-distances reaches r);
 *  - an empty cluster keeps its centre (DBoW3's meanValue is undefined there);
 *  - a node stops after max_iterations assignments (the seeding's is the first); DBoW3 has no limit. */
typedef struct lislam_bow_trainer lislam_bow_trainer;
typedef struct {
  int32_t k;              /* children per node, 2..64 */
  int32_t L;              /* levels below the root, 1..10 */
  int32_t max_iterations; /* >= 1 */
  uint64_t seed;
} lislam_bow_train_config;
#define LISLAM_BOW_TRAIN_MAX_L 10
#define LISLAM_BOW_TRAIN_MAX_DESCRIPTORS (1 << 23) /* every sum of distances fits 31 bits */
#define LISLAM_BOW_PHASE_SEED 0
#define LISLAM_BOW_PHASE_ASSIGN 1
#define LISLAM_BOW_PHASE_MEANS 2
#define LISLAM_BOW_PHASE_PARTITION 3
typedef struct {
  int32_t profile; /* in: nonzero = wait for the device after every phase and fill phase_ms (slower) */
  int32_t n_nodes, n_words, n_zero_words; /* the root included; leaves; leaves of weight 0 */
  int32_t n_levels;                       /* levels that held a node to cluster, <= L */
  /* per level (index 0 = the root's step): steps run, those with more than k descriptors (k-means), the
   * largest iteration count among them (0 if none), how many of them stopped at max_iterations */
  int32_t level_steps[LISLAM_BOW_TRAIN_MAX_L], level_clustered[LISLAM_BOW_TRAIN_MAX_L];
  int32_t level_iterations[LISLAM_BOW_TRAIN_MAX_L], level_capped[LISLAM_BOW_TRAIN_MAX_L];
  double level_ms[LISLAM_BOW_TRAIN_MAX_L];    /* host wall clock of the level */
  double phase_ms[LISLAM_BOW_TRAIN_MAX_L][4]; /* LISLAM_BOW_PHASE_*, only with profile */
  double weights_ms;                          /* descent, image counts, log */
  double total_ms;                            /* the whole call, renumbering included */
} lislam_bow_train_stats;
/* Room for cap_images images and cap_descriptors descriptors (<= LISLAM_BOW_TRAIN_MAX_DESCRIPTORS, else
 * LISLAM_ERR_CAPACITY). */
int lislam_bow_trainer_create(lislam_ctx* ctx, int32_t cap_images, int32_t cap_descriptors, lislam_bow_trainer** out);
int lislam_bow_trainer_destroy(lislam_bow_trainer* t);
int lislam_bow_trainer_size(lislam_bow_trainer* t, int32_t* n_images, int32_t* n_descriptors);
/* n_images images: packed 32-byte rows one image after the other (host or device memory), counts[n_images]
 * (host).  An image without descriptors counts towards N.  A negative count is LISLAM_ERR_ARG, more images
 * or descriptors than there is room for LISLAM_ERR_CAPACITY; neither adds anything.  Allowed after a
 * lislam_bow_train: the next training sees every image added so far. */
int lislam_bow_trainer_add(lislam_bow_trainer* t, const void* desc, const int32_t* counts, int32_t n_images);
/* The same for the descriptors LISLAM_OUT_ORB_DESCRIPTORS reports of scans [first_scan, first_scan + n_scans)
 * of a batch of the same context, read where they lie on the device.  Errors as lislam_bow_add_batch. */
int lislam_bow_trainer_add_batch(lislam_bow_trainer* t, lislam_batch* b, int32_t first_scan, int32_t n_scans);
/* Vocabulary::create(k, L, TF_IDF) over everything added.  cfg == NULL: k 10, L 5 (DBoW3's constructor
 * defaults), max_iterations 100, seed 0.  *n_nodes (nullable) = the size of the arrays; stats nullable.
 * A trainer without descriptors trains to the root alone (n_nodes 1), a tree lislam_bow_create rejects.
 * May be repeated with another configuration.  k, L or max_iterations out of range: LISLAM_ERR_ARG. */
int lislam_bow_train(lislam_bow_trainer* t, const lislam_bow_train_config* cfg, int32_t* n_nodes,
                     lislam_bow_train_stats* stats);
/* The arrays of the last training (host, cap_nodes rows each, each nullable): what lislam_bow_create takes.
 * LISLAM_ERR_STATE before a training, LISLAM_ERR_CAPACITY if cap_nodes is below n_nodes. */
int lislam_bow_trainer_vocabulary(lislam_bow_trainer* t, int32_t cap_nodes, int32_t* parent, uint8_t* descriptor,
                                  double* weight);

/* ---- Pose-graph optimization: the factor graph of feature_tracker::mapOdomHandle / loopClosureThread
 * (src/intensity_feature_tracker.cpp:395-583, :314-381) as a device-resident least-squares problem,
 * solved in batch (Levenberg-Marquardt; it replaces iSAM2's incremental update with the batch optimum
 * of the same factors).  All fp64.  A pose is 7 doubles qx qy qz qw tx ty tz (as LISLAM_OUT_POSE); a
 * tangent vector is [omega(3), v(3)], rotation first (GTSAM's Pose3 order), so variances[6] read as
 * gtsam::noiseModel::Diagonal::Variances does: rad^2 x 3, m^2 x 3.  Exp / Log are the full SE(3) maps,
 * the retraction is T <- T Exp(delta).
 *   between factor (i, j, Z, variances, robust), h = Ti^-1 Tj: e = Log(Z^-1 h) / sigma,
 *     J_j = D / sigma, J_i = -D Ad(h^-1) / sigma, D = the inverse right Jacobian of SE(3) at e sigma;
 *   prior (node, P, variances): e = Log(P^-1 T) / sigma, J = D / sigma;
 *   robust = 1: Cauchy(k = 1), cost log(1 + |e|^2) / 2, IRLS weight 1 / (1 + |e|^2); robust = 0: |e|^2 / 2.
 * Domain: the relative rotation of every Z^-1 h (and P^-1 T) stays below pi - 0.1; outside it the
 * result is undefined, as Log itself is.
 * Outer loop: solve (H + lambda clamp(diag H, 1e-6, 1e32)) delta = -g, accept iff the cost strictly
 * decreases (lambda <- max(lambda / 10, 1e-12)), else lambda <- 10 lambda; stop when an accepted step's
 * relative cost decrease is below rel_cost_tol, lambda > 1e10 or after max_iterations solves.  The
 * linear solve is CG preconditioned by the block-tridiagonal part of the damped matrix. */
typedef struct lislam_pgo lislam_pgo;
typedef struct {
  int32_t max_iterations;    /* LM iterations (50) */
  int32_t cg_max_iterations; /* per solve; 0 = 6 L + 8, L = the edges with |i - j| != 1 (0) */
  double lambda_init;        /* (1e-4) */
  double rel_cost_tol;       /* (1e-10) */
  double cg_rel_tol;         /* |r| / |g| (1e-12) */
} lislam_pgo_config;
#define LISLAM_PGO_CONVERGED 0      /* info[0]: relative cost decrease below rel_cost_tol */
#define LISLAM_PGO_LAMBDA_LIMIT 1   /* lambda > 1e10 */
#define LISLAM_PGO_MAX_ITERATIONS 2 /* max_iterations solves done */
/* cfg == NULL: the values in brackets. */
int lislam_pgo_create(lislam_ctx* ctx, const lislam_pgo_config* cfg, int32_t node_capacity, int32_t edge_capacity,
                      lislam_pgo** out);
int lislam_pgo_destroy(lislam_pgo* p);
int lislam_pgo_size(lislam_pgo* p, int32_t* nodes, int32_t* edges);
/* n nodes with consecutive ids; pose7[n][7] = each node's initial estimate (host). */
int lislam_pgo_add_nodes(lislam_pgo* p, const double* pose7, int32_t n);
/* The graph's one prior (PriorFactor<Pose3>, :444-455); a second call replaces it.  linearize and
 * optimize need it (LISLAM_ERR_STATE without). */
int lislam_pgo_set_prior(lislam_pgo* p, int32_t node, const double* pose7, const double* var6);
/* n between factors (host arrays; robust nullable = all 0).  from < to, from > to and repeated pairs
 * are accepted; from == to, ids out of range and non-positive variances are LISLAM_ERR_ARG and leave
 * the graph unchanged. */
int lislam_pgo_add_edges(lislam_pgo* p, const int32_t* from, const int32_t* to, const double* meas7, const double* var6,
                         const int32_t* robust, int32_t n);
/* mapOdomHandle's pose_from.between(pose_to) for scans [first_scan, first_scan + n_scans) of a batch
 * whose odometry has run: each scan's LISLAM_OUT_POSE row, read where it lies on the device, becomes a
 * node, and every scan but the first gets an edge pose[k-1]^-1 pose[k] from the node before it; the
 * first one does too when the graph is not empty and first_scan > 0 (the batch then holds its
 * predecessor's pose).  var6 == NULL: odometryNoise_ (1e-6 x 3, 1e-8, 1e-8, 1e-6). */
int lislam_pgo_add_batch(lislam_pgo* p, lislam_batch* batch, int32_t first_scan, int32_t n_scans, const double* var6);
/* Edges [first, first + n) as the graph holds them (host arrays, each nullable). */
int lislam_pgo_edges(lislam_pgo* p, int32_t first, int32_t n, int32_t* from, int32_t* to, double* meas7, double* var6,
                     int32_t* robust);
/* The factors at the current estimate, the prior last (E = edges): residual[E+1][6] (whitened),
 * J_from[E][36], J_to[E+1][36] (row-major), weight[E+1], cost.  Host arrays, each nullable. */
int lislam_pgo_linearize(lislam_pgo* p, double* residual, double* J_from, double* J_to, double* weight, double* cost);
/* info[8] = status (LISLAM_PGO_*), LM iterations, accepted steps, total CG iterations, most CG
 * iterations in one solve, nodes, edges, 0; stats[4] = initial cost, final cost, final lambda, last CG
 * relative residual.  The same graph gives the same bytes from run to run. */
int lislam_pgo_optimize(lislam_pgo* p, int32_t* info, double* stats);
/* Nodes [first, first + n): pose7[n][7] and pose6d[n][6] = float x, y, z, roll, pitch, yaw, the
 * PointTypePose that getTransformMatrix (:152-165) turns back into the node's matrix: it builds
 * RzRyRx(yaw, pitch, roll), so roll is the angle about z and yaw the one about x (|pitch| < pi / 2). */
int lislam_pgo_poses(lislam_pgo* p, int32_t first, int32_t n, double* pose7, float* pose6d);

/* ---- Keyframe selection: feature_tracker::getKeyframe (src/intensity_feature_tracker.cpp:741-815, called
 * at :721) behind tfBroadcast's T_s2m_ = T_s2m_ * T_s2s_ (:819), the join between the per-scan ORB front
 * end and the back end's pools.  State (ctor :31-37), device resident: T_s2m = I, prev_p = 0, prev_R = 0,
 * next id 0, no keyframe yet.  For frame k, in stream order:
 *   T_s2m = T_s2m * [R(q) t; 0 0 0 1]   every frame, the identity of a skipped frame (:728) too; R(q) by
 *                                       Eigen's toRotationMatrix formula, the 4x4 product entry by entry as
 *                                       ((a0 b0 + a1 b1) + a2 b2) + a3 b3, plain double, no FMA
 *   good[k] != 1: keyframe_id[k] = -1   getKeyframe is called on good frames only (:693, :721)
 *   p, R = T_s2m's translation and rotation; the frame is selected iff no keyframe exists yet, or
 *   time[k] - last_time > time_interval and |p - prev_p| > distance_interval (:774-777, both strict);
 *   then node = (time[k], id, p, prev_p, R, prev_R), keyframe_id[k] = id, last_time = time[k],
 *   prev_p = p, prev_R = R, id += 1.
 * Decision: the reference's first branch tests cloudKeyPoses3D_->points.empty() (:749), a container
 * another thread fills (:536), so the number of frames that take it depends on scheduling there.  Here it
 * is taken exactly once, by the first good frame of the selector's life.
 * Two calls over the halves of a stream give what one call over the whole stream gives.
 * include/lislam_feeds.h declares the forms of the back end's feeds that take the selected scans as a list. */
typedef struct lislam_keysel lislam_keysel;
typedef struct {
  double time_interval;     /* KEYFRAME_TIME_INTERVAL: config/spot.yaml:35 has 0.3; readParameters' own default is 15 (:1120) */
  double distance_interval; /* KEYFRAME_DISTANCE_INTERVAL (0.3; "outdoor: 3") */
} lislam_keysel_config;
/* cfg == NULL: 0.3, 0.3.  A NaN interval is LISLAM_ERR_ARG. */
int lislam_keysel_create(lislam_ctx* ctx, const lislam_keysel_config* cfg, lislam_keysel** out);
int lislam_keysel_destroy(lislam_keysel* s);
/* n frames in stream order.  T_s2s[n][7] (q x,y,z,w, t) and good[n]: host or device memory; time[n]: host.
 * Outputs (host, each nullable): keyframe_id[n] (-1 = not a keyframe), *n_selected, T_s2m[n][16] row-major
 * after each frame, node[n][26] of which the first *n_selected rows are written, one per keyframe in
 * order: time, id, cur_position_[3], prev_position_[3], cur_rotation_[9], prev_rotation_[9], the
 * rotations row-major (FactorGraphNode, src/keyframe.h:115-121).  n == 0 is a no-op (*n_selected = 0). */
int lislam_keysel_step(lislam_keysel* s, const double* T_s2s, const int32_t* good, const double* time, int32_t n,
                       int32_t* keyframe_id, int32_t* n_selected, double* T_s2m, double* node);
/* The same for scans [first_scan, first_scan + n_scans) of a batch: each scan's LISLAM_OUT_ORB_T row and
 * its LISLAM_OUT_ORB_STATS[0] (good means == 1) are read where they lie on the device, after a pending
 * device-decided cascade has settled.  LISLAM_ERR_STATE unless lislam_batch_intensity_odometry has run
 * over those scans; the other error codes as lislam_place_add_batch. */
int lislam_keysel_step_batch(lislam_keysel* s, lislam_batch* b, int32_t first_scan, int32_t n_scans, const double* time,
                             int32_t* keyframe_id, int32_t* n_selected, double* T_s2m, double* node);
/* Each nullable: the keyframes selected so far, T_s2m (row-major 4x4), the last keyframe's time (NaN
 * before the first). */
int lislam_keysel_state(lislam_keysel* s, int32_t* n_keyframes, double* T_s2m16, double* last_time);

/* HIP-event timing of the mapping kernels of a context (recorded on its stream, no host sync
 * while recording).  lislam_map_kernel_times synchronizes, returns the total ms and launch count
 * per kernel since the previous read (arrays of LISLAM_MAP_NUM_KERNELS, in the order below) and
 * clears the record. */
#define LISLAM_MAP_NUM_KERNELS 25 /* k_knn, k_fit, k_lm_eval, k_lm_step, map rebuild (keys + sort +
                                     gather + cell table), Add_Points downsample (claim + resolve),
                                     k_orb_pyramid, k_orb_fast, k_orb_select, k_orb_finish,
                                     k_orb_blur (the padded-level blur of images too large for
                                     k_orb_pyramid), k_orb_desc, k_orb_match, k_orb_lm,
                                     k_ground_screen, k_ground_ransac, k_ground_extract,
                                     k_lc_step, k_lc_apply, k_fuse, k_orb_roiblur (the ROI blur +
                                     border rows after k_orb_pyramid), k_lm_solve (a whole pose
                                     solve in one launch; k_lm_eval / k_lm_step are no longer
                                     launched), k_mw_match, k_mw_select, k_mw_gate (the sliding
                                     window's L2 match, selection and gate) */
int lislam_map_set_timing(lislam_ctx* ctx, int32_t enable);
int lislam_map_kernel_times(lislam_ctx* ctx, float* ms, int32_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* LISLAM_H_ */
