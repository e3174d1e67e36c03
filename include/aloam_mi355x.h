/* include/aloam_mi355x.h — C ABI of libaloam_mi355x.so: the MI355X (gfx950) drop-in for A-LOAM's hot path.
 *
 * The reference (HKUST-Aerial-Robotics/A-LOAM) has no plugin / FFI interface: each stage is a ROS node whose
 * per-scan work sits in one function body over file-scope globals.  This ABI cuts exactly at those bodies
 * (SURVEY.md §8(b) "B2 in-process function seams"); every entry point below names the reference code it
 * replaces.  A ROS node keeps its subscribe / sync / publish code and calls these instead of PCL + Ceres
 * (INTEGRATION.md shows the ~50-line change per node).
 *
 * Conventions
 *   - plain C, no exceptions across the boundary; return 0 = ok, negative = error (aloam_last_error()).
 *   - one aloam_ctx = `batch` independent sequences advanced in lock-step on ONE device and ONE HIP stream (any of them may sit a step out or
 *     restart in place: aloam_set_active, aloam_reset_sequences)
 *     (batch = 1 is the reference's single-sensor node).  A context is not thread-safe; distinct contexts
 *     are independent (one per GPU / per process for multi-GPU; no collectives — sequences never exchange data).
 *     Every call runs on the context's device and restores the calling thread's current HIP device before returning.
 *   - points are 16-byte records {float x, y, z, w}; w = `intensity` of pcl::PointXYZI
 *     (reference include/aloam_velodyne/common.h:43).  Input records may use any stride >= 16 bytes that is a multiple of 4
 *     (16 = KITTI .bin, 32 = the PointCloud2 point_step pcl::toROSMsg<PointXYZI> produces, reference src/kittiHelper.cpp:153-154),
 *     or stride 12 = {x, y, z} only: scan registration never reads the 4th float of its input (it overwrites intensity with
 *     scanID + relTime, reference src/scanRegistration.cpp:132-133,239), so a driver may leave it off the wire (a quarter less
 *     PCIe traffic for the host-fed entries).  Not with ring_from_field, which IS the 4th float.
 *   - quaternions are (x, y, z, w) like para_q (reference src/laserOdometry.cpp:96-100).
 *   - there is NO CPU fallback: every entry point fails with ALOAM_E_HIP if the HIP runtime / a gfx950 device
 *     is unavailable.
 */
#ifndef ALOAM_MI355X_H_
#define ALOAM_MI355X_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct aloam_ctx aloam_ctx;

enum {
  ALOAM_OK = 0,
  ALOAM_E_ARG = -1,        /* bad argument */
  ALOAM_E_SCAN_LINES = -2, /* n_scans not 16/32/64 without ring_from_field (reference src/scanRegistration.cpp:472-476) */
  ALOAM_E_EMPTY = -3,      /* no point of some scan survives the NaN / minimum-range filter */
  ALOAM_E_CAPACITY = -4,   /* a scan exceeds max_points, a ring exceeds max_ring_points, or (mapping) the map pool / voxel scratch was too small
                              in some step since the last aloam_synchronize: the steps have still run, the points that did not fit are
                              missing from the map */
  ALOAM_E_HIP = -5,        /* HIP runtime error / no device / internal device-side time-out */
  ALOAM_E_STATE = -6       /* call order (e.g. odometry before any registration) */
};

/* Launch-file parameters (reference launch/aloam_velodyne_HDL_64.launch:3-13) + sizing of the device buffers. */
typedef struct aloam_config {
  int n_scans;             /* `scan_line`   : 16 / 32 / 64 (reference src/scanRegistration.cpp:466)                       */
  float min_range;         /* `minimum_range` (reference src/scanRegistration.cpp:468): 0.3 VLP-16/HDL-32, 5 HDL-64          */
  int ring_from_field;     /* 0: ring from the elevation formulas (src/scanRegistration.cpp:166-205); 1: ring = int(w)     */
  int batch;               /* independent sequences processed per call                                                      */
  int max_points;          /* capacity per scan; the reference's global arrays hold 400000 (src/scanRegistration.cpp:66-69) */
  int max_ring_points;     /* capacity per ring: 2059 or 4107 (LDS sizing of the per-ring selection kernel)                 */
  int device;              /* HIP device ordinal                                                                            */
  int lm_max_iterations;   /* options.max_num_iterations = 4 (reference src/laserOdometry.cpp:496)                          */
  int outer_iterations;    /* opti_counter loop = 2 (reference src/laserOdometry.cpp:278)                                   */
  int distortion;          /* 0 = #define DISTORTION 0 (reference src/laserOdometry.cpp:59, the shipped setting); 1: every point is
                              moved / constrained with its own interpolation ratio s = (intensity - int(intensity)) / SCAN_PERIOD
                              (src/laserOdometry.cpp:115-116,376-377,474-475; src/lidarFactor.hpp:29-30,81-82)              */
} aloam_config;

/* Which cloud of a sequence (topic names of reference src/scanRegistration.cpp:480-488, src/laserOdometry.cpp:205-209). */
enum {
  ALOAM_CLOUD_FULL = 0,        /* /velodyne_cloud_2        ring-ordered laserCloud (src/scanRegistration.cpp:246-252).  The device keeps one slab per
                                  ring; the dense ring-by-ring cloud is assembled when this id is first asked for after a registration  */
  ALOAM_CLOUD_SHARP = 1,       /* /laser_cloud_sharp                                              */
  ALOAM_CLOUD_LESS_SHARP = 2,  /* /laser_cloud_less_sharp                                         */
  ALOAM_CLOUD_FLAT = 3,        /* /laser_cloud_flat                                               */
  ALOAM_CLOUD_LESS_FLAT = 4,   /* /laser_cloud_less_flat                                          */
  ALOAM_CLOUD_CORNER_LAST = 5, /* /laser_cloud_corner_last (laserCloudCornerLast after the swap)  */
  ALOAM_CLOUD_SURF_LAST = 6    /* /laser_cloud_surf_last   (laserCloudSurfLast after the swap)    */
};

typedef struct aloam_odom_stats {
  int corner_corr[2];      /* corner_correspondence (reference src/laserOdometry.cpp:382): [0] first outer iteration, [1] second — or the last one when outer_iterations > 2 */
  int plane_corr[2];       /* plane_correspondence  per outer iteration (reference src/laserOdometry.cpp:480) */
  int lm_iterations[2];    /* LM iterations executed per ceres::Solve stand-in                                 */
  int lm_successful[2];
  double initial_cost[2];
  double final_cost[2];
  int termination[2];      /* 0 max-iter, 1 parameter tol, 2 function tol, 3 gradient tol, 4 no residuals, 5 failure, 6 minimum trust-region radius (Ceres: CONVERGENCE) */
} aloam_odom_stats;

/* ---- lifetime -------------------------------------------------------------------------------------------- */
void aloam_default_config(aloam_config* cfg);                       /* HDL-64 launch values, batch 1           */
int aloam_create(const aloam_config* cfg, aloam_ctx** out);          /* replaces the nodes' global state (src/scanRegistration.cpp:60-83, src/laserOdometry.cpp:59-108) */
/* The reference runs its three stages as three processes; a node that hosts one stage only needs that stage's device buffers.
 * `stages` = any combination of ALOAM_STAGE_*; entry points of a stage that was left out fail with ALOAM_E_STATE.
 * aloam_create == aloam_create_stages(cfg, ALOAM_STAGE_ALL, out). */
enum { ALOAM_STAGE_REGISTRATION = 1, ALOAM_STAGE_ODOMETRY = 2, ALOAM_STAGE_MAPPING = 4, ALOAM_STAGE_ALL = 7 };
int aloam_create_stages(const aloam_config* cfg, int stages, aloam_ctx** out);
void aloam_destroy(aloam_ctx* ctx);
const char* aloam_last_error(const aloam_ctx* ctx);                  /* replaces printf / ROS_BREAK diagnostics */
void* aloam_stream(aloam_ctx* ctx);                                  /* the hipStream_t all work is queued on   */
int aloam_synchronize(aloam_ctx* ctx);                               /* waits + surfaces device-side error flags */
/* pcl::VoxelGrid (src/scanRegistration.cpp:402-405, src/laserMapping.cpp:543-549,793-799) sums the members of a voxel in the order an UNSTABLE
 * std::sort leaves its index vector in.  ALOAM_SUM_INPUT_ORDER (default, the throughput path) sums them in input order: centroids of three or more
 * points may differ from the reference's in their last bits (<= 4 ulp), nothing else does.  ALOAM_SUM_REFERENCE_ORDER replays libstdc++'s introsort
 * on the device (one workgroup per filter call) and sums in the order it produces: the reference's bits, about 4x slower (registration + odometry; more with mapping at large batches) -
 * a validation mode for comparing long free-running sequences with the reference's own output.  Takes effect from the next call; not to be changed mid-sequence. */
enum { ALOAM_SUM_INPUT_ORDER = 0, ALOAM_SUM_REFERENCE_ORDER = 1 };
int aloam_set_voxel_sum_order(aloam_ctx* ctx, int order);

/* ---- stage 1: body of laserCloudHandler (reference src/scanRegistration.cpp:127-411) ----------------------- */
/* Host input: scans[b] points to n_in[b] records of stride_bytes.  Blocking w.r.t. the host buffers only.    */
int aloam_scan_register(aloam_ctx* ctx, const void* const* scans, const int* n_in, int stride_bytes);
/* Device-resident input: sequence b starts at d_scans + b * seq_stride_bytes.  Fully asynchronous.           */
int aloam_scan_register_device(aloam_ctx* ctx, const void* d_scans, long long seq_stride_bytes, const int* n_in, int stride_bytes);

/* Host-resident batch in ONE buffer (sequence b at h_scans + b * seq_stride_bytes, n_in[b] * stride_bytes readable bytes each;
 * rows 0 .. batch-2 are copied with the batch-wide maximum length, which stays inside the buffer because another row follows):
 * what a driver thread that receives the
 * sensor messages (reference src/scanRegistration.cpp:114-133) hands over.  One batched H2D copy per call on a dedicated copy
 * stream into one of two device slabs, so the copy of call k + 1 runs under the kernels of call k; asynchronous when the buffer is
 * pinned (hipHostMalloc / hipHostRegister).  The buffer must stay unmodified until aloam_input_consumed() or aloam_synchronize(). */
int aloam_scan_register_host(aloam_ctx* ctx, const void* h_scans, long long seq_stride_bytes, const int* n_in, int stride_bytes);
int aloam_input_consumed(aloam_ctx* ctx);                            /* waits until every host buffer handed over so far has been copied and read */

/* ---- stage 2: odometry main-loop body (reference src/laserOdometry.cpp:265-506,554-568) -------------------- */
int aloam_odometry_step(aloam_ctx* ctx);                             /* asynchronous; all sequences             */

/* ---- throughput entry: stage 1 + stage 2 for one sweep of every sequence, asynchronous -------------------- */
int aloam_process_device(aloam_ctx* ctx, const void* d_scans, long long seq_stride_bytes, const int* n_in, int stride_bytes);

int aloam_process_host(aloam_ctx* ctx, const void* h_scans, long long seq_stride_bytes, const int* n_in, int stride_bytes);   /* same from a host buffer (see aloam_scan_register_host) */

/* ---- stage 1 from 16-bit range images ----------------------------------------------------------------------------------------
 * A spinning LiDAR produces a 16-bit range per laser and firing and a 16-bit azimuth per firing; a driver inflates that to 12 - 16 bytes per point
 * before laserCloudHandler sees it (reference src/scanRegistration.cpp:127-133).  These entries take the sensor's own numbers, 2 bytes per point, and
 * decode them in the front-end kernels: a sixth to an eighth of the PCIe bytes of the host-fed path.
 *
 * aloam_range_decoder describes the sensor: set once per context (the tables are copied to the device; the call waits for the stream).
 *
 * A sweep of n_cols columns is one blob per sequence:
 *     uint16 az[(n_cols + 7) & ~7]      azimuth code of every column (the padding makes the ranges start 16-byte aligned)
 *     uint16 range[n_cols * rows]       in the decoder's order
 * Point i of the sweep, every operation in f32 and rounded on its own:
 *     (col, row) = COLUMN_MAJOR: (i / rows, i % rows);  ROW_MAJOR: (i % n_cols, i / n_cols)
 *     code = range[i];   a = (az[col] + az_off[row]) mod n_az                       (into 0 .. n_az-1)
 *     rho  = (float)code * range_scale + range_off[row]
 *     rxy  = rho * cos_el[row]
 *     x = rxy * az_x[a];   y = rxy * az_y[a];   z = rho * sin_el[row] + z_off[row];   w = (float)ring_id[row]
 * code == 0 (no return) or az[col] >= n_az gives (NaN, NaN, NaN): the NaN filter removes it, as removeNaNFromPointCloud would
 * (src/scanRegistration.cpp:136).  The decoded sweep, no-return cells included and in storage order, IS the input of laserCloudHandler: everything
 * downstream evaluates the reference's expressions on that f32 point, and the ring is (int)w under the ring_from_field rule (outside 0 .. n_scans-1:
 * rejected; such a point still counts for the first / last kept point).  The reference's elevation formulas (:166-205) are not evaluated and
 * aloam_config.ring_from_field plays no part.  There is no trigonometry on the device: the caller's az_x / az_y fix the axis convention. */
enum { ALOAM_RANGE_COLUMN_MAJOR = 0,   /* firing order: point i = column i / rows, row i % rows                       */
       ALOAM_RANGE_ROW_MAJOR = 1 };    /* ring-major (KITTI-like): point i = row i / n_cols, column i % n_cols        */
typedef struct aloam_range_decoder {
  int rows;                /* lasers per column, 1 .. 128                                                                        */
  int n_az;                /* azimuth codes per turn, 1 .. 65536 (Velodyne: 36000)                                               */
  int order;               /* ALOAM_RANGE_COLUMN_MAJOR / ALOAM_RANGE_ROW_MAJOR                                                   */
  float range_scale;       /* metres per range code                                                                              */
  const float* az_x;       /* [n_az] cosine of the azimuth of every code, in the caller's axis convention                        */
  const float* az_y;       /* [n_az] sine                                                                                        */
  const float* cos_el;     /* [rows] cosine of every laser's elevation                                                           */
  const float* sin_el;     /* [rows] sine                                                                                        */
  const float* range_off;  /* [rows] metres added to the scaled range                                                            */
  const float* z_off;      /* [rows] metres added to z (vertical offset of the laser)                                            */
  const int* az_off;       /* [rows] azimuth codes added to the column's, |az_off| < n_az: the per-laser rotational correction   */
  const int* ring_id;      /* [rows] the reference's scanID of every laser, 0 .. n_scans-1, or -1: the row is rejected (how a caller
                              reproduces the scanID > 50 cut of src/scanRegistration.cpp:198 on HDL-64)                          */
} aloam_range_decoder;
/* ALOAM_E_ARG on any bad field (aloam_last_error names it), nothing is changed then.  May be called again with another decoder. */
int aloam_set_range_decoder(aloam_ctx* ctx, const aloam_range_decoder* decoder);
/* The four entries of stage 1 / the throughput path for range images: sequence b's blob at base + b * seq_stride_bytes holds n_cols[b] columns.
 * n_cols[b] * rows > max_points: ALOAM_E_CAPACITY; a negative count: ALOAM_E_ARG; before aloam_set_range_decoder: ALOAM_E_STATE - each before
 * anything is queued.  Device blobs must be 2-byte aligned with an even seq_stride_bytes.  The host forms go through the same two staging slabs, copy
 * stream and events as aloam_scan_register_host (aloam_input_consumed works unchanged; rows 0 .. batch-2 are copied with the batch-wide largest blob
 * length), and a context may alternate between float records and range images from one sweep to the next. */
int aloam_scan_register_range_device(aloam_ctx* ctx, const void* d_sweeps, long long seq_stride_bytes, const int* n_cols);
int aloam_scan_register_range_host(aloam_ctx* ctx, const void* h_sweeps, long long seq_stride_bytes, const int* n_cols);
int aloam_process_range_device(aloam_ctx* ctx, const void* d_sweeps, long long seq_stride_bytes, const int* n_cols);   /* + aloam_odometry_step */
int aloam_process_range_host(aloam_ctx* ctx, const void* h_sweeps, long long seq_stride_bytes, const int* n_cols);     /* + aloam_odometry_step */

/* ---- stage 3: scan-to-map refinement, body of process() (reference src/laserMapping.cpp:231-893), no frame dropping ---- */
/* Replaces the node's globals (cube arrays laserCloudCornerArray / SurfArray[4851], q_wmap_wodom, t_wmap_wodom, `parameters`,
 * laserCloudCen*; src/laserMapping.cpp:72-116) and reads the launch parameters mapping_line_resolution / mapping_plane_resolution
 * (:898-905).  pool_points = capacity of the device-resident map per sequence and feature class.  Call once, before the first step. */
/* pool_points is where the map STARTS: the reference's cubes are std::vectors that grow as long as the sensor travels
 * (src/laserMapping.cpp:737-783), so the pools (one per sequence and class; cubes grow by doubling inside it, the pool is compacted when
 * fragmented; one cube may hold up to the whole pool) are doubled - between steps, contents moved, at aloam_mapping_step - whenever the
 * live points plus what the queued steps can add would no longer fit, up to aloam_mapping_set_pool_limit (default 2^26 points, or
 * whatever the device memory holds).  Only at that ceiling do points get dropped: such frames are counted on the device and the first
 * aloam_synchronize after one returns ALOAM_E_CAPACITY once (however many asynchronous steps were queued in between), then ALOAM_OK
 * again until it happens anew. */
int aloam_mapping_enable(aloam_ctx* ctx, float mapping_line_resolution, float mapping_plane_resolution, int pool_points);
int aloam_mapping_set_pool_limit(aloam_ctx* ctx, int max_pool_points);   /* ceiling of the pool growth, per sequence and class; before or after enable */
/* out: current pool_points, growths so far, the limit, live points of the fullest (sequence, class) pool after the last finished step */
int aloam_get_map_pool_info(aloam_ctx* ctx, int out[4]);
/* One frame for every sequence, asynchronous.  Consumes what the odometry node publishes for the frame — /laser_cloud_corner_last,
 * /laser_cloud_surf_last, /velodyne_cloud_3, /laser_odom_to_init (src/laserOdometry.cpp:508-591) — straight from the context
 * (call after aloam_odometry_step / aloam_process_device), or as injected through aloam_set_last / aloam_set_full_cloud / aloam_set_state. */
int aloam_mapping_step(aloam_ctx* ctx);
int aloam_set_full_cloud(aloam_ctx* ctx, int seq, const float* cloud_xyzw, int n);          /* /velodyne_cloud_3 (src/laserMapping.cpp:189-194) */
/* State injection, mapping node: laserCloudCornerArray / SurfArray (feature_class 0 / 1) of one sequence replaced by n_cubes cubes
 * (window indices i + 21 j + 441 k as src/laserMapping.cpp:527, their populations, their points back to back), and
 * laserCloudCenWidth / Height / Depth, q_wmap_wodom, t_wmap_wodom, frameCount (src/laserMapping.cpp:72-74,84-91,115-116). */
int aloam_set_map(aloam_ctx* ctx, int seq, int feature_class, const int* cube_ids, const int* counts, int n_cubes, const float* points_xyzw);
int aloam_set_map_frame(aloam_ctx* ctx, int seq, const int cen[3], const double q_wmap_wodom[4], const double t_wmap_wodom[3], int frame_count);
/* /aft_mapped_to_init pose = q_w_curr, t_w_curr (src/laserMapping.cpp:851-863) and the map<-odom correction (:148-152) */
int aloam_get_map_pose(aloam_ctx* ctx, int seq, double q_w_curr[4], double t_w_curr[3], double q_wmap_wodom[4], double t_wmap_wodom[3]);
/* laserCloudCenWidth/Height/Depth, frameCount, submap sizes (corner, surf), stack sizes (corner, surf), factors per iteration
 * (corner[2], surf[2]), LM iterations[2], termination of the first solve, pool compactions so far */
int aloam_get_map_info(aloam_ctx* ctx, int seq, int out[16]);
int aloam_map_cube_counts(aloam_ctx* ctx, int seq, int feature_class, int* out_4851);      /* points per cube of the 21 x 21 x 11 window */
int aloam_get_map_cube(aloam_ctx* ctx, int seq, int feature_class, int cube, float* out_xyzw, int cap_points);   /* laserCloud*Array[cube] */
enum { ALOAM_MAP_REGISTERED = 2, ALOAM_MAP_CORNER_STACK = 3, ALOAM_MAP_SURF_STACK = 4 };    /* /velodyne_cloud_registered (:836-846); laserCloud*Stack (:542-550) */
/* ALOAM_MAP_SURROUND: /laser_cloud_surround = laserCloudSurround (src/laserMapping.cpp:803-821): for every cube of the last step's 5 x 5 x 3
 * window in the i, j, k order of :512-529, its corner cube then its surf cube, as they are after the step's insert and re-filter; empty
 * before a sequence's first mapping step.  ALOAM_MAP_FULL: /laser_cloud_map = laserCloudMap (:823-834): all 4851 cubes in index order,
 * corner then surf for each.  Both are assembled on the device by the same kernels as aloam_export_clouds. */
enum { ALOAM_MAP_SURROUND = 5, ALOAM_MAP_FULL = 6 };
/* REGISTERED, CORNER_STACK, SURF_STACK, SURROUND or FULL of one sequence.  Returns the point count; out_xyzw may be NULL when cap_points is 0. */
int aloam_get_map_cloud(aloam_ctx* ctx, int seq, int which, float* out_xyzw, int cap_points);

/* ---- results (each synchronises the stream) ---------------------------------------------------------------- */
int aloam_cloud_size(aloam_ctx* ctx, int seq, int which);            /* replaces cloud.points.size()            */
int aloam_get_cloud(aloam_ctx* ctx, int seq, int which, float* out_xyzw, int cap_points);  /* what pcl::toROSMsg publishes (src/scanRegistration.cpp:413-441, src/laserOdometry.cpp:574-590) */
int aloam_get_pose(aloam_ctx* ctx, int seq, double q_w_curr[4], double t_w_curr[3], double q_last_curr[4], double t_last_curr[3]); /* /laser_odom_to_init (src/laserOdometry.cpp:511-522) + para_q / para_t */
int aloam_get_odom_stats(aloam_ctx* ctx, int seq, aloam_odom_stats* out);

/* ---- batched export: what the nodes publish, for every sequence, in one asynchronous call ------------------------------
 * Replaces the publishers of the three nodes read one sequence at a time: /laser_odom_to_init (src/laserOdometry.cpp:511-522), the cloud
 * topics (src/scanRegistration.cpp:413-441, src/laserOdometry.cpp:574-590), /aft_mapped_to_init (src/laserMapping.cpp:851-863),
 * /laser_cloud_surround, /laser_cloud_map and /velodyne_cloud_registered (src/laserMapping.cpp:803-846).
 *
 * Both calls are queued on the context's stream and return without waiting for the device: they make no host synchronisation and read
 * nothing back.  They write the state at that point of the stream (a step queued after them does not change what they write); the caller
 * waits with aloam_synchronize or an event on aloam_stream.  Every value has exactly the bits the matching getter returns after a
 * synchronise, sequences that sat out the last step and clouds injected through aloam_set_* included.
 *
 * Destinations: device memory of the context's device, or pinned host memory (hipHostMalloc, hipHostRegister; the kernels write through
 * its device mapping).  Every pointer is classified before anything is queued: pageable host memory, another device's memory and NULL are
 * refused with ALOAM_E_ARG (a kernel store to pageable memory would fault the device).  dst_xyzw must be 16-byte aligned; it may be NULL
 * when cap_points is 0. */
typedef struct aloam_pose_record {            /* one per sequence; 240 bytes                                                           */
  double q_w[4], t_w[3];                      /* /laser_odom_to_init          = aloam_get_pose q_w_curr / t_w_curr                      */
  double q_last_curr[4], t_last_curr[3];      /* para_q / para_t              = aloam_get_pose                                          */
  double map_q_w[4], map_t_w[3];              /* /aft_mapped_to_init          = aloam_get_map_pose (zeros without mapping)              */
  double q_wmap_wodom[4], t_wmap_wodom[3];    /* map <- odom correction       = aloam_get_map_pose (zeros without mapping)              */
  int inited;                                 /* systemInited of the sequence (src/laserOdometry.cpp:69,267-271)                        */
  int map_frames;                             /* frameCount of the mapping node (src/laserMapping.cpp:115); -1 without mapping          */
  int pad[2];
} aloam_pose_record;

/* Cloud ids of aloam_export_clouds: an ALOAM_CLOUD_* value, or ALOAM_EXPORT_MAP + one of ALOAM_MAP_REGISTERED .. ALOAM_MAP_FULL. */
enum { ALOAM_EXPORT_MAP = 16, ALOAM_EXPORT_MAX_IDS = 12 };

int aloam_export_poses(aloam_ctx* ctx, aloam_pose_record* dst);   /* dst[batch] */
/* Segment (i, b) = cloud ids[i] of sequence b, packed at [dst_offsets[i * batch + b], dst_offsets[i * batch + b + 1]) in points of 16 bytes;
 * dst_offsets[n_ids * batch] is the total.  The device writes dst_offsets (n_ids * batch + 1 values) always, and a segment's points only
 * when the segment ends at or before cap_points: nothing is ever written past cap_points, cap_points = 0 is the size query, and an overflow
 * is no error (compare the total with the capacity).  0 <= n_ids <= ALOAM_EXPORT_MAX_IDS; unknown or repeated ids: ALOAM_E_ARG; a map id
 * without aloam_mapping_enable, or a cloud this context holds no buffer for (aloam_create_stages): ALOAM_E_STATE.  `ids` is read during
 * the call only.  The full cloud (ALOAM_CLOUD_FULL) is made from the ring slabs first if no consumer has asked for it since the last
 * registration, as aloam_get_cloud does. */
int aloam_export_clouds(aloam_ctx* ctx, const int* ids, int n_ids, float* dst_xyzw, long long cap_points, long long* dst_offsets);

/* ---- teacher forcing / state injection (what the topic hand-over between the nodes allows) ----------------- */
int aloam_set_features(aloam_ctx* ctx, int seq, const float* sharp, int n_sharp, const float* less_sharp, int n_less_sharp,
                       const float* flat, int n_flat, const float* less_flat, int n_less_flat);   /* the 4 feature topics (src/laserOdometry.cpp:243-258) */
int aloam_set_last(aloam_ctx* ctx, int seq, const float* corner_last, int n_corner, const float* surf_last, int n_surf); /* laserCloudCornerLast / SurfLast + kd-tree input (src/laserOdometry.cpp:554-568) */
int aloam_set_state(aloam_ctx* ctx, int seq, const double para_q[4], const double para_t[3], const double q_w_curr[4],
                    const double t_w_curr[3]);                       /* src/laserOdometry.cpp:93-98              */
int aloam_set_system_inited(aloam_ctx* ctx, int inited);             /* systemInited (src/laserOdometry.cpp:69,267-271), of every sequence */

/* ---- per-sequence lifecycle: sequences that sit out steps, and restart in place --------------------------------------
 * Every sequence of a batch has its own lifecycle: its own systemInited flag and its own laserCloudCornerLast / SurfLast buffer
 * (the swap of src/laserOdometry.cpp:554-563 is per sequence).
 *
 * aloam_set_active: which sequences take part in the calls that follow; active[b] != 0 for each of the `batch` sequences, NULL = all
 * (the default).  Each registration, odometry and mapping call uses the mask in force when it is made.  No synchronisation: the mask
 * is staged through a pinned ring, like the point counts.
 *   - In a context with both stages, the mask may not change between a registration and the odometry step that consumes it:
 *     ALOAM_E_STATE, and the mask in force stays as it was.
 *   - The mapping step may use another mask than the odometry step of the same frame: a sequence idle in mapping has dropped that frame
 *     in mapping, as the reference's mapping node drops frames when it falls behind (src/laserMapping.cpp:299-303).
 *   - An idle sequence is neither read nor written by that call: input, features, dense cloud, curvature and labels, odometry state and
 *     statistics, correspondences, last clouds, map pose, cubes and pool contents, registered cloud.  Every getter returns the same bits
 *     before and after an idle step.  Its n_in row must still be in 0 .. max_points; its points are never read (NaN / garbage is fine).
 *   - An ACTIVE sequence with no surviving point still fails with ALOAM_E_EMPTY.  An all-idle step is legal and changes nothing.
 *   - An active sequence that is not initialised (new context, aloam_reset_sequences, aloam_set_system_inited(0)) has a first frame
 *     in its next odometry step: no solve, only the swap (src/laserOdometry.cpp:267-271), while the others solve.
 *
 * aloam_reset_sequences: the n listed sequences become exactly what a freshly created context holds, with its mapping configuration and
 * pool limit kept: identity poses, not initialised, no last clouds, no correspondences; with mapping enabled an empty map (its pool space
 * released), cen = (10, 10, 5), identity q_wmap_wodom, frame_count 0, error / compaction counters zero.  Queued on the stream with no
 * host synchronisation (valid between asynchronous steps and with the graph-replayed odometry step).  Out-of-range or repeated ids:
 * ALOAM_E_ARG, nothing is reset.  The other sequences are not touched.
 */
int aloam_set_active(aloam_ctx* ctx, const int* active);
int aloam_reset_sequences(aloam_ctx* ctx, const int* seqs, int n);

/* ---- localization against a frozen prior map --------------------------------------------------------------------------------
 * aloam_set_map_frozen: which sequences localize against their map instead of extending it, in the mapping steps that follow.
 * frozen[b] != 0 for each of the `batch` sequences; NULL = none (the default).
 *   - A frozen, active sequence's mapping step does everything up to and including the pose: transformAssociateToMap
 *     (src/laserMapping.cpp:142-146, called at :309), the centre cube and window shifts (:311-507; the slab that falls off is emptied, as in
 *     a normal step), the valid cubes and submap (:509-539), the stack voxel filters (:542-550), the 5-NN search, line and plane fits and
 *     the solve (:554-733), transformUpdate (:148-152, called at :734), /velodyne_cloud_registered (:836-846) and frameCount++ (:888).  It
 *     skips the insertion (:737-783) and the per-cube re-filter (:788-801).
 *   - Its map afterwards: every cube holds the same points, in the same order and with the same bits; the cube table has only moved by
 *     the shift permutation of that step.  pool_used does not change and no compaction runs.  ALOAM_MAP_SURROUND and ALOAM_MAP_FULL show
 *     that unchanged map.
 *   - Pose bits: the pose, statistics and registered cloud of a frozen step are bit-identical to what a normal step computes from the same
 *     state (in the reference the solve comes before the insert).  The submap search grid of a frozen sequence is rebuilt only when its
 *     submap changes (the sensor entered another 50 m cube, or the map / frame was replaced), with the same results.
 *   - The mask behaves like the active mask: host state staged per call, no synchronisation; each mapping step uses the mask in force when
 *     it is queued; independent of aloam_set_active (an idle sequence is idle, frozen or not); not changed by aloam_reset_sequences or
 *     aloam_load_sequences; not part of a sequence record (ALOAM_SEQ_RECORD_VERSION, MapSeq and aloam_pose_record are unchanged).
 *   - A step whose active sequences are all frozen adds nothing to any map: it never grows the map pools nor waits for the device to size them.
 *   - The initial guess in the map frame is set with aloam_set_map_frame (q_wmap_wodom, t_wmap_wodom: map <- odometry); the factor counts
 *     of aloam_get_map_info (corner / surf factors per iteration) are the per-sequence localization score, e.g. to rank several guesses of
 *     one map loaded into several slots.
 *   - ALOAM_E_STATE in a context without ALOAM_STAGE_MAPPING or before aloam_mapping_enable; argument errors as for aloam_set_active. */
int aloam_set_map_frozen(aloam_ctx* ctx, const int* frozen);

/* ---- scoring and applying batches of map-pose hypotheses ---------------------------------------------------------------------
 * A frozen mapping step refines a guess that is already close (about 1 m and 2.5 deg of yaw).  A coarser guess is searched:
 * many candidate corrections (map <- odometry, as aloam_set_map_frame takes them) are scored against the state one frozen step has left on
 * the device, the best one is installed, and the next frozen steps refine it.  No step, no map copy and no slot per hypothesis.
 *
 * aloam_score_map_corrections: for each listed sequence seqs[i] and each candidate cand[c], scores[i * K + c] :=
 *   - What a score is.  The state the sequence's last mapping step left is read: its laserCloudCornerStack / SurfStack
 *     (ALOAM_MAP_CORNER_STACK / ALOAM_MAP_SURF_STACK), the odometry pose that step started from, and the search grid of its submap.  The
 *     start pose is transformAssociateToMap (src/laserMapping.cpp:142-146) with the candidate in place of the sequence's correction; then
 *     every stack point goes through the first data association of a mapping step (:554-687: pointAssociateToMap, the five nearest
 *     submap points, the line fit and the plane fit with their tests), and every factor's residual is evaluated once at the start pose
 *     (src/lidarFactor.hpp:36-51, :116-123, under HuberLoss(0.1) as :565).  Nothing of the sequence is written.
 *   - Exactness.  corner_factors / surf_factors equal, as integers, the corner / surf factors of iteration 0 that aloam_get_map_info
 *     reports after a frozen mapping step of the same frame started from aloam_set_map_frame(same cen, cand, same frame_count), whenever
 *     that step keeps the same window (same cen and centre cube afterwards): the same device functions run in the same order.  A
 *     candidate that moves the sensor into another 50 m cube is still scored, against the submap that is there (the window of the last
 *     step), not the one a step from that candidate would select.
 *   - Which sequences.  Each listed sequence must have been active AND frozen in its last mapping step, with nothing since that
 *     invalidates its search grid: a mapping step in which it grew its map, aloam_reset_sequences, aloam_load_sequences, aloam_set_map,
 *     aloam_set_map_frame, a reallocation of the map pools (by any sequence).  All of these are host calls, so a per-sequence host flag
 *     decides without a synchronise: otherwise ALOAM_E_STATE and nothing is queued.  Steps the sequence sat out, odometry steps and
 *     aloam_apply_map_corrections keep it.  A sequence whose step failed the gate (submap of <= 10 corner or <= 50 surf points, :554)
 *     scores zeros.  seqs distinct and in range, n >= 0, K >= 1: else ALOAM_E_ARG.  ALOAM_E_STATE before aloam_mapping_enable.  Allowed
 *     between asynchronous steps; the active and frozen masks in force play no part.
 *   - Candidates are shared by all listed sequences (cand[K]); a host that wants another grid per sequence calls once per group of
 *     sequences.  Quaternions are used as given (not normalised), like aloam_set_map_frame's.
 *   - best[i] (may be NULL): the candidate with the most corner_factors + surf_factors; ties: the lower cost; ties: the lower index.
 *     A cost that is NaN (a non-finite candidate) ranks as +infinity.  n * K <= 2^18 pairs per call, else ALOAM_E_ARG (split the candidates).
 *   - Determinism.  Counts are integer sums.  cost is summed in a fixed order that depends on the stacks alone (per-workgroup partials in
 *     fixed slots, then one ordered pass; no floating-point atomics): two calls on the same state return the same bits, whatever n, K
 *     and the position of the candidate in cand.
 *
 * aloam_apply_map_corrections: for each listed sequence, q_wmap_wodom, t_wmap_wodom := cand[choice[i]], with choice read ON THE DEVICE
 * in stream order: the `best` of a scoring call queued before it can be passed straight in, with no synchronise in between.  Every getter
 * and aloam_export_poses then return the bits aloam_set_map_frame(current cen, that candidate, current frame_count) would give (that call
 * leaves q_w_curr / t_w_curr as the last step left them; so does this one), with one difference: aloam_set_map_frame synchronises and
 * invalidates the search grid, this call does neither - the window has not moved, the grid stays valid, and the next frozen step may reuse
 * it.  Any sequence may be listed (no frozen step is required).  A choice[i] outside 0 .. K-1 on the device leaves that sequence untouched
 * and is counted; the next aloam_synchronize returns ALOAM_E_ARG for it, once.
 *
 * Both calls are queued on the context's stream, make no host synchronisation and read nothing back (the first scoring call, and one
 * with a larger n * K than any before, allocates its scratch).  scores, best and choice: device memory of the context's device or pinned
 * host memory, classified before anything is queued as aloam_export_clouds classifies its destinations (pageable, managed, another
 * device's memory and NULL: ALOAM_E_ARG); 8- / 4-byte aligned.  cand: those two, or pageable host memory, which is staged with one copy
 * (it may be reused when the call returns; device and pinned candidates must stay unchanged until the call has run). */
typedef struct aloam_map_correction { double q_wmap_wodom[4], t_wmap_wodom[3], pad; } aloam_map_correction;   /* 64 bytes */
typedef struct aloam_map_score {                /* 32 bytes                                                                                  */
  int corner_factors, surf_factors;             /* factors the FIRST association of a frozen mapping step counts from this correction       */
  int corner_found, surf_found;                 /* stack points whose 5th neighbour is closer than 1 m (src/laserMapping.cpp:582,650)        */
  double cost;                                  /* sum over those factors of 0.5 * HuberLoss(0.1) of the squared residual, at the start pose */
  int pad[2];
} aloam_map_score;
int aloam_score_map_corrections(aloam_ctx* ctx, const int* seqs, int n, const aloam_map_correction* cand, int K,
                                aloam_map_score* scores /* [n][K] */, int* best /* [n], may be NULL */);
int aloam_apply_map_corrections(aloam_ctx* ctx, const int* seqs, int n, const aloam_map_correction* cand, int K, const int* choice /* [n] */);

/* ---- map tiles and the map spill: keeping the cubes that leave the window ------------------------------------------------------
 * A map is the 21 x 21 x 11 window of 50 m cubes around the sensor (src/laserMapping.cpp:72-80).  When the sensor comes within three
 * cubes of an edge the window shifts, and the slab that falls off is cleared and re-enters empty at the other side (:323-507): in the
 * reference, and in aloam_mapping_step, those points are gone.  The spill keeps them.  It changes nothing a mapping step computes: a
 * re-entered cube still starts empty; the cubes are only copied out before they are emptied.
 *
 * aloam_map_tile: one cube of one class with absolute coordinates.  cube[] is the window index (i, j, k) minus the window centre
 * (laserCloudCenWidth / Height / Depth) = int((t + 25) / 50), minus one when t + 25 < 0 (:312-321), of the coordinates of its points, so a
 * tile does not depend on the window it was cut from.  first_point indexes the array of 16-byte points (x, y, z, intensity) that goes with
 * a tile array.
 *
 * aloam_map_spill_enable: after aloam_mapping_enable, once.  Allocates, per sequence and class, a row of max_tiles tiles and a row of
 * max_points points, and counters.  From then on every aloam_mapping_step queues one more kernel in front of its first one: for every
 * ACTIVE sequence, growing or frozen, that computes the shift this step is about to make (the same arithmetic on the same state:
 * transformAssociateToMap :142-146, the centre cube :311-321, the shift loop) and, when there is one, appends every non-empty cube that the
 * shift empties to the sequence's rows as a tile: class 0 (corner) and class 1 (surf) rows apart, each in ascending window index
 * i + 21 j + 441 k, cube = index minus the centre BEFORE the step, frame = frameCount before the step, the points in the cube's order and
 * bits.  Idle sequences spill nothing.  A context that never calls this launches exactly what it launched before.
 *   - A tile is kept whole or not at all.  One that does not fit what is left of its rows is dropped and counted (later, smaller tiles
 *     of the same step are still kept); the next aloam_synchronize returns ALOAM_E_CAPACITY once, "map spill full".  Drain often enough.
 *   - aloam_reset_sequences and aloam_load_sequences do not touch a slot's spill: the host drains a slot before it reuses it.  The spill
 *     is not part of a sequence record (ALOAM_SEQ_RECORD_VERSION, MapSeq and aloam_pose_record are unchanged).
 *   - max_tiles in 1 .. 2^20, max_points in 1 .. 2^26: else ALOAM_E_ARG.  ALOAM_E_STATE before aloam_mapping_enable or when already enabled.
 *
 * aloam_export_map_spill: the drain.  Queued on the context's stream, no host synchronisation, nothing read back.  For the n listed
 * sequences (distinct, in range) the device always writes dst_offsets[0 .. n] (tiles) and dst_offsets[n + 1 .. 2 n + 1] (points):
 * sequence seqs[i]'s tiles - its corner row, then its surf row - go to tiles_dst[dst_offsets[i] .. dst_offsets[i + 1]) and their points to
 * points_dst[dst_offsets[n + 1 + i] .. dst_offsets[n + 2 + i]), with first_point rewritten to index points_dst.  A sequence's tiles and
 * points are written only when BOTH ranges end inside cap_tiles / cap_points; nothing is ever written past the caps, and caps of 0 are the
 * size query (tiles_dst / points_dst may then be NULL).  With clear != 0 the sequences that were written are emptied, in stream order; the
 * others keep their spill.  Destinations are classified like aloam_export_clouds': device memory of the context's device or pinned host
 * memory; pageable, managed, another device's memory and NULL are refused with ALOAM_E_ARG before anything is queued.
 *
 * aloam_get_map_spill_info (synchronises): out = tiles held (corner, surf), points held (corner, surf), tiles dropped so far, points
 * dropped so far, max_tiles, max_points. */
typedef struct aloam_map_tile {      /* 32 bytes */
  int cube[3];                       /* absolute cube (see above) */
  int feature_class;                 /* 0 corner, 1 surf */
  int count;                         /* points */
  int frame;                         /* frameCount of the sequence when the tile was cut; 0 for tiles of other origin */
  long long first_point;             /* index of its first point in the points array that goes with the tile array */
} aloam_map_tile;
int aloam_map_spill_enable(aloam_ctx* ctx, int max_tiles, int max_points);
int aloam_export_map_spill(aloam_ctx* ctx, const int* seqs, int n, aloam_map_tile* tiles_dst, long long cap_tiles, float* points_dst_xyzw,
                           long long cap_points, long long* dst_offsets /* [2][n + 1] */, int clear);
int aloam_get_map_spill_info(aloam_ctx* ctx, int seq, int out[8]);

/* ---- the atlas: a frozen sequence's window served from a map of any extent ----------------------------------------------------
 * One immutable tile store per context, shared by all its sequences.  A sequence attached to it localizes (aloam_set_map_frozen) in a
 * map larger than the 21 x 21 x 11 window: whenever its window is stale or about to shift (src/laserMapping.cpp:323-507), the window is
 * cut fresh from the atlas, so it never loses a cube and cubes more than a window away from where it started are there when it arrives.
 *
 * aloam_atlas_load: tiles[n_tiles] and the points[n_points] they index (what aloam_export_map_spill and a-loam_amd/atlas.py produce),
 * from pageable or pinned host memory or device memory of the context's device (managed / another device's memory: ALOAM_E_ARG).
 * Synchronous, like aloam_mapping_enable.  Every tile is validated before anything changes: class 0 / 1, count >= 0, its range inside
 * n_points, cube coordinates in -512 .. 511 (else ALOAM_E_ARG).  n_tiles = 0 unloads.  Replacing or unloading while a sequence is attached:
 * ALOAM_E_STATE.  ALOAM_E_STATE before aloam_mapping_enable.
 *   - Per class the points are packed and an open-addressing directory absolute cube -> (first, count) is built on the host (16-byte
 *     entries, load factor <= 1/2) and uploaded once.
 *   - Several tiles of one (cube, class) - a cube that left the window, was re-entered and left again, or two sessions - are concatenated
 *     in array order and filtered once with that class's pcl::VoxelGrid leaf (mapping_line_resolution / mapping_plane_resolution): what
 *     the per-cube re-filter (:788-801) would have made of them had they been one cube.  Always the input-order sum, whatever
 *     aloam_set_voxel_sum_order says.  A cube with one tile is taken as it is.  A concatenation larger than a map pool row grows the pools
 *     first, or is ALOAM_E_CAPACITY at the pool limit; nothing is truncated.  (The pools are grown before the new atlas is installed: when
 *     a later allocation of the load fails, the atlas stays as it was but the pools - contents kept - may already be larger.)
 *
 * aloam_atlas_attach: attached[b] != 0 for each of the `batch` sequences; NULL = none.  Host state staged per call like the frozen mask.
 * Attaching needs a loaded atlas (ALOAM_E_STATE) and grows the map pools until a row holds the largest window of the atlas
 * (ALOAM_E_CAPACITY above the pool limit, nothing changed).  Newly attached sequences are marked stale, in stream order; aloam_set_map,
 * aloam_set_map_frame, aloam_reset_sequences and aloam_load_sequences keep the attachment and mark the sequences they touch stale, so
 * aloam_set_map_frame(cen, guess, 0) is how a localization starts.  aloam_apply_map_corrections does not (the window has not moved).
 *   - An attached sequence that is active in a mapping step must be frozen: otherwise aloam_mapping_step returns ALOAM_E_STATE and queues
 *     nothing.
 *   - In such a step, before the window shifts would run: not stale and no shift - nothing happens.  Otherwise, for the centre the shift
 *     leads to, each of the 4851 cubes is looked up in the directory, the descriptors are packed back to back from the start of the pool
 *     row (as after aloam_load_sequences) and the points copied; cen becomes the new centre, pool_used the totals, the search grids are
 *     rebuilt.  The step itself then shifts nothing.  ALOAM_MAP_SURROUND / ALOAM_MAP_FULL, the getters, records, scoring and apply work on
 *     the window as they do without an atlas.  The map spill skips attached sequences (nothing is lost).
 *
 * aloam_atlas_info: out = tiles given; cubes (corner, surf) and points (corner, surf) after merging; extent of the bounding box in cubes
 * (x, y, z); the largest number of points any 21 x 21 x 11 box of cubes holds (corner, surf); 1 when that is exact (sliding sums over the
 * bounding box), 0 when it is the class total (bounding box above 2^24 cells); device bytes.  Zeros when no atlas is loaded. */
int aloam_atlas_load(aloam_ctx* ctx, const aloam_map_tile* tiles, long long n_tiles, const float* points_xyzw, long long n_points);
int aloam_atlas_attach(aloam_ctx* ctx, const int* attached /* [batch], NULL = none */);
int aloam_atlas_info(aloam_ctx* ctx, long long out[12]);

/* ---- place recognition: scan-context descriptors and batched matching ------------------------------------------------------------
 * Stands beside the reference, like the frozen map, the hypotheses and the atlas: A-LOAM has no place recognition.  A frozen step refines
 * a guess that is about 1 m and 2.5 deg off, aloam_score_map_corrections searches a grid of a few metres around one; this section finds
 * the guess with no prior at all.  The signature of a sweep is Scan Context (G. Kim, A. Kim, "Scan Context: Egocentric Spatial Descriptor
 * for Place Recognition within 3D Point Cloud Map", IROS 2018): a polar grid of ALOAM_PLACE_RINGS x ALOAM_PLACE_SECTORS cells around the
 * sensor, each the greatest height of its points.  A turn of the sensor about z is a cyclic shift of the sectors, so one match returns a
 * stored place and a yaw.  Opt-in: a context that never calls aloam_places_enable launches exactly what it launched before.
 *
 * The descriptor is a function of the set of points of a sequence's ALOAM_CLOUD_FULL (the points scan registration keeps, in the
 * sensor frame; their order plays no part), every operation a separately rounded f32 operation:
 *     rho = sqrtf(x * x + y * y);  r = (int)(rho * (20.f / max_range));  points with r >= 20 are skipped
 *     theta = atan2f(y, x) + (float)M_PI   (atan2f with glibc's bits);  s = min((int)(theta * (float)(60 / (2 pi))), 59)
 *     D[r][s] = max over its points of max(z + sensor_height, 0);  empty cells are 0
 * It is made from the ring slabs (the dense cloud is not assembled for it), at most once per registered sweep, by the first
 * aloam_places_add / aloam_places_match that lists the sequence.
 *
 * aloam_places_enable: once per context; allocates the store (capacity in 1 .. 2^20 entries) and one descriptor per sequence.
 * max_range > 0 and sensor_height finite (80 m and 2 m suit a car-mounted HDL-64), else ALOAM_E_ARG.  Contexts without
 * ALOAM_STAGE_REGISTRATION: ALOAM_E_STATE, here and in every other call of this section.
 *
 * aloam_places_add: appends one entry per listed sequence (distinct, in range), in listed order and in stream order; no host
 * synchronisation.  The store index of entry i is the count before the call + i, so the host knows it when the call returns.  The tag is
 * read on the device at that point of the stream: map_q_w / map_t_w as aloam_export_poses would write them with mapping enabled, else
 * q_w / t_w; frame = map_frames, or -1 without mapping; slot = the sequence; n_points = the points of the sweep.  A store that cannot take
 * all n: ALOAM_E_CAPACITY, nothing is queued.
 *
 * Which sequences may be listed (add and match): those that have registered a sweep since the context was created or since the slot
 * was last reset or loaded (a host flag, like the one of aloam_score_map_corrections); otherwise ALOAM_E_STATE and nothing is queued.  A
 * sequence that sat out the last registration uses the sweep it still holds.
 *
 * aloam_places_match: for each listed sequence i (its descriptor Q) the T best entries of [ranges[2 i], ranges[2 i + 1]) go to
 * dst[i * T ..], best first; entry = -1 (shift -1, distance 0) fills what the range does not provide.  For an entry C and a shift:
 *     d(shift) = 1 - (1 / cnt) * sum over the columns j where C[:, j] and Q[:, (j - shift) mod 60] are both non-zero of their cosine
 * cnt = the number of such columns (a shift with cnt = 0 is skipped; an entry with no valid shift is never returned).  The entry's distance
 * is the minimum over the 60 shifts, ties to the lower shift; entries rank by (distance, index).  A match with shift s means: the sensor
 * stands at the stored pose turned by +s * 6 deg about its own z.  1 <= T <= 8, 0 <= lo <= hi <= count at the time of the call: else
 * ALOAM_E_ARG.  Stream-ordered, no host synchronisation (the first call, and one with more (sequence, entry) pairs than any before,
 * allocates scratch); `ranges` is read during the call only; dst: device memory of the context's device or pinned host memory, classified
 * like the destinations of aloam_export_clouds.  All 60 shifts of a query against a tile of entries are one 64 x 1200 x tile product
 * of unit-normalised columns on the f32-input matrix cores, in a fixed K order: a (query, entry) result has the same bits whatever n, T,
 * the range and the position in the list.
 *
 * aloam_places_export / aloam_places_load: entries [first, first + count) to dst (device or pinned), and count records appended from src
 * (device, pinned, or pageable through one staged copy); both stream-ordered.  A load validates every record before anything changes
 * (cells finite and non-negative, and the positive ones inside [2^-62, 2^60] (2.2e-19 .. 1.2e18; the cells are heights in metres), else
 * ALOAM_E_ARG; records in device memory are read back once for that).  Inside that range the f32 squares of a column's cells and their sum
 * are normal numbers: a column is non-zero for the match exactly when one of its cells is.  aloam_places_clear empties the
 * store in stream order.  aloam_places_info: out = count, capacity, max_range bits, sensor_height bits (IEEE-754).
 *
 * The store is not part of a sequence record (ALOAM_SEQ_RECORD_VERSION, MapSeq and aloam_pose_record are unchanged);
 * aloam_reset_sequences and aloam_load_sequences leave it alone. */
enum { ALOAM_PLACE_RINGS = 20, ALOAM_PLACE_SECTORS = 60 };
typedef struct aloam_place {                  /* 4880 bytes */
  float cells[ALOAM_PLACE_SECTORS][ALOAM_PLACE_RINGS];   /* sector-major: a yaw shift is an offset */
  double q[4], t[3];                          /* pose of the sensor when the place was stored */
  int slot;                                   /* the sequence that stored it */
  int frame;                                  /* its map_frames then; -1 without mapping */
  int n_points;                               /* points of the sweep */
  int pad[3];
} aloam_place;
typedef struct aloam_place_match { int entry, shift; float distance; int pad; } aloam_place_match;   /* 16 bytes */
int aloam_places_enable(aloam_ctx* ctx, int capacity, float max_range, float sensor_height);
int aloam_places_add(aloam_ctx* ctx, const int* seqs, int n);
int aloam_places_match(aloam_ctx* ctx, const int* seqs, int n, const int* ranges /* [n][2] */, int T, aloam_place_match* dst /* [n][T] */);
int aloam_places_export(aloam_ctx* ctx, int first, int count, aloam_place* dst);
int aloam_places_load(aloam_ctx* ctx, const aloam_place* src, int count);
int aloam_places_clear(aloam_ctx* ctx);
int aloam_places_info(aloam_ctx* ctx, int out[4]);

/* ---- sequence records: save and restore whole sequences, in batched stream-ordered calls ------------------------------
 * A sequence record is everything that makes up a sequence between two frames - odometry pose and statistics, systemInited, the last
 * clouds (laserCloudCornerLast / SurfLast, src/laserOdometry.cpp:554-563), and with mapping the map pose, window centre, frame count,
 * counters, the last step's window and every non-empty cube (src/laserMapping.cpp:72-116) - in a position-independent byte layout.  A
 * sequence loaded into a slot of any context whose configuration is compatible (below) continues bit for bit as if it had never left.
 *
 * aloam_save_sequences: records of the n sequences seqs[0 .. n) (distinct, in range; idle and never-initialised sequences too), queued on
 * the context's stream with no host synchronisation and no read-back, holding the state at that point of the stream.  dst and dst_offsets:
 * device memory of the context's device or pinned host memory (as for aloam_export_clouds; pageable memory, another device's memory and
 * NULL are refused with ALOAM_E_ARG before anything is queued; dst may be NULL when cap_bytes is 0), dst 16-byte aligned.  The device always
 * writes dst_offsets[0 .. n] in bytes: record i lies at [dst_offsets[i], dst_offsets[i + 1]), every record a multiple of 256 bytes.  A
 * record is written whole, and only when it ends at or before cap_bytes: nothing is ever written past cap_bytes, and cap_bytes = 0 is the
 * size query.
 *
 * aloam_load_sequences: record i of src (at [src_offsets[i], src_offsets[i + 1])) into slot slots[i], for n distinct slots (one record
 * may go to several slots: a fork).  src and src_offsets may be device memory of the context's device, pinned host memory, or pageable
 * host memory (staged through context scratch, so a record read from a file loads directly); src 16-byte aligned.  The call synchronises
 * the context's stream once and reads the n headers (the map pools are sized on the host; records in device memory: one small gather
 * kernel and a second wait); every header is checked before anything is
 * queued - magic, version, length equal to the offsets' difference, the parts held and the compatibility fields - and a failed load
 * changes nothing.  The rest is asynchronous: src must stay unchanged until aloam_synchronize or an event on aloam_stream.  A loaded slot
 * first becomes what aloam_reset_sequences makes of it, then receives the record; the active mask is not changed.
 *   - Compatibility: n_scans, ring_from_field, min_range, distortion, lm_max_iterations, outer_iterations, the voxel sum order, the parts
 *     held (odometry: the context has ALOAM_STAGE_ODOMETRY; map: mapping is enabled) and the two mapping resolutions must equal the saving
 *     context's, else ALOAM_E_ARG with the field named by aloam_last_error.  Batch, device, max_points, pool size and pool limit may
 *     differ: a last cloud larger than the target's max_points, or a map class above its pool limit, is ALOAM_E_CAPACITY; a map above its
 *     pool size grows the pools first.
 *   - Frame boundaries: both calls fail with ALOAM_E_STATE between a registration and the odometry step that consumes it.  A sequence
 *     saved after a frame's odometry step but before its mapping step has dropped that frame in mapping (src/laserMapping.cpp:299-303).
 *     In a context with ALOAM_STAGE_ODOMETRY a loaded slot takes part in one registration and odometry step before it may be active in a
 *     mapping step; until then aloam_mapping_step returns ALOAM_E_STATE and queues nothing.
 *   - The per-step scratch of a sequence (current sweep and its features, dense cloud, curvature, labels, ring starts, correspondences,
 *     search grids, stacks, registered cloud) is not part of a record: it reads as after aloam_reset_sequences until the next step.  Nor
 *     is the residue of older sweeps that ALOAM_CLOUD_LESS_SHARP / LESS_FLAT return past the previous last clouds after an odometry step.
 *     The cubes are packed back to back in the target's pool; aloam_get_map_info's compaction count is kept.
 * Records of another version are refused; the payload carries no checksum. */
enum { ALOAM_SEQ_RECORD_MAGIC = 0x51534c41, ALOAM_SEQ_RECORD_VERSION = 1 };   /* magic: the bytes "ALSQ" */
enum { ALOAM_SEQ_PART_ODOMETRY = 1, ALOAM_SEQ_PART_MAP = 2 };
typedef struct aloam_seq_record_header {     /* first 128 bytes of a record                                                      */
  unsigned int magic;                        /* ALOAM_SEQ_RECORD_MAGIC                                                            */
  unsigned int version;                      /* ALOAM_SEQ_RECORD_VERSION                                                          */
  long long bytes;                           /* whole record, a multiple of 256                                                   */
  int parts;                                 /* ALOAM_SEQ_PART_* held                                                             */
  int n_scans, ring_from_field;              /* the saving context's configuration (aloam_config) ...                            */
  unsigned int min_range_bits;               /* ... min_range as its IEEE-754 bits                                                */
  int distortion, lm_max_iterations, outer_iterations;
  int sum_order;                             /* ALOAM_SUM_*                                                                       */
  unsigned int line_res_bits, plane_res_bits;   /* mapping resolutions as bits; 0 without the map part                           */
  int inited;                                /* systemInited of the sequence                                                      */
  int n_corner_last, n_surf_last;            /* points of the last clouds (0 without the odometry part)                          */
  int n_cubes[2];                            /* non-empty cubes, corner / surf                                                    */
  int map_points[2];                         /* points of those cubes, corner / surf                                              */
  int err_events;                            /* map-pool capacity events of the sequence so far (not reported again after a load) */
  int seq_meta_bytes, odom_bytes, map_seq_bytes;   /* sizes of the fixed sections that follow the header                         */
  int pad[6];
} aloam_seq_record_header;
int aloam_save_sequences(aloam_ctx* ctx, const int* seqs, int n, void* dst, long long cap_bytes, long long* dst_offsets);
int aloam_load_sequences(aloam_ctx* ctx, const int* slots, int n, const void* src, const long long* src_offsets);

/* ---- pose information: how well the geometry constrained the pose a solve returned ---------------------------------------------------
 * The 6 x 6 information matrix (J^T J of the robustified residuals) of the last odometry or mapping solve of each listed sequence, at the
 * pose that solve left, with its eigen-decomposition and the two 3 x 3 marginals.  A pose with thousands of factors and a small cost can
 * still be unconstrained along one direction (a corridor, a tunnel, an open field): the smallest eigenvalue of trans_info against the next
 * one says so, and its eigenvector says which way.  The matrix reports what the solver saw, not the truth.
 *
 * Definition, operation by operation (a-loam_amd/information.py restates it in numpy):
 *   1. Factor set.  The factor records the last solve of the sequence read: odometry - the correspondences of the last outer iteration
 *      (aloam_get_correspondences); mapping - the line and plane-norm factors of the second iteration (aloam_get_map_factors).
 *   2. Pose.  The one that solve left: odometry q_last_curr / t_last_curr (para_q / para_t), mapping q_w_curr / t_w_curr.  After a solve
 *      that ended as FAILURE this is the restored entry pose.
 *   3. Rows.  Per line factor the three residuals r = (lp - a) x (lp - b) / |a - b|, per plane factor the one residual r = n . (lp - j)
 *      (odometry, n = normalize((j - l) x (j - m))) or r = n . lp + d (mapping), with lp = q cp + t, or with aloam_config.distortion = 1 (odometry)
 *      lp = slerp(identity, q, s) cp + s t, s = the interpolation ratio of the query point (its intensity's fractional part / 0.1).
 *   4. Weights.  Every residual block is scaled by sqrt(rho'(|r|^2)) of HuberLoss(0.1), as in the solver: rho' = 1 for |r|^2 <= 0.01, else
 *      0.1 / |r|.  cost = 1/2 sum rho(|r|^2).  No Jacobi (column) scaling.
 *   5. Tangent and units.  The solver's tangent is Ceres' EigenQuaternionParameterization::Plus, q' = (sin|d| d/|d|, cos|d|) * q: a LEFT
 *      perturbation by the rotation vector theta = 2 d, expressed in the target frame (odometry: the last sweep's frame; mapping: the map
 *      frame), followed by t' = t + dt in the same frame.  With H_d = sum w J_d^T J_d and g_d = sum w J_d^T r in that tangent,
 *      info = S H_d S and gradient = S g_d, S = diag(1/2, 1/2, 1/2, 1, 1, 1): radians and metres, order (theta_x, theta_y, theta_z, t_x, t_y, t_z).
 *   6. Eigenpairs.  Cyclic Jacobi in f64 with a fixed rotation order (0,1), (0,2) .. (4,5), sweeps until sum |a_pq| <= 1e-17 sum |a_pp|:
 *      a function of the matrix alone.  Ascending eigenvalues; column k of `eigenvectors` (row-major) belongs to eigenvalues[k]; the
 *      component of largest magnitude of every eigenvector is positive, the lowest index deciding a tie.
 *   7. Marginals.  trans_info = H_tt - H_tr H_rr^-1 H_rt and rot_info = H_rr - H_rt H_tt^-1 H_tr (Schur complements: the information about
 *      one half when the other is unknown), through a 3 x 3 Cholesky factorisation of the block that is inverted; a block counts as
 *      positive definite when every pivot exceeds 1e-12 times its diagonal entry.  Their eigenpairs as in 6.
 * Covariance.  Not computed on the device: cov = sigma^2 V diag(1 / lambda) V^T with sigma^2 = 2 cost / (rows - 6), V / lambda the
 * eigenpairs of `info` (a-loam_amd/information.py covariance(); INTEGRATION.md for nav_msgs/Odometry, whose order is translation first).
 *
 * status: ALOAM_INFO_NONE - no solve of that kind has run for this sequence since the context was created or since the last of these that
 *   touched it: aloam_reset_sequences, aloam_load_sequences (both kinds); aloam_set_state, aloam_set_features, aloam_set_last (odometry:
 *   they replace the pose, the feature counts or the clouds its records belong to); aloam_set_map, aloam_set_map_frame,
 *   aloam_apply_map_corrections (mapping: the pose of its solve is in a map or frame that is gone).  For the odometry kind also a
 *   registration of a new sweep that the odometry step has not consumed yet (the records are read through the feature counts of the sweep
 *   they were made from, as aloam_get_correspondences reads them), and a first frame, which solves nothing.  Everything but status and
 *   frame is zero.
 *   ALOAM_INFO_NO_FACTORS - the solve ran with no residual block (mapping: the gate of src/laserMapping.cpp:554 was false); everything but
 *   status and frame is zero.  ALOAM_INFO_SINGULAR - info, its eigenpairs, gradient, cost and counts are valid, but a block needed for a
 *   Schur complement is not positive definite: that marginal and its eigenpairs are zero.
 * A sequence that sat out the last step reports exactly the bits it reported before that step.
 *
 * Call semantics, as aloam_export_poses: queued on the context's stream, no host synchronisation, nothing read back; it writes the state at
 * that point of the stream.  dst[i] belongs to seqs[i]; its bits do not depend on n, on i or on the other sequences listed.  dst is device
 * memory of the context's device or pinned host memory, 8-byte aligned, classified before anything is queued: pageable, another device's,
 * managed or NULL with n > 0 -> ALOAM_E_ARG.  Out-of-range or repeated ids, n outside 0 .. batch, an unknown `which` -> ALOAM_E_ARG.
 * ALOAM_INFO_MAPPING before aloam_mapping_enable, or a kind whose stage the context was created without -> ALOAM_E_STATE.  n = 0 is legal
 * and queues nothing.  `seqs` is read during the call only.  The flags behind ALOAM_INFO_NONE are host state of the context, not part of
 * a sequence record (ALOAM_SEQ_RECORD_VERSION is unchanged). */
enum { ALOAM_INFO_ODOMETRY = 0, ALOAM_INFO_MAPPING = 1 };
enum { ALOAM_INFO_OK = 0, ALOAM_INFO_NONE = 1, ALOAM_INFO_NO_FACTORS = 2, ALOAM_INFO_SINGULAR = 3 };
typedef struct aloam_pose_information {       /* one per listed sequence; 1048 bytes                                                    */
  double info[36];                            /* 6 x 6, row-major, symmetric; order (theta_x, theta_y, theta_z, t_x, t_y, t_z)          */
  double eigenvalues[6];                      /* ascending                                                                              */
  double eigenvectors[36];                    /* row-major, column k belongs to eigenvalues[k]                                          */
  double trans_info[9], trans_eigenvalues[3], trans_eigenvectors[9];   /* H_tt - H_tr H_rr^-1 H_rt                                      */
  double rot_info[9], rot_eigenvalues[3], rot_eigenvectors[9];         /* H_rr - H_rt H_tt^-1 H_tr                                      */
  double gradient[6];                         /* J^T r, same units                                                                      */
  double cost;                                /* 1/2 sum rho(|r|^2) at that pose                                                        */
  int n_line, n_plane, rows;                  /* residual blocks per class; rows = 3 n_line + n_plane                                   */
  int status;                                 /* ALOAM_INFO_OK ..                                                                       */
  int frame;                                  /* mapping: frameCount after that step; odometry: -1                                      */
  int pad[3];
} aloam_pose_information;
int aloam_export_pose_information(aloam_ctx* ctx, int which, const int* seqs, int n, aloam_pose_information* dst /* [n] */);

/* ---- pose graphs: keyframes, odometry / loop / anchor edges, and a batched solve --------------------------------------------------------
 * One graph per sequence, kept on the device: nodes are poses entered from the sequence's own state, edges are relative poses between two
 * nodes (odometry, loop closures) or absolute poses of one node (anchors: a localization in an atlas).  aloam_graph_optimize runs
 * Levenberg-Marquardt over the graphs of the listed sequences, one workgroup each.  Beside the reference (A-LOAM has no back end) and
 * opt-in: a context that never calls aloam_graph_enable launches what it launched before.  a-loam_amd/posegraph.py restates every
 * operation in numpy; DESIGN.md §7k.
 *
 * Poses.  X = (q, t), q = (x, y, z, w): x' = q x q* + t.  Xa o Xb = (q_a q_b, q_a t_b + t_a); X^-1 = (q*, -(q* t)).
 * Problem.  For an edge (i, j, Z, Omega): E = Z^-1 o X_i^-1 o X_j, evaluated as q_d = q_i* q_j, t_d = q_i* (t_j - t_i), q_E = q_Z* q_d,
 *   t_E = q_Z* (t_d - t_Z); X_i is the identity for an anchor (i = -1).  q_E is negated when its w < 0.  r = (2 q_E.xyz, t_E), s = r^T Omega r.
 *   cost = 1/2 sum rho(s): rho(s) = s for plain edges; for edges flagged ALOAM_GRAPH_EDGE_ROBUST it is Ceres' HuberLoss(huber_delta),
 *   s <= delta^2 ? s : 2 delta sqrt(s) - delta^2, applied as the solvers apply it (rows scaled by sqrt(rho'), rho' = delta / sqrt(s)).
 *   Node 0 is held fixed.  The tangent of a node is a LEFT perturbation, q' = exp(theta / 2) q, t' = t + dt, order (theta, t): the order and
 *   the units (radians, metres) of aloam_pose_information.info, so the upper triangle of such a record can be copied into an edge.
 *
 * aloam_graph_enable(ctx, max_nodes, max_edges): once per context; every sequence gets a row of max_nodes nodes and max_edges edges (the
 *   odometry edges count).  1 <= max_nodes <= 2^20, 1 <= max_edges <= 2^22, else ALOAM_E_ARG; a second call: ALOAM_E_STATE.  Needs
 *   ALOAM_STAGE_ODOMETRY.  Every other call of this section returns ALOAM_E_STATE before it, and queues nothing on any error.
 * aloam_graph_add_nodes: one node per listed sequence (distinct, in range), stream-ordered, no host synchronisation.  The pose is read on
 *   the device at that point of the stream, as aloam_places_add reads it: q_w_curr / t_w_curr and frameCount with mapping enabled, else
 *   the odometry's q_w / t_w and -1.  Node k > 0 also gets the odometry edge (k - 1, k) with Z = X[k-1]^-1 o X[k] of the entered poses and
 *   the information odom_info[i] (upper triangle, 21 doubles; required; finite and positive definite, else ALOAM_E_ARG), and the estimate
 *   X_opt[k-1] o Z; node 0's estimate is its entered pose.  The counts are host state: the new node's index is aloam_graph_info's count
 *   before the call.  A row without room for the node or its edge: ALOAM_E_CAPACITY.
 * aloam_graph_add_edges: `edges` in host memory (pinned or pageable), read during the call.  Everything is validated before anything is
 *   queued: seq in range; -1 <= i < nodes, 0 <= j < nodes, i != j; q finite and within 1e-6 of unit norm (stored normalised); t finite;
 *   info finite and positive definite (a host Cholesky succeeds); flags 0 or ALOAM_GRAPH_EDGE_ROBUST: else ALOAM_E_ARG.  No room:
 *   ALOAM_E_CAPACITY.  Edges are appended to their sequence's row in the order given.  (Stream-ordered on the device; the copy out of
 *   pageable memory may wait on the host for the stream, unlike aloam_graph_add_nodes and aloam_graph_optimize.)
 * aloam_graph_export / aloam_graph_export_edges: nodes / edges [first, first + count) of one sequence, stream-ordered, into device memory
 *   of the context's device or pinned host memory, 8-byte aligned (pageable, managed, another device's, NULL with count > 0: ALOAM_E_ARG).
 * aloam_graph_clear: the listed sequences' graphs become empty (counts are host state; later adds overwrite in stream order).
 * aloam_graph_info: out = {nodes, edges, max_nodes, max_edges} of one sequence.
 * The graph is NOT part of a sequence record: aloam_reset_sequences, aloam_save_sequences and aloam_load_sequences leave it alone, like the
 *   map spill.  The caller clears a slot's graph before the slot starts another drive.
 *
 * aloam_graph_optimize: stream-ordered; dst[i] belongs to seqs[i], in device or pinned memory like the exports; its bits and the exported
 *   nodes do not depend on n, on i or on the other sequences listed.  opt = NULL: the defaults.  Options (the algorithm's parameters):
 *   max_iterations >= 0, pcg_max_iterations >= 1, the tolerances >= 0 and finite, huber_delta > 0, else ALOAM_E_ARG.
 *   status: ALOAM_GRAPH_OK; ALOAM_GRAPH_NO_EDGES - fewer than two nodes or no edge, nothing done; ALOAM_GRAPH_FAILED - the solve ended as a
 *   failure or above its initial cost: the estimates are as they were.  The estimates (q_opt, t_opt) are written back only when the final
 *   cost is not above the initial one.  termination: 0 max_iterations, 2 function_tolerance (|cost change| <= tol * cost), 3
 *   gradient_tolerance (max-norm of the gradient in the tangent above), 5 failure (five unusable steps in a row, or a non-finite
 *   evaluation), 6 minimum trust-region radius.  The loop is the trust-region Levenberg-Marquardt of the odometry and mapping solvers
 *   (initial radius 1e4, diagonal clamp [1e-6, 1e32], acceptance above 1e-3 relative decrease); each step is solved by conjugate
 *   gradients preconditioned with the block-tridiagonal chain, to pcg_tolerance relative in the preconditioned norm.  No host
 *   synchronisation.  A node's incident edges are ordered by one lane, d^2 / 2 moves for d of them: meant for up to a few hundred
 *   edges on one node. */
enum { ALOAM_GRAPH_EDGE_ROBUST = 1 };
enum { ALOAM_GRAPH_OK = 0, ALOAM_GRAPH_NO_EDGES = 1, ALOAM_GRAPH_FAILED = 2 };
typedef struct aloam_graph_node {             /* 128 bytes                                                                              */
  double q[4], t[3];                          /* the pose as entered, in the sequence's own (drifting) frame; changed only by aloam_graph_apply */
  double q_opt[4], t_opt[3];                  /* the current estimate                                                                   */
  int frame;                                  /* frameCount when it was entered (mapping), else -1                                      */
  int pad[3];
} aloam_graph_node;
typedef struct aloam_graph_edge {             /* 240 bytes                                                                              */
  int seq, i, j, flags;                       /* i = -1: the fixed world frame (an anchor of node j)                                    */
  double q[4], t[3];                          /* Z: the measured pose of node j in the frame of node i                                  */
  double info[21];                            /* upper triangle, row-major, of the 6 x 6 information, order (theta_x .. t_z)            */
} aloam_graph_edge;
typedef struct aloam_graph_options {          /* 40 bytes                                                                               */
  int max_iterations;                         /* 20                                                                                     */
  int pcg_max_iterations;                     /* 200                                                                                    */
  double function_tolerance;                  /* 1e-10, relative cost change                                                            */
  double gradient_tolerance;                  /* 1e-10, max-norm                                                                        */
  double pcg_tolerance;                       /* 1e-8, relative in the preconditioned norm                                              */
  double huber_delta;                         /* 1.0: s is a squared Mahalanobis distance, so delta is in standard deviations           */
} aloam_graph_options;
typedef struct aloam_graph_result {           /* 64 bytes                                                                               */
  int status, termination;
  int lm_iterations, accepted_steps, pcg_iterations;
  int nodes, edges, pad;
  double initial_cost, final_cost, gradient_max, reserved;
} aloam_graph_result;
void aloam_graph_default_options(aloam_graph_options* opt);
int aloam_graph_enable(aloam_ctx* ctx, int max_nodes, int max_edges);
int aloam_graph_add_nodes(aloam_ctx* ctx, const int* seqs, int n, const double* odom_info /* [n][21] */);
int aloam_graph_add_edges(aloam_ctx* ctx, const aloam_graph_edge* edges, int n);
int aloam_graph_export(aloam_ctx* ctx, int seq, int first, int count, aloam_graph_node* dst);
int aloam_graph_export_edges(aloam_ctx* ctx, int seq, int first, int count, aloam_graph_edge* dst);
int aloam_graph_clear(aloam_ctx* ctx, const int* seqs, int n);
int aloam_graph_info(aloam_ctx* ctx, int seq, int out[4]);
int aloam_graph_optimize(aloam_ctx* ctx, const int* seqs, int n, const aloam_graph_options* opt, aloam_graph_result* dst /* [n] */);

/* ---- keyframe clouds and the map at the graph's poses ---------------------------------------------------------------------------------
 * aloam_graph_optimize moves the poses of a graph's nodes; this section lets the map follow.  Every node keeps its own clouds on the device
 * in the sensor frame, and map tiles (aloam_map_tile, the format aloam_export_map_spill writes and aloam_atlas_load reads) are assembled
 * from them at whichever poses the graph holds now.  Opt-in and beside the reference: a context that never calls
 * aloam_graph_keyframes_enable launches exactly what it launched before.  a-loam_amd/atlas.py (tiles_from_keyframes) restates the
 * definition in numpy; DESIGN.md §7l.
 *
 * aloam_graph_keyframes_enable(ctx, max_corner_points, max_surf_points): once per context, after aloam_graph_enable and
 *   aloam_mapping_enable and while every sequence's graph is empty, else ALOAM_E_STATE.  Allocates, per sequence and class, a row of that
 *   many 16-byte points, per node a descriptor (first, count) per class, per sequence and class an append cursor on the device.  Sizes in
 *   1 .. 2^26, else ALOAM_E_ARG; nothing stays allocated behind a refusal.  Every other call of this section is ALOAM_E_STATE before it.
 *   From then on aloam_graph_add_nodes queues one more kernel behind its own: for every listed sequence the sequence's
 *   laserCloudCornerStack / laserCloudSurfStack (ALOAM_MAP_CORNER_STACK / ALOAM_MAP_SURF_STACK) as they are at that point of the stream
 *   become the new node's clouds.  They are in the sensor frame: associate-to-map of them with the node's pose is where the mapping step
 *   put them.
 *   - A node's clouds are kept whole or not at all.  A node whose corner or surf cloud does not fit what is left of its rows is kept
 *     without clouds (counts of 0) and counted; the next aloam_synchronize returns ALOAM_E_CAPACITY once, "keyframe store full".
 *   - A listed sequence that has not been active in a mapping step since the context was created or the slot was last reset or loaded
 *     (a host flag, like the one of aloam_score_map_corrections): aloam_graph_add_nodes returns ALOAM_E_STATE and queues nothing.
 *   - aloam_graph_clear also rewinds the listed sequences' cursors, in stream order.  aloam_reset_sequences, aloam_save_sequences and
 *     aloam_load_sequences leave the store alone, like the graph; it is not part of a sequence record.
 * aloam_graph_export_keyframes: the clouds of nodes [first, first + count) of one sequence and class, packed in node order.  Stream-
 *   ordered; destinations are classified like those of aloam_export_clouds (device memory of the context's device or pinned host memory).
 *   dst_offsets[0 .. count] is always written (node first + j at [dst_offsets[j], dst_offsets[j + 1])); the points are written only when
 *   the range ends inside cap_points; a cap of 0 is the size query (points_dst may then be NULL).
 * aloam_graph_keyframe_info (synchronises): out = points held (corner, surf), capacities (corner, surf), nodes kept without clouds so far,
 *   their points, and two reserved zeros.
 *
 * aloam_graph_export_map: for each of the n requests (host memory, read during the call), the map made of the nodes
 *   [first, first + count) of sequence seq at their entered poses (q, t) or their estimates (q_opt, t_opt):
 *   - every point p of every node k becomes w = associate-to-map(p, X_k): rotation and translation in f64, each component stored to f32,
 *     the intensity kept (the operations of the mapping step, in that order);
 *   - the cube of w is int((v + 25) / 50), minus one when v + 25 < 0, of (double)w.x, w.y, w.z (the definition under "map tiles"; -75
 *     exactly lands in cube -2); points whose cube lies outside -512 .. 511 on some axis are left out and counted in `outside`;
 *   - the members of a (cube, class) are its points in node order, then point order inside the node;
 *   - they are filtered once with that class's pcl::VoxelGrid leaf (mapping_line_resolution / mapping_plane_resolution), always the
 *     input-order sum, as in aloam_atlas_load, and always applied, even when one node contributes: a rotated cloud is not on its own grid;
 *   - corner tiles come first, then surf tiles, each ascending in (cube[0], cube[1], cube[2]); frame is 0; first_point indexes points_dst.
 *   dst_offsets[0 .. n] holds the tile offsets and dst_offsets[n + 1 .. 2 n + 1] the point offsets, always written; a request's tiles and
 *   points are written only when BOTH of its ranges end inside cap_tiles / cap_points, nothing is ever written past a cap, and caps of 0
 *   are the size query, as in aloam_export_map_spill.  stats_dst (NULL = not wanted) receives one record per request.  The bits written
 *   for a request do not depend on n, on its position in the list or on the other requests; a sequence may be listed more than once.
 *   Checked before anything is queued, ALOAM_E_ARG: seq in range; 0 <= first, 0 <= count, first + count <= the sequence's nodes; pose 0 or
 *   1; n <= 32768; the destinations like those of the exports (stats_dst too).
 *   It SYNCHRONISES the context's stream once, after the transform pass: the counts per (cube, class) are read back, and from them the
 *   host lays out the cubes and plans the rounds of the voxel filter as aloam_atlas_load does.  Keyframe points never pass through host
 *   memory; everything behind that point is stream-ordered (wait with aloam_synchronize before reading the destinations).  Meant to be
 *   called once per loop closure, not once per sweep.  A (cube, class) with more raw points than a map pool row grows the map pools first;
 *   at the pool limit it is ALOAM_E_CAPACITY and nothing is written.  The counts are kept per (cube, piece of 4096 points) in a
 *   directory sized for a dozen cubes per sweep; a call whose points scatter over more cubes than it holds runs its first pass again with
 *   the directory doubled (one more synchronisation each time; the size is kept for later calls), and one that needs more than 2^22
 *   entries is ALOAM_E_CAPACITY with nothing written: export fewer nodes per call. */
enum { ALOAM_GRAPH_POSE_ENTERED = 0, ALOAM_GRAPH_POSE_OPTIMIZED = 1 };
typedef struct aloam_graph_map_request {      /* 16 bytes: nodes [first, first + count) of sequence seq                                 */
  int seq, first, count, pose;                /* pose: ALOAM_GRAPH_POSE_ENTERED (q, t) or ALOAM_GRAPH_POSE_OPTIMIZED (q_opt, t_opt)     */
} aloam_graph_map_request;
typedef struct aloam_graph_map_stats {        /* 32 bytes                                                                               */
  int tiles[2], points[2];                    /* of the request: corner, surf                                                           */
  int raw_points[2];                          /* keyframe points that went into its cubes                                               */
  int outside;                                /* points whose cube lies outside -512 .. 511 on some axis: left out                      */
  int written;                                /* 1 when the request's tiles and points were written                                     */
} aloam_graph_map_stats;
int aloam_graph_keyframes_enable(aloam_ctx* ctx, int max_corner_points, int max_surf_points);
int aloam_graph_export_keyframes(aloam_ctx* ctx, int seq, int first, int count, int feature_class, float* points_dst_xyzw, long long cap_points,
                                 long long* dst_offsets /* [count + 1] */);
int aloam_graph_keyframe_info(aloam_ctx* ctx, int seq, long long out[8]);
int aloam_graph_export_map(aloam_ctx* ctx, const aloam_graph_map_request* req, int n, aloam_map_tile* tiles_dst, long long cap_tiles,
                           float* points_dst_xyzw, long long cap_points, long long* dst_offsets /* [2][n + 1] */,
                           aloam_graph_map_stats* stats_dst /* [n] or NULL */);

/* ---- a solved graph carried into the live state ----------------------------------------------------------------------------------------
 * aloam_graph_optimize and aloam_graph_export_map end in exports; aloam_graph_apply closes the loop in the sequence itself, so that the
 * next aloam_mapping_step registers against the corrected geometry and the next node is entered in the corrected frame.  Opt-in and
 * beside the reference: a context that never calls it launches exactly what it launched before.  a-loam_amd/posegraph.py
 * (apply_correction) and a-loam_amd/atlas.py (window_from_keyframes) restate the definition in numpy; DESIGN.md §7m.
 *
 * For each of the n requests (host memory, read during the call) whose sequence holds K >= 1 nodes, everything is read on the device at
 * that point of the stream (aloam_graph_optimize, aloam_graph_apply, aloam_mapping_step need no synchronise from the caller in between),
 * every operation a separately rounded f64 operation:
 *   - the correction comes from the LAST node K - 1, whatever first and count are: q_D = normalise(q_opt conj(q)), t_D = t_opt - q_D t;
 *   - q_wmap_wodom := q_D q_wmap_wodom, t_wmap_wodom := q_D t_wmap_wodom + t_D, and q_w_curr / t_w_curr (aloam_get_map_pose) the same way;
 *     the odometry state and frameCount are not touched;
 *   - every node of the sequence is rebased: (q, t) := (q_opt, t_opt), bit copies; q_opt, t_opt and every edge stay.  The live frame has
 *     become the optimised one, and aloam_graph_add_nodes forms the next odometry edge from the entered poses;
 *   - with ALOAM_GRAPH_APPLY_MAP the sequence's 2 x 4851 cubes are replaced by the map of nodes [first, first + count) at (q_opt, t_opt),
 *     exactly as aloam_graph_export_map defines it, cut at the new window centre cen' = (10, 10, 5) - cube(t_w_curr'): the tile of
 *     absolute cube c lands at window index c + cen'; tiles outside the window are left out and their filtered points counted in
 *     outside_window.  The cubes are packed from the start of the pool row in ascending window index, as aloam_set_map would write that
 *     cut.  The rebuilt map holds KEYFRAMES ONLY: the points of sweeps between keyframes are gone.  The old window is not spilled
 *     (aloam_map_spill_enable): its cubes are in the old frame.
 * All or nothing per sequence: a window that does not fit its pool row leaves pose, nodes and map as they were (status
 *   ALOAM_GRAPH_APPLY_NO_ROOM).  The call grows the map pools first, to the largest 21 x 21 x 11 box of cubes of any listed map (filtered
 *   points per class; where the sensor will be is known on the device only), so that this is a second line only; at the pool limit the call returns ALOAM_E_CAPACITY with nothing
 *   changed.  K = 0: status ALOAM_GRAPH_APPLY_NO_NODES, nothing changed.
 * Checked before anything is queued, nothing changes on a refusal.  ALOAM_E_STATE: before aloam_graph_enable or aloam_mapping_enable;
 *   ALOAM_GRAPH_APPLY_MAP before aloam_graph_keyframes_enable; a listed sequence frozen (aloam_set_map_frozen) or attached
 *   (aloam_atlas_attach): its map is not its own.  ALOAM_E_ARG: seq out of range or listed twice; first, count outside the sequence's
 *   nodes; flags other than ALOAM_GRAPH_APPLY_POSE or ALOAM_GRAPH_APPLY_POSE | ALOAM_GRAPH_APPLY_MAP; dst not device memory of the
 *   context's device or pinned host memory (classified like the exports).  n = 0 is ALOAM_OK.
 * With ALOAM_GRAPH_APPLY_POSE alone on every request the call is stream-ordered with no host synchronisation.  With
 *   ALOAM_GRAPH_APPLY_MAP it SYNCHRONISES the context's stream where aloam_graph_export_map does (its transform, group and filter passes
 *   run into internal scratch) and once more behind the filter, to size the pools from the filtered counts.  Keyframe points never pass
 *   through host memory.  Meant to be called once per loop closure.
 * Afterwards the sequence's submap grids are built anew, aloam_score_map_corrections is ALOAM_E_STATE until its next frozen step and the
 *   pose information of its last mapping solve is gone (ALOAM_INFO_NONE).  The stored places (aloam_places_*) keep their old-frame poses:
 *   after an apply a place's pose is to be taken from its node.
 * dst[i] belongs to req[i]; its bits, and everything written for a sequence, do not depend on n, on the position in the list or on the
 *   other requests. */
enum { ALOAM_GRAPH_APPLY_POSE = 1, ALOAM_GRAPH_APPLY_MAP = 2 };
enum { ALOAM_GRAPH_APPLIED = 0, ALOAM_GRAPH_APPLY_NO_NODES = 1, ALOAM_GRAPH_APPLY_NO_ROOM = 2 };
typedef struct aloam_graph_apply_request {    /* 16 bytes: the map is made of nodes [first, first + count) of sequence seq              */
  int seq, first, count, flags;               /* flags: ALOAM_GRAPH_APPLY_POSE, or ALOAM_GRAPH_APPLY_POSE | ALOAM_GRAPH_APPLY_MAP       */
} aloam_graph_apply_request;
typedef struct aloam_graph_apply_result {     /* 104 bytes                                                                              */
  int status;                                 /* ALOAM_GRAPH_APPLIED, ALOAM_GRAPH_APPLY_NO_NODES or ALOAM_GRAPH_APPLY_NO_ROOM           */
  int nodes;                                  /* K: the nodes the sequence held, all rebased                                            */
  int cen[3];                                 /* the window centre afterwards (NO_ROOM: the one that did not fit)                       */
  int cubes[2], points[2];                    /* with MAP: non-empty cubes and points of the new window, corner / surf; else 0          */
  int raw_points[2];                          /* with MAP: keyframe points that went into the map of the listed nodes                   */
  int outside_window;                         /* with MAP: filtered points of tiles that lie outside the window                         */
  double q_corr[4], t_corr[3];                /* D (identity rotation for NO_NODES)                                                     */
} aloam_graph_apply_result;
int aloam_graph_apply(aloam_ctx* ctx, const aloam_graph_apply_request* req, int n, aloam_graph_apply_result* dst /* [n] */);

/* ---- loop edges measured on the device: batched keyframe registration -------------------------------------------------------------------
 * aloam_places_match finds a revisit and aloam_graph_add_edges consumes a loop edge; this section measures it.  One stream-ordered call
 * registers the clouds of node j against a local target made of the clouds of nodes [first, first + count) of the same sequence and returns
 * the edge (i, j, Z, info) ready for aloam_graph_add_edges.  It uses neither the atlas nor a sequence slot, touches no live sequence and
 * does not synchronise the host.  Opt-in and beside the reference: a context that never calls aloam_graph_loops_enable launches exactly
 * what it launched before.  a-loam_amd/loopreg.py restates the definition in numpy; DESIGN.md §7n.
 *
 * For a request (seq, i, j, first, count, pose, guess q, t), every f64 operation separately rounded:
 *   - X_k is node k's entered pose (q, t) or its estimate (q_opt, t_opt), chosen by pose.  Every target node k gets T_k = X_i^-1 o X_k as
 *     this header defines a relative pose, q_d = conj(q_i) q_k, t_d = conj(q_i) (t_k - t_i); node i goes through the same arithmetic.
 *   - per class the points of nodes first .. first + count - 1, in node order, then point order, become associate-to-map(p, T_k) (f64
 *     rotation and translation, stored to f32, intensity kept); the class's whole target cloud is filtered once with pcl::VoxelGrid (leaf
 *     mapping_line_resolution / mapping_plane_resolution, always the input-order sum, as in aloam_graph_export_map).  The target lives in
 *     the frame of node i: its coordinates are tens of metres however far the drive has gone.
 *   - the gate of src/laserMapping.cpp:554: the filtered corner target must hold more than 10 points and the surf target more than 50,
 *     else ALOAM_LOOP_TARGET_TOO_SMALL and Z is the guess.
 *   - the source is node j's two clouds as stored; `parameters` = the guess; then outer_iterations rounds of exactly what
 *     aloam_mapping_step does between its grid build and transformUpdate (the same kernels): associate-to-map of every source point, the
 *     five nearest by (f32 distance, index in the filtered target) all closer than 1 m, the line test and the plane fit, and the
 *     Levenberg-Marquardt solve with lm_max_iterations over LidarEdgeFactor / LidarPlaneNormFactor, HuberLoss(0.1); a FAILURE restores the
 *     round's entry pose.  These are the REQUEST's options, not the context's.
 *   - Z = the final `parameters`, the pose of node j in the frame of node i.  One more evaluation of the last round's records at Z gives
 *     the factor counts, the cost and info_left = J^T J in radians and metres, in the LEFT tangent of aloam_pose_information
 *     (q <- exp(theta / 2) q, t <- t + dt).
 *   - the graph's residual perturbs Z on the RIGHT (q_Z exp(phi / 2), t_Z + R_Z tau), so theta = R_Z phi, dt = R_Z tau and
 *     info = T^T info_left T with T = blockdiag(R_Z, R_Z): that is what an aloam_graph_edge wants.  Both are upper triangles, 21 doubles.
 * status: ALOAM_LOOP_OK; ALOAM_LOOP_NO_CLOUDS - node j or every target node was kept without clouds; ALOAM_LOOP_TARGET_TOO_SMALL;
 *   ALOAM_LOOP_TOO_LARGE - the raw target of a class exceeds the enabled capacity (decided on the device, where the counts are);
 *   ALOAM_LOOP_SOLVE_FAILED - the last round ended in FAILURE or info_left is not positive definite (no factor at all included).  With
 *   every status but ALOAM_LOOP_OK Z is the guess and info, info_left are zero.  Whether an ALOAM_LOOP_OK edge is a GOOD loop is the
 *   caller's decision, from the counts, the cost and the information; enter it with ALOAM_GRAPH_EDGE_ROBUST.
 *
 * aloam_graph_loops_enable(ctx, max_requests, max_target_corner_points, max_target_surf_points): once per context, after
 *   aloam_graph_keyframes_enable, else ALOAM_E_STATE.  1 <= max_requests <= 32768, capacities in 1 .. 2^24, else ALOAM_E_ARG; nothing
 *   stays allocated behind a refusal.  Allocates the scratch of max_requests slots (raw and filtered target, search grid, source copy,
 *   neighbours, factor records, and a voxel-filter scratch of its own); when the device or the pinned memory for it cannot be had, or the
 *   runtime refuses an event or the grid kernel's LDS size, it is ALOAM_E_HIP with the cause named by aloam_last_error, and again nothing
 *   stays allocated.  Every other call of this section is ALOAM_E_STATE before it.
 * aloam_graph_register_loops: req is host memory, read during the call; everything is checked before anything is queued, ALOAM_E_ARG with
 *   nothing changed: seq in range; count >= 1 and [first, first + count) inside the sequence's nodes; first <= i < first + count; j a
 *   node outside [first, first + count); pose 0 or 1; the guess finite and unit to 1e-6 (stored normalised, as aloam_graph_add_edges
 *   does); outer_iterations >= 1, lm_max_iterations >= 0 (opt NULL = the defaults); dst device memory of the context's device or pinned
 *   host memory, 8-byte aligned (classified like the exports).  n = 0 is ALOAM_OK.  A sequence, and a (seq, i, j), may be listed more than
 *   once.  Stream-ordered, no host synchronisation, like aloam_graph_optimize: the requests go through a pinned staging ring, and
 *   n > max_requests runs in rounds over the same scratch.  dst[r] belongs to req[r]; its bits do not depend on n, on the position in
 *   the list, on the round or on the other requests.
 * aloam_graph_loop_export_target (below, with the intermediate arrays): the filtered target of a scratch slot as the last call left it. */
enum { ALOAM_LOOP_OK = 0, ALOAM_LOOP_NO_CLOUDS = 1, ALOAM_LOOP_TARGET_TOO_SMALL = 2, ALOAM_LOOP_TOO_LARGE = 3, ALOAM_LOOP_SOLVE_FAILED = 4 };
typedef struct aloam_graph_loop_request {     /* 96 bytes                                                                               */
  int seq, i, j;                              /* the edge: node j measured in the frame of node i                                       */
  int first, count;                           /* the target: nodes [first, first + count), i among them, j not                          */
  int pose;                                   /* ALOAM_GRAPH_POSE_ENTERED or ALOAM_GRAPH_POSE_OPTIMIZED: which poses place the target   */
  int pad[2];
  double q[4], t[3];                          /* the guess of Z                                                                         */
  double reserved;
} aloam_graph_loop_request;
typedef struct aloam_graph_loop_options {     /* 8 bytes                                                                                */
  int outer_iterations;                       /* 2: the reference's mapping value (src/laserMapping.cpp:562)                            */
  int lm_max_iterations;                      /* 4: the reference's mapping value (:711)                                                */
} aloam_graph_loop_options;
typedef struct aloam_graph_loop_result {      /* 448 bytes                                                                              */
  int status;                                 /* ALOAM_LOOP_OK ..                                                                       */
  int n_line, n_plane;                        /* factors of the evaluation at Z                                                         */
  int lm_iterations, lm_termination;          /* of the last round                                                                      */
  int pad;
  int target_points[2], target_raw[2];        /* the target after and before the filter: corner, surf                                   */
  int source_points[2];                       /* node j's clouds                                                                        */
  double cost;                                /* 1/2 sum rho at Z                                                                       */
  double q[4], t[3];                          /* Z                                                                                      */
  double info[21];                            /* the edge's information (right tangent of Z), upper triangle, order (theta_x .. t_z)    */
  double info_left[21];                       /* the registration's (left tangent, as aloam_pose_information)                           */
} aloam_graph_loop_result;
void aloam_graph_loop_default_options(aloam_graph_loop_options* opt);
int aloam_graph_loops_enable(aloam_ctx* ctx, int max_requests, int max_target_corner_points, int max_target_surf_points);
int aloam_graph_register_loops(aloam_ctx* ctx, const aloam_graph_loop_request* req, int n, const aloam_graph_loop_options* opt,
                               aloam_graph_loop_result* dst /* [n] */);

/* ---- a pose grid searched around a loop guess ---------------------------------------------------------------------------------------------
 * aloam_graph_register_loops converges from a guess inside the registration's basin: a source point is kept only when its fifth neighbour
 * lies within 1 m, so the basin is a few decimetres and a few degrees.  A place match gives the guess to 6 degrees of yaw and puts the
 * sweep AT the stored place; a revisit in the other lane, or after metres of drift, is metres off, and the registration then ends
 * somewhere with status ALOAM_LOOP_OK.  aloam_graph_search_loops searches a grid of poses around every request's guess first, scores each
 * node by what the registration's first association would count from it, and runs the registration from the best node: one stream-ordered
 * call, no host synchronisation.  Opt-in and beside the reference: aloam_graph_register_loops keeps its behaviour and its launches, and a
 * context that never calls aloam_graph_search_loops allocates and launches exactly what it did before.  a-loam_amd/loopreg.py restates the
 * definition as search_grid() / search_best(); DESIGN.md §7q.
 *
 * For a request (seq, i, j, first, count, pose, guess q_g, t_g) and a grid (radius_m, step_m, yaw_deg, yaw_step_deg); every f64
 * operation is separately rounded:
 *   - axes: m = floor(radius_m / step_m + 1e-9), or 0 when step_m == 0; a = floor(yaw_deg / yaw_step_deg + 1e-9), or 0 when
 *     yaw_step_deg == 0.  K = (2a + 1)(2m + 1)^2 nodes, yaw outermost, then y, then x: node (ix, iy, iyaw), each index symmetric about 0,
 *     has index ((iyaw + a)(2m + 1) + (iy + m))(2m + 1) + (ix + m).
 *   - a node's pose: dx = ix * step_m, dy = iy * step_m, dyaw = iyaw * yaw_step_deg.  Z is the pose of node j in the frame of node i; the
 *     node turns the guess about the z axis of node i's frame through the guessed sensor position, then shifts it along node i's x and
 *     y: q_c = dq q_g (Hamilton product) with dq = (0, 0, sin h, cos h), h = (dyaw * (pi / 180)) / 2, and t_c = t_g + (dx, dy, 0).  For
 *     iyaw == 0 the quaternion is q_g itself and a zero offset leaves its coordinate untouched: the centre node is the guess bit for bit.
 *     Roll, pitch and z are not searched.  sin h and cos h are computed on the host (the C library's sin / cos) and reach the kernel as a
 *     table, so a model that calls the same library scores the same poses bit for bit; hence a <= 31.
 *   - a score: the aloam_map_score of aloam_score_map_corrections taken at `parameters` = (q_c, t_c) directly (a slot has no odometry
 *     frame, so there is no transformAssociateToMap).  For every source point - node j's two clouds as stored - associate-to-map, the five
 *     nearest in the filtered target by (f32 distance, index), all closer than 1 m, the line test or the plane fit, and each valid
 *     factor's residual under HuberLoss(0.1) at that pose.  The counts are those of round 0 of a registration started from that node, as
 *     integers.
 *   - ranking: the rule of aloam_score_map_corrections - most corner_factors + surf_factors, then the lower cost (NaN ranks as
 *     +infinity), then the lower index - with one addition: if the winner has zero factors, the centre node (the guess) is taken, not
 *     index 0, which is a corner of the grid.
 *   - registration: `parameters` := the best node's pose; everything after that is aloam_graph_register_loops as it is (outer_iterations
 *     rounds, the evaluation, the information).  For every status but ALOAM_LOOP_OK, Z in the loop result is still the request's guess.
 *   - skipped: a slot whose status before the solve is not ALOAM_LOOP_OK (NO_CLOUDS, TOO_LARGE, TARGET_TOO_SMALL) is not searched: best =
 *     -1, zero scores, q, t equal to the guess.
 * The request checks are those of aloam_graph_register_loops.  search NULL = the defaults; its values finite and >= 0, a <= 31 and
 * 1 <= K <= 2^14, else ALOAM_E_ARG.  search_dst [n] and scores ([n][K], may be NULL) are device memory of the context's device or pinned
 * host memory, 8-byte aligned, classified like dst.  Everything is checked before anything is queued; n = 0 is ALOAM_OK; ALOAM_E_STATE
 * before aloam_graph_loops_enable.  A round holds at most min(max_requests, 2^18 / K) requests.  The search scratch (32 bytes x 4 per
 * request and node of a round) is allocated by the first call that needs it and grown by a larger one; when that fails it is ALOAM_E_HIP
 * and nothing of it stays allocated.
 * Determinism: a node's score, best, and every bit of dst[r] and search_dst[r] do not depend on n, on the position in the list, on the
 * round, on the other requests or on the rest of the grid; a node's score depends only on its pose and the slot's clouds.  Counts are
 * integer sums; the cost is summed in a fixed order that depends on the source clouds alone; no floating-point atomics.  With a grid of
 * one node (radius_m = yaw_deg = 0) dst is byte for byte what aloam_graph_register_loops writes for the same requests. */
typedef struct aloam_graph_loop_search {        /* 32 bytes: the grid around every request's guess */
  double radius_m, step_m, yaw_deg, yaw_step_deg;
} aloam_graph_loop_search;
typedef struct aloam_graph_loop_search_result { /* 160 bytes */
  int status;                 /* the plan / gate status the search saw (ALOAM_LOOP_*) */
  int nodes, best;            /* K; index of the node taken, -1 when nothing was searched */
  int ix, iy, iyaw;           /* its grid indices */
  int pad[2];
  double q[4], t[3], reserved;              /* the pose the registration started from */
  aloam_map_score best_score, guess_score;  /* of that node and of the centre node */
} aloam_graph_loop_search_result;
void aloam_graph_loop_default_search(aloam_graph_loop_search* s);   /* 3.0, 0.5, 12.5, 2.5 (relocalize()'s steps) */
int aloam_graph_search_loops(aloam_ctx* ctx, const aloam_graph_loop_request* req, int n, const aloam_graph_loop_search* search,
                             const aloam_graph_loop_options* opt, aloam_graph_loop_result* dst /* [n] */,
                             aloam_graph_loop_search_result* search_dst /* [n] */, aloam_map_score* scores /* [n][K] or NULL */);

/* ---- pose-graph marginals: the covariance of an edge's residual under the graph, and its chi-square --------------------------------------
 * aloam_graph_register_loops measures a loop edge; whether it is a GOOD loop is decided here.  s = r^T Omega r is not the test: after a
 * long drive the graph's own uncertainty about X_i^-1 o X_j dominates a correct edge's residual.  The test is the innovation
 * chi2 = r^T (Sigma_r + Omega^-1)^-1 r against a 6-dof quantile (22.46 at p = 0.999), with Sigma_r the covariance of the residual under the
 * graph alone.  One stream-ordered call computes it for a list of candidate edges, one workgroup each.  It reads the graphs and writes
 * nothing in them.  Opt-in and beside the reference: a context that never calls aloam_graph_marginals launches exactly what it launched
 * before.  a-loam_amd/posegraph.py restates the definition as marginals(); DESIGN.md §7p.
 *
 * For a request (edge = a candidate (seq, i, j, Z, Omega), mode), everything read on the device at that point of the stream:
 *   - the linearisation point is the sequence's current estimates (q_opt, t_opt).  H = sum rho'_e J_e^T Omega_e J_e over the sequence's
 *     edges, as aloam_graph_optimize builds it: node 0 fixed, edges flagged ALOAM_GRAPH_EDGE_ROBUST weighted by rho' at huber_delta, no
 *     Levenberg-Marquardt damping.  H is positive definite whenever the graph has two nodes or more: the odometry chain ties every node to
 *     node 0 with positive-definite information.
 *   - r, J_i, J_j are the candidate's residual and Jacobians of the section "pose graphs" at the estimates; J_i is zero for i = -1 and the
 *     block of node 0 is zero.  The candidate is never robustified (its flags are validated and ignored).
 *   - Sigma_r = J H^-1 J^T, J = [J_i J_j]: six solves H y_c = (J^T)_c by the chain-preconditioned conjugate gradients of
 *     aloam_graph_optimize from y = 0, one after the other; Sigma_r[:, c] = J_i y_c[i] + J_j y_c[j], symmetrised as (M + M^T) / 2.  It is
 *     the covariance, under the graph alone, of r = (2 q_E.xyz, t_E): to first order the RIGHT tangent of Z, the one aloam_graph_edge.info
 *     lives in.  A column whose right-hand side is zero (i = -1, j = 0) takes 0 iterations and is no failure.
 *   - ALOAM_GRAPH_MARGINAL_MEASURED: Z and Omega as given.  s_edge = r^T Omega r; chi2 = r^T (Sigma_r + Omega^-1)^-1 r, by one thread:
 *     Omega^-1 from a Cholesky factor of Omega, S = Sigma_r + Omega^-1 factored with every pivot above 1e-12 of its diagonal entry,
 *     chi2 = |L_S^-1 r|^2.  With Sigma_r = 0, chi2 is s_edge.
 *   - ALOAM_GRAPH_MARGINAL_AT_ESTIMATE: Z := X_i^-1 o X_j of the estimates (X_j for i = -1), as this header defines a relative pose; the
 *     request's q, t and info are ignored and not validated.  r is what the arithmetic leaves (about 1e-17); s_edge and chi2 are 0.
 *     Sigma_r is then the covariance of the relative pose of the two nodes, or of node j against the frame of the fixed node 0.
 * status: ALOAM_GRAPH_MARGINAL_OK; ..._NO_EDGES - fewer than two nodes, nothing computed; ..._NOT_CONVERGED - a column ended at
 *   pcg_max_iterations without meeting pcg_tolerance: everything is still written from what it had; ..._FAILED - a non-finite
 *   linearisation, a chain factorisation that fails, p^T A p <= 0, or S not positive definite: cov and chi2 are zeros.
 *   pcg_iterations: the total over the six columns.  nodes, edges: the counts used.  q, t: the Z the residual was taken against.
 * Options (opt = NULL: the defaults): pcg_max_iterations >= 1 per column (200); pcg_tolerance >= 0 and finite (1e-10, relative in the
 *   preconditioned norm); huber_delta > 0 and finite (1.0): else ALOAM_E_ARG.
 *
 * aloam_graph_marginals: req is host memory (pinned or pageable), read during the call; dst is device memory of the context's device or
 *   pinned host memory, 8-byte aligned (classified like the exports).  Everything is checked before anything is queued and nothing changes
 *   on a refusal: ALOAM_E_STATE before aloam_graph_enable; ALOAM_E_ARG for seq out of range, i or j out of range (-1 <= i < nodes,
 *   0 <= j < nodes, i != j), a mode that is neither of the two, and in MEASURED mode a Z or Omega that aloam_graph_add_edges would refuse
 *   (q stored normalised, as there).  n = 0 is ALOAM_OK.  Stream-ordered, no host synchronisation: the requests go through a pinned
 *   staging ring.  A (seq, i, j) may be listed any number of times.  dst[r] belongs to req[r]; its bits do not depend on n, on r, on the
 *   round or on the other requests.  Every request has a scratch row of its own (one linearisation of its sequence's graph: 200 doubles
 *   per node and 115 per edge of the largest graph listed); at most as many rows as fit 1 GiB are allocated, on first use, and at least
 *   one; more requests run in rounds over the same rows in stream order. */
enum { ALOAM_GRAPH_MARGINAL_MEASURED = 0, ALOAM_GRAPH_MARGINAL_AT_ESTIMATE = 1 };
enum { ALOAM_GRAPH_MARGINAL_OK = 0, ALOAM_GRAPH_MARGINAL_NO_EDGES = 1, ALOAM_GRAPH_MARGINAL_NOT_CONVERGED = 2, ALOAM_GRAPH_MARGINAL_FAILED = 3 };
typedef struct aloam_graph_marginal_request { /* 248 bytes                                                                              */
  aloam_graph_edge edge;                      /* the candidate: seq, i, j, Z = (q, t), info; flags 0 or ALOAM_GRAPH_EDGE_ROBUST, ignored */
  int mode;                                   /* ALOAM_GRAPH_MARGINAL_MEASURED or ALOAM_GRAPH_MARGINAL_AT_ESTIMATE                      */
  int pad;
} aloam_graph_marginal_request;
typedef struct aloam_graph_marginal_options { /* 24 bytes                                                                               */
  int pcg_max_iterations;                     /* 200, per column                                                                        */
  int pad;
  double pcg_tolerance;                       /* 1e-10, relative in the preconditioned norm                                             */
  double huber_delta;                         /* 1.0: the weight of the graph's robust edges, as aloam_graph_options.huber_delta        */
} aloam_graph_marginal_options;
typedef struct aloam_graph_marginal_result {  /* 440 bytes                                                                              */
  int status, mode;
  int seq, i, j;
  int pcg_iterations;                         /* the six columns together                                                               */
  int nodes, edges;                           /* of the sequence's graph, as used                                                       */
  double chi2, s_edge;
  double r[6];                                /* the candidate's residual at the estimates, order (theta_x .. t_z)                      */
  double q[4], t[3];                          /* Z: as given (normalised), or X_i^-1 o X_j of the estimates                             */
  double cov[36];                             /* Sigma_r, row-major, symmetric                                                          */
} aloam_graph_marginal_result;
void aloam_graph_marginal_default_options(aloam_graph_marginal_options* opt);
int aloam_graph_marginals(aloam_ctx* ctx, const aloam_graph_marginal_request* req, int n, const aloam_graph_marginal_options* opt,
                          aloam_graph_marginal_result* dst /* [n] */);

/* ---- graph records: save and load pose graphs with their keyframe clouds ---------------------------------------------------------------
 * A sequence record leaves the graph family out.  A graph record is its counterpart: the nodes and edges of one sequence's pose graph and,
 * when the keyframe store is enabled, every node's descriptor and clouds, in a position-independent byte layout, packed and unpacked on the
 * device.  Opt-in and beside the reference: a context that never calls the two functions launches exactly what it launched before, and
 * sequence records keep their format (ALOAM_SEQ_RECORD_VERSION is unchanged).  a-loam_amd/graph_records.py restates the format in numpy;
 * DESIGN.md §7r.
 *
 * Layout, every section a whole number of 16-byte units (nodes 128 bytes, edges 240, descriptors 16, points 16):
 *   header (128) | nodes[N] | edges[E] [ | descriptors[N] | corner points | surf points ] | zeros up to a multiple of 256.
 *   A descriptor is {first corner, first surf, count corner, count surf}: where the node's clouds lie in the two point sections.  The
 *   padding is written as zeros, so the bytes of a record depend on the graph alone, not on n, on the record's position in the list or on
 *   the other records.  The edges carry the saving slot in `seq`, as aloam_graph_export_edges returns them.  The keyframe part
 *   (ALOAM_GRAPH_PART_KEYFRAMES) is held exactly when the store is enabled; a node kept without clouds is saved as it is, its descriptor
 *   carrying the rows' fill positions with counts of 0.
 *
 * aloam_graph_save: records of the graphs of the n sequences seqs[0 .. n) (distinct, in range; an empty graph gives a record of a header),
 *   with the contract of aloam_save_sequences: queued on the context's stream with no host synchronisation and no read-back, holding the
 *   state at that point of the stream; dst and dst_offsets are device memory of the context's device or pinned host memory (classified
 *   like the exports' destinations, else ALOAM_E_ARG before anything is queued; dst may be NULL when cap_bytes is 0), dst 16-byte
 *   aligned.  dst_offsets[0 .. n] is always written, in bytes; a record is written whole, and only when it ends at or before cap_bytes;
 *   cap_bytes = 0 is the size query.  ALOAM_E_STATE before aloam_graph_enable.
 *
 * aloam_graph_load: record i of src (at [src_offsets[i], src_offsets[i + 1])) into slot slots[i], for n distinct slots; the offsets rise
 *   by whole records.  A record is position independent: listing its bytes once per slot forks a graph.  src and src_offsets may be
 *   device memory of the context's device, pinned host memory, or pageable host memory (staged through context scratch, so a record read
 *   from a file loads directly); src 16-byte aligned.  The call synchronises the context's stream once (offsets handed in as device
 *   memory are read back before, with a wait of their own).  Before that wait the records that the device cannot reach are staged and a
 *   check kernel runs over every record; the host then reads the n headers and one verdict per record, and everything is decided
 *   before anything of the context changes: a refused load changes nothing.
 *   - ALOAM_E_STATE: before aloam_graph_enable; a target slot whose graph is not empty (aloam_graph_clear it first).
 *   - ALOAM_E_ARG, the field named by aloam_last_error: magic, version, `bytes` different from the offsets' difference or from what the
 *     counts give, section sizes, parts other than what the context holds (the keyframe part if and only if the store is enabled), and,
 *     with the keyframe part, mapping resolutions other than the context's (the clouds are stacks filtered at those leaves).
 *   - ALOAM_E_CAPACITY: more nodes than max_nodes, more edges than max_edges, more points of a class than the keyframe row holds.
 *   - ALOAM_E_ARG with "payload" in the error text, decided by the check kernel: an edge outside -1 <= i < nodes, 0 <= j < nodes, i != j,
 *     or with a flag other than ALOAM_GRAPH_EDGE_ROBUST; descriptors that are not back to back from 0 (first[k] = first[k-1] + count[k-1],
 *     counts >= 0), or whose last one does not end at kf_points.  These are the values the solve and the gather kernels index with: a
 *     damaged file is refused before any of them runs.  The numeric payload (poses, measurements, information matrices, points) is
 *     trusted, as sequence records trust theirs; a record carries no checksum.
 *   The rest is asynchronous: the nodes, the edges with `seq` rewritten to the target slot, the descriptors, the points and the slot's
 *   two append cursors are written in stream order, and src must stay unchanged until aloam_synchronize or an event on aloam_stream.  The
 *   slot's count of nodes kept without clouds (aloam_graph_keyframe_info) is the slot's history and is left alone.  Batch, device,
 *   max_nodes, max_edges and the keyframe row sizes may differ from the saving context's.
 * Taken together: a sequence record and a graph record of the same sequence, saved at the same point of the stream and loaded into one
 *   slot of a compatible context, continue bit for bit - later aloam_graph_add_nodes (the odometry edge from the loaded last node),
 *   aloam_graph_add_edges, aloam_graph_optimize, aloam_graph_export_map, aloam_graph_apply, aloam_graph_register_loops /
 *   aloam_graph_search_loops and aloam_graph_marginals.  (After aloam_load_sequences a slot takes part in a mapping step before
 *   aloam_graph_add_nodes may keep its stacks, as after a reset.)
 * Profiling: the pack runs in the slot save_sequences and the unpack in load_sequences; aloam_profile_get's algorithmic bytes of those two
 *   slots keep describing the last sequence save / load, and a graph call's bytes are the offsets it returns. */
enum { ALOAM_GRAPH_RECORD_MAGIC = 0x52474c41, ALOAM_GRAPH_RECORD_VERSION = 1 };   /* magic: the bytes "ALGR" */
enum { ALOAM_GRAPH_PART_GRAPH = 1, ALOAM_GRAPH_PART_KEYFRAMES = 2 };
typedef struct aloam_graph_record_header {    /* first 128 bytes of a record                                                            */
  unsigned int magic;                         /* ALOAM_GRAPH_RECORD_MAGIC                                                               */
  unsigned int version;                       /* ALOAM_GRAPH_RECORD_VERSION                                                             */
  long long bytes;                            /* whole record, a multiple of 256                                                        */
  int parts;                                  /* ALOAM_GRAPH_PART_* held                                                                */
  int nodes, edges;
  int kf_points[2];                           /* points of the keyframe clouds, corner / surf; 0 without the keyframe part              */
  int seq;                                    /* the slot it was saved from (informational)                                             */
  unsigned int line_res_bits, plane_res_bits; /* mapping resolutions as IEEE-754 bits with the keyframe part, else 0                    */
  int node_bytes, edge_bytes, desc_bytes, point_bytes;   /* strides of the sections: 128, 240, 16, 16                                   */
  int pad[16];
} aloam_graph_record_header;
int aloam_graph_save(aloam_ctx* ctx, const int* seqs, int n, void* dst, long long cap_bytes, long long* dst_offsets /* [n + 1] */);
int aloam_graph_load(aloam_ctx* ctx, const int* slots, int n, const void* src, const long long* src_offsets /* [n + 1] */);

/* ---- the robust solve: graduated non-convexity over the flagged edges --------------------------------------------------------------------
 * The chi-square gate of aloam_graph_marginals judges a candidate against the graph's own covariance, which grows with drift; and the Huber
 * loss of aloam_graph_optimize does not redescend: a wrong loop edge that got in keeps pulling with constant force.
 * aloam_graph_optimize_robust solves a graph so that such edges end with no force at all: GNC-TLS, graduated non-convexity with a
 * truncated least-squares loss (Yang, Antonante, Tzoumas, Carlone, RA-L 2020; GTSAM's GncOptimizer), an outer loop of weighted
 * least-squares solves that runs inside one kernel, one workgroup per listed graph.  Opt-in and beside the reference: a context that never
 * calls it launches exactly what it launched before.  a-loam_amd/posegraph.py restates the definition as optimize_robust(); DESIGN.md §7s.
 *
 * Definition.  R = the edges flagged ALOAM_GRAPH_EDGE_ROBUST; s_e = r^T Omega r with the edge's own information; c2 = inlier_chi2.  The
 * weighted problem for weights w is the plain problem of the section "pose graphs" with Omega_e <- w_e Omega_e for e in R and every flag
 * cleared.  There is no Huber in this call: huber_delta is unused.
 *   1. s at the entry estimates; s_max = max over R.  A non-finite s_e or pose: ALOAM_GRAPH_FAILED with termination 5, nothing written back.
 *   2. R empty, or 2 s_max - c2 <= 0: GNC is skipped.  One weighted solve with w = 1; outer_iterations = 1, mu = 0, and every flagged edge
 *      counts as an inlier.
 *   3. Otherwise mu = c2 / (2 s_max - c2), and for it = 1 .. max_outer_iterations:
 *        thresholds, with s at the current estimates: lo = mu / (mu + 1) * c2, hi = (mu + 1) / mu * c2;
 *        weights: w_e = 1 if s_e <= lo, w_e = 0 if s_e >= hi, otherwise w_e = sqrt(c2 * mu * (mu + 1) / s_e) - mu;
 *        solve: the trust-region Levenberg-Marquardt of aloam_graph_optimize on the weighted problem, from the current estimates, with opt;
 *        stop after the solve of the first iteration in which every weight was exactly 0 or 1, otherwise mu *= mu_step.
 *   4. The estimates (q_opt, t_opt) are written back only if no inner solve ended as a failure; if one did, the call reports
 *      ALOAM_GRAPH_FAILED and leaves the estimates as they were.  An inner solve that accepts nothing is not a failure.
 *      ALOAM_GRAPH_NO_EDGES is reported as by aloam_graph_optimize.
 * A weight of 0 gives an edge no information at all, so what ties the nodes together must not be flagged: flag loop and anchor edges only,
 * and leave the odometry edges unflagged - they keep the chain positive definite.
 *
 * aloam_graph_optimize_robust: stream-ordered, no host synchronisation; nothing is queued on any error.  seqs, opt and dst are validated
 *   as in aloam_graph_optimize (ALOAM_E_STATE before aloam_graph_enable; distinct sequences in range; dst device memory of the context's
 *   device or pinned host memory).  robust = NULL: the defaults; max_outer_iterations >= 1, inlier_chi2 > 0 and finite, mu_step > 1 and
 *   finite, else ALOAM_E_ARG.  weights_dst may be NULL; otherwise it is classified like dst, as device or pinned memory, and
 *   weights_stride (in doubles) must be at least the largest edge count listed, else ALOAM_E_ARG.  Row i of weights_dst receives one double
 *   per edge of seqs[i]: 1.0 for unflagged edges, the final weight for flagged ones; entries beyond the edge count are not written.
 *   Every bit written for seqs[i] - the result, the weights and the exported nodes - is independent of n, of i and of the other
 *   sequences listed.
 *   The call changes only q_opt / t_opt: edges, flags, counts and the entered poses stay byte for byte, and nothing is stored between
 *   calls.  A later aloam_graph_optimize sees the graph exactly as entered, the rejected edges with their full information: a graph with
 *   rejected edges should keep being solved with the robust call.
 *   Scratch: beside the rows of aloam_graph_optimize (shared with it), n * row_edges * 256 B for the scaled copy of the edges, w and s,
 *   row_edges the largest edge count listed.  Timed under the profiling slot pose_graph. */
typedef struct aloam_graph_robust_options {   /* 32 bytes                                                                               */
  int max_outer_iterations;                   /* 100                                                                                    */
  int pad;
  double inlier_chi2;                         /* 22.46: c^2, the squared Mahalanobis distance beyond which an edge is an outlier
                                                 (the 6-dof chi-square quantile at p = 0.999, as the gate of aloam_graph_marginals)     */
  double mu_step;                             /* 1.4                                                                                    */
  double reserved;
} aloam_graph_robust_options;
typedef struct aloam_graph_robust_result {    /* 128 bytes                                                                              */
  aloam_graph_result solve;                   /* status; termination and gradient_max of the LAST inner solve; lm_iterations,
                                                 accepted_steps, pcg_iterations summed over all inner solves; initial_cost: all weights 1
                                                 at the entry estimates; final_cost: final weights at the final estimates               */
  int outer_iterations, robust_edges, inliers, outliers;   /* w == 1 / w == 0 among the flagged edges; the rest were undecided at the cap */
  double mu, s_max, truncated_cost;           /* last mu used (0: GNC skipped); largest flagged s at entry;
                                                 1/2 (sum_unflagged s + sum_flagged min(s, c^2)) at the end                             */
  double reserved[3];
} aloam_graph_robust_result;
void aloam_graph_robust_default_options(aloam_graph_robust_options* opt);
int aloam_graph_optimize_robust(aloam_ctx* ctx, const int* seqs, int n, const aloam_graph_options* opt, const aloam_graph_robust_options* robust,
                                aloam_graph_robust_result* dst /* [n] */, double* weights_dst /* [n][weights_stride] or NULL */, long long weights_stride);

/* ---- loop candidates by pose proximity -------------------------------------------------------------------------------------------------
 * aloam_places_match answers "which stored sweep looks like this one"; this section answers "which keyframes does the graph itself say I am
 * next to": a radius search over the positions of a sequence's own nodes, as the LOAM-family back ends propose loops (a radius and a
 * minimum age), for a batch of queries in one stream-ordered call.  It writes aloam_graph_loop_request records, guess and target window
 * filled in, ready for aloam_graph_search_loops / aloam_graph_register_loops: propose -> search and register -> gate -> add -> solve.  It
 * needs neither the place store nor the keyframe store.  Opt-in and beside the reference: a context that never calls it allocates nothing for
 * it and launches exactly what it launched before.  a-loam_amd/posegraph.py restates the definition as propose_loops(); DESIGN.md §7v.
 *
 * Definition of a query (seq, j), every f64 operation separately rounded:
 *   1. X_k is node k's entered pose (q, t) or its estimate (q_opt, t_opt), chosen by pose.
 *   2. The eligible nodes are i in [0, j - min_gap]; none when j < min_gap.
 *   3. For each eligible i: (dx, dy, dz) = t_i - t_j, d2 = (dx*dx + dy*dy) + dz*dz, r = (double)(j - i) * growth_m_per_node + radius_m;
 *      i is a hit when d2 <= r*r.  The growth term lets the radius follow the drift between two nodes far apart on the chain.
 *   4. Selection is greedy, at most K rounds: each round takes, among the hits still live, the one with the least (d2, i) - lower d2 first,
 *      then lower i - and removes every hit i' with |i' - i| <= separation (one pass by the same place fills many consecutive nodes; this
 *      keeps one candidate per pass).  counts[q] is the number taken.
 *   5. The record of the k-th node taken: seq, i, j and pose as given; first = max(0, i - half_window); count = i + half_window - first + 1;
 *      the guess (q, t) = X_i^-1 o X_j as this header defines a relative pose, q_d = conj(q_i) q_j, t_d = conj(q_i) (t_j - t_i); pad and
 *      reserved are zero.  dist2[q][k] = d2.
 *   6. Rows k >= counts[q] of dst are all-zero bytes and their dist2 entries are 0.0.  Every byte of dst[0 .. n*K) and of counts[0 .. n) is
 *      written (and of dist2[0 .. n*K) unless it is NULL); nothing outside them is written.
 *
 * aloam_graph_propose_loops: queries is host memory, n pairs (seq, j), read during the call; everything is checked before anything is
 *   queued, ALOAM_E_ARG with nothing changed: seq in range; 0 <= j < the sequence's nodes (host state); pose 0 or 1; radius_m and
 *   growth_m_per_node finite and >= 0; min_gap >= 1; 0 <= half_window < min_gap, so the window never reaches j, which
 *   aloam_graph_register_loops requires; separation >= 0; 1 <= K <= 16; dst, counts and dist2 (which may be NULL) device memory of the
 *   context's device or pinned host memory, classified like the exports, dst and dist2 8-byte aligned and counts 4-byte aligned.
 *   ALOAM_E_STATE before aloam_graph_enable.  n = 0 is ALOAM_OK.  A sequence, and a (seq, j), may be listed any number of times.
 *   Stream-ordered, no host synchronisation: the queries go through a pinned staging ring, and a large n runs in rounds.  The call reads
 *   the graph and writes nothing in it.  Every bit of a query's outputs is independent of n, of its position in the list, of the round and
 *   of the other queries.  Which edges the graph already holds is the caller's knowledge (it added them): posegraph.unclosed() drops the
 *   proposals next to one.  Timed under the profiling slot pose_graph. */
int aloam_graph_propose_loops(aloam_ctx* ctx, const int* queries /* [n][2]: seq, j */, int n, int pose,
                              double radius_m, double growth_m_per_node, int min_gap, int half_window, int separation, int K,
                              aloam_graph_loop_request* dst /* [n][K] */, int* counts /* [n] */, double* dist2 /* [n][K] or NULL */);

/* ---- trimming a graph in place: a sliding window over the keyframes -------------------------------------------------------------------------
 * The rows of aloam_graph_enable and aloam_graph_keyframes_enable are fixed; when they fill, aloam_graph_add_nodes returns ALOAM_E_CAPACITY or
 * keeps the node without clouds, and aloam_graph_clear throws the whole graph away.  aloam_graph_trim drops the oldest nodes of the listed
 * sequences on the device, compacts the node, edge, descriptor and point rows in place, and turns every constraint from a dropped node to a
 * kept one into an anchor edge with the same residual.  Everything behind it - the solves, the marginals, the proposal, the registration,
 * aloam_graph_export_map, aloam_graph_apply, aloam_graph_save / aloam_graph_load and the next aloam_graph_add_nodes - runs on the trimmed
 * graph unchanged: anchors (i = -1) and a fixed node 0 exist in every kernel.  Opt-in and beside the reference: a context that never calls
 * it allocates nothing for it and launches exactly what it launched before.  a-loam_amd/posegraph.py restates the definition as trim(),
 * a-loam_amd/graph_records.py the keyframe store's part as trim_keyframes(); the device reproduces them byte for byte.  DESIGN.md §7x.
 *
 * Definition, for one listed sequence; f = first[k] is the old index of the node that becomes node 0.
 *   Nodes.  Nodes [0, f) are dropped.  Old node n >= f becomes node n - f, a bit copy of its 128 bytes: entered pose, estimate, frame.  New
 *     node 0 (old f) is the node every solver holds fixed.  The trim conditions on the dropped nodes and on node f at their current
 *     estimates; it does not marginalise them: no dense prior among the kept nodes is formed, and what the dropped nodes' uncertainty would
 *     have added to the kept ones is not carried over.  Solve before trimming.
 *   Edges, in their stored order (a stable compaction), the first rule that applies:
 *     1. j > f and (i >= f or i == -1): kept.  i' = i - f (or -1), j' = j - f; Z, info and flags are bit copies.
 *     2. j > f and 0 <= i < f: anchored.  i' = -1, j' = j - f, Z' = X_opt[i] o Z, computed as (quat_mul(q_opt_i, q_Z),
 *        quat_rotate(q_opt_i, t_Z) + t_opt_i), every f64 operation rounded on its own; the result is stored as computed, not renormalised.
 *        info and flags are bit copies.  With X_i the identity, E = Z'^-1 o X_j is the old Z^-1 o X_i^-1 o X_j: residual, tangent, Huber
 *        weight and information are unchanged.
 *     3. i > f and j == f: kept, i' = i - f, j' = 0.
 *     4. i > f and 0 <= j < f: removed and counted as removed_reverse; no exact anchor form exists for it.  aloam_graph_add_nodes and
 *        aloam_graph_propose_loops only ever produce i < j.
 *     5. Everything else touches no node above f and is a constant of the problem: removed and counted as removed_fixed.
 *   Keyframe store, when enabled, per class: d = desc[f].first[cls] and m = cursor[cls] - d.  Points [d, d + m) move to [0, m); descriptor
 *     n >= f moves to n - f with first -= d, counts unchanged; the cursor becomes m.  The counters of nodes kept without clouds stay.
 *
 * aloam_graph_trim: seqs and first are host memory, read during the call.  out (plain host memory, may be NULL) receives per listed sequence
 *   {nodes, edges, anchored, removed_fixed, removed_reverse, corner points freed, surf points freed, 0} after the trim.  Checked before
 *   anything is queued, ALOAM_E_ARG with nothing queued and nothing changed: seqs distinct and in range; 0 <= first[k] < nodes of that
 *   sequence (host state), so a graph with 0 nodes admits no value; NULL lists with n > 0; n < 0.  first[k] == 0 is allowed and changes
 *   nothing in that sequence.  ALOAM_E_STATE before aloam_graph_enable.  n = 0 is ALOAM_OK.
 *   Stream-ordered behind what was queued before; the items go through a pinned staging ring.  The call then SYNCHRONISES the context's
 *   stream once, behind its kernels, as aloam_graph_export_map does: the edge counts are host state and the host holds no copy of the
 *   edge endpoints, so it reads back the eight integers per sequence and sets the counts (aloam_graph_info) from them.  Meant to be called
 *   once per many keyframes, not once per sweep.  What an application wants of the dropped part it takes first, with
 *   aloam_graph_export_map or aloam_graph_save.  A listed sequence's bytes do not depend on n, on its position in the list or on the other
 *   sequences; unlisted sequences are untouched.  Timed under the profiling slot pose_graph, with the rows moved as algorithmic bytes. */
int aloam_graph_trim(aloam_ctx* ctx, const int* seqs, const int* first, int n, int* out /* [n][8] or NULL */);

/* ---- joined graphs: links between sequences and a joint solve ------------------------------------------------------------------------------
 * Every call above stops at the boundary of one sequence: an aloam_graph_edge carries one seq, aloam_graph_optimize solves one graph per
 * workgroup.  This section joins sessions: a link is a measurement between a node of one sequence and a node of another, a group is a set
 * of sequences (its members) with the links among them, and a joint solve optimises a group as ONE graph in one frame - a fleet on one
 * site, the same vehicle on different days - so that two sessions correct each other.  The joined graph is laid out in scratch rows and
 * solved by the kernels of aloam_graph_optimize / aloam_graph_optimize_robust as they are; what is new is the gather, the alignment and the
 * write-back.  Opt-in and beside the reference: a context that never calls it allocates nothing for it and launches exactly what it launched
 * before.  a-loam_amd/posegraph.py restates the definition as join(), align_member(), split() and optimize_joint(); DESIGN.md §7y.
 *
 * The links are NOT STORED.  The host owns them, as it owns loop requests, and passes them on every call; no record of a sequence changes
 * shape.  After an aloam_graph_trim of a member at `first` the host shifts its own link indices of that member by -first and drops the
 * links whose node was dropped.
 *
 * The joined graph of a group.
 *   Nodes: the members' rows laid end to end in member order, as bit copies; off[m] is the sum of the node counts of the members before m.
 *   Edges, first part: every member's edges in member order and stored order, with i >= 0 shifted by off[m] and j shifted by off[m];
 *     anchors keep i = -1; seq, Z, info and flags are bit copies.
 *   Edges, second part: the group's links in list order as edges (off[seq_i] + i, off[seq_j] + j, Z, info, flags) with seq = seq_i.
 *   This edge order is also the order of weights_dst.
 *   Joined node 0, which is node 0 of the group's first member, is the fixed one; every other member's node 0 is free.
 * Alignment.  align[m] != 0 (never for the first member of a group) says that this member's estimates and anchors are still in its own
 *   frame; it is moved into the group's frame before the solve.  The member's tree link is the first link, in the group's list order, that
 *   joins it to a member earlier in the group's member list.  If the member is the seq_j side, A = (Xg[seq_i][i] o Z) o X[j]^-1; if it is
 *   the seq_i side, A = (Xg[seq_j][j] o Z^-1) o X[i]^-1.  X is the member's own estimate, Xg the earlier member's estimate as placed in
 *   the joined row, so chains of newly joined members work.  compose(a, b) = (quat_mul(q_a, q_b), quat_rotate(q_a, t_b) + t_a) and
 *   inverse(a) = (q*, -quat_rotate(q*, t)), every f64 operation rounded on its own; q_A is then divided by its norm (the squares summed
 *   in index order): the estimates it is built from are chained products that nothing renormalises, and A must be a rigid transform.
 *   Nothing else is renormalised.  Every node's (q_opt, t_opt)
 *   becomes A o X_opt; every anchor edge of the member becomes Z' = A o Z with residual, information and flags unchanged (a left
 *   multiplication of both cancels in Z^-1 o X_j); q, t, frame and relative edges are untouched.  Alignment is applied ONCE, when a
 *   sequence first joins: aligning a member again re-composes its anchors and its estimates with a transform that is then close to, but
 *   not exactly, the identity.  With align NULL or all zeros the gather is a pure copy.
 * Write-back.  After the solve every member's q_opt / t_opt are the joined row's, and an aligned member's anchors hold Z' - whatever the
 *   solve's status, except ALOAM_GRAPH_NO_EDGES (fewer than two joined nodes or no joined edge), where nothing is written.  From then on
 *   the member's estimates live in the group's frame and the existing calls run on it unchanged: aloam_graph_add_nodes (the next node is
 *   X_opt[k-1] o Z), aloam_graph_trim, aloam_graph_export_map, aloam_graph_apply, and a solo aloam_graph_optimize.
 *
 * aloam_graph_optimize_joint / aloam_graph_optimize_joint_robust: members (sequence indices), align (may be NULL), links and groups are host
 *   memory, read during the call.  groups[g] = {member_first, member_count, link_first, link_count} indexes members / align and links.
 *   dst receives one result per group, weights_dst (may be NULL) the final weights of a group's joined edges at
 *   weights_dst[g * weights_stride + e].  Options and results are those of aloam_graph_optimize / aloam_graph_optimize_robust.
 *   Checked before anything is queued, ALOAM_E_ARG with nothing queued and nothing changed, the field named in aloam_last_error: members in
 *   range and distinct over the whole call; the groups tile members and links contiguously and in order; member_count >= 1 and every
 *   member holds at least one node; align of a group's first member is 0; a link's two sequences are distinct members of the link's own
 *   group; its node indices lie inside the members' counts; q, t, info, flags by the rules of aloam_graph_add_edges (q is stored
 *   normalised); every member after the first has a link to an earlier member of its group (the gauge, and the tree link); a group's
 *   summed nodes do not exceed 2^20 and its summed edges plus links 2^22; the options as for the per-sequence solves; dst and weights_dst
 *   device memory of the context's device or pinned host memory; weights_stride at least the largest joined edge count; NULL lists;
 *   negative counts.  ALOAM_E_STATE before aloam_graph_enable.  n_groups = 0 is ALOAM_OK.
 *   Stream-ordered, no host synchronisation: one pinned staging ring, three launches (gather, the solve, scatter), one workgroup per
 *   group in the first two, so a group costs what one graph of the summed size costs.  (A call whose lists outgrow the ring, or whose
 *   groups outgrow the joined rows, waits for the stream once while they are rebuilt.)  Scratch: the joined rows, n_groups x the largest
 *   group, beside the rows of the solve.  The bits of a group's result and of its members' rows do not depend on the other groups, on the
 *   group's position or on n_groups; sequences that are no member are untouched.  A group of one member with no links is byte for byte
 *   aloam_graph_optimize (or aloam_graph_optimize_robust) of that sequence.  Timed under the profiling slot pose_graph. */
struct aloam_graph_link {                     /* 256 bytes                                                                              */
  int seq_i, i, seq_j, j;                     /* node j of seq_j measured in the frame of node i of seq_i; seq_i != seq_j               */
  int flags, pad[3];                          /* 0 or ALOAM_GRAPH_EDGE_ROBUST                                                           */
  double q[4], t[3];                          /* Z                                                                                      */
  double info[21];                            /* as aloam_graph_edge.info (right tangent of Z)                                          */
};
typedef struct aloam_graph_link aloam_graph_link;
struct aloam_graph_joint_group {              /* 16 bytes                                                                               */
  int member_first, member_count, link_first, link_count;
};
typedef struct aloam_graph_joint_group aloam_graph_joint_group;
int aloam_graph_optimize_joint(aloam_ctx* ctx, const int* members, const int* align /* [n_members] or NULL */, int n_members,
                               const aloam_graph_link* links, int n_links, const aloam_graph_joint_group* groups, int n_groups,
                               const aloam_graph_options* opt, aloam_graph_result* dst /* [n_groups] */);
int aloam_graph_optimize_joint_robust(aloam_ctx* ctx, const int* members, const int* align /* [n_members] or NULL */, int n_members,
                                      const aloam_graph_link* links, int n_links, const aloam_graph_joint_group* groups, int n_groups,
                                      const aloam_graph_options* opt, const aloam_graph_robust_options* robust,
                                      aloam_graph_robust_result* dst /* [n_groups] */, double* weights_dst /* [n_groups][weights_stride] or NULL */,
                                      long long weights_stride);

/* ---- the map of joined sequences ---------------------------------------------------------------------------------------------------------------
 * aloam_graph_optimize_joint puts the estimates of several sequences into one frame; aloam_graph_export_map still builds a map from the
 * nodes of ONE sequence, so two sessions that share a frame come out as two maps, with every (cube, class) they both reach present twice
 * and filtered twice.  This call makes the one map: tiles from the keyframes of several sequences, every (cube, class) filtered once over
 * all of its members.  Opt-in and beside the reference: a context that never calls it allocates nothing for it and launches exactly what
 * it launched before, and aloam_graph_export_map queues exactly the launches it queued before.  a-loam_amd/atlas.py (tiles_from_parts)
 * restates the definition; DESIGN.md §7za.
 *
 * A part is nodes [first, first + count) of sequence seq under a frame; a group is a run of parts, in the caller's order, with one choice of
 * pose.  The call reads no group membership and nothing about joins is stored on the device: a part is any node range of any sequence, a
 * sequence may appear in several parts and in several groups, ranges may overlap, count = 0 is allowed.
 *
 * The map of group g is the map aloam_graph_export_map defines, made of the concatenation of its parts' nodes in part order, nodes in node
 * order inside each part: every point through associate-to-map with its node's pose X_k ((q, t) or (q_opt, t_opt), by the group's pose),
 * the cube of the result, the members of a (cube, class) in that order, one pcl::VoxelGrid pass with the class's leaf and the input-order
 * sum - always, also when only one node contributes -, corner tiles first, then surf tiles, each ascending in cube, frame 0; points whose
 * cube lies outside -512 .. 511 on some axis are left out and counted.  Offsets, both caps and the size query, written, raw_points and
 * outside, the single synchronisation after the transform pass, the growing directory and the growing pools are those of
 * aloam_graph_export_map with "request" read as "group": dst_offsets[0 .. n_groups] holds the tile offsets, dst_offsets[n_groups + 1 ..
 * 2 n_groups + 1] the point offsets.
 * Frames.  frame = -1: the part's poses are used as stored, no arithmetic is applied, the bits are X_k's.  frame = f >= 0: X_k' = A o X_k
 *   with A = frames[f] = (q_A xyzw, t_A), the compose of the joined-graphs section: q' = quat_mul(q_A, q_k), t' = quat_rotate(q_A, t_k) + t_A,
 *   every f64 operation rounded on its own, nothing renormalised.  Use -1 for members that a joint solve has already aligned, an index for
 *   a session that is not aligned yet (A from a first link, as in aloam_graph_propose_links).
 * The bytes written for a group do not depend on n_groups, on its position, on the other groups or on the directory's size.  A group of one
 *   part with frame = -1 is byte for byte aloam_graph_export_map of (seq, first, count, pose); a group whose parts are adjacent ranges of
 *   one sequence ([a, b) then [b, c), frame = -1) is the group of the single part [a, c).
 * Checked before anything is queued, ALOAM_E_ARG with nothing changed and the field named in aloam_last_error: seq in range; 0 <= first,
 *   0 <= count, first + count <= the sequence's nodes; frame in [-1, n_frames); frames finite with q_A unit to 1e-6; pose 0 or 1 and pad 0;
 *   the groups tile parts contiguously and in order; part_count >= 0; n_groups <= 32768; NULL lists and negative counts; the destinations
 *   as for the exports.  ALOAM_E_STATE before aloam_graph_keyframes_enable.  n_groups = 0 is ALOAM_OK, with the offsets written.  A
 *   (group, class) whose parts are bounded, on the host, by more than 65536 pieces of 4096 points is ALOAM_E_CAPACITY before anything is
 *   queued, with the group named.  Timed under the profiling slot graph_map. */
struct aloam_graph_map_part {                 /* 16 bytes: nodes [first, first + count) of sequence seq                                 */
  int seq, first, count, frame;               /* frame: -1 = the poses as stored, else an index into frames                             */
};
typedef struct aloam_graph_map_part aloam_graph_map_part;
struct aloam_graph_map_group {                /* 16 bytes: parts [part_first, part_first + part_count) make one map                     */
  int part_first, part_count, pose, pad;      /* pose: ALOAM_GRAPH_POSE_ENTERED or ALOAM_GRAPH_POSE_OPTIMIZED; pad: 0                   */
};
typedef struct aloam_graph_map_group aloam_graph_map_group;
int aloam_graph_export_map_joint(aloam_ctx* ctx, const aloam_graph_map_part* parts, int n_parts,
                                 const double* frames /* [n_frames][7] or NULL */, int n_frames,
                                 const aloam_graph_map_group* groups, int n_groups,
                                 aloam_map_tile* tiles_dst, long long cap_tiles,
                                 float* points_dst_xyzw, long long cap_points,
                                 long long* dst_offsets /* [2][n_groups + 1] */,
                                 aloam_graph_map_stats* stats_dst /* [n_groups] or NULL */);

/* ---- links measured on the device: register, search and propose between sequences ----------------------------------------------------------
 * aloam_graph_optimize_joint consumes links; this section measures them.  The chain propose -> search and register -> gate -> link ->
 * joint solve runs between two sequences with the same stream-ordered, batched calls that run it inside one: no atlas, no spare sequence
 * slot, no host synchronisation.  Opt-in and beside the reference: a context that never calls a function of this section allocates and
 * launches exactly what it launched before, and aloam_graph_register_loops / aloam_graph_search_loops / aloam_graph_propose_loops queue
 * exactly the launches they queued before.  a-loam_amd/posegraph.py (propose_links, frame_from_link) and a-loam_amd/loopreg.py
 * (link_request, link_from_result) restate the definitions; DESIGN.md §7z.
 *
 * A link request names a frame (node i of seq_i), a target (nodes [first, first + count) of seq_i, i among them), a source (node j of
 * seq_j, seq_j != seq_i) and a guess of Z, the pose of node j of seq_j in the frame of node i of seq_i.  The guess sits at byte 32, as in
 * aloam_graph_loop_request.
 *
 * aloam_graph_register_links(ctx, req, n, opt, dst) writes aloam_graph_loop_result dst[n].  Its definition is that of
 *   aloam_graph_register_loops, word for word, with two substitutions: the target is built from seq_i's nodes, descriptors and point rows
 *   (X_k, T_k = X_i^-1 o X_k and the poses chosen by `pose` are seq_i's), and the source is node j's two clouds from seq_j's rows.  No pose
 *   of seq_j is read: the two sessions need not share a frame, because the guess carries everything about their relation.  The statuses
 *   (ALOAM_LOOP_NO_CLOUDS: node j of seq_j or every target node of seq_i was kept without clouds), the options, the result record, the
 *   rounds of n > max_requests and the determinism clause (dst[r] does not depend on n, on the position, on the round or on the other
 *   requests) are unchanged.  Z is the pose of node j of seq_j in the frame of node i of seq_i and `info` its right-tangent information:
 *   what an aloam_graph_link wants.
 * aloam_graph_search_links(ctx, req, n, search, opt, dst, search_dst, scores) is the same call with the pose grid of
 *   aloam_graph_search_loops scored around every guess first; grid, score, ranking, records and limits are unchanged.
 * Checked before anything is queued, ALOAM_E_ARG with the field named in aloam_last_error and nothing changed, by the rules of the
 *   per-sequence calls with these differences: seq_i and seq_j both in range and seq_i != seq_j (for one sequence the loop calls exist);
 *   count >= 1, [first, first + count) and first <= i < first + count are held against seq_i's node count; 0 <= j < seq_j's node count;
 *   there is no "j outside the window" rule.  ALOAM_E_STATE before aloam_graph_loops_enable.  n = 0 is ALOAM_OK.  Timed under the profiling
 *   slot loop_register.  The staging of the link records (a pinned ring and a device array of max_requests records) is made by the first
 *   link call that needs it; when it cannot be had it is ALOAM_E_HIP and nothing of it stays allocated.  aloam_graph_loop_export_target
 *   returns a slot's filtered target after a link call as after a loop call.
 *
 * aloam_graph_propose_links: for every query (seq_j, j, seq_i) the nodes of seq_i near node j of seq_j, as link requests.  Every f64
 *   operation is rounded on its own.
 *   1. X_k = (q, t) or its estimate (q_opt, t_opt), chosen by pose, for both sequences.
 *   2. X_j' = X_j when frames is NULL (no arithmetic: the bits are X_j's); otherwise X_j' = A o X_j with A = frames[query] = (q_A, t_A), the
 *      pose of seq_j's frame in seq_i's frame: compose of the joined-graphs section, q_j' = quat_mul(q_A, q_j),
 *      t_j' = quat_rotate(q_A, t_j) + t_A.  q_A is stored normalised by the host, as a link's q is.
 *   3. The eligible nodes are all nodes [0, nodes(seq_i)): no minimum gap and no growth term, an index distance between two chains means
 *      nothing.
 *   4. (dx, dy, dz) = t_i - t_j'; d2 = (dx*dx + dy*dy) + dz*dz; i is a hit when d2 <= radius_m * radius_m.
 *   5. At most K rounds of the greedy rule of aloam_graph_propose_loops: the live hit with the least (d2, i) - lower d2 first, then lower i -
 *      is taken, and every hit i' with |i' - i| <= separation dies.  counts[q] is the number taken.
 *   6. Record k: seq_i, i, first = max(0, i - half_window), count = min(i + half_window, nodes(seq_i) - 1) - first + 1 (the window is
 *      clamped at BOTH ends: no minimum gap keeps it off the end of the chain), seq_j, j, pose, and the guess X_i^-1 o X_j',
 *      q_d = conj(q_i) q_j', t_d = conj(q_i) (t_j' - t_i); pad and reserved are zero; dist2[q][k] = d2.
 *   7. Rows behind counts[q] are all-zero bytes; every byte of the three outputs is written and nothing outside them is written.
 *   frames NULL is for members already joined and aligned; before that A comes from the first link,
 *   A = (X_i o Z) o X_j^-1 (align_member's transform; posegraph.frame_from_link).
 *   queries (n triples) and frames (n x 7 doubles, or NULL) are host memory, read during the call.  Checked before anything is queued,
 *   ALOAM_E_ARG with nothing changed: both sequences in range and distinct; 0 <= j < seq_j's nodes; pose 0 or 1; radius_m finite and >= 0;
 *   half_window >= 0; separation >= 0; 1 <= K <= 16; frames finite and q_A unit to 1e-6; dst and dist2 (may be NULL) 8-byte aligned and
 *   counts 4-byte aligned, device memory of the context's device or pinned host memory, classified like the exports.  ALOAM_E_STATE before
 *   aloam_graph_enable.  n = 0 is ALOAM_OK.  Stream-ordered, no host synchronisation: the queries go through a pinned staging ring made
 *   by the first call, and n > 2048 runs in rounds.  It reads the graphs and writes nothing in them; a query's bytes are independent of n,
 *   of its position in the list, of the round and of the other queries.  Timed under the profiling slot pose_graph. */
struct aloam_graph_link_request {             /* 96 bytes; the guess at byte 32, as in aloam_graph_loop_request                          */
  int seq_i, i;                               /* the frame: node i of sequence seq_i                                                    */
  int first, count;                           /* the target: nodes [first, first + count) of seq_i, i among them                        */
  int seq_j, j;                               /* the source: the clouds of node j of sequence seq_j, seq_j != seq_i                     */
  int pose;                                   /* ALOAM_GRAPH_POSE_ENTERED / _OPTIMIZED: which poses of seq_i place the target           */
  int pad;
  double q[4], t[3];                          /* the guess of Z: node j of seq_j in the frame of node i of seq_i                        */
  double reserved;
};
typedef struct aloam_graph_link_request aloam_graph_link_request;
int aloam_graph_register_links(aloam_ctx* ctx, const aloam_graph_link_request* req, int n, const aloam_graph_loop_options* opt,
                               aloam_graph_loop_result* dst /* [n] */);
int aloam_graph_search_links(aloam_ctx* ctx, const aloam_graph_link_request* req, int n, const aloam_graph_loop_search* search,
                             const aloam_graph_loop_options* opt, aloam_graph_loop_result* dst /* [n] */,
                             aloam_graph_loop_search_result* search_dst /* [n] */, aloam_map_score* scores /* [n][K] or NULL */);
int aloam_graph_propose_links(aloam_ctx* ctx, const int* queries /* [n][3]: seq_j, j, seq_i */, const double* frames /* [n][7]: q, t, or NULL */,
                              int n, int pose, double radius_m, int half_window, int separation, int K,
                              aloam_graph_link_request* dst /* [n][K] */, int* counts /* [n] */, double* dist2 /* [n][K] or NULL */);

/* ---- intermediate arrays, for parity tests ----------------------------------------------------------------- */
/* cloudCurvature / cloudLabel are kept by the aloam_scan_register* entries only; after aloam_process_device / aloam_process_host
 * (which skip those 5 bytes per point) the two getters fail with ALOAM_E_STATE. */
int aloam_get_ring_ranges(aloam_ctx* ctx, int seq, int* start, int* count);     /* scanStartInd-5 / ring sizes (src/scanRegistration.cpp:246-252) */
int aloam_get_curvature(aloam_ctx* ctx, int seq, float* out, int cap);          /* cloudCurvature (src/scanRegistration.cpp:66,262)               */
int aloam_get_labels(aloam_ctx* ctx, int seq, int* out, int cap);               /* cloudLabel (src/scanRegistration.cpp:69)                       */
/* correspondences of the last outer iteration: edges 9 floats (cp,a,b), planes 12 floats (cp,j,l,m), plus the
 * index of the query feature each belongs to (src/laserOdometry.cpp:365-381,460-479). */
int aloam_get_correspondences(aloam_ctx* ctx, int seq, float* edges, int cap_edges, int* n_edges, int* edge_query,
                              float* planes, int cap_planes, int* n_planes, int* plane_query);
/* factor records the last mapping solve of `seq` read (second iteration), in the dense order the solver visits them (tile after tile of
 * 256 stack points, stack order inside a tile): lines 9 doubles (cp, a, b), planes 7 doubles (cp, n, d) (src/laserMapping.cpp:618,683).
 * Counts of zero when the gate (:554) was false.  Synchronises. */
int aloam_get_map_factors(aloam_ctx* ctx, int seq, double* lines, int cap_lines, int* n_lines, double* planes, int cap_planes, int* n_planes);
/* The filtered target of scratch slot `slot` and class feature_class (0 corner, 1 surf) as the last aloam_graph_register_loops left it
 * (request r of a call ran in slot r % max_requests).  Stream-ordered; dst_xyzw and count are classified like the exports' destinations;
 * count is always written, the points only when they fit cap (0 with dst NULL: the size query). */
int aloam_graph_loop_export_target(aloam_ctx* ctx, int slot, int feature_class, float* dst_xyzw, long long cap, int* count);
/* The joined rows of group `group` of the last aloam_graph_optimize_joint / aloam_graph_optimize_joint_robust as that call left them: the
 * nodes with the solved estimates, the edges as gathered.  Synchronises.  nodes_dst and edges_dst are plain host memory and may be NULL;
 * counts = {nodes, edges, of these the members' edges, links} is always written, a row only when its dst is given and it fits its cap.
 * ALOAM_E_STATE before the first joint call, ALOAM_E_ARG for a group the last call did not have. */
int aloam_graph_joint_export(aloam_ctx* ctx, int group, aloam_graph_node* nodes_dst, long long cap_nodes, aloam_graph_edge* edges_dst, long long cap_edges,
                             int counts[4]);

/* How the ring ids of the clouds the last aloam_odometry_step searched (laserCloudCornerLast, laserCloudSurfLast of that step) are ordered, as
 * found when their kd-tree stand-ins were built (src/laserOdometry.cpp:567-568): 0 = int(intensity) never decreases with the index; 1 = it decreases, but never by more than 2 below an earlier
 * value (sweeps whose first ray had no return: relTime < 0 for the points before it, src/scanRegistration.cpp:211-214,239) - the reference's
 * neighbour walks (src/laserOdometry.cpp:315-361,410-455) then still visit one index range and run on the fast path; 2 = neither (literal walks);
 * -1 = ring ids / coordinates outside the range the grids are exact for (literal search). */
int aloam_get_last_cloud_order(aloam_ctx* ctx, int seq, int out[2]);

/* What the odometry solve of this context keeps in LDS across the passes of a solve: out[0] = plane factor slots per thread, out[1] = edge factor
 * slots per thread, out[2] = bytes of dynamic LDS per workgroup.  All zero in a context created with ALOAM_SOLVE_STAGE=0 in the environment (every
 * pass then reads the factor records from global memory; the results are the same bits).  No device work; ALOAM_E_STATE without the odometry stage. */
int aloam_get_solve_lds(aloam_ctx* ctx, int out[3]);

/* ---- per-kernel timing (hipEvents on the context's stream), for bench.py's roofline object ----------------- */
int aloam_profile_enable(aloam_ctx* ctx, int on);
int aloam_profile_kernel_count(void);
const char* aloam_profile_kernel_name(int kernel);
/* accumulated since the last enable: total milliseconds, launches, algorithmic bytes moved */
int aloam_profile_get(aloam_ctx* ctx, int kernel, double* total_ms, long long* launches, double* algorithmic_bytes);

#ifdef __cplusplus
}
#endif
#endif
