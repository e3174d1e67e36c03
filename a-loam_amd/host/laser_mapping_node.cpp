// a-loam_amd/host/laser_mapping_node.cpp — the `alaserMapping` node on top of libaloam_mi355x.so.
// Same subscriptions, queue alignment, publications, frame ids and tf as the reference (src/laserMapping.cpp:175-304,
// 803-938); the body of process() between the queue handling and the publishers (:307-802) is calls into the C ABI.  The
// frames are processed in the spin loop instead of a second thread: with the work on the GPU the node is never behind, so
// the reference's "drop queued frames" branch (:299-303) is kept but does not fire in practice.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <mutex>
#include <queue>
#include <string>
#include <vector>
#include <cmath>
// Pinned memory for the record of `save_map`: the HIP runtime API (a build that finds its headers links libamdhip64, e.g. CMake's
// hip::host; hipcc and hip::host define the platform, a plain compiler gets it here).
#if __has_include(<hip/hip_runtime_api.h>)
#if !defined(__HIP_PLATFORM_AMD__) && !defined(__HIP_PLATFORM_NVIDIA__)
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>
#define ALOAM_NODE_HAVE_HIP 1
#endif

#include <geometry_msgs/PoseStamped.h>
#include <nav_msgs/Odometry.h>
#include <nav_msgs/Path.h>
#include <tf/transform_broadcaster.h>
#include <tf/transform_datatypes.h>

#include "aloam_ros_common.hpp"

namespace {
aloam_ctx* g_ctx = nullptr;
std::queue<sensor_msgs::PointCloud2ConstPtr> cornerLastBuf, surfLastBuf, fullResBuf;
std::queue<nav_msgs::Odometry::ConstPtr> odometryBuf;
std::mutex mBuf;
ros::Publisher pubLaserCloudSurround, pubLaserCloudMap, pubLaserCloudFullRes, pubOdomAftMapped, pubOdomAftMappedHighFrec, pubLaserAfterMappedPath;
nav_msgs::Path laserAfterMappedPath;
double q_wmap_wodom[4] = {0, 0, 0, 1}, t_wmap_wodom[3] = {0, 0, 0};
int frameCount = 0;

void quat_mul(const double a[4], const double b[4], double o[4]) {
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
void quat_rot(const double q[4], const double v[3], double o[3]) {
  double ux = q[1] * v[2] - q[2] * v[1], uy = q[2] * v[0] - q[0] * v[2], uz = q[0] * v[1] - q[1] * v[0];
  ux += ux; uy += uy; uz += uz;
  o[0] = v[0] + q[3] * ux + (q[1] * uz - q[2] * uy);
  o[1] = v[1] + q[3] * uy + (q[2] * ux - q[0] * uz);
  o[2] = v[2] + q[3] * uz + (q[0] * uy - q[1] * ux);
}
nav_msgs::Odometry make_odom(const double q[4], const double t[3], const ros::Time& stamp) {
  nav_msgs::Odometry o;
  o.header.frame_id = "/camera_init";
  o.child_frame_id = "/aft_mapped";
  o.header.stamp = stamp;
  o.pose.pose.orientation.x = q[0]; o.pose.pose.orientation.y = q[1]; o.pose.pose.orientation.z = q[2]; o.pose.pose.orientation.w = q[3];
  o.pose.pose.position.x = t[0]; o.pose.pose.position.y = t[1]; o.pose.pose.position.z = t[2];
  return o;
}
sensor_msgs::PointCloud2 map_cloud_msg(int which, const ros::Time& stamp) {   // /laser_cloud_surround (:806-812), /laser_cloud_map (:823-829)
  std::vector<float> all(4);
  const int n = aloam_get_map_cloud(g_ctx, 0, which, nullptr, 0);
  if (n > 0) {
    all.resize(4 * static_cast<size_t>(n));
    aloam_get_map_cloud(g_ctx, 0, which, all.data(), n);
  }
  return aloam_host::xyzi_to_msg(all.data(), n > 0 ? n : 0, stamp, "/camera_init");
}
}  // namespace
aloam_ctx* aloam_node_context() { return g_ctx; }

void laserCloudCornerLastHandler(const sensor_msgs::PointCloud2ConstPtr& m) { mBuf.lock(); cornerLastBuf.push(m); mBuf.unlock(); }
void laserCloudSurfLastHandler(const sensor_msgs::PointCloud2ConstPtr& m) { mBuf.lock(); surfLastBuf.push(m); mBuf.unlock(); }
void laserCloudFullResHandler(const sensor_msgs::PointCloud2ConstPtr& m) { mBuf.lock(); fullResBuf.push(m); mBuf.unlock(); }
void laserOdometryHandler(const nav_msgs::Odometry::ConstPtr& laserOdometry) {   // :197-228: queue + high-frequency corrected pose
  mBuf.lock();
  odometryBuf.push(laserOdometry);
  mBuf.unlock();
  const double qo[4] = {laserOdometry->pose.pose.orientation.x, laserOdometry->pose.pose.orientation.y, laserOdometry->pose.pose.orientation.z,
                        laserOdometry->pose.pose.orientation.w};
  const double to[3] = {laserOdometry->pose.pose.position.x, laserOdometry->pose.pose.position.y, laserOdometry->pose.pose.position.z};
  double q[4], t[3];
  quat_mul(q_wmap_wodom, qo, q);
  quat_rot(q_wmap_wodom, to, t);
  for (int k = 0; k < 3; ++k) t[k] += t_wmap_wodom[k];
  pubOdomAftMappedHighFrec.publish(make_odom(q, t, laserOdometry->header.stamp));
}

static void process() {
  std::vector<float> corner, surf, full;
  while (!cornerLastBuf.empty() && !surfLastBuf.empty() && !fullResBuf.empty() && !odometryBuf.empty()) {
    mBuf.lock();
    while (!odometryBuf.empty() && odometryBuf.front()->header.stamp.toSec() < cornerLastBuf.front()->header.stamp.toSec()) odometryBuf.pop();
    if (odometryBuf.empty()) { mBuf.unlock(); break; }
    while (!surfLastBuf.empty() && surfLastBuf.front()->header.stamp.toSec() < cornerLastBuf.front()->header.stamp.toSec()) surfLastBuf.pop();
    if (surfLastBuf.empty()) { mBuf.unlock(); break; }
    while (!fullResBuf.empty() && fullResBuf.front()->header.stamp.toSec() < cornerLastBuf.front()->header.stamp.toSec()) fullResBuf.pop();
    if (fullResBuf.empty()) { mBuf.unlock(); break; }
    const double tCorner = cornerLastBuf.front()->header.stamp.toSec(), tSurf = surfLastBuf.front()->header.stamp.toSec();
    const double tFull = fullResBuf.front()->header.stamp.toSec(), tOdom = odometryBuf.front()->header.stamp.toSec();
    if (tCorner != tOdom || tSurf != tOdom || tFull != tOdom) {
      printf("time corner %f surf %f full %f odom %f \n", tCorner, tSurf, tFull, tOdom);
      printf("unsync messeage!");
      mBuf.unlock();
      break;
    }
    const int nCorner = aloam_host::msg_to_xyzi(*cornerLastBuf.front(), &corner); cornerLastBuf.pop();
    const int nSurf = aloam_host::msg_to_xyzi(*surfLastBuf.front(), &surf); surfLastBuf.pop();
    const int nFull = aloam_host::msg_to_xyzi(*fullResBuf.front(), &full); fullResBuf.pop();
    const nav_msgs::Odometry::ConstPtr od = odometryBuf.front();
    odometryBuf.pop();
    while (!cornerLastBuf.empty()) { cornerLastBuf.pop(); printf("drop lidar frame in mapping for real time performance \n"); }   // :299-303
    mBuf.unlock();

    const double qo[4] = {od->pose.pose.orientation.x, od->pose.pose.orientation.y, od->pose.pose.orientation.z, od->pose.pose.orientation.w};
    const double to[3] = {od->pose.pose.position.x, od->pose.pose.position.y, od->pose.pose.position.z};
    const double id_q[4] = {0, 0, 0, 1}, id_t[3] = {0, 0, 0};
    if (aloam_set_last(g_ctx, 0, corner.data(), nCorner, surf.data(), nSurf) != ALOAM_OK || aloam_set_full_cloud(g_ctx, 0, full.data(), nFull) != ALOAM_OK ||
        aloam_set_state(g_ctx, 0, id_q, id_t, qo, to) != ALOAM_OK || aloam_mapping_step(g_ctx) != ALOAM_OK) {
      ROS_WARN("mapping step failed: %s", aloam_last_error(g_ctx));
      continue;
    }
    const int rc_sync = aloam_synchronize(g_ctx);
    if (rc_sync == ALOAM_E_CAPACITY) ROS_WARN("mapping: %s", aloam_last_error(g_ctx));   // the step has run; only points that did not fit are missing from the map
    else if (rc_sync != ALOAM_OK) { ROS_WARN("mapping step failed: %s", aloam_last_error(g_ctx)); continue; }
    {
      int info[16];
      if (aloam_get_map_info(g_ctx, 0, info) == ALOAM_OK && !(info[4] > 10 && info[5] > 50)) ROS_WARN("time Map corner and surf num are not enough");   // :554,730-733
    }
    double q_w[4], t_w[3];
    aloam_get_map_pose(g_ctx, 0, q_w, t_w, q_wmap_wodom, t_wmap_wodom);
    const ros::Time stamp = ros::Time().fromSec(tOdom);

    // :803-834: the window of this step (laserCloudSurroundInd, :512-529) and the whole map, assembled on the device
    if (frameCount % 5 == 0) pubLaserCloudSurround.publish(map_cloud_msg(ALOAM_MAP_SURROUND, stamp));
    if (frameCount % 20 == 0) pubLaserCloudMap.publish(map_cloud_msg(ALOAM_MAP_FULL, stamp));
    {  // /velodyne_cloud_registered (:836-846)
      std::vector<float> reg(4 * static_cast<size_t>(nFull > 0 ? nFull : 1));
      const int n = aloam_get_map_cloud(g_ctx, 0, ALOAM_MAP_REGISTERED, reg.data(), nFull);
      pubLaserCloudFullRes.publish(aloam_host::xyzi_to_msg(reg.data(), n, stamp, "/camera_init"));
    }
    const nav_msgs::Odometry odomAftMapped = make_odom(q_w, t_w, stamp);                  // :851-863
    pubOdomAftMapped.publish(odomAftMapped);
    geometry_msgs::PoseStamped pose;                                                      // :865-871
    pose.header = odomAftMapped.header;
    pose.pose = odomAftMapped.pose.pose;
    laserAfterMappedPath.header.stamp = odomAftMapped.header.stamp;
    laserAfterMappedPath.header.frame_id = "/camera_init";
    laserAfterMappedPath.poses.push_back(pose);
    pubLaserAfterMappedPath.publish(laserAfterMappedPath);
    static tf::TransformBroadcaster br;                                                   // :873-887
    tf::Transform transform;
    tf::Quaternion q;
    transform.setOrigin(tf::Vector3(t_w[0], t_w[1], t_w[2]));
    q.setW(q_w[3]); q.setX(q_w[0]); q.setY(q_w[1]); q.setZ(q_w[2]);
    transform.setRotation(q);
    br.sendTransform(tf::StampedTransform(transform, odomAftMapped.header.stamp, "/camera_init", "/aft_mapped"));
    frameCount++;
  }
}

// String parameters through NodeHandle::getParam where the ROS API has it (roscpp); a stand-in without string parameters leaves them unset.
template <class NH> auto string_param(const NH& nh, const std::string& name, std::string& out, int) -> decltype(nh.getParam(name, out)) {
  return nh.getParam(name, out);
}
template <class NH> bool string_param(const NH&, const std::string&, std::string&, long) { return false; }

// `prior_map`: a sequence record (aloam_save_sequences of a mapping-only context: the map part only) loaded into slot 0.  The record carries
// the first session's map <- odom correction and frame count; a new drive starts its odometry afresh, so the correction becomes the drive's
// start pose in the map (`initial_pose`: x, y, z, yaw; default the map origin) and the frame count 0.  The window centre stays the record's.
bool load_record(const std::string& path, const double initial_pose[4]) {
  std::ifstream f(path, std::ios::binary);
  std::vector<char> rec((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const int slot = 0;
  const long long off[2] = {0, static_cast<long long>(rec.size())};
  if (!f.good() && !f.eof()) { ROS_ERROR("prior_map %s: cannot read", path.c_str()); return false; }
  if (aloam_load_sequences(g_ctx, &slot, 1, rec.data(), off) != ALOAM_OK || aloam_synchronize(g_ctx) != ALOAM_OK) {   // pageable memory: staged by the call
    ROS_ERROR("prior_map %s: %s", path.c_str(), aloam_last_error(g_ctx));
    return false;
  }
  int info[16];
  const double q[4] = {0.0, 0.0, std::sin(initial_pose[3] / 2), std::cos(initial_pose[3] / 2)};
  if (aloam_get_map_info(g_ctx, 0, info) != ALOAM_OK || aloam_set_map_frame(g_ctx, 0, info, q, initial_pose, 0) != ALOAM_OK) {   // info[0..2]: cen
    ROS_ERROR("prior_map %s: %s", path.c_str(), aloam_last_error(g_ctx));
    return false;
  }
  return true;
}

// `save_map`: the record of slot 0 written to a file on shutdown (pinned memory: the device writes offsets and record).
void save_record(const std::string& path) {
#ifdef ALOAM_NODE_HAVE_HIP
  const int seq = 0;
  long long* off = nullptr;
  void* rec = nullptr;
  bool ok = hipHostMalloc(reinterpret_cast<void**>(&off), 2 * sizeof(long long), 0) == hipSuccess &&
            aloam_save_sequences(g_ctx, &seq, 1, nullptr, 0, off) == ALOAM_OK && aloam_synchronize(g_ctx) == ALOAM_OK &&   // size query
            hipHostMalloc(&rec, static_cast<size_t>(off[1]), 0) == hipSuccess &&
            aloam_save_sequences(g_ctx, &seq, 1, rec, off[1], off) == ALOAM_OK && aloam_synchronize(g_ctx) == ALOAM_OK;
  if (ok) {
    std::ofstream f(path, std::ios::binary);
    f.write(static_cast<const char*>(rec), off[1]);
    ok = f.good();
  }
  if (!ok) ROS_ERROR("save_map %s failed: %s", path.c_str(), aloam_last_error(g_ctx));
  if (rec) (void)hipHostFree(rec);
  if (off) (void)hipHostFree(off);
#else
  ROS_ERROR("save_map %s: this build of the node has no HIP runtime headers (pinned memory for the record)", path.c_str());
#endif
}

int main(int argc, char** argv) {
  ros::init(argc, argv, "laserMapping");
  ros::NodeHandle nh;
  float lineRes = 0, planeRes = 0;
  nh.param<float>("mapping_line_resolution", lineRes, 0.4);
  nh.param<float>("mapping_plane_resolution", planeRes, 0.8);
  int n_scans = 64, pool_points = 1 << 17;
  nh.param<int>("scan_line", n_scans, 64);
  nh.param<int>("map_pool_points", pool_points, 1 << 17);  // where the device-resident map starts (points per feature class); it doubles as the map grows, like the reference's std::vector cubes
  printf("line resolution %f plane resolution %f \n", lineRes, planeRes);

  aloam_config cfg;
  aloam_default_config(&cfg);
  cfg.n_scans = n_scans;
  cfg.batch = 1;
  cfg.max_points = 400000;
  if (aloam_create_stages(&cfg, ALOAM_STAGE_MAPPING, &g_ctx) != ALOAM_OK || aloam_mapping_enable(g_ctx, lineRes, planeRes, pool_points) != ALOAM_OK) {   // this node hosts stage 3 only
    ROS_ERROR("aloam set-up: %s", g_ctx ? aloam_last_error(g_ctx) : "out of memory");
    return 1;
  }
  int reference_sum_order = 0;                             // 1: pcl::VoxelGrid's own summation order in the stack / cube filters (validation: ~80 ms per HDL-64 frame)
  nh.param<int>("reference_sum_order", reference_sum_order, 0);
  if (reference_sum_order) aloam_set_voxel_sum_order(g_ctx, ALOAM_SUM_REFERENCE_ORDER);
  // Localization against a prior map: `prior_map` = a record written by `save_map` of an earlier run, `localization_only` = 1 freezes the
  // sequence (aloam_set_map_frozen): every frame is localized in the map, which stays as loaded.
  std::string prior_map, save_map;
  string_param(nh, "prior_map", prior_map, 0);
  string_param(nh, "save_map", save_map, 0);
  int localization_only = 0;
  nh.param<int>("localization_only", localization_only, 0);
  double initial_pose[4] = {0.0, 0.0, 0.0, 0.0};          // with prior_map: where this drive starts in the map (metres, yaw in radians)
  nh.param<double>("initial_pose_x", initial_pose[0], 0.0);
  nh.param<double>("initial_pose_y", initial_pose[1], 0.0);
  nh.param<double>("initial_pose_z", initial_pose[2], 0.0);
  nh.param<double>("initial_pose_yaw", initial_pose[3], 0.0);
  if (!prior_map.empty() && !load_record(prior_map, initial_pose)) return 1;
  if (localization_only) {
    const int frozen = 1;
    if (aloam_set_map_frozen(g_ctx, &frozen) != ALOAM_OK) { ROS_ERROR("localization_only: %s", aloam_last_error(g_ctx)); return 1; }
  }
  ros::Subscriber subLaserCloudCornerLast = nh.subscribe<sensor_msgs::PointCloud2>("/laser_cloud_corner_last", 100, laserCloudCornerLastHandler);
  ros::Subscriber subLaserCloudSurfLast = nh.subscribe<sensor_msgs::PointCloud2>("/laser_cloud_surf_last", 100, laserCloudSurfLastHandler);
  ros::Subscriber subLaserOdometry = nh.subscribe<nav_msgs::Odometry>("/laser_odom_to_init", 100, laserOdometryHandler);
  ros::Subscriber subLaserCloudFullRes = nh.subscribe<sensor_msgs::PointCloud2>("/velodyne_cloud_3", 100, laserCloudFullResHandler);
  pubLaserCloudSurround = nh.advertise<sensor_msgs::PointCloud2>("/laser_cloud_surround", 100);
  pubLaserCloudMap = nh.advertise<sensor_msgs::PointCloud2>("/laser_cloud_map", 100);
  pubLaserCloudFullRes = nh.advertise<sensor_msgs::PointCloud2>("/velodyne_cloud_registered", 100);
  pubOdomAftMapped = nh.advertise<nav_msgs::Odometry>("/aft_mapped_to_init", 100);
  pubOdomAftMappedHighFrec = nh.advertise<nav_msgs::Odometry>("/aft_mapped_to_init_high_frec", 100);
  pubLaserAfterMappedPath = nh.advertise<nav_msgs::Path>("/aft_mapped_path", 100);

  ros::Rate rate(500);                                     // the reference's worker polls every 2 ms (:890-891)
  while (ros::ok()) {
    ros::spinOnce();
    process();
    rate.sleep();
  }
  if (!save_map.empty()) save_record(save_map);
  aloam_destroy(g_ctx);
  g_ctx = nullptr;
  return 0;
}
